#!/usr/bin/env python3
"""Cost of classifier-free guidance in the NAR stage: NAR.forward over the seven levels, end to end, with guidance off and on
(w = 1.5, the default null twins), at 1 and at 32 utterances x 750 frames in bf16 on the registry-size `nar` model (d = 1024, 16 heads,
12 layers; synthetic weights).  The two arms are interleaved on one box: PAIRS times (off, on), each call synchronised and timed on its
own after one warm-up of both; the medians are reported, with no threshold.  A guided level is one evaluation of twice the
utterances on a grid padded to the longest of them, so about twice the option-free time is what to expect.  The off arm passes
guidance=0.0, which is the path of a call without the keyword: its ids are compared with such a call (they must be identical).

    python tools/nar_guidance_latency.py [--out profiles/round27_nar_guidance.json] [--pairs 6] [--batches 1,32]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tts-with-diffusion-model_amd"))
sys.path.insert(0, ROOT)

FRAMES, LEVELS, WEIGHT = 750, 7, 1.5


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(model, batch, pairs):
    import torch
    from vall_e.vall_e import synth
    texts, proms, resps = synth.make_nar_inputs(batch, 1, t_text=(20, 50), t_prom=(100, 225), t_resp=(FRAMES, FRAMES + 1))
    texts, proms, resps = ([t.to(model.device) for t in lst] for lst in (texts, proms, resps))
    bare = model(texts, proms, resps, seed=7)
    off = lambda: model(texts, proms, resps, seed=7, guidance=0.0)
    on = lambda: model(texts, proms, resps, seed=7, guidance=WEIGHT)
    ids_off, ids_on = off(), on()          # warm-up: workspaces, lazy kernel loads
    same = all(bool(torch.equal(a, b)) for a, b in zip(bare, ids_off))
    assert same, "the guidance-free arm must draw what a call without the keyword draws"
    t_off, t_on = [], []
    for _ in range(pairs):
        t_off.append(timed(off))
        t_on.append(timed(on))
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    return dict(batch=batch, frames=FRAMES, levels=LEVELS, pairs=pairs, off_ms=t_off, on_ms=t_on, off_median_ms=m_off, on_median_ms=m_on,
                on_over_off=m_on / m_off, added_ms=m_on - m_off, off_ids_equal_call_without_keyword=same,
                ids_changed_by_guidance=float(torch.cat([(a[:, 1:] != b[:, 1:]).float().mean()[None] for a, b in zip(ids_off, ids_on)]).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round27_nar_guidance.json"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--batches", default="1,32")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from bench import build_id
    from vall_e.vall_e import NAR, synth
    cfg = synth.NARConfig()                          # the registry's `nar`: 1024 / 16 / 12
    model = NAR(cfg.n_tokens, cfg.d_model, cfg.n_heads, cfg.n_layers)
    model.load_state_dict(synth.make_nar_state_dict(cfg, 0))
    model = model.to(torch.bfloat16).to("cuda:0")
    result = dict(build_id=build_id(), device=torch.cuda.get_device_name(0), dtype="bf16", config="nar (d 1024, 16 heads, 12 layers)",
                  on_arm=f"guidance={WEIGHT}, default null twins", rows=[])
    for batch in (int(b) for b in args.batches.split(",")):
        row = measure(model, batch, args.pairs)
        print(f"[nar_guidance_latency] batch {batch:3d}: off {row['off_median_ms']:.2f} ms, on {row['on_median_ms']:.2f} ms "
              f"(x {row['on_over_off']:.3f}), off arm = call without the keyword: {row['off_ids_equal_call_without_keyword']}, "
              f"ids of levels 1..7 changed: {row['ids_changed_by_guidance']:.3f}", flush=True)
        result["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"[nar_guidance_latency] wrote {args.out}")


if __name__ == "__main__":
    main()

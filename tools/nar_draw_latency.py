#!/usr/bin/env python3
"""Cost of the NAR stage's draw options: NAR.forward over the seven levels, end to end, without options and with
top_k=50, top_p=0.9, return_logprobs=True, at 1 and at 32 utterances x 750 frames in bf16 on the registry-size `nar` model (d = 1024,
16 heads, 12 layers; synthetic weights).  The two arms are interleaved on one box: PAIRS times (off, on), each call synchronised and
timed on its own after one warm-up of both; the medians are reported, with no threshold.  The off arm passes every option at its
default, which is the path of a call without keywords: its ids are compared with such a call (they must be identical).

    python tools/nar_draw_latency.py [--out profiles/round26_nar_draw.json] [--pairs 6] [--batches 1,32]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tts-with-diffusion-model_amd"))
sys.path.insert(0, ROOT)

FRAMES, LEVELS = 750, 7


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
    off = lambda: model(texts, proms, resps, seed=7, top_k=0, top_p=1.0, known=None, known_mask=None, return_logprobs=False)
    on = lambda: model(texts, proms, resps, seed=7, top_k=50, top_p=0.9, return_logprobs=True)
    ids_off, (ids_on, scores) = off(), on()          # warm-up: workspaces, lazy kernel loads
    same = all(bool(torch.equal(a, b)) for a, b in zip(bare, ids_off))
    assert same, "the option-free arm must draw what a call without keywords draws"
    t_off, t_on = [], []
    for _ in range(pairs):
        t_off.append(timed(off))
        t_on.append(timed(on))
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    lp = torch.cat(scores)
    return dict(batch=batch, frames=FRAMES, levels=LEVELS, pairs=pairs, off_ms=t_off, on_ms=t_on, off_median_ms=m_off, on_median_ms=m_on,
                added_ms=m_on - m_off, added_percent=100.0 * (m_on / m_off - 1.0), added_us_per_level=(m_on - m_off) * 1e3 / LEVELS,
                off_ids_equal_call_without_keywords=same, ids_changed_by_the_cuts=float(torch.cat([(a != b).float().mean()[None] for a, b in zip(ids_off, ids_on)]).mean()),
                logprob_finite=bool(torch.isfinite(lp).all()), mean_logprob=float(lp.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round26_nar_draw.json"))
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
                  on_arm="top_k=50, top_p=0.9, return_logprobs=True", rows=[])
    for batch in (int(b) for b in args.batches.split(",")):
        row = measure(model, batch, args.pairs)
        print(f"[nar_draw_latency] batch {batch:3d}: off {row['off_median_ms']:.2f} ms, on {row['on_median_ms']:.2f} ms "
              f"({row['added_percent']:+.2f} %, {row['added_us_per_level']:+.1f} us per level), off arm = call without keywords: "
              f"{row['off_ids_equal_call_without_keywords']}", flush=True)
        result["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"[nar_draw_latency] wrote {args.out}")


if __name__ == "__main__":
    main()

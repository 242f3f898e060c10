#!/usr/bin/env python3
"""Cost of AR.generate_audio(return_logprobs=True): the same call with the keyword off and on, end to end, at 1 and at 32 utterances
x 750 frames in bf16 (the libritts configuration of bench.py), for the D3PM loop and for reveal_steps = 16.  The two arms are
interleaved on one box: PAIRS times (off, on), each call synchronised and timed on its own after one warm-up of both; the medians
are reported, with no threshold.  The ids of the two arms are compared as well (they must be identical).

    python tools/logprob_latency.py [--out profiles/round22_logprob.json] [--pairs 6] [--batches 1,32]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tts-with-diffusion-model_amd"))
sys.path.insert(0, ROOT)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(model, cfg, batch, reveal_steps, pairs):
    import torch
    from vall_e.vall_e import synth
    texts, proms = synth.make_inputs(cfg, batch, 1)
    kw = dict(seed=7) if reveal_steps is None else dict(seed=7, reveal_steps=reveal_steps)
    off = lambda: model.generate_audio(texts, proms, **kw)
    on = lambda: model.generate_audio(texts, proms, return_logprobs=True, **kw)
    ids, (ids_on, scores) = off(), on()              # warm-up: workspaces, lazy kernel loads
    same = bool(torch.equal(ids, ids_on))
    scored = int((scores.step >= 1).sum())
    t_off, t_on = [], []
    for _ in range(pairs):
        t_off.append(timed(off))
        t_on.append(timed(on))
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    evaluations = cfg.timesteps - 1 if reveal_steps is None else reveal_steps
    return dict(batch=batch, frames=cfg.n_frames, loop="d3pm" if reveal_steps is None else f"reveal_steps={reveal_steps}", pairs=pairs,
                off_ms=t_off, on_ms=t_on, off_median_ms=m_off, on_median_ms=m_on, added_ms=m_on - m_off, added_percent=100.0 * (m_on / m_off - 1.0),
                added_us_per_evaluation=(m_on - m_off) * 1e3 / evaluations, evaluations=evaluations, ids_identical=same, scored_frames=scored,
                mean_logprob=float(scores.logprob[scores.step >= 1].mean()) if scored else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round22_logprob.json"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--reveal-steps", type=int, default=16)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from bench import build_id
    from vall_e.vall_e import AR, synth
    cfg = synth.D3PMConfig.libritts()
    model = AR.from_config(cfg)
    model.load_state_dict(synth.make_state_dict(cfg, 0))
    model = model.to(torch.bfloat16).to("cuda:0")
    result = dict(build_id=build_id(), device=torch.cuda.get_device_name(0), dtype="bf16", config="libritts", rows=[])
    for batch in (int(b) for b in args.batches.split(",")):
        for n in (None, args.reveal_steps):
            row = measure(model, cfg, batch, n, args.pairs)
            print(f"[logprob_latency] batch {batch:3d} {row['loop']:>16s}: off {row['off_median_ms']:.2f} ms, on {row['on_median_ms']:.2f} ms "
                  f"({row['added_percent']:+.2f} %, {row['added_us_per_evaluation']:+.1f} us per evaluation), ids identical: {row['ids_identical']}",
                  flush=True)
            result["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"[logprob_latency] wrote {args.out}")


if __name__ == "__main__":
    main()

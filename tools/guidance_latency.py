#!/usr/bin/env python3
"""Time of AR.generate_audio(guidance=w) against the unguided call of the same build, in bf16 at 750 frames (the libritts
configuration of bench.py), the whole reverse process (condition encoders + 99 evaluations), for B = 1 and B = 16 utterances:
  unguided_B    the call without guidance at B utterances;
  guided_B      guidance = 1.5 at B utterances: every evaluation runs 2B utterances (each one and its null twin), the sampler launch
                draws B x 750 rows from twice the logits;
  unguided_2B   the call without guidance at 2B utterances: the same evaluations, a sampler over twice the rows reading the same bytes.
The expectation to CHECK, not a threshold: guided_B costs what unguided_2B costs.  The three arms are interleaved on one box, PAIRS
rounds of (unguided_B, guided_B, unguided_2B), each call synchronised and timed on its own after one warm-up of all three; medians are
reported with the spread of each arm.  Optionally (--parent-tree) the default bench.py path of this build is run against a built
checkout of the parent commit, interleaved, with --dump-outputs: the ids must be byte-identical.

    python tools/guidance_latency.py [--out profiles/round11_guidance.json] [--pairs 6] [--parent-tree DIR]

Reports time only; it makes no statement about audio quality (the weights are synthetic and were not trained with dropped conditions)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tts-with-diffusion-model_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from reveal_latency import bench_against_parent, timed  # noqa: E402


def measure(model, cfg, batch, pairs, weight):
    from vall_e.vall_e import synth
    texts, proms = synth.make_inputs(cfg, 2 * batch, 1)
    arms = dict(unguided_B=lambda: model.generate_audio(texts[:batch], proms[:batch], seed=7),
                guided_B=lambda: model.generate_audio(texts[:batch], proms[:batch], seed=7, guidance=weight),
                unguided_2B=lambda: model.generate_audio(texts, proms, seed=7))
    for fn in arms.values():                        # warm-up: workspaces, lazy kernel loads
        fn()
    times = {k: [] for k in arms}
    for _ in range(pairs):
        for k, fn in arms.items():
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    row = dict(batch=batch, frames=cfg.n_frames, evaluations=cfg.timesteps - 1, guidance=weight, pairs=pairs)
    for k in arms:
        row[k + "_ms"] = times[k]
        row[k + "_median_ms"] = med[k]
        row[k + "_spread_ms"] = max(times[k]) - min(times[k])
    row["guided_over_unguided_B"] = med["guided_B"] / med["unguided_B"]
    row["guided_over_unguided_2B"] = med["guided_B"] / med["unguided_2B"]
    row["guided_tokens_per_s"] = batch * cfg.n_frames / med["guided_B"] * 1e3
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round11_guidance.json"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--weight", type=float, default=1.5)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: also run bench.py's default path against it")
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
        row = measure(model, cfg, batch, args.pairs, args.weight)
        print(f"[guidance_latency] batch {batch:3d}: unguided B {row['unguided_B_median_ms']:.1f} ms, guided B {row['guided_B_median_ms']:.1f} ms, "
              f"unguided 2B {row['unguided_2B_median_ms']:.1f} ms (guided / unguided 2B {row['guided_over_unguided_2B']:.3f})", flush=True)
        result["rows"].append(row)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    write()
    if args.parent_tree:
        result["bench_default_path_vs_parent"] = bench_against_parent(args.parent_tree)
        print("[guidance_latency] bench.py default path vs parent:", json.dumps(result["bench_default_path_vs_parent"]), flush=True)
    write()
    print(f"[guidance_latency] wrote {args.out}")


if __name__ == "__main__":
    main()

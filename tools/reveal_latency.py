#!/usr/bin/env python3
"""Time of AR.generate_audio under the confidence-ordered reveal schedule (reveal_steps = 8, 16, 32) against the default D3PM loop of
the same build, at 1 and at 32 utterances x 750 frames in bf16 (the libritts configuration of bench.py).  Every reveal arm is
interleaved with the default arm on one box: PAIRS times (default, reveal), each call synchronised and timed on its own after one
warm-up of both; the medians are reported.  Optionally (--parent-tree) the default bench.py path of this build is run against a built
checkout of the parent commit, interleaved, with --dump-outputs: the ids must be byte-identical.

    python tools/reveal_latency.py [--out profiles/round9_reveal_latency.json] [--pairs 4] [--parent-tree DIR]

Reports time only; it makes no statement about audio quality (the weights are synthetic)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
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
    from vall_e.vall_e import synth
    texts, proms = synth.make_inputs(cfg, batch, 1)
    base = lambda: model.generate_audio(texts, proms, seed=7)
    arm = lambda: model.generate_audio(texts, proms, seed=7, reveal_steps=reveal_steps)
    base(); arm()                                   # warm-up: workspaces, lazy kernel loads
    tb, ta = [], []
    for _ in range(pairs):
        tb.append(timed(base))
        ta.append(timed(arm))
    n_tok = batch * cfg.n_frames
    mb, ma = statistics.median(tb), statistics.median(ta)
    return dict(batch=batch, frames=cfg.n_frames, reveal_steps=reveal_steps, pairs=pairs, default_ms=tb, reveal_ms=ta,
                default_median_ms=mb, reveal_median_ms=ma, speedup=mb / ma, default_evaluations=cfg.timesteps - 1,
                default_tokens_per_s=n_tok / mb * 1e3, reveal_tokens_per_s=n_tok / ma * 1e3)


def bench_against_parent(parent_tree, steps=2):
    """bench.py's default path in this tree and in a built checkout of the parent commit: tokens/s of both, interleaved, and whether
    the dumped ids are identical."""
    out = {}
    parent_tree = os.path.abspath(parent_tree)
    with tempfile.TemporaryDirectory() as tmp:
        for name, tree in (("parent", parent_tree), ("this", ROOT), ("parent_again", parent_tree), ("this_again", ROOT)):
            env = {k: v for k, v in os.environ.items() if k != "D3PM_HIP_LIB"}
            d = os.path.join(tmp, name)
            r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--cpu-steps", "0",
                                "--no-latency", "--no-nar", "--no-nq8", "--no-fp8", "--no-vctk", "--no-kernel-events", "--dump-outputs", d],
                               env=env, cwd=tree, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py ({name}) failed:\n{r.stderr[-2000:]}")
            res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            out[name] = dict(value=res.get("value"), unit=res.get("unit"), metric=res.get("metric"),
                             ids=open(os.path.join(d, "ids.npy"), "rb").read())
    same = out["parent"]["ids"] == out["this"]["ids"] == out["parent_again"]["ids"] == out["this_again"]["ids"]
    for v in out.values():
        del v["ids"]
    out["ids_byte_identical"] = same
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round9_reveal_latency.json"))
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--reveal-steps", default="8,16,32")
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
        for n in (int(v) for v in args.reveal_steps.split(",")):
            row = measure(model, cfg, batch, n, args.pairs)
            print(f"[reveal_latency] batch {batch:3d} reveal_steps {n:3d}: default {row['default_median_ms']:.1f} ms, reveal "
                  f"{row['reveal_median_ms']:.1f} ms ({row['speedup']:.2f}x)", flush=True)
            result["rows"].append(row)
    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    write()
    if args.parent_tree:
        result["bench_default_path_vs_parent"] = bench_against_parent(args.parent_tree)
        print("[reveal_latency] bench.py default path vs parent:", json.dumps(result["bench_default_path_vs_parent"]), flush=True)
    write()
    print(f"[reveal_latency] wrote {args.out}")


if __name__ == "__main__":
    main()

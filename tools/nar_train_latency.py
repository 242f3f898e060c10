#!/usr/bin/env python3
"""Time of one NAR training step, NAR.forward_backward, at the `nar-quarter` shape (d_model 256, 4 heads, 12 layers), fp32, four
ragged utterances of synth.make_nar_inputs(4, 1, t_text=(20, 50), t_prom=(100, 225), t_resp=(300, 750), n_levels=8) with synthetic
weights, levels drawn from the seed, dropout off and on (p = 0.1).  The arms are interleaved on one box: STEPS times (off, on), each
call synchronised and timed on its own after one warm-up of both; the medians of STEPS are reported.  The measurement runs in a
child process under `timeout`, so a GPU step that hangs ends there and nothing is started after it.

    python tools/nar_train_latency.py [--out profiles/round24_nar_train.json] [--steps 6] [--limit 600]

A number, no threshold: nothing in the suite depends on it.  The step runs the generic fp32 kernels of the training side, whose
attention backward pass recomputes the probabilities per query and per key.  Reports time only; it makes no statement about audio
quality (the weights are synthetic)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tts-with-diffusion-model_amd"))
sys.path.insert(0, ROOT)

SHAPE = dict(d_model=256, n_heads=4, n_layers=12)
LENGTHS = dict(t_text=(20, 50), t_prom=(100, 225), t_resp=(300, 750))
BATCH, SEED = 4, 7


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(steps):
    import torch
    from vall_e.vall_e import NAR, synth
    from vall_e.vall_e.nar_train import NARTrainer
    cfg = synth.NARConfig(**SHAPE)
    model = NAR(cfg.n_tokens, cfg.d_model, cfg.n_heads, cfg.n_layers)
    model.load_state_dict(synth.make_nar_state_dict(cfg, 0))
    model = model.float().to("cuda:0")
    texts, proms, resps = synth.make_nar_inputs(BATCH, 1, n_levels=8, **LENGTHS)
    trainer = NARTrainer(model)
    seen = {}

    def step(dropout):
        for p in model.parameters():
            p.grad = None
        loss, levels = trainer.step(texts, proms, resps, seed=SEED, dropout=dropout)
        seen["levels"], seen["loss"] = levels, float(loss)
    step(False); step(True)                         # warm-up: lazy kernel loads, allocator
    t_off, t_on = [], []
    for _ in range(steps):
        t_off.append(timed(lambda: step(False)))
        t_on.append(timed(lambda: step(True)))
    return dict(SHAPE, batch=BATCH, rows_per_utterance=[len(t) + len(p) + len(r) + 2 for t, p, r in zip(texts, proms, resps)],
                response_frames=[len(r) for r in resps], levels=seen["levels"], steps=steps, dropout_off_ms=t_off, dropout_on_ms=t_on,
                dropout_off_median_ms=statistics.median(t_off), dropout_on_median_ms=statistics.median(t_on),
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round24_nar_train.json"))
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--limit", type=int, default=600, help="seconds the child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:                                  # one process: prints its row as the last line
        print(json.dumps(measure(args.steps)), flush=True)
        return 0
    import __graft_entry__ as g
    g.build()
    from bench import build_id
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:                           # a fault, an abort or the time limit: nothing more is started on the GPU
        print(f"[nar_train_latency] exit status {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}", flush=True)
        return r.returncode
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    result = dict(build_id=build_id(), dtype="f32", shape="nar-quarter", **row)
    print(f"[nar_train_latency] nar-quarter, {BATCH} utterances of {row['rows_per_utterance']} rows: forward_backward "
          f"{row['dropout_off_median_ms']:.1f} ms, with dropout {row['dropout_on_median_ms']:.1f} ms (medians of {args.steps})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"[nar_train_latency] wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

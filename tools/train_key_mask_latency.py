#!/usr/bin/env python3
"""Time of the training step with the key mask, D3PMTrainer.forward_backward(timesteps=3, mask_padding=True), against the same
step with the padding as keys, one utterance, fp32, at two shapes:
  native   the upstream-native model (d = 32, canvas 448, s_text 50, s_prompt 398) on the 300 frames of
           tests/golden/native_forward.npz and the text / prompt of synth.make_inputs;
  d512     the LibriTTS shape (d = 512, canvas 768, s_text 50, s_prompt 225) with 500 live frames and the text / prompt of
           synth.make_inputs.
The arms are interleaved on one box: PAIRS times (off, on), each call synchronised and timed on its own after one warm-up of
both; the medians of PAIRS are reported.  Every shape runs in a child process of its own under `timeout`, so a GPU step that
hangs ends there and nothing is started after it.

    python tools/train_key_mask_latency.py [--out profiles/round18_train_key_mask.json] [--pairs 6] [--limit 300]

A number, no threshold: nothing was known about the speed of this step before.  The masked backward pass skips the masked keys'
waves and the key loops stop at the length, so it does less work; the forward pass runs the masked arm of the generic attention.
Reports time only; it makes no statement about audio quality (the weights are synthetic)."""
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

SHAPES = ("native", "d512")
TIMESTEPS, SEED = 3, 7


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def setup(shape):
    """-> cfg, model (fp32 on cuda:0), text, prompt, resps of one utterance"""
    import numpy as np
    import torch
    from vall_e.vall_e import AR, synth
    if shape == "native":
        cfg = synth.D3PMConfig.native()
        model = AR.reference_native()
        g = np.load(os.path.join(ROOT, "tests", "golden", "native_forward.npz"))
        resps = torch.from_numpy(g["resps"].astype(np.int64))
    else:
        cfg = synth.D3PMConfig.libritts()
        model = AR.from_config(cfg)
        resps = torch.randint(1, cfg.n_classes - 1, (500,), generator=torch.Generator().manual_seed(5))
    model.load_state_dict(synth.make_state_dict(cfg, 0))
    texts, proms = synth.make_inputs(cfg, 2, 1)
    return cfg, model.float().to("cuda:0"), texts[0], proms[0], resps


def measure(shape, pairs):
    import torch
    from vall_e.vall_e.train import D3PMTrainer, key_mask_lengths
    cfg, model, text, prom, resps = setup(shape)
    trainer = D3PMTrainer(model)

    def step(mask):
        for p in model.parameters():
            p.grad = None
        trainer.forward_backward([text], [prom], [resps], seed=SEED, timesteps=TIMESTEPS, mask_padding=mask)
    step(False); step(True)                         # warm-up: lazy kernel loads, allocator
    t_off, t_on = [], []
    for _ in range(pairs):
        t_off.append(timed(lambda: step(False)))
        t_on.append(timed(lambda: step(True)))
    frames, tl, pl = key_mask_lengths(cfg, [text], [prom], [resps])
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    return dict(shape=shape, d_model=cfg.d_model, canvas=cfg.canvas, s_text=cfg.s_text, s_prompt=cfg.s_prompt, timesteps=TIMESTEPS,
                frame_keys=frames[0], text_keys=tl[0], prompt_keys=pl[0], pairs=pairs, mask_off_ms=t_off, mask_on_ms=t_on,
                mask_off_median_ms=m_off, mask_on_median_ms=m_on, on_over_off=m_on / m_off, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round18_train_key_mask.json"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--limit", type=int, default=300, help="seconds each shape's child process may take")
    ap.add_argument("--child", choices=SHAPES, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:                                  # one shape, one process: prints its row as the last line
        print(json.dumps(measure(args.child, args.pairs)), flush=True)
        return 0
    import __graft_entry__ as g
    g.build()
    from bench import build_id
    result = dict(build_id=build_id(), dtype="f32", batch=1, rows=[])
    for shape in SHAPES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", shape, "--pairs", str(args.pairs)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:                       # a fault, an abort or the time limit: nothing more is started on the GPU
            print(f"[train_key_mask_latency] {shape}: exit status {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}", flush=True)
            return r.returncode
        row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        result.setdefault("device", row.pop("device"))
        print(f"[train_key_mask_latency] {shape:6s}: mask off {row['mask_off_median_ms']:.1f} ms, mask on {row['mask_on_median_ms']:.1f} ms "
              f"(on / off {row['on_over_off']:.3f}); keys {row['frame_keys']} / {row['text_keys']} / {row['prompt_keys']}", flush=True)
        result["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"[train_key_mask_latency] wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

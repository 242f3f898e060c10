#!/usr/bin/env python3
"""Time of AR.generate_audio(mask_padding=True) against the unmasked call of the same build on the same batch, at 32 and at 1
utterances x 750 frames in bf16 (the libritts configuration of bench.py), the whole reverse process (condition encoders + 99
evaluations):
  full     every length full (750 frames, texts of s_text phonemes, prompts of s_prompt rows): no key tile is skipped, so this is what
           the masked arms themselves cost (their registers, the select in the ragged tile, the length loads);
  ragged   frame counts drawn once from 250 .. 750 (seeded), texts and prompts of synth.make_inputs: both arms run the same
           n_frames, the masked one does not walk the key tiles behind a length.
Every masked arm is interleaved with the unmasked arm on one box: PAIRS times (off, on), each call synchronised and timed on its own
after one warm-up of both; the medians are reported.  Optionally (--parent-tree) the default bench.py path of this build is run
against a built checkout of the parent commit, interleaved, with --dump-outputs: the ids must be byte-identical.

    python tools/key_mask_latency.py [--out profiles/round10_key_mask.json] [--pairs 6] [--parent-tree DIR]

Reports time only; it makes no statement about audio quality (the weights are synthetic and were not trained with the mask)."""
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


def inputs(cfg, batch, kind):
    """-> texts, proms, n_frames (a list of `batch` ints)"""
    import numpy as np
    import torch
    from vall_e.vall_e import synth
    if kind == "full":
        g = torch.Generator().manual_seed(5)
        return ([torch.randint(1, 70, (cfg.s_text,), generator=g) for _ in range(batch)],
                [torch.randint(0, 1024, (cfg.s_prompt, cfg.n_levels), generator=g) for _ in range(batch)], [cfg.n_frames] * batch)
    texts, proms = synth.make_inputs(cfg, batch, 1)
    lens = np.random.Generator(np.random.PCG64(10)).integers(250, cfg.n_frames + 1, size=32)      # one draw; batch 1 takes its first
    return texts, proms, [int(v) for v in lens[:batch]]


def measure(model, cfg, batch, kind, pairs):
    texts, proms, lens = inputs(cfg, batch, kind)
    off = lambda: model.generate_audio(texts, proms, seed=7, n_frames=lens)
    on = lambda: model.generate_audio(texts, proms, seed=7, n_frames=lens, mask_padding=True)
    off(); on()                                     # warm-up: workspaces, lazy kernel loads
    t_off, t_on = [], []
    for _ in range(pairs):
        t_off.append(timed(off))
        t_on.append(timed(on))
    n_tok = sum(lens)
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    f, tl, pl = model.key_lengths(texts, proms, lens)
    return dict(batch=batch, lengths=kind, frames=lens, text_keys=tl, prompt_keys=pl, canvas=cfg.canvas, s_text=cfg.s_text,
                s_prompt=cfg.s_prompt, pairs=pairs, mask_off_ms=t_off, mask_on_ms=t_on, mask_off_median_ms=m_off,
                mask_on_median_ms=m_on, on_over_off=m_on / m_off, mask_off_tokens_per_s=n_tok / m_off * 1e3,
                mask_on_tokens_per_s=n_tok / m_on * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round10_key_mask.json"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--batches", default="32,1")
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
        for kind in ("full", "ragged"):
            row = measure(model, cfg, batch, kind, args.pairs)
            print(f"[key_mask_latency] batch {batch:3d} {kind:6s}: mask off {row['mask_off_median_ms']:.1f} ms, mask on "
                  f"{row['mask_on_median_ms']:.1f} ms (on / off {row['on_over_off']:.3f})", flush=True)
            result["rows"].append(row)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    write()
    if args.parent_tree:
        result["bench_default_path_vs_parent"] = bench_against_parent(args.parent_tree)
        print("[key_mask_latency] bench.py default path vs parent:", json.dumps(result["bench_default_path_vs_parent"]), flush=True)
    write()
    print(f"[key_mask_latency] wrote {args.out}")


if __name__ == "__main__":
    main()

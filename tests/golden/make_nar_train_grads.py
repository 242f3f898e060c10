"""Fixture of the NAR training step: loss and gradients of the reference's OWN NAR (nar.py:53-74 over base.py:403-488) by
torch.autograd -> tests/golden/nar_train_grads.npz.  Build container only (needs the reference checkout, loaded through
ref_harness exactly as make_golden.py:gen_nar loads it); CPU, a few seconds:

    python tests/golden/make_nar_train_grads.py

The reference's NAR(d_model=128, n_heads=2, n_layers=2, p_dropout=0.0) in train mode runs its training call on
synth.make_nar_inputs(3, 1, n_levels=8) with synth.make_nar_state_dict weights; torch.randint is replaced for the call so that
the levels are (0, 3, 6), and `loss["nll"].backward()` gives the gradients.  fp32 autograd over tests/nar_train_ref.py must give
the same loss within 1e-6 and every gradient within 1e-5 of that tensor's maximum (the two graphs sum in different orders).
Kept: the levels, the loss, and per parameter nar_train_ref.summary -- sum, absolute sum, 8 strided samples; for the three
embedding tables the indices of the non-zero rows, the samples taken from those rows.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tts-with-diffusion-model_amd"), ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_harness as rh  # noqa: E402
import nar_train_ref as R  # noqa: E402
from vall_e.vall_e import synth  # noqa: E402

LEVELS = (0, 3, 6)
W_SEED, IN_SEED = 0, 1


def reference_nar_module():
    rh.load_reference_modules()
    spec = importlib.util.spec_from_file_location(rh._PKG + ".nar", os.path.join(rh.REF_ROOT, "vall_e", "vall_e", "nar.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[rh._PKG + ".nar"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    assert rh.reference_available(), "needs the reference checkout (build container only)"
    torch.manual_seed(0)
    mod = reference_nar_module()
    cfg = synth.NARConfig(d_model=128, n_heads=2, n_layers=2)
    sd32 = synth.make_nar_state_dict(cfg, W_SEED)
    m = mod.NAR(cfg.n_tokens, d_model=cfg.d_model, n_heads=cfg.n_heads, n_layers=cfg.n_layers, p_dropout=0.0).train()
    m.load_state_dict(sd32)
    texts, proms, resps = synth.make_nar_inputs(3, IN_SEED, n_levels=8)

    orig = torch.randint
    torch.randint = lambda *a, **k: torch.tensor(LEVELS)       # nar.py:56 draws the levels from the global generator
    try:
        out = m(texts, proms, resps)
    finally:
        torch.randint = orig
    assert out == []
    loss = m.loss["nll"]
    loss.backward()

    loss_r, grads_r = R.loss_and_grads(sd32, cfg.n_heads, cfg.n_layers, texts, proms, resps, LEVELS, dtype=torch.float32)
    assert abs(float(loss.detach()) - loss_r) <= 1e-6, (float(loss.detach()), loss_r)
    res = {"levels": np.array(LEVELS, dtype=np.int64), "loss": np.array(float(loss.detach()), dtype=np.float64)}
    worst = 0.0
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        scale = float(p.grad.abs().max())
        err = float((p.grad - grads_r[name]).abs().max())
        assert err <= 1e-5 * scale, (name, err, scale)
        worst = max(worst, err / scale)
        stats, rows = R.summary(name, p.grad)
        res["g/" + name] = stats
        if rows is not None:
            res["rows/" + name] = rows.astype(np.int32)
    assert sorted(k[2:] for k in res if k.startswith("g/")) == sorted(sd32), "one entry per parameter"
    np.savez_compressed(os.path.join(HERE, "nar_train_grads.npz"), **res)
    print(f"nar_train_grads.npz: loss {float(loss.detach()):.6f} (restatement off by {abs(float(loss.detach()) - loss_r):.1e}), "
          f"{len(sd32)} gradients, worst restatement error {worst:.1e} of the tensor's maximum")


if __name__ == "__main__":
    main()

"""Key-padding masks in the training step (DESIGN.md "Key masks in the training step"): forward_backward(mask_padding=True) and
forward(mask_padding=True) against the CPU oracle at the TRUNCATED shape -- canvas = n_frames = L, s_text = len(text), s_prompt =
rows(prompt) -- which is what the masked step computes:

    loss = (L / C) loss' + (T - 1) (C - L) ln(K) / (C L'),      grad = (L / C) grad'  for every parameter

(every padded query row adds the constant CE(0-logits, target 0) = ln K to the canvas mean and nothing to any gradient).  Native
shape (d = 32, 16 heads of width 2, canvas 448, s_text 50, s_prompt 398), the 300 frames of tests/golden/native_forward.npz (no
code 0: L = L' = 300, no multiple of 64), texts and prompts shorter than their pads.  Tolerances: tests/test_gpu_train.py."""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from key_mask_mirror import masked_mirror_encoder
from oracle import d3pm_oracle as O
from oracle import philox
from util import REPORT, load, native_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _native():
    cfg, sd32, texts, proms, _ = native_setup(torch.float32)
    g = load("native_forward.npz")
    resps = torch.from_numpy(g["resps"].astype(np.int64))
    assert resps.shape == (300,) and int((resps == 0).sum()) == 0
    for t, p in zip(texts[:2], proms[:2]):
        assert 0 < t.shape[0] < cfg.s_text and 0 < p.shape[0] < cfg.s_prompt
    return cfg, sd32, texts, proms, resps, int(g["seed"])


def _model(sd32, dtype=torch.float32):
    from vall_e.vall_e import AR
    m = AR.reference_native()
    m.load_state_dict(sd32)
    return m.to(dtype).to(DEV)


def _step(sd32, texts, proms, resps, **kw):
    from vall_e.vall_e.train import D3PMTrainer
    m = _model(sd32)
    loss, _ = D3PMTrainer(m).forward_backward(texts, proms, resps, **kw)
    return float(loss), {n: (None if p.grad is None else p.grad.detach().cpu().clone()) for n, p in m.named_parameters()}


def _truncated(cfg, L, n_text, n_prompt):
    return dataclasses.replace(O.Shape.of(cfg), canvas=L, n_frames=L, s_text=n_text, s_prompt=n_prompt)


def _oracle(cfg, sd, shape, text, prom, resps, seed, T, utt=0, grad=True):
    """O.training_forward at `shape`; q_noise(t) = the first shape.canvas rows of the canvas-wide Philox draw of utterance `utt`."""
    sd = {k: v.clone().requires_grad_(grad and v.is_floating_point()) for k, v in sd.items()}

    def q_noise(t):
        return torch.from_numpy(philox.uniform_batch(seed, t, utt, 1, cfg.canvas, stream=philox.STREAM_Q_SAMPLE))[0][: shape.canvas]

    with torch.set_grad_enabled(grad):
        loss, logits = O.training_forward(sd, shape, text, prom, resps, q_noise, timesteps=T)
    if not grad:
        return float(loss), logits
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}


@functools.lru_cache(maxsize=None)
def _oracle_truncated(T):
    """The plain truncated reference of utterance 0, shared by the tests that need it."""
    cfg, sd32, texts, proms, resps, seed = _native()
    shape = _truncated(cfg, 300, texts[0].shape[0], proms[0].shape[0])
    return _oracle(cfg, sd32, shape, texts[0], proms[0], resps, seed, T)


def _masked_loss(cfg, ref_loss, L, n_live, T):
    C = cfg.canvas
    return (L / C) * ref_loss + (T - 1) * (C - L) * math.log(cfg.n_classes) / (C * n_live)


def _check(cfg, got_loss, got, ref_loss, ref, L, n_live, T, tag):
    """loss within 1e-4 * max(1, |ref|), every gradient within 2e-4 * max|ref| + 1e-7 of (L / C) * the oracle's, >= 230 tensors."""
    want_loss = _masked_loss(cfg, ref_loss, L, n_live, T)
    print(f"{tag}: loss {got_loss:.8f} expected {want_loss:.8f} (oracle at the truncated shape {ref_loss:.8f})")
    assert abs(got_loss - want_loss) < 1e-4 * max(1.0, abs(want_loss)), (got_loss, want_loss)
    worst, checked = {}, 0
    for name, g in got.items():
        if ".cross_attn2." in name or name.startswith("token_emb"):
            assert g is None, name
            continue
        want = ref.get(name)
        assert want is not None, name
        assert g is not None, f"no gradient for {name}"
        want = want * (L / cfg.canvas)
        if name in ("text_emb.weight", "resps_emb.weight"):     # nn.Embedding(padding_idx=0) upstream: row 0 gets no gradient
            want = want.clone()
            want[0] = 0
        err, scale = (g - want).abs().max().item(), want.abs().max().item()
        worst[name] = err / max(scale, 1e-8)
        checked += 1
        assert err <= 2e-4 * scale + 1e-7, f"{name}: max |grad error| {err:.3e} vs gradient scale {scale:.3e}"
    w = max(worst, key=worst.get)
    print(f"{tag}: {checked} tensors, worst relative error {worst[w]:.3e} ({w})")
    assert checked >= 230
    REPORT[f"train_key_mask_{tag}"] = {"loss_hip": got_loss, "loss_expected": want_loss, "tensors_checked": checked,
                                       "worst_relative_error": worst[w], "worst_tensor": w}


def _atomically_accumulated(name):
    """tests/test_gpu_guidance.py::_atomically_accumulated: the gradients d3pm_train.hip sums with atomicAdd (LayerNorm weights and
    biases, FiLM -> timestep_fc / time_emb, the embedding tables); two runs of one call differ in their last bits there."""
    return "norm" in name or "timestep_fc" in name or name.endswith("_emb.weight")


def _same_step(a, b, tag):
    """loss and every fixed-order gradient bit for bit, the atomic ones within 2e-4 * scale + 1e-7."""
    (l0, g0), (l1, g1) = a, b
    assert l0 == l1, (tag, l0, l1)
    assert g0.keys() == g1.keys()
    exact = [n for n in g0 if not _atomically_accumulated(n)]
    assert len(exact) >= 150 and {"final.weight", "final.bias"} <= set(exact)
    assert sum(g0[n] is not None for n in exact) >= 100
    for n in g0:
        if g0[n] is None:
            assert g1[n] is None, (tag, n)
        elif n in exact:
            assert torch.equal(g0[n], g1[n]), f"{tag}: {n} is not bit-equal"
        else:
            assert (g0[n] - g1[n]).abs().max().item() <= 2e-4 * g0[n].abs().max().item() + 1e-7, (tag, n)


# ---- 1. the masked step is the model at the truncated shape ---------------------------------------------------------------------
def test_masked_step_matches_autograd_over_the_oracle_at_the_truncated_shape():
    cfg, sd32, texts, proms, resps, seed = _native()
    T = 4
    ref_loss, ref = _oracle_truncated(T)
    loss, got = _step(sd32, [texts[0]], [proms[0]], [resps], seed=seed, timesteps=T, mask_padding=True)
    _check(cfg, loss, got, ref_loss, ref, 300, 300, T, "native_f32")
    # the mask took effect: encoder and block gradients are not those of the step with the padding as keys
    _, plain = _step(sd32, [texts[0]], [proms[0]], [resps], seed=seed, timesteps=T)
    moved = {n: (got[n] - plain[n]).abs().max().item() / plain[n].abs().max().item() for n in got
             if got[n] is not None and n.startswith(("encodertext.", "encoder2.", "blocks."))}
    far = [n for n, v in moved.items() if v > 1e-3]
    print(f"{len(far)} of {len(moved)} encoder / block gradients moved by more than 1e-3; largest {max(moved.values()):.3e}")
    assert any(n.startswith(("encodertext.", "encoder2.")) for n in far) and any(n.startswith("blocks.") for n in far)


# ---- 2. the evaluation-only loss ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f32", "f16"])
def test_forward_takes_the_mask(tag):
    """AR.forward(mask_padding=True): the loss follows the same formula, within 2e-4 (fp32) / 4e-3 (a model in fp16) -- the bounds
    DESIGN_HISTORY.md section 7 records for forward; the returned logits keep their shape."""
    cfg, sd32, texts, proms, resps, seed = _native()
    T = 3
    dtype = torch.float32 if tag == "f32" else torch.float16
    if tag == "f32":
        ref_loss = _oracle_truncated(T)[0]
    else:
        shape = _truncated(cfg, 300, texts[0].shape[0], proms[0].shape[0])
        ref_loss, _ = _oracle(cfg, {k: v.to(dtype) for k, v in sd32.items()}, shape, texts[0], proms[0], resps, seed, T, grad=False)
    want = _masked_loss(cfg, ref_loss, 300, 300, T)
    m = _model(sd32, dtype)
    m.timesteps = T
    last = m([texts[0]], [proms[0]], [resps], seed=seed, mask_padding=True)
    loss = float(m.loss)
    plain = _model(sd32, dtype)
    plain.timesteps = T
    plain([texts[0]], [proms[0]], [resps], seed=seed)
    print(f"forward {tag}: loss {loss:.8f} expected {want:.8f}; with the padding as keys {float(plain.loss):.8f}")
    REPORT[f"train_key_mask_forward_{tag}"] = {"hip": loss, "expected": want, "unmasked": float(plain.loss)}
    assert abs(loss - want) < (2e-4 if tag == "f32" else 4e-3), (loss, want)
    assert last.shape == (cfg.canvas, cfg.n_classes) and last.dtype == dtype and bool((last[300:] == 0).all())
    assert float(last[:300].float().abs().max()) > 0
    if tag == "f32":      # and it is the loss the training step reports
        l_step, _ = _step(sd32, [texts[0]], [proms[0]], [resps], seed=seed, timesteps=T, mask_padding=True)
        assert abs(loss - l_step) < 1e-4 * max(1.0, abs(l_step)), (loss, l_step)


# ---- 3. full lengths are neutral ------------------------------------------------------------------------------------------------
def test_full_lengths_and_the_default_are_the_step_of_today():
    cfg, sd32, _, _, _, seed = _native()
    g = torch.Generator().manual_seed(7)
    text = torch.randint(1, 100, (cfg.s_text,), generator=g)
    prom = torch.randint(0, cfg.n_classes - 1, (cfg.s_prompt, cfg.n_levels), generator=g)
    resps = torch.randint(1, cfg.n_classes - 1, (cfg.canvas,), generator=g)
    kw = dict(seed=seed, timesteps=3)
    base = _step(sd32, [text], [prom], [resps], **kw)
    _same_step(base, _step(sd32, [text], [prom], [resps], mask_padding=True, **kw), "full lengths, mask_padding=True")
    _same_step(base, _step(sd32, [text], [prom], [resps], mask_padding=False, **kw), "mask_padding=False")


# ---- 4. with train-mode dropout -------------------------------------------------------------------------------------------------
def test_masked_step_with_dropout_matches_the_oracle_with_the_mirror_encoder(monkeypatch):
    from vall_e.vall_e.train import DROPOUT_TRAIN
    cfg, sd32, texts, proms, resps, seed = _native()
    T = 3
    shape = _truncated(cfg, 300, texts[0].shape[0], proms[0].shape[0])
    # without dropout the mirror is the oracle's encoder
    x = torch.randn(shape.s_text, cfg.d_model, generator=torch.Generator().manual_seed(0))
    for name in ("encodertext", "encoder2"):
        a = masked_mirror_encoder(seed, 0, 0.0, 0.0, (cfg.s_text, cfg.s_prompt))(sd32, name, x, shape)
        b = O.cond_encoder(sd32, name, x, shape)
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item(), name
    monkeypatch.setattr(O, "cond_encoder", masked_mirror_encoder(seed, 0, *DROPOUT_TRAIN, (cfg.s_text, cfg.s_prompt)))
    ref_loss, ref = _oracle(cfg, sd32, shape, texts[0], proms[0], resps, seed, T)
    monkeypatch.undo()
    loss, got = _step(sd32, [texts[0]], [proms[0]], [resps], seed=seed, timesteps=T, dropout=True, mask_padding=True)
    _check(cfg, loss, got, ref_loss, ref, 300, 300, T, "native_f32_dropout")
    # the dropout took effect: the encoder gradients of the reference are not the eval-mode ones (the loss barely feels it)
    _, plain = _oracle_truncated(T)
    for name in ref:
        if name == "text_emb.weight" or name.startswith("encoder2."):
            moved = (ref[name] - plain[name]).abs().max().item() / plain[name].abs().max().item()
            assert moved > 1e-3, (name, moved)


# ---- 5. a dropped condition keeps its padding ------------------------------------------------------------------------------------
def test_a_dropped_text_keeps_all_of_its_padding_as_keys():
    """cond_drop = (1, 0): the oracle on the empty text with s_text left at the padded count, the other lengths truncated."""
    cfg, sd32, texts, proms, resps, seed = _native()
    T = 3
    shape = _truncated(cfg, 300, cfg.s_text, proms[0].shape[0])
    ref_loss, ref = _oracle(cfg, sd32, shape, texts[0][:0], proms[0], resps, seed, T)
    loss, got = _step(sd32, [texts[0]], [proms[0]], [resps], seed=seed, timesteps=T, cond_drop=(1.0, 0.0), mask_padding=True)
    _check(cfg, loss, got, ref_loss, ref, 300, 300, T, "native_f32_text_dropped")


# ---- 6. a batch is its shards ----------------------------------------------------------------------------------------------------
def test_two_utterance_batch_equals_its_shards_with_utt0():
    """tolerance and structure of tests/test_gpu_train_dropout.py::test_two_utterance_batch_equals_its_shards_with_utt0"""
    cfg, sd32, texts, proms, resps0, seed = _native()
    resps1 = torch.randint(1, cfg.n_classes - 1, (260,), generator=torch.Generator().manual_seed(1))
    kw = dict(seed=seed, timesteps=3, dropout=True, mask_padding=True)
    lb, gb = _step(sd32, texts[:2], proms[:2], [resps0, resps1], **kw)
    l0, g0 = _step(sd32, [texts[0]], [proms[0]], [resps0], utt0=0, **kw)
    l1, g1 = _step(sd32, [texts[1]], [proms[1]], [resps1], utt0=1, **kw)
    assert abs(lb - (l0 + l1) / 2) <= 1e-5 * abs(lb)
    assert gb.keys() == g0.keys() == g1.keys()
    worst = {}
    for name in gb:
        if gb[name] is None:
            assert g0[name] is None and g1[name] is None, name
            continue
        want = (g0[name] + g1[name]) / 2
        scale = max(g0[name].abs().max().item(), g1[name].abs().max().item(), 1e-12)
        err = (gb[name] - want).abs().max().item()
        worst[name] = err / scale
        assert err <= 1e-5 * scale + 1e-10, (name, err, scale)
    assert len(worst) >= 230
    # and the mask is part of what a shard computes: without it the second utterance's step differs
    l1_plain, _ = _step(sd32, [texts[1]], [proms[1]], [resps1], utt0=1, seed=seed, timesteps=3, dropout=True)
    assert abs(l1 - l1_plain) > 1e-6
    REPORT["train_key_mask_shard_equality"] = {"loss_batch": lb, "loss_shards_mean": (l0 + l1) / 2,
                                               "worst_relative_error": max(worst.values()), "worst_tensor": max(worst, key=worst.get)}

"""Training-step dropout of the condition encoders on the GPU: the mask the kernels draw is the numpy mirror's bit for bit
(tests/test_train_dropout_api.py), the attention forward / backward with probability dropout match torch autograd over an
explicit softmax(scale Q K^T) o Z @ V, and the whole step with dropout=True matches autograd over the CPU oracle whose
condition encoder applies the six sites with the mirror's masks."""
import numpy as np
import pytest
import torch

from dropout_mirror import mirror_encoder as _mirror_encoder
from dropout_mirror import z as _z
from oracle import d3pm_oracle as O
from oracle import philox
from util import REPORT, load, native_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = (12345, (0xDEADBEEF << 32) | 77)          # the second has the high key word set


# ---- 1. mask bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [33, 50, 2048])
@pytest.mark.parametrize("p", [0.01, 0.1, 0.5])
def test_dropout_op_draws_the_mirror_mask(N, p):
    from vall_e.vall_e import train as T
    M, ld = 7, N + 5
    g = torch.Generator(device="cpu").manual_seed(N)
    for seed in SEEDS:
        for utt in (0, 3):
            for site in (T.dropout_site(0, 1, 2), T.dropout_site(1, T.MLP_LAYER, 1)):
                want = _z(seed, utt, site, (M, N), p).to(DEV)
                ones = torch.ones(M, ld, device=DEV)[:, :N]
                out_buf = torch.full((M, ld + 3), 7.0, device=DEV)
                y = T.dropout(ones, p, seed, utt, site, out=out_buf[:, :N])
                assert torch.equal(y, want), (seed, utt, site, (y != want).sum().item())
                assert bool((out_buf[:, N:] == 7.0).all())                      # nothing written past a row
                r = torch.randn(M, N + 2, generator=g).to(DEV)[:, :N]
                assert torch.equal(T.dropout(ones, p, seed, utt, site, residual=r), r + want)
                xr = torch.randn(M, ld, generator=g).to(DEV)
                x0 = xr.clone()
                T.dropout(xr[:, :N], p, seed, utt, site, out=xr[:, :N])            # in place
                assert torch.equal(xr[:, :N], x0[:, :N] * want) and torch.equal(xr[:, N:], x0[:, N:])


# ---- 2. attention with probability dropout, forward and backward -----------------------------------------------------------
def _attn_ref(q, k, v, H, scale, Z):
    """explicit softmax(scale q k^T) o Z @ v in float64; q [B,Tq,d], k / v [B,S,d], Z [B,H,Tq,S]."""
    B, Tq, d = q.shape
    S, hd = k.shape[1], d // H
    qh, kh, vh = (t.reshape(B, -1, H, hd).transpose(1, 2) for t in (q, k, v))
    P = torch.softmax((qh * scale) @ kh.transpose(-1, -2), dim=-1)
    return ((P * Z) @ vh).transpose(1, 2).reshape(B, Tq, d)


@pytest.mark.parametrize("B,H,hd,S", [(2, 16, 2, 50), (1, 16, 2, 398), (1, 16, 32, 225)])
def test_attention_dropout_forward_and_backward_match_autograd(B, H, hd, S):
    from vall_e.vall_e import _hip
    from vall_e.vall_e import train as T
    d, p, seed, utt0 = H * hd, 0.1, SEEDS[1], 5
    site = T.dropout_site(1, 1, 0)
    scale = hd ** -0.5
    g = torch.Generator(device="cpu").manual_seed(S + hd)
    qkv = torch.randn(B, S, 3 * d, generator=g).to(DEV)
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    do = torch.randn(B, S, d, generator=g).to(DEV)
    Z = torch.stack([_z(seed, utt0 + b, site, (H, S, S), p) for b in range(B)]).double().to(DEV)
    ref = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
    o_ref = _attn_ref(*ref, H, scale, Z)
    o_ref.backward(do.double())
    o = T.attention_dropout(q, k, v, H, scale, p, seed, utt0, site)
    fwd_err = (o.double() - o_ref).abs().max().item() / o_ref.abs().max().item()
    assert fwd_err <= 1e-5, fwd_err
    errs = {"forward": fwd_err}
    for beta in (0.0, 1.0):
        dqkv = torch.randn(B, S, 3 * d, generator=g).to(DEV)
        old = dqkv.clone()
        T.attention_bwd(q, k, v, do, dqkv[..., :d], dqkv[..., d:2 * d], dqkv[..., 2 * d:], H, scale, beta_kv=beta,
                        drop=(p, seed, utt0, site))
        for n_, got, r, base in (("dq", dqkv[..., :d], ref[0], 0.0), ("dk", dqkv[..., d:2 * d], ref[1], beta),
                                 ("dv", dqkv[..., 2 * d:], ref[2], beta)):
            sl = {"dq": slice(0, d), "dk": slice(d, 2 * d), "dv": slice(2 * d, 3 * d)}[n_]
            want = r.grad + base * old[..., sl].double()
            err = (got.double() - want).abs().max().item() / r.grad.abs().max().item()
            errs[f"{n_}_beta{int(beta)}"] = err
            assert err <= 2e-5, (n_, beta, err)
    # p = 0: the new entries are the existing generic attention and its backward
    o0 = T.attention_dropout(q, k, v, H, scale, 0.0, seed, utt0, site)
    o_gen = _hip.op_attention(q, k, v, H, scale, family=_hip.FAMILY_GENERIC)
    assert (o0 - o_gen).abs().max().item() <= 1e-6 * o_gen.abs().max().item()
    a, b_ = torch.zeros(B, S, 3 * d, device=DEV), torch.zeros(B, S, 3 * d, device=DEV)
    T.attention_bwd(q, k, v, do, a[..., :d], a[..., d:2 * d], a[..., 2 * d:], H, scale, drop=(0.0, seed, utt0, site))
    T.attention_bwd(q, k, v, do, b_[..., :d], b_[..., d:2 * d], b_[..., 2 * d:], H, scale)
    assert (a - b_).abs().max().item() <= 1e-6 * b_.abs().max().item()
    REPORT[f"attention_dropout_B{B}_H{H}_hd{hd}_S{S}"] = errs


# ---- 3.-5. the whole training step -----------------------------------------------------------------------------------------
def _model(sd32):
    from vall_e.vall_e import AR
    m = AR.reference_native()
    m.load_state_dict(sd32)
    return m.float().to(DEV)


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _step(sd32, texts, proms, resps, **kw):
    from vall_e.vall_e.train import D3PMTrainer
    m = _model(sd32)
    loss, _ = D3PMTrainer(m).forward_backward(texts, proms, resps, **kw)
    return float(loss), _grads(m)


def _native():
    cfg, sd32, texts, proms, _ = native_setup(torch.float32)
    g = load("native_forward.npz")
    return cfg, sd32, texts, proms, torch.from_numpy(g["resps"].astype(np.int64)), int(g["seed"])


def test_gradients_with_dropout_match_autograd_over_the_oracle(monkeypatch):
    from vall_e.vall_e.train import DROPOUT_TRAIN
    cfg, sd32, texts, proms, resps, seed = _native()
    T = 4
    shape = O.Shape.of(cfg)
    # the mirror is the oracle's encoder when nothing is dropped
    x = torch.randn(cfg.s_text, cfg.d_model, generator=torch.Generator().manual_seed(0))
    for name in ("encodertext", "encoder2"):
        a, b = _mirror_encoder(seed, 0, 0.0, 0.0)(sd32, name, x, shape), O.cond_encoder(sd32, name, x, shape)
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item(), name
    monkeypatch.setattr(O, "cond_encoder", _mirror_encoder(seed, 0, *DROPOUT_TRAIN))
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd32.items()}

    def q_noise(t):
        return torch.from_numpy(philox.uniform_batch(seed, t, 0, 1, cfg.canvas, stream=philox.STREAM_Q_SAMPLE))[0]

    ref_loss, _ = O.training_forward(sd, shape, texts[0], proms[0], resps, q_noise, timesteps=T)
    ref_loss.backward()
    ref_loss = float(ref_loss.detach())
    ref = {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}
    loss, got = _step(sd32, [texts[0]], [proms[0]], [resps], seed=seed, timesteps=T, dropout=True)
    assert abs(loss - ref_loss) < 1e-4 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    worst, checked = {}, 0
    for name, want in ref.items():
        if ".cross_attn2." in name or name.startswith("token_emb"):
            continue
        assert name in got, f"no gradient for {name}"
        if name in ("text_emb.weight", "resps_emb.weight"):     # nn.Embedding(padding_idx=0) upstream: row 0 gets no gradient
            want = want.clone()
            want[0] = 0
        err = (got[name].cpu() - want).abs().max().item()
        scale = want.abs().max().item()
        worst[name] = err / max(scale, 1e-8)
        checked += 1
        assert err <= 2e-4 * scale + 1e-7, f"{name}: max |grad error| {err:.3e} vs gradient scale {scale:.3e}"
    assert checked >= 230
    # dropout took effect: the encoder gradients are not the eval-mode ones
    _, plain = _step(sd32, [texts[0]], [proms[0]], [resps], seed=seed, timesteps=T)
    moved = {}
    for name in got:
        if name == "text_emb.weight" or name.startswith("encoder2."):
            moved[name] = (got[name] - plain[name]).abs().max().item() / plain[name].abs().max().item()
            assert moved[name] > 1e-3, (name, moved[name])
    REPORT["train_gradcheck_native_f32_dropout"] = {"loss_hip": loss, "loss_autograd": ref_loss, "tensors_checked": checked,
                                                    "worst_relative_error": max(worst.values()), "worst_tensor": max(worst, key=worst.get),
                                                    "least_relative_change_vs_eval": min(moved.values())}


def test_zero_probability_is_the_eval_mode_step():
    cfg, sd32, texts, proms, resps, seed = _native()
    l0, g0 = _step(sd32, [texts[0]], [proms[0]], [resps], seed=seed, timesteps=3)
    l1, g1 = _step(sd32, [texts[0]], [proms[0]], [resps], seed=seed, timesteps=3, dropout=(0.0, 0.0))
    assert abs(l0 - l1) <= 1e-6 * abs(l0)
    assert g0.keys() == g1.keys()
    # p = 0 launches nothing new, so the two runs differ only where LayerNorm / embedding gradients accumulate with fp32 atomics
    # in a different order: equal to rounding, not to the bit.  Those sums cancel (a LayerNorm weight's gradient can be 1e-6
    # while its terms are larger), hence the small absolute floor, 1000 x below the one of the autograd comparisons.
    worst = {}
    for name in g0:
        err = (g0[name] - g1[name]).abs().max().item()
        worst[name] = err
        assert err <= 1e-6 * g0[name].abs().max().item() + 1e-10, (name, err)
    REPORT["train_dropout_zero_p_vs_eval"] = {"loss_eval": l0, "loss_p0": l1, "worst_abs_error": max(worst.values()),
                                              "worst_tensor": max(worst, key=worst.get)}


def test_two_utterance_batch_equals_its_shards_with_utt0():
    cfg, sd32, texts, proms, resps0, seed = _native()
    gen = torch.Generator().manual_seed(1)
    resps1 = torch.randint(1, cfg.n_classes - 1, (260,), generator=gen)
    kw = dict(seed=seed, timesteps=3, dropout=True)
    lb, gb = _step(sd32, texts[:2], proms[:2], [resps0, resps1], **kw)
    l0, g0 = _step(sd32, [texts[0]], [proms[0]], [resps0], utt0=0, **kw)
    l1, g1 = _step(sd32, [texts[1]], [proms[1]], [resps1], utt0=1, **kw)
    assert abs(lb - (l0 + l1) / 2) <= 1e-5 * abs(lb)
    assert gb.keys() == g0.keys() == g1.keys()
    worst = {}
    for name in gb:
        want = (g0[name] + g1[name]) / 2
        # relative to the larger of the two utterances' gradients (where they cancel, the mean is smaller than the terms whose
        # rounding it carries), with the absolute floor of the fp32-atomic sums of test_zero_probability_is_the_eval_mode_step
        scale = max(g0[name].abs().max().item(), g1[name].abs().max().item(), 1e-12)
        err = (gb[name] - want).abs().max().item()
        worst[name] = err / scale
        assert err <= 1e-5 * scale + 1e-10, (name, err, scale)
    REPORT["train_dropout_shard_equality"] = {"loss_batch": lb, "loss_shards_mean": (l0 + l1) / 2,
                                              "worst_relative_error": max(worst.values()), "worst_tensor": max(worst, key=worst.get)}

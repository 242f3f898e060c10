"""Key-padding masks in the training step, kernel level (include/d3pm_hip.h "Key-padding masks in the training step"):
d3pm_op_attention_bwd_keylen_f32 and d3pm_op_attention_dropout_keylen_f32 against float64 autograd over an explicit softmax with
-inf on the keys >= key_len[b] (the dropout factors Z, drawn at the padded extents, included where used), and the exact statements:
what a masked key receives, that nothing behind key_len is read, that a masked utterance is the unmasked entry on the truncated
views, and that a full mask / no mask are the existing entries.

Shapes (B, H, hd, Tq, S), the smallest at which these kernels can go wrong: a mask of a single key, one inside a 64-lane stride and
a full one in one call; Tq != S with a mask that crosses a lane stride and a head as wide as a wave; and one where the per-lane
keep-bits go beyond bit 0."""
import functools

import pytest
import torch

from dropout_mirror import z as _z

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, UTT0 = (0xDEADBEEF << 32) | 77, 5          # the high key word set
SHAPES = [((3, 16, 2, 50, 50), (1, 37, 50)), ((2, 2, 64, 70, 130), (65, 128)), ((1, 16, 32, 225, 225), (200,))]
IDS = ["B3_hd2_S50", "B2_hd64_Tq70_S130", "B1_hd32_S225"]
PS = [0.0, 0.1]


def _site():
    from vall_e.vall_e import train as T
    return T.dropout_site(1, 1, 0)


def _ref(q, k, v, H, scale, key_len, Z):
    """explicit softmax(scale q k^T + mask) o Z @ v in float64; q [B,Tq,d], k / v [B,S,d], Z [B,H,Tq,S] or None."""
    B, Tq, d = q.shape
    S, hd = k.shape[1], d // H
    qh, kh, vh = (t.reshape(B, -1, H, hd).transpose(1, 2) for t in (q, k, v))
    sc = (qh * scale) @ kh.transpose(-1, -2)
    dead = torch.arange(S, device=q.device)[None, :] >= torch.as_tensor(key_len, device=q.device)[:, None]      # [B, S]
    P = torch.softmax(sc.masked_fill(dead[:, None, None, :], float("-inf")), dim=-1)
    if Z is not None:
        P = P * Z
    return (P @ vh).transpose(1, 2).reshape(B, Tq, d)


@functools.lru_cache(maxsize=None)
def _case(idx, p):
    """Inputs (q and do dense, k | v halves of one [B, S, 2d] buffer as the trainer has them) and the float64 reference, once."""
    (B, H, hd, Tq, S), key_len = SHAPES[idx]
    d, scale = H * hd, hd ** -0.5
    g = torch.Generator(device="cpu").manual_seed(1000 * idx + S)
    q = torch.randn(B, Tq, d, generator=g).to(DEV)
    kv = torch.randn(B, S, 2 * d, generator=g).to(DEV)
    do = torch.randn(B, Tq, d, generator=g).to(DEV)
    old = torch.randn(B, S, 2 * d, generator=g).to(DEV)
    Z = None
    if p > 0:      # drawn at the padded extents: index (h Tq + i) S + j, whatever the mask
        Z = torch.stack([_z(SEED, UTT0 + b, _site(), (H, Tq, S), p) for b in range(B)]).double().to(DEV)
    ref = [t.double().clone().requires_grad_(True) for t in (q, kv[..., :d], kv[..., d:])]
    o_ref = _ref(*ref, H, scale, key_len, Z)
    o_ref.backward(do.double())
    c = dict(B=B, H=H, hd=hd, Tq=Tq, S=S, d=d, scale=scale, key_len=key_len, kl=torch.tensor(key_len, dtype=torch.int32, device=DEV),
             q=q, kv=kv, do=do, old=old, o_ref=o_ref.detach(), grads=[t.grad for t in ref], p=p,
             drop=(p, SEED, UTT0, _site()) if p > 0 else None)
    return c


def _forward(c, kv=None, key_len="kl"):
    from vall_e.vall_e import _hip
    from vall_e.vall_e import train as T
    kv, d = c["kv"] if kv is None else kv, c["d"]
    kl = c["kl"] if isinstance(key_len, str) else key_len
    if c["p"] > 0:
        return T.attention_dropout(c["q"], kv[..., :d], kv[..., d:], c["H"], c["scale"], c["p"], SEED, UTT0, _site(), key_len=kl)
    return _hip.op_attention(c["q"], kv[..., :d], kv[..., d:], c["H"], c["scale"], family=_hip.FAMILY_GENERIC, key_len=kl)


def _backward(c, beta, kv=None, key_len="kl"):
    """-> (dq [B,Tq,d], dkv [B,S,2d]) with dkv starting from c["old"]."""
    from vall_e.vall_e import train as T
    kv, d = c["kv"] if kv is None else kv, c["d"]
    kl = c["kl"] if isinstance(key_len, str) else key_len
    dq, dkv = torch.full_like(c["q"], 7.0), c["old"].clone()
    T.attention_bwd(c["q"], kv[..., :d], kv[..., d:], c["do"], dq, dkv[..., :d], dkv[..., d:], c["H"], c["scale"], beta_kv=beta,
                    drop=c["drop"], key_len=kl)
    return dq, dkv


def _dead_rows(c):
    return torch.arange(c["S"], device=DEV)[None, :] >= c["kl"][:, None]      # [B, S]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_masked_forward_and_backward_match_autograd(idx, p):
    """forward <= 1e-5 and dQ / dK / dV <= 2e-5 relative (the bounds of test_attention_dropout_forward_and_backward_match_autograd),
    beta_kv 0 and 1; the dK / dV rows of masked keys are exactly 0 at beta = 0 and exactly the old contents at beta = 1."""
    c = _case(idx, p)
    d = c["d"]
    o = _forward(c)
    fwd_err = (o.double() - c["o_ref"]).abs().max().item() / c["o_ref"].abs().max().item()
    print(f"{IDS[idx]} p={p}: forward {fwd_err:.3e}")
    assert fwd_err <= 1e-5, fwd_err
    dead = _dead_rows(c)
    assert dead.any() and not dead.all(dim=1).any()
    for beta in (0.0, 1.0):
        dq, dkv = _backward(c, beta)
        for name, got, want, base in (("dq", dq, c["grads"][0], None), ("dk", dkv[..., :d], c["grads"][1], c["old"][..., :d]),
                                      ("dv", dkv[..., d:], c["grads"][2], c["old"][..., d:])):
            full = want if base is None else want + beta * base.double()
            err = (got.double() - full).abs().max().item() / want.abs().max().item()
            print(f"{IDS[idx]} p={p} beta={beta}: {name} {err:.3e}")
            assert err <= 2e-5, (name, beta, err)
            if base is not None:
                assert float(want[dead].abs().max()) == 0.0                     # the reference gives a masked key nothing either
                expect = torch.zeros_like(base[dead]) if beta == 0.0 else base[dead]
                assert torch.equal(got[dead], expect), (name, beta)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_rows_behind_key_len_are_not_read(idx, p):
    """NaN in the K and V rows behind key_len changes no output bit, forward or backward."""
    c = _case(idx, p)
    poisoned = c["kv"].clone()
    poisoned[_dead_rows(c)] = float("nan")
    assert torch.isnan(poisoned).any()
    o, o_nan = _forward(c), _forward(c, kv=poisoned)
    assert not torch.isnan(o_nan).any() and torch.equal(o, o_nan)
    for beta in (0.0, 1.0):
        (dq, dkv), (dq_nan, dkv_nan) = _backward(c, beta), _backward(c, beta, kv=poisoned)
        assert not torch.isnan(dq_nan).any() and not torch.isnan(dkv_nan).any(), beta
        assert torch.equal(dq, dq_nan) and torch.equal(dkv, dkv_nan), beta


@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_a_masked_utterance_is_the_unmasked_entry_on_the_truncated_views(idx):
    """Without dropout: utterance b of a masked call equals d3pm_op_attention_bwd_f32 on k[b:b+1, :key_len[b]], v[b:b+1, :key_len[b]]
    -- dQ and the live rows of dK / dV, bit for bit (the forward of the same views too)."""
    from vall_e.vall_e import _hip
    from vall_e.vall_e import train as T
    c = _case(idx, 0.0)
    d, H, scale = c["d"], c["H"], c["scale"]
    o = _forward(c)
    for beta in (0.0, 1.0):
        dq, dkv = _backward(c, beta)
        for b, n in enumerate(c["key_len"]):
            q1, kv1, do1 = c["q"][b:b + 1], c["kv"][b:b + 1, :n], c["do"][b:b + 1]
            dq1, dkv1 = torch.full_like(q1, 7.0), c["old"][b:b + 1].clone()
            T.attention_bwd(q1, kv1[..., :d], kv1[..., d:], do1, dq1, dkv1[:, :n, :d], dkv1[:, :n, d:], H, scale, beta_kv=beta)
            assert torch.equal(dq[b:b + 1], dq1), (beta, b)
            assert torch.equal(dkv[b:b + 1, :n], dkv1[:, :n]), (beta, b)
            if beta == 0.0:
                kvc = torch.empty(1, n, 2 * d, device=DEV).copy_(kv1)      # the forward binding wants the batch stride of n rows
                o1 = _hip.op_attention(q1, kvc[..., :d], kvc[..., d:], H, scale, family=_hip.FAMILY_GENERIC)
                assert torch.equal(o[b:b + 1], o1), b


def _bwd_entry(c, beta, key_len, p):
    """d3pm_op_attention_bwd_keylen_f32 called directly (key_len may be None = NULL, which the binding never passes on)."""
    from vall_e.vall_e import _hip
    from vall_e.vall_e.train import _ptr, _seed
    d = c["d"]
    q, k, v, do = c["q"], c["kv"][..., :d], c["kv"][..., d:], c["do"]
    dq, dkv = torch.full_like(q, 7.0), c["old"].clone()
    stats = torch.empty(c["B"] * c["H"] * c["Tq"] * 2, dtype=torch.float32, device=DEV)
    _hip.check(_hip.lib().d3pm_op_attention_bwd_keylen_f32(
        _ptr(q), q.stride(1), _ptr(k), _ptr(v), k.stride(1), _ptr(do), do.stride(1), _ptr(dq), dq.stride(1), _ptr(dkv[..., :d]),
        _ptr(dkv[..., d:]), dkv.stride(1), _ptr(stats), c["B"], c["Tq"], c["S"], c["H"], c["hd"], float(c["scale"]), float(beta),
        _ptr(key_len), float(p), _seed(SEED), UTT0, _site(), _hip.stream_ptr()), "d3pm_op_attention_bwd_keylen_f32")
    return dq, dkv


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_a_full_mask_and_no_mask_are_the_existing_entries(idx, p):
    """key_len = [S] * B and key_len = NULL against d3pm_op_attention_bwd_f32 / d3pm_op_attention_bwd_dropout_f32 and the existing
    forwards, bit for bit; p = 0 through the new entries against the entries without dropout."""
    from vall_e.vall_e import _hip
    from vall_e.vall_e import train as T
    c = _case(idx, p)
    d, H, scale = c["d"], c["H"], c["scale"]
    full = torch.full((c["B"],), c["S"], dtype=torch.int32, device=DEV)
    k, v = c["kv"][..., :d], c["kv"][..., d:]
    o_old = _forward(c, key_len=None)                                   # d3pm_op_attention / d3pm_op_attention_dropout_f32
    assert torch.equal(_forward(c, key_len=full), o_old)
    if p == 0.0:      # the dropout-forward entry at p = 0, masked and full, is the generic attention
        assert torch.equal(T.attention_dropout(c["q"], k, v, H, scale, 0.0, SEED, UTT0, _site(), key_len=full), o_old)
        assert torch.equal(T.attention_dropout(c["q"], k, v, H, scale, 0.0, SEED, UTT0, _site(), key_len=c["kl"]), _forward(c))
    for beta in (0.0, 1.0):
        dq_old, dkv_old = _backward(c, beta, key_len=None)              # d3pm_op_attention_bwd_f32 / _bwd_dropout_f32
        for kl in (full, None):
            dq, dkv = _bwd_entry(c, beta, kl, p)
            assert torch.equal(dq, dq_old) and torch.equal(dkv, dkv_old), (beta, kl is None)
    if p > 0:
        return
    c1 = _case(idx, 0.1)      # same inputs; its masked p = 0 call is the masked call without dropout
    dq0, dkv0 = _backward(c, 0.0)
    dq1, dkv1 = _bwd_entry(c1, 0.0, c1["kl"], 0.0)
    assert torch.equal(dq0, dq1) and torch.equal(dkv0, dkv1)


def test_the_entries_keep_the_argument_checks():
    """p outside [0, 1), the 4096 limit of the per-lane bit set under dropout (and only there), NULL pointers: refused, nothing launched."""
    from vall_e.vall_e import _hip
    from vall_e.vall_e import train as T
    B, H, hd, Tq, S = 1, 1, 2, 4, 4100
    q, kv, do = torch.zeros(B, Tq, 2, device=DEV), torch.zeros(B, S, 4, device=DEV), torch.zeros(B, Tq, 2, device=DEV)
    kl = torch.tensor([S], dtype=torch.int32, device=DEV)
    dq, dkv = torch.full_like(q, 7.0), torch.full_like(kv, 7.0)
    args = (q, kv[..., :2], kv[..., 2:], do, dq, dkv[..., :2], dkv[..., 2:], H, hd ** -0.5)
    for drop in ((0.1, 1, 0, 0), (1.0, 1, 0, 0), (-0.5, 1, 0, 0)):
        with pytest.raises(_hip.D3PMError):
            T.attention_bwd(*args, drop=drop, key_len=kl)
    with pytest.raises(_hip.D3PMError):
        T.attention_dropout(q, kv[..., :2], kv[..., 2:], H, hd ** -0.5, 1.0, 1, 0, 0, key_len=kl)
    with pytest.raises(_hip.D3PMError, match="key_len"):
        T.attention_bwd(*args, key_len=kl.long())
    torch.cuda.synchronize()
    assert bool((dq == 7.0).all()) and bool((dkv == 7.0).all()), "a refused call launches nothing"
    T.attention_bwd(*args, key_len=kl)      # without dropout 4100 keys are fine
    assert bool((dq == 0.0).all()) and bool((dkv == 0.0).all())

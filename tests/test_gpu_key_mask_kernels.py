"""Key-padding masks in the kernels the throughput path runs (d3pm_mfma_attn32.hip: attn32p_hd64 / attn32_hd64 / attn32_cross_hd64;
d3pm_mfma_attn.hip: attn_cross_hd64 and the paired attn_mfma_hd64) through d3pm_op_attention_keylen and
d3pm_op_attention_pair_keylen.  Contract, inputs and bound: tests/attention_ref.py, used as it is.

Four checks per schedule and storage type, on rows behind the length that hold large finite poison (K = 240: a masked score would be
the largest by far; V = 3e4):
  (a) the output is finite and does not change by one bit when the poison is replaced by other values;
  (b) an utterance equals the unmasked kernel on S = its length, bit for bit -- for the self-attention where the length is a
      multiple of 64 (the tile walk is then the same), for the pairs at every length (behind the lengths those kernels ARE the
      unmasked ones on the valid counts);
  (c) the recovered probabilities are exactly 0 behind the length and obey probability_bound against softmax_fp64(.., lens) in
      front of it;
  (d) every length = the padded count gives the unmasked launch, bit for bit."""
import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 2
D = H * R.HD
SCALE = 0.125
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
POISON = ((240.0, 3e4), (-97.0, -1234.0))      # (K, V) behind the length, two fillings


@pytest.fixture(autouse=True)
def _default_tuning(built_lib):
    from vall_e.vall_e import _hip
    _hip.reset_tuning()
    yield
    _hip.reset_tuning()


class Packed:
    """K and V of one problem as views of packed [B, S, 2 d] device rows."""

    def __init__(self, k, v):
        self.kv = torch.zeros(k.shape[0], k.shape[1], 2 * k.shape[2], dtype=k.dtype, device=DEV)
        self.d = k.shape[2]
        self.kv[..., :self.d] = k.to(DEV)
        self.kv[..., self.d:] = v.to(DEV)

    def set_v(self, v):
        self.kv[..., self.d:] = v.to(DEV)
        return self

    @property
    def k(self):
        return self.kv[..., :self.d]

    @property
    def v(self):
        return self.kv[..., self.d:]


def _rand_v(Bn, S, dtype, seed):
    return torch.randn(Bn, S, D, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _poisoned(k, v, lens, fill):
    kp, vp = k.clone(), v.clone()
    for b, n in enumerate(lens):
        kp[b, n:] = fill[0]
        vp[b, n:] = fill[1]
    return kp, vp


def _kl(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def _behind(ph, lens):
    """largest recovered probability of a masked key"""
    worst = 0.0
    for b, n in enumerate(lens):
        if n < ph.shape[-1]:
            worst = max(worst, float(ph[b, :, :, n:].abs().max()))
    return worst


# ---- self-attention on the 32 x 32 x 16 instruction ---------------------------------------------------------------------------
TQ, S_PAD = 128, 256
LENS = [1, 64, 65, 128, 129, 192, 193, 256]      # 1 .. 4 tiles, ragged and whole


def _self(g, q, p, key_len=None):
    from vall_e.vall_e import _hip
    with _hip.tuning(attn_query_groups=g):
        return _hip.op_attention(q, p.k, p.v, H, SCALE, family=2, key_len=key_len)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("g", [32, 33], ids=["pipelined", "plain"])
def test_masked_self_attention_32x32(g, dtype):
    Bn = len(LENS)
    q, k = R.flat_inputs(Bn, H, TQ, S_PAD, dtype, seed=11)
    v = _rand_v(Bn, S_PAD, dtype, seed=12)
    qd, kl = q.to(DEV), _kl(LENS)
    failures = []
    outs = []
    for fill in POISON:
        kp, vp = _poisoned(k, v, LENS, fill)
        outs.append(_self(g, qd, Packed(kp, vp), kl))
    if not bool(torch.isfinite(outs[0]).all()):
        failures.append("(a) non-finite output")
    if not torch.equal(outs[0], outs[1]):
        failures.append("(a) the output depends on the rows behind the length")
    for b, n in enumerate(LENS):
        if n % R.TILE:
            continue
        alone = _self(g, qd[b:b + 1].contiguous(), Packed(k[b:b + 1, :n].contiguous(), v[b:b + 1, :n].contiguous()))
        if not torch.equal(outs[0][b:b + 1], alone):
            failures.append(f"(b) utterance {b} (length {n}) differs from the unmasked kernel on S = {n}")
    kp, vp = _poisoned(k, v, LENS, POISON[0])
    p = Packed(kp, vp)
    ph = R.recover_probabilities(lambda pv: _self(g, qd, p.set_v(pv), kl), Bn, S_PAD, H, dtype)
    if _behind(ph, LENS) != 0.0:
        failures.append(f"(c) a masked key has probability {_behind(ph, LENS)}")
    rep = R.check_probabilities(ph, R.softmax_fp64(q, kp, SCALE, LENS), R.probability_bound(q, kp, SCALE, dtype, LENS), dtype)
    print(f"[key_mask] self g={g} {dtype}: {rep}")
    if not rep.ok:
        failures.append(f"(c) {rep}")
    clean = Packed(k, v)
    if not torch.equal(_self(g, qd, clean, _kl([S_PAD] * Bn)), _self(g, qd, clean)):
        failures.append("(d) full lengths differ from the unmasked launch")
    assert not failures, "\n".join(failures)


# ---- the cross-attention pair -------------------------------------------------------------------------------------------------
TQ2, S1_PAD, S2_PAD = 288, 50, 225
LENS1 = [a for a in (1, 17, 50) for _ in range(4)]
LENS2 = [1, 64, 65, 225] * 3
PAIR = [("resident_auto", {"attn_cross_resident": 2}),
        ("resident16", {"attn_cross_resident": 4}),
        ("resident32", {"attn_cross_resident": 5}),
        ("tile_split_grid", {"attn_cross_resident": 0, "attn_pair_sequential": 0}),
        ("tile_sequential", {"attn_cross_resident": 0, "attn_pair_sequential": 2})]


def _pair(knobs, q1, p1, q2, p2, kl1=None, kl2=None):
    from vall_e.vall_e import _hip
    with _hip.tuning(**knobs):
        return _hip.op_attention_pair(q1, p1.k, p1.v, q2, p2.k, p2.v, H, SCALE, key_len=kl1, key_len2=kl2)


def _recover_pair(knobs, q1d, p1, q2d, p2, kl1, kl2, Bn, dtype):
    nb1, nb2 = R.n_blocks(S1_PAD), R.n_blocks(S2_PAD)
    c1, c2 = [], []
    for blk in range(max(nb1, nb2)):
        p1.set_v(R.probe_values(Bn, S1_PAD, H, min(blk, nb1 - 1), dtype))
        p2.set_v(R.probe_values(Bn, S2_PAD, H, min(blk, nb2 - 1), dtype))
        o1, o2 = _pair(knobs, q1d, p1, q2d, p2, kl1, kl2)
        if blk < nb1:
            c1.append(R.heads(o1.cpu()))
        if blk < nb2:
            c2.append(R.heads(o2.cpu()))
    return torch.cat(c1, -1)[..., :S1_PAD], torch.cat(c2, -1)[..., :S2_PAD]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_masked_cross_attention_pairs(dtype):
    Bn = len(LENS1)
    q1, k1 = R.flat_inputs(Bn, H, TQ2, S1_PAD, dtype, seed=21)
    q2, k2 = R.flat_inputs(Bn, H, TQ2, S2_PAD, dtype, seed=22)
    v1, v2 = _rand_v(Bn, S1_PAD, dtype, seed=23), _rand_v(Bn, S2_PAD, dtype, seed=24)
    q1d, q2d, kl1, kl2 = q1.to(DEV), q2.to(DEV), _kl(LENS1), _kl(LENS2)
    refs = None
    failures, masked = [], {}
    for name, knobs in PAIR:
        outs = []
        for fill in POISON:
            k1p, v1p = _poisoned(k1, v1, LENS1, fill)
            k2p, v2p = _poisoned(k2, v2, LENS2, fill)
            outs.append(_pair(knobs, q1d, Packed(k1p, v1p), q2d, Packed(k2p, v2p), kl1, kl2))
        masked[name] = outs[0]
        for side in (0, 1):
            if not bool(torch.isfinite(outs[0][side]).all()):
                failures.append(f"{name} (a) non-finite output, problem {side + 1}")
            if not torch.equal(outs[0][side], outs[1][side]):
                failures.append(f"{name} (a) problem {side + 1} depends on the rows behind the length")
        for b, (n1, n2) in enumerate(zip(LENS1, LENS2)):
            a1, a2 = _pair(knobs, q1d[b:b + 1].contiguous(), Packed(k1[b:b + 1, :n1].contiguous(), v1[b:b + 1, :n1].contiguous()),
                           q2d[b:b + 1].contiguous(), Packed(k2[b:b + 1, :n2].contiguous(), v2[b:b + 1, :n2].contiguous()))
            if not (torch.equal(outs[0][0][b:b + 1], a1) and torch.equal(outs[0][1][b:b + 1], a2)):
                failures.append(f"{name} (b) utterance {b} (lengths {n1}, {n2}) differs from the unmasked pair on those key counts")
        k1p, v1p = _poisoned(k1, v1, LENS1, POISON[0])
        k2p, v2p = _poisoned(k2, v2, LENS2, POISON[0])
        if refs is None:
            refs = [(R.softmax_fp64(q, k, SCALE, ln), R.probability_bound(q, k, SCALE, dtype, ln))
                    for q, k, ln in ((q1, k1p, LENS1), (q2, k2p, LENS2))]
        got = _recover_pair(knobs, q1d, Packed(k1p, v1p), q2d, Packed(k2p, v2p), kl1, kl2, Bn, dtype)
        for side, ph, ln, (ref, rel) in zip(("text", "prompt"), got, (LENS1, LENS2), refs):
            if _behind(ph, ln) != 0.0:
                failures.append(f"{name} (c) {side}: a masked key has probability {_behind(ph, ln)}")
            rep = R.check_probabilities(ph, ref, rel, dtype)
            print(f"[key_mask] pair {name} {side} {dtype}: {rep}")
            if not rep.ok:
                failures.append(f"{name} (c) {side}: {rep}")
        c1, c2 = Packed(k1, v1), Packed(k2, v2)
        full = _pair(knobs, q1d, c1, q2d, c2, _kl([S1_PAD] * Bn), _kl([S2_PAD] * Bn))
        plain = _pair(knobs, q1d, c1, q2d, c2)
        if not (torch.equal(full[0], plain[0]) and torch.equal(full[1], plain[1])):
            failures.append(f"{name} (d) full lengths differ from the unmasked launch")
        one = _pair(knobs, q1d, c1, q2d, c2, None, kl2)      # a mask on the prompt problem alone leaves the text problem unmasked
        if not torch.equal(one[0], plain[0]):
            failures.append(f"{name}: key_len2 alone changed problem 1")
    for side in (0, 1):
        if not torch.equal(masked["resident16"][side], masked["tile_split_grid"][side]):
            failures.append(f"resident16 differs from the tile-by-tile pair under the mask, problem {side + 1}")
    assert not failures, "\n".join(failures)


def test_pair_key_len_arguments_are_validated_on_the_host():
    from vall_e.vall_e import _hip
    Bn = 2
    q1, k1 = R.flat_inputs(Bn, H, 16, 20, torch.float16, seed=1)
    q2, k2 = R.flat_inputs(Bn, H, 16, 65, torch.float16, seed=2)
    p1, p2 = Packed(k1, _rand_v(Bn, 20, torch.float16, 3)), Packed(k2, _rand_v(Bn, 65, torch.float16, 4))
    for bad in (torch.ones(Bn, dtype=torch.int64, device=DEV), torch.ones(Bn + 1, dtype=torch.int32, device=DEV), torch.ones(Bn, dtype=torch.int32)):
        with pytest.raises(_hip.D3PMError, match="key_len2"):
            _hip.op_attention_pair(q1.to(DEV), p1.k, p1.v, q2.to(DEV), p2.k, p2.v, H, SCALE, key_len2=bad)
        with pytest.raises(_hip.D3PMError, match="key_len"):
            _hip.op_attention_pair(q1.to(DEV), p1.k, p1.v, q2.to(DEV), p2.k, p2.v, H, SCALE, key_len=bad)

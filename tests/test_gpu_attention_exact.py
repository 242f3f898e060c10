"""Per-key exactness of every attention schedule (d3pm_generic.hip, d3pm_mfma_attn.hip, d3pm_mfma_attn32.hip,
d3pm_mfma_attn_lat.hip) through d3pm_op_attention / d3pm_op_attention_keylen / d3pm_op_attention_pair.

The max-abs-error tests of test_gpu_kernels.py cannot see one key that is dropped, counted twice or read from the neighbouring row:
with a nearly flat softmax over S keys it moves the output by |v| / S, under their limit.  Here the inputs are built so that a
single key is either everything (selector inputs: the output is one V row, bit for bit) or measured by itself (probe values: the
output is the probability matrix, compared entry by entry with float64 under a bound derived from the contract).  Inputs, bound
and their derivation: tests/attention_ref.py; that the bound catches the mistakes it is meant to catch: tests/test_attention_ref_api.py.

Two utterances, two heads of 64, at most 300 queries and 256 keys; K / V are views of packed [.., 2 d] rows; every (utterance,
head) has different data.

"Every schedule" means every schedule these three entries reach.  Two forms are launched by the deduplicated sampler loop alone and
have entries and tests of their own: the resident 32 x 32 x 16 pair with query segments (attn32_cross_hd64 SEG,
d3pm_op_attention_pair_segments) in tests/test_gpu_segment_ops.py, and the pipelined 32 x 32 x 16 self-attention with query segments
and its keys read through a row index (attn32p_hd64 SEG / GATHER, d3pm_op_attention_gather) in tests/test_gpu_attention_gather.py.
Both are compared bit for bit with the fixed-stride schedules pinned here, and tests/test_gpu_segment_ops.py runs the selector
inputs of this file through both."""
import pytest
import torch

import attention_ref as R
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H = 2, 2
D = H * R.HD
SCALE = 0.125
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]

# (name, family, tuning): single-problem schedules.  32 / 33 take the 32 x 32 x 16 kernel only for whole 128-query blocks and 64-key
# tiles ((128, 64) and (256, 192) below) and fall through to the 16 x 16 x 32 kernel elsewhere; nothing is asserted about which ran.
SINGLE = [("generic", 1, {})] + [(f"mfma_qg{g}", 2, {"attn_query_groups": g}) for g in (1, 2, 4, 32, 33)]
PAIR = [("tile_split_grid", {"attn_cross_resident": 0, "attn_pair_sequential": 0}),
        ("tile_sequential", {"attn_cross_resident": 0, "attn_pair_sequential": 2}),
        ("resident16", {"attn_cross_resident": 4}),
        ("resident32", {"attn_cross_resident": 5}),
        ("key_split", {"attn_query_groups": 4, "attn_cross_resident": 0})]
SINGLE_SHAPES = [(128, 64), (256, 192), (100, 65), (200, 130), (67, 127), (16, 1)]
PAIR_SHAPES = [(256, 64, 256), (300, 50, 225), (100, 1, 65), (130, 33, 129)]


@pytest.fixture(autouse=True)
def _default_tuning(built_lib):
    from vall_e.vall_e import _hip
    _hip.reset_tuning()
    yield
    _hip.reset_tuning()


class Packed:
    """K and V of one problem as views of packed [B, S, 2 d] device rows; V can be replaced between launches."""

    def __init__(self, k, v=None):
        self.kv = torch.zeros(k.shape[0], k.shape[1], 2 * k.shape[2], dtype=k.dtype, device=DEV)
        self.kv[..., :k.shape[2]] = k.to(DEV)
        self.d = k.shape[2]
        if v is not None:
            self.set_v(v)

    def set_v(self, v):
        self.kv[..., self.d:] = v.to(DEV)
        return self

    @property
    def k(self):
        return self.kv[..., :self.d]

    @property
    def v(self):
        return self.kv[..., self.d:]


def run_single(family, knobs, q, p, key_len=None):
    from vall_e.vall_e import _hip
    with _hip.tuning(**knobs):
        return _hip.op_attention(q, p.k, p.v, q.shape[2] // R.HD, SCALE, family=family, key_len=key_len)


def run_pair(knobs, q1, p1, q2, p2):
    from vall_e.vall_e import _hip
    with _hip.tuning(**knobs):
        return _hip.op_attention_pair(q1, p1.k, p1.v, q2, p2.k, p2.v, q1.shape[2] // R.HD, SCALE)


def _rand_v(Bn, S, dtype, seed, d=D):
    return torch.randn(Bn, S, d, generator=torch.Generator().manual_seed(seed)).to(dtype)


RATIOS = {}


def _note(test, schedule, dtype, rep):
    key = f"{test}/{schedule}/{IDS[DTYPES.index(dtype)] if dtype in DTYPES else 'f32'}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), rep.worst_ratio)
    REPORT.setdefault("attention_exact_error_over_bound", {})[key] = RATIOS[key]


def _print_ratios(test):
    for key in sorted(RATIOS):
        if key.startswith(test + "/"):
            print(f"[attention_exact] {key}: worst error / bound {RATIOS[key]:.3f}")


def _wrong_rows(o, want):
    bad = (o.cpu() != want).any(-1)
    return [(int(b), int(i)) for b, i in torch.nonzero(bad)[:6].tolist()]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_selector_returns_the_value_row_bit_for_bit(dtype):
    """Query i is K row pi(i) of +-4 sign codes: its own key leads by >= 2^40 in the log2 domain, the softmax is one-hot below fp32
    rounding and the row sum is exactly 1, so O[b, i, head h] must be V[b, pi(i), head h] unchanged on every schedule -- the
    partial states of the key-split kernel combine with weights 1 and <= 2^-69.  Where Tq < S a second pass with
    pi(i) = S - 1 - (i mod S) selects the tail keys."""
    failures = []
    for Tq, S in SINGLE_SHAPES:
        for reverse in ((False, True) if Tq < S else (False,)):
            q, k, pi, gap = R.selector_inputs(B, H, Tq, S, dtype, seed=Tq * 1000 + S, reverse=reverse)
            assert float(gap.min()) >= 40.0
            v = _rand_v(B, S, dtype, seed=S)
            want = v[:, pi]
            qd, p = q.to(DEV), Packed(k, v)
            for name, fam, knobs in SINGLE:
                o = run_single(fam, knobs, qd, p)
                if not torch.equal(o.cpu(), want):
                    failures.append(f"{name} Tq={Tq} S={S} reverse={reverse}: wrong (b, i) {_wrong_rows(o, want)}")
    for Tq, S1, S2 in PAIR_SHAPES:
        q1, k1, pi1, gap1 = R.selector_inputs(B, H, Tq, S1, dtype, seed=Tq * 1000 + S1)
        q2, k2, pi2, gap2 = R.selector_inputs(B, H, Tq, S2, dtype, seed=Tq * 1000 + S2 + 7)
        assert float(gap1.min()) >= 40.0 and float(gap2.min()) >= 40.0
        v1, v2 = _rand_v(B, S1, dtype, seed=S1 + 1), _rand_v(B, S2, dtype, seed=S2 + 2)
        p1, p2 = Packed(k1, v1), Packed(k2, v2)
        for name, knobs in PAIR:
            o1, o2 = run_pair(knobs, q1.to(DEV), p1, q2.to(DEV), p2)
            for side, o, want in (("text", o1, v1[:, pi1]), ("prompt", o2, v2[:, pi2])):
                if not torch.equal(o.cpu(), want):
                    failures.append(f"pair {name} {side} Tq={Tq} S={S1}/{S2}: wrong (b, i) {_wrong_rows(o, want)}")
    assert not failures, "\n".join(failures)


def _recover_single(fam, knobs, qd, p, S, dtype, key_len=None, Bn=B, Hn=H):
    return R.recover_probabilities(lambda v: run_single(fam, knobs, qd, p.set_v(v), key_len), Bn, S, Hn, dtype)


def _recover_pair(knobs, q1d, p1, S1, q2d, p2, S2, dtype):
    """Both probability matrices of a paired launch: max(blocks) launches, the shorter problem repeats its last block."""
    nb1, nb2 = R.n_blocks(S1), R.n_blocks(S2)
    c1, c2 = [], []
    for blk in range(max(nb1, nb2)):
        p1.set_v(R.probe_values(B, S1, H, min(blk, nb1 - 1), dtype))
        p2.set_v(R.probe_values(B, S2, H, min(blk, nb2 - 1), dtype))
        o1, o2 = run_pair(knobs, q1d, p1, q2d, p2)
        if blk < nb1:
            c1.append(R.heads(o1.cpu()))
        if blk < nb2:
            c2.append(R.heads(o2.cpu()))
    return torch.cat(c1, -1)[..., :S1], torch.cat(c2, -1)[..., :S2]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_recovered_probabilities_match_fp64(dtype):
    """Flat N(0, 0.7^2) inputs, V = one 64-key block of the identity per launch: ceil(S / 64) launches return the normalised
    probability every key had.  Each entry obeys the bound of attention_ref (a few per cent bf16, half a per cent fp16; a dropped
    or doubled key is 100 %), every entry is in the relative class, and each recovered row sums to 1 within S u."""
    failures = []
    for Tq, S in SINGLE_SHAPES:
        q, k = R.flat_inputs(B, H, Tq, S, dtype, seed=Tq * 1000 + S)
        ref, rel = R.softmax_fp64(q, k, SCALE), R.probability_bound(q, k, SCALE, dtype)
        qd, p = q.to(DEV), Packed(k)
        for name, fam, knobs in SINGLE:
            rep = R.check_probabilities(_recover_single(fam, knobs, qd, p, S, dtype), ref, rel, dtype)
            _note("flat", name, dtype, rep)
            if not (rep.ok and rep.frac_relative == 1.0):
                failures.append(f"{name} Tq={Tq} S={S}: {rep}")
    for Tq, S1, S2 in PAIR_SHAPES:
        q1, k1 = R.flat_inputs(B, H, Tq, S1, dtype, seed=Tq * 1000 + S1)
        q2, k2 = R.flat_inputs(B, H, Tq, S2, dtype, seed=Tq * 1000 + S2 + 7)
        refs = [(R.softmax_fp64(q, k, SCALE), R.probability_bound(q, k, SCALE, dtype)) for q, k in ((q1, k1), (q2, k2))]
        p1, p2 = Packed(k1), Packed(k2)
        for name, knobs in PAIR:
            got = _recover_pair(knobs, q1.to(DEV), p1, S1, q2.to(DEV), p2, S2, dtype)
            for side, ph, (ref, rel) in zip(("text", "prompt"), got, refs):
                rep = R.check_probabilities(ph, ref, rel, dtype)
                _note("flat", "pair_" + name, dtype, rep)
                if not (rep.ok and rep.frac_relative == 1.0):
                    failures.append(f"pair {name} {side} Tq={Tq} S={S1}/{S2}: {rep}")
    _print_ratios("flat")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_score_ranges(family, dtype):
    """Scores steered tile by tile (attention_ref.FAMILIES): all strongly negative (the first-tile reference is negative), falling
    (the "no raise" branch), rising by 2^7.5 (under the deferral of 2^8) and by 2^8.5 (over it: the rescale), and up then down.
    S = 256 and the ragged 200, Tq = 128; the single problem on every schedule and the prompt side of a pair (50 flat text keys)
    on every pair schedule.  Probabilities recovered and bounded as in the flat test; outputs finite."""
    failures = []
    Tq = 128
    for S in (256, 200):
        q, k, off = R.steered_inputs(family, B, H, Tq, S, dtype, seed=S + len(family))
        assert R.steps_on_intended_side(family, off), off
        ref, rel = R.softmax_fp64(q, k, SCALE), R.probability_bound(q, k, SCALE, dtype)
        qd, p = q.to(DEV), Packed(k)
        for name, fam, knobs in SINGLE:
            ph = _recover_single(fam, knobs, qd, p, S, dtype)
            rep = R.check_probabilities(ph, ref, rel, dtype)
            _note("ranges", name, dtype, rep)
            if not (rep.ok and bool(torch.isfinite(ph).all())):
                failures.append(f"{name} {family} S={S}: {rep}")
        q1, k1 = R.flat_inputs(B, H, Tq, 50, dtype, seed=S)
        ref1, rel1 = R.softmax_fp64(q1, k1, SCALE), R.probability_bound(q1, k1, SCALE, dtype)
        p1 = Packed(k1)
        for name, knobs in PAIR:
            ph1, ph2 = _recover_pair(knobs, q1.to(DEV), p1, 50, qd, p, S, dtype)
            for side, ph, rf, rl in (("text", ph1, ref1, rel1), ("prompt", ph2, ref, rel)):
                rep = R.check_probabilities(ph, rf, rl, dtype)
                _note("ranges", "pair_" + name, dtype, rep)
                if not (rep.ok and bool(torch.isfinite(ph).all())):
                    failures.append(f"pair {name} {side} {family} S={S}: {rep}")
    _print_ratios("ranges")
    assert not failures, "\n".join(failures)


KEY_LENS = [(130, [1, 64, 65, 130]), (256, [63, 128, 129, 256])]


@pytest.mark.parametrize("S_pad,lens", KEY_LENS, ids=["pad130", "pad256"])
def test_key_len_equals_the_truncated_problem(S_pad, lens):
    """d3pm_op_attention_keylen: four utterances with different numbers of valid keys in one padded batch.  The rows at and past
    key_len[b] hold large finite poison (K = 240: the masked scores would be the largest by far; V = 3e4) -- the contract masks
    them, it does not promise that they are not read, hence no NaN.  For the generic family (f32, f16, bf16) and the MFMA family
    with attn_query_groups 1 and 2, utterance b of the masked launch equals bit for bit the same schedule on that utterance alone
    with S = key_len[b] and no mask (the tile walk is the same), and the recovered probabilities obey the bound against
    softmax_fp64(.., key_len).  attn_query_groups 4, 32 and 33 name kernels that refuse a mask (their *_supported say so):
    mfma_attention then FALLS BACK to its automatic choice between one and two query groups -- one at this grid -- so their masked
    result must equal the attn_query_groups = 1 result bit for bit; none returns D3PM_E_SHAPE."""
    Bn, Tq = 4, 72
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    failures = []
    cases = [("generic", 1, {}, dt) for dt in (torch.float32, torch.float16, torch.bfloat16)]
    cases += [(f"mfma_qg{g}", 2, {"attn_query_groups": g}, dt) for g in (1, 2) for dt in DTYPES]
    masked_qg1 = {}
    for name, fam, knobs, dtype in cases:
        q, k = R.flat_inputs(Bn, H, Tq, S_pad, dtype, seed=S_pad)
        v = _rand_v(Bn, S_pad, dtype, seed=S_pad + 1)
        kp, vp = k.clone(), v.clone()
        for b, n in enumerate(lens):
            kp[b, n:] = 240.0
            vp[b, n:] = 3e4
        qd, p = q.to(DEV), Packed(kp, vp)
        o = run_single(fam, knobs, qd, p, kl)
        if name == "mfma_qg1":
            masked_qg1[dtype] = (qd, p, o.clone())
        if not bool(torch.isfinite(o).all()):
            failures.append(f"{name} {dtype}: non-finite output")
        for b, n in enumerate(lens):
            alone = run_single(fam, knobs, qd[b:b + 1].contiguous(), Packed(k[b:b + 1, :n].contiguous(), v[b:b + 1, :n].contiguous()))
            if not torch.equal(o[b:b + 1], alone):
                failures.append(f"{name} {dtype} utterance {b} (key_len {n}): differs from the truncated problem at (b, i) "
                                f"{_wrong_rows(o[b:b + 1], alone.cpu())}")
        ref, rel = R.softmax_fp64(q, kp, SCALE, lens), R.probability_bound(q, kp, SCALE, dtype, lens)
        rep = R.check_probabilities(_recover_single(fam, knobs, qd, p, S_pad, dtype, kl, Bn=Bn), ref, rel, dtype)
        _note("key_len", name, dtype, rep)
        if not rep.ok:
            failures.append(f"{name} {dtype}: {rep}")
        p.set_v(vp)
    for dtype in DTYPES:
        qd, p, o1 = masked_qg1[dtype]
        for g in (4, 32, 33):
            o = run_single(2, {"attn_query_groups": g}, qd, p, kl)
            if not torch.equal(o, o1):
                failures.append(f"mfma_qg{g} {dtype}: the fallback under a mask differs from attn_query_groups = 1")
    _print_ratios("key_len")
    assert not failures, "\n".join(failures)


def test_key_len_argument_is_validated_on_the_host():
    from vall_e.vall_e import _hip
    q, k = R.flat_inputs(B, H, 16, 65, torch.float16, seed=1)
    p = Packed(k, _rand_v(B, 65, torch.float16, seed=2))
    for bad in (torch.ones(B, dtype=torch.int64, device=DEV), torch.ones(B + 1, dtype=torch.int32, device=DEV), torch.ones(B, dtype=torch.int32)):
        with pytest.raises(_hip.D3PMError, match="key_len"):
            _hip.op_attention(q.to(DEV), p.k, p.v, H, SCALE, key_len=bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_sequential_equals_split_grid(dtype):
    """attn_mfma_hd64<.., PAIR = true> (attn_pair_sequential = 2: one workgroup runs the text problem and then the prompt problem)
    against the split grid (0), attn_cross_resident = 0, one and two query groups: the code and the order per workgroup are the
    same, so both outputs must be the same bits."""
    failures = []
    for Tq, S1, S2 in PAIR_SHAPES:
        q1, k1 = R.flat_inputs(B, H, Tq, S1, dtype, seed=Tq + S1)
        q2, k2 = R.flat_inputs(B, H, Tq, S2, dtype, seed=Tq + S2 + 7)
        p1, p2 = Packed(k1, _rand_v(B, S1, dtype, seed=1)), Packed(k2, _rand_v(B, S2, dtype, seed=2))
        for g in (1, 2):
            outs = [run_pair({"attn_cross_resident": 0, "attn_query_groups": g, "attn_pair_sequential": seq}, q1.to(DEV), p1, q2.to(DEV), p2)
                    for seq in (0, 2)]
            for side, a, b in (("text", outs[0][0], outs[1][0]), ("prompt", outs[0][1], outs[1][1])):
                if not torch.equal(a, b):
                    failures.append(f"qg{g} {side} Tq={Tq} S={S1}/{S2}: differs at (b, i) {_wrong_rows(a, b.cpu())}")
    assert not failures, "\n".join(failures)

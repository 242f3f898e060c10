"""The block-scaled fp8 path (csrc/d3pm_mx.hip, csrc/d3pm_mx.h) bit for bit: quantisers, GEMM, MX-output epilogue.

Everything is compared on 100 % of the elements with tests/mx_ref.py, a host definition of the format that shares no code with the
kernels or with the package's torch quantiser (tests/test_mx_ref.py holds the two hosts together without a GPU).  The GEMM operands
are dyadic: products of e4m3 codes and power-of-two scales on one quantum, every partial sum below 2^22 quanta, so the fp32
accumulator of any tile walk holds the exact sum and what is stored is decided by the epilogue alone -- the 16-bit rounding chain
of tests/gemm_exact_ref.py, or for the MX output the quantiser's rule on v = acc + bias.  Every output and operand lies in a
storage prefilled with a NaN pattern (0xA5 for bytes), with guard bands on either side; the guards are compared after every call
and the operands with their snapshots.  A stray store stays inside the allocation; nothing here provokes a fault.

inf and NaN inputs of the quantisers are not defined by include/d3pm_hip.h and are left out."""
import pytest
import torch

import gemm_exact_ref as R
import mx_ref as X
from test_gpu_gemm_edges import _check_sweep, _gelu64, gelu_delta
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
VARIANTS = [("auto", 0), ("v6", 6), ("v8", 8)]
EPILOGUES = ("bias", "nobias", "r1", "r1mask", "r1mask_inplace")
WITH_R1 = ("r1", "r1mask", "r1mask_inplace")
GEMM_CASES = [(s, True) for s in X.GEMM_SHAPES] + [(X.TIGHT_SHAPE, False)]
U8 = torch.uint8


def _name(dtype):
    return IDS[DTYPES.index(dtype)]


def _shape_id(c):
    return "x".join(map(str, c))


def _case_id(c):
    return f"{_shape_id(c[0])}-{'padded' if c[1] else 'tight'}"


@pytest.fixture(autouse=True)
def _default_tuning(built_lib):
    from vall_e.vall_e import _hip
    _hip.reset_tuning()
    yield
    _hip.reset_tuning()


def _runs(M, N, K):
    """the schedules that admit the shape: gemm_variant 0 always, 6 / 8 where the shape is made of their whole tiles"""
    return [(n, v) for n, v in VARIANTS if v == 0 or X.mx_tile(M, N, K, v)]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _codes(rows, cols, ld=None, fill=None):
    return R.guarded(rows, cols, cols if ld is None else ld, U8, device=DEV, fill=fill)


def _scales(rows, K, fill=None):
    return R.guarded_flat((rows, 4, K // 128), U8, device=DEV, fill=fill)


def _same_storage(a, b):
    return torch.equal(a, b) if a.dtype == U8 else torch.equal(a.view(torch.int16), b.view(torch.int16))


def _differ(got, exp, what, shape_of="codes"):
    wrong = got.cpu() != exp
    if not wrong.any():
        return None
    at = tuple(wrong.nonzero()[0].tolist())
    return f"{what}: {int(wrong.sum())} of {wrong.numel()} {shape_of} differ, first at {list(at)}: {int(got.cpu()[at]):#04x} for {int(exp[at]):#04x}"


# ---- the quantiser ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M", X.QUANT_M)
@pytest.mark.parametrize("K", X.QUANT_K)
def test_quantize_mx_equals_the_format_and_writes_nothing_but_its_rows(built_lib, dtype, M, K):
    """d3pm_op_quantize_mx with ldx = K and ldx = K + 8: codes and scale bytes of every block equal mx_ref -- blocks of very different
    magnitude and the planted ones (all-zero row and block, -0, maxima 1.75 2^E and 1.8125 2^E, the ties 17 / 19 beside 32, the largest
    finite value, f16 subnormals, bf16 blocks below 2^-126 whose scale is clamped at byte 1).  K = 128 and 384 have one short piece,
    K = 640 and 1152 a whole and a short one (the `live` lanes); M = 1 and 5 leave waves of the last workgroup without a row."""
    from vall_e.vall_e import _hip
    xc = X.quantiser_operand(M, K, dtype, 7 * K + M)
    ec, es = X.quantize(xc)
    assert int((ec & 0x7F).max()) <= 0x7E
    for ldx in (K, K + 8):
        what = f"quantize {M}x{K} ldx {ldx} {_name(dtype)}"
        xs, x = R.guarded(M, K, ldx, dtype, device=DEV, fill=xc)
        snap = xs.clone()
        cs, c = _codes(M, K)
        ss, s = _scales(M, K)
        gc, gs = _hip.op_quantize_mx(x, out=(c, s))
        assert gc.data_ptr() == c.data_ptr() and gs.data_ptr() == s.data_ptr()
        problems = [p for p in (_differ(s, es, what, "scale bytes"), _differ(c, ec, what)) if p]
        assert not problems, "\n".join(problems)
        assert int((c & 0x7F).max()) <= 0x7E, f"{what}: the NaN code 0x7F"
        R.assert_untouched(cs, c, what + " codes")
        R.assert_untouched(ss, s, what + " scales")
        assert _same_storage(xs, snap), f"{what}: x was written"
    n8, ns = _hip.op_quantize_mx(xc.to(DEV))                  # the allocating form existing callers use
    assert torch.equal(n8.cpu(), ec) and torch.equal(ns.cpu(), es)


# ---- LayerNorm -> MX ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M", X.LN_M)
def test_layernorm_mx_is_mx_ref_of_the_16_bit_layernorm(built_lib, dtype, M):
    """d3pm_op_layernorm_mx and the two-output d3pm_op_layernorm_mx_pair (the sampler's norm2 | norm22 launch), with and without FiLM:
    each output is mx_ref of d3pm_op_layernorm's 16-bit rows (that op has its own tests).  M = 1, 5, 37 and 1023 are 1, 2, 10 and 256
    workgroups of four rows: fewer than the eight XCDs, a remainder of 2 workgroups, a whole multiple with a ragged last workgroup
    (the `row >= M` exit) -- every arm of the XCD remap."""
    from vall_e.vall_e import _hip
    d = 512
    g = torch.Generator().manual_seed(100 + M)
    xc = (torch.randn(M, d, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).to(dtype)
    xc[M // 2] = 0                                                      # a masked frame: LN(0) = bias
    xs, x = R.guarded(M, d, d, dtype, device=DEV, fill=xc)
    vec = lambda scale, shift, n=d: (shift + scale * torch.randn(n, generator=g)).to(dtype).to(DEV)      # noqa: E731
    w, b, w2, b2, film = vec(0.1, 1.0), vec(0.1, 0.0), vec(0.3, 1.0), vec(0.5, 0.0), vec(0.2, 0.0, 2 * d)
    snap = xs.clone()
    for fl in (None, film):
        what = f"layernorm_mx M {M} {_name(dtype)} film {fl is not None}"
        e1 = X.quantize(_hip.op_layernorm(x, w, b, film=fl).cpu())
        e2 = X.quantize(_hip.op_layernorm(x, w2, b2).cpu())
        outs = [_codes(M, d) + _scales(M, d) for _ in range(3)]      # (code storage, codes, scale storage, scales)
        _hip.op_layernorm_mx(x, w, b, film=fl, out=(outs[0][1], outs[0][3]))
        _hip.op_layernorm_mx_pair(x, w, b, w2, b2, film=fl, out=(outs[1][1], outs[1][3]), out2=(outs[2][1], outs[2][3]))
        problems = []
        for (cs, c, ss, s), (ec, es), tag in zip(outs, (e1, e1, e2), ("one output", "pair, first", "pair, second")):
            problems += [p for p in (_differ(s, es, f"{what} {tag}", "scale bytes"), _differ(c, ec, f"{what} {tag}")) if p]
            R.assert_untouched(cs, c, f"{what} {tag} codes")
            R.assert_untouched(ss, s, f"{what} {tag} scales")
        assert not problems, "\n".join(problems)
        assert _same_storage(xs, snap), f"{what}: x was written"


# ---- the GEMM -----------------------------------------------------------------------------------------------------------------------------
_CPU = {}


def _mask():
    return (torch.arange(X.MASK_PERIOD) % 3 != 1).to(U8)


def _operands(M, N, K):
    key = (M, N, K)
    if key not in _CPU:
        _CPU[key] = dict(X.dyadic_mx_operands(M, N, K, M + N + K), mask=_mask(), expected={})
    return _CPU[key]


def _expected16(o, dtype, epi):
    key = (dtype, "r1mask" if epi == "r1mask_inplace" else epi)
    if key not in o["expected"]:
        o["expected"][key] = X.expected_16bit(o["x"], o["w"], None if epi == "nobias" else o["bias"], dtype, r1=o["r1"] if epi in WITH_R1 else None,
                                              row_mask=o["mask"] if epi.startswith("r1mask") else None, mask_period=X.MASK_PERIOD)
    return o["expected"][key]


class Inputs:
    """The operands of one case in guarded device storages, with a snapshot of every storage."""

    def __init__(self, o, dtype, ldx, ldr, x8=None, sx=None, bias=None):
        M, K = o["x8"].shape
        N = o["w8"].shape[0]
        self.store = {}
        self.store["x8"], self.x8 = _codes(M, K, ldx, fill=o["x8"] if x8 is None else x8)
        self.store["sx"], self.sx = _scales(M, K, fill=o["sx"] if sx is None else sx)
        self.store["w8"], self.w8 = _codes(N, K, fill=o["w8"])
        self.store["sw"], self.sw = _scales(N, K, fill=o["sw"])
        self.store["bias"], self.bias = R.guarded_flat((N,), dtype, device=DEV, fill=(o["bias"] if bias is None else bias).to(dtype))
        self.store["r1"], self.r1 = R.guarded(M, N, ldr, dtype, device=DEV, fill=o["r1"].to(dtype))
        self.store["mask"], self.mask = R.guarded_flat((X.MASK_PERIOD,), U8, device=DEV, fill=o["mask"])
        self.snap = {k: v.clone() for k, v in self.store.items()}

    def assert_unchanged(self, what):
        for k, v in self.store.items():
            assert _same_storage(v, self.snap[k]), f"{what}: the operand {k} (or its guard) was written"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", GEMM_CASES, ids=_case_id)
def test_linear_mx_16_bit_output_is_the_rounding_chain(built_lib, dtype, case):
    """gemm_mx_big<.., OUT8 = false> -- epilogue_store<T, EPI, 4, 6, true, false, true> -- under gemm_variant 0, 6 and 8, with
    ldx = K + 16, ldy = N + 8, ldr = N + 16 (one shape also tight), epilogues bias / nobias / r1 / r1mask and r1mask in place
    (Y == R1: the only form the sampler launches for fc2): every stored element equals epilogue_chain of the de-quantised operands,
    the guards of Y and every operand are untouched."""
    from vall_e.vall_e import _hip
    (M, N, K), padded = case
    ldx, ldy, ldr = (K + 16, N + 8, N + 16) if padded else (K, N, N)
    o = _operands(M, N, K)
    inp = Inputs(o, dtype, ldx, ldr)
    problems = []
    for epi in EPILOGUES:
        exp = _bits(_expected16(o, dtype, epi)).to(DEV)
        for name, variant in _runs(M, N, K):
            what = f"{_case_id(case)} {_name(dtype)} {epi} {name}"
            if epi == "r1mask_inplace":
                ys, y = R.guarded(M, N, ldr, dtype, device=DEV, fill=o["r1"].to(dtype))
            else:
                ys, y = R.guarded(M, N, ldy, dtype, device=DEV)
            r1 = None if epi not in WITH_R1 else y if epi == "r1mask_inplace" else inp.r1
            with _hip.tuning(gemm_variant=variant):
                got = _hip.op_linear_mx(inp.x8, inp.sx, inp.w8, inp.sw, None if epi == "nobias" else inp.bias, dtype, r1=r1,
                                        row_mask=inp.mask if epi.startswith("r1mask") else None, mask_period=X.MASK_PERIOD, out=y, ldy=y.stride(0))
            assert got.data_ptr() == y.data_ptr() and got.shape == (M, N)
            wrong = _bits(got) != exp
            if wrong.any():      # every epilogue and schedule runs before the test fails
                at = tuple(wrong.nonzero()[0].tolist())
                problems.append(f"{what}: {int(wrong.sum())} of {M * N} elements differ from the rounding chain, first at {list(at)}: "
                                f"{got[at].item()!r} for {_expected16(o, dtype, epi)[at].item()!r}")
            R.assert_untouched(ys, y, what)
            inp.assert_unchanged(what)
    assert not problems, "\n".join(problems)
    assert _hip.TUNING.gemm_variant == 0


# bias blocks of the MX-output test, all on the product quantum 2^-4: under an all-zero row of X they are the row the epilogue quantises
def _planted_bias(N, base):
    small = [0.0625] * 31
    blocks = [[0.0] * 32, [-0.0] * 32, [-0.0, 1.0, -0.0, -3.0] * 8]
    for E in (0, 5):
        blocks += [[1.75 * 2.0 ** E] + small, small + [-1.75 * 2.0 ** E], [1.8125 * 2.0 ** E] + small,
                   [17 * 2.0 ** E, 19 * 2.0 ** E, 32 * 2.0 ** E, -17 * 2.0 ** E, -19 * 2.0 ** E] + [2.0 ** E] * 27]
    bias = base.clone()
    for i, blk in enumerate(blocks[:N // 32]):
        bias[32 * i:32 * i + 32] = torch.tensor(blk, dtype=torch.float64)
    assert torch.equal((bias / X.QUANTUM).round() * X.QUANTUM, bias) and float(bias.abs().max()) <= 1024
    return bias


def _mx_out_case(M, N, K):
    """operands of the MX-output tests: the dyadic ones with rows 5 and M - 1 of X zeroed and the planted blocks in the bias"""
    key = ("mx", M, N, K)
    if key not in _CPU:
        o = _operands(M, N, K)
        x = o["x"].clone()
        x[[5, M - 1]] = 0
        x8, sx = X.quantize(x)
        bias = _planted_bias(N, o["bias"])
        assert (o["bound"] + 1024 / X.QUANTUM) < X.EXACT_QUANTA
        _CPU[key] = dict(x=x, x8=x8, sx=sx, bias=bias, with_bias=X.expected_mx(x, o["w"], bias), without=X.expected_mx(x, o["w"], None))
    return _CPU[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", X.GEMM_SHAPES, ids=_shape_id)
def test_linear_mx_output_equals_mx_ref_on_every_code_and_scale(built_lib, dtype, shape):
    """gemm_mx_big<.., OUT8 = true> without activation: v = acc + bias is exact in fp32, so codes AND scale bytes equal mx_ref of v on
    every element (mx_block_quantise, mx_store_row64, the SY store).  Rows 5 and M - 1 of X are all zero: there v is the bias, which
    carries the boundary (1.75 2^E, 1.8125 2^E), tie, all-zero and -0 blocks.  With and without bias, under every schedule."""
    from vall_e.vall_e import _hip
    M, N, K = shape
    o, c = _operands(M, N, K), _mx_out_case(M, N, K)
    inp = Inputs(o, dtype, K + 16, N, x8=c["x8"], sx=c["sx"], bias=c["bias"])
    assert torch.equal(inp.bias.cpu().double(), c["bias"])
    problems = []
    for tag, bias, (ec, es) in (("bias", inp.bias, c["with_bias"]), ("nobias", None, c["without"])):
        for name, variant in _runs(M, N, K):
            what = f"mx out {_shape_id(shape)} {_name(dtype)} {tag} {name}"
            cs, y8 = _codes(M, N)
            ss, sy = _scales(M, N)
            with _hip.tuning(gemm_variant=variant):
                g8, gs = _hip.op_linear_mx(inp.x8, inp.sx, inp.w8, inp.sw, bias, dtype, out8=y8, out_scales=sy)
            assert g8.data_ptr() == y8.data_ptr() and gs.data_ptr() == sy.data_ptr()
            problems += [p for p in (_differ(sy, es, what, "scale bytes"), _differ(y8, ec, what)) if p]
            assert int((y8 & 0x7F).max()) <= 0x7E, f"{what}: the NaN code 0x7F"
            R.assert_untouched(cs, y8, what + " codes")
            R.assert_untouched(ss, sy, what + " scales")
            inp.assert_unchanged(what)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [s for s in X.GEMM_SHAPES if s[1] % 512 == 0], ids=_shape_id)
def test_the_mx_output_is_the_operand_the_next_gemm_reads(built_lib, dtype, shape):
    """The consumer's view of (Y8, SY): the kernel's own MX output is the X of a second d3pm_op_linear_mx (K = N, as fc1 -> fc2).
    Its weight rows are one-hot -- output column n reads element (m, k_n) of Y alone, every other product is an exact zero -- so the
    result is exact whatever Y holds, and must equal the chain evaluated on mx_ref's codes and scales: a block scale stored one slot
    off changes the power of two of the elements it serves.  The picked columns visit every 32-block of Y."""
    from vall_e.vall_e import _hip
    M, N, K = shape
    o, c = _operands(M, N, K), _mx_out_case(M, N, K)
    N2, per = 128, N // 128
    g = torch.Generator().manual_seed(N)
    w2 = torch.zeros(N2, N, dtype=torch.float64)
    cols = torch.arange(N2) * per + torch.randint(0, per, (N2,), generator=g)
    w2[torch.arange(N2), cols] = (torch.randint(1, 5, (N2,), generator=g) * (torch.randint(0, 2, (N2,), generator=g) * 2 - 1)).double() \
        * torch.exp2(torch.randint(-2, 1, (N2,), generator=g).double())
    assert set((cols // 32).tolist()) == set(range(N // 32))
    w28, sw2 = X.quantize(w2)
    assert torch.equal(X.dequantize(w28, sw2), w2)
    y_ref = X.dequantize(*c["with_bias"])
    exp = _bits(R.epilogue_chain(y_ref, w2, None, dtype))
    inp = Inputs(o, dtype, K + 16, N, x8=c["x8"], sx=c["sx"], bias=c["bias"])
    w2s, w2d = _codes(N2, N, fill=w28)
    s2s, s2d = _scales(N2, N, fill=sw2)
    for name, variant in _runs(M, N, K):
        what = f"chain {_shape_id(shape)} {_name(dtype)} {name}"
        cs, y8 = _codes(M, N)
        ss, sy = _scales(M, N)
        zs, z = R.guarded(M, N2, N2 + 8, dtype, device=DEV)
        with _hip.tuning(gemm_variant=variant):
            _hip.op_linear_mx(inp.x8, inp.sx, inp.w8, inp.sw, inp.bias, dtype, out8=y8, out_scales=sy)
        snap8, snaps = cs.clone(), ss.clone()
        got = _hip.op_linear_mx(y8, sy, w2d, s2d, None, dtype, out=z, ldy=z.stride(0))      # 192 x 128 tiles (N2 = 128)
        wrong = _bits(got.cpu()) != exp
        assert not wrong.any(), f"{what}: {int(wrong.sum())} of {M * N2} elements differ, first at {wrong.nonzero()[0].tolist()}"
        R.assert_untouched(zs, z, what)
        assert torch.equal(cs, snap8) and torch.equal(ss, snaps), f"{what}: the consumer wrote its X"
        inp.assert_unchanged(what)


# ---- GELU ----------------------------------------------------------------------------------------------------------------------------------
SWEEP_M, SWEEP_K = 192, 512


def _gelu_run(dtype, variant, mx_out):
    """all-zero X and W, bias = the sweep: the pre-activation of column n of every row is bias[n] exactly"""
    from vall_e.vall_e import _hip
    bias, N = X.gelu_sweep_bias(dtype)
    x8 = torch.zeros(SWEEP_M, SWEEP_K, dtype=U8, device=DEV)
    sx = torch.ones(SWEEP_M, 4, SWEEP_K // 128, dtype=U8, device=DEV)
    w8 = torch.zeros(N, SWEEP_K, dtype=U8, device=DEV)
    sw = torch.full((N, 4, SWEEP_K // 128), 127, dtype=U8, device=DEV)
    bs, b = R.guarded_flat((N,), dtype, device=DEV, fill=bias)
    what = f"gelu sweep {_name(dtype)} v{variant} {'mx' if mx_out else '16-bit'}"
    with _hip.tuning(gemm_variant=variant):
        if mx_out:
            cs, y8 = _codes(SWEEP_M, N)
            ss, sy = _scales(SWEEP_M, N)
            _hip.op_linear_mx(x8, sx, w8, sw, b, dtype, act=1, out8=y8, out_scales=sy)
            R.assert_untouched(cs, y8, what + " codes")
            R.assert_untouched(ss, sy, what + " scales")
            assert bool((y8 == y8[:1]).all()) and bool((sy == sy[:1]).all()), f"{what}: the rows differ"
            out = (y8[:1].cpu(), sy[:1].cpu())
        else:
            ys, y = R.guarded(SWEEP_M, N, N + 8, dtype, device=DEV)
            _hip.op_linear_mx(x8, sx, w8, sw, b, dtype, act=1, out=y, ldy=y.stride(0))
            R.assert_untouched(ys, y, what)
            assert bool((_bits(y) == _bits(y[:1])).all()), f"{what}: the rows differ"
            out = y[:1].cpu()
    R.assert_untouched(bs, b, what + " bias")
    return bias, out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", [6, 8])
def test_mx_output_gelu_of_every_16_bit_value(built_lib, dtype, variant):
    """The MX-output epilogue with GELU on every finite 16-bit pre-activation in [-8, 8] (31 values of the sweep and an anchor per
    block: no block maximum within SWEEP_MARGIN of a scale boundary, asserted on the CPU by tests/test_mx_ref.py and again here).
    Reference: the float64 value g of the TANH form the source states (mx_ref.gelu_tanh64), not erf.  The scale bytes equal mx_ref's
    of g on every block; every code lies between rn_e4m3((g - delta) / s) and rn_e4m3((g + delta) / s) with delta of
    mx_ref.gelu_tanh_delta (derived from the fp32 operations and the 1-ulp accuracy of v_exp_f32 / v_rcp_f32), and equals the
    code where the two ends agree.  REPORT receives how many codes differ from plain rn_e4m3(g / s) and by how many code steps."""
    bias, (y8, sy) = _gelu_run(dtype, variant, True)
    v = bias.double()[None, :]
    g = X.gelu_tanh64(v)
    delta = X.gelu_tanh_delta(v, g)
    gm = g.abs().view(-1, 32).amax(dim=1)
    assert bool((X.boundary_distance(gm) > X.SWEEP_MARGIN).all())
    es = X.scale_bytes(gm)
    gs = sy.permute(0, 2, 1).reshape(-1)
    assert torch.equal(gs, es), f"{int((gs != es).sum())} of {es.numel()} scale bytes differ, first at block {(gs != es).nonzero()[0].item()}"
    s = torch.exp2(es.double() - 127).repeat_interleave(32)[None, :]
    lo_c, hi_c = X.codes_of(((g - delta) / s).clamp(-448, 448)), X.codes_of(((g + delta) / s).clamp(-448, 448))
    plain = X.codes_of(g / s)
    assert int((y8 & 0x7F).max()) <= 0x7E, "the NaN code 0x7F"
    got, lo, hi = X.values_of(y8), X.values_of(lo_c), X.values_of(hi_c)
    order = lambda c: torch.where(c >= 0x80, -(c.long() & 0x7F), c.long())      # noqa: E731   (code steps; -0 and +0 coincide)
    steps = (order(y8) - order(plain)).abs()
    REPORT[f"mx_gelu_sweep_{_name(dtype)}_v{variant}"] = {"elements": y8.numel(), "codes_off_rn_e4m3_of_exact": int((steps != 0).sum()),
                                                          "max_code_steps_from_rn_e4m3_of_exact": int(steps.max()),
                                                          "codes_where_the_bound_admits_two": int((lo_c != hi_c).sum())}
    print(f"mx gelu sweep {_name(dtype)} v{variant}: {REPORT[f'mx_gelu_sweep_{_name(dtype)}_v{variant}']}")
    bad = ~((got >= lo) & (got <= hi)) | ((lo_c == hi_c) & (y8 != lo_c))
    assert not bad.any(), (f"{int(bad.sum())} of {bad.numel()} codes lie outside the bound; the first pre-activations: {v[bad][:8].tolist()} gave "
                           f"{[hex(int(t)) for t in y8[bad][:8]]} for {[hex(int(t)) for t in plain[bad][:8]]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", [6, 8])
def test_mx_gemm_16_bit_gelu_of_every_16_bit_value(built_lib, dtype, variant):
    """The 16-bit GELU epilogue of the MX kernel (exact-erf form, as the 16-bit GEMMs): gelu_delta and _check_sweep of
    tests/test_gpu_gemm_edges.py as they are."""
    bias, y = _gelu_run(dtype, variant, False)
    pre = bias.double()[None, :]
    g = _gelu64(pre)
    _check_sweep(dtype, "gelu", pre, y, g, gelu_delta(pre, g), f"mx_v{variant}")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_linear_mx_refuses_what_it_cannot_run_and_writes_nothing(built_lib):
    """Every refusal of mx_linear_supported returns D3PMError before a launch: all buffers live in one arena whose bytes are compared
    afterwards.  The overlap cases place an output ON an input inside that arena (nothing could leave it even if a launch happened)."""
    from vall_e.vall_e import _hip
    dtype = torch.bfloat16
    M, N, K = 192, 256, 512
    arena = torch.full((1 << 22,), 0xA5, dtype=U8, device=DEV)
    cursor = [4096]

    def take(nbytes):
        at = cursor[0]
        cursor[0] = (at + nbytes + 4096 + 255) // 256 * 256
        assert cursor[0] <= arena.numel()
        return arena[at:at + nbytes]
    b8 = lambda r, c, ld=None: take(r * (ld or c)).view(r, ld or c)[:, :c]                      # noqa: E731
    b16 = lambda r, c, ld=None: take(2 * r * (ld or c)).view(dtype).view(r, ld or c)[:, :c]      # noqa: E731
    sc = lambda r, k: take(r * (k // 32)).view(r, 4, k // 128)                                  # noqa: E731
    x8, sx, w8, sw = b8(M, K), sc(M, K), b8(N, K), sc(N, K)
    bias, r1, mask = take(2 * N).view(dtype), b16(M, N), take(7)
    y, y8, sy = b16(M, N), b8(M, N), sc(M, N)
    run = _hip.op_linear_mx
    cases = {
        "K = 256": lambda: run(b8(M, 256), sc(M, 256), b8(N, 256), sc(N, 256), bias, dtype, out=y),
        "N = 192": lambda: run(x8, sx, b8(192, K), sc(192, K), bias[:192], dtype, out=b16(M, 192, 200), ldy=200),
        "M = 100": lambda: run(x8[:100], sx[:100], w8, sw, bias, dtype, out=y),
        "ldx % 16": lambda: run(b8(M, K, K + 8), sx, w8, sw, bias, dtype, out=y),
        "ldy % 8": lambda: run(x8, sx, w8, sw, bias, dtype, out=b16(M, N, N + 4), ldy=N + 4),
        "ldr % 8": lambda: run(x8, sx, w8, sw, bias, dtype, out=y, r1=b16(M, N, N + 4)),
        "GELU with R1": lambda: run(x8, sx, w8, sw, bias, dtype, act=1, r1=r1, out=y),
        "a mask without R1": lambda: run(x8, sx, w8, sw, bias, dtype, row_mask=mask, mask_period=7, out=y),
        "MX output with R1": lambda: run(x8, sx, w8, sw, bias, dtype, r1=r1, out8=y8, out_scales=sy),
        "MX output with a mask": lambda: run(x8, sx, w8, sw, bias, dtype, row_mask=mask, mask_period=7, out8=y8, out_scales=sy),
        "Y8 without SY": lambda: run(x8, sx, w8, sw, bias, dtype, out8=y8),
        "fp32 output": lambda: run(x8, sx, w8, sw, None, torch.float32, out=take(4 * M * N).view(torch.float32).view(M, N)),
        "an activation other than GELU": lambda: run(x8, sx, w8, sw, bias, dtype, act=2, out=y),
    }
    # each output on each input: the output starts 256 bytes into the input (or at its start where it is shorter), 16-byte aligned
    def on(t, nbytes):
        off = t.data_ptr() - arena.data_ptr() + (256 if t.numel() > 256 else 0)
        assert off + nbytes + 4096 <= arena.numel()
        return arena[off:off + nbytes]
    for iname, t in (("X8", x8), ("SX", sx), ("W8", w8), ("SW", sw)):
        cases[f"Y on {iname}"] = lambda t=t: run(x8, sx, w8, sw, bias, dtype, out=on(t, 2 * M * N).view(dtype).view(M, N))
        cases[f"Y8 on {iname}"] = lambda t=t: run(x8, sx, w8, sw, bias, dtype, out8=on(t, M * N).view(M, N), out_scales=sy)
        cases[f"SY on {iname}"] = lambda t=t: run(x8, sx, w8, sw, bias, dtype, out8=y8, out_scales=on(t, M * (N // 32)).view(M, 4, N // 128))
    # one byte in common: the last byte of SY on the first of SW, the first byte of SY on the last of X8 (SY fits the gaps between buffers)
    nsy = M * (N // 32)
    cases["the end of SY on the start of SW"] = lambda: run(x8, sx, w8, sw, bias, dtype, out8=y8,
                                                           out_scales=arena[sw.data_ptr() - arena.data_ptr() - nsy + 1:][:nsy].view(M, 4, N // 128))
    cases["the start of SY on the end of X8"] = lambda: run(x8, sx, w8, sw, bias, dtype, out8=y8,
                                                           out_scales=arena[x8.data_ptr() - arena.data_ptr() + M * K - 1:][:nsy].view(M, 4, N // 128))
    assert nsy < 4096
    torch.cuda.synchronize()
    snap = arena.clone()
    for name, call in cases.items():
        with pytest.raises(_hip.D3PMError):
            call()
            pytest.fail(f"{name}: not refused")
        torch.cuda.synchronize()
        assert torch.equal(arena, snap), f"{name}: refused, but something was written"
    # the same buffers are accepted once nothing is wrong with the call: the refusals above are not the arena's
    arena[x8.data_ptr() - arena.data_ptr():][:M * K] = 0
    arena[w8.data_ptr() - arena.data_ptr():][:N * K] = 0
    bias.zero_()
    r1.zero_()
    run(x8, sx, w8, sw, bias, dtype, out=y)
    run(x8, sx, w8, sw, bias, dtype, r1=r1, out=r1)
    run(x8, sx, w8, sw, bias, dtype, out8=y8, out_scales=sy)
    assert bool((y == 0).all()) and bool((r1 == 0).all()) and bool(((y8 & 0x7F) == 0).all()) and bool((sy == 1).all())

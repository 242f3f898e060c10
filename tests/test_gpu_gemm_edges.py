"""Every GEMM schedule at its ragged edges: exact results, untouched surroundings, unchanged operands (csrc/d3pm_mfma_tile.h
epilogue_store; csrc/d3pm_mfma_gemm.hip, d3pm_mfma_gemm_lat.hip, d3pm_mfma_gemm_big.hip; csrc/d3pm_plan.cpp plan_linear).

The operands are dyadic (tests/gemm_exact_ref.py): every partial sum is exact in fp32 whatever the order, so the stored 16-bit value is
decided by the rounding chain of the epilogue alone, and every family, schedule and tile geometry has to reproduce the host evaluation
of that chain bit for bit on every element -- in partial tiles, with row strides that differ from the widths, in place, and with the
moments of the stored rows.  Result, operands and moment buffers live in storages prefilled with a NaN pattern, with at least a full
tile of guard rows on either side: a store past row M, into the pad columns or into a moment slot of a row that does not exist is seen
as a changed guard element, a load that strays onto a stored element as a NaN or an inexact value.  (The guards keep a stray store
inside the allocation; nothing here provokes a fault.)

The activation sweep at the end drives the MFMA epilogues with every finite 16-bit pre-activation in [-8, 8]."""
import math

import pytest
import torch

import gemm_exact_ref as R
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
GENERIC, MFMA = 1, 2      # _hip.FAMILY_GENERIC / FAMILY_MFMA
MASK_PERIOD = 7
# (name, tuning) per family: the schedules whose kernels the family's shapes reach; "auto" is gemm_variant 0
SCHEDULES = {
    "k128": [("auto", dict(gemm_variant=0)), ("v2", dict(gemm_variant=2)), ("v3", dict(gemm_variant=3)), ("v5", dict(gemm_variant=5))],
    "panel64": [("auto", dict(gemm_variant=0)), ("v4_lat1", dict(gemm_variant=4, lat_tile=1)), ("v4_lat2", dict(gemm_variant=4, lat_tile=2)),
                ("v4_lat3", dict(gemm_variant=4, lat_tile=3))],
    "big": [("auto", dict(gemm_variant=0)), ("v6", dict(gemm_variant=6)), ("v7", dict(gemm_variant=7)), ("v8", dict(gemm_variant=8))],
}
ALL_SCHEDULES = [("auto", dict(gemm_variant=0))] + [s for fam in ("k128", "panel64", "big") for s in SCHEDULES[fam][1:]]
EPILOGUES = ("bias", "nobias", "r1", "r1r2", "r1mask", "r1_inplace", "relu")
WITH_R1 = ("r1", "r1r2", "r1mask", "r1_inplace")
CASES = [(fam, M, N, K, padded) for fam, shapes in R.SHAPES.items() for i, (M, N, K, _) in enumerate(shapes)
         for padded in ((True, False) if i == 0 or N % 8 else (True,))]      # one shape per family (and the odd N) also runs tight


def _case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-{'padded' if c[4] else 'tight'}"


def _strides(N, K, padded):
    n8 = (N + 7) // 8 * 8
    return (K + 8, n8 + 8, N + 16) if padded else (K, n8, N)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _mask():
    return (torch.arange(MASK_PERIOD) % 3 != 1).to(torch.uint8)


_CPU = {}


def _operands(dtype, M, N, K, moments=False):
    """dyadic operands and the expected rows per epilogue, computed once per (type, shape) and never changed"""
    key = (dtype, M, N, K, moments)
    if key not in _CPU:
        x, w, bias, r1, r2 = R.dyadic_operands(M, N, K, dtype, 1000 * M + N + K, moments=moments)
        _CPU[key] = dict(x=x, w=w, bias=bias, r1=r1, r2=r2, mask=_mask(), expected={})
    return _CPU[key]


def _expected(o, dtype, epi):
    if epi not in o["expected"]:
        r1 = o["r1"] if epi in WITH_R1 else None
        o["expected"][epi] = R.epilogue_chain(o["x"], o["w"], None if epi == "nobias" else o["bias"], dtype, act="relu" if epi == "relu" else "none",
                                              r1=r1, r2=o["r2"] if epi == "r1r2" else None, row_mask=o["mask"] if epi == "r1mask" else None,
                                              mask_period=MASK_PERIOD)
    return o["expected"][epi]


class Inputs:
    """The operands of one case in guarded device storages, with a snapshot of every storage."""

    def __init__(self, o, dtype, ldx, ldr):
        M, K = o["x"].shape
        N = o["w"].shape[0]
        self.store = {}
        self.store["x"], self.x = R.guarded(M, K, ldx, dtype, device=DEV, fill=o["x"])
        self.store["w"], self.w = R.guarded(N, K, K, dtype, device=DEV, fill=o["w"])
        self.store["bias"], self.bias = R.guarded_flat((N,), dtype, device=DEV, fill=o["bias"])
        self.store["r1"], self.r1 = R.guarded(M, N, ldr, dtype, device=DEV, fill=o["r1"])
        self.store["r2"], self.r2 = R.guarded(M, N, ldr, dtype, device=DEV, fill=o["r2"])
        self.store["mask"], self.mask = R.guarded_flat((MASK_PERIOD,), torch.uint8, device=DEV, fill=o["mask"])
        self.snap = {k: v.clone() for k, v in self.store.items()}

    def assert_unchanged(self, what):
        for k, v in self.store.items():
            a, b = (v, self.snap[k]) if v.dtype == torch.uint8 else (v.view(torch.int16), self.snap[k].view(torch.int16))
            assert torch.equal(a, b), f"{what}: the operand {k} (or its guard) was written"


def _linear(inp, epi, family, tune, y, r1=None):
    from vall_e.vall_e import _hip
    r1 = (inp.r1 if r1 is None else r1) if epi in WITH_R1 else None
    with _hip.tuning(**tune):
        return _hip.op_linear(inp.x, inp.w, None if epi == "nobias" else inp.bias, act=2 if epi == "relu" else 0, r1=r1,
                              r2=inp.r2 if epi == "r1r2" else None, row_mask=inp.mask if epi == "r1mask" else None, mask_period=MASK_PERIOD,
                              family=family, out=y, ldy=y.stride(0))


def _epilogues(fam, with_r1):
    # ReLU exists in the 128 x 128 one-tile kernel alone (and in the generic family), without a residual: planned for every gemm_variant
    return [e for e in EPILOGUES if (with_r1 or e not in WITH_R1) and (e != "relu" or fam == "k128")]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_every_schedule_is_exact_and_stays_inside_its_result(built_lib, dtype, case):
    """Per epilogue and schedule: the stored view equals the host chain bit for bit (so generic equals MFMA bit for bit), everything
    outside the view of Y is untouched, x, w, bias, r1, r2 and the mask are unchanged (r1 excepted where it is the output)."""
    from vall_e.vall_e import _hip
    fam, M, N, K, padded = case
    with_r1 = dict((s[:3], s[3]) for s in R.SHAPES[fam])[(M, N, K)]
    ldx, ldy, ldr = _strides(N, K, padded)
    o = _operands(dtype, M, N, K)
    inp = Inputs(o, dtype, ldx, ldr)
    problems = []
    for epi in _epilogues(fam, with_r1):
        exp = _bits(_expected(o, dtype, epi))
        stored = {}
        for name, tune in [("generic", {})] + SCHEDULES[fam]:
            what = f"{_case_id(case)} {IDS[DTYPES.index(dtype)]} {epi} {name}"
            family = GENERIC if name == "generic" else MFMA
            if epi == "relu" and name not in ("generic", "v5"):
                continue
            if family == MFMA:      # the planner's admission rule: a refusal by the library below is then a finding
                assert R.k128_ok(M, N, K, ldx, ldr if epi == "r1_inplace" else ldy, ldr if epi in WITH_R1 else None), what
            if epi == "r1_inplace":      # out is r1: the view of Y has R1's stride
                ys, y = R.guarded(M, N, ldr, dtype, device=DEV, fill=o["r1"])
                got = _linear(inp, epi, family, tune, y, r1=y)
            else:
                ys, y = R.guarded(M, N, ldy, dtype, device=DEV)
                got = _linear(inp, epi, family, tune, y)
            assert got.data_ptr() == y.data_ptr() and got.shape == (M, N)
            stored[name] = _bits(got.cpu())
            wrong = stored[name] != exp
            if wrong.any():      # every schedule runs before the test fails, so that one run names all that differ
                at = tuple(wrong.nonzero()[0].tolist())
                problems.append(f"{what}: {int(wrong.sum())} of {M * N} elements differ from the rounding chain, first at {list(at)}: "
                                f"{got.cpu()[at].item()!r} for {_expected(o, dtype, epi)[at].item()!r}")
            R.assert_untouched(ys, y, what)
            inp.assert_unchanged(what)
        for name, b in stored.items():
            if not torch.equal(b, stored["generic"]):
                problems.append(f"{_case_id(case)} {epi}: {name} differs from the generic family")
    assert not problems, "\n".join(problems)
    assert _hip.TUNING.gemm_variant == 0 and _hip.TUNING.lat_tile == 0


# ---- moments of the stored rows ------------------------------------------------------------------------------------------------------
def _slack_rows(M, parts):
    """bool [ceil(M / 16), parts, 16, 2]: the slots of the rows M .. 16 ceil(M / 16) - 1, which the layout holds and no row owns"""
    nblk = (M + 15) // 16
    rows = torch.arange(nblk)[:, None, None, None] * 16 + torch.arange(16)[None, None, :, None]
    return (rows >= M).expand(nblk, parts, 16, 2)


def _moment_call(inp, epi, tune, y, st, live=False):
    from vall_e.vall_e import _hip
    with _hip.tuning(**tune):
        if live:
            M = inp.x.shape[0]
            _hip.op_linear_live(inp.x, inp.w, inp.bias, y, torch.tensor([M], dtype=torch.int32, device=DEV), r1=inp.r1,
                                row_mask=inp.mask if epi == "r1mask" else None, stats_out=st)
        else:
            _hip.op_linear_stats(inp.x, inp.w, inp.bias, inp.r1, r2=inp.r2 if epi == "r1r2" else None,
                                 row_mask=inp.mask if epi == "r1mask" else None, mask_period=MASK_PERIOD, out=y, stats=st)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("padded", [True, False], ids=["padded", "tight"])
@pytest.mark.parametrize("M,N,K", R.MOMENT_SHAPES)
def test_moments_are_exact_and_no_slot_of_a_missing_row_is_written(built_lib, dtype, M, N, K, padded):
    """d3pm_op_linear_stats with integer operands of |y| <= 64: 512 * 64^2 < 2^24, so the fp32 moments are exact in every order too.
    Y equals the chain, the pair of every (row < M, part) equals the float64 moments of the stored row, and nothing else of the moment
    storage is written -- neither its guards nor the slots of the rows M .. 16 ceil(M / 16) - 1 inside the layout, which every
    producer leaves alone (part_stats_store's `ok`; include/d3pm_hip.h, d3pm_op_row_stats).  (The lanes of the rows >= M compute row
    M - 1 again from clamped loads and address its pair, so without `ok` they would store the same bits a second time: what this test
    pins is the address -- the slot of the row itself would be one of the slack slots.)  On the whole-tile shape the short
    tiles (gemm_variant 9 / 10) run too, through d3pm_op_linear_live with the quad format."""
    from vall_e.vall_e import _hip
    ldx, ldy, ldr = _strides(N, K, padded)
    o = _operands(dtype, M, N, K, moments=True)
    inp = Inputs(o, dtype, ldx, ldr)
    big = all(R.big_tile(M, N, K, v) for v in (6, 7, 8))
    runs = [(name, tune, False) for name, tune in ALL_SCHEDULES]
    if big:
        runs += [(f"v{v}_quads", dict(gemm_variant=v), True) for v in (9, 10) if R.big_tile(M, N, K, v)]
    for epi in ("r1", "r1r2", "r1mask"):
        expected = _expected(o, dtype, epi)
        assert expected.abs().max() <= 64
        for name, tune, live in runs:
            if live and epi == "r1r2":
                continue                 # the short tiles are instantiated for R1 [+ mask] + quads alone (d3pm_plan.cpp short_tile_epilogue)
            what = f"{M}x{N}x{K} {IDS[DTYPES.index(dtype)]} {epi} {name}"
            assert R.k128_ok(M, N, K, ldx, ldy, ldr), what
            part = 128 if live else 32
            ys, y = R.guarded(M, N, ldy, dtype, device=DEV)
            ss, st = R.guarded_flat(((M + 15) // 16, N // part, 16, 2), torch.float32, device=DEV)
            _moment_call(inp, epi, tune, y, st, live)
            assert torch.equal(_bits(y.cpu()), _bits(expected)), f"{what}: the stored rows differ from the rounding chain"
            got = _hip.stats_rows(st, M).cpu().double()
            assert torch.equal(got, R.part_moments(expected, part)), f"{what}: the moments are not those of the stored rows"
            R.assert_untouched(ys, y, what)
            R.assert_untouched(ss, st, what + " moments", also=_slack_rows(M, N // part))
            inp.assert_unchanged(what)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_stats_leaves_the_slots_of_missing_rows_alone(built_lib, dtype):
    """d3pm_op_row_stats itself, on rows with a stride: exact moments for rows < M, nothing else written."""
    from vall_e.vall_e import _hip
    M, d = 200, 512
    o = _operands(dtype, M, d, 64, moments=True)
    y = _expected(o, dtype, "r1")
    xs, x = R.guarded(M, d, d + 8, dtype, device=DEV, fill=y)
    ss, st = R.guarded_flat(((M + 15) // 16, d // 32, 16, 2), torch.float32, device=DEV)
    _hip.op_row_stats(x, stats=st)
    assert torch.equal(_hip.stats_rows(st, M).cpu().double(), R.part_moments(y))
    R.assert_untouched(ss, st, "row_stats", also=_slack_rows(M, d // 32))


# ---- the folded projection -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fam", list(R.FOLD_SHAPES))
def test_folded_projection_with_strides_guards_and_zero_rows(built_lib, dtype, fam):
    """d3pm_op_linear_fold with ldx and ldy padded into guarded storage equals the tight call bit for bit under every schedule of the
    family and leaves the guards alone.  The exact value is not available here (rsqrt), except for the all-zero rows every padded frame
    of the canvas is in production: their moments are (0, 0), so mean = 0, the variance clamps to 0, rc = -0 (fold_row_scalars) and
    y = fma(0, ra, fma(-0, s_n, b'_n)) = b'_n: with act = 0 the stored row is rn(fold_b) bit for bit."""
    from vall_e.vall_e import _hip
    M, N, K = R.FOLD_SHAPES[fam]
    g = torch.Generator().manual_seed(M + N)
    xc = (torch.randn(M, K, generator=g) * 1.5 + 0.5).to(dtype)
    zero_rows = [0, 7, M // 2, M - 1]
    xc[zero_rows] = 0
    gamma = (1.0 + 0.3 * torch.randn(K, generator=g)).to(dtype).to(DEV)
    beta = (0.2 * torch.randn(K, generator=g)).to(dtype).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).to(DEV)
    b = (0.1 * torch.randn(N, generator=g)).to(dtype).to(DEV)
    wf, fs, fb = _hip.op_fold_weights(w, b, gamma, beta)
    xs, x = R.guarded(M, K, K + 8, dtype, device=DEV, fill=xc)
    x_tight = xc.to(DEV)
    st = _hip.op_row_stats(x)
    assert torch.equal(st, _hip.op_row_stats(x_tight))
    snap = xs.clone()
    first = {}
    for name, tune in SCHEDULES[fam] + ([("v4", dict(gemm_variant=4))] if fam == "k128" else []):
        for act in (0, 1):
            what = f"fold {fam} {IDS[DTYPES.index(dtype)]} act {act} {name}"
            with _hip.tuning(**tune):
                tight = _hip.op_linear_fold(x_tight, wf, fs, fb, st, act=act)
                ys, y = R.guarded(M, N, N + 8, dtype, device=DEV)
                got = _hip.op_linear_fold(x, wf, fs, fb, st, act=act, out=y)
            assert got.data_ptr() == y.data_ptr()
            assert torch.equal(_bits(y), _bits(tight)), f"{what}: strides change the result"
            assert not torch.isnan(tight.float()).any(), what
            R.assert_untouched(ys, y, what)
            assert torch.equal(xs.view(torch.int16), snap.view(torch.int16)), f"{what}: x was written"
            if act == 0:
                assert torch.equal(_bits(y[zero_rows]), _bits(fb.to(dtype).expand(len(zero_rows), N))), f"{what}: a zero row is not rn(fold_b)"
            assert torch.equal(_bits(y), _bits(first.setdefault(act, y))), f"{what}: differs from {SCHEDULES[fam][0][0]}"


# ---- activation sweep --------------------------------------------------------------------------------------------------------------------
SWEEP_K, SWEEP_M = 256, 384      # x = the K x K identity and its first 128 rows again: 384 rows are two whole 192-row big tiles
U = 2.0 ** -24                   # half an ulp of fp32 relative to the value: the error of one fp32 operation
TINY = 4 * 2.0 ** -149           # a few fp32 operations whose result is subnormal (bf16 subnormals halve into fp32 ones)


def _gelu64(v):
    return 0.5 * v * torch.special.erfc(-v / math.sqrt(2.0))      # = 0.5 v (1 + erf(v / sqrt 2)) without the cancellation


def gelu_delta(v, g):
    """|fp32 result of gelu_erf (csrc/d3pm_mfma_tile.h) - exact GELU| for an exact 16-bit v, from what the source claims:
      z' = fl(v * fl(1 / sqrt 2)) = z (1 + e), |e| <= 2 U (the constant and the product); erf moves by at most
           |z| 2 U max|erf'| e^(-z^2) <= 2 U (2 / sqrt pi) max(z e^(-z^2)) = 2 U * 0.4840 < U;
      E  = erf_fit(z') within 1.4 U absolute of erf(z') (the header comment of erf_fit, |z'| <= 5.66 < 6), so |E - erf z| <= 2.4 U;
      s  = fl(1 + E) = (1 + erf z) + a + b with |a| <= 2.4 U and |b| <= U (1 + erf z + 2.4 U);
      h  = 0.5f * v is exact; out = fl(h s) = h s (1 + e5), |e5| <= U.
    So |out - g| <= 0.5 |v| (|a| + |b|) (1 + U) + |g| U (+ TINY where an intermediate is an fp32 subnormal)."""
    one_plus_erf = torch.special.erfc(-v / math.sqrt(2.0))
    return 0.5 * v.abs() * (2.4 * U + U * (one_plus_erf + 2.4 * U)) * (1 + U) + g.abs() * U + TINY


def silu_delta(v, g):
    """|fp32 result of v / (1.0f + expf(-v)) - exact SiLU|: expf is within 1 ulp = 2 U relative (HIP's documented bound for expf),
    d = fl(1 + e) and the correctly rounded quotient fl(v / d) add U each.  With E = exp(-v), the relative error of 1 + E (1 + e1) is
    sigmoid(-v) |e1|, so |out - g| <= |g| (2 U sigmoid(-v) + 2 U) up to second order, which the factor (1 + 2^-20) covers
    (the first-order term is below 2^-22) (+ TINY for subnormal quotients)."""
    return g.abs() * (2 * U * torch.sigmoid(-v) + 2 * U) * (1 + 2.0 ** -20) + TINY


def _sweep(dtype, act, tune):
    from vall_e.vall_e import _hip
    vals = R.finite_values(dtype)
    N = (vals.numel() + SWEEP_K - 1) // SWEEP_K
    N = (N + 127) // 128 * 128
    w = vals.repeat((N * SWEEP_K + vals.numel() - 1) // vals.numel())[:N * SWEEP_K].view(N, SWEEP_K)
    eye = torch.eye(SWEEP_K, dtype=dtype)
    x = torch.cat([eye, eye[:SWEEP_M - SWEEP_K]])
    ys, y = R.guarded(SWEEP_M, N, N + 8, dtype, device=DEV)
    with _hip.tuning(**tune):
        _hip.op_linear(x.to(DEV), w.to(DEV), torch.zeros(N, dtype=dtype, device=DEV), act=act, family=MFMA, out=y, ldy=y.stride(0))
    R.assert_untouched(ys, y, f"sweep act {act} {tune}")
    pre = torch.cat([w.T, w.T[:SWEEP_M - SWEEP_K]])            # Y[m][n] = act(w[n][m mod K])
    return pre.double(), y.cpu()


def _check_sweep(dtype, name, pre, got, g, delta, tag):
    lo, hi = R.rn16(g - delta, dtype).double(), R.rn16(g + delta, dtype).double()
    gd = got.double()
    plain = R.rn16(g, dtype)
    steps = R.ulp_steps(got, plain)
    tail = pre <= -2.0
    # the excess over plain rn16(g): in storage ulps where the value carries them (v > -2); in the negative tail, where 1 + erf cancels
    # against the 2^-24 grid and the kernel's claim is an absolute one, in absolute terms
    REPORT[f"gemm_sweep_{name}_{IDS[DTYPES.index(dtype)]}_{tag}"] = {
        "max_ulp_from_rn16_of_exact_above_minus_2": int(steps[~tail].max()), "elements_off_rn16_of_exact_above_minus_2": int((steps[~tail] != 0).sum()),
        "elements_off_rn16_of_exact_negative_tail": int((steps[tail] != 0).sum()), "elements": got.numel(),
        "negative_tail_max_abs_excess": float((gd - plain.double())[tail].abs().max()), "negative_tail_max_abs_err": float((gd - g)[tail].abs().max())}
    print(f"sweep {name} {dtype} {tag}: {REPORT[f'gemm_sweep_{name}_{IDS[DTYPES.index(dtype)]}_{tag}']}")
    bad = ~((gd >= lo) & (gd <= hi))      # (a NaN fails both comparisons)
    assert not bad.any(), (f"{name} {dtype} {tag}: {int(bad.sum())} of {bad.numel()} stored values lie outside [rn16(g - delta), rn16(g + delta)]; the worst "
                           f"pre-activations: {pre[bad][:8].tolist()} gave {gd[bad][:8].tolist()} for {g[bad][:8].tolist()}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tag,tune", [("v5", dict(gemm_variant=5)), ("v4", dict(gemm_variant=4)), ("v8", dict(gemm_variant=8))])
def test_gelu_of_every_16_bit_value(built_lib, dtype, tag, tune):
    """act = GELU through the 128 x 128 one-tile, the panel64 and the 192 x 128 big-tile epilogue (384 x 256 x 256 is admitted by all
    three: two whole 192-row tiles): every stored value lies in [rn16(g - delta), rn16(g + delta)] with g the float64 GELU and delta
    of gelu_delta.  REPORT receives the measured distance from plain rn16(g)."""
    assert R.k128_ok(SWEEP_M, 256, SWEEP_K, SWEEP_K, 264) and R.panel64_ok(SWEEP_M, 256, SWEEP_K, SWEEP_K, 264) and R.big_tile(SWEEP_M, 256, SWEEP_K, 8)
    pre, got = _sweep(dtype, 1, tune)
    g = _gelu64(pre)
    _check_sweep(dtype, "gelu", pre, got, g, gelu_delta(pre, g), tag)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_relu_and_silu_of_every_16_bit_value(built_lib, dtype):
    """The condition encoders' activations (the 128 x 128 one-tile kernel): ReLU exact by value (-0 equals +0), SiLU within silu_delta."""
    pre, got = _sweep(dtype, 2, dict(gemm_variant=5))
    assert torch.equal(got.double(), torch.clamp_min(pre, 0.0)), "ReLU is not exact"
    pre, got = _sweep(dtype, 3, dict(gemm_variant=5))
    g = pre * torch.sigmoid(pre)
    _check_sweep(dtype, "silu", pre, got, g, silu_delta(pre, g), "v5")

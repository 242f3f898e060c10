"""The host reference of the exact GEMM tests (tests/gemm_exact_ref.py) against torch's eager 16-bit CPU ops, without a GPU: the
rounding chain, the operand generator's exactness bound for every shape tests/test_gpu_gemm_edges.py uses, the guards, and the
single-rounding conversion the activation bounds are built with."""
import pytest
import torch

import gemm_exact_ref as R

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
EPILOGUES = ("bias", "nobias", "r1", "r1r2", "r1mask", "relu")
ALL_SHAPES = [s[:3] for fam in R.SHAPES.values() for s in fam]


def _eager(x, w, bias, dtype, epi, r1, r2, mask, period):
    """The same chain with torch's own 16-bit ops: each of them computes in fp32 and rounds once."""
    acc = x.float() @ w.float().T                  # exact for dyadic operands, in any order
    v = (acc + bias.float()).to(dtype) if epi != "nobias" else acc.to(dtype)
    if epi == "relu":
        v = torch.relu(v)
    if epi in ("r1", "r1mask"):
        v = r1 + v
    if epi == "r1r2":
        v = (r1 + r2) + v
    if epi == "r1mask":
        v = v * (mask[torch.arange(x.shape[0]) % period] != 0).to(dtype)[:, None]
    return v


def _chain(x, w, bias, dtype, epi, r1, r2, mask, period, **kw):
    return R.epilogue_chain(x, w, None if epi == "nobias" else bias, dtype, act="relu" if epi == "relu" else "none",
                            r1=r1 if epi in ("r1", "r1r2", "r1mask") else None, r2=r2 if epi == "r1r2" else None,
                            row_mask=mask if epi == "r1mask" else None, mask_period=period, **kw)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("epi", EPILOGUES)
def test_chain_equals_eager_16_bit_ops(dtype, epi):
    M, N, K = 129, 136, 192
    x, w, bias, r1, r2 = R.dyadic_operands(M, N, K, dtype, 3)
    mask = (torch.arange(7) % 3 != 1).to(torch.uint8)
    got, ref = _chain(x, w, bias, dtype, epi, r1, r2, mask, 7), _eager(x, w, bias, dtype, epi, r1, r2, mask, 7)
    assert got.dtype == dtype and torch.equal(_bits(got), _bits(ref))
    if epi == "r1mask":      # the sign of a masked negative value survives, as `v * mask` leaves it in the kernels
        assert (_bits(got)[1] == -0x8000).any() and (_bits(got)[1] == 0).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_swapped_residual_order_is_caught(dtype):
    """The mutation of the reference: rn(rn(R1 + v) + R2) instead of rn(rn(R1 + R2) + v) gives other bits on a good share of the elements,
    so a kernel that rounds in that order cannot pass."""
    x, w, bias, r1, r2 = R.dyadic_operands(129, 136, 64, dtype, 4)
    ref = _eager(x, w, bias, dtype, "r1r2", r1, r2, None, 1)
    wrong = _chain(x, w, bias, dtype, "r1r2", r1, r2, None, 1, swap_residual_order=True)
    assert (_bits(wrong) != _bits(ref)).float().mean() > 0.1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,N,K", ALL_SHAPES)
def test_bound_and_rounding_for_every_gpu_shape(dtype, M, N, K):
    assert R.exactness_bound(K, dtype) < 2 ** 24
    x, w, bias, r1, r2 = R.dyadic_operands(M, N, K, dtype, M + N + K)
    q = 2.0 ** (R.X_EXP + R.W_EXP)
    acc = x.double() @ w.double().T
    assert (acc.abs().max() + bias.double().abs().max()) / q <= R.exactness_bound(K, dtype)
    assert torch.equal(acc / q, (acc / q).round())
    for t in (bias, r1, r2):
        assert torch.equal(t.double() / q, (t.double() / q).round())
    s = acc + bias.double()
    if dtype == torch.bfloat16:      # most results need rounding: the rounding points are exercised
        assert (s.to(dtype).double() != s).double().mean() > 0.5
    rr = r1.double() + r2.double()
    assert (rr.to(dtype).double() != rr).double().mean() > 0.25


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,N,K", R.MOMENT_SHAPES)
def test_moment_operands_keep_the_squares_exact(dtype, M, N, K):
    x, w, bias, r1, r2 = R.dyadic_operands(M, N, K, dtype, M + K, moments=True)
    mask = (torch.arange(7) % 3 != 1).to(torch.uint8)
    for epi in ("r1", "r1r2", "r1mask"):
        y = _chain(x, w, bias, dtype, epi, r1, r2, mask, 7)
        assert torch.equal(y.double(), y.double().round()) and y.abs().max() <= 64
        assert N * 64 ** 2 < 2 ** 24
        m = R.part_moments(y)
        assert torch.equal(m.float().double(), m) and m.shape == (M, N // 32, 2)
        assert (y != 0).float().mean() > 0.5


@pytest.mark.parametrize("dtype", DTYPES + [torch.float32], ids=IDS + ["f32"])
def test_assert_untouched_sees_one_flipped_guard_element(dtype):
    rows, cols, ld = 5, 24, 32
    for where in ("front", "pad", "behind", "first", "last"):
        storage, view = R.guarded(rows, cols, ld, dtype)
        view.fill_(1.0)                                    # writing the view itself is what a kernel is for
        R.assert_untouched(storage, view)
        at = {"front": R.GUARD_ROWS * ld - 1, "pad": R.GUARD_ROWS * ld + cols, "behind": (R.GUARD_ROWS + rows) * ld, "first": 0,
              "last": storage.numel() - 1}[where]
        ints = storage.view(torch.int16 if dtype != torch.float32 else torch.int32)
        ints[at] ^= 1
        with pytest.raises(AssertionError, match="outside the view"):
            R.assert_untouched(storage, view, where)
    storage, view = R.guarded_flat((3, 4, 16, 2), torch.float32)
    view[:2] = 0.5
    R.assert_untouched(storage, view, also=torch.arange(3)[:, None, None, None].expand(3, 4, 16, 2) >= 2)
    view[2, 1, 15, 0] = 0.0
    with pytest.raises(AssertionError, match="belong to no row"):
        R.assert_untouched(storage, view, also=torch.arange(3)[:, None, None, None].expand(3, 4, 16, 2) >= 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rn16_rounds_once(dtype):
    """Just beside the midpoint of two neighbours the conversion through fp32 rounds to the midpoint first and then to even; rn16 must
    give the nearer neighbour."""
    vals = R.finite_values(dtype)
    assert vals.numel() == {torch.float16: 2 * (0x4800 + 1), torch.bfloat16: 2 * (0x4100 + 1)}[dtype] and vals.abs().max() == 8
    pos = vals[1:vals.numel() // 2].double()                # 0 < a < b neighbours
    a, b = pos[:-1], pos[1:]
    mid = (a + b) / 2
    for sign in (1.0, -1.0):
        assert torch.equal(R.rn16(sign * mid * (1 + 2.0 ** -30), dtype).double(), sign * b)
        assert torch.equal(R.rn16(sign * mid * (1 - 2.0 ** -30), dtype).double(), sign * a)
        even = torch.where((_bits(a.to(dtype)) & 1) == 0, a, b)
        assert torch.equal(R.rn16(sign * mid, dtype).double(), sign * even)
    x = torch.randn(100000, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 3
    assert (R.rn16(x, dtype) != x.to(dtype)).float().mean() < 1e-3      # and it is the ordinary conversion nearly everywhere


def test_every_shape_is_admitted_by_its_family():
    """The Python copies of the planner's admission rules (csrc/d3pm_plan.cpp) accept the shapes of their family with the strides the GPU
    test passes, so that a D3PM_E_SHAPE on the GPU is a finding and not a skipped case."""
    for fam, shapes in R.SHAPES.items():
        for M, N, K, with_r1 in shapes:
            n8 = (N + 7) // 8 * 8
            for ldx, ldy, ldr in ((K, n8, N), (K + 8, n8 + 8, N + 16)):
                assert R.k128_ok(M, N, K, ldx, ldy, ldr if with_r1 else None), (fam, M, N, K)
                if fam == "panel64":
                    assert R.panel64_ok(M, N, K, ldx, ldy, ldr if with_r1 else None)
                if fam == "big":
                    assert all(R.big_tile(M, N, K, v) for v in (6, 7, 8))
    M, N, K = R.MOMENT_SHAPES[-1]
    assert all(R.big_tile(M, N, K, v) for v in (6, 7, 8, 9, 10))
    assert R.big_tile(*R.FOLD_SHAPES["big"], 8) and R.FOLD_SHAPES["big"][2] == 512

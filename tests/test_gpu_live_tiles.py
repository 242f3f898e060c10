"""The big-tile GEMM on a device-side live row count in the geometries the live-row estimate selects (csrc/d3pm_mfma_gemm_big.hip;
csrc/d3pm_plan.cpp big_tile with LinearArgs::rows_est; d3pm_op_linear_live_rows).

The short tiles of the deduplicated loop's producers -- 96 x 128 and 128 x 128, forced by gemm_variant = 9 / 10 -- and 192 x 256 tiles
(gemm_variant = 6) on a capacity of 768 rows, N = 512, K = 256 (four k-steps: the loop's last-step edge) and K = 2048, f16 and bf16,
the two producer epilogues with quads and the dual form, live counts around every tile edge and estimates of every kind (none, one
row, one tile, below and above the live count, the capacity).  Rows below the live count and their quads equal those of 192 x 128
tiles (geometry 3, gemm_variant = 8) at the same live count bit for bit; every row from the end of the last live tile on keeps the
sentinel the output was filled with.  A second test lets the automatic rule choose at the capacity of 32 utterances, where the
estimate moves a producer from 96-row to 128-row to 192-row tiles."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, N = 768, 512
TILE_ROWS = {6: 192, 9: 96, 10: 128}      # gemm_variant -> rows of the tile it forces
EPILOGUES = ("r1_stats", "r1_mask_stats", "dual")
SENTINEL = 9.0


def _lives(tm):
    return sorted({0, 1, tm - 1, tm, tm + 1, 383, 384, 385, 767, 768})


def _estimates(live, tm):
    return sorted({0, 1, tm, max(live - 1, 0), min(live + 1, M), M})


def _operands(dtype, K, rows, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=gen) * 0.3).to(dtype).to(DEV)      # noqa: E731
    return {"x": r(rows, K), "x2": r(rows, K), "w": r(N, K), "b": r(N), "res": r(rows, N),
            "mask": (torch.rand(rows, generator=gen) < 0.7).to(torch.uint8).to(DEV)}


@pytest.fixture(scope="module")
def operands(built_lib):
    cache = {}

    def get(dtype, K):
        if (dtype, K) not in cache:
            cache[(dtype, K)] = _operands(dtype, K, M, 7 * K + 1)
        return cache[(dtype, K)]
    return get


def _quad_rows(st, rows):
    """quads [rows / 16][N / 128][16][2] as [rows][N / 128][2]"""
    return st.view(rows // 16, N // 128, 16, 2).permute(0, 2, 1, 3).reshape(rows, N // 128, 2)


def _live(o, epi, live, rows_est):
    from vall_e.vall_e import _hip
    rows = o["x"].shape[0]
    y = torch.full((rows, N), SENTINEL, dtype=o["x"].dtype, device=DEV)
    st = torch.full((rows // 16, N // 128, 16, 2), SENTINEL, dtype=torch.float32, device=DEV)
    m_live = torch.tensor([live], dtype=torch.int32, device=DEV)
    kw = dict(r1=o["res"], stats_out=st, rows_est=rows_est)
    if epi == "r1_mask_stats":
        kw["row_mask"] = o["mask"]
    elif epi == "dual":
        kw["x2"] = o["x2"]
    _hip.op_linear_live(o["x"], o["w"], o["b"], y, m_live, **kw)
    return y, _quad_rows(st, rows)


def _check(o, epi, live, rows_est, ref, tag, tm, whole_tile=True):
    y, st = _live(o, epi, live, rows_est)
    ref_y, ref_st = ref
    edge = (live + tm - 1) // tm * tm
    assert torch.equal(y[:live], ref_y[:live]), tag
    assert torch.equal(st[:live], ref_st[:live]), tag + ("quads",)
    assert (y[edge:] == SENTINEL).all(), tag + ("a row behind the last live tile was written",)
    assert (st[edge:] == SENTINEL).all(), tag + ("quads behind the last live tile were written",)
    if whole_tile:      # ... and the last live tile was written whole: it is `tm` rows high, the geometry that was asked for ran
        assert not (y[live:edge] == SENTINEL).all(dim=1).any() and not (st[live:edge] == SENTINEL).any(), tag + ("the last live tile is not whole",)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("K", [256, 2048])
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("variant", sorted(TILE_ROWS), ids=["192x256", "96x128", "128x128"])
def test_forced_geometry_equals_192x128_tiles(operands, dtype, K, epi, variant):
    from vall_e.vall_e import _hip
    o, tm = operands(dtype, K), TILE_ROWS[variant]
    for live in _lives(tm):
        if ("ref", epi, live) not in o:      # computed once per (operands, epilogue, live count), shared by the three geometries
            with _hip.tuning(gemm_variant=8):
                o[("ref", epi, live)] = _live(o, epi, live, None)
        ref = o[("ref", epi, live)]
        if live:
            assert not (ref[0][:live] == SENTINEL).all(dim=1).any()
        for rows_est in _estimates(live, tm):
            with _hip.tuning(gemm_variant=variant):
                _check(o, epi, live, rows_est, ref, (str(dtype), K, epi, variant, "m_live", live, "rows_est", rows_est), tm)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_the_automatic_rule_at_the_capacity_of_32_utterances(built_lib, dtype):
    """gemm_variant = 0: the estimate plans 96 x 128 tiles up to 6144 rows, 128 x 128 up to 8192, 192 x 128 above and without one
    (tests/test_live_tiles_plan_api.py pins the rule); the live count lies below, at and far above the estimate.  All give the rows of
    forced 192 x 128 tiles; behind the live count nothing is written from the next multiple of 384 on, whichever tile ran."""
    from vall_e.vall_e import _hip
    rows = 32 * 768
    o = _operands(dtype, 256, rows, 11)
    for epi in EPILOGUES:
        for live in (1, 6000, 8190, 15000, rows):
            with _hip.tuning(gemm_variant=8):
                ref = _live(o, epi, live, None)
            for rows_est in (0, 3000, 6144, 6145, 8192, 8193, rows - 1, rows):
                _check(o, epi, live, rows_est, ref, (str(dtype), epi, "m_live", live, "rows_est", rows_est), 384, whole_tile=False)

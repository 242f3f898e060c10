"""gemm_mfma_panel64 on a device-side live row count (csrc/d3pm_mfma_gemm_lat.hip; LinearArgs::m_live / m_est, d3pm_op_linear_live_est).

The latency family forced for a capacity of 768 rows (gemm_variant = 4) in each of its three tile geometries (lat_tile 1 / 2 / 3 = 64,
96 and 32 rows), f16 and bf16, the three projection shapes of a block (K = 2048 streams eight 256-k rounds), the four epilogue sets
the deduplicated loop runs on it, live counts around every tile edge and estimates that make the grid smaller than, equal to and larger
than the live tiles (0 = no estimate: the capacity's grid).  Rows below the live count, and their moment parts, equal the same
projection over all rows on the 128 x 128 family bit for bit; every row from the end of the last live tile on keeps the sentinel the
output was filled with.  The dual cross-attention out-projection goes through the same entry (its second operand) against the two
launches of the 128 x 128 family."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = 768
LIVES = (1, 31, 32, 33, 95, 96, 97, 383, 384, 385, 768)
ESTIMATES = (0, 32, 384, 768)
EPILOGUES = ("plain", "lnf", "r1_stats", "r1_mask_stats")
TILE_ROWS = {1: 64, 2: 96, 3: 32}
SENTINEL = 9.0


@pytest.fixture(scope="module")
def operands(built_lib):
    cache = {}

    def get(dtype, N, K):
        if (dtype, N, K) not in cache:
            gen = torch.Generator().manual_seed(1000 * N + K)
            r = lambda *s: (torch.randn(*s, generator=gen) * 0.3).to(dtype).to(DEV)      # noqa: E731
            cache[(dtype, N, K)] = {"x": r(M, K), "x2": r(M, K), "w": r(N, K), "b": r(N), "res": r(M, N),
                                    "fs": torch.randn(N, generator=gen).to(DEV), "fb": torch.randn(N, generator=gen).to(DEV),
                                    "mask": (torch.rand(M, generator=gen) < 0.7).to(torch.uint8).to(DEV)}
        return cache[(dtype, N, K)]
    return get


def _reference(o, epi):
    """(y, moment parts [M, N / 32, 2] or None) over all M rows on the 128 x 128 family, computed once per (operands, epilogue)"""
    from vall_e.vall_e import _hip
    if ("ref", epi) not in o:
        with _hip.tuning(gemm_variant=5):
            if epi == "plain":
                y, st = _hip.op_linear(o["x"], o["w"], o["b"]).contiguous(), None
            elif epi == "lnf":
                y, st = _hip.op_linear_fold(o["x"], o["w"], o["fs"], o["fb"], _hip.op_row_stats(o["x"])), None
            elif epi == "r1_stats":
                y, st = _hip.op_linear_stats(o["x"], o["w"], o["b"], o["res"])
            elif epi == "r1_mask_stats":
                y, st = _hip.op_linear_stats(o["x"], o["w"], o["b"], o["res"], row_mask=o["mask"], mask_period=M)
            else:      # dual: o_text -> h, then x' = (res + h) + o_prompt
                h = _hip.op_linear(o["x"], o["w"], o["b"]).contiguous()
                y, st = _hip.op_linear_stats(o["x2"], o["w"], o["b"], o["res"], r2=h)
        torch.cuda.synchronize()
        o[("ref", epi)] = (y, None if st is None else _hip.stats_rows(st, M).clone())
    return o[("ref", epi)]


def _live(o, epi, live, m_est):
    from vall_e.vall_e import _hip
    N = o["w"].shape[0]
    y = torch.full((M, N), SENTINEL, dtype=o["x"].dtype, device=DEV)
    st = torch.full((M // 16, N // 32, 16, 2), SENTINEL, dtype=torch.float32, device=DEV)
    m_live = torch.tensor([live], dtype=torch.int32, device=DEV)
    if epi == "plain":
        _hip.op_linear_live(o["x"], o["w"], o["b"], y, m_live, m_est=m_est)
    elif epi == "lnf":
        o.setdefault("parts", _hip.op_row_stats(o["x"]))
        _hip.op_linear_live(o["x"], o["w"], None, y, m_live, fold_s=o["fs"], fold_b=o["fb"], stats_in=o["parts"], m_est=m_est)
    elif epi == "r1_stats":
        _hip.op_linear_live(o["x"], o["w"], o["b"], y, m_live, r1=o["res"], stats_out=st, m_est=m_est)
    elif epi == "r1_mask_stats":
        _hip.op_linear_live(o["x"], o["w"], o["b"], y, m_live, r1=o["res"], row_mask=o["mask"], stats_out=st, m_est=m_est)
    else:
        _hip.op_linear_live(o["x"], o["w"], o["b"], y, m_live, x2=o["x2"], r1=o["res"], stats_out=st, m_est=m_est)
    return y, _hip.stats_rows(st, M)


def _check(o, epi, tile, what):
    ref_y, ref_st = _reference(o, epi)
    assert not (ref_y == SENTINEL).all(dim=1).any()
    for live in LIVES:
        for m_est in ESTIMATES:
            y, st = _live(o, epi, live, m_est)
            edge = (live + tile - 1) // tile * tile
            tag = (what, epi, "m_live", live, "m_est", m_est)
            assert torch.equal(y[:live], ref_y[:live]), tag
            assert (y[edge:] == SENTINEL).all(), tag + ("a row behind the last live tile was written",)
            if ref_st is not None:
                assert torch.equal(st[:live], ref_st[:live]), tag + ("moment parts",)
                assert (st[edge:] == SENTINEL).all(), tag + ("moments behind the last live tile were written",)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("lat_tile", [1, 2, 3])
@pytest.mark.parametrize("N,K", [(512, 512), (1536, 512), (512, 2048)])
def test_rows_below_the_live_count_equal_the_128_family(operands, dtype, lat_tile, N, K):
    from vall_e.vall_e import _hip
    o = operands(dtype, N, K)
    for epi in EPILOGUES:
        _reference(o, epi)
    with _hip.tuning(gemm_variant=4, lat_tile=lat_tile):
        for epi in EPILOGUES:
            _check(o, epi, TILE_ROWS[lat_tile], (str(dtype), lat_tile, N, K))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_dual_out_projection_on_a_live_count(operands, dtype):
    """d3pm_op_linear_live_est with a second operand reaches plan_cross_out: the 32 x 64 dual form of the latency family (automatic at
    this capacity), both products through one weight panel."""
    o = operands(dtype, 512, 512)
    _check(o, "dual", 32, (str(dtype), "dual"))

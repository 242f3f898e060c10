"""The self-attention with its keys read through a row index (include/d3pm_hip.h: d3pm_op_attention_gather; attn32p_hd64 GATHER,
csrc/d3pm_mfma_attn32.hip): what the deduplicated sampler loop launches instead of copying k | v rows back into canvas order.

Every expected value is made the same way: k[key_row[b]] / v[key_row[b]] materialised with torch (the index clamped into the pool, as
the kernel promises), then the fixed-stride kernel through _hip.op_attention(..., family=32, key_len=...) under attn_query_groups =
32, then torch.equal.  No tolerance is involved: the same key values arrive in the same order, so every bit is the same.

The key pool is the slice [8 : 8 + R] of a tensor with 8 guard rows on each side filled with 50: an index that escapes the clamp reads
a guard row, which changes bits instead of leaving the allocation.

Two utterances, two heads of 64 (d = 128), R = 384 pool rows; S = 64 ends in the prologue, 128 walks two tiles without staging a
third, 256 runs the loop with tiles staged two ahead and the clamp of the staged tile index behind the last one.

Two more cases at the kernel's design point: the geometry the loop launches at the benchmark's model (768 keys, 8 heads, [rows][3 d]
stride, query segments of 128 and 768 rows), and a pool of 3.07 GB -- strictly between 2^31 and 2^32 bytes -- in which key_row names
rows on both sides of byte 2^31, the row that straddles it and the last row, with indices beyond kv_rows - 1 that clamp onto it.  Only
the indexed rows of that pool are written; it is freed when the module is done."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, HD = 2, 2, 64
D = H * HD
R, GUARD = 384, 8
SCALE = 0.125
SENTINEL = -7.0
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]

_POOLS = {}


@pytest.fixture(autouse=True)
def _default_tuning(built_lib):
    from vall_e.vall_e import _hip
    _hip.reset_tuning()
    yield
    _hip.reset_tuning()


def _pool(dtype, width):
    """(k, v) = columns [width - 2 d : width - d] and [width - d : width] of the R live rows of a guarded [R + 16][width] pool, and
    queries [512][d]; made once per (dtype, width) and never written afterwards"""
    key = (dtype, width)
    if key not in _POOLS:
        gen = torch.Generator().manual_seed(11 + width)
        full = torch.full((R + 2 * GUARD, width), 50.0, dtype=dtype)
        full[GUARD:GUARD + R] = torch.randn(R, width, generator=gen).to(dtype)
        full = full.to(DEV)
        live = full[GUARD:GUARD + R]
        q = torch.randn(512, D, generator=gen).to(dtype).to(DEV)
        _POOLS[key] = (live[:, width - 2 * D:width - D], live[:, width - D:], q)
    return _POOLS[key]


def _index(kind, S, seed=0, R=R):
    gen = torch.Generator().manual_seed(100 + S + seed)
    if kind == "identity":      # consecutive rows per utterance: what the fixed-stride kernel walks
        idx = torch.stack([torch.arange(S) + b * (R - S) for b in range(B)])
    elif kind == "same":        # every key the same row
        idx = torch.stack([torch.full((S,), 5), torch.full((S,), R - 1)])
    elif kind == "random":      # duplicates, from the whole pool: also rows "of" the other utterance
        idx = torch.randint(0, R, (B, S), generator=gen)
        idx[:, 1] = idx[:, 0]
    else:                       # "outside": [-8, 0) and [R, R + 8) among valid ones
        idx = torch.randint(0, R, (B, S), generator=gen)
        lo = torch.randint(-GUARD, 0, (B, S), generator=gen)
        hi = torch.randint(R, R + GUARD, (B, S), generator=gen)
        pick = torch.randint(0, 3, (B, S), generator=gen)
        idx = torch.where(pick == 0, lo, torch.where(pick == 1, hi, idx))
        idx[0, 0], idx[0, S - 1], idx[1, 0], idx[1, S - 1] = -GUARD, R + GUARD - 1, R, -1
    return idx.to(torch.int32).to(DEV)


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _expected(q, k, v, key_row, seg_start, seg_len, key_len=None, heads=H):
    """per utterance: the fixed-stride 32 x 32 x 16 kernel on the materialised keys of its clamped index (the pool is k's rows)"""
    from vall_e.vall_e import _hip
    out = torch.full_like(q, SENTINEL)
    d = q.shape[1]
    idx = key_row.long().clamp(0, k.shape[0] - 1)
    with _hip.tuning(attn_query_groups=32):
        for b, (s0, n) in enumerate(zip(seg_start, seg_len)):
            kv = torch.cat([k[idx[b]], v[idx[b]]], dim=-1).unsqueeze(0).contiguous()      # [1, S, 2 d]
            kl = None if key_len is None else key_len[b:b + 1].contiguous()
            out[s0:s0 + n] = _hip.op_attention(q[s0:s0 + n].unsqueeze(0), kv[..., :d], kv[..., d:], heads, SCALE, family=32, key_len=kl)[0]
    return out


def _gathered(q, k, v, key_row, seg_start, seg_len, key_len=None, heads=H):
    from vall_e.vall_e import _hip
    out = torch.full_like(q, SENTINEL)
    _hip.op_attention_gather(q, k, v, key_row, _i32(seg_start), _i32(seg_len), heads, SCALE, out, key_len=key_len)
    return out


def _check(q, k, v, key_row, seg_start, seg_len, key_len=None, heads=H):
    want = _expected(q, k, v, key_row, seg_start, seg_len, key_len, heads)
    got = _gathered(q, k, v, key_row, seg_start, seg_len, key_len, heads)
    torch.cuda.synchronize()
    covered = torch.zeros(q.shape[0], dtype=torch.bool, device=DEV)
    for s0, n in zip(seg_start, seg_len):
        covered[s0:s0 + n] = True
    assert bool((want[covered] != SENTINEL).any()) and not bool(torch.isnan(want.float()).any())
    assert torch.equal(got[~covered], torch.full_like(got[~covered], SENTINEL)), "a row outside the segments was written"
    bad = (got != want).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"{len(bad)} rows differ from the fixed-stride kernel, first {bad[:8]}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["identity", "same", "random", "outside"])
@pytest.mark.parametrize("S", [64, 128, 256])
def test_key_counts(S, kind, dtype):
    k, v, q = _pool(dtype, 2 * D)
    _check(q[:256], k, v, _index(kind, S), (0, 128), (128, 128))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lens", [(256, 219), (64, 129), (1, 192)])
def test_key_lengths(lens, dtype):
    k, v, q = _pool(dtype, 2 * D)
    _check(q[:256], k, v, _index("outside", 256, seed=sum(lens)), (0, 128), (128, 128), key_len=_i32(lens))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_segments(dtype):
    """query capacity 256 per utterance, segments of 128 and 256 rows; rows 384 .. 511 belong to no segment and keep the sentinel"""
    k, v, q = _pool(dtype, 2 * D)
    _check(q, k, v, _index("random", 256, seed=3), (0, 128), (128, 256))
    _check(q, k, v, _index("outside", 128, seed=4), (0, 128), (128, 256), key_len=_i32((128, 77)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_packed_qkv_stride(dtype):
    """k / v as columns d : 2d and 2d : 3d of a [R][3d] pool: the layout the loop reads"""
    k, v, q = _pool(dtype, 3 * D)
    assert k.stride(0) == 3 * D and v.stride(0) == 3 * D
    _check(q[:256], k, v, _index("random", 256, seed=5), (0, 128), (128, 128))
    _check(q[:256], k, v, _index("outside", 192, seed=6), (0, 128), (128, 128), key_len=_i32((192, 65)))


# ---- the loop's own geometry ------------------------------------------------------------------------------------------------------
LOOP_H, LOOP_S, LOOP_R = 8, 768, 2048
LOOP_D = LOOP_H * HD


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["random", "outside"])
def test_loop_geometry(kind, dtype):
    """what the deduplicated loop launches at the benchmark's model: 768 keys per utterance (twelve tiles, the staged index 3 KiB behind
    the static tiles), 8 heads of 64, k / v the columns d : 2 d and 2 d : 3 d of a [rows][3 d] pool (2048 rows between 8 guard rows of 50
    on each side), two utterances with query segments of 128 and 768 rows"""
    gen = torch.Generator().manual_seed(21)
    full = torch.full((LOOP_R + 2 * GUARD, 3 * LOOP_D), 50.0, dtype=dtype)
    full[GUARD:GUARD + LOOP_R] = torch.randn(LOOP_R, 3 * LOOP_D, generator=gen).to(dtype)
    live = full.to(DEV)[GUARD:GUARD + LOOP_R]
    k, v = live[:, LOOP_D:2 * LOOP_D], live[:, 2 * LOOP_D:]
    assert k.stride(0) == 3 * LOOP_D and v.stride(0) == 3 * LOOP_D
    q = torch.randn(128 + 768, LOOP_D, generator=gen).to(dtype).to(DEV)
    _check(q, k, v, _index(kind, LOOP_S, seed=7, R=LOOP_R), (0, 128), (128, 768), heads=LOOP_H)


# ---- 32-bit byte offsets across 2^31 ----------------------------------------------------------------------------------------------
BIG_ROWS = 1_000_000                     # x 3 * 512 columns x 2 bytes = 3 072 000 000 bytes: between 2^31 and 2^32
BIG_LINE = 2 ** 31 // (3 * LOOP_D * 2)   # row 699 050 starts below byte 2^31 and ends above it
BIG_NAMED = [0, 1, 2 ** 30 // (3 * LOOP_D * 2), BIG_LINE - 1, BIG_LINE, BIG_LINE + 1, BIG_LINE + 2, BIG_ROWS - 2, BIG_ROWS - 1]
BIG_BEYOND = [BIG_ROWS, BIG_ROWS + 7, 2 ** 31 - 1]      # clamp onto the last row
BIG_BELOW = [-1, -2 ** 31]                              # clamp onto row 0


@pytest.fixture(scope="module")
def big_pool(built_lib):
    """one uninitialised allocation for both dtypes, freed when the module is done; only the rows a test indexes are ever written"""
    assert 2 ** 31 < BIG_ROWS * 3 * LOOP_D * 2 < 2 ** 32 and BIG_LINE * 3 * LOOP_D * 2 < 2 ** 31 < (BIG_LINE + 1) * 3 * LOOP_D * 2
    holder = [torch.empty((BIG_ROWS, 3 * LOOP_D), dtype=torch.int16, device=DEV)]
    yield holder
    holder.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_offsets_across_2_to_the_31_bytes(big_pool, dtype):
    """The design point of the 32-bit byte offsets: a pool of 3.07 GB.  key_row names rows on both sides of byte 2^31, the row that
    straddles it, the last row (whose v columns end with the allocation), and indices beyond kv_rows - 1 and below 0, which must clamp
    to the last and the first row.  An offset that went through a signed 32-bit intermediate would turn negative from row 699 051 on."""
    pool = big_pool[0].view(dtype)
    gen = torch.Generator().manual_seed(31)
    named = torch.tensor(BIG_NAMED)
    pool[named.to(DEV)] = torch.randn(len(named), 3 * LOOP_D, generator=gen).to(dtype).to(DEV)
    k, v = pool[:, LOOP_D:2 * LOOP_D], pool[:, 2 * LOOP_D:]
    S = 128
    choice = torch.tensor(BIG_NAMED + BIG_BEYOND + BIG_BELOW)
    idx = choice[torch.randint(0, len(choice), (B, S), generator=gen)]
    idx[0, :len(choice)] = choice                       # every one of them at least once, the straddling row in both utterances
    idx[1, S - len(choice):] = choice.flip(0)
    q = torch.randn(256, LOOP_D, generator=gen).to(dtype).to(DEV)
    key_row = idx.to(torch.int32).to(DEV)
    assert int(key_row.max()) == 2 ** 31 - 1 and int(key_row.min()) == -2 ** 31
    _check(q, k, v, key_row, (0, 128), (128, 128), heads=LOOP_H)
    _check(q, k, v, key_row, (0, 128), (128, 128), key_len=_i32((S, 65)), heads=LOOP_H)

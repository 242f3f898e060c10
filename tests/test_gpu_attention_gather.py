"""The self-attention with its keys read through a row index (include/d3pm_hip.h: d3pm_op_attention_gather; attn32p_hd64 GATHER,
csrc/d3pm_mfma_attn32.hip): what the deduplicated sampler loop launches instead of copying k | v rows back into canvas order.

Every expected value is made the same way: k[key_row[b]] / v[key_row[b]] materialised with torch (the index clamped into the pool, as
the kernel promises), then the fixed-stride kernel through _hip.op_attention(..., family=32, key_len=...) under attn_query_groups =
32, then torch.equal.  No tolerance is involved: the same key values arrive in the same order, so every bit is the same.

The key pool is the slice [8 : 8 + R] of a tensor with 8 guard rows on each side filled with 50: an index that escapes the clamp reads
a guard row, which changes bits instead of leaving the allocation.

Two utterances, two heads of 64 (d = 128), R = 384 pool rows; S = 64 ends in the prologue, 128 walks two tiles without staging a
third, 256 runs the loop with tiles staged two ahead and the clamp of the staged tile index behind the last one."""
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


def _index(kind, S, seed=0):
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


def _expected(q, k, v, key_row, seg_start, seg_len, key_len=None):
    """per utterance: the fixed-stride 32 x 32 x 16 kernel on the materialised keys of its clamped index"""
    from vall_e.vall_e import _hip
    out = torch.full_like(q, SENTINEL)
    idx = key_row.long().clamp(0, R - 1)
    with _hip.tuning(attn_query_groups=32):
        for b, (s0, n) in enumerate(zip(seg_start, seg_len)):
            kv = torch.cat([k[idx[b]], v[idx[b]]], dim=-1).unsqueeze(0).contiguous()      # [1, S, 2 d]
            kl = None if key_len is None else key_len[b:b + 1].contiguous()
            out[s0:s0 + n] = _hip.op_attention(q[s0:s0 + n].unsqueeze(0), kv[..., :D], kv[..., D:], H, SCALE, family=32, key_len=kl)[0]
    return out


def _gathered(q, k, v, key_row, seg_start, seg_len, key_len=None):
    from vall_e.vall_e import _hip
    out = torch.full_like(q, SENTINEL)
    _hip.op_attention_gather(q, k, v, key_row, _i32(seg_start), _i32(seg_len), H, SCALE, out, key_len=key_len)
    return out


def _check(q, k, v, key_row, seg_start, seg_len, key_len=None):
    want = _expected(q, k, v, key_row, seg_start, seg_len, key_len)
    got = _gathered(q, k, v, key_row, seg_start, seg_len, key_len)
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

"""The gathered self-attention with an utterance's distinct K | V rows pooled in LDS (include/d3pm_hip.h: d3pm_op_attention_gather_pool;
attn32p_hd64 POOL, csrc/d3pm_mfma_attn32.hip): what the deduplicated loop launches in the iterations that expect few rows per utterance.

Every expected value is d3pm_op_attention_gather on the same inputs, compared with torch.equal over the WHOLE output (rows no segment
owns keep the sentinel): the pool hands the walk the same key values in the same order, so no bit may differ.

The caller's promise -- the row named through key_row and the one named through seg_key / pool_src hold the same bytes -- is kept by
construction.  Without pool_src (blocks 1 .. of the loop) key_row[b, j] = seg_start[b] + clamp(seg_key[b, j] - seg_start[b], 0,
seg_len[b] - 1): the index the pool resolves, written out.  With pool_src (block 0: the class of a compact row) key_row[b, j] =
pool_src[that row]: another index than seg_key that names equal rows, classes beyond kv_rows - 1 included (both sides clamp).

Pool, guards, heads and index kinds are those of tests/test_gpu_attention_gather.py: 384 pool rows between guard rows of 50, two
utterances x two heads of 64.  S = 64 ends in the prologue, 128 walks two tiles, 256 runs the loop with the clamp of the staged tile."""
import pytest
import torch

import test_gpu_attention_gather as TG

pytestmark = pytest.mark.gpu
DEV, B, H, D, R, GUARD, SCALE, SENTINEL = TG.DEV, TG.B, TG.H, TG.D, TG.R, TG.GUARD, TG.SCALE, TG.SENTINEL
DTYPES, IDS = TG.DTYPES, TG.IDS
_i32 = TG._i32


@pytest.fixture(autouse=True)
def _default_tuning(built_lib):
    from vall_e.vall_e import _hip
    _hip.reset_tuning()
    yield
    _hip.reset_tuning()


def _seg_key(kind, S, starts, lens, seed=0):
    """[B, S] int32: the compact row of every canvas position"""
    gen = torch.Generator().manual_seed(300 + S + seed)
    rows = []
    for s0, n in zip(starts, lens):
        if kind == "identity":
            r = s0 + torch.arange(S) % n
        elif kind == "same":
            r = torch.full((S,), s0 + n - 1)
        elif kind == "random":      # duplicates
            r = s0 + torch.randint(0, n, (S,), generator=gen)
            r[1] = r[0]
        else:                       # "outside": rows in front of and behind the segment among its own: they clamp onto its ends
            r = s0 + torch.randint(-GUARD, n + GUARD, (S,), generator=gen)
            r[0], r[S - 1] = s0 - GUARD, s0 + n + GUARD - 1
        rows.append(r)
    return torch.stack(rows).to(torch.int32).to(DEV)


def _resolved(seg_key, starts, lens):
    """the row of k / v the pool reads for every key, without pool_src"""
    s0 = torch.tensor(starts, device=DEV).view(-1, 1)
    n = torch.tensor(lens, device=DEV).view(-1, 1)
    return (s0 + torch.minimum((seg_key.long() - s0).clamp(min=0), n - 1)).to(torch.int32)


def _run_pair(q, k, v, key_row, seg_key, starts, lens, heads, pool_rows, qblocks_grid, pool_src=None, key_len=None, pool_key_row=None):
    from vall_e.vall_e import _hip
    want = torch.full_like(q, SENTINEL)
    got = torch.full_like(q, SENTINEL)
    _hip.op_attention_gather(q, k, v, key_row, _i32(starts), _i32(lens), heads, SCALE, want, key_len=key_len)
    _hip.op_attention_gather_pool(q, k, v, key_row if pool_key_row is None else pool_key_row, seg_key, _i32(starts), _i32(lens), heads, SCALE, got,
                                  pool_rows=pool_rows, qblocks_grid=qblocks_grid, pool_src=pool_src, key_len=key_len)
    torch.cuda.synchronize()
    live = torch.zeros(q.shape[0], dtype=torch.bool, device=DEV)
    for s0, n in zip(starts, lens):
        live[s0:s0 + n] = True
    assert bool((want[live] != SENTINEL).any()) and not bool(torch.isnan(want.float()).any())
    bad = (got != want).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"{len(bad)} rows differ from d3pm_op_attention_gather, first {bad[:8]}"
    assert torch.equal(got, want)


def _check(dtype, S, kind, starts, lens, pool_rows=128, qblocks_grid=1, key_len=None, rows=256, seed=0):
    k, v, q = TG._pool(dtype, 2 * D)
    seg_key = _seg_key(kind, S, starts, lens, seed)
    _run_pair(q[:rows], k, v, _resolved(seg_key, starts, lens), seg_key, starts, lens, H, pool_rows, qblocks_grid, key_len=key_len)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["identity", "same", "random", "outside"])
@pytest.mark.parametrize("S", [64, 128, 256])
def test_key_counts(S, kind, dtype):
    _check(dtype, S, kind, (0, 128), (128, 77))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lens", [(1, 31), (32, 33), (127, 128)])
def test_segment_lengths(lens, dtype):
    _check(dtype, 256, "random", (0, lens[0]), lens, seed=sum(lens))
    _check(dtype, 128, "outside", (3, 3 + lens[0]), lens, rows=384, seed=sum(lens))      # segments at rows that are no multiple of anything


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lens", [(256, 219), (64, 129), (1, 192)])
def test_key_lengths(lens, dtype):
    _check(dtype, 256, "outside", (0, 128), (128, 90), key_len=_i32(lens), seed=sum(lens))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fallback_beside_pool(dtype):
    """129 rows do not fit a pool of 128: that utterance walks key_row (and two query blocks) beside one that is pooled, in one launch"""
    _check(dtype, 256, "random", (0, 100), (100, 129), seed=1)
    _check(dtype, 256, "outside", (0, 129), (129, 100), key_len=_i32((200, 256)), seed=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pooled_workgroup_reads_the_pool(dtype):
    """key_row handed to the pooled launch names row 0 for every key of the pooled utterance (a promise broken on purpose): the result is
    still that of the honest index, so those workgroups took their keys from the pool; the utterance of 129 rows keeps its honest key_row"""
    k, v, q = TG._pool(dtype, 2 * D)
    starts, lens = (0, 100), (100, 129)
    seg_key = _seg_key("random", 256, starts, lens, seed=9)
    honest = _resolved(seg_key, starts, lens)
    broken = honest.clone()
    broken[0] = 0
    assert not torch.equal(broken, honest)
    _run_pair(q[:256], k, v, honest, seg_key, starts, lens, H, 128, 1, pool_key_row=broken)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_workgroup_walks_three_query_blocks(dtype):
    """seg_len = 300 in a pool of 384 rows (145 KiB of LDS with the tiles) and one query block per (utterance, head) in the grid"""
    _check(dtype, 256, "random", (0, 300), (300, 84), pool_rows=384, qblocks_grid=1, rows=512, seed=4)
    _check(dtype, 128, "outside", (0, 300), (300, 84), pool_rows=384, qblocks_grid=1, rows=512, key_len=_i32((128, 70)), seed=5)


def _block0(dtype, k, v, q, S, starts, lens, heads, kv_rows, key_len=None, seed=0):
    """pool_src = the class of a compact row, classes beyond kv_rows - 1 among them; key_row = the class of a position"""
    gen = torch.Generator().manual_seed(500 + seed)
    n_rows = max(s0 + n for s0, n in zip(starts, lens))
    pool_src = torch.randint(0, kv_rows + GUARD, (n_rows,), generator=gen)
    pool_src[starts[0]], pool_src[starts[1]] = kv_rows + GUARD - 1, kv_rows      # both clamp onto the last row
    pool_src = pool_src.to(torch.int32).to(DEV)
    seg_key = _seg_key("random", S, starts, lens, seed)
    key_row = pool_src[seg_key.long()]
    assert not torch.equal(key_row, seg_key) and int(key_row.max()) >= kv_rows
    _run_pair(q, k, v, key_row, seg_key, starts, lens, heads, 128, 1, pool_src=pool_src, key_len=key_len)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_block0_form(dtype):
    k, v, q = TG._pool(dtype, 2 * D)
    _block0(dtype, k, v, q[:256], 256, (0, 128), (128, 61), H, R, seed=1)
    _block0(dtype, k, v, q[:256], 128, (5, 133), (128, 123), H, R, key_len=_i32((128, 65)), seed=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_loop_geometry(dtype):
    """what the loop launches at the benchmark's model in its first iterations: 768 keys, 8 heads of 64, k / v the columns d : 2 d and
    2 d : 3 d of a [rows][3 d] pool, dense segments of 2 and 120 rows; both forms"""
    heads, S, rows = TG.LOOP_H, TG.LOOP_S, TG.LOOP_R
    d = heads * TG.HD
    gen = torch.Generator().manual_seed(23)
    full = torch.full((rows + 2 * GUARD, 3 * d), 50.0, dtype=dtype)
    full[GUARD:GUARD + rows] = torch.randn(rows, 3 * d, generator=gen).to(dtype)
    live = full.to(DEV)[GUARD:GUARD + rows]
    k, v = live[:, d:2 * d], live[:, 2 * d:]
    assert k.stride(0) == 3 * d and v.stride(0) == 3 * d
    q = torch.randn(128, d, generator=gen).to(dtype).to(DEV)
    starts, lens = (0, 2), (2, 120)
    seg_key = _seg_key("random", S, starts, lens, seed=7)
    _run_pair(q, k, v, _resolved(seg_key, starts, lens), seg_key, starts, lens, heads, 128, 1)
    _block0(dtype, k, v, q, S, starts, lens, heads, rows, seed=8)

"""Dense segments of the deduplicated sampler loop (include/d3pm_hip.h: d3pm_op_dedup_index_align; csrc/d3pm_dedup.hip,
attn32p_hd64<.., SEG> in csrc/d3pm_mfma_attn32.hip): an utterance owns exactly its distinct classes, back to back, so a segment has
any length and starts at any row.

  * the index with seg_align = 1 against numpy (the reference of tests/test_gpu_dedup.py with pad = the class count), on that file's four
    token cases; seg_align = 128 through the new entry against d3pm_op_dedup_index, array for array; any other value is refused;
  * the gathered self-attention on segments that start and end inside a 128-query workgroup and inside a 32-query wave: every row of a
    segment equals the fixed-stride kernel on that utterance's materialised keys (the segment's queries padded to whole workgroups with
    finite rows: a row's bits do not depend on its block-mates, tests/test_gpu_dedup.py pins that), every other row of the output
    keeps the sentinel it was created with -- an unpredicated store of the workgroup that overhangs a segment would overwrite either the
    next utterance's rows or the rows behind the last segment -- and the queries behind the last segment are NaN, which must reach no
    stored row;
  * the segmented cross pair on the same segment lists against each utterance's rows alone, same sentinel and NaN rows;
  * the device-side live row count at counts that are no multiple of a tile (1, 65, 200, 385, 767), every epilogue the loop uses and
    the final layer: rows below the count equal the full launch, rows from the next tile boundary on keep the sentinel.

The loop itself is covered by the ln_fold = 1 against ln_fold = 3 cases of tests/test_gpu_dedup.py (ids and the trace of every iteration,
byte for byte; test_canvas_known_frames_keys_and_nucleus runs per-utterance lengths, 768 and 1 among them).

Every comparison is torch.equal / np.array_equal: no tolerance appears in this file."""
import numpy as np
import pytest
import torch

import test_gpu_attention_gather as TG
import test_gpu_dedup as TD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0
SCALE = 0.125
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
# (start, len) of two utterances, back to back: one row and a segment across a workgroup edge; a segment that ends one row past a wave;
# 127 | 129 around the workgroup edge; a whole number of workgroups followed by one row less; the aligned layout
SEGMENTS = [((0, 1), (1, 130)), ((0, 33), (33, 95)), ((0, 127), (127, 129)), ((0, 256), (256, 255)), ((0, 128), (128, 128))]
SEG_IDS = ["1_130", "33_95", "127_129", "256_255", "128_128"]

gemm_operands = TD.gemm_operands      # the operands of the live-count tests of tests/test_gpu_dedup.py (M = 768), one copy for this module


@pytest.fixture(autouse=True)
def _default_tuning(built_lib):
    from vall_e.vall_e import _hip
    _hip.reset_tuning()
    yield
    _hip.reset_tuning()


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


# ---- the index ------------------------------------------------------------------------------------------------------------------
def _index_ref(tokens, fmask, n_classes, align):
    """tests/test_gpu_dedup.py:_index_ref with the segment granularity as an argument (align = 1: pad = len(reps))"""
    batch, canvas = tokens.shape
    seg_start, seg_len, row_of, cid, cmask = [], [], np.zeros((batch, canvas), np.int64), [], []
    start = 0
    for b in range(batch):
        cls = np.where(fmask[b] != 0, np.clip(tokens[b], 0, n_classes - 1), n_classes)
        _, first = np.unique(cls, return_index=True)
        reps = np.sort(first)
        rank = {int(cls[p]): k for k, p in enumerate(reps)}
        row_of[b] = [start + rank[int(c)] for c in cls]
        pad = (len(reps) + align - 1) // align * align
        cid += [int(cls[p]) for p in reps] + [n_classes] * (pad - len(reps))
        cmask += [int(cls[p] != n_classes) for p in reps] + [0] * (pad - len(reps))
        seg_start.append(start)
        seg_len.append(pad)
        start += pad
    m_pad = (start + 383) // 384 * 384
    cid += [n_classes] * (m_pad - start)
    cmask += [0] * (m_pad - start)
    return np.array(seg_start), np.array(seg_len), start, row_of.reshape(-1), np.array(cid), np.array(cmask)


def _table(n_classes, d):
    return (torch.randn(n_classes, d, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("case", ["equal", "distinct", "eight", "ragged"])
def test_dense_index_and_compact_embedding_against_numpy(built_lib, case):
    from vall_e.vall_e import _hip
    n_classes, d = 1025, 512
    tokens, fmask = TD._index_inputs(case)
    table = _table(n_classes, d)
    got = _hip.op_dedup_index(torch.from_numpy(tokens).to(DEV), torch.from_numpy(fmask).to(DEV), n_classes, table, seg_align=1)
    torch.cuda.synchronize()
    seg_start, seg_len, m_live, row_of, cid, cmask = _index_ref(tokens, fmask, n_classes, 1)
    assert np.array_equal(got["seg_start"].cpu().numpy(), seg_start) and np.array_equal(got["seg_len"].cpu().numpy(), seg_len)
    assert np.array_equal(seg_start, np.concatenate([[0], np.cumsum(seg_len)[:-1]]))      # the exclusive prefix sum of the counts
    assert int(got["m_live"].item()) == m_live == seg_len.sum()
    m_pad = len(cid)
    if case == "equal":
        assert (seg_len == 1).all() and m_live == 4 and m_pad == 384
    if case == "distinct":
        assert m_live == tokens.size == m_pad
    if case == "ragged":      # 768 live frames of 40 ids, one live frame + the padded class, ...: lengths that are no multiple of anything
        assert seg_len[1] == 2 and (seg_len % 128 != 0).all()
    assert np.array_equal(got["row_of"].cpu().numpy(), row_of)
    assert np.array_equal(got["cid"].cpu().numpy()[:m_pad], cid) and np.array_equal(got["cmask"].cpu().numpy()[:m_pad], cmask)
    # a position's compact row carries its class; no unowned row inside a segment; rows the index does not define keep their sentinels
    cls = np.where(fmask != 0, np.clip(tokens, 0, n_classes - 1), n_classes).reshape(-1)
    assert np.array_equal(cid[row_of], cls)
    assert np.array_equal(np.unique(row_of), np.arange(m_live)), "a compact row below m_live that no position maps to"
    assert (got["cid"].cpu().numpy()[m_pad:] == -7).all() and (got["cmask"].cpu().numpy()[m_pad:] == 7).all() and (got["x"][m_pad:] == 3.0).all()
    assert (got["stats"].view(-1, 4, 16, 2)[m_pad // 16:] == 5.0).all()
    # the compact embedding: the table row of a live class, zeros on padded / unowned rows, and the moments of exactly those rows
    x = got["x"][:m_pad]
    ref = torch.where(torch.from_numpy(cmask).to(DEV).bool()[:, None], table[torch.from_numpy(np.minimum(cid, n_classes - 1)).to(DEV)], torch.zeros_like(x))
    assert torch.equal(x, ref)
    quads = got["stats"].view(-1, 4, 16, 2)[: m_pad // 16].permute(0, 2, 1, 3).reshape(m_pad, 4, 2)
    parts = _hip.stats_rows(_hip.op_row_stats(x.contiguous()), m_pad)                  # [m_pad, 16, 2]
    want = ((parts[:, 0::4] + parts[:, 1::4]) + parts[:, 2::4]) + parts[:, 3::4]
    assert torch.equal(quads, want)
    dead = torch.from_numpy(cmask == 0).to(DEV)
    assert (x[dead] == 0).all() and (quads[dead] == 0).all()
    assert (x[m_live:] == 0).all() and (quads[m_live:] == 0).all()


def _old_entry(tokens, frame_mask, n_classes, table):
    """d3pm_op_dedup_index itself, into the arrays _hip.op_dedup_index creates (the wrapper routes to the new entry)"""
    from vall_e.vall_e import _hip
    batch, canvas = tokens.shape
    n, d = batch * canvas, table.shape[1]
    i32 = lambda k, fill: torch.full((k,), fill, dtype=torch.int32, device=DEV)      # noqa: E731
    out = {"seg_start": i32(batch, -1), "seg_len": i32(batch, -1), "m_live": i32(1, -1), "row_of": i32(n, -1), "cid": i32(n, -7),
           "cmask": torch.full((n,), 7, dtype=torch.uint8, device=DEV), "x": torch.full((n, d), 3.0, dtype=table.dtype, device=DEV),
           "stats": torch.full((((n + 15) // 16) * 16 * (d // 32) * 2,), 5.0, dtype=torch.float32, device=DEV)}
    scratch = i32(n + batch, 0)
    p = _hip._p
    _hip.check(_hip.lib().d3pm_op_dedup_index(_hip.dtype_code(table.dtype), p(tokens), p(frame_mask), batch, canvas, n_classes, d, p(table),
                                              p(out["seg_start"]), p(out["seg_len"]), p(out["m_live"]), p(out["row_of"]), p(out["cid"]),
                                              p(out["cmask"]), p(out["x"]), p(out["stats"]), p(scratch), _hip.stream_ptr()), "d3pm_op_dedup_index")
    return out


@pytest.mark.parametrize("case", ["equal", "distinct", "eight", "ragged"])
def test_align_128_through_the_new_entry_equals_the_old_entry(built_lib, case):
    from vall_e.vall_e import _hip
    n_classes = 1025
    tokens, fmask = (torch.from_numpy(t).to(DEV) for t in TD._index_inputs(case))
    table = _table(n_classes, 512)
    new = _hip.op_dedup_index(tokens, fmask, n_classes, table, seg_align=128)
    old = _old_entry(tokens, fmask, n_classes, table)
    torch.cuda.synchronize()
    assert set(new) == set(old)
    for name in old:
        assert torch.equal(new[name], old[name]), name
    assert bool((old["seg_len"] % 128 == 0).all())


@pytest.mark.parametrize("seg_align", [0, 2, 64, 127, 256, -1])
def test_other_alignments_are_refused(built_lib, seg_align):
    from vall_e.vall_e import _hip
    tokens, fmask = (torch.from_numpy(t).to(DEV) for t in TD._index_inputs("eight"))
    with pytest.raises(_hip.D3PMError):
        _hip.op_dedup_index(tokens, fmask, 1025, _table(1025, 512), seg_align=seg_align)
    torch.cuda.synchronize()


# ---- attention ------------------------------------------------------------------------------------------------------------------
def _covered(rows, segs):
    covered = torch.zeros(rows, dtype=torch.bool, device=DEV)
    for s0, n in segs:
        assert not bool(covered[s0:s0 + n].any()), "the test's own segments overlap"
        covered[s0:s0 + n] = True
    return covered


def _poisoned(q, segs):
    """a copy of q whose rows behind the last segment are NaN"""
    q = q.clone()
    q[max(s0 + n for s0, n in segs):] = float("nan")
    return q


def _verdict(what, got, want, covered):
    assert bool(torch.isfinite(want[covered].float()).all()) and not bool((want[covered] == SENTINEL).all(dim=1).any()), what
    stray = (got[~covered] != SENTINEL).any(dim=1).nonzero().flatten().tolist()
    assert not stray, f"{what}: {len(stray)} rows outside the segments were written, first {[int((~covered).nonzero()[i]) for i in stray[:8]]}"
    assert not bool(torch.isnan(got.float()).any()), f"{what}: a NaN query behind the last segment reached a stored row"
    bad = (got != want).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"{what}: {len(bad)} rows differ, first {bad[:8]}"


def _expected_self(q, k, v, key_row, segs, key_len):
    """per utterance: the fixed-stride 32 x 32 x 16 kernel on the materialised keys of its clamped index (TG._expected), the segment's
    queries padded to whole 128-query workgroups with copies of its last row"""
    from vall_e.vall_e import _hip
    out = torch.full_like(q, SENTINEL)
    d = q.shape[1]
    idx = key_row.long().clamp(0, k.shape[0] - 1)
    with _hip.tuning(attn_query_groups=32):
        for b, (s0, n) in enumerate(segs):
            kv = torch.cat([k[idx[b]], v[idx[b]]], dim=-1).unsqueeze(0).contiguous()      # [1, S, 2 d]
            kl = None if key_len is None else key_len[b:b + 1].contiguous()
            whole = (n + 127) // 128 * 128
            qs = torch.cat([q[s0:s0 + n], q[s0 + n - 1:s0 + n].repeat(whole - n, 1)]).unsqueeze(0).contiguous()
            out[s0:s0 + n] = _hip.op_attention(qs, kv[..., :d], kv[..., d:], TG.H, SCALE, family=32, key_len=kl)[0, :n]
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("masked", [False, True], ids=["all_keys", "key_len"])
@pytest.mark.parametrize("S", [64, 128, 256])
@pytest.mark.parametrize("segs", SEGMENTS, ids=SEG_IDS)
def test_gathered_self_attention_on_dense_segments(segs, S, masked, dtype):
    """two utterances, two heads of 64, a pool of 384 rows, 512 query rows (capacity 512 per utterance: four workgroups, of which those
    behind the segment leave at once and the one across its end clamps and predicates)"""
    from vall_e.vall_e import _hip
    k, v, q = TG._pool(dtype, 2 * TG.D)
    q = _poisoned(q, segs)
    key_row = TG._index("outside", S, seed=17)
    key_len = _i32((S, S // 2 + 1)) if masked else None
    want = _expected_self(q, k, v, key_row, segs, key_len)
    got = torch.full_like(q, SENTINEL)
    _hip.op_attention_gather(q, k, v, key_row, _i32(s for s, _ in segs), _i32(n for _, n in segs), TG.H, SCALE, got, key_len=key_len)
    torch.cuda.synchronize()
    _verdict(f"self-attention, segments {segs}, {S} keys", got, want, _covered(q.shape[0], segs))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("masked", [False, True], ids=["all_keys", "key_len"])
@pytest.mark.parametrize("segs", SEGMENTS, ids=SEG_IDS)
def test_cross_pair_on_dense_segments(segs, masked, dtype):
    """two utterances x two heads, 50 text and 96 prompt keys (the smallest of tests/test_gpu_segment_ops.py), capacity 512: each
    utterance's rows against the same rows run alone as a [1, seg_len, d] problem"""
    from vall_e.vall_e import _hip
    H, d, S1, S2, cap = 2, 128, 50, 96, 512
    rows = cap + 128
    gen = torch.Generator().manual_seed(23 + segs[1][1])
    q1, q2 = (_poisoned(torch.randn(rows, d, generator=gen).to(dtype).to(DEV), segs) for _ in range(2))
    kv1, kv2 = (torch.randn(2, S, 2 * d, generator=gen).to(dtype).to(DEV) for S in (S1, S2))
    k1, v1, k2, v2 = kv1[..., :d], kv1[..., d:], kv2[..., :d], kv2[..., d:]
    l1, l2 = (_i32((1, 33)), _i32((65, 96))) if masked else (None, None)
    o1, o2 = (torch.full((rows, d), SENTINEL, dtype=dtype, device=DEV) for _ in range(2))
    w1, w2 = o1.clone(), o2.clone()
    with _hip.tuning(attn_cross_resident=5):
        _hip.op_attention_pair_segments(q1, k1, v1, q2, k2, v2, _i32(s for s, _ in segs), _i32(n for _, n in segs), H, SCALE, o1, o2, cap,
                                        key_len=l1, key_len2=l2)
        for b, (s0, n) in enumerate(segs):
            a1, a2 = _hip.op_attention_pair(q1[s0:s0 + n].unsqueeze(0), k1[b:b + 1], v1[b:b + 1], q2[s0:s0 + n].unsqueeze(0), k2[b:b + 1],
                                            v2[b:b + 1], H, SCALE, key_len=None if l1 is None else l1[b:b + 1].contiguous(),
                                            key_len2=None if l2 is None else l2[b:b + 1].contiguous())
            w1[s0:s0 + n], w2[s0:s0 + n] = a1[0], a2[0]
    torch.cuda.synchronize()
    covered = _covered(rows, segs)
    _verdict(f"cross pair (text), segments {segs}", o1, w1, covered)
    _verdict(f"cross pair (prompt), segments {segs}", o2, w2, covered)


# ---- live row counts that are no multiple of a tile -------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["lnf", "lnf_gelu", "r1_stats", "mask", "dual", "final"])
def test_live_row_count_inside_a_tile(gemm_operands, epi):
    """tests/test_gpu_dedup.py:test_live_row_count_from_device_memory at the counts dense segments produce: 192 x 128 tiles forced for
    the loop's epilogues, the final layer on the 128 x 128 one-tile-per-workgroup kernel"""
    from vall_e.vall_e import _hip
    o = gemm_operands
    M = o["M"]
    o.setdefault("quads", TD._quads_of(o["x"]))
    N = {"lnf": 1536, "final": 1025}.get(epi, 512)
    ld = 1032 if epi == "final" else N
    tile = 128 if epi == "final" else 192
    rows_of = lambda st: st.permute(0, 2, 1, 3).reshape(M, 4, 2)      # noqa: E731  quads [M / 16][4][16][2] -> [M][4][2]
    with _hip.tuning(gemm_variant=5 if epi == "final" else 8):
        def run(live):
            y = torch.full((M, ld), 9.0, dtype=torch.bfloat16, device=DEV)
            st = torch.full((M // 16, 4, 16, 2), 9.0, dtype=torch.float32, device=DEV)
            TD._live_call(o, epi, y[:, :N] if epi == "final" else y, st, torch.tensor([live], dtype=torch.int32, device=DEV))
            torch.cuda.synchronize()
            return y[:, :N], st
        full_y, full_st = run(M)
        assert not (full_y == 9.0).all(dim=1).any()
        for live in (1, 65, 200, 385, 767):
            y, st = run(live)
            edge = (live + tile - 1) // tile * tile
            assert torch.equal(y[:live], full_y[:live]), (epi, live)
            assert (y[edge:] == 9.0).all(), (epi, live, "a row behind the last live tile was written")
            if epi in ("r1_stats", "mask", "dual"):
                assert torch.equal(rows_of(st)[:live], rows_of(full_st)[:live]) and (st[edge // 16:] == 9.0).all(), (epi, live)

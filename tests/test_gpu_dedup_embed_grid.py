"""dedup_embed_rows on a fixed grid (csrc/d3pm_dedup.hip): every workgroup forms the segment prefix once (a wave scan per 256
utterances) and its waves stride over the canvas positions and the compact rows below m_pad.  d3pm_op_dedup_index_align at seg_align 1
and 128 against a numpy index built here, every output array with torch.equal / np.array_equal:

  * batch 3 x canvas 128 (n = 384: one 384-row tile, far fewer rows than waves in the grid), one utterance of one class, one with
    every position distinct, one fully padded;
  * batch 66 x canvas 128 (n = 8448 = 22 x 384): more utterances than lanes of a wave, the same three kinds among random ones.

Compared: seg_start, seg_len, m_live, row_of, cid, cmask, the compact embedding x and its moments -- zero rows and zero moments where a
segment is padding and from m_live to the next multiple of 384; the moments bit for bit against d3pm_op_row_stats of the expected rows
and, within the fp32 summation bound, against float64 sums in numpy -- and the sentinels of every row behind that, which nothing may write.
The same expectations hold for the one-wave-per-index kernel this one replaces: they describe the arrays, not the grid."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_CLASSES, D = 1025, 512
CANVAS = 128


@pytest.fixture(autouse=True)
def _default_tuning(built_lib):
    from vall_e.vall_e import _hip
    _hip.reset_tuning()
    yield
    _hip.reset_tuning()


def _inputs(batch):
    """tokens int32, frame mask uint8 [batch, CANVAS]: utterance 0 all one class, 1 every position distinct, 2 fully padded; the others
    (batch 66) cycle through those three kinds, a few ids on ragged lengths, and ids out of range"""
    gen = np.random.default_rng(batch)
    tokens = np.zeros((batch, CANVAS), np.int32)
    fmask = np.ones((batch, CANVAS), np.uint8)
    for b in range(batch):
        kind = b % 5
        if kind == 0:
            tokens[b] = 1024 if b == 0 else int(gen.integers(0, N_CLASSES))
        elif kind == 1:
            tokens[b] = gen.permutation(N_CLASSES)[:CANVAS]
        elif kind == 2:
            tokens[b] = gen.integers(0, N_CLASSES, CANVAS)
            fmask[b] = 0
        elif kind == 3:
            tokens[b] = gen.integers(0, 9, CANVAS)
            fmask[b, int(gen.integers(1, CANVAS)):] = 0
        else:
            tokens[b] = gen.integers(-5, N_CLASSES + 40, CANVAS)
    return tokens, fmask


def _index_ref(tokens, fmask, align):
    batch, canvas = tokens.shape
    seg_start, seg_len, row_of, cid, cmask = [], [], np.zeros((batch, canvas), np.int64), [], []
    start = 0
    for b in range(batch):
        cls = np.where(fmask[b] != 0, np.clip(tokens[b], 0, N_CLASSES - 1), N_CLASSES)
        _, first = np.unique(cls, return_index=True)
        reps = np.sort(first)                                   # the first position of each class, in position order
        rank = {int(cls[p]): k for k, p in enumerate(reps)}
        row_of[b] = [start + rank[int(c)] for c in cls]
        pad = (len(reps) + align - 1) // align * align
        cid += [int(cls[p]) for p in reps] + [N_CLASSES] * (pad - len(reps))
        cmask += [int(cls[p] != N_CLASSES) for p in reps] + [0] * (pad - len(reps))
        seg_start.append(start)
        seg_len.append(pad)
        start += pad
    m_pad = (start + 383) // 384 * 384
    cid += [N_CLASSES] * (m_pad - start)
    cmask += [0] * (m_pad - start)
    return np.array(seg_start), np.array(seg_len), start, row_of.reshape(-1), np.array(cid), np.array(cmask)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("align", [1, 128])
@pytest.mark.parametrize("batch", [3, 66])
def test_index_arrays_and_compact_embedding_against_numpy(batch, align, dtype):
    from vall_e.vall_e import _hip
    tokens, fmask = _inputs(batch)
    n = batch * CANVAS
    assert n % 384 == 0
    table = (torch.randn(N_CLASSES, D, generator=torch.Generator().manual_seed(1)) * 0.5).to(dtype).to(DEV)
    got = _hip.op_dedup_index(torch.from_numpy(tokens).to(DEV), torch.from_numpy(fmask).to(DEV), N_CLASSES, table, seg_align=align)
    torch.cuda.synchronize()
    seg_start, seg_len, m_live, row_of, cid, cmask = _index_ref(tokens, fmask, align)
    m_pad = len(cid)
    assert m_live <= m_pad <= n
    if align == 1:
        assert seg_len[0] == 1 and seg_len[1] == CANVAS and seg_len[2] == 1
        assert batch == 3 or m_pad < n, "the larger case is to leave rows behind m_pad"
    else:
        assert (seg_len == 128).all() and m_live == n

    def i64(name):
        return got[name].cpu().numpy().astype(np.int64)

    assert np.array_equal(i64("seg_start"), seg_start), "seg_start"
    assert np.array_equal(i64("seg_len"), seg_len), "seg_len"
    assert int(got["m_live"].item()) == m_live
    assert np.array_equal(i64("row_of"), row_of), "row_of"
    assert np.array_equal(i64("cid")[:m_pad], cid), "cid"
    assert np.array_equal(i64("cmask")[:m_pad], cmask), "cmask"
    # rows behind m_pad: nothing is written
    assert (i64("cid")[m_pad:] == -7).all() and (i64("cmask")[m_pad:] == 7).all() and bool((got["x"][m_pad:] == 3.0).all())
    assert bool((got["stats"].view(-1, 4, 16, 2)[m_pad // 16:] == 5.0).all())
    # the compact embedding and its moments (quads of 128 columns, 16-row groups: the layout of the d = 512 loop)
    x = got["x"][:m_pad]
    live = torch.from_numpy(cmask).to(DEV).bool()
    want_x = torch.where(live[:, None], table[torch.from_numpy(np.minimum(cid, N_CLASSES - 1)).to(DEV)], torch.zeros_like(x))
    assert torch.equal(x, want_x), "x"
    quads = got["stats"].view(-1, 4, 16, 2)[: m_pad // 16].permute(0, 2, 1, 3).reshape(m_pad, 4, 2)
    parts = _hip.stats_rows(_hip.op_row_stats(want_x.contiguous()), m_pad)      # [m_pad, 16, 2]: moments of 32-column parts
    want_q = ((parts[:, 0::4] + parts[:, 1::4]) + parts[:, 2::4]) + parts[:, 3::4]
    assert torch.equal(quads, want_q), "stats"
    # the same moments in numpy, float64, from the expected rows alone: (sum, sum of squares) of each 128-column quad.  The kernel adds
    # 128 fp32 terms in some order, every product exact (16-bit factors): |error| <= 127 * 2^-24 * the sum of the terms' magnitudes
    v = want_x.float().cpu().numpy().astype(np.float64).reshape(m_pad, 4, 128)
    got_q = quads.cpu().numpy().astype(np.float64)
    bound = 127 * 2.0 ** -24
    assert (np.abs(got_q[..., 0] - v.sum(-1)) <= bound * np.abs(v).sum(-1)).all(), "stats: sums against numpy"
    assert (np.abs(got_q[..., 1] - (v * v).sum(-1)) <= bound * (v * v).sum(-1)).all(), "stats: sums of squares against numpy"
    assert bool((x[~live] == 0).all()) and bool((quads[~live] == 0).all())
    assert bool((x[m_live:] == 0).all()) and bool((quads[m_live:] == 0).all())

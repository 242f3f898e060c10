"""The kernels only the deduplicated sampler loop launches, each through a test entry of its own (include/d3pm_hip.h):

  * d3pm_op_attention_pair_segments -- attn32_cross_hd64<.., SEG> (csrc/d3pm_mfma_attn32.hip), the resident 32 x 32 x 16 cross pair with
    query segments, masked and unmasked.  Every expected value is the fixed-stride kernel (_hip.op_attention_pair under
    attn_cross_resident = 5) on one utterance's segment rows alone, a [1, seg_len, d] problem, compared with torch.equal: a row's bits do
    not depend on its block-mates (tests/test_gpu_dedup.py pins that).  The outputs start as a sentinel, and every row no segment owns
    must still hold it: the kernel walks 256-query blocks over segments that are multiples of 128, so a segment of 128, 384 or 640 rows
    ends in a half-filled block whose other half belongs to the next utterance.  Two grids: n_qsplit = n_qblocks (3 utterances x 2
    heads) and the benchmark's n_qsplit = 1 (32 utterances x 8 heads: one workgroup walks every block of its utterance, the next
    block's queries fetched under the current one).
  * the selector anchor, the one expectation that is not kernel against kernel: attention_ref.selector_inputs make the softmax one-hot, so
    every output row of the segment pair and of the gathered self-attention (d3pm_op_attention_gather, its pool rows shuffled and
    key_row the inverse permutation) must be a V row, bit for bit.
  * d3pm_op_posterior_sample_rows -- dedup_sample_rows / _filtered / _top_p, kKnown on and off (csrc/d3pm_sample.hip): canvas row r
    draws from the logits of compact row row_of[r].  Id for id it must equal the existing posterior-sample entries on
    logits_c[row_of.clamp(0, rows - 1)]: the index is clamped, the Philox row stays the canvas row (many rows share few logits rows
    and must still draw their own noise), a known row returns x_t and touches neither its index nor any logits (its index points at
    a NaN row), the second output equals the first.  Compact rows no index names hold NaN.  One anchor against the CPU oracle's
    posterior and Philox noise on the reference's own logits, under the criterion of test_gpu_parity.py: no id differs.

No tolerance appears in this file."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_ref as R
from oracle import d3pm_oracle as O
from oracle import philox
from util import f16, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 0.125
SENTINEL = -7.0
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
CAP = 768


@pytest.fixture(autouse=True)
def _default_tuning(built_lib):
    from vall_e.vall_e import _hip
    _hip.reset_tuning()
    yield
    _hip.reset_tuning()


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


# ---- cross pair with segments ---------------------------------------------------------------------------------------------------
def _back_to_back(lens):
    starts, s = [], 0
    for n in lens:
        starts.append(s)
        s += n
    return starts


def _packed(Bn, S, d, dtype, gen, key_len=None):
    """K | V as one [B, S, 2 d] device tensor; with key_len the rows at and past it hold finite poison (K = 240: a masked score would be
    the largest by far; V = 3e4), as in test_key_len_equals_the_truncated_problem"""
    kv = torch.randn(Bn, S, 2 * d, generator=gen).to(dtype)
    if key_len is not None:
        for b, n in enumerate(key_len):
            kv[b, n:, :d] = 240.0
            kv[b, n:, d:] = 3e4
    return kv.to(DEV)


def _check_pair(dtype, H, lens, starts, S1, S2, seed, kl1=None, kl2=None, tail=128):
    """the segment launch against every utterance alone; rows outside the segments keep the sentinel"""
    from vall_e.vall_e import _hip
    Bn, d = len(lens), H * R.HD
    rows = max(s + n for s, n in zip(starts, lens)) + tail
    gen = torch.Generator().manual_seed(seed)
    q1, q2 = (torch.randn(rows, d, generator=gen).to(dtype).to(DEV) for _ in range(2))
    kv1, kv2 = _packed(Bn, S1, d, dtype, gen, kl1), _packed(Bn, S2, d, dtype, gen, kl2)
    k1, v1, k2, v2 = kv1[..., :d], kv1[..., d:], kv2[..., :d], kv2[..., d:]
    l1, l2 = (None if kl is None else _i32(kl) for kl in (kl1, kl2))
    o1, o2 = (torch.full((rows, d), SENTINEL, dtype=dtype, device=DEV) for _ in range(2))
    w1, w2 = o1.clone(), o2.clone()
    with _hip.tuning(attn_cross_resident=5):
        _hip.op_attention_pair_segments(q1, k1, v1, q2, k2, v2, _i32(starts), _i32(lens), H, SCALE, o1, o2, CAP, key_len=l1, key_len2=l2)
        for b, (s0, n) in enumerate(zip(starts, lens)):
            a1, a2 = _hip.op_attention_pair(q1[s0:s0 + n].unsqueeze(0), k1[b:b + 1], v1[b:b + 1], q2[s0:s0 + n].unsqueeze(0), k2[b:b + 1],
                                            v2[b:b + 1], H, SCALE, key_len=None if l1 is None else l1[b:b + 1].contiguous(),
                                            key_len2=None if l2 is None else l2[b:b + 1].contiguous())
            w1[s0:s0 + n], w2[s0:s0 + n] = a1[0], a2[0]
    torch.cuda.synchronize()
    covered = torch.zeros(rows, dtype=torch.bool, device=DEV)
    for s0, n in zip(starts, lens):
        assert not bool(covered[s0:s0 + n].any()), "the test's own segments overlap"
        covered[s0:s0 + n] = True
    what = f"lens {tuple(lens)[:6]} starts {tuple(starts)[:6]} keys {S1}/{S2} lengths {kl1 and tuple(kl1)[:4]}/{kl2 and tuple(kl2)[:4]}"
    for side, got, want in (("text", o1, w1), ("prompt", o2, w2)):
        assert bool(torch.isfinite(want.float()).all()) and not bool((want[covered] == SENTINEL).all(dim=1).any()), (side, what)
        stray = (got[~covered] != SENTINEL).any(dim=1).nonzero().flatten().tolist()
        assert not stray, f"{side}: {len(stray)} rows outside the segments were written, first {[int((~covered).nonzero()[i]) for i in stray[:8]]}; {what}"
        bad = (got != want).any(dim=1).nonzero().flatten().tolist()
        assert not bad, f"{side}: {len(bad)} rows differ from the utterance alone, first {bad[:8]}; {what}"


SMALL_LAYOUTS = [((128, 384, 768), None), ((640, 128, 256), None), ((384, 128, 640), (0, 512, 896))]      # (lens, starts; None = back to back)
SMALL_KEYS = [(64, 225), (50, 96), (64, 256)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_segment_pair_small_grid(dtype):
    """3 utterances x 2 heads: n_qsplit = n_qblocks = 3, one workgroup per 256-query block.  Back to back, the half-filled last block
    of a 128-, 384- or 640-row segment is followed directly by the next utterance's live rows; the third layout leaves gaps of 128
    rows (which must keep the sentinel) in front of the second and the third segment."""
    for i, (lens, starts) in enumerate(SMALL_LAYOUTS):
        for j, (S1, S2) in enumerate(SMALL_KEYS):
            _check_pair(dtype, 2, lens, starts or _back_to_back(lens), S1, S2, seed=10 * i + j)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_segment_pair_small_grid_with_key_lengths(dtype):
    """the same layouts under key_len1 / key_len2, a text length of 1 and a prompt length of 65 among them"""
    lengths = [((1, 50, 64), (65, 225, 96)), ((64, 1, 33), (256, 65, 1)), ((17, 64, 1), (129, 256, 65))]
    for i, (lens, starts) in enumerate(SMALL_LAYOUTS):
        kl1, kl2 = lengths[i]
        _check_pair(dtype, 2, lens, starts or _back_to_back(lens), 64, 256, seed=40 + i, kl1=kl1, kl2=kl2)
    _check_pair(dtype, 2, SMALL_LAYOUTS[0][0], _back_to_back(SMALL_LAYOUTS[0][0]), 50, 225, seed=44, kl1=(50, 1, 7), kl2=None)
    _check_pair(dtype, 2, SMALL_LAYOUTS[1][0], _back_to_back(SMALL_LAYOUTS[1][0]), 64, 225, seed=45, kl1=None, kl2=(65, 225, 2))


BENCH_B, BENCH_H = 32, 8
BENCH_LENS = [(128, 256, 384, 640, 768)[b % 5] for b in range(BENCH_B)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_segment_pair_benchmark_grid(dtype):
    """32 utterances x 8 heads of 64 (d = 512), capacity 768, 64 text and 225 prompt keys: 256 (utterance, head) pairs cover the CUs, so
    n_qsplit = 1 and one workgroup walks every block of its segment.  Every utterance against itself alone."""
    _check_pair(dtype, BENCH_H, BENCH_LENS, _back_to_back(BENCH_LENS), 64, 225, seed=70)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_segment_pair_benchmark_grid_with_key_lengths(dtype):
    gen = torch.Generator().manual_seed(71)
    kl1 = torch.randint(1, 65, (BENCH_B,), generator=gen).tolist()
    kl2 = torch.randint(1, 226, (BENCH_B,), generator=gen).tolist()
    kl1[0], kl1[1], kl1[2], kl2[0], kl2[1], kl2[2] = 1, 64, 33, 65, 225, 1
    _check_pair(dtype, BENCH_H, BENCH_LENS, _back_to_back(BENCH_LENS), 64, 225, seed=72, kl1=kl1, kl2=kl2)


# ---- selector anchor --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_selector_returns_the_value_row_through_segments_and_through_the_key_index(dtype):
    """Query i is K row pi(i) of +-4 sign codes (attention_ref.selector_inputs): the softmax is one-hot below fp32 rounding, so output
    row i of utterance b is V[b, pi(i)] unchanged -- whatever block, segment or pool row it travelled through."""
    from vall_e.vall_e import _hip
    Bn, H = 3, 2
    d = H * R.HD
    lens = (128, 384, 768)
    starts = _back_to_back(lens)
    rows = sum(lens) + 128
    gen = torch.Generator().manual_seed(5)

    def flat_queries(q):      # [B, CAP, d] -> [rows, d]: the first seg_len[b] queries of utterance b at its segment
        out = torch.zeros(rows, d, dtype=dtype)
        for b, (s0, n) in enumerate(zip(starts, lens)):
            out[s0:s0 + n] = q[b, :n]
        return out.to(DEV)

    def verdict(name, got, v, pi):
        covered = torch.zeros(rows, dtype=torch.bool)
        for b, (s0, n) in enumerate(zip(starts, lens)):
            covered[s0:s0 + n] = True
            bad = (got[s0:s0 + n].cpu() != v[b, pi[:n]]).any(dim=1).nonzero().flatten().tolist()
            assert not bad, f"{name}: utterance {b}, {len(bad)} rows are not their V row, first {bad[:8]}"
        assert bool((got.cpu()[~covered] == SENTINEL).all()), f"{name}: a row outside the segments was written"

    # the segment pair: 50 text keys, 225 prompt keys
    q1, k1, pi1, gap1 = R.selector_inputs(Bn, H, CAP, 50, dtype, seed=1)
    q2, k2, pi2, gap2 = R.selector_inputs(Bn, H, CAP, 225, dtype, seed=2)
    assert float(gap1.min()) >= 40.0 and float(gap2.min()) >= 40.0
    v1, v2 = torch.randn(Bn, 50, d, generator=gen).to(dtype), torch.randn(Bn, 225, d, generator=gen).to(dtype)
    kv1, kv2 = torch.cat([k1, v1], -1).to(DEV), torch.cat([k2, v2], -1).to(DEV)
    o1, o2 = (torch.full((rows, d), SENTINEL, dtype=dtype, device=DEV) for _ in range(2))
    with _hip.tuning(attn_cross_resident=5):
        _hip.op_attention_pair_segments(flat_queries(q1), kv1[..., :d], kv1[..., d:], flat_queries(q2), kv2[..., :d], kv2[..., d:], _i32(starts),
                                        _i32(lens), H, SCALE, o1, o2, CAP)
    torch.cuda.synchronize()
    verdict("segment pair, text", o1, v1, pi1)
    verdict("segment pair, prompt", o2, v2, pi2)

    # the gathered self-attention: 256 keys per utterance, the pool rows shuffled, key_row the inverse permutation
    S = 256
    q, k, pi, gap = R.selector_inputs(Bn, H, CAP, S, dtype, seed=3)
    assert float(gap.min()) >= 40.0
    v = torch.randn(Bn, S, d, generator=gen).to(dtype)
    perm = torch.randperm(Bn * S, generator=gen)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(Bn * S)
    pool = torch.cat([k, v], -1).view(Bn * S, 2 * d)[perm].to(DEV)      # pool[inv[b * S + j]] = key j of utterance b
    out = torch.full((rows, d), SENTINEL, dtype=dtype, device=DEV)
    _hip.op_attention_gather(flat_queries(q), pool[:, :d], pool[:, d:], inv.view(Bn, S).to(torch.int32).to(DEV), _i32(starts), _i32(lens), H,
                             SCALE, out)
    torch.cuda.synchronize()
    verdict("gathered self-attention", out, v, pi)


# ---- sampler through row_of -------------------------------------------------------------------------------------------------------
T_STEPS = 100
# (n_classes, mask_id).  K = 1025 takes the predicate-free routine (sample_row_1025) when the mask id lies below 1024 -- the
# reference's 512 -- and the general sample_row otherwise, so (1025, 1024) and the smaller class count both run the general routine.
CLASSES = [(1025, 512), (1025, 1024), (301, 300)]
SHAPES = [(2, 768), (3, 513)]      # (batch, canvas): 1536 rows, and 1539 rows -- the last workgroup of four waves holds three


def _shape(canvas, K, mask_id, dtype):
    from vall_e.vall_e import _hip
    return _hip.Shape(512, 8, 2, canvas, 64, 225, K, mask_id, T_STEPS, _hip.dtype_code(dtype), 1, C.pointer(_hip.TUNING))


def _reference_ids(shape, sched, logits, x_t, t, seed, utt0, flags, known, smp):
    """the existing entry of the arm on logits [B, canvas, K]: d3pm_posterior_sample / _known / _sampling / _nucleus"""
    from vall_e.vall_e import _hip
    lib, p = _hip.lib(), (lambda x: None if x is None else C.c_void_p(x.data_ptr()))
    assert logits.is_contiguous() and tuple(logits.shape) == tuple(x_t.shape) + (shape.n_classes,)
    out = torch.empty_like(x_t)
    head = (C.byref(shape), x_t.shape[0], p(logits), _hip.dtype_code(logits.dtype), p(x_t), p(out))
    tail = (int(t), C.byref(sched.c_struct), seed, utt0, flags, None)
    st = _hip.stream_ptr()
    if isinstance(smp, _hip.Nucleus):
        _hip.check(lib.d3pm_posterior_sample_nucleus(*head, p(known), *tail, C.byref(smp), None, st), "d3pm_posterior_sample_nucleus")
    elif isinstance(smp, _hip.Sampling):
        _hip.check(lib.d3pm_posterior_sample_sampling(*head, p(known), *tail, C.byref(smp), st), "d3pm_posterior_sample_sampling")
    elif known is not None:
        _hip.check(lib.d3pm_posterior_sample_known(*head, p(known), *tail, st), "d3pm_posterior_sample_known")
    else:
        _hip.check(lib.d3pm_posterior_sample(*head, *tail, st), "d3pm_posterior_sample")
    return out


ARMS = [("plain", {}), ("greedy", {"greedy": True}), ("known", {"known": True}), ("known_greedy", {"known": True, "greedy": True}),
        ("filtered", {"temperature": 0.8, "top_k": 40}), ("filtered_known", {"temperature": 1.3, "top_k": 7, "known": True}),
        ("top_p", {"top_p": 0.9}), ("top_p_filtered_known", {"temperature": 0.9, "top_k": 50, "top_p": 0.8, "known": True})]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,mask_id", CLASSES, ids=[f"K{k}_mask{m}" for k, m in CLASSES])
def test_sampler_through_row_of_equals_the_plain_sampler_on_the_gathered_rows(K, mask_id, dtype):
    from vall_e.vall_e import _hip
    sched = _hip.Schedule(T_STEPS)
    for case, (Bn, canvas) in enumerate(SHAPES):
        shape = _shape(canvas, K, mask_id, dtype)
        rows = Bn * canvas
        gen = torch.Generator().manual_seed(1000 * case + K + mask_id)
        # few logits rows for many canvas rows: 37 compact rows scattered over the buffer, rows 0 and rows - 1 among them (where the
        # clamp lands); every other compact row holds NaN.  Row stride 8 columns wider than K, as in the loop's workspace.
        named = torch.cat([torch.tensor([0, rows - 1]), torch.randperm(rows - 2, generator=gen)[:35] + 1])
        ldl = (K + 7) // 8 * 8 + 8
        buf = torch.full((rows, ldl), float("nan"), dtype=dtype)
        buf[named, :K] = (torch.randn(len(named), K, generator=gen) * 3.0).to(dtype)
        row_of = named[torch.randint(0, len(named), (rows,), generator=gen)]
        outside = torch.rand(rows, generator=gen)
        row_of = torch.where(outside < 0.05, torch.randint(-2 ** 31, 0, (rows,), generator=gen), row_of)
        row_of = torch.where(outside > 0.95, torch.randint(rows, 2 ** 31 - 1, (rows,), generator=gen), row_of)
        row_of[3], row_of[rows - 1], row_of[5], row_of[rows - 2] = -1, rows, -2 ** 31, 2 ** 31 - 1
        x_t = torch.where(torch.rand(rows, generator=gen) < 0.6, torch.tensor(mask_id), torch.randint(0, K, (rows,), generator=gen))
        known = (torch.rand(rows, generator=gen) < 0.3).to(torch.uint8)
        known[rows - 1], known[0] = 1, 1
        # the known arms: a second buffer whose row 0 is NaN too.  A known row's index is out of range below (it would clamp onto
        # that row 0) or names a NaN row directly; the other rows keep indices that resolve to named rows behind row 0 (indices at or
        # above `rows` included: they clamp onto the named row rows - 1)
        taken = set(named.tolist())
        nan_row = next(r for r in range(1, rows) if r not in taken)
        buf_known = buf.clone()
        buf_known[0] = float("nan")
        is_known = known.bool()
        row_of_known = torch.where(torch.rand(rows, generator=gen) < 0.5, torch.tensor(nan_row), torch.tensor(-5))
        elsewhere = named[1:][torch.randint(0, len(named) - 1, (rows,), generator=gen)]
        row_of_known = torch.where(is_known, row_of_known, torch.where(row_of <= 0, elsewhere, row_of))
        dev = lambda t_, dt=None: (t_ if dt is None else t_.to(dt)).to(DEV)      # noqa: E731
        buf_d, buf_known_d = dev(buf), dev(buf_known)
        idx_d, idx_known_d = dev(row_of, torch.int32), dev(row_of_known, torch.int32)
        x_d = dev(x_t, torch.int32).view(Bn, canvas)
        known_d = dev(known).view(Bn, canvas)
        for name, arm in ARMS:
            kn = known_d if arm.get("known") else None
            lg, idx = (buf_known_d, idx_known_d) if kn is not None else (buf_d, idx_d)
            gathered = lg[idx.long().clamp(0, rows - 1)][:, :K].contiguous().view(Bn, canvas, K)
            if kn is None:
                assert not bool(torch.isnan(gathered.float()).any())
            else:
                assert bool(torch.isnan(gathered.float()[kn.bool()]).all()) and not bool(torch.isnan(gathered.float()[~kn.bool()]).any())
            opts = {k: v for k, v in arm.items() if k in ("temperature", "top_k", "top_p")}
            smp = _hip.nucleus_options(n_classes=K, **opts)
            flags = _hip.FLAG_GREEDY if arm.get("greedy") else 0
            for t in (99, 50, 1):
                utt0 = 3 + t
                got, second = _hip.op_posterior_sample_rows(shape, sched, lg[:, :K], idx, x_d, t, 77, utt0=utt0, flags=flags, known=kn,
                                                            want_second=True, **opts)
                want = _reference_ids(shape, sched, gathered, x_d, t, 77, utt0, flags, kn, smp)
                torch.cuda.synchronize()
                what = f"{name} t={t} rows={rows} K={K}"
                bad = (got != want).flatten().nonzero().flatten().tolist()
                assert not bad, f"{what}: {len(bad)} ids differ from the plain sampler on the gathered rows, first rows {bad[:8]}"
                assert torch.equal(second, got), f"{what}: the second output differs from the first"
                assert bool(((got >= 0) & (got < K)).all()), what
                if kn is not None:
                    assert torch.equal(got[kn.bool()], x_d[kn.bool()]), f"{what}: a known row did not keep x_t"
                if name == "plain" and t == 1:      # rows that share one logits row and one x_t still draw their own noise
                    same = (idx.long().clamp(0, rows - 1) == 0) & (x_d.flatten() == mask_id)
                    assert int(same.sum()) >= 8 and len(set(got.flatten()[same].tolist())) > 1, what


def test_sampler_through_row_of_against_the_oracle(built_lib):
    """The reference's own fp16 logits and x_t (tests/golden/native_step.npz), stored at permuted compact rows (NaN in the columns behind
    the classes): the ids must be the CPU oracle's -- its posterior (oracle.d3pm_oracle) plus Gumbel noise from oracle.philox -- with no mismatch, the
    criterion test_posterior_and_sample_on_reference_logits applies to the plain sampler; at utterance 0 they are also the ids the
    reference itself drew."""
    from vall_e.vall_e import _hip, synth
    cfg = synth.D3PMConfig.native()
    g = load("native_step.npz")
    logits, x_t, t = f16(g["logits_full_f16"]), torch.from_numpy(g["x_t"].astype(np.int64)), int(g["t"])
    canvas, K = logits.shape
    assert (canvas, K) == (cfg.canvas, cfg.n_classes)
    tabs = O.scalar_tables(O.cosine_betas(cfg.timesteps), cfg.timesteps)
    post = O.posterior_logits_closed(logits, x_t, t, tabs, cfg.mask_id)
    shape = _hip.Shape(cfg.d_model, cfg.n_heads, cfg.n_layers, canvas, cfg.s_text, cfg.s_prompt, K, cfg.mask_id, cfg.timesteps,
                       _hip.dtype_code(torch.float16), 1, C.pointer(_hip.TUNING))
    sched = _hip.Schedule(cfg.timesteps)
    perm = torch.randperm(canvas, generator=torch.Generator().manual_seed(3))
    buf = torch.full((canvas, K + 7), float("nan"), dtype=torch.float16)
    buf[perm, :K] = logits
    x_d = x_t.to(torch.int32).view(1, canvas).to(DEV)
    for utt0 in (0, 3):
        want = O.gumbel_argmax(post, torch.from_numpy(philox.uniform_batch(123, t, utt0, 1, canvas, K)[0]), t).numpy()
        got = _hip.op_posterior_sample_rows(shape, sched, buf.to(DEV)[:, :K], perm.to(torch.int32).to(DEV), x_d, t, 123, utt0=utt0)
        torch.cuda.synchronize()
        mism = int((got[0].cpu().numpy() != want).sum())
        assert mism == 0, f"utt0 = {utt0}: {mism} ids differ from the oracle's draw"
        if utt0 == 0:
            assert np.array_equal(want, g["x_next_seed123"].astype(np.int64))

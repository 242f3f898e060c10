"""One denoiser row per distinct token of an utterance (include/d3pm_hip.h: d3pm_tuning.ln_fold, d3pm_op_dedup_index,
d3pm_op_linear_live; csrc/d3pm_dedup.hip).

  * the index kernels against numpy: first-occurrence order, 128-row segments, row_of, the compact embedding and its zero rows;
  * the device-side live row count of the big-tile GEMM (every epilogue the loop uses) and of the final-layer kernel: rows below the
    count equal the full launch bit for bit, rows from the next tile boundary on keep a sentinel;
  * the sampler loops under ln_fold = 1 (deduplicated) and ln_fold = 3 (every row): final ids and the trace of every iteration,
    byte for byte, at the smallest shape that takes the path (16 utterances x 768 frames, d = 512, two layers); every variant also
    shows by the library's launch counters that its default really runs another launch list than ln_fold = 3, and the guided, reveal,
    fp8, n_q = 8 and one-utterance calls that theirs is the same one;
  * the 32 x 32 attention kernels: a query row's bits do not change when a wave-mate fires the deferred-maximum path.
"""
import contextlib
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, CANVAS = 16, 768


def _cfg():
    from vall_e.vall_e import synth
    return dataclasses.replace(synth.D3PMConfig.libritts(), n_heads=8, n_layers=2, canvas=CANVAS, n_frames=700)


@contextlib.contextmanager
def _ln_fold(value):
    """ln_fold = 3 is the library's every-row arm; the `tuning` context manager lists the shipped schedules only"""
    from vall_e.vall_e import _hip
    saved = _hip.TUNING.ln_fold
    _hip.set_tuning_field("ln_fold", value)
    try:
        yield
    finally:
        _hip.set_tuning_field("ln_fold", saved)


# ---- index kernels ------------------------------------------------------------------------------------------------------------
def _index_ref(tokens, fmask, n_classes):
    batch, canvas = tokens.shape
    seg_start, seg_len, row_of, cid, cmask = [], [], np.zeros((batch, canvas), np.int64), [], []
    start = 0
    for b in range(batch):
        cls = np.where(fmask[b] != 0, np.clip(tokens[b], 0, n_classes - 1), n_classes)
        _, first = np.unique(cls, return_index=True)
        reps = np.sort(first)                              # representatives in position order
        rank = {int(cls[p]): k for k, p in enumerate(reps)}
        row_of[b] = [start + rank[int(c)] for c in cls]
        pad = (len(reps) + 127) // 128 * 128
        cid += [int(cls[p]) for p in reps] + [n_classes] * (pad - len(reps))
        cmask += [int(cls[p] != n_classes) for p in reps] + [0] * (pad - len(reps))
        seg_start.append(start)
        seg_len.append(pad)
        start += pad
    m_pad = (start + 383) // 384 * 384
    cid += [n_classes] * (m_pad - start)
    cmask += [0] * (m_pad - start)
    return np.array(seg_start), np.array(seg_len), start, row_of.reshape(-1), np.array(cid), np.array(cmask)


def _index_inputs(case):
    gen = np.random.default_rng(5)
    batch, canvas = 4, 768
    fmask = np.ones((batch, canvas), np.uint8)
    if case == "equal":
        tokens = np.full((batch, canvas), 1024, np.int32)
    elif case == "distinct":
        tokens = np.stack([gen.permutation(canvas) for _ in range(batch)]).astype(np.int32)
    elif case == "eight":
        tokens = gen.choice([3, 1024, 17, 900, 5, 6, 1023, 1], size=(batch, canvas)).astype(np.int32)
    else:      # ragged frame masks, ids out of range among the live ones
        tokens = gen.integers(0, 40, size=(batch, canvas)).astype(np.int32)
        tokens[0, 5], tokens[1, 9] = -3, 5000
        for b, n in enumerate((768, 1, 333, 640)):
            fmask[b, n:] = 0
    return tokens, fmask


@pytest.mark.parametrize("case", ["equal", "distinct", "eight", "ragged"])
def test_index_and_compact_embedding_against_numpy(built_lib, case):
    from vall_e.vall_e import _hip
    n_classes, d = 1025, 512
    tokens, fmask = _index_inputs(case)
    table = (torch.randn(n_classes, d, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(DEV)
    got = _hip.op_dedup_index(torch.from_numpy(tokens).to(DEV), torch.from_numpy(fmask).to(DEV), n_classes, table)
    torch.cuda.synchronize()
    seg_start, seg_len, m_live, row_of, cid, cmask = _index_ref(tokens, fmask, n_classes)
    assert np.array_equal(got["seg_start"].cpu().numpy(), seg_start) and np.array_equal(got["seg_len"].cpu().numpy(), seg_len)
    assert (seg_len % 128 == 0).all() and int(got["m_live"].item()) == m_live == seg_len.sum()
    if case == "distinct":
        assert m_live == tokens.size
    if case == "equal":
        assert m_live == 128 * tokens.shape[0]
    assert np.array_equal(got["row_of"].cpu().numpy(), row_of)
    m_pad = len(cid)
    assert np.array_equal(got["cid"].cpu().numpy()[:m_pad], cid) and np.array_equal(got["cmask"].cpu().numpy()[:m_pad], cmask)
    # a position's compact row carries its class; rows the index does not define keep their sentinels
    cls = np.where(fmask != 0, np.clip(tokens, 0, n_classes - 1), n_classes).reshape(-1)
    assert np.array_equal(cid[row_of], cls)
    assert (got["cid"].cpu().numpy()[m_pad:] == -7).all() and (got["x"][m_pad:] == 3.0).all()
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


# ---- device-side live row count -----------------------------------------------------------------------------------------------
def _quads_of(x):
    from vall_e.vall_e import _hip
    st = _hip.op_row_stats(x)                                                          # [M / 16, 16, 16, 2]
    return (((st[:, 0::4] + st[:, 1::4]) + st[:, 2::4]) + st[:, 3::4]).contiguous()  # [M / 16, 4, 16, 2]


@pytest.fixture(scope="module")
def gemm_operands(built_lib):
    gen = torch.Generator().manual_seed(11)
    r = lambda *s: (torch.randn(*s, generator=gen) * 0.3).to(torch.bfloat16).to(DEV)      # noqa: E731
    M = 768
    return {"M": M, "x": r(M, 512), "x2": r(M, 512), "xk": r(M, 2048), "res": r(M, 512), "w1536": r(1536, 512), "w512": r(512, 512),
            "w2048": r(512, 2048), "w1025": r(1025, 512), "b512": r(512), "b1025": r(1025),
            "fs": torch.randn(1536, generator=gen).to(DEV), "fb": torch.randn(1536, generator=gen).to(DEV),
            "mask": (torch.rand(M, generator=gen) < 0.7).to(torch.uint8).to(DEV)}


def _live_call(o, epi, y, st, m_live):
    from vall_e.vall_e import _hip
    if epi in ("lnf", "lnf_gelu"):
        N = 1536 if epi == "lnf" else 512
        return _hip.op_linear_live(o["x"], o["w1536"][:N], None, y, m_live, act=int(epi == "lnf_gelu"), fold_s=o["fs"][:N], fold_b=o["fb"][:N],
                                   stats_in=o["quads"])
    if epi == "r1_stats":
        return _hip.op_linear_live(o["x"], o["w512"], o["b512"], y, m_live, r1=o["res"], stats_out=st)
    if epi == "mask":
        return _hip.op_linear_live(o["xk"], o["w2048"], o["b512"], y, m_live, r1=o["res"], row_mask=o["mask"], stats_out=st)
    if epi == "dual":
        return _hip.op_linear_live(o["x"], o["w512"], o["b512"], y, m_live, x2=o["x2"], r1=o["res"], stats_out=st)
    return _hip.op_linear_live(o["x"], o["w1025"], o["b1025"], y, m_live)               # final


@pytest.mark.parametrize("epi", ["lnf", "lnf_gelu", "r1_stats", "mask", "dual", "final"])
def test_live_row_count_from_device_memory(gemm_operands, epi):
    """192 x 128 tiles forced (gemm_variant = 8: 16 or 48 workgroups for 4 .. 48 live tiles, so the grid exceeds the tile count at every
    live count below the capacity); the final layer on the one-tile-per-workgroup 128 x 128 kernel (gemm_variant = 5)."""
    from vall_e.vall_e import _hip
    o = gemm_operands
    M = o["M"]
    o.setdefault("quads", _quads_of(o["x"]))
    N = {"lnf": 1536, "final": 1025}.get(epi, 512)
    ld = 1032 if epi == "final" else N
    tile = 128 if epi == "final" else 192
    with _hip.tuning(gemm_variant=5 if epi == "final" else 8):
        def run(live):
            y = torch.full((M, ld), 9.0, dtype=torch.bfloat16, device=DEV)
            st = torch.full((M // 16, 4, 16, 2), 9.0, dtype=torch.float32, device=DEV)
            _live_call(o, epi, y[:, :N] if epi == "final" else y, st, torch.tensor([live], dtype=torch.int32, device=DEV))
            torch.cuda.synchronize()
            return y[:, :N], st
        full_y, full_st = run(M)
        assert not (full_y == 9.0).all(dim=1).any()
        if epi == "lnf":      # the quads are the parts summed in the consumers' order: the established parts-format op gives the same rows
            assert torch.equal(full_y, _hip.op_linear_fold(o["x"], o["w1536"], o["fs"], o["fb"], _hip.op_row_stats(o["x"])))
        for live in (128, 192, 384, 768):
            y, st = run(live)
            edge = (live + tile - 1) // tile * tile
            assert torch.equal(y[:live], full_y[:live]), (epi, live)
            assert (y[edge:] == 9.0).all(), (epi, live, "a row behind the last live tile was written")
            if epi in ("r1_stats", "mask", "dual"):
                assert torch.equal(st[: live // 16], full_st[: live // 16]) and (st[edge // 16:] == 9.0).all(), (epi, live)


# ---- the loops ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(built_lib):
    from vall_e.vall_e import AR, synth
    cfg = _cfg()
    cache = {}

    def get(dtype):
        if dtype not in cache:
            m = AR.from_config(cfg)
            m.load_state_dict(synth.make_state_dict(cfg, 0))
            m = m.to(dtype).to(DEV)
            texts, proms = synth.make_inputs(cfg, B, 1)
            cache[dtype] = (m, texts, proms) + tuple(m.encode_conditions(texts, proms))
        return cache[dtype]
    return cfg, get


def _both(smp, x0, fm, kv, what, t_start, t_stop, **kw):
    out = {}
    for ln_fold in (1, 3):
        x = x0.clone()
        with _ln_fold(ln_fold):
            tr = smp.sample_loop(x, fm, t_start, t_stop, kv[0], kv[1], seed=91, trace=True, **kw)
        torch.cuda.synchronize()
        out[ln_fold] = (x, tr)
    (xa, ta), (xb, tb) = out[1], out[3]
    per_iter = (ta != tb).flatten(1).sum(dim=1).tolist()
    assert torch.equal(ta, tb), f"{what}: ids of the trace that differ between ln_fold = 1 and 3, per iteration: {per_iter}"
    assert torch.equal(xa, xb) and not torch.equal(xa, x0), what
    return xa, ta


def _launches(smp, x0, fm, kv, ln_fold, t_start, t_stop, reveal_steps=None, **kw):
    """launches per kernel class in the bracketed iterations (t % 16 == 0): the index and the key expansions count in the small-kernel
    class, so a deduplicated iteration never has the counts of the every-row one"""
    from vall_e.vall_e import _hip
    try:
        _hip.prof_enable(_hip.K_ALL, 512)
        with _ln_fold(ln_fold):
            if reveal_steps is not None:
                smp.reveal_loop(x0.clone(), fm, reveal_steps, kv[0], kv[1], seed=91, **kw)
            else:
                smp.sample_loop(x0.clone(), fm, t_start, t_stop, kv[0], kv[1], seed=91, **kw)
        torch.cuda.synchronize()
        counts = tuple(_hip.prof_read_class(k)[0] for k in range(_hip.K_ALL))
        assert sum(counts) > 0, "no iteration of this loop was bracketed"
        return counts
    finally:
        _hip.prof_disable()


def _deduplicates(smp, x0, fm, kv, t_start=97, t_stop=94, **kw):
    """does the default run another launch list than ln_fold = 3 for these arguments?"""
    return _launches(smp, x0, fm, kv, 1, t_start, t_stop, **kw) != _launches(smp, x0, fm, kv, 3, t_start, t_stop, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_plain_loop_from_the_all_masked_start(models, dtype):
    cfg, get = models
    m, _, _, ct, cp = get(dtype)
    smp = m.sampler()
    kv = smp.cond_kv(ct, cp)
    x, fm = m.canvas_init(B)
    assert int(fm.sum()) < fm.numel()
    t0 = cfg.timesteps - 1
    _, tr = _both(smp, x, fm, kv, f"all-masked start {dtype}", t0, t0 - 13)
    distinct = [len(set(tr[i, 0].tolist())) for i in (0, tr.shape[0] - 1)]
    assert distinct[0] < 64, distinct      # the path under test really merges rows here
    # ... and the default really is another launch list than ln_fold = 3
    assert _deduplicates(smp, x, fm, kv)


def test_start_with_every_id_distinct(models):
    cfg, get = models
    m, _, _, ct, cp = get(torch.bfloat16)
    smp = m.sampler()
    kv = smp.cond_kv(ct, cp)
    gen = torch.Generator().manual_seed(2)
    ids = torch.stack([torch.randperm(CANVAS, generator=gen) for _ in range(B)]).to(torch.int32).to(DEV)      # segment = the whole canvas
    fm = torch.ones(CANVAS, dtype=torch.uint8, device=DEV)
    _both(smp, ids, fm, kv, "all distinct", 30, 26)
    assert _deduplicates(smp, ids, fm, kv, 33, 30)


def test_canvas_known_frames_keys_and_nucleus(models):
    cfg, get = models
    m, texts, proms, ct, cp = get(torch.bfloat16)
    smp = m.sampler()
    gen = torch.Generator().manual_seed(8)
    lens = [int(v) for v in torch.randint(90, CANVAS + 1, (B,), generator=gen)]
    lens[0], lens[1] = CANVAS, 1
    known = [torch.randint(0, 1024, (min(40, n),), generator=gen) if b % 3 == 0 else None for b, n in enumerate(lens)]
    x, fm, km = m.canvas_init_known(B, lens, known=known)
    kv = smp.cond_kv(ct, cp)
    t0 = cfg.timesteps - 1
    out, _ = _both(smp, x, fm, kv, "canvas + known", t0, t0 - 6, known=km)
    assert torch.equal(out[km.bool()], x[km.bool()])
    assert _deduplicates(smp, x, fm, kv, known=km)
    _both(smp, x, fm, kv, "canvas + known + nucleus", t0, t0 - 5, known=km, temperature=0.9, top_k=50, top_p=0.9)
    assert _deduplicates(smp, x, fm, kv, known=km, temperature=0.9, top_k=50, top_p=0.9)
    f, tl, pl = m.key_lengths(texts, proms, lens)
    keys = tuple(torch.tensor(v, dtype=torch.int32, device=DEV) for v in (f, tl, pl))
    ctk, cpk = smp.encode_conditions(*m._padded_inputs(texts, proms), keys[1], keys[2])
    kvk = smp.cond_kv(ctk, cpk)
    _both(smp, x, fm, kvk, "canvas + known + keys", t0, t0 - 5, known=km, keys=keys)
    assert _deduplicates(smp, x, fm, kvk, known=km, keys=keys)      # the masked attention kernels take the segments too


def test_a_shard_under_regime_batch_equals_the_unsplit_batch(models):
    from vall_e.vall_e import _hip
    cfg, get = models
    m, _, _, ct, cp = get(torch.bfloat16)
    smp = m.sampler()
    x, fm = m.canvas_init(B)
    t0 = cfg.timesteps - 1
    whole = x.clone()
    smp.sample_loop(whole, fm, t0, t0 - 6, *smp.cond_kv(ct, cp), seed=91)
    half = B // 2
    with _hip.tuning(regime_batch=B):
        for lo in (0, half):
            kv = smp.cond_kv(ct[lo:lo + half].contiguous(), cp[lo:lo + half].contiguous())
            part = x[lo:lo + half].clone()
            smp.sample_loop(part, fm, t0, t0 - 6, *kv, seed=91, utt0=lo)
            assert torch.equal(part, whole[lo:lo + half]), lo
            every_row = x[lo:lo + half].clone()
            with _ln_fold(3):
                smp.sample_loop(every_row, fm, t0, t0 - 6, *kv, seed=91, utt0=lo)
            assert torch.equal(every_row, part), lo
    # (whether a shard itself deduplicates follows from ITS projections' tiles; either way its ids are the unsplit, deduplicated batch's)


def test_guided_and_one_utterance_calls_keep_their_launch_list(models):
    cfg, get = models
    m, texts, proms, ct, cp = get(torch.bfloat16)
    smp = m.sampler()
    x, fm = m.canvas_init(B)
    kv1 = smp.cond_kv(ct[:1].contiguous(), cp[:1].contiguous())
    assert not _deduplicates(smp, x[:1], fm, kv1)
    half = B // 2
    nt, npm = m._null_conditions(texts[:half], None, 1), m._null_conditions(proms[:half], None, 2)
    ct2, cp2 = m.encode_conditions(list(texts[:half]) + nt, list(proms[:half]) + npm)
    kv2 = smp.cond_kv(ct2, cp2)
    assert not _deduplicates(smp, x[:half], fm, kv2, guidance=1.5)


def test_reveal_and_fp8_loops_keep_their_launch_list(models):
    cfg, get = models
    m, _, _, ct, cp = get(torch.bfloat16)
    smp = m.sampler()
    kv = smp.cond_kv(ct, cp)
    x, fm = m.canvas_init(B)
    n_steps = next(n for n in range(4, 48) if any(t % 16 == 0 for t in smp.reveal_plan(n)))      # a plan with a bracketed timestep
    assert not _deduplicates(smp, x, fm, kv, reveal_steps=n_steps)
    assert not _deduplicates(smp, x, fm, kv, fp8=True)


def test_n_q_8_loop_keeps_its_launch_list(built_lib):
    from vall_e.vall_e import AR, synth
    cfg = dataclasses.replace(synth.D3PMConfig.libritts_8q(), n_heads=8, n_layers=2, canvas=CANVAS, n_frames=700)
    m = AR.from_config(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, 0))
    m = m.to(torch.bfloat16).to(DEV)
    texts, proms = synth.make_inputs(cfg, B, 1)
    smp = m.sampler()
    kv = smp.cond_kv(*m.encode_conditions(texts, proms))
    x, fm = m.canvas_init(B)
    assert x.shape == (B, CANVAS, 8)
    assert not _deduplicates(smp, x, fm, kv)


def test_graph_captured_loop(models):
    """generate_audio(graph=True) replays the captured loop: nothing in the deduplicated launch list reads a count back to the host"""
    cfg, get = models
    m, texts, proms, _, _ = get(torch.bfloat16)
    out = {}
    for ln_fold in (1, 3):
        with _ln_fold(ln_fold):
            out[ln_fold] = m.generate_audio(texts, proms, steps=8, seed=12, graph=True)
        torch.cuda.synchronize()
    assert torch.equal(out[1], out[3])
    with _ln_fold(1):
        assert torch.equal(m.generate_audio(texts, proms, steps=8, seed=12, graph=False), out[1])
    # the same call deduplicates: counted on the eager loop (an attached profiler keeps generate_audio from capturing a graph)
    from vall_e.vall_e import _hip
    counts = {}
    for ln_fold in (1, 3):
        try:
            _hip.prof_enable(_hip.K_ALL, 512)
            with _ln_fold(ln_fold):
                m.generate_audio(texts, proms, steps=17, seed=12, graph=True)
            torch.cuda.synchronize()
            counts[ln_fold] = tuple(_hip.prof_read_class(k)[0] for k in range(_hip.K_ALL))
        finally:
            _hip.prof_disable()
    assert sum(counts[3]) > 0 and counts[1] != counts[3], counts


# ---- the deduplicated evaluation against the CPU oracle ---------------------------------------------------------------------------
def _half_denoised(cfg, rng):
    """[B, canvas] canvases with every other live frame carrying an id.  Utterance 0 draws its ids from eight values, so nearly all of
    its rows merge; the ids of utterance 1 are all distinct, so none of its revealed rows do; the others draw from all 1024."""
    x = np.zeros((B, cfg.canvas), np.int64)
    x[:, : cfg.n_frames] = cfg.mask_id
    live = np.arange(0, cfg.n_frames, 2)
    for b in range(B):
        if b == 0:
            x[b, live] = rng.choice([3, 1023, 17, 900, 5, 6, 640, 1], size=live.shape)
        elif b == 1:
            x[b, live] = rng.permutation(np.setdiff1d(np.arange(1024), [cfg.mask_id]))[: len(live)]
        else:
            x[b, live] = rng.integers(0, 1024, size=live.shape)
    return x


@pytest.mark.parametrize("tag,dtype,tie,frac", [("f16", torch.float16, 0.06, 0.01), ("bf16", torch.bfloat16, 0.5, 0.05)])
def test_deduplicated_step_against_the_oracle(models, tag, dtype, tie, frac):
    """x_49 of sample_loop(x_50, .., 50, 48, trace=True) -- iteration 50 of a call that runs the deduplicated launch list: table rows,
    compact projections, segment attention, gathered keys, the sampler through row_of -- against the CPU oracle's own draw from its own
    logits, conditions and Philox noise, exactly as test_libritts_shape_step_against_the_oracle compares the every-row evaluation:
    an id may differ only where the oracle's Gumbel race was a near-tie.  The bounds are that test's (worst gap < 0.06 fp16 / 0.5
    bf16, mismatch fraction < 0.01 / 0.05), set on the six-layer model; two layers accumulate less rounding.
    Measured here (two layers, utterances 0 and 1, 1400 live frames), fp16 and bf16 alike, ln_fold = 1 and 3 alike: worst gap 0.0,
    mismatch fraction 0.0 (0 of 1400).  What that covers: 700 of the 1400 frames are masked and race; at t = 50 the oracle lets 3 + 13 of
    them leave the mask, and it decided 2 of the 700 races by less than 0.06 and 19 by less than 0.5 (smallest 0.039).  The revealed
    frames keep their id whatever the logits are."""
    from oracle import d3pm_oracle as O
    from oracle import philox
    from util import REPORT
    from vall_e.vall_e import synth
    cfg, get = models
    m, texts, proms, ct, cp = get(dtype)
    smp = m.sampler()
    kv = smp.cond_kv(ct, cp)
    _, fm = m.canvas_init(B)
    xs = _half_denoised(cfg, np.random.default_rng(7))
    x0 = torch.from_numpy(xs.astype(np.int32)).to(DEV)
    assert len(set(xs[0].tolist())) <= 10 and len(set(xs[1, : cfg.n_frames : 2].tolist())) == (cfg.n_frames + 1) // 2
    t, seed = 50, 321
    traces = {}
    for ln_fold in (1, 3):
        x = x0.clone()
        with _ln_fold(ln_fold):
            traces[ln_fold] = smp.sample_loop(x, fm, t, t - 2, kv[0], kv[1], seed=seed, trace=True)
        torch.cuda.synchronize()
    # the launch counters are read in iterations with t % 16 == 0 only, and the two lists differ in count where an iteration prepares
    # the next one (the index launches): the same call extended by two iterations has t = 48 as such an iteration (the choice of the
    # launch list is made once per call and does not look at the step range beyond "at least two iterations")
    assert _deduplicates(smp, x0, fm, kv, t, t - 4)
    orc = O.Oracle({k: v.to(dtype) for k, v in synth.make_state_dict(cfg, 0).items()}, O.Shape.of(cfg))
    mask = torch.zeros(cfg.canvas, dtype=torch.bool)
    mask[: cfg.n_frames] = True
    assert torch.equal(fm.cpu().bool().view(-1)[-cfg.canvas:], mask)
    live = slice(0, cfg.n_frames)
    stats = {}
    wants = []
    for b in range(2):
        with torch.no_grad():
            ocp, oct_ = orc.conditions(texts[b], proms[b])
            ref = orc.logits(torch.from_numpy(xs[b]), t, ocp, oct_, mask)
            post = orc.posterior(ref, torch.from_numpy(xs[b]), t)
        u = torch.from_numpy(philox.uniform_batch(seed, t, b, 1, cfg.canvas)[0])
        v = post.float() + -torch.log(-torch.log(torch.clamp(u, min=torch.finfo(torch.float32).tiny, max=1.0)))
        wants.append((v, torch.argmax(v, dim=-1).numpy()))
    for ln_fold, tr in traces.items():
        worst_gap, mism, total = 0.0, 0, 0
        for b, (v, want) in enumerate(wants):
            nxt = tr[0, b].cpu().numpy()
            for r in np.nonzero(nxt[live] != want[live])[0]:      # position by position: how clearly had the oracle's race been decided?
                worst_gap = max(worst_gap, (v[r, want[r]] - v[r, nxt[r]]).item())
            mism += int((nxt[live] != want[live]).sum())
            total += cfg.n_frames
        stats[ln_fold] = (worst_gap, mism / total)
        REPORT[f"dedup_{tag}_ln_fold{ln_fold}_sampled_id_worst_gap"] = worst_gap
        REPORT[f"dedup_{tag}_ln_fold{ln_fold}_sampled_id_mismatch_frac"] = mism / total
        print(f"[dedup oracle] {tag} ln_fold={ln_fold}: worst gap {worst_gap:.4f}, mismatch fraction {mism / total:.5f} ({mism} of {total})")
    # the every-row arm first: if IT misses a bound the inputs are at fault, not the deduplicated evaluation
    assert stats[3][0] < tie and stats[3][1] < frac, f"ln_fold = 3 misses the bounds on these inputs: {stats[3]}"
    assert stats[1][0] < tie, f"a sampled id differs where the oracle's race was decided by {stats[1][0]}"
    assert stats[1][1] < frac, stats[1]
    assert torch.equal(traces[1], traces[3])


# ---- attention: a query row's bits do not depend on its wave-mates ------------------------------------------------------------------
def _hostile_inputs(dtype):
    """128 queries, 96 keys, one head of 64.  Every query carries the direction w (|w| = 1) and the keys of the third 32-key block
    carry 17 w, which lifts every query's scores there by ~ +3 in the log2 domain -- above its running maximum, below the deferral
    threshold of 2^8.  The hostile query is 20 w: its third-block scores exceed its first-block maximum by ~ 60 > 8 and fire the rare
    path for its wave."""
    gen = torch.Generator().manual_seed(4)
    w = torch.zeros(64)
    w[3] = 1.0
    q = torch.randn(128, 64, generator=gen) * 0.1 + w
    k = torch.randn(128, 64, generator=gen) * 0.1
    k[64:96] += 17.0 * w
    v = torch.randn(128, 64, generator=gen)
    hostile = q.clone()
    hostile[5] = 20.0 * w
    to = lambda t: t.to(dtype).to(DEV)[None].contiguous()      # noqa: E731
    return to(q), to(hostile), to(k), to(v)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_attention_rows_do_not_depend_on_their_wave_mates(built_lib, dtype):
    from vall_e.vall_e import _hip
    q, qh, k, v = _hostile_inputs(dtype)
    others = torch.arange(128, device=DEV) != 5
    scale = 0.125
    with _hip.tuning(attn_query_groups=32):      # attn32p_hd64, 96 of the 128 padded keys valid
        kl = torch.tensor([96], dtype=torch.int32, device=DEV)
        a, b = _hip.op_attention(q, k, v, 1, scale, key_len=kl), _hip.op_attention(qh, k, v, 1, scale, key_len=kl)
        assert torch.equal(a[0, others], b[0, others]), "self-attention: a row changed with its wave-mate"
        assert not torch.equal(a[0, 5], b[0, 5])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cross_attention_rows_do_not_depend_on_their_wave_mates(built_lib, dtype):
    from vall_e.vall_e import _hip
    q, qh, k, v = _hostile_inputs(dtype)
    others = torch.arange(128, device=DEV) != 5
    scale = 0.125
    with _hip.tuning(attn_cross_resident=5):     # attn32_cross_hd64: 64 text keys, 96 prompt keys
        kt, vt, kp, vp = (t.clone()[None] for t in (k[0, :64], v[0, :64], k[0, :96], v[0, :96]))
        a1, a2 = _hip.op_attention_pair(q, kt, vt, q, kp, vp, 1, scale)
        b1, b2 = _hip.op_attention_pair(qh, kt, vt, qh, kp, vp, 1, scale)
        assert torch.equal(a1[0, others], b1[0, others]) and torch.equal(a2[0, others], b2[0, others]), "cross-attention: a row changed with its wave-mate"
        assert not torch.equal(a2[0, 5], b2[0, 5])

"""Per-frame log-probability of the revealed id (include/d3pm_hip.h: d3pm_frame_scores) on the GPU.

What carries no tolerance: under the neutral triple the value is the reveal step's greedy confidence bit for bit; the guided and the
indexed arm equal the plain arm on host-combined / gathered logits; a scored loop returns the ids of the unscored one and the two grids
of its chained step entries; `step` is the timestep of the first trace entry that is not the mask; the deduplicated loop gives the
grids of the every-row loop; an utterance does not depend on the batch it rides in.  What carries one: a value sits within 1.0e-4 of
the float64 log_softmax with the mask class removed (tests/logprob_ref.py; the bound the header derives for the reveal score).
python -m pytest tests/test_gpu_logprob.py -m gpu"""
import contextlib
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import guidance_ref as G
import logprob_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T = 2, 37      # 74 rows: no multiple of the 4 rows of a workgroup, 19 workgroups
KS = [1025, 257]
DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def pp(v):
    return None if v is None else C.c_void_p(v.data_ptr())


class Step:
    """The step entries on a bare shape (no weights): K and the canvas are free."""

    def __init__(self, K, canvas=T):
        from vall_e.vall_e import _hip, synth
        self.hip = _hip
        self.shape = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
        self.shape.n_classes, self.shape.mask_id, self.shape.canvas, self.shape.n_q = K, K // 2, canvas, 1
        self.K, self.canvas, self.mask_id = K, canvas, K // 2
        self.sched = _hip.Schedule(100)

    def reveal_all(self, logits, x_t, fm, known, t):
        """d3pm_reveal_step, greedy, choice_temperature 0, t_next 0, the neutral triple -> x_next, cand, score (device)"""
        hip = self.hip
        x_next = torch.full_like(x_t, -7)
        cand = torch.full(x_t.shape, -7, dtype=torch.int32, device=DEV)
        score = torch.full(x_t.shape, 12345.0, dtype=torch.float32, device=DEV)
        cv = hip.Canvas(fm.data_ptr(), known.data_ptr())
        hip.check(hip.lib().d3pm_reveal_step(C.byref(self.shape), x_t.shape[0], pp(logits), hip.dtype_code(logits.dtype), pp(x_t), pp(x_next), None,
                                             C.byref(cv), int(t), 0, C.byref(self.sched.c_struct), 5, 0, hip.FLAG_GREEDY, None, 0.0, pp(cand),
                                             pp(score), hip.stream_ptr()), "d3pm_reveal_step")
        return x_next, cand, score

    def grids(self, n=B, fill=None):
        lp = torch.full((n, self.canvas), 777.0 if fill is None else fill[0], dtype=torch.float32, device=DEV)
        st = torch.full((n, self.canvas), -99 if fill is None else fill[1], dtype=torch.int32, device=DEV)
        return lp, st

    def init(self, x, fm, known, scores, shared=False):
        hip = self.hip
        fs = hip.FrameScores(scores[0].data_ptr(), scores[1].data_ptr())
        cv = hip.Canvas(fm.data_ptr(), None if known is None else known.data_ptr())
        return hip.lib().d3pm_frame_scores_init(C.byref(self.shape), x.shape[0], pp(x), pp(fm) if shared else None, None if shared else C.byref(cv),
                                                C.byref(fs), hip.stream_ptr())

    def step(self, logits, x_next, t, scores, *, ldl=None, row_of=None, w=None, shape=None, fs=None):
        hip = self.hip
        fs = hip.FrameScores(scores[0].data_ptr(), scores[1].data_ptr()) if fs is None else fs
        gd = None if w is None else hip.Guidance(w)
        return hip.lib().d3pm_frame_scores_step(C.byref(self.shape if shape is None else shape), x_next.shape[0], pp(logits),
                                                hip.dtype_code(logits.dtype), self.K if ldl is None else ldl, pp(row_of),
                                                None if gd is None else C.byref(gd), pp(x_next), int(t), C.byref(fs), hip.stream_ptr())


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _case(K, dtype, seed):
    """logits in `dtype` (fp32 holds fp16-grid values), x_t, frame mask with a padded tail, known map, all on the device + the numpy state"""
    l, x, fm, known = R.cases(B, T, K, seed)
    if dtype == torch.float32:
        l = R.rn16(l).astype(np.float32)
    logits = _dev(l, dtype)
    return logits, _dev(x), _dev(fm), _dev(known), R.free_masked(x, fm, known, K // 2)


# ---- 1. against the reveal step, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_value_is_the_reveal_steps_greedy_confidence_bit_for_bit(built_lib, dtype, K):
    st = Step(K)
    logits, x, fm, known, free = _case(K, dtype, seed=K)
    assert 20 <= free.sum() < free.size and (fm.cpu().numpy() == 0).any() and known.sum() > 0
    t = 60
    x_next, cand, score = st.reveal_all(logits, x, fm, known, t)
    scores = st.grids()
    assert st.init(x, fm, known, scores) == 0 and st.step(logits, x_next, t, scores) == 0
    torch.cuda.synchronize()
    lp, step = scores[0].cpu(), scores[1].cpu()
    f = torch.from_numpy(free)
    assert (x_next.cpu()[f] != st.mask_id).all(), "t_next = 0 reveals every masked free row"
    assert torch.equal(lp[f], score.cpu()[f]), f"{(lp[f] != score.cpu()[f]).sum().item()} of {int(f.sum())} values differ from the reveal score"
    assert (step[f] == t).all()
    assert (step[~f] == -1).all() and (lp[~f] == 0).all(), "padding, known and already revealed rows"
    assert torch.isfinite(lp).all() and (lp[f] < 0).all()


# ---- 2. against the definition, 3. monotone state ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_values_against_the_float64_definition_and_the_state_is_monotone(built_lib, dtype, K):
    st = Step(K)
    logits, x, fm, known, free = _case(K, dtype, seed=K + 1)
    ln = logits.float().cpu().numpy().reshape(B * T, K)
    rows = np.flatnonzero(free.reshape(-1))
    later = rows[2::3]                       # every third masked row is not revealed by the first call
    first = np.setdiff1d(rows, later)
    ids = R.other_ids(B * T, K, seed=7)
    xn = x.cpu().numpy().reshape(-1).copy()
    xn[first] = ids[first]
    assert (xn[later] == st.mask_id).all() and (ids != st.mask_id).all()
    assert np.isfinite(R.rn16(ln)[first, ids[first]].astype(np.float32)).all(), "the ids' own logits are finite"
    scores = st.grids()
    t1, t2 = 60, 41
    assert st.init(x, fm, known, scores) == 0 and st.step(logits, _dev(xn.reshape(B, T)), t1, scores) == 0
    torch.cuda.synchronize()
    lp, step = scores[0].cpu().numpy().reshape(-1), scores[1].cpu().numpy().reshape(-1)
    err = np.abs(lp[first].astype(np.float64) - R.logprob64(ln[first], st.mask_id, ids[first])).max()
    print(f"[logprob] K={K} {dtype}: max |logprob - log_softmax64| = {err:.3e} over {len(first)} rows (bound {R.TOL:.1e})")
    assert err <= R.TOL
    assert (step[first] == t1).all() and (step[later] == 0).all() and (lp[later] == 0).all(), "a row that keeps the mask id stays at step 0"
    off = np.setdiff1d(np.arange(B * T), rows)
    assert (step[off] == -1).all() and (lp[off] == 0).all()
    # 3. a second call at a lower t with OTHER logits in the buffer reveals the rest and leaves the scored rows as they are
    l2 = np.roll(ln, 5, axis=1)[::-1].copy()
    if dtype == torch.bfloat16:
        l2 = G.on_grid(l2, "bfloat16")
    xn2 = xn.copy()
    xn2[later] = ids[later]
    xn2[first[::2]] = (ids[first[::2]] + 1) % 256      # a scored row whose id moves later keeps its score (the D3PM loop redraws)
    assert st.step(_dev(l2.reshape(B, T, K), dtype), _dev(xn2.reshape(B, T)), t2, scores) == 0
    torch.cuda.synchronize()
    lp2, step2 = scores[0].cpu().numpy().reshape(-1), scores[1].cpu().numpy().reshape(-1)
    keep = np.setdiff1d(np.arange(B * T), later)
    assert np.array_equal(lp2[keep].view(np.uint32), lp[keep].view(np.uint32)) and np.array_equal(step2[keep], step[keep])
    assert (step2[later] == t2).all()
    assert np.abs(lp2[later].astype(np.float64) - R.logprob64(l2[later], st.mask_id, ids[later])).max() <= R.TOL
    assert not np.allclose(lp2[later], R.logprob64(ln[later], st.mask_id, ids[later]), atol=1e-2), "the second call read the second buffer"


# ---- 4. guided arm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_guided_arm_equals_the_plain_arm_on_host_combined_logits(built_lib, dtype, K):
    st = Step(K)
    grid = "bfloat16" if dtype == torch.bfloat16 else np.float16
    c, u = G.crafted(B * T, K, seed=K + 3, dtype=grid)
    both = _dev(np.concatenate([c, u]).reshape(2 * B, T, K), dtype)
    assert np.array_equal(both.float().cpu().numpy().reshape(2 * B * T, K), np.concatenate([c, u])), "the inputs sit on the dtype's grid"
    _, x, fm, known, free = _case(K, dtype, seed=K + 2)
    ids = R.other_ids(B * T, K, seed=9)
    xn = np.where(free.reshape(-1), ids, x.cpu().numpy().reshape(-1)).astype(np.int32)
    xn[np.flatnonzero(free.reshape(-1))[::5]] = st.mask_id
    x_next = _dev(xn.reshape(B, T))
    moved = 0
    for w in (0.5, 1.5, 3.0):
        assert G.exact(c, u, w).all() and G.exact_rational(c, u, w, n=300)
        z = _dev(G.combine(c, u, w).astype(np.float32).reshape(B, T, K))      # fp32 logits on the fp16 grid
        ref, got, swapped = st.grids(), st.grids(), st.grids()
        for sc in (ref, got, swapped):
            assert st.init(x, fm, known, sc) == 0
        assert st.step(z, x_next, 33, ref) == 0 and st.step(both, x_next, 33, got, w=w) == 0
        assert st.step(torch.cat([both[B:], both[:B]]).contiguous(), x_next, 33, swapped, w=w) == 0
        torch.cuda.synchronize()
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), f"w={w}: {(got[0] != ref[0]).sum().item()} values differ"
        assert int((ref[1] == 33).sum()) >= 20
        moved += int((swapped[0] != ref[0]).sum())
    assert moved > 0, "a kernel that swaps the halves gives other values"


# ---- 5. indexed arm -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_indexed_arm_equals_the_plain_arm_on_gathered_logits(built_lib, dtype, K):
    """Nine compact rows at the head of a buffer of stride K + 7 with the loop's capacity of B * T rows (the index is clamped into the
    capacity, as dedup_sample_rows clamps it): row_of maps the 74 rows onto the nine with repeats, -3 clamps to row 0 and 10^6 to the
    last row of the buffer."""
    st = Step(K)
    rows, ldl, n_compact = B * T, K + 7, 9
    g = torch.Generator().manual_seed(K)
    buf = (torch.randn(rows, ldl, generator=g) * 3).to(dtype).to(DEV)
    row_of = ((torch.arange(rows) * 5 + torch.randint(0, 2, (rows,), generator=g)) % n_compact).to(torch.int32)
    row_of[4], row_of[40] = -3, 10 ** 6
    assert len(set(row_of.tolist())) == n_compact + 2
    src = row_of.clamp(0, rows - 1).long()
    dense = buf[src.to(DEV), :K].contiguous().reshape(B, T, K)
    _, x, fm, known, free = _case(K, dtype, seed=K + 4)
    assert free.reshape(-1)[4] and free.reshape(-1)[40], "the two clamped rows are scored"
    xn = np.where(free.reshape(-1), R.other_ids(rows, K, seed=3), x.cpu().numpy().reshape(-1)).astype(np.int32)
    x_next = _dev(xn.reshape(B, T))
    ref, got = st.grids(), st.grids()
    assert st.init(x, fm, known, ref) == 0 and st.init(x, fm, known, got) == 0
    assert st.step(dense, x_next, 12, ref) == 0
    assert st.step(buf, x_next, 12, got, ldl=ldl, row_of=row_of.to(DEV)) == 0
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), f"{(got[0] != ref[0]).sum().item()} values differ"
    assert int((ref[1] == 12).sum()) == int(free.sum())
    own = st.grids()      # (the plain arm on the buffer itself reads other rows: the index is what was compared)
    assert st.init(x, fm, known, own) == 0 and st.step(buf, x_next, 12, own, ldl=ldl) == 0
    torch.cuda.synchronize()
    assert not torch.equal(own[0], ref[0])


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(built_lib):
    from vall_e.vall_e import _hip, synth
    E_ARG, E_SHAPE = -1, -4
    st = Step(1025)
    logits, x, fm, known, _ = _case(1025, torch.float16, seed=1)
    x_next = _dev(R.other_ids((B, T), 1025, seed=2))
    scores = st.grids(fill=(3.5, 0))      # step 0 everywhere: a step call that launched would score every row
    fs = _hip.FrameScores(scores[0].data_ptr(), scores[1].data_ptr())
    sh2 = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
    sh2.n_classes, sh2.mask_id, sh2.canvas, sh2.n_q = st.shape.n_classes, st.shape.mask_id, st.shape.canvas, 2
    row_of = torch.zeros(B * T, dtype=torch.int32, device=DEV)
    lib, cv = _hip.lib(), _hip.Canvas(fm.data_ptr(), known.data_ptr())

    def init(fs_, shape=st.shape, shared=None, canvas=cv):
        return lib.d3pm_frame_scores_init(C.byref(shape), B, pp(x), pp(shared), None if canvas is None else C.byref(canvas),
                                          None if fs_ is None else C.byref(fs_), _hip.stream_ptr())
    no_lp, no_st = _hip.FrameScores(None, scores[1].data_ptr()), _hip.FrameScores(scores[0].data_ptr(), None)
    for rc, want in ((init(None), E_ARG), (init(no_lp), E_ARG), (init(no_st), E_ARG), (init(fs, sh2), E_SHAPE), (init(fs, shared=fm[0].contiguous()), E_ARG),
                     (init(fs, canvas=None), E_ARG)):
        assert rc == want and lib.d3pm_last_error(), (rc, want)
    f32 = logits.float()
    for rc, want in ((st.step(logits, x_next, 5, scores, fs=no_lp), E_ARG), (st.step(logits, x_next, 5, scores, fs=no_st), E_ARG),
                     (lib.d3pm_frame_scores_step(C.byref(st.shape), B, pp(logits), _hip.F16, 1025, None, None, pp(x_next), 5, None, _hip.stream_ptr()), E_ARG),
                     (st.step(logits, x_next, 5, scores, shape=sh2), E_SHAPE),
                     (st.step(torch.cat([logits, logits]), x_next, 5, scores, row_of=row_of, w=1.5), E_ARG),
                     (st.step(f32, x_next, 5, scores, row_of=row_of), E_ARG),
                     (st.step(logits, x_next, 0, scores), E_ARG), (st.step(logits, x_next, 5, scores, ldl=1000), E_ARG),
                     (st.step(logits, x_next, 5, scores, w=-1.0), E_ARG)):
        assert rc == want and lib.d3pm_last_error(), (rc, want)
    torch.cuda.synchronize()
    assert (scores[0] == 3.5).all() and (scores[1] == 0).all(), "a refused call launches nothing"


def test_loop_entries_refuse_and_launch_nothing(native):
    from vall_e.vall_e import _hip
    m, cfg, texts, proms = native(torch.float16)
    smp = m.sampler()
    lib, sh, sched = _hip.lib(), smp.shape, smp.schedule.c_struct
    x, fm = m.canvas_init(1)
    x0 = x.clone()
    kv_t, kv_p = smp.cond_kv(*m.encode_conditions(texts[:1], proms[:1]))
    ws = smp.workspace(2)
    lp = torch.full((1, cfg.canvas), 3.5, dtype=torch.float32, device=DEV)
    stp = torch.full((1, cfg.canvas), 0, dtype=torch.int32, device=DEV)
    fs = _hip.FrameScores(lp.data_ptr(), stp.data_ptr())
    sh2 = _hip.make_shape(dataclasses.replace(cfg, n_q=2), torch.float16)
    fp8 = C.c_void_p(ws.data_ptr())      # any non-null pointer: refused before it is read
    ks = _hip.Keys(None, None, None)
    rv = _hip.Reveal(4, 0.0)

    def loop(fs_, flags=0, shape=sh, f8=None, keys=None, gd=None):
        return lib.d3pm_sample_loop_scored(C.byref(shape), C.byref(smp.weights.c_struct), f8, 1, pp(x), pp(fm), None, 3, 0, pp(smp.film), pp(kv_t),
                                           pp(kv_p), C.byref(sched), 1, 0, flags, pp(ws), ws.numel(), None, None, None if keys is None else C.byref(keys),
                                           None if gd is None else C.byref(gd), None if fs_ is None else C.byref(fs_), _hip.stream_ptr())

    def reveal(fs_, flags=0, shape=sh):
        return lib.d3pm_reveal_loop_scored(C.byref(shape), C.byref(smp.weights.c_struct), 1, pp(x), pp(fm), None, pp(smp.film), pp(kv_t), pp(kv_p),
                                           C.byref(sched), 1, 0, flags, pp(ws), ws.numel(), None, None, C.byref(rv), None,
                                           None if fs_ is None else C.byref(fs_), _hip.stream_ptr())
    half = _hip.FrameScores(lp.data_ptr(), None)
    for rc, want in ((loop(None), -1), (loop(half), -1), (loop(fs, shape=sh2), -4), (loop(fs, flags=_hip.FLAG_SEED_IN_HBM), -1),
                     (loop(fs, f8=fp8, keys=ks), -1), (loop(fs, f8=fp8, gd=_hip.Guidance(1.0)), -1), (loop(fs, gd=_hip.Guidance(-1.0)), -1),
                     (reveal(None), -1), (reveal(half), -1), (reveal(fs, shape=sh2), -4), (reveal(fs, flags=_hip.FLAG_SEED_IN_HBM), -1)):
        assert rc == want and lib.d3pm_last_error(), (rc, want)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and (lp == 3.5).all() and (stp == 0).all(), "a refused call launches nothing"
    for kw in (dict(graph=True), dict(return_logprobs=1)):
        with pytest.raises(ValueError):
            m.generate_audio(texts[:1], proms[:1], seed=3, steps=3, **{"return_logprobs": True, **kw})


# ---- the loops ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native(built_lib):
    from vall_e.vall_e import AR, synth
    cfg = synth.D3PMConfig.native()
    sd = synth.make_state_dict(cfg, 0)
    texts, proms = synth.make_inputs(cfg, 3, 1)
    cache = {}

    def get(dtype):
        if dtype not in cache:
            m = AR.reference_native()
            m.load_state_dict(sd)
            cache[dtype] = m.to(dtype).to(DEV)
        return cache[dtype], cfg, texts, proms
    return get


DB, DCANVAS = 16, 768


@pytest.fixture(scope="module")
def d512(built_lib):
    """the shape of tests/test_gpu_dedup.py: 16 x 768, d = 512, two layers, bf16"""
    from vall_e.vall_e import AR, synth
    cfg = dataclasses.replace(synth.D3PMConfig.libritts(), n_heads=8, n_layers=2, canvas=DCANVAS, n_frames=700)
    m = AR.from_config(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, 0))
    m = m.to(torch.bfloat16).to(DEV)
    texts, proms = synth.make_inputs(cfg, DB, 1)
    ct, cp = m.encode_conditions(texts, proms)
    return m, cfg, texts, proms, ct, cp


@contextlib.contextmanager
def _ln_fold(value):
    from vall_e.vall_e import _hip
    saved = _hip.TUNING.ln_fold
    _hip.set_tuning_field("ln_fold", value)
    try:
        yield
    finally:
        _hip.set_tuning_field("ln_fold", saved)


STEPS = 6


def _pair(smp, x0, fm, kv, t0, *, reveal=None, **kw):
    """the unscored and the scored loop at the same seed -> (x, trace, scores) of the scored one, ids and trace asserted equal"""
    out = []
    for scored in (False, True):
        x = x0.clone()
        sk = dict(scores=smp.new_scores(x.shape[0])) if scored else {}
        if reveal is not None:
            tr = smp.reveal_loop(x, fm, reveal, kv[0], kv[1], seed=91, trace=True, **kw, **sk)
        else:
            tr = smp.sample_loop(x, fm, t0, t0 - STEPS, kv[0], kv[1], seed=91, trace=True, **kw, **sk)
        torch.cuda.synchronize()
        out.append((x, tr, sk.get("scores")))
    (xa, ta, _), (xb, tb, sc) = out
    assert torch.equal(xa, xb) and torch.equal(ta, tb), f"the scored loop moved {(ta != tb).sum().item()} ids of the trace"
    assert not torch.equal(xb, x0)
    return xb, tb, sc


def _check_step_against_trace(trace, ts, x0, fm, known, scores, mask_id=512):
    """9. step is the timestep of the first trace entry whose id is not the mask; -1 rows are exactly the padding and known rows (and
    rows that held an id at entry); logprob is finite, <= 0, and 0 exactly where step < 1."""
    x0n = x0.cpu().numpy()
    fmn = np.broadcast_to(fm.cpu().numpy(), x0n.shape)
    kn = np.zeros_like(x0n, dtype=np.uint8) if known is None else known.cpu().numpy()
    free = R.free_masked(x0n, fmn, kn, mask_id)
    want = R.first_reveal(trace.cpu().numpy(), ts, x0n, free, mask_id)
    lp, step = scores[0].cpu().numpy(), scores[1].cpu().numpy()
    assert np.array_equal(step, want), f"{(step != want).sum()} entries of step disagree with the trace"
    assert np.array_equal(step == -1, ~free)
    assert np.isfinite(lp).all() and (lp <= 0).all() and (lp[step < 1] == 0).all() and (lp[step >= 1] < 0).all()
    return int((step >= 1).sum())


# ---- 7. ids are untouched, 9. step agrees with the trace ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_scored_loops_return_the_ids_of_the_unscored_native(native, dtype):
    from vall_e.vall_e import _hip
    m, cfg, texts, proms = native(dtype)
    smp = m.sampler()
    t, p = list(texts[:2]), list(proms[:2])
    kv = smp.cond_kv(*m.encode_conditions(t, p))
    t0 = cfg.timesteps - 1
    ts = list(range(t0, t0 - STEPS, -1))
    x, fm = m.canvas_init(2)
    _, tr, sc = _pair(smp, x, fm, kv, t0)                                                     # plain
    assert _check_step_against_trace(tr, ts, x, fm, None, sc) > 0
    if dtype == torch.float32:
        return
    g = torch.Generator().manual_seed(3)
    lens = [cfg.canvas, 77]
    xk, fmk, km = m.canvas_init_known(2, lens, [torch.randint(0, 1024, (40,), generator=g), None])
    _, tr, sc = _pair(smp, xk, fmk, kv, t0, known=km)                                       # n_frames ragged + known
    assert _check_step_against_trace(tr, ts, xk, fmk, km, sc) > 0
    _, tr, sc = _pair(smp, xk, fmk, kv, t0, known=km, temperature=0.9, top_k=50, top_p=0.9)  # nucleus
    assert _check_step_against_trace(tr, ts, xk, fmk, km, sc) > 0
    f, tl, pl = m.key_lengths(t, p, lens)
    keys = tuple(torch.tensor(v, dtype=torch.int32, device=DEV) for v in (f, tl, pl))
    kvk = smp.cond_kv(*smp.encode_conditions(*m._padded_inputs(t, p), keys[1], keys[2]))
    _, tr, sc = _pair(smp, xk, fmk, kvk, t0, known=km, keys=keys)                          # keys
    assert _check_step_against_trace(tr, ts, xk, fmk, km, sc) > 0
    with _hip.tuning(regime_batch=0):
        nt, npm = m._null_conditions(t, None, 1), m._null_conditions(p, None, 2)
        kvg = smp.cond_kv(*m.encode_conditions(t + nt, p + npm))
        _, tr, sc = _pair(smp, x, fm, kvg, t0, guidance=1.5)                               # guidance
    assert _check_step_against_trace(tr, ts, x, fm, None, sc) > 0
    for ct in (0.0, 4.5):                                                                  # the reveal loop
        _, tr, sc = _pair(smp, xk, fmk, kv, t0, reveal=5, known=km, choice_temperature=ct)
        n = _check_step_against_trace(tr, smp.reveal_plan(5), xk, fmk, km, sc)
        assert n == int(R.free_masked(xk.cpu().numpy(), fmk.cpu().numpy(), km.cpu().numpy(), 512).sum()), "the reveal loop leaves no free row masked"


def test_scored_loops_return_the_ids_of_the_unscored_d512_and_fp8(d512):
    m, cfg, texts, proms, ct, cp = d512
    smp = m.sampler()
    kv = smp.cond_kv(ct, cp)
    x, fm = m.canvas_init(DB)
    t0 = cfg.timesteps - 1
    ts = list(range(t0, t0 - STEPS, -1))
    for kw in ({}, dict(fp8=True)):
        _, tr, sc = _pair(smp, x, fm, kv, t0, **kw)
        assert _check_step_against_trace(tr, ts, x, fm, None, sc) > 0


# ---- 8. loop = chained step entries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain fp16", "plain fp32", "guided", "reveal"])
def test_scored_loop_equals_the_chained_step_entries_native(native, mode):
    from vall_e.vall_e import _hip
    m, cfg, texts, proms = native(torch.float32 if mode == "plain fp32" else torch.float16)
    smp = m.sampler()
    t, p = list(texts[:2]), list(proms[:2])
    t0, seed, w = cfg.timesteps - 1, 17, 1.5
    with torch.cuda.device(DEV), _hip.tuning(regime_batch=0):
        if mode == "guided":
            t, p = t + m._null_conditions(t, None, 1), p + m._null_conditions(p, None, 2)
        kv_t, kv_p = smp.cond_kv(*m.encode_conditions(t, p))
        x0, fm = m.canvas_init(2)
        x, got, ref = x0.clone(), smp.new_scores(2), smp.new_scores(2)
        y = x0.clone()
        smp.frame_scores_init(y, fm, ref)
        if mode == "reveal":
            smp.reveal_loop(x, fm, 5, kv_t, kv_p, seed, scores=got)
            ts = smp.reveal_plan(5) + [0]
            for i in range(5):
                lg, _ = smp.denoise(y, fm, ts[i], kv_t, kv_p)
                y, _, _ = smp.reveal_step(lg, y, fm, ts[i], ts[i + 1], seed)
                smp.frame_scores_step(lg, y, ts[i], ref)
        else:
            smp.sample_loop(x, fm, t0, t0 - STEPS, kv_t, kv_p, seed, scores=got, **(dict(guidance=w) if mode == "guided" else {}))
            for tt in range(t0, t0 - STEPS, -1):
                if mode == "guided":
                    lg, _ = smp.denoise(torch.cat([y, y]).contiguous(), fm, tt, kv_t, kv_p)
                    y, _ = smp.posterior_sample(lg[:2], y, tt, seed, guidance=w, null_logits=lg[2:])
                    smp.frame_scores_step(lg[:2], y, tt, ref, guidance=w, null_logits=lg[2:])
                else:
                    lg, _ = smp.denoise(y, fm, tt, kv_t, kv_p)
                    y, _ = smp.posterior_sample(lg, y, tt, seed)
                    smp.frame_scores_step(lg, y, tt, ref)
        torch.cuda.synchronize()
    assert torch.equal(x, y)
    assert torch.equal(got[1], ref[1]), f"{(got[1] != ref[1]).sum().item()} entries of step differ"
    assert torch.equal(got[0], ref[0]), f"{(got[0] != ref[0]).sum().item()} values differ, largest {(got[0] - ref[0]).abs().max().item():.3e}"
    assert int((got[1] >= 1).sum()) > 0


# ---- 10. deduplicated shape --------------------------------------------------------------------------------------------------------------
def _launches(smp, x0, fm, kv, ln_fold, t_start, t_stop):
    """launches per kernel class in the bracketed iterations (t % 16 == 0) of a scored loop, as tests/test_gpu_dedup.py counts them"""
    from vall_e.vall_e import _hip
    try:
        _hip.prof_enable(_hip.K_ALL, 512)
        with _ln_fold(ln_fold):
            smp.sample_loop(x0.clone(), fm, t_start, t_stop, kv[0], kv[1], seed=91, scores=smp.new_scores(x0.shape[0]))
        torch.cuda.synchronize()
        counts = tuple(_hip.prof_read_class(k)[0] for k in range(_hip.K_ALL))
        assert sum(counts) > 0, "no iteration of this loop was bracketed"
        return counts
    finally:
        _hip.prof_disable()


def test_deduplicated_scored_loop_equals_the_every_row_loop(d512):
    """equal ids give equal logits bit for bit, so the compact row a canvas row reads through row_of holds the bits
    its own row would hold, and both grids of the two launch lists agree exactly."""
    from vall_e.vall_e import _hip
    m, cfg, texts, proms, ct, cp = d512
    smp = m.sampler()
    kv = smp.cond_kv(ct, cp)
    x0, fm = m.canvas_init(DB)
    t0 = cfg.timesteps - 1
    a, b = _launches(smp, x0, fm, kv, 1, 97, 94), _launches(smp, x0, fm, kv, 3, 97, 94)
    assert a != b, "the scored default loop runs the deduplicated launch list"
    assert a[_hip.K_SAMPLE] == b[_hip.K_SAMPLE] == 2, "the sampler launch and the launch behind it, once per bracketed iteration"
    out = {}
    for ln_fold in (1, 3):
        x, sc = x0.clone(), smp.new_scores(DB)
        with _ln_fold(ln_fold):
            smp.sample_loop(x, fm, t0, t0 - STEPS, kv[0], kv[1], seed=91, scores=sc)
        torch.cuda.synchronize()
        out[ln_fold] = (x, sc)
    (xa, sa), (xb, sb) = out[1], out[3]
    assert torch.equal(xa, xb) and torch.equal(sa[1], sb[1]), "ids and step"
    assert int((sa[1] >= 1).sum()) > 0
    diff = (sa[0] - sb[0]).abs().max().item()
    assert torch.equal(sa[0], sb[0]), f"logprob differs between ln_fold = 1 and 3 where ids and step agree: largest difference {diff:.3e}"


# ---- 11. batch independence ---------------------------------------------------------------------------------------------------------------
def _ragged_batch_against_each_utterance_alone(m, cfg, texts, proms, lens, known, cases, logprob_bits):
    """-> the largest |logprob difference| met (0.0 where the grids are bit-equal).  ids and step are asserted bit for bit always,
    logprob where logprob_bits says so."""
    Bn, worst = len(lens), 0.0
    texts, proms = list(texts[:Bn]), list(proms[:Bn])

    def same(got, ref, what):
        nonlocal worst
        assert torch.equal(got[0], ref[0]), f"{what}: ids"
        assert torch.equal(got[1].step, ref[1].step), f"{what}: step"
        d = (got[1].logprob - ref[1].logprob).abs().max().item()
        worst = max(worst, d)
        if logprob_bits:
            assert torch.equal(got[1].logprob, ref[1].logprob), f"{what}: logprob, largest difference {d:.3e}"
    for kw in cases:
        kw = dict(seed=5, return_logprobs=True, **kw)
        ids, sc = m.generate_audio(texts, proms, n_frames=lens, known=known, **kw)
        assert type(sc).__name__ == "FrameScores" and sc.logprob.dtype == torch.float32 and sc.step.dtype == torch.int32
        assert tuple(sc.logprob.shape) == tuple(sc.step.shape) == tuple(ids.shape) == (Bn, cfg.canvas)
        assert torch.equal(ids, m.generate_audio(texts, proms, n_frames=lens, known=known, **{**kw, "return_logprobs": False}))
        assert int((sc.step >= 1).sum()) > 0 and (sc.step[0, :40] == -1).all() and (sc.step[-1, lens[-1]:] == -1).all()
        for b in range(Bn):
            one, s1 = m.generate_audio([texts[b]], [proms[b]], n_frames=[lens[b]], known=[known[b]], utt0=b, global_batch=Bn, **kw)
            assert tuple(s1.step.shape) == (cfg.canvas,), "squeezed like the ids of one utterance"
            same((one, s1), (ids[b], type(sc)(sc.logprob[b], sc.step[b])), f"utterance {b} alone")
        same(m.generate_audio(texts, proms, n_frames=lens, known=known, streams=2, **kw), (ids, sc), "two stream chunks")
    return worst


def _known3():
    g = torch.Generator().manual_seed(9)
    return [torch.randint(0, 1024, (40,), generator=g), None, torch.randint(0, 1024, (5,), generator=g)]


CASES = (dict(steps=STEPS), dict(reveal_steps=4, choice_temperature=1.0), dict(steps=4, guidance=1.5, top_p=0.9))


def test_a_scored_utterance_of_a_ragged_batch_is_that_utterance_alone_native_fp32(native):
    """fp32 runs on the generic kernels alone, whose rows do not depend on the batch they ride in: both grids bit for bit."""
    m, cfg, texts, proms = native(torch.float32)
    _ragged_batch_against_each_utterance_alone(m, cfg, texts, proms, [cfg.canvas, 300, 77], _known3(), CASES, logprob_bits=True)
    ids, tr, sc = m.generate_audio(texts[:1], proms[:1], seed=5, steps=3, return_trace=True, return_logprobs=True)
    assert tuple(tr.shape) == (3, 1, cfg.canvas) and tuple(sc.step.shape) == (cfg.canvas,)


def test_a_scored_utterance_of_a_ragged_batch_is_that_utterance_alone_d512(d512):
    """d = 512, bf16: every projection runs on an MFMA family whatever the batch (they accumulate in one order, csrc/d3pm_plan.cpp) and
    the attention shape follows the declared logical batch: both grids bit for bit, the batch deduplicated or not."""
    m, cfg, texts, proms, _, _ = d512
    _ragged_batch_against_each_utterance_alone(m, cfg, texts, proms, [cfg.canvas, 333, 77], _known3(), CASES, logprob_bits=True)


def test_a_scored_utterance_of_a_ragged_batch_native_fp16_ids_and_step(native):
    """The native shape in fp16 is the one place where the LOGITS of an utterance depend on the batch it rides in: at d = 32 the planner
    (csrc/d3pm_plan.cpp plan_linear) takes fc2 (N = 32, K = 128) to the generic fp32 kernel at one utterance (448 rows) and to the
    128 x 128 MFMA kernel at two or three (896 / 1344 rows), which accumulate in different orders, so the fp16 logits move in their
    last bit.  That is the denoiser as it stands, not this feature: ids and step are asserted bit for bit; logprob, a function of
    those logits, is only measured here.  Measured on MI355X: largest |difference| 2.9e-3 (one fp16 quantum of a logit of magnitude
    4 .. 8 is 3.9e-3); at fp32 and at d = 512 the two tests above hold bit for bit."""
    m, cfg, texts, proms = native(torch.float16)
    worst = _ragged_batch_against_each_utterance_alone(m, cfg, texts, proms, [cfg.canvas, 300, 77], _known3(), CASES, logprob_bits=False)
    print(f"[logprob] native fp16, utterance alone / stream chunks vs the batch: largest |logprob difference| {worst:.3e}")

"""Reveal with revision (include/d3pm_hip.h: d3pm_revise) on the GPU.

What carries no tolerance: given the scores and candidates the device reports, the ids of a step equal the host selection of
tests/revise_ref.py, id for id; a masked row's cand / score are those of d3pm_reveal_step bit for bit; a held row's score without order
noise is float32(lp) + float32(bonus) with lp what d3pm_frame_scores_step reports, bit for bit; the masked count after every step equals
the plan; the loop equals its step entries, grids included; an utterance does not depend on the batch it rides in.  What carries one:
lp sits within 1.0e-4 of the float64 definition (tests/logprob_ref.py: the header's bound), and a held row's score with order noise within
1.0e-4 + lambda * 1e-5 of the float64 value with the keyed Gumbel (the bound of test_gpu_reveal.py; the fp32 add of the bonus, one
rounding at magnitude <= 64 = 3.8e-6, fits the 3.2e-5 the header's budget leaves).
python -m pytest tests/test_gpu_revise.py -m gpu"""
import ctypes as C

import numpy as np
import pytest
import torch

import logprob_ref as L
import reveal_ref as R
import revise_ref as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1.0e-4
CAND0, SCORE0 = -7, 12345.0      # what cand_out / score_out hold before a step: rows that are not free keep them


def pp(v):
    return None if v is None else C.c_void_p(v.data_ptr())


def _dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


class Step:
    """d3pm_reveal_step_revise / d3pm_reveal_step / d3pm_frame_scores_step on a bare shape (no weights): K and the canvas are free."""

    def __init__(self, K=1025, canvas=448):
        from vall_e.vall_e import _hip, synth
        self.hip = _hip
        self.shape = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
        self.shape.n_classes, self.shape.mask_id, self.shape.canvas, self.shape.n_q = K, K // 2, canvas, 1
        self.K, self.canvas, self.mask_id = K, canvas, K // 2
        self.sched = _hip.Schedule(100)
        self.cbar = R.cbar_f32(self.sched.cbar)

    def keep_frac(self, t_next):
        return np.float32(self.cbar[t_next]) if t_next > 0 else np.float32(0.0)

    def __call__(self, logits, x_t, fm, t, t_next, seed, *, bonus=0.0, known=None, nucleus=None, ct=0.0, flags=0, utt0=0, in_place=False,
                 shared=False, scores=None):
        """-> x_next, cand, score (numpy).  bonus None: d3pm_reveal_step on the same arguments."""
        hip = self.hip
        logits, x_t, fm = _dev(logits), _dev(x_t), _dev(fm)
        known = None if known is None else _dev(known)
        B = x_t.shape[0]
        assert x_t.dtype == torch.int32 and logits.shape == (B, self.canvas, self.K) and x_t.shape[1] == self.canvas
        x_next = x_t.clone() if in_place else torch.full_like(x_t, -7)
        src = x_next if in_place else x_t
        cand = torch.full(x_t.shape, CAND0, dtype=torch.int32, device=DEV)
        score = torch.full(x_t.shape, SCORE0, dtype=torch.float32, device=DEV)
        cv = hip.Canvas(fm.data_ptr(), None if known is None else known.data_ptr())
        nu = None if nucleus is None else hip.Nucleus(*nucleus)
        head = (C.byref(self.shape), B, pp(logits), hip.dtype_code(logits.dtype), pp(src), pp(x_next), pp(fm) if shared else None,
                None if shared else C.byref(cv), int(t), int(t_next), C.byref(self.sched.c_struct), seed, utt0, flags, None if nu is None else C.byref(nu),
                float(ct), pp(cand), pp(score))
        if bonus is None:
            hip.check(hip.lib().d3pm_reveal_step(*head, hip.stream_ptr()), "d3pm_reveal_step")
        else:
            rs = hip.Revise(bonus)
            fs = None if scores is None else hip.FrameScores(scores[0].data_ptr(), scores[1].data_ptr())
            hip.check(hip.lib().d3pm_reveal_step_revise(*head, C.byref(rs), None if fs is None else C.byref(fs), hip.stream_ptr()),
                      "d3pm_reveal_step_revise")
        torch.cuda.synchronize()
        return x_next.cpu().numpy(), cand.cpu().numpy(), score.cpu().numpy()

    def logprob(self, logits, x_t, held, t=60):
        """lp of the held rows as d3pm_frame_scores_step reports it: grids with step 0 on those rows, x_next = x_t -> float32 numpy"""
        hip = self.hip
        logits, x_t = _dev(logits), _dev(x_t)
        lp = torch.zeros(x_t.shape, dtype=torch.float32, device=DEV)
        st = _dev(np.where(held, 0, -1).astype(np.int32))
        fs = hip.FrameScores(lp.data_ptr(), st.data_ptr())
        hip.check(hip.lib().d3pm_frame_scores_step(C.byref(self.shape), x_t.shape[0], pp(logits), hip.dtype_code(logits.dtype), self.K, None, None,
                                                   pp(x_t), int(t), C.byref(fs), hip.stream_ptr()), "d3pm_frame_scores_step")
        torch.cuda.synchronize()
        assert np.array_equal(st.cpu().numpy() == t, held)
        return lp.cpu().numpy()


CANVASES = [5, 64, 70, 448]      # less than one key slot, exactly one, two with a partial last one, the native canvas


# ---- 1. selection, exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1025, 777])
@pytest.mark.parametrize("canvas", CANVASES)
def test_selection_equals_the_host_selection_on_the_devices_scores(built_lib, K, canvas):
    """Two canvases: `a` with 30 % of the rows held, and `b` with 80 % of them held under the step (99, 98), whose cbar[98] = 0.9995 lets
    an utterance hold a single id, so that held rows MUST be re-masked; the last steps (t_next = 0) hold F ids and reveal every masked
    row."""
    st = Step(K, canvas)
    a = V.case(K, canvas, seed=K + canvas, held=0.3)
    b = V.case(K, canvas, seed=K + canvas + 1, held=0.8)
    seen = set()
    runs = [(a, (99, 98), 0, 0.0, 0, 0.0), (a, (99, 0), 0, 0.0, 0, 0.0), (a, (60, 40), 0, 0.0, 5, 0.5), (a, (60, 40), 1, 0.0, 0, 0.0),
            (a, (30, 12), 0, 2.0, 3, 0.5), (a, (1, 0), 1, 0.0, 0, 3.0), (b, (99, 98), 0, 0.0, 0, 0.5), (b, (30, 12), 0, 2.0, 0, 0.0)]
    for (l, x, fm, known, _), (t, t_next), flags, ct, utt0, bonus in runs:
        masked, held, free = V.kinds(x, fm, known, st.mask_id)
        kw = dict(seed=11, known=known, flags=flags, ct=ct, utt0=utt0, bonus=bonus)
        out, cand, score = st(_dev(l, torch.float16), x, fm, t, t_next, **kw)
        want = V.step(x, fm, known, cand, score, st.mask_id, st.keep_frac(t_next))
        assert np.array_equal(out, want), f"t={t}->{t_next}: {np.sum(out != want)} ids differ from the host selection"
        assert np.array_equal(out[~free], x[~free]), "known and padded rows equal x_t"
        assert (cand[~free] == CAND0).all() and (score[~free] == SCORE0).all(), "rows that are not free are left unwritten"
        assert np.isfinite(score[free]).all() and (cand[free] != st.mask_id).all() and np.array_equal(cand[held], x[held])
        now = free & (out != st.mask_id)
        assert np.array_equal(out[now], cand[now])
        for u in range(x.shape[0]):
            F, hold = int(free[u].sum()), V.hold_count(int(free[u].sum()), st.keep_frac(t_next))
            assert int(now[u].sum()) == hold, (u, F, hold)
            if hold == F and F:
                seen.add("hold = F")
        if (held & ~now).any():
            seen.add("re-masked")
        if (masked & now).any():
            seen.add("revealed")
        out2, _, _ = st(_dev(l, torch.float16), x, fm, t, t_next, in_place=True, **kw)
        assert np.array_equal(out2, out), "in place"
    # crafted so: canvas b's first utterance has more held rows than the step (99, 98) lets it hold
    _, held_b, free_b = V.kinds(b[1], b[2], b[3], st.mask_id)
    assert int(held_b[0].sum()) > V.hold_count(int(free_b[0].sum()), st.keep_frac(98))
    assert seen == {"hold = F", "re-masked", "revealed"}, seen


# ---- 2. masked rows: d3pm_reveal's, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1025, 777])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_masked_rows_are_scored_as_by_the_reveal_step_bit_for_bit(built_lib, dtype, K):
    canvas, t, t_next = 70, 60, 40
    st = Step(K, canvas)
    l, x, fm, known, _ = V.case(K, canvas, seed=K + 2)
    masked, held, _ = V.kinds(x, fm, known, st.mask_id)
    assert masked.sum() > 40 and held.sum() > 20
    logits = _dev(l, dtype)
    for nucleus in (None, (0.7, 50, 0.9)):
        for flags, ct in ((0, 2.0), (0, 0.0), (1, 2.0)):
            kw = dict(seed=21, known=known, nucleus=nucleus, ct=ct, flags=flags, utt0=2)
            _, c0, s0 = st(logits, x, fm, t, t_next, bonus=None, **kw)
            _, c1, s1 = st(logits, x, fm, t, t_next, bonus=0.5, **kw)
            assert np.array_equal(c1[masked], c0[masked]), (nucleus, flags, ct)
            assert np.array_equal(s1[masked].view(np.uint32), s0[masked].view(np.uint32)), (nucleus, flags, ct)
            assert (c0[held] == CAND0).all() and np.array_equal(c1[held], x[held])


# ---- 3. held rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1025, 777])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_held_rows_score_the_log_probability_of_their_id_plus_the_bonus(built_lib, dtype, K):
    from vall_e.vall_e import _hip
    canvas, seed, utt0 = 70, 33, 1
    st = Step(K, canvas)
    l, x, fm, known, _ = V.case(K, canvas, seed=K + 4, held=0.5)
    _, held, _ = V.kinds(x, fm, known, st.mask_id)
    logits = _dev(l, dtype)
    lp = st.logprob(logits, x, held)
    rows = np.flatnonzero(held.reshape(-1))
    lp64 = L.logprob64(logits.float().cpu().numpy().reshape(-1, K)[rows], st.mask_id, x.reshape(-1)[rows])
    err = np.abs(lp.reshape(-1)[rows].astype(np.float64) - lp64).max()
    print(f"[revise held] K={K} {dtype}: max |lp - logprob64| = {err:.3e} (bound {L.TOL:.1e})")
    assert err <= L.TOL
    # no order noise: one fp32 add, bit for bit -- also under a sampling filter (it does not touch held rows) and under greedy
    for bonus in (0.0, 0.5, 3.0):
        for nucleus, flags, ct, t_next in ((None, 0, 0.0, 40), ((0.7, 50, 0.9), 0, 0.0, 40), (None, 1, 4.5, 40), (None, 0, 4.5, 0)):
            _, cand, score = st(logits, x, fm, 60, t_next, seed, bonus=bonus, known=known, nucleus=nucleus, ct=ct, flags=flags, utt0=utt0)
            assert np.array_equal(cand[held], x[held])
            want = (lp[held] + np.float32(bonus)).astype(np.float32)
            assert np.array_equal(score[held].view(np.uint32), want.view(np.uint32)), (bonus, nucleus, flags, ct, t_next)
    # choice_temperature: the keyed Gumbel of stream 4, scaled by lambda = ct * float(cbar[t_next])
    ct, bonus = 4.5, 0.5
    for t, t_next in ((60, 40), (99, 93)):
        v = _hip.uniform(seed, t, utt0 * canvas, 3 * canvas, 4, 4, DEV).cpu().numpy()[rows, 0]
        lam = np.float32(ct) * st.keep_frac(t_next)
        _, cand, score = st(logits, x, fm, t, t_next, seed, bonus=bonus, known=known, ct=ct, utt0=utt0)
        want = lp64 + bonus + np.float64(lam) * R.gumbel64(v)
        err = np.abs(score.reshape(-1)[rows].astype(np.float64) - want).max()
        print(f"[revise held] K={K} {dtype} t={t}->{t_next} lambda={lam:.4f}: max error {err:.3e}")
        assert err <= TOL + float(lam) * 1e-5
        assert np.array_equal(cand[held], x[held])


# ---- 4. a bonus that pins every held row ------------------------------------------------------------------------------------------------
def _crafted(st, seed=5):
    """F = 70 free rows each, keep = floor(70 cbar[50]); the utterances hold keep + 5, keep and keep - 4 masked rows."""
    canvas = st.canvas
    keep = 70 - V.hold_count(70, st.keep_frac(50))
    assert 6 <= keep <= 60
    g = np.random.default_rng(seed)
    fm = np.ones((3, canvas), np.uint8)
    x = g.integers(0, 500, (3, canvas)).astype(np.int32)
    pos = [g.permutation(canvas)[:keep + extra] for extra in (5, 0, -4)]
    for b in range(3):
        x[b, pos[b]] = st.mask_id
    l = (g.standard_normal((3, canvas, st.K)) * 3).astype(np.float32)
    return l, x, fm, keep


def test_a_large_bonus_pins_held_rows_and_only_the_quota_remasks(built_lib):
    st = Step(1025, 70)
    l, x, fm, keep = _crafted(st)
    masked, held, free = V.kinds(x, fm, None, st.mask_id)
    logits = _dev(l, torch.float16)
    out, cand, score = st(logits, x, fm, 70, 50, seed=3, bonus=1.0e4)
    ref, _, _ = st(logits, x, fm, 70, 50, seed=3, bonus=None)
    for b in (0, 1):      # masked >= floor(F kf): every held row stays, the masked rows compete as under d3pm_reveal
        assert np.array_equal(out[b], ref[b]), b
    assert [(out[b] != x[b]).sum() for b in (0, 1)] == [5, 0]
    gone = held[2] & (out[2] == st.mask_id)
    assert int(gone.sum()) == 4 and np.array_equal(out[2][~gone], x[2][~gone]), "exactly floor(F kf) - masked held rows are re-masked"
    # ... those with the lowest score = float32(lp + 1e4), ties at the higher frame index
    lp = st.logprob(logits, x, held)
    s2 = (lp[2] + np.float32(1.0e4)).astype(np.float32)
    assert np.array_equal(score[2][held[2]].view(np.uint32), s2[held[2]].view(np.uint32))
    idx = np.flatnonzero(held[2])
    worst = idx[np.lexsort((-idx, s2[idx]))][:4]
    assert np.array_equal(np.sort(worst), np.flatnonzero(gone))
    # in lp itself: no re-masked row is surer than a kept one by more than the spacing of fp32 at 1e4 (2^-10), which the add rounds to
    assert lp[2][gone].max() <= lp[2][held[2] & ~gone].min() + 2.0 ** -10


# ---- 5. constant logits, greedy: every score of one kind ties ---------------------------------------------------------------------------
def test_constant_logits_under_greedy_who_wins_the_ties(built_lib):
    """Constant logits: a masked row's conf and a held row's conf_h are the same number, log(1 / 1024) in the kernel's arithmetic.
    bonus 0: ALL free rows tie, the first `hold` frames of the utterance hold an id after the step (the masked ones among them take
    class 0, the greedy candidate), every later frame is masked.  bonus 0.5: the held rows come first, in frame order; then the masked
    rows, in frame order."""
    st = Step(1025, 70)
    _, x, fm, keep = _crafted(st)
    masked, held, _ = V.kinds(x, fm, None, st.mask_id)
    hold = 70 - keep
    lc = _dev(np.full((3, 70, 1025), 0.75, np.float32), torch.float16)
    out, cand, score = st(lc, x, fm[0], 70, 50, seed=3, bonus=0.0, flags=1, shared=True)
    assert len(np.unique(score.view(np.uint32))) == 1, "held and masked rows tie bit for bit"
    for b in range(3):
        want = np.where(np.arange(70) < hold, np.where(masked[b], 0, x[b]), st.mask_id)
        assert np.array_equal(out[b], want), b
    out, cand, score = st(lc, x, fm[0], 70, 50, seed=3, bonus=0.5, flags=1, shared=True)
    assert len(np.unique(score[held])) == 1 and len(np.unique(score[masked])) == 1 and score[held][0] > score[masked][0]
    for b in range(3):
        h, m = np.flatnonzero(held[b]), np.flatnonzero(masked[b])
        want = np.full(70, st.mask_id)
        want[h[:hold]] = x[b][h[:hold]]
        want[m[:max(0, hold - len(h))]] = 0
        assert np.array_equal(out[b], want), b
    assert (held[2].sum() > hold) and (held[0].sum() < hold)


# ---- 6. - 9. on models ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native(built_lib):
    from vall_e.vall_e import AR, synth
    cfg = synth.D3PMConfig.native()
    m = AR.reference_native()
    m.load_state_dict(synth.make_state_dict(cfg, 0))
    m = m.half().to(DEV)
    texts, proms = synth.make_inputs(cfg, 3, 1)
    return m, cfg, texts, proms


LENS = [448, 300, 77]


def _known():
    g = torch.Generator().manual_seed(9)
    return [torch.randint(0, 1024, (40,), generator=g), None, torch.randint(0, 1024, (5,), generator=g)]


def _loop_vs_steps(m, cfg, texts, proms, lens, known, N, bonus, **kw):
    """the loop with trace and frame scores against d3pm_frame_scores_init + the chained step entries; then the loop without scores"""
    smp = m.sampler()
    B = len(texts)
    ct, cp = m.encode_conditions(texts, proms)
    kv_t, kv_p = smp.cond_kv(ct, cp)
    x, fm, kmap = m.canvas_init_known(B, lens, known)
    xs, x2 = x.clone(), x.clone()
    got, ref = smp.new_scores(B), smp.new_scores(B)
    trace = smp.reveal_loop(x, fm, N, kv_t, kv_p, seed=77, trace=True, known=kmap, revise=bonus, scores=got, **kw)
    ts = smp.reveal_plan(N) + [0]
    smp.frame_scores_init(xs, fm, ref, known=kmap)
    remasked = 0
    for i in range(N):
        lg, _ = smp.denoise_canvas(xs, fm, ts[i], kv_t, kv_p)
        nxt, _, _ = smp.reveal_step(lg, xs, fm, ts[i], ts[i + 1], seed=77, known=kmap, revise=bonus, scores=ref, **kw)
        smp.frame_scores_step(lg, nxt, ts[i], ref)
        assert torch.equal(trace[i], nxt), f"step {i} (t={ts[i]}): the loop and the step entries disagree on {(trace[i] != nxt).sum().item()} ids"
        remasked += int(((xs != 512) & (nxt == 512)).sum())
        xs = nxt
    torch.cuda.synchronize()
    assert torch.equal(x, xs)
    assert torch.equal(got[1], ref[1]), f"{(got[1] != ref[1]).sum().item()} entries of step differ"
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)), f"{(got[0] != ref[0]).sum().item()} values of logprob differ"
    trace2 = smp.reveal_loop(x2, fm, N, kv_t, kv_p, seed=77, trace=True, known=kmap, revise=bonus, **kw)
    assert torch.equal(trace2, trace) and torch.equal(x2, x), "the grids do not move an id"
    return remasked


def test_loop_equals_steps_native_fp16(native):
    m, cfg, texts, proms = native
    _loop_vs_steps(m, cfg, texts, proms, LENS, _known(), 6, 0.0)
    _loop_vs_steps(m, cfg, texts, proms, LENS, _known(), 3, 0.5, temperature=0.7, top_k=50, top_p=0.9, choice_temperature=4.5)


@pytest.mark.parametrize("with_known", [True, False], ids=["known", "none_known"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_loop_equals_steps_d512_bf16_fused_commit(built_lib, dtype, with_known):
    """The d = 512 16-bit configurations take the folded LayerNorms, so the loop's second launch is reveal_commit_prep_rows (commit +
    the next evaluation's embedding rows, moments and fc1 fold), in whichever moment format the plan picks: every instantiation of it
    under kRevise = true (dtype x known-frame map or none).  N = 3: two fused commits, x -> x_alt and x_alt -> x, then the unfused last."""
    from vall_e.vall_e import AR, synth
    cfg = synth.D3PMConfig.libritts()
    m = AR.from_config(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, 0))
    m = m.to(dtype).to(DEV)
    texts, proms = synth.make_inputs(cfg, 2, 1)
    g = torch.Generator().manual_seed(4)
    known = [torch.randint(0, 1024, (60,), generator=g), None] if with_known else [None, None]
    assert (m.canvas_init_known(2, [750, 333], known)[2] is None) == (not with_known)
    n = _loop_vs_steps(m, cfg, texts, proms, [750, 333], known, 3, 0.0, choice_temperature=1.0)
    print(f"[fused commit {dtype} known={with_known}] rows re-masked in 3 steps: {n}")
    if dtype == torch.bfloat16 and with_known:
        assert n > 0, "the fused commit re-masked rows"


@pytest.mark.parametrize("N", [1, 4, 16])
def test_masked_counts_follow_the_plan_and_the_scores_follow_the_trace(native, N):
    m, cfg, texts, proms = native
    known = _known()
    out, trace, fs = m.generate_audio(texts, proms, seed=5, n_frames=LENS, known=known, reveal_steps=N, choice_temperature=1.0, revise=0.0,
                                      return_trace=True, return_logprobs=True)
    assert trace.shape == (N, 3, cfg.canvas) and torch.equal(trace[-1].long(), out)
    smp = m.sampler()
    cbar = R.cbar_f32(smp.schedule.cbar)
    ts = smp.reveal_plan(N)
    x0, fm, kmap = (v.cpu().numpy() for v in m.canvas_init_known(3, LENS, known))
    tr, step, lp = trace.cpu().numpy(), fs.step.cpu().numpy(), fs.logprob.cpu().numpy()
    masked, held, free = V.kinds(x0, fm, kmap, 512)
    remasked = 0
    for b in range(3):
        got = [int((tr[i, b][free[b]] == 512).sum()) for i in range(N)]
        assert got == V.plan(int(free[b].sum()), cbar, cfg.timesteps, N), (b, got)
        assert (tr[-1, b][free[b]] != 512).all(), "at the end no free row holds the mask id"
        k = kmap[b] != 0
        for i in range(N):
            assert np.array_equal(tr[i, b][k], x0[b][k]), "known ids come back unchanged"
            assert (tr[i, b][LENS[b]:] == 0).all(), "padded rows stay 0"
            prev = x0[b] if i == 0 else tr[i - 1, b]
            remasked += int((free[b] & (prev != 512) & (tr[i, b] == 512)).sum())
    want = V.last_reveal(tr, ts, x0, free, 512)
    assert np.array_equal(step, want), f"{(step != want).sum()} entries of step disagree with the trace"
    assert np.array_equal(step >= 1, free), "every free row left the mask at some step"
    assert np.isfinite(lp).all() and (lp[step < 1] == 0).all() and (lp[step >= 1] < 0).all()
    if N == 16:
        assert remasked > 0, "with fresh order noise every step, sixteen steps re-mask at least one row"
        assert len(np.unique(step[free])) > 2
    if N == 1:
        assert remasked == 0 and (step[free] == ts[0]).all()


def test_utterances_are_independent_of_batch_shards_and_streams(native):
    """On the native shape in fp32, which runs on the generic kernels alone: their rows do not depend on the batch they ride in.  In
    fp16 this shape is the one place where the LOGITS of an utterance move in their last bit with the batch (csrc/d3pm_plan.cpp
    plan_linear takes fc2 to the generic kernel at 448 rows and to an MFMA kernel at 896 / 1344; tests/test_gpu_logprob.py measures
    2.9e-3 on logprob there) -- the denoiser as it stands; a held row's score IS that logprob, so there a near tie can fall the other
    way (measured: utterance 2 of 3 alone differs from the batch in fp16)."""
    from vall_e.vall_e import AR, synth
    _, cfg, texts, proms = native
    m = AR.reference_native()
    m.load_state_dict(synth.make_state_dict(cfg, 0))
    m = m.float().to(DEV)
    known = _known()
    for extra in ({}, dict(mask_padding=True)):
        kw = dict(seed=5, reveal_steps=4, choice_temperature=1.0, revise=0.5, **extra)
        full = m.generate_audio(texts, proms, n_frames=LENS, known=known, **kw)
        for b in range(3):
            alone = m.generate_audio([texts[b]], [proms[b]], n_frames=[LENS[b]], known=[known[b]], utt0=b, global_batch=3, **kw)
            assert torch.equal(alone, full[b]), f"utterance {b} alone differs from the batch ({extra})"
        shards = torch.cat([m.generate_audio(texts[:2], proms[:2], n_frames=LENS[:2], known=known[:2], utt0=0, global_batch=3, **kw),
                            m.generate_audio(texts[2:], proms[2:], n_frames=LENS[2:], known=known[2:], utt0=2, global_batch=3, **kw)[None]])
        assert torch.equal(shards, full)
        assert torch.equal(m.generate_audio(texts, proms, n_frames=LENS, known=known, streams=2, **kw), full)


def test_revise_none_is_the_loop_it_was(native):
    m, cfg, texts, proms = native
    kw = dict(seed=5, n_frames=LENS, known=_known(), reveal_steps=6, choice_temperature=1.0, return_trace=True)
    out0, tr0 = m.generate_audio(texts, proms, **kw)
    out1, tr1 = m.generate_audio(texts, proms, revise=None, **kw)
    assert torch.equal(out0, out1) and torch.equal(tr0, tr1)
    out2, tr2 = m.generate_audio(texts, proms, revise=0.0, **kw)
    assert not torch.equal(tr2, tr0), "a bonus of 0 is ON: held and masked rows on equal terms"

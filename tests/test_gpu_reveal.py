"""Confidence-ordered reveal in N denoiser evaluations (include/d3pm_hip.h: d3pm_reveal) on the GPU.

What carries no tolerance: given the scores and candidates the device reports (cand_out / score_out of the step entry), the ids of a
step equal the host selection of tests/reveal_ref.py, id for id; the masked count after every step equals the plan; the loop equals
its step entries; an utterance does not depend on the batch it rides in.  What carries one: a score sits within 1.0e-4 of
log_softmax64(z''')[cand] (relative error of S <= (n_classes + 8) 2^-24 = 6.2e-5, three fp32 roundings at magnitude <= 32 add
3 * 2^-19 = 5.7e-6), and a noisy candidate may differ from the float64 mirror only where the mirror's two best scores are closer than
1.0e-3 (it must then be the runner-up; at most 1 % of the rows).
python -m pytest tests/test_gpu_reveal.py -m gpu"""
import ctypes as C

import numpy as np
import pytest
import torch

import reveal_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCORE_TOL = 1.0e-4
GAP = 1.0e-3


class Step:
    """d3pm_reveal_step on a bare shape (no weights): K and the canvas are free."""

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

    def __call__(self, logits, x_t, fm, t, t_next, seed, *, known=None, nucleus=None, ct=0.0, flags=0, utt0=0, in_place=False, shared=False):
        hip = self.hip
        logits, x_t, fm = logits.to(DEV).contiguous(), x_t.to(DEV).contiguous(), fm.to(DEV).contiguous()
        known = None if known is None else known.to(DEV).contiguous()
        B = x_t.shape[0]
        assert x_t.dtype == torch.int32 and logits.shape == (B, self.canvas, self.K) and x_t.shape[1] == self.canvas
        x_next = x_t.clone() if in_place else torch.full_like(x_t, -7)
        src = x_next if in_place else x_t
        cand = torch.full(x_t.shape, -7, dtype=torch.int32, device=DEV)
        score = torch.full(x_t.shape, 12345.0, dtype=torch.float32, device=DEV)
        pp = lambda v: None if v is None else C.c_void_p(v.data_ptr())
        cv = hip.Canvas(fm.data_ptr(), None if known is None else known.data_ptr())
        nu = None if nucleus is None else hip.Nucleus(*nucleus)
        hip.check(hip.lib().d3pm_reveal_step(C.byref(self.shape), B, pp(logits), hip.dtype_code(logits.dtype), pp(src), pp(x_next),
                                             pp(fm) if shared else None, None if shared else C.byref(cv), int(t), int(t_next),
                                             C.byref(self.sched.c_struct), seed, utt0, flags, None if nu is None else C.byref(nu), float(ct),
                                             pp(cand), pp(score), hip.stream_ptr()), "d3pm_reveal_step")
        torch.cuda.synchronize()
        return x_next.cpu().numpy(), cand.cpu().numpy(), score.cpu().numpy()


def _case(K, canvas, seed, B=3, revealed=0.3, with_known=True):
    """Ragged batch of B utterances: logits of the randn * 3 kind with every fifth row constant, x_t with masked rows, already revealed
    rows mixed in, known rows (utterances 0 and 1) and padded rows (0 beyond the utterance's length)."""
    g = torch.Generator().manual_seed(seed)
    mask_id = K // 2
    lens = [canvas, max(1, (2 * canvas) // 3), max(1, canvas // 3)][:B]
    l = torch.randn(B, canvas, K, generator=g) * 3
    l[:, 0::5] = 0.75
    fm = (torch.arange(canvas)[None] < torch.tensor(lens)[:, None]).to(torch.uint8)
    ids = torch.randint(0, min(K, 1024), (B, canvas), generator=g)
    ids = torch.where(ids == mask_id, ids + 1, ids)
    x = torch.full((B, canvas), mask_id, dtype=torch.int64)
    done = torch.rand(B, canvas, generator=g) < revealed
    x = torch.where(done, ids, x)
    known = torch.zeros(B, canvas, dtype=torch.uint8)
    if with_known:
        known[0, : max(1, canvas // 8)] = 1
        known[1, 1::7] = 1
        known &= fm
        x = torch.where(known != 0, (ids + 3) % min(K, 1024), x)
        x[1, 1] = mask_id if known[1, 1] else x[1, 1]          # a known 512 is legal and is not a masked row
    x = torch.where(fm != 0, x, torch.zeros_like(x)).to(torch.int32)
    return l, x, fm, (known if with_known else None), lens


def _masked(x, fm, known, mask_id):
    x, fm = np.asarray(x), np.asarray(fm) != 0
    free = fm & ~(np.zeros_like(fm) if known is None else np.asarray(known) != 0)
    return free & (x == mask_id), free


CANVASES = [5, 64, 70, 448]      # less than one key slot, exactly one, two with a partial last one, the native canvas


# ---- 1. selection, exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1025, 777])
@pytest.mark.parametrize("canvas", CANVASES)
def test_selection_equals_the_host_selection_on_the_devices_scores(built_lib, K, canvas):
    st = Step(K, canvas)
    l, x, fm, known, _ = _case(K, canvas, seed=K + canvas)
    xn, fn, kn = x.numpy(), fm.numpy(), known.numpy()
    masked, free = _masked(xn, fn, kn, st.mask_id)
    seen = set()
    for (t, t_next), flags, ct, utt0 in [((99, 98), 0, 0.0, 0), ((99, 0), 0, 0.0, 0), ((60, 40), 0, 0.0, 5), ((60, 40), 1, 0.0, 0), ((30, 12), 0, 2.0, 3),
                                         ((1, 0), 1, 0.0, 0)]:
        out, cand, score = st(l.half(), x, fm, t, t_next, seed=11, known=known, flags=flags, ct=ct, utt0=utt0)
        want = R.step(xn, fn, kn, cand, score, st.mask_id, st.keep_frac(t_next))
        assert np.array_equal(out, want), f"t={t}->{t_next}: {np.sum(out != want)} ids differ from the host selection"
        changed = out != xn
        assert not changed[~masked].any(), "unselected, known and padded rows equal x_t"
        assert (out[changed] != st.mask_id).all() and np.array_equal(out[changed], cand[changed])
        assert (cand[~masked] == -7).all() and (score[~masked] == 12345.0).all(), "rows that were not masked are left unwritten"
        assert np.isfinite(score[masked]).all() and (cand[masked] != st.mask_id).all()
        for b in range(x.shape[0]):
            _, n_rev = R.quota(int(free[b].sum()), int(masked[b].sum()), st.keep_frac(t_next))
            assert int(changed[b].sum()) == n_rev
            seen.add("all" if n_rev == masked[b].sum() and n_rev else "none" if n_rev == 0 else "some")
        out2, _, _ = st(l.half(), x, fm, t, t_next, seed=11, known=known, flags=flags, ct=ct, utt0=utt0, in_place=True)
        assert np.array_equal(out2, out), "in place"
    assert "all" in seen and (canvas < 64 or "none" in seen), seen      # (a handful of rows need not give a quota of 0)


def test_selection_quota_of_one_and_constant_logits(built_lib):
    """Crafted counts: with F = 70 free rows and keep = floor(70 cbar[50]), utterances that hold keep, keep + 1 and keep + 5 masked rows
    reveal 0, 1 and 5 of them.  Constant logits under greedy: every score ties, the lowest frame indices win."""
    K, canvas = 1025, 70
    st = Step(K, canvas)
    keep, _ = R.quota(70, 70, st.keep_frac(50))
    assert 6 <= keep <= 60
    g = torch.Generator().manual_seed(5)
    fm = torch.ones(3, canvas, dtype=torch.uint8)
    x = torch.randint(0, 500, (3, canvas), generator=g).to(torch.int32)
    pos = [torch.randperm(canvas, generator=g)[:keep + extra] for extra in (0, 1, 5)]
    for b in range(3):
        x[b, pos[b]] = st.mask_id
    l = torch.randn(3, canvas, K, generator=g) * 3
    out, cand, score = st(l.half(), x, fm, 70, 50, seed=3, shared=False)
    assert [(out[b] != x[b].numpy()).sum() for b in range(3)] == [0, 1, 5]
    assert np.array_equal(out, R.step(x.numpy(), fm.numpy(), None, cand, score, st.mask_id, st.keep_frac(50)))
    best = np.where(x[1].numpy() == st.mask_id, score[1], -np.inf).argmax()
    assert out[1, best] == cand[1, best] != st.mask_id, "a quota of one takes the most confident row"
    # constant logits, greedy, a shared mask [canvas]
    lc = torch.full((3, canvas, K), 0.75)
    out, cand, score = st(lc.half(), x, fm[0], 70, 50, seed=3, flags=1, shared=True)
    for b, extra in enumerate((0, 1, 5)):
        first = np.sort(pos[b].numpy())[:extra]
        assert np.array_equal(np.flatnonzero(out[b] != x[b].numpy()), first), "all scores tie: the lowest indices win"
        assert (out[b, first] == 0).all(), "greedy on constant logits: the first class"
    m = x.numpy() == st.mask_id
    assert len(np.unique(score[m])) == 1


# ---- 2. + 3. scores and candidates -----------------------------------------------------------------------------------------------
TRIPLES = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 1.0), (1.0, 1, 1.0)]


@pytest.mark.parametrize("K", [1025, 777])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_scores_and_candidates_against_the_float64_mirror(built_lib, dtype, K):
    """With top_k = 1 the candidate equals the host first-index argmax wherever the row's maximum is unique (rows whose maximum is
    tied keep every tied class, and the draw picks among them: the candidate then lies in that set)."""
    from vall_e.vall_e import _hip
    canvas, t, t_next, seed, utt0 = 70, 60, 40, 21, 2
    st = Step(K, canvas)
    l, x, fm, known, _ = _case(K, canvas, seed=K)
    logits = l.to(dtype)
    masked, _ = _masked(x.numpy(), fm.numpy(), known.numpy(), st.mask_id)
    rows = np.flatnonzero(masked.reshape(-1))
    u = _hip.uniform(seed, t, utt0 * canvas, 3 * canvas, K, 0, DEV).cpu().numpy()[rows]
    worst = 0.0
    for tau, k, p in TRIPLES:
        z3 = R.filtered_logits(logits.float().numpy().reshape(-1, K)[rows], st.mask_id, tau, k, p)
        ls = R.log_softmax64(z3)
        r = np.arange(len(rows))
        for greedy in (False, True):
            _, cand, score = st(logits, x, fm, t, t_next, seed, known=known, nucleus=(tau, k, p), flags=int(greedy), utt0=utt0)
            cand, score = cand.reshape(-1)[rows], score.reshape(-1)[rows]
            assert (cand != st.mask_id).all() and np.isfinite(z3[r, cand]).all(), "the candidate lies in the kept set, never the mask id"
            err = np.abs(score.astype(np.float64) - ls[r, cand]).max()
            worst = max(worst, err)
            assert err <= SCORE_TOL, (tau, k, p, greedy, err)
            best, second, gap = R.mirror_candidates(z3, None if greedy else u)
            if greedy:
                assert np.array_equal(cand, best), "greedy: the host first-index argmax, exactly"
                continue
            if k == 1:
                unique = (z3 == z3.max(-1, keepdims=True)).sum(-1) == 1
                assert np.array_equal(cand[unique], R.first_argmax(z3)[unique])
            off = cand != best
            assert (gap[off] < GAP).all() and np.array_equal(cand[off], second[off]), "a row may differ from the mirror only on a near tie"
            assert off.sum() <= 0.01 * len(rows), f"{off.sum()} of {len(rows)} rows excused"
    print(f"[reveal scores] K={K} {dtype}: max |score - log_softmax64(z''')[cand]| = {worst:.3e} (bound {SCORE_TOL:.1e})")


# ---- 7. choice_temperature -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1025, 777])
def test_choice_temperature_adds_the_keyed_gumbel(built_lib, K):
    from vall_e.vall_e import _hip
    canvas, seed, utt0, ct = 70, 33, 1, 4.5
    st = Step(K, canvas)
    l, x, fm, known, _ = _case(K, canvas, seed=K + 7)
    masked, _ = _masked(x.numpy(), fm.numpy(), known.numpy(), st.mask_id)
    rows = np.flatnonzero(masked.reshape(-1))
    ls = R.log_softmax64(R.filtered_logits(l.half().float().numpy().reshape(-1, K)[rows], st.mask_id))
    r = np.arange(len(rows))
    for t, t_next in ((60, 40), (99, 93), (7, 0)):
        v = _hip.uniform(seed, t, utt0 * canvas, 3 * canvas, 4, 4, DEV).cpu().numpy()[rows, 0]
        lam = np.float32(ct) * st.keep_frac(t_next)
        out, cand, score = st(l.half(), x, fm, t, t_next, seed, known=known, ct=ct, utt0=utt0)
        _, cand0, score0 = st(l.half(), x, fm, t, t_next, seed, known=known, ct=0.0, utt0=utt0)
        assert np.array_equal(cand, cand0), "the order noise does not move the candidates"
        want = ls[r, cand.reshape(-1)[rows]] + np.float64(lam) * R.gumbel64(v)
        err = np.abs(score.reshape(-1)[rows].astype(np.float64) - want).max()
        print(f"[reveal choice] K={K} t={t}->{t_next} lambda={lam:.4f}: max error {err:.3e}")
        assert err <= SCORE_TOL + float(lam) * 1e-5
        if t_next == 0:
            assert lam == 0 and np.array_equal(score, score0), "the last step: lambda = 0, score = conf bit for bit"
        else:
            assert not np.array_equal(score, score0)
        assert np.array_equal(out, R.step(x.numpy(), fm.numpy(), known.numpy(), cand, score, st.mask_id, st.keep_frac(t_next)))
    # greedy draws nothing: score = conf bit for bit whatever choice_temperature is
    _, _, sg = st(l.half(), x, fm, 60, 40, seed, known=known, ct=ct, flags=1)
    _, _, sg0 = st(l.half(), x, fm, 60, 40, seed, known=known, ct=0.0, flags=1)
    assert np.array_equal(sg, sg0)


# ---- 4. - 6. on models -----------------------------------------------------------------------------------------------------------
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


def _known(cfg):
    g = torch.Generator().manual_seed(9)
    return [torch.randint(0, 1024, (40,), generator=g), None, torch.randint(0, 1024, (5,), generator=g)]


@pytest.mark.parametrize("N", [1, 4, 16])
def test_masked_counts_follow_the_plan(native, N):
    m, cfg, texts, proms = native
    known = _known(cfg)
    out, trace = m.generate_audio(texts, proms, seed=5, n_frames=LENS, known=known, reveal_steps=N, return_trace=True)
    assert trace.shape == (N, 3, cfg.canvas) and torch.equal(trace[-1].long(), out)
    cbar = R.cbar_f32(m.sampler().schedule.cbar)
    x0, fm, kmap = m.canvas_init_known(3, LENS, known)
    tr = trace.cpu().numpy()
    for b in range(3):
        masked, free = _masked(x0[b].cpu().numpy(), fm[b].cpu().numpy(), kmap[b].cpu().numpy(), 512)
        F = int(free.sum())
        got = [int((tr[i, b][free] == 512).sum()) for i in range(N)]
        assert got == R.plan(F, int(masked.sum()), cbar, cfg.timesteps, N), (b, got)
        assert (tr[-1, b][free] != 512).all(), "at the end no free row holds the mask id"
        k = kmap[b].cpu().numpy() != 0
        for i in range(N):
            assert np.array_equal(tr[i, b][k], x0[b].cpu().numpy()[k]), "known ids come back unchanged"
            assert (tr[i, b][LENS[b]:] == 0).all(), "padded rows stay 0"


def _loop_vs_steps(m, cfg, texts, proms, lens, known, N, **kw):
    smp = m.sampler()
    B = len(texts)
    ct, cp = m.encode_conditions(texts, proms)
    kv_t, kv_p = smp.cond_kv(ct, cp)
    x, fm, kmap = m.canvas_init_known(B, lens, known)
    xs = x.clone()
    trace = smp.reveal_loop(x, fm, N, kv_t, kv_p, seed=77, trace=True, known=kmap, **kw)
    ts = smp.reveal_plan(N) + [0]
    assert ts == R.timesteps(cfg.timesteps, N)
    for i in range(N):
        lg, _ = smp.denoise_canvas(xs, fm, ts[i], kv_t, kv_p)
        nxt, _, _ = smp.reveal_step(lg, xs, fm, ts[i], ts[i + 1], seed=77, known=kmap, **kw)
        assert torch.equal(trace[i], nxt), f"step {i} (t={ts[i]}): the loop and the step entries disagree on {(trace[i] != nxt).sum().item()} ids"
        xs = nxt
    assert torch.equal(x, xs)
    return trace


def test_loop_equals_steps_native_fp16(native):
    m, cfg, texts, proms = native
    _loop_vs_steps(m, cfg, texts, proms, LENS, _known(cfg), 6)
    _loop_vs_steps(m, cfg, texts, proms, LENS, _known(cfg), 3, temperature=0.7, top_k=50, top_p=0.9, choice_temperature=4.5)


@pytest.mark.parametrize("with_known", [True, False], ids=["known", "none_known"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_loop_equals_steps_d512_bf16_fused_commit(built_lib, dtype, with_known):
    """The d = 512 16-bit configurations take the folded LayerNorms, so the loop's second launch is reveal_commit_prep_rows (commit +
    the next evaluation's embedding rows, moments and fc1 fold), in whichever moment format the plan picks: every instantiation of it
    under kRevise = false (dtype x known-frame map or none).  N = 3: two fused commits, x -> x_alt and x_alt -> x, then the unfused last."""
    from vall_e.vall_e import AR, synth
    cfg = synth.D3PMConfig.libritts()
    m = AR.from_config(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, 0))
    m = m.to(dtype).to(DEV)
    texts, proms = synth.make_inputs(cfg, 2, 1)
    g = torch.Generator().manual_seed(4)
    known = [torch.randint(0, 1024, (60,), generator=g), None] if with_known else [None, None]
    assert (m.canvas_init_known(2, [750, 333], known)[2] is None) == (not with_known)
    _loop_vs_steps(m, cfg, texts, proms, [750, 333], known, 3)


def test_utterances_are_independent_of_batch_shards_and_streams(native):
    m, cfg, texts, proms = native
    known = _known(cfg)
    kw = dict(seed=5, reveal_steps=4, choice_temperature=1.0)
    full = m.generate_audio(texts, proms, n_frames=LENS, known=known, **kw)
    for b in range(3):
        alone = m.generate_audio([texts[b]], [proms[b]], n_frames=[LENS[b]], known=[known[b]], utt0=b, global_batch=3, **kw)
        assert torch.equal(alone, full[b]), f"utterance {b} alone differs from the batch"
    shards = torch.cat([m.generate_audio(texts[:2], proms[:2], n_frames=LENS[:2], known=known[:2], utt0=0, global_batch=3, **kw),
                        m.generate_audio(texts[2:], proms[2:], n_frames=LENS[2:], known=known[2:], utt0=2, global_batch=3, **kw)[None]])
    assert torch.equal(shards, full)
    assert torch.equal(m.generate_audio(texts, proms, n_frames=LENS, known=known, streams=2, **kw), full)


def test_reveal_steps_none_is_the_loop_it_was(native):
    m, cfg, texts, proms = native
    smp = m.sampler()
    out = m.generate_audio(texts, proms, seed=5, steps=6, reveal_steps=None)
    ct, cp = m.encode_conditions(texts, proms)
    kv_t, kv_p = smp.cond_kv(ct, cp)
    x, fm = m.canvas_init(3)
    smp.sample_loop(x, fm, 6, 0, kv_t, kv_p, 5)
    assert torch.equal(out, x.long())

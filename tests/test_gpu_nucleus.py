"""The nucleus (top-p) cut on the x0-logits inside the sampler launch (include/d3pm_hip.h: d3pm_nucleus).

The ids carry no tolerance: a call equals the UNFILTERED entry fed with host logits -- temperature and top-k applied on the host,
then cut at the threshold theta the device reports (theta_out of the step entry) -- id for id.  theta itself is checked from the host
logits alone, in float64: it is one of the row's values, the softmax mass of {z'' >= theta} is >= top_p - EPS and the mass of
{z'' > theta} is < top_p + EPS, EPS = 1.0e-3 (n_classes / 2^20 + 2^-20 at 1025 classes: truncation of less than one unit of 2^-20
per class, Q >= 2^20, expf to a few ulp).  The rest are exact anchors that need no theta_out, and compositions:
  1. + 2. single step: every logits dtype, the K = 1025 routine and the general one, every kind of row, n_q = 8, known frames;
  3. top_p = 2^-11 == top_k = 1; crafted two-level rows == the predicted kept set; {tau, k, 1} == the _sampling entry; the neutral
     triple == the plain loop;
  4. the fused loop == denoise -> host cut at the step entry's theta -> unfiltered posterior_sample, step by step (16-bit and fp8,
     ragged, known frames); an utterance of a batch == that utterance alone; shards and stream chunks == the unsplit batch; the
     early-out routine == the general routine on rows whose kept token was cut;
  5. with top_p = 0.9 every id a masked row reveals lies in that row's kept set.
python -m pytest tests/test_gpu_nucleus.py -m gpu"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import nucleus_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEG_INF = float("-inf")
EPS = 1.0e-3


def host_filter(l, tau, k):
    """d3pm_sampling on the host -> float32 numpy array of the fp16 values z''."""
    return R.host_filter(l.detach().float().cpu().numpy(), tau, k)


def host_cut(l, tau, k, theta):
    """z''' as a tensor the unfiltered entry takes: z'' cut at the DEVICE's theta (NaN = a known row: never read)."""
    return torch.from_numpy(R.cut_at(host_filter(l, tau, k), theta.detach().float().cpu().numpy()))


def check_theta(z2, theta, p, skip=None):
    """Test 2, from the host logits alone: theta is a value of its row, and the float64 softmax mass it keeps brackets top_p."""
    z2 = z2.reshape(-1, z2.shape[-1])
    th = theta.detach().float().cpu().numpy().reshape(-1)
    rows = np.ones(len(th), bool) if skip is None else ~skip.reshape(-1)
    assert np.isfinite(th[rows]).all()
    assert (z2[rows] == th[rows, None]).any(-1).all(), "theta is one of the row's z'' values"
    sm = torch.softmax(torch.from_numpy(z2[rows]).double(), -1).numpy()
    ge = np.where(z2[rows] >= th[rows, None], sm, 0.0).sum(-1)
    gt = np.where(z2[rows] > th[rows, None], sm, 0.0).sum(-1)
    print(f"[theta] top_p={p}: kept mass {ge.min():.6f} .. {ge.max():.6f}, mass above theta up to {gt.max():.6f}, "
          f"kept classes {int((z2[rows] >= th[rows, None]).sum(-1).min())} .. {int((z2[rows] >= th[rows, None]).sum(-1).max())}")
    assert (ge >= p - EPS).all(), f"kept mass {ge.min()} < top_p - eps"
    assert (gt < p + EPS).all(), f"mass above theta {gt.max()} >= top_p + eps: a smaller set would have done"


# ---- the step entries through ctypes, for any class count ----------------------------------------------------------------------
class Step:
    """d3pm_posterior_sample_nucleus / _sampling / _known on a bare shape (no weights): K and n_q are free."""

    def __init__(self, K=1025, canvas=448, n_q=1, mask_id=None):
        from vall_e.vall_e import _hip, synth
        self.hip = _hip
        cfg = synth.D3PMConfig.native()
        self.shape = _hip.make_shape(cfg, torch.float16)
        self.shape.n_classes, self.shape.mask_id, self.shape.canvas, self.shape.n_q = K, (K // 2 if mask_id is None else mask_id), canvas, n_q
        self.K, self.canvas, self.n_q, self.mask_id = K, canvas, n_q, self.shape.mask_id
        self.sched = _hip.Schedule(100)

    def __call__(self, logits, x_t, t, seed, *, nucleus=None, sampling=None, entry="nucleus", known=None, flags=0, utt0=0, post=False,
                 theta=False):
        hip = self.hip
        logits = logits.to(DEV).contiguous()
        x_t = x_t.to(DEV).contiguous()
        B = x_t.shape[0]
        assert x_t.dtype == torch.int32 and logits.shape == tuple(x_t.shape) + (self.K,) and x_t.shape[1] == self.canvas
        x_next = torch.full_like(x_t, -7)
        po = torch.zeros(logits.shape, dtype=torch.int16, device=DEV) if post else None
        th = torch.full(x_t.shape, 12345.0, dtype=torch.float32, device=DEV) if theta else None
        pp = lambda v: None if v is None else C.c_void_p(v.data_ptr())
        head = (C.byref(self.shape), B, pp(logits), hip.dtype_code(logits.dtype), pp(x_t), pp(x_next), pp(known), int(t),
                C.byref(self.sched.c_struct), seed, utt0, flags, pp(po))
        if entry == "nucleus":
            nu = None if nucleus is None else hip.Nucleus(*nucleus)
            hip.check(hip.lib().d3pm_posterior_sample_nucleus(*head, None if nu is None else C.byref(nu), pp(th), hip.stream_ptr()), "nucleus")
        elif entry == "sampling":
            sm = None if sampling is None else hip.Sampling(*sampling)
            hip.check(hip.lib().d3pm_posterior_sample_sampling(*head, None if sm is None else C.byref(sm), hip.stream_ptr()), "sampling")
        else:
            assert nucleus is None and sampling is None and not theta
            hip.check(hip.lib().d3pm_posterior_sample_known(*head, hip.stream_ptr()), "known")
        torch.cuda.synchronize()
        return x_next.cpu(), (None if po is None else po.cpu()), (None if th is None else th.cpu())


def _rows(K, mask_id, rows, seed):
    """Logits of the tests' randn * 3 kind and x_t for every kind of row, cycling with the row index:
       0 masked | 1 revealed, logits peaked on the kept token (the early-out fires) | 2 revealed, the kept token among the lowest
       logits (the nucleus cuts it) | 3 revealed, logits peaked on ANOTHER class (the kept token loses) | 4 revealed, plain logits |
       5 masked, constant logits (all tie at theta: all kept) | 6 masked, signed zeros and -inf classes | 7 masked, sharply peaked."""
    g = torch.Generator().manual_seed(seed)
    l = torch.randn(rows, K, generator=g) * 3
    x = torch.randint(0, min(K, 1024), (rows,), generator=g)
    x = torch.where(x == mask_id, x + 1, x)
    r = torch.arange(rows)
    kind = r % 8
    other = (x + 17) % min(K, 1024)
    other = torch.where(other == mask_id, other + 1, other)
    l[r[kind == 1], x[kind == 1]] += 14.0
    l[r[kind == 2], x[kind == 2]] = -11.0
    l[r[kind == 3], other[kind == 3]] += 12.0
    l[kind == 5] = 0.75
    z = l[kind == 6]
    z[:, 0::3] = 0.0; z[:, 1::3] = -0.0; z[:, 5::7] = NEG_INF
    l[kind == 6] = z
    l[kind == 7] *= 4.0
    masked = (kind == 0) | (kind >= 5)
    x = torch.where(masked, torch.full_like(x, mask_id), x)
    return l, x.to(torch.int32), kind


ALL = -1             # top_k = n_classes of the case: through the top-k selection, which then keeps every class
COMBOS = [(1.0, 0, 0.5), (1.0, 0, 0.9), (1.0, 0, 0.99), (0.7, 50, 0.9), (1.3, 0, 0.5), (0.5, ALL, 0.99), (1.3, 20, 0.99)]
TS = (99, 50, 1, 0)


# ---- 1. + 2. -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1025, 777])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_single_step_equals_the_unfiltered_entry_on_host_logits_cut_at_the_devices_theta(built_lib, dtype, K):
    """K = 1025 takes sample_row_1025 (and the general routine when the posterior is asked for), K = 777 the general routine."""
    st = Step(K)
    B, T = 2, st.canvas
    l32, x, kind = _rows(K, st.mask_id, B * T, seed=K + 1)
    logits = l32.to(dtype).reshape(B, T, K)
    x = x.reshape(B, T)
    revealed = (x != st.mask_id).reshape(-1)
    n_cut_kept = n_lost = n_early = 0
    for tau, k, p in COMBOS:
        k = K if k == ALL else k
        z2 = host_filter(logits, tau, k)
        theta0 = None
        for t, greedy in itertools.product(TS, (0, 1)):
            seed = 1000 * t + 7
            got, _, th = st(logits, x, t, seed, nucleus=(tau, k, p), flags=greedy, theta=True)
            if theta0 is None:
                theta0 = th
                check_theta(z2, th, p)
                z3 = torch.from_numpy(R.cut_at(z2, th.numpy()))
                kept = torch.isfinite(z3.reshape(-1, K)).sum(-1)
                assert int(kept[kind == 5].min()) == K, "the constant rows keep everything: all tie at theta"
                cut = ~torch.isfinite(z3.reshape(-1, K)[torch.arange(B * T), x.reshape(-1).long()])
                if p <= 0.9:
                    assert int((cut & revealed & (kind == 2)).sum()) == int((kind == 2).sum()), "kind-2 rows: the kept token is cut"
            assert torch.equal(th, theta0), "theta depends on the logits and the three numbers only"
            ref, _, _ = st(z3, x, t, seed, entry="known", flags=greedy)
            assert torch.equal(got, ref), f"tau={tau} k={k} p={p} t={t} greedy={greedy}: {(got != ref).sum().item()} ids differ; kinds {kind[(got != ref).reshape(-1)].unique().tolist()}"
            plain, _, _ = st(logits, x, t, seed, nucleus=(tau, k, p), flags=greedy)
            assert torch.equal(plain, got), "the ids do not depend on theta_out"
            if p == 0.9 and k == 0 and t and not greedy:
                moved = (got.reshape(-1) != x.reshape(-1)) & revealed
                n_cut_kept += int((moved & (kind == 2)).sum())
                n_lost += int((moved & (kind == 3)).sum())
                n_early += int((~moved & (kind == 1)).sum())
        # the general routine at this K with the posterior written: bit patterns too; and the routine with the early-out against it
        got, gp, th = st(logits, x, 50, 77, nucleus=(tau, k, p), post=True, theta=True)
        ref, rp, _ = st(z3, x, 50, 77, entry="known", post=True)
        assert torch.equal(th, theta0), "the general routine finds the same theta"
        assert torch.equal(got, ref) and torch.equal(gp, rp), f"tau={tau} k={k} p={p}: posterior bit patterns differ"
        assert torch.isfinite(gp.view(torch.float16).float()).all(), "a class that was cut carries log(eps), not -inf or NaN"
        fast, _, _ = st(logits, x, 50, 77, nucleus=(tau, k, p))
        assert torch.equal(fast, got), "early-out / predicate-free routine vs the general routine under the nucleus"
    assert n_early > 100 and n_lost > 0, (n_early, n_lost)
    assert n_cut_kept > 0, "rows whose kept token was cut AND lost the race must occur"


def _step_nq(st, logits, x_t, t, seed, **kw):
    """Step.__call__ for grids with a level axis: [B, canvas, n_q] ids, [B, canvas, n_q, K] logits."""
    B, T, Q = x_t.shape
    flat = Step(st.K, canvas=T * Q)
    flat.shape = st.shape                          # the real shape (canvas T, n_q Q): the helper only checks tensor extents
    nxt, po, th = Step.__call__(flat, logits.reshape(B, T * Q, st.K), x_t.reshape(B, T * Q), t, seed, **kw)
    return nxt.reshape(B, T, Q), po, (None if th is None else th.reshape(B, T, Q))


def test_single_step_with_a_known_map_and_with_eight_levels(built_lib):
    g = torch.Generator().manual_seed(3)
    st = Step(1025)
    B, T, K = 3, st.canvas, 1025
    l32, x, kind = _rows(K, st.mask_id, B * T, seed=5)
    logits, x = l32.half().reshape(B, T, K), x.reshape(B, T)
    known = (torch.rand(B, T, generator=g) < 0.3).to(torch.uint8).to(DEV)
    kn = known.cpu().bool()
    for (tau, k, p), t in itertools.product(((0.5, 50, 0.9), (1.0, 0, 0.5), (1.3, 1025, 0.99)), (99, 1, 0)):
        got, _, th = st(logits, x, t, 11, nucleus=(tau, k, p), known=known, utt0=4, theta=True)
        assert torch.isnan(th[kn]).all() and torch.isfinite(th[~kn]).all(), "a known row writes NaN, every other row its theta"
        check_theta(host_filter(logits, tau, k), th, p, skip=kn.numpy())
        ref, _, _ = st(host_cut(logits, tau, k, th), x, t, 11, entry="known", known=known, utt0=4)
        free, _, thf = st(logits, x, t, 11, nucleus=(tau, k, p), utt0=4, theta=True)
        assert torch.equal(got, ref) and torch.equal(got, torch.where(kn, x, free)), (tau, k, p, t)
        assert torch.equal(thf[~kn], th[~kn])
    # n_q = 8: each level's 1025 logits are cut on their own (row = frame * 8 + level)
    st8 = Step(1025, canvas=64, n_q=8)
    B, T = 2, 64
    l32, x, kind = _rows(K, st8.mask_id, B * T * 8, seed=6)
    logits, x = l32.to(torch.bfloat16).reshape(B, T, 8, K), x.reshape(B, T, 8)
    known = (torch.rand(B, T, generator=g) < 0.25).to(torch.uint8).to(DEV)
    kn = known.cpu().bool()
    for (tau, k, p), t, greedy in itertools.product(((0.5, 50, 0.9), (1.0, 0, 0.5), (1.3, 0, 0.99)), (99, 50, 0), (0, 1)):
        got, _, th = _step_nq(st8, logits, x, t, 21, nucleus=(tau, k, p), flags=greedy, known=known, theta=True)
        assert torch.isnan(th[kn]).all() and torch.isfinite(th[~kn]).all()
        check_theta(host_filter(logits, tau, k), th, p, skip=kn[..., None].expand(B, T, 8).numpy())
        ref, _, _ = _step_nq(st8, host_cut(logits, tau, k, th), x, t, 21, entry="known", flags=greedy, known=known)
        assert torch.equal(got, ref), (tau, k, p, t, greedy)
        assert torch.equal(got[kn], x[kn])


# ---- 3. exact anchors without theta_out --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1025, 777])
def test_exact_anchors_on_the_step_entry(built_lib, K):
    st = Step(K)
    B, T = 2, st.canvas
    l32, x, kind = _rows(K, st.mask_id, B * T, seed=31)
    x = x.reshape(B, T)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        logits = l32.to(dtype).reshape(B, T, K)
        for t, greedy, tau in itertools.product((99, 50, 0), (0, 1), (1.0, 0.7)):
            seed = 3 * t + 1
            # top_p <= 1/1280 keeps exactly the classes tied at the maximum: the ids of top_k = 1
            a, _, _ = st(logits, x, t, seed, nucleus=(tau, 0, 2.0 ** -11), flags=greedy)
            b, _, _ = st(logits, x, t, seed, sampling=(tau, 1), entry="sampling", flags=greedy)
            assert torch.equal(a, b), f"top_p = 2^-11 vs top_k = 1: t={t} greedy={greedy} tau={tau}"
            # {tau, k, 1} is d3pm_sampling{tau, k}; NULL and the neutral triple are the plain entry
            a, _, _ = st(logits, x, t, seed, nucleus=(tau, 50, 1.0), flags=greedy)
            b, _, _ = st(logits, x, t, seed, sampling=(tau, 50), entry="sampling", flags=greedy)
            assert torch.equal(a, b), "{tau, k, 1}"
            a, _, th = st(logits, x, t, seed, nucleus=(tau, 50, 1.0), flags=greedy, theta=True)
            assert torch.equal(a, b) and bool((th == NEG_INF).all()), "top_p = 1 with a theta output: the same ids, theta = -inf"
        plain, _, _ = st(logits, x, 50, 5, entry="known")
        for nu in (None, (1.0, 0, 1.0)):
            a, _, _ = st(logits, x, 50, 5, nucleus=nu)
            assert torch.equal(a, plain), "the neutral triple"
    # crafted two-level rows: the kept set is predicted on the host without any exp's last bit (tests/nucleus_ref.py)
    cases = R.two_level_cases(K)
    for top_p in sorted({c[1] for c in cases}):
        mine = [c for c in cases if c[1] == top_p]
        rows = np.stack([mine[i % len(mine)][0] for i in range(T)])[None]
        want = np.full_like(rows, NEG_INF)
        for i in range(T):
            keep = mine[i % len(mine)][2]
            want[0, i, keep] = rows[0, i, keep]
        xm = torch.full((1, T), st.mask_id, dtype=torch.int32)
        for i in range(1, T, 2):                  # every second row revealed, on a class the nucleus keeps
            ok = [j for j in mine[i % len(mine)][2] if j != st.mask_id and j < 1024]
            xm[0, i] = int(ok[0]) if ok else st.mask_id
        for t, greedy in itertools.product((99, 50, 1, 0), (0, 1)):
            got, _, th = st(torch.from_numpy(rows), xm, t, 9 + t, nucleus=(1.0, 0, top_p), flags=greedy, theta=True)
            ref, _, _ = st(torch.from_numpy(want), xm, t, 9 + t, entry="known", flags=greedy)
            assert torch.equal(got, ref), f"two-level rows, top_p={top_p} t={t} greedy={greedy}"
            assert np.array_equal(th[0].numpy(), np.array([mine[i % len(mine)][3] for i in range(T)], dtype=np.float32))


# ---- models ---------------------------------------------------------------------------------------------------------------------
def _model(cfg, dtype, seed=0):
    from vall_e.vall_e import AR, synth
    m = AR.from_config(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, seed))
    return m.to(dtype).to(DEV)


@pytest.fixture(scope="module")
def native():
    from vall_e.vall_e import synth
    cfg = synth.D3PMConfig.native()
    texts, proms = synth.make_inputs(cfg, 8, 1)
    return cfg, texts, proms, _model(cfg, torch.float16)


@pytest.fixture(scope="module")
def libri():
    from vall_e.vall_e import synth
    cfg = synth.D3PMConfig.libritts()
    texts, proms = synth.make_inputs(cfg, 32, 1)
    return cfg, texts, proms, _model(cfg, torch.bfloat16)


def _kv(m, texts, proms):
    smp = m.sampler()
    ct, cp = m.encode_conditions(texts, proms)
    return (smp,) + tuple(smp.cond_kv(ct, cp))


def test_neutral_triple_is_the_plain_loop_and_top_p_changes_what_is_drawn(native):
    from vall_e.vall_e import _hip
    cfg, texts, proms, m = native
    B = 2
    smp, kv_t, kv_p = _kv(m, texts[:B], proms[:B])
    x0, fm = m.canvas_init(B)
    ws = smp.workspace(B)

    def loop(nucleus, canvas=False, entry="d3pm_sample_loop_nucleus", struct=None):
        x = x0.clone()
        cv = smp._check_canvas(B, fm) if canvas else None
        nu = None if nucleus is None else (struct or _hip.Nucleus)(*nucleus)
        _hip.check(getattr(_hip.lib(), entry)(
            C.byref(smp.shape), C.byref(smp.weights.c_struct), None, B, x.data_ptr(), None if canvas else fm.data_ptr(),
            None if cv is None else C.byref(cv), 99, 0, smp.film.data_ptr(), kv_t.data_ptr(), kv_p.data_ptr(), C.byref(smp.schedule.c_struct),
            45, 0, 0, ws.data_ptr(), ws.numel(), None, None if nu is None else C.byref(nu), _hip.stream_ptr()), entry)
        return x

    ref = x0.clone()
    smp.sample_loop(ref, fm, 99, 0, kv_t, kv_p, 45)                      # d3pm_sample_loop
    assert torch.equal(loop(None), ref), "NULL"
    assert torch.equal(loop((1.0, 0, 1.0)), ref), "{1, 0, 1}"
    assert torch.equal(loop(None, canvas=True), ref) and torch.equal(loop((1.0, 0, 1.0), canvas=True), ref), "the canvas form"
    filt = loop((0.7, 50), entry="d3pm_sample_loop_sampling", struct=_hip.Sampling)
    assert torch.equal(loop((0.7, 50, 1.0)), filt), "{tau, k, 1} is d3pm_sampling{tau, k}"
    assert torch.equal(loop((1.0, 0, 2.0 ** -11)), loop((1.0, 1), entry="d3pm_sample_loop_sampling", struct=_hip.Sampling)), "2^-11 vs top_k = 1"
    kw = dict(steps=99, seed=45)
    pub = m.generate_audio(texts[:B], proms[:B], **kw)
    assert torch.equal(pub, ref.long())
    assert torch.equal(m.generate_audio(texts[:B], proms[:B], top_p=1.0, **kw), pub)
    assert torch.equal(m.generate_audio(texts[:B], proms[:B], top_p=2.0 ** -11, **kw), m.generate_audio(texts[:B], proms[:B], top_k=1, **kw))
    assert not torch.equal(m.generate_audio(texts[:B], proms[:B], top_p=0.9, **kw), pub), "top_p = 0.9 must change what is drawn"
    with pytest.raises(ValueError):
        m.generate_audio(texts[:1], proms[:1], steps=2, seed=1, graph=True, top_p=0.9)


# ---- 4. composition ----------------------------------------------------------------------------------------------------------------
def _loop_vs_steps(m, texts, proms, t_start, seed, tau, k, p, *, n_frames=None, known=None, kmask=None, fp8=False):
    B = len(texts)
    smp, kv_t, kv_p = _kv(m, texts, proms)
    per_utt = known is not None or not (n_frames is None or isinstance(n_frames, int))
    out, trace = m.generate_audio(texts, proms, steps=t_start, seed=seed, n_frames=n_frames, known=known, known_mask=kmask, fp8=fp8,
                                  temperature=tau, top_k=k, top_p=p, return_trace=True)
    if per_utt:
        xs, fm, km = m.canvas_init_known(B, n_frames, known, kmask)
    else:
        (xs, fm), km = m.canvas_init(B, n_frames), None
    free = np.ones((B, xs.shape[1]), bool) if km is None else ~km.cpu().bool().numpy()
    for i, t in enumerate(range(t_start, 0, -1)):
        if per_utt:
            lg, _ = smp.denoise_canvas(xs, fm, t, kv_t, kv_p)
        else:
            lg, _ = smp.denoise(xs, fm, t, kv_t, kv_p, fp8=fp8)
        dev, _, th = smp.posterior_sample(lg, xs, t, seed, known=km, temperature=tau, top_k=k, top_p=p, want_theta=True)
        if i % 16 == 0:
            check_theta(host_filter(lg, tau, k), th, p, skip=~free)
        nxt, _ = smp.posterior_sample(host_cut(lg, tau, k, th).to(DEV), xs, t, seed, known=km)      # the UNFILTERED kernel
        assert torch.equal(dev, nxt), f"t = {t}: the step entry differs from the unfiltered kernel on host-cut logits"
        assert torch.equal(trace[i], nxt), f"t = {t}: {(trace[i] != nxt).sum().item()} ids of the fused loop differ from the step-by-step composition"
        xs = nxt
    assert torch.equal(out.reshape(xs.shape), xs.long())
    return out


@pytest.mark.parametrize("tau,k,p", [(1.0, 0, 0.9), (0.7, 50, 0.5), (1.3, 0, 0.99)])
def test_loop_native_shape_whole_loop(native, tau, k, p):
    cfg, texts, proms, m = native
    _loop_vs_steps(m, texts[:2], proms[:2], 99, 3, tau, k, p)


def test_loop_native_shape_ragged_with_known_frames(native):
    cfg, texts, proms, m = native
    lens = [350, 131, cfg.canvas, 37]
    g = torch.Generator().manual_seed(2)
    known = [torch.randint(0, 1024, (L,), generator=g) for L in lens]
    kmask = [None, torch.rand(131, generator=g) < 0.4, torch.arange(cfg.canvas) % 3 == 0, None]
    known[0], known[3] = known[0][:100], None
    _loop_vs_steps(m, texts[:4], proms[:4], 99, 8, 0.7, 50, 0.9, n_frames=lens, known=known, kmask=kmask)


@pytest.mark.parametrize("fp8", [False, True])
def test_loop_d512_thirty_two_utterances(libri, fp8):
    """The launch the loop really runs at this shape: the sampler + the next iteration's embedding rows, quad moments and fc1 fold."""
    cfg, texts, proms, m = libri
    _loop_vs_steps(m, texts, proms, 3, 17, 1.0, 0, 0.9, fp8=fp8)


def test_loop_d512_ragged_with_known_frames(libri):
    cfg, texts, proms, m = libri
    lens = [1, cfg.canvas, 37, 333]
    g = torch.Generator().manual_seed(4)
    known = [None, torch.randint(0, 1024, (200,), generator=g), torch.randint(0, 1024, (37,), generator=g), None]
    kmask = [None, None, torch.rand(37, generator=g) < 0.5, None]
    _loop_vs_steps(m, texts[:4], proms[:4], 4, 19, 1.3, 20, 0.9, n_frames=lens, known=known, kmask=kmask)


def test_batch_equals_each_utterance_alone_and_any_split(libri):
    cfg, texts, proms, m = libri
    B, kw = 12, dict(steps=4, seed=5, temperature=0.7, top_p=0.9)
    lens = [min(37 + 61 * b, cfg.canvas) for b in range(B)]
    whole = m.generate_audio(texts[:B], proms[:B], n_frames=lens, **kw)
    for b in (0, 5, 11):
        alone = m.generate_audio(texts[b:b + 1], proms[b:b + 1], n_frames=lens[b], utt0=b, global_batch=B, **kw)
        assert torch.equal(whole[b], alone), f"utterance {b}: {(whole[b] != alone).sum().item()} ids differ from the utterance alone"
    chunked = m.generate_audio(texts[:B], proms[:B], n_frames=lens, streams=2, **kw)
    assert torch.equal(chunked, whole), "stream chunks"
    lo, hi = 5, 9
    shard = m.generate_audio(texts[lo:hi], proms[lo:hi], n_frames=lens[lo:hi], utt0=lo, global_batch=B, **kw)
    assert torch.equal(shard, whole[lo:hi]), "a shard (utt0, global_batch)"
    assert not torch.equal(whole, m.generate_audio(texts[:B], proms[:B], n_frames=lens, steps=4, seed=5, temperature=0.7))


# ---- 5. the property a reader can check without the arithmetic ------------------------------------------------------------------------
def test_with_top_p_09_every_revealed_id_lies_in_the_rows_kept_set(built_lib):
    """A property of THESE inputs, not of the contract: a class that was cut keeps the weight eps in the reference arithmetic, so now
    and then a cut class wins a revealing draw, as the reference says it should.  The inputs are therefore rows on which the CPU
    oracle itself (Oracle arithmetic on the host logits cut at theta, same Philox uniforms) reveals only kept ids -- asserted first,
    on the CPU -- and the kernel must then do the same.  The kept set is {z'' >= theta} with the device's theta, which test 2 pins."""
    from oracle import d3pm_oracle as O
    from oracle import philox
    T, K = 64, 1025
    st = Step(K, canvas=T)
    tabs = O.scalar_tables(O.cosine_betas(100), 100)
    g = torch.Generator().manual_seed(12)
    logits = (torch.randn(1, T, K, generator=g) * 3).half()
    x = torch.full((1, T), st.mask_id, dtype=torch.int32)
    n_revealed = 0
    for tau, t in itertools.product((0.5, 1.0, 1.3), (99, 50, 10, 1)):
        seed = 5 + t
        got, _, th = st(logits, x, t, seed, nucleus=(tau, 0, 0.9), theta=True)
        check_theta(host_filter(logits, tau, 0), th, 0.9)
        z3 = host_cut(logits, tau, 0, th)
        kept = torch.isfinite(z3)[0]
        post = O.posterior_logits_closed(z3[0].half(), x[0].long(), t, tabs)
        ref = O.gumbel_argmax(post, torch.from_numpy(philox.uniform_batch(seed, t, 0, 1, T)[0]), t)
        ref_rev = ref != st.mask_id
        assert bool(kept[torch.arange(T), ref][ref_rev].all()), "precondition: the CPU oracle reveals only kept ids on these inputs"
        got = got[0].long()
        rev = got != st.mask_id
        n_revealed += int(rev.sum())
        assert bool(kept[torch.arange(T), got][rev].all()), f"tau={tau} t={t}: a masked row revealed an id outside its nucleus"
    assert n_revealed > 100

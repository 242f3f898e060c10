"""Temperature and top-k on the x0-logits inside the sampler launch (include/d3pm_hip.h: d3pm_sampling).

The contract has no tolerance in it: a filtered draw equals the UNFILTERED entry fed with logits that were filtered on the host,

    z' = rn16(rn16(l) / temperature);   theta = the top_k-th largest z' (with multiplicity);   z'' = z' >= theta ? z' : -inf,

so everything here is equality of int32 ids (and of fp16 posterior bit patterns where they are asked for):
  1. single step: every logits dtype, the predicate-free K = 1025 routine and the general one, every kind of row;
  2. neutral values == the existing entries over a whole loop, {1, K} (through the filter arm) == the same ids;
  3. the fused loop == denoise -> host filter -> unfiltered posterior_sample, step by step (16-bit and fp8, ragged, known frames);
  4. an utterance of a filtered batch == that utterance alone; shards and stream chunks == the unsplit batch;
  5. the CPU oracle on host-filtered logits, by the near-tie criterion of test_gpu_parity.py;
  6. with top_k = 50 every id a masked row reveals lies in that row's kept set.
python -m pytest tests/test_gpu_sampling_filter.py -m gpu"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEG_INF = float("-inf")


def host_filter(l, tau, k):
    """The definition, in torch on the CPU -> fp32 tensor that holds the fp16 values z'' (the step entries take logits_dtype, so
    this goes to the unfiltered kernel whatever the model dtype).  The division is an fp32 tensor / fp32 tensor one on the CPU: a
    true IEEE division, like the kernel's."""
    z = l.detach().cpu().half().float()
    z = (z / torch.tensor(tau, dtype=torch.float32)).half().float()
    if k > 0:
        theta = torch.topk(z, k, dim=-1).values[..., -1:]
        z = torch.where(z >= theta, z, torch.full_like(z, NEG_INF))
    return z


def test_host_filter_is_the_definition_in_numpy_too():
    """The torch lines above against the same five lines in numpy, ties at theta and signed zeros included."""
    g = torch.Generator().manual_seed(0)
    l = (torch.randn(64, 1025, generator=g) * 3).half()
    l[0] = 1.5; l[1, ::2] = 0.0; l[1, 1::2] = -0.0; l[2, 5:900] = NEG_INF
    for tau, k in itertools.product((0.5, 0.7, 1.0, 1.3), (0, 1, 50, 1025)):
        z = (l.numpy().astype(np.float32) / np.float32(tau)).astype(np.float16).astype(np.float32)
        if k:
            theta = np.sort(z, axis=-1)[:, ::-1][:, k - 1:k]
            z = np.where(z >= theta, z, -np.inf).astype(np.float32)
        got = host_filter(l, tau, k).numpy()
        assert np.array_equal(got, z), (tau, k)
        if k == 50:
            kept = np.isfinite(got[3:]).sum(-1)
            assert kept.min() >= 50 and kept.max() <= 53


# ---- the step entries through ctypes, for any class count ----------------------------------------------------------------------
class Step:
    """d3pm_posterior_sample_sampling / d3pm_posterior_sample_known on a bare shape (no weights): K and n_q are free."""

    def __init__(self, K=1025, canvas=448, n_q=1, mask_id=None):
        from vall_e.vall_e import _hip, synth
        self.hip = _hip
        cfg = synth.D3PMConfig.native()
        self.shape = _hip.make_shape(cfg, torch.float16)
        self.shape.n_classes, self.shape.mask_id, self.shape.canvas, self.shape.n_q = K, (K // 2 if mask_id is None else mask_id), canvas, n_q
        self.K, self.canvas, self.n_q, self.mask_id = K, canvas, n_q, self.shape.mask_id
        self.sched = _hip.Schedule(100)

    def __call__(self, logits, x_t, t, seed, *, sampling=None, entry="sampling", known=None, flags=0, utt0=0, post=False):
        hip = self.hip
        logits = logits.to(DEV).contiguous()
        x_t = x_t.to(DEV).contiguous()
        B = x_t.shape[0]
        assert x_t.dtype == torch.int32 and logits.shape == tuple(x_t.shape) + (self.K,) and x_t.shape[1] == self.canvas
        x_next = torch.full_like(x_t, -7)
        po = torch.zeros(logits.shape, dtype=torch.int16, device=DEV) if post else None
        pp = lambda v: None if v is None else C.c_void_p(v.data_ptr())
        head = (C.byref(self.shape), B, pp(logits), hip.dtype_code(logits.dtype), pp(x_t), pp(x_next), pp(known), int(t),
                C.byref(self.sched.c_struct), seed, utt0, flags, pp(po))
        if entry == "sampling":
            sm = None if sampling is None else hip.Sampling(*sampling)
            hip.check(hip.lib().d3pm_posterior_sample_sampling(*head, None if sm is None else C.byref(sm), hip.stream_ptr()), "sampling")
        else:
            assert sampling is None
            hip.check(hip.lib().d3pm_posterior_sample_known(*head, hip.stream_ptr()), "known")
        torch.cuda.synchronize()
        return x_next.cpu(), (None if po is None else po.cpu())


def _rows(K, mask_id, rows, seed):
    """Logits of the tests' randn * 3 kind and x_t for every kind of row, cycling with the row index:
       0 masked | 1 revealed, logits peaked on the kept token (the early-out fires) | 2 revealed, the kept token among the lowest
       logits (top_k cuts it) | 3 revealed, logits peaked on ANOTHER class (the kept token loses) | 4 revealed, plain logits |
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


TAUS, TS = (0.5, 1.0, 1.3), (99, 50, 1, 0)


@pytest.mark.parametrize("K", [1025, 777])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_single_step_equals_the_unfiltered_entry_on_host_filtered_logits(built_lib, dtype, K):
    """K = 1025 takes sample_row_1025 (and the general routine when the posterior is asked for), K = 777 the general routine."""
    st = Step(K)
    B, T = 2, st.canvas
    l32, x, kind = _rows(K, st.mask_id, B * T, seed=K)
    logits = l32.to(dtype).reshape(B, T, K)
    x = x.reshape(B, T)
    revealed = (x != st.mask_id).reshape(-1)
    n_cut_kept = n_lost = n_early = 0
    for tau, k in itertools.product(TAUS, (0, 1, 50, K)):
        hf = host_filter(logits, tau, k)
        if k == 50:
            kept = torch.isfinite(hf.reshape(-1, K)).sum(-1)
            assert int(kept.min()) >= 50 and int(kept[kind == 5].min()) == K, "ties at theta are all kept; the constant rows keep everything"
            assert int((kept > 50).sum()) > 0, "the inputs must hold rows with exact ties at theta"
            cut = ~torch.isfinite(hf.reshape(-1, K)[torch.arange(B * T), x.reshape(-1).long()])
            assert int((cut & revealed & (kind == 2)).sum()) == int((kind == 2).sum()), "kind-2 rows: the kept token is filtered out"
        for t, greedy in itertools.product(TS, (0, 1)):
            seed = 1000 * t + 7
            got, _ = st(logits, x, t, seed, sampling=(tau, k), flags=greedy)
            ref, _ = st(hf, x, t, seed, entry="known", flags=greedy)
            assert torch.equal(got, ref), f"tau={tau} k={k} t={t} greedy={greedy}: {(got != ref).sum().item()} ids differ; kinds {kind[(got != ref).reshape(-1)].unique().tolist()}"
            if k == 50 and t and not greedy:
                moved = (got.reshape(-1) != x.reshape(-1)) & revealed
                n_cut_kept += int((moved & (kind == 2)).sum())
                n_lost += int((moved & (kind == 3)).sum())
                n_early += int((~moved & (kind == 1)).sum())
        # the general routine at this K with the posterior written: bit patterns too
        got, gp = st(logits, x, 50, 77, sampling=(tau, k), post=True)
        ref, rp = st(hf, x, 50, 77, entry="known", post=True)
        assert torch.equal(got, ref) and torch.equal(gp, rp), f"tau={tau} k={k}: posterior bit patterns differ"
        assert torch.isfinite(gp.view(torch.float16).float()).all(), "a filtered-out class carries log(eps), not -inf or NaN"
        fast, _ = st(logits, x, 50, 77, sampling=(tau, k))
        assert torch.equal(fast, got), "early-out / predicate-free routine vs the general routine under the filter"
    assert n_early > 300 and n_lost > 50, (n_early, n_lost)
    assert n_cut_kept > 0, "rows whose kept token was filtered out AND lost the race must occur"


def test_single_step_with_a_known_map_and_with_eight_levels(built_lib):
    g = torch.Generator().manual_seed(3)
    # known frames
    st = Step(1025)
    B, T, K = 3, st.canvas, 1025
    l32, x, kind = _rows(K, st.mask_id, B * T, seed=5)
    logits, x = l32.half().reshape(B, T, K), x.reshape(B, T)
    known = (torch.rand(B, T, generator=g) < 0.3).to(torch.uint8).to(DEV)
    for (tau, k), t in itertools.product(((0.5, 50), (1.3, 1), (1.0, 1025), (0.7, 0)), (99, 1, 0)):
        got, _ = st(logits, x, t, 11, sampling=(tau, k), known=known, utt0=4)
        ref, _ = st(host_filter(logits, tau, k), x, t, 11, entry="known", known=known, utt0=4)
        free, _ = st(logits, x, t, 11, sampling=(tau, k), utt0=4)
        assert torch.equal(got, ref) and torch.equal(got, torch.where(known.cpu().bool(), x, free)), (tau, k, t)
    # n_q = 8: each level's 1025 logits are filtered on their own (row = frame * 8 + level)
    st8 = Step(1025, canvas=64, n_q=8)
    B, T = 2, 64
    l32, x, kind = _rows(K, st8.mask_id, B * T * 8, seed=6)
    logits, x = l32.to(torch.bfloat16).reshape(B, T, 8, K), x.reshape(B, T, 8)
    kn = (torch.rand(B, T, generator=g) < 0.25).to(torch.uint8).to(DEV)
    for (tau, k), t, greedy in itertools.product(((0.5, 50), (1.3, 1), (1.0, 1025)), (99, 50, 0), (0, 1)):
        got, _ = _step_nq(st8, logits, x, t, 21, sampling=(tau, k), flags=greedy, known=kn)
        ref, _ = _step_nq(st8, host_filter(logits, tau, k), x, t, 21, entry="known", flags=greedy, known=kn)
        assert torch.equal(got, ref), (tau, k, t, greedy)
        assert torch.equal(got[kn.cpu().bool()], x[kn.cpu().bool()])


def _step_nq(st, logits, x_t, t, seed, **kw):
    """Step.__call__ for grids with a level axis: [B, canvas, n_q] ids, [B, canvas, n_q, K] logits."""
    B, T, Q = x_t.shape
    flat = Step(st.K, canvas=T * Q)
    flat.shape = st.shape                          # the real shape (canvas T, n_q Q): the helper only checks tensor extents
    known = kw.pop("known", None)
    nxt, po = Step.__call__(flat, logits.reshape(B, T * Q, st.K), x_t.reshape(B, T * Q), t, seed, known=known, **kw)
    return nxt.reshape(B, T, Q), po


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


# ---- 2. neutral values ------------------------------------------------------------------------------------------------------------
def test_neutral_values_are_the_existing_entries_over_a_whole_loop(native):
    from vall_e.vall_e import _hip
    cfg, texts, proms, m = native
    B = 2
    smp, kv_t, kv_p = _kv(m, texts[:B], proms[:B])
    x0, fm = m.canvas_init(B)
    ws = smp.workspace(B)

    def loop(sampling, canvas=False, x_init=x0):
        x = x_init.clone()
        cv = smp._check_canvas(B, fm) if canvas else None
        sm = None if sampling is None else _hip.Sampling(*sampling)
        _hip.check(_hip.lib().d3pm_sample_loop_sampling(
            C.byref(smp.shape), C.byref(smp.weights.c_struct), None, B, x.data_ptr(), None if canvas else fm.data_ptr(),
            None if cv is None else C.byref(cv), 99, 0, smp.film.data_ptr(), kv_t.data_ptr(), kv_p.data_ptr(), C.byref(smp.schedule.c_struct),
            45, 0, 0, ws.data_ptr(), ws.numel(), None, None if sm is None else C.byref(sm), _hip.stream_ptr()), "d3pm_sample_loop_sampling")
        return x

    ref = x0.clone()
    smp.sample_loop(ref, fm, 99, 0, kv_t, kv_p, 45)                      # d3pm_sample_loop
    assert torch.equal(loop(None), ref), "NULL options"
    assert torch.equal(loop((1.0, 0)), ref), "{1, 0}"
    assert torch.equal(loop(None, canvas=True), ref) and torch.equal(loop((1.0, 0), canvas=True), ref), "the canvas form"
    assert torch.equal(loop((1.0, 1025)), ref), "{1, K}: through the filter arm, every class kept"
    assert torch.equal(loop((1.0, 1025), canvas=True), ref)
    kw = dict(steps=99, seed=45)
    pub = m.generate_audio(texts[:B], proms[:B], **kw)
    assert torch.equal(pub, ref.long())
    assert torch.equal(m.generate_audio(texts[:B], proms[:B], temperature=1.0, top_k=0, **kw), pub)
    assert torch.equal(m.generate_audio(texts[:B], proms[:B], top_k=1025, **kw), pub)
    assert not torch.equal(m.generate_audio(texts[:B], proms[:B], top_k=50, **kw), pub), "top_k = 50 must change what is drawn"
    assert not torch.equal(m.generate_audio(texts[:B], proms[:B], temperature=0.7, **kw), pub)
    # the step entry: NULL and {1, 0} == d3pm_posterior_sample, {1, K} the same ids
    lg, _ = smp.denoise(x0, fm, 60, kv_t, kv_p)
    a, _ = smp.posterior_sample(lg, x0, 60, 9)
    b, _ = smp.posterior_sample(lg, x0, 60, 9, temperature=1.0, top_k=0)
    c, _ = smp.posterior_sample(lg, x0, 60, 9, top_k=1025)
    assert torch.equal(a, b) and torch.equal(a, c)


# ---- 3. the fused loop ------------------------------------------------------------------------------------------------------------
def _loop_vs_steps(m, texts, proms, t_start, seed, tau, k, *, n_frames=None, known=None, kmask=None, fp8=False):
    B = len(texts)
    smp, kv_t, kv_p = _kv(m, texts, proms)
    per_utt = known is not None or not (n_frames is None or isinstance(n_frames, int))
    out, trace = m.generate_audio(texts, proms, steps=t_start, seed=seed, n_frames=n_frames, known=known, known_mask=kmask, fp8=fp8,
                                  temperature=tau, top_k=k, return_trace=True)
    if per_utt:
        xs, fm, km = m.canvas_init_known(B, n_frames, known, kmask)
    else:
        (xs, fm), km = m.canvas_init(B, n_frames), None
    for i, t in enumerate(range(t_start, 0, -1)):
        if per_utt:
            lg, _ = smp.denoise_canvas(xs, fm, t, kv_t, kv_p)
        else:
            lg, _ = smp.denoise(xs, fm, t, kv_t, kv_p, fp8=fp8)
        nxt, _ = smp.posterior_sample(host_filter(lg, tau, k).to(DEV), xs, t, seed, known=km)      # the UNFILTERED kernel
        assert torch.equal(trace[i], nxt), f"t = {t}: {(trace[i] != nxt).sum().item()} ids of the fused filtered loop differ from the step-by-step composition"
        xs = nxt
    assert torch.equal(out.reshape(xs.shape), xs.long())
    return out


@pytest.mark.parametrize("tau,k", [(0.7, 50), (1.3, 0), (1.0, 1), (0.5, 1025)])
def test_loop_native_shape_whole_loop(native, tau, k):
    cfg, texts, proms, m = native
    _loop_vs_steps(m, texts[:2], proms[:2], 99, 3, tau, k)


def test_loop_native_shape_ragged_with_known_frames(native):
    cfg, texts, proms, m = native
    lens = [350, 131, cfg.canvas, 37]
    g = torch.Generator().manual_seed(2)
    known = [torch.randint(0, 1024, (L,), generator=g) for L in lens]
    kmask = [None, torch.rand(131, generator=g) < 0.4, torch.arange(cfg.canvas) % 3 == 0, None]
    known[0], known[3] = known[0][:100], None
    _loop_vs_steps(m, texts[:4], proms[:4], 99, 8, 0.7, 50, n_frames=lens, known=known, kmask=kmask)


@pytest.mark.parametrize("fp8", [False, True])
def test_loop_d512_thirty_two_utterances(libri, fp8):
    """The launch the loop really runs at this shape: the sampler + the next iteration's embedding rows, quad moments and fc1 fold."""
    cfg, texts, proms, m = libri
    _loop_vs_steps(m, texts, proms, 3, 17, 0.7, 50, fp8=fp8)


def test_loop_d512_ragged_with_known_frames(libri):
    cfg, texts, proms, m = libri
    lens = [1, cfg.canvas, 37, 333]
    g = torch.Generator().manual_seed(4)
    known = [None, torch.randint(0, 1024, (200,), generator=g), torch.randint(0, 1024, (37,), generator=g), None]
    kmask = [None, None, torch.rand(37, generator=g) < 0.5, None]
    _loop_vs_steps(m, texts[:4], proms[:4], 4, 19, 1.3, 20, n_frames=lens, known=known, kmask=kmask)


# ---- 4. invariance ------------------------------------------------------------------------------------------------------------------
def test_filtered_batch_equals_each_utterance_alone_and_any_split(libri):
    cfg, texts, proms, m = libri
    B, kw = 12, dict(steps=4, seed=5, temperature=0.7, top_k=50)
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
    assert not torch.equal(whole, m.generate_audio(texts[:B], proms[:B], n_frames=lens, steps=4, seed=5))


def test_graph_replay_refuses_sampling_options(native):
    cfg, texts, proms, m = native
    with pytest.raises(ValueError):
        m.generate_audio(texts[:1], proms[:1], steps=2, seed=1, graph=True, top_k=50)


# ---- 5. the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau,k", [(0.7, 50), (1.3, 0), (0.5, 1)])
def test_oracle_on_host_filtered_logits_by_the_near_tie_criterion(native, tau, k):
    """Oracle.posterior + gumbel_argmax with the Philox uniforms on host-filtered logits against the kernel's filtered draw on the
    raw logits.  The criterion is test_gpu_parity.py's (_audit): an id may differ only where the oracle's own race between the two
    candidates was decided by less than 0.05 (~3 fp16 quanta of a posterior logit near -20); the only order-dependent quantity is
    still fact2 of the mask class.  No new tolerance."""
    from oracle import d3pm_oracle as O
    from oracle import philox
    from util import native_setup
    cfg, texts, proms, m = native
    smp, kv_t, kv_p = _kv(m, texts[:1], proms[:1])
    orc = native_setup(torch.float16)[4]
    x, fm = m.canvas_init(1)
    mism = audited = total = 0
    worst = 0.0
    for t in range(99, 0, -1):
        lg, _ = smp.denoise(x, fm, t, kv_t, kv_p)
        nxt, _ = smp.posterior_sample(lg, x, t, 123, temperature=tau, top_k=k)
        hf = host_filter(lg[0], tau, k)
        xc = x[0].cpu().long()
        post = orc.posterior(hf, xc, t)
        u = torch.from_numpy(philox.uniform_batch(123, t, 0, 1, cfg.canvas)[0])
        ref = O.gumbel_argmax(post, u, t)
        got = nxt[0].cpu().long()
        bad = torch.nonzero(got != ref).reshape(-1)
        if len(bad):
            gum = -torch.log(-torch.log(torch.clamp(u, min=torch.finfo(torch.float32).tiny, max=1.0)))
            v = post.float() + gum
            for r in bad.tolist():
                gap = (v[r, ref[r]] - v[r, got[r]]).item()
                worst = max(worst, gap)
                audited += int(gap < 0.05)
            mism += len(bad)
        total += cfg.canvas
        x = nxt
    print(f"[oracle] tau={tau} k={k}: {mism} of {total} ids differ, {audited} of them near-ties, worst gap {worst:.4f}")
    assert mism == audited, f"{mism - audited} mismatches are not near-ties (worst gap {worst})"
    assert mism / total < 2e-3


# ---- 6. the property a reader can check without the arithmetic ------------------------------------------------------------------------
def test_with_top_k_50_every_revealed_id_lies_in_the_rows_kept_set(built_lib):
    """A property of THESE inputs, not of the contract: a class that was cut keeps the weight eps in the reference arithmetic, so in
    about one revealing draw in a thousand (975 cut classes x 1e-6 against a kept mass of ~1) a filtered-out class wins, as the
    reference says it should.  The inputs are therefore the 64-row kind on which the CPU oracle itself (Oracle arithmetic on the
    host-filtered logits, same Philox uniforms) reveals only kept ids -- asserted first, on the CPU -- and the kernel must then do
    the same.  (That the kernel draws what the unfiltered kernel draws on host-filtered logits, cut winners included, is test 1.)"""
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
        hf = host_filter(logits, tau, 50)
        kept = torch.isfinite(hf)[0]
        assert 50 <= int(kept.sum(-1).min()) and int(kept.sum(-1).max()) <= 53
        seed = 5 + t
        post = O.posterior_logits_closed(hf[0].half(), x[0].long(), t, tabs)
        ref = O.gumbel_argmax(post, torch.from_numpy(philox.uniform_batch(seed, t, 0, 1, T)[0]), t)
        ref_rev = ref != st.mask_id
        assert bool(kept[torch.arange(T), ref][ref_rev].all()), "precondition: the CPU oracle reveals only kept ids on these inputs"
        got, _ = st(logits, x, t, seed, sampling=(tau, 50))
        got = got[0].long()
        rev = got != st.mask_id
        n_revealed += int(rev.sum())
        assert bool(kept[torch.arange(T), got][rev].all()), f"tau={tau} t={t}: a masked row revealed an id outside its 50 kept classes"
    assert n_revealed > 100

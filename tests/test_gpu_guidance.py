"""Classifier-free guidance inside the sampler launch (include/d3pm_hip.h: d3pm_guidance).

The ids carry no tolerance anywhere:
  1. row level   d3pm_posterior_sample_guided == d3pm_posterior_sample (and its _known / _sampling / _nucleus forms) on logits combined
                 on the host (tests/guidance_ref.py), id for id: every logits dtype, K = 1025 and the general routine, crafted twins;
  2. the loop    d3pm_sample_loop_guided == d3pm_denoise_step at 2B chained with the guided step entry, where the fused preparation
                 launch runs (d = 512, bf16, folded LayerNorms) and where it does not (native shape);
  3. twin = cond with the utterance's own inputs as its null twin, w = 2 gives the unguided ids of a shard of a 2B batch;
  4. null        the default twin's logits are the oracle's logits for the empty text and prompt (fp32, 1e-3: the bound
                 tests/test_gpu_key_mask.py and tests/test_gpu_parity.py give the same comparison);
  5. a guided utterance of a ragged batch == that utterance alone; stream chunks == the unsplit call; also under mask_padding;
  6. compositions and refusals;
  7. the training hook: cond_drop against autograd over the oracle on the empty conditions.
python -m pytest tests/test_gpu_guidance.py -m gpu"""
import ctypes as C

import numpy as np
import pytest
import torch

import guidance_ref as R
from oracle import d3pm_oracle as O
from oracle import philox
from util import REPORT, load, native_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS = (0.5, 1.5, 3.0)


def _model(cfg, dtype, sd):
    from vall_e.vall_e import AR
    m = AR.from_config(cfg)
    m.load_state_dict(sd)
    return m.to(dtype).to(DEV)


@pytest.fixture(scope="module")
def native():
    from vall_e.vall_e import synth
    cfg = synth.D3PMConfig.native()
    sd = synth.make_state_dict(cfg, 0)
    texts, proms = synth.make_inputs(cfg, 8, 1)
    models = {}

    def get(dtype):
        if dtype not in models:
            models[dtype] = _model(cfg, dtype, sd)
        return models[dtype]
    return cfg, sd, texts, proms, get


@pytest.fixture(scope="module")
def libri():
    from vall_e.vall_e import synth
    cfg = synth.D3PMConfig.libritts()
    sd = synth.make_state_dict(cfg, 0)
    texts, proms = synth.make_inputs(cfg, 12, 1)
    return cfg, sd, texts, proms, _model(cfg, torch.bfloat16, sd)


# ---- 1. row level ---------------------------------------------------------------------------------------------------------------------
class Step:
    """The step entries on a bare shape (no weights): K and the canvas are free."""

    def __init__(self, K, canvas):
        from vall_e.vall_e import _hip, synth
        self.hip = _hip
        self.shape = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
        self.shape.n_classes, self.shape.mask_id, self.shape.canvas, self.shape.n_q = K, K // 2, canvas, 1
        self.K, self.canvas, self.mask_id = K, canvas, K // 2
        self.sched = _hip.Schedule(100)

    def _tail(self, x_t, t, seed, flags):
        return int(t), C.byref(self.sched.c_struct), seed, 0, flags

    def unguided(self, logits, x_t, t, seed, *, known=None, sampling=None, nucleus=None, flags=0):
        hip, pp = self.hip, (lambda v: None if v is None else C.c_void_p(v.data_ptr()))
        logits, x_t = logits.to(DEV).contiguous(), x_t.to(DEV).contiguous()
        x_next = torch.full_like(x_t, -7)
        head = (C.byref(self.shape), x_t.shape[0], pp(logits), hip.dtype_code(logits.dtype), pp(x_t), pp(x_next))
        if nucleus is not None:
            nu = hip.Nucleus(*nucleus)
            hip.check(hip.lib().d3pm_posterior_sample_nucleus(*head, pp(known), *self._tail(x_t, t, seed, flags), None, C.byref(nu), None,
                                                              hip.stream_ptr()), "nucleus")
        elif sampling is not None:
            sm = hip.Sampling(*sampling)
            hip.check(hip.lib().d3pm_posterior_sample_sampling(*head, pp(known), *self._tail(x_t, t, seed, flags), None, C.byref(sm),
                                                               hip.stream_ptr()), "sampling")
        elif known is not None:
            hip.check(hip.lib().d3pm_posterior_sample_known(*head, pp(known), *self._tail(x_t, t, seed, flags), None, hip.stream_ptr()), "known")
        else:
            hip.check(hip.lib().d3pm_posterior_sample(*head, *self._tail(x_t, t, seed, flags), None, hip.stream_ptr()), "plain")
        torch.cuda.synchronize()
        return x_next.cpu()

    def guided(self, both, x_t, t, seed, w, *, known=None, nucleus=None, flags=0):
        hip, pp = self.hip, (lambda v: None if v is None else C.c_void_p(v.data_ptr()))
        both, x_t = both.to(DEV).contiguous(), x_t.to(DEV).contiguous()
        assert both.shape == (2 * x_t.shape[0], self.canvas, self.K)
        x_next = torch.full_like(x_t, -7)
        cv = None if known is None else hip.Canvas(None, known.data_ptr())
        nu = None if nucleus is None else hip.Nucleus(*nucleus)
        gd = hip.Guidance(w)
        hip.check(hip.lib().d3pm_posterior_sample_guided(C.byref(self.shape), x_t.shape[0], pp(both), hip.dtype_code(both.dtype), pp(x_t),
                                                         pp(x_next), None if cv is None else C.byref(cv), *self._tail(x_t, t, seed, flags),
                                                         None if nu is None else C.byref(nu), C.byref(gd), hip.stream_ptr()), "guided")
        torch.cuda.synchronize()
        return x_next.cpu()


def _to(dtype, a):
    return torch.from_numpy(a).to(dtype)


@pytest.mark.parametrize("K", [1025, 257])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_guided_step_equals_the_unguided_entry_on_host_combined_logits(built_lib, dtype, K):
    """B = 2 utterances of 37 frames (74 rows: no multiple of the 4 rows of a workgroup, 19 workgroups), every row's twin its own.
    fp32 logits hold fp16-grid values; the reference is exact for these inputs (asserted).  Rows cycle through masked | revealed at
    the conditioned peak | revealed at the guided peak | revealed elsewhere."""
    B, T = 2, 37
    st = Step(K, T)
    grid = "bfloat16" if dtype == torch.bfloat16 else np.float16
    c, u = R.crafted(B * T, K, seed=K + 3, dtype=grid)
    both = _to(dtype, np.concatenate([c, u]).reshape(2 * B, T, K))
    assert np.array_equal(both.float().numpy().reshape(2 * B * T, K), np.concatenate([c, u])), "the inputs sit on the dtype's grid"
    r = np.arange(B * T)
    x = np.full(B * T, st.mask_id, dtype=np.int32)
    x[r % 4 == 1] = c.argmax(-1)[r % 4 == 1]
    x[r % 4 == 2] = R.combine(c, u, 1.5).astype(np.float32).argmax(-1)[r % 4 == 2]
    x[r % 4 == 3] = (r[r % 4 == 3] * 7) % min(K, 1024)
    x = torch.from_numpy(x).reshape(B, T)
    g = torch.Generator().manual_seed(K)
    known = (torch.rand(B, T, generator=g) < 0.3).to(torch.uint8).to(DEV)
    k = min(50, K)
    modes = [("plain", {}, {}), ("known", dict(known=known), dict(known=known)),
             ("temperature + top-k", dict(sampling=(0.7, k)), dict(nucleus=(0.7, k, 1.0))),
             ("top-p", dict(nucleus=(1.0, 0, 0.9)), dict(nucleus=(1.0, 0, 0.9))),
             ("all three + known", dict(nucleus=(1.3, k, 0.95), known=known), dict(nucleus=(1.3, k, 0.95), known=known)),
             ("greedy", dict(flags=1), dict(flags=1))]
    moved = 0
    for w in WS:
        assert R.exact(c, u, w).all() and R.exact_rational(c, u, w, n=300)
        z = torch.from_numpy(R.combine(c, u, w).astype(np.float32)).reshape(B, T, K)      # fp32 logits on the fp16 grid
        for (name, kw_ref, kw_g), t in [(m, t) for m in modes for t in (60, 1, 0)]:
            seed = 1000 * t + int(w * 8)
            ref = st.unguided(z, x, t, seed, **kw_ref)
            got = st.guided(both, x, t, seed, w, **kw_g)
            assert torch.equal(got, ref), f"{name} w={w} t={t}: {(got != ref).sum().item()} of {B * T} ids differ"
            if name == "greedy" and t == 0:      # what a kernel that ignores u, or swaps the halves, would return
                assert (ref.reshape(-1).numpy() != c.argmax(-1)).mean() >= 0.5 and (ref.reshape(-1).numpy() != u.argmax(-1)).mean() >= 0.5
                swapped = st.guided(torch.cat([both[B:], both[:B]]), x, t, seed, w, **kw_g)
                moved += int((swapped != ref).sum())
    assert moved > 0


# ---- 2. the loop == the steps ----------------------------------------------------------------------------------------------------------
def _loop_vs_steps(m, cfg, texts, proms, B, steps, w, seed, **opts):
    from vall_e.vall_e import _hip
    smp = m.sampler()
    with torch.cuda.device(DEV), _hip.tuning(regime_batch=0):
        nt, npm = m._null_conditions(texts[:B], None, 1), m._null_conditions(proms[:B], None, 2)
        ct, cp = m.encode_conditions(list(texts[:B]) + nt, list(proms[:B]) + npm)
        kv_t, kv_p = smp.cond_kv(ct, cp)
        x0, fm = m.canvas_init(B)
        x = x0.clone()
        trace = smp.sample_loop(x, fm, steps, 0, kv_t, kv_p, seed, guidance=w, trace=True, **opts)
        y = x0.clone()
        for i, t in enumerate(range(steps, 0, -1)):
            lg, _ = smp.denoise(torch.cat([y, y]).contiguous(), fm, t, kv_t, kv_p)
            y, _ = smp.posterior_sample(lg[:B], y, t, seed, guidance=w, null_logits=lg[B:], **opts)
            assert torch.equal(trace[i], y), f"step t={t}: {(trace[i] != y).sum().item()} ids differ"
        torch.cuda.synchronize()
    assert torch.equal(x, y) and tuple(trace.shape) == (steps, B, cfg.canvas)
    return x


def test_loop_equals_the_steps_where_the_fused_preparation_runs(libri):
    """d = 512, bf16, folded LayerNorms: from the second iteration on the embedding rows and moments of BOTH halves come from the
    guided sampler launch of the iteration before."""
    cfg, _, texts, proms, m = libri
    a = _loop_vs_steps(m, cfg, texts, proms, 2, 5, 1.5, 11)
    b = _loop_vs_steps(m, cfg, texts, proms, 2, 5, 1.5, 11, temperature=0.8, top_k=40, top_p=0.9)
    assert not torch.equal(a, b)


def test_loop_equals_the_steps_native(native):
    cfg, _, texts, proms, get = native
    _loop_vs_steps(get(torch.float16), cfg, texts, proms, 2, 6, 3.0, 5)


# ---- 3. the twin is the condition ------------------------------------------------------------------------------------------------------
def _twin_is_cond(m, texts, proms, B, steps, seed):
    t, p = list(texts[:B]), list(proms[:B])
    got = m.generate_audio(t, p, seed=seed, steps=steps, guidance=2.0, null_text_list=t, null_proms_list=p)
    ref = m.generate_audio(t, p, seed=seed, steps=steps, global_batch=2 * B)
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} ids differ"


def test_twin_equal_to_the_condition_gives_the_unguided_ids_native_full_loop(native):
    cfg, _, texts, proms, get = native
    _twin_is_cond(get(torch.float16), texts, proms, 2, None, 21)


@pytest.mark.parametrize("B", [1, 6])
def test_twin_equal_to_the_condition_gives_the_unguided_ids_d512(libri, B):
    """B = 6: the evaluation of 12 utterances crosses the attention regime at 11, like the unguided shard of a batch of 12."""
    cfg, _, texts, proms, m = libri
    _twin_is_cond(m, texts, proms, B, 6, 31 + B)


# ---- 4. the null condition -------------------------------------------------------------------------------------------------------------
def test_default_null_twin_is_the_oracles_empty_condition_fp32(native):
    from vall_e.vall_e.ar_discrete import MASK_ID
    cfg, sd, texts, proms, get = native
    m = get(torch.float32)
    smp = m.sampler()
    g = torch.Generator().manual_seed(4)
    L = cfg.n_frames
    x = torch.zeros(cfg.canvas, dtype=torch.int64)
    x[:L] = torch.where(torch.rand(L, generator=g) < 0.5, torch.full((L,), MASK_ID), torch.randint(0, 1024, (L,), generator=g))
    with torch.cuda.device(DEV):
        ct, cp = m.encode_conditions([texts[0]] + m._null_conditions(texts[:1], None, 1), [proms[0]] + m._null_conditions(proms[:1], None, 2))
        kv_t, kv_p = smp.cond_kv(ct, cp)
        _, fm = m.canvas_init(1)
        xt = x.to(torch.int32).to(DEV)[None]
        lg, _ = smp.denoise(torch.cat([xt, xt]).contiguous(), fm, 40, kv_t, kv_p)
    orc = O.Oracle({k: v.float() for k, v in sd.items()}, O.Shape.of(cfg))
    with torch.no_grad():
        rcp, rct = orc.conditions(texts[0][:0], proms[0][:0])
        ref = orc.logits(x, 40, rcp, rct, torch.arange(cfg.canvas) < L)
        ccp, cct = orc.conditions(texts[0], proms[0])
        cond = orc.logits(x, 40, ccp, cct, torch.arange(cfg.canvas) < L)
    err = (lg[1].cpu() - ref).abs().max().item()
    err_c = (lg[0].cpu() - cond).abs().max().item()
    apart = (ref - cond).abs().max().item()
    print(f"[guidance] fp32 null twin vs oracle {err:.2e}, conditioned half {err_c:.2e}, null vs conditioned {apart:.2e}")
    REPORT["guidance_null_fp32_vs_oracle"] = {"null": err, "cond": err_c, "null_vs_cond": apart}
    assert err < 1e-3 and err_c < 1e-3 and apart > 10 * 1e-3


# ---- 5. batch independence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_padding", [False, True])
def test_a_guided_utterance_of_a_ragged_batch_is_that_utterance_alone_d512(libri, mask_padding):
    cfg, _, texts, proms, m = libri
    B, lens = 3, [37, cfg.canvas, 333]
    t, p = list(texts[:B]), list(proms[:B])
    kw = dict(seed=9, steps=4, guidance=1.5, mask_padding=mask_padding)
    whole = m.generate_audio(t, p, n_frames=lens, **kw)
    for b in range(B):
        alone = m.generate_audio([t[b]], [p[b]], n_frames=[lens[b]], utt0=b, global_batch=B, **kw)
        assert torch.equal(whole[b], alone), f"utterance {b}: {(whole[b] != alone).sum().item()} ids differ"
    chunks = m.generate_audio(t, p, n_frames=lens, streams=2, **kw)
    assert torch.equal(whole, chunks)


def test_a_guided_utterance_of_a_ragged_batch_is_that_utterance_alone_native(native):
    cfg, _, texts, proms, get = native
    m = get(torch.float16)
    B, lens = 3, [37, cfg.canvas, 129]
    t, p = list(texts[:B]), list(proms[:B])
    nt = [texts[5][:7], None, texts[6]]      # a caller-given negative condition for two of them
    for mp in (False, True):
        kw = dict(seed=2, steps=4, guidance=3.0, mask_padding=mp, top_p=0.9)
        whole = m.generate_audio(t, p, n_frames=lens, null_text_list=nt, **kw)
        for b in range(B):
            alone = m.generate_audio([t[b]], [p[b]], n_frames=[lens[b]], utt0=b, global_batch=B, null_text_list=[nt[b]], **kw)
            assert torch.equal(whole[b], alone)
        assert torch.equal(whole, m.generate_audio(t, p, n_frames=lens, null_text_list=nt, streams=3, **kw))


# ---- 6. compositions and refusals ------------------------------------------------------------------------------------------------------
def test_known_frames_trace_zero_weight_and_refusals(native):
    cfg, _, texts, proms, get = native
    m = get(torch.float16)
    t, p = list(texts[:2]), list(proms[:2])
    g = torch.Generator().manual_seed(1)
    known = [torch.randint(0, 1024, (40,), generator=g), None]
    out, trace = m.generate_audio(t, p, seed=3, steps=5, guidance=1.5, n_frames=[100, 60], known=known, return_trace=True)
    assert tuple(trace.shape) == (5, 2, cfg.canvas) and torch.equal(trace[-1].long().cpu(), out.cpu())
    assert torch.equal(out[0, :40].cpu(), known[0]) and torch.equal(trace[:, 0, :40].long().cpu(), known[0].expand(5, 40))
    plain = m.generate_audio(t, p, seed=3, steps=5)
    assert torch.equal(m.generate_audio(t, p, seed=3, steps=5, guidance=0.0), plain)
    assert not torch.equal(m.generate_audio(t, p, seed=3, steps=5, guidance=3.0), plain)
    for kw in (dict(graph=True), dict(fp8=True), dict(reveal_steps=4)):
        with pytest.raises(ValueError):
            m.generate_audio(t, p, seed=3, steps=5, guidance=1.0, **kw)
    # the C entries refuse with D3PM_E_ARG and a message, nothing launched
    from vall_e.vall_e import _hip
    smp = m.sampler()
    lib, sh, sched = _hip.lib(), smp.shape, smp.schedule.c_struct
    x, fm = m.canvas_init(1)
    lg = torch.zeros(2, cfg.canvas, cfg.n_classes, dtype=torch.float16, device=DEV)
    pp = lambda v: C.c_void_p(v.data_ptr())

    def step(gd, flags=0):
        return lib.d3pm_posterior_sample_guided(C.byref(sh), 1, pp(lg), _hip.F16, pp(x), pp(x), None, 5, C.byref(sched), 1, 0, flags, None,
                                                None if gd is None else C.byref(gd), _hip.stream_ptr())
    for gd, flags in ((None, 0), (_hip.Guidance(-0.5), 0), (_hip.Guidance(float("nan")), 0), (_hip.Guidance(float("inf")), 0),
                      (_hip.Guidance(1.0), 4)):      # 4 = D3PM_FLAG_SEED_IN_HBM
        assert step(gd, flags) == -1 and lib.d3pm_last_error(), (gd, flags)
    ws = smp.workspace(2)
    kv_t, kv_p = smp.cond_kv(*m.encode_conditions(t, p))
    fp8 = C.c_void_p(ws.data_ptr())      # any non-null pointer: refused before it is read

    def loop(gd, flags=0, f8=None):
        return lib.d3pm_sample_loop_guided(C.byref(sh), C.byref(smp.weights.c_struct), f8, 1, pp(x), pp(fm), None, 3, 0, pp(smp.film), pp(kv_t),
                                           pp(kv_p), C.byref(sched), 1, 0, flags, pp(ws), ws.numel(), None, None, None,
                                           None if gd is None else C.byref(gd), _hip.stream_ptr())
    for gd, flags, f8 in ((None, 0, None), (_hip.Guidance(-1.0), 0, None), (_hip.Guidance(1.0), 4, None), (_hip.Guidance(1.0), 0, fp8)):
        assert loop(gd, flags, f8) == -1 and lib.d3pm_last_error()
    torch.cuda.synchronize()
    assert int((x.cpu() != m.canvas_init(1)[0].cpu()).sum()) == 0, "a refused call launches nothing"


# ---- 7. the training hook ---------------------------------------------------------------------------------------------------------------
def _oracle_grads(cfg, sd32, text, prom, resps, seed, T):
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd32.items()}

    def q_noise(t):
        return torch.from_numpy(philox.uniform_batch(seed, t, 0, 1, cfg.canvas, stream=philox.STREAM_Q_SAMPLE))[0]

    loss, _ = O.training_forward(sd, O.Shape.of(cfg), text, prom, resps, q_noise, timesteps=T)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}


def _hip_grads(sd32, text, prom, resps, seed, T, **kw):
    from vall_e.vall_e import AR
    from vall_e.vall_e.train import D3PMTrainer
    m = AR.reference_native()
    m.load_state_dict(sd32)
    m = m.float().to(DEV)
    loss, _ = D3PMTrainer(m).forward_backward([text], [prom], [resps], seed=seed, timesteps=T, **kw)
    return float(loss), {n: (None if p.grad is None else p.grad.detach().cpu().clone()) for n, p in m.named_parameters()}


def _check_grads(got_loss, got, ref_loss, ref):
    """the tolerances of tests/test_gpu_train.py::test_gradients_match_autograd_over_the_oracle"""
    assert abs(got_loss - ref_loss) < 1e-4 * max(1.0, abs(ref_loss)), (got_loss, ref_loss)
    checked = 0
    for name, g in got.items():
        if ".cross_attn2." in name or name.startswith("token_emb"):
            continue
        want = ref.get(name)
        if want is None:
            assert g is None or float(g.abs().max()) == 0.0, name
            continue
        assert g is not None, f"no gradient for {name}"
        if name in ("text_emb.weight", "resps_emb.weight"):
            want = want.clone()
            want[0] = 0
        err, scale = (g - want).abs().max().item(), want.abs().max().item()
        assert err <= 2e-4 * scale + 1e-7, f"{name}: max |grad error| {err:.3e} vs gradient scale {scale:.3e}"
        checked += 1
    assert checked > 100


def _atomically_accumulated(name):
    """Gradients that csrc/d3pm_train.hip sums with atomicAdd, in whatever order the waves arrive: the weight and bias of every
    LayerNorm (layernorm_bwd_rows: dw, db), the FiLM gradient of norm3 (dfilm) and what is computed from it -- timestep_fc's weight and
    bias and time_emb -- and the embedding tables (embed_bwd_rows: text_emb, proms_emb, resps_emb).  Two runs of one and the same call
    differ in their last bits there.  Every other gradient comes out of matmul / colsum / attention kernels with a fixed order."""
    return "norm" in name or "timestep_fc" in name or name.endswith("_emb.weight")


def test_cond_drop_matches_autograd_over_the_oracle_on_the_empty_conditions():
    """cond_drop = (1, 1) and a "text only" seed against autograd over the oracle on the empty conditions, with the tolerances of
    tests/test_gpu_train.py; the device decision against the mirror.
    cond_drop = 0 against the call without the argument: the issue asks for the gradients bit for bit.  That holds, and is asserted,
    for the loss and for every gradient that is accumulated in a fixed order (at least 150 named tensors, `final` among them).  It
    CANNOT hold for the tensors _atomically_accumulated names: there two runs of today's call are not bit-equal to each other, so no
    test can ask it of a third.  This is a deviation from the issue's wording: those tensors are held to 2e-4 * scale + 1e-7, the
    tolerance the issue sets for the same tensors against the oracle, which a change of arithmetic would not pass unnoticed
    (accumulation-order noise in fp32 is four orders below it)."""
    from vall_e.vall_e.train import cond_drop_decision
    cfg, sd32, texts, proms, _ = native_setup(torch.float32)
    g = load("native_forward.npz")
    resps = torch.from_numpy(g["resps"].astype(np.int64))
    seed, T = int(g["seed"]), 3
    text, prom = texts[0], proms[0]
    # both dropped: the oracle on the empty text and prompt
    _check_grads(*_hip_grads(sd32, text, prom, resps, seed, T, cond_drop=(1.0, 1.0)), *_oracle_grads(cfg, sd32, text[:0], prom[:0], resps, seed, T))
    # 0 is the step without the argument
    l0, g0 = _hip_grads(sd32, text, prom, resps, seed, T)
    l1, g1 = _hip_grads(sd32, text, prom, resps, seed, T, cond_drop=0.0)
    assert l0 == l1, "the loss (the whole forward pass) bit for bit"
    same = lambda a, b: (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))
    atomic = [n for n in g0 if _atomically_accumulated(n)]
    exact = [n for n in g0 if not _atomically_accumulated(n)]
    assert len(exact) >= 150 and {"final.weight", "final.bias"} <= set(exact), (len(exact), len(atomic))
    assert sum(g0[n] is not None for n in exact) >= 100
    differ = [n for n in exact if not same(g0[n], g1[n])]
    assert not differ, f"not bit-equal to the call without the argument: {differ}"
    for n in atomic:
        if g0[n] is None:
            assert g1[n] is None, n
            continue
        scale = g0[n].abs().max().item()
        assert (g0[n] - g1[n]).abs().max().item() <= 2e-4 * scale + 1e-7, n
    # a seed for which the mirror says "text only" at p = 0.5: the device decision agrees and the step is the oracle's on (empty, prompt)
    s = next(s for s in range(seed, seed + 64) if R.cond_drop_mirror(s, 0, 0.5, 0.5) == (True, False))
    for utt in range(6):
        assert cond_drop_decision(s, utt, 0.5, 0.5, DEV) == R.cond_drop_mirror(s, utt, 0.5, 0.5)
        assert cond_drop_decision(s, utt, 0.3, 0.9, DEV) == R.cond_drop_mirror(s, utt, 0.3, 0.9)
    _check_grads(*_hip_grads(sd32, text, prom, resps, s, T, cond_drop=0.5), *_oracle_grads(cfg, sd32, text[:0], prom, resps, s, T))

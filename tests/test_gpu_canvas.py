"""Per-utterance canvases on the GPU (include/d3pm_hip.h: d3pm_canvas): lengths and known frames in one
batch.  Every comparison between HIP paths is an equality of ids; the audit against the CPU oracle is the one check with a bound.
  1. an int n_frames, n_frames=[L] * B and no known frames give the same ids;
  2. utterance b of a ragged batch = that utterance alone with n_frames=L_b, utt0 + b and the same global_batch;
  3. a known map that is all zero = no map;
  4. the fused loop = denoise -> posterior_sample -> torch.where(known, x_T, x_next), step by step;
  5. shards and stream chunks reproduce the unsplit ragged / known batch."""
import numpy as np
import pytest
import torch

from oracle import philox
from util import native_setup

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _model(cfg, dtype, seed=0):
    from vall_e.vall_e import AR, synth
    m = AR.from_config(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, seed))
    return m.to(dtype).to(DEV)


@pytest.fixture(scope="module")
def libri():
    from vall_e.vall_e import synth
    cfg = synth.D3PMConfig.libritts()
    texts, proms = synth.make_inputs(cfg, 32, 1)
    models = {}

    def get(dtype):
        if dtype not in models:
            models[dtype] = _model(cfg, dtype)
        return models[dtype]
    return cfg, texts, proms, get


@pytest.fixture(scope="module")
def native():
    from vall_e.vall_e import synth
    cfg = synth.D3PMConfig.native()
    texts, proms = synth.make_inputs(cfg, 8, 1)
    models = {}

    def get(dtype):
        if dtype not in models:
            models[dtype] = _model(cfg, dtype)
        return models[dtype]
    return cfg, texts, proms, get


def _lengths(B, canvas):
    """1, the whole canvas, and values that are no multiples of 16, 32 or 128."""
    pool = [1, canvas, 37, canvas - 1, 333, 129, 15, 250, 97, 401, 7, 211]
    return [min(pool[i % len(pool)] + 2 * (i // len(pool)), canvas) for i in range(B)]


def _known_for(lens, seed=3):
    """prefix (no mask), gap, scattered, none -- cycling over the utterances."""
    g = torch.Generator().manual_seed(seed)
    known, kmask = [], []
    for b, L in enumerate(lens):
        kind = b % 4
        ids = torch.randint(0, 1024, (L,), generator=g)
        if kind == 0 or L < 4:
            known.append(ids[: max(1, L // 3)]); kmask.append(None)                  # a prefix to continue
        elif kind == 1:
            mk = torch.ones(L, dtype=torch.bool); mk[L // 4: L // 2] = False          # a gap to fill
            known.append(ids); kmask.append(mk)
        elif kind == 2:
            known.append(ids); kmask.append(torch.rand(L, generator=g) < 0.4)         # scattered
        else:
            known.append(None); kmask.append(None)
    return known, kmask


def _assert_rows_alone(m, texts, proms, lens, which, out, *, steps, seed, utt0=0, known=None, kmask=None, **kw):
    B = len(lens)
    for b in which:
        alone = m.generate_audio(texts[b:b + 1], proms[b:b + 1], n_frames=lens[b], steps=steps, seed=seed, utt0=utt0 + b, global_batch=B,
                                 known=None if known is None else known[b:b + 1], known_mask=None if kmask is None else kmask[b:b + 1], **kw)
        assert torch.equal(out[b], alone.reshape(out[b].shape)), \
            f"utterance {b} (L = {lens[b]}): {(out[b] != alone.reshape(out[b].shape)).sum().item()} ids differ from the utterance alone"


# ---- equality 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["native-fp16", "libritts-bf16"])
def test_uniform_lengths_and_empty_maps_are_todays_ids(native, libri, which):
    cfg, texts, proms, get = native if which == "native-fp16" else libri
    m = get(torch.float16 if which == "native-fp16" else torch.bfloat16)
    B, steps = 4, (99 if which == "native-fp16" else 12)
    ref = m.generate_audio(texts[:B], proms[:B], n_frames=350, steps=steps, seed=21)
    seq = m.generate_audio(texts[:B], proms[:B], n_frames=[350] * B, steps=steps, seed=21)
    assert torch.equal(seq, ref)
    zero = [torch.zeros(350, dtype=torch.bool)] * B
    none = m.generate_audio(texts[:B], proms[:B], n_frames=350, steps=steps, seed=21, known=[torch.zeros(350, dtype=torch.long)] * B, known_mask=zero)
    assert torch.equal(none, ref)
    # equality 3 at the kernels: an all-zero map travels to the known-row arm of the sampler and changes nothing
    smp = m.sampler()
    ct, cp = m.encode_conditions(texts[:B], proms[:B])
    kv_t, kv_p = smp.cond_kv(ct, cp)
    x, fm = m.canvas_init(B, [350] * B)
    smp.sample_loop(x, fm, steps, 0, kv_t, kv_p, 21, known=torch.zeros_like(fm))
    assert torch.equal(x.long(), ref)
    x, fm1 = m.canvas_init(B, 350)      # a shared mask with a map: repeated per utterance
    smp.sample_loop(x, fm1, steps, 0, kv_t, kv_p, 21, known=torch.zeros_like(fm))
    assert torch.equal(x.long(), ref)


# ---- equality 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ragged_batch_of_four_d512(libri, dtype):
    """Below the attention regime boundary of 11 utterances; the row moments travel as 32-column parts."""
    cfg, texts, proms, get = libri
    m = get(dtype)
    lens = [1, cfg.canvas, 333, 37]
    out = m.generate_audio(texts[:4], proms[:4], n_frames=lens, steps=10, seed=7)
    assert out.shape == (4, cfg.canvas)
    _assert_rows_alone(m, texts, proms, lens, range(4), out, steps=10, seed=7)


@pytest.mark.parametrize("B", [12, 32])
def test_ragged_batch_above_the_regime_boundary_d512(libri, B):
    """12 and 32 utterances (at 32 the folded sequence runs on big tiles and the moments travel as quads), short runs."""
    cfg, texts, proms, get = libri
    m = get(torch.bfloat16)
    lens = _lengths(B, cfg.canvas)
    out = m.generate_audio(texts[:B], proms[:B], n_frames=lens, steps=4, seed=9)
    _assert_rows_alone(m, texts, proms, lens, [0, 1, 2, 3, B - 1], out, steps=4, seed=9)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_ragged_batch_native_shape(native, dtype):
    """fp32 runs the generic family; fp16 is the dtype the reference samples in."""
    cfg, texts, proms, get = native
    m = get(dtype)
    lens = [1, cfg.canvas, 349, 37, 130]
    out = m.generate_audio(texts[:5], proms[:5], n_frames=lens, steps=12, seed=4)
    _assert_rows_alone(m, texts, proms, lens, range(5), out, steps=12, seed=4)


def test_ragged_batch_without_the_layernorm_fold_d512(libri):
    """ln_fold = 0: the fused-embed LayerNorm, the row-panel form of fc2 and the stand-alone sampler carry the period."""
    from vall_e.vall_e import _hip
    cfg, texts, proms, get = libri
    m = get(torch.bfloat16)
    with _hip.tuning(ln_fold=0):
        for B, which in ((4, range(4)), (32, [0, 1, 2, 31])):
            lens = _lengths(B, cfg.canvas)
            out = m.generate_audio(texts[:B], proms[:B], n_frames=lens, steps=3, seed=13)
            _assert_rows_alone(m, texts, proms, lens, which, out, steps=3, seed=13)


def test_ragged_and_known_batch_with_eight_levels(libri):
    """n_q = 8: the map is per frame, all levels of a known frame are kept."""
    from vall_e.vall_e import synth
    cfg = synth.D3PMConfig.libritts_8q()
    _, texts, proms, _ = libri
    m = _model(cfg, torch.bfloat16)
    lens = [37, cfg.canvas, 1]
    g = torch.Generator().manual_seed(2)
    known = [torch.randint(0, 1024, (20, 8), generator=g), None, None]
    out, trace = m.generate_audio(texts[:3], proms[:3], n_frames=lens, steps=4, seed=6, known=known, return_trace=True)
    assert out.shape == (3, cfg.canvas, 8)
    assert all(torch.equal(trace[i, 0, :20].long().cpu(), known[0]) for i in range(trace.shape[0]))
    _assert_rows_alone(m, texts, proms, lens, range(3), out, steps=4, seed=6, known=known)


# ---- equalities 3 and 4 ----------------------------------------------------------------------------------------------------------
def _loop_vs_steps(m, texts, proms, lens, known, kmask, t_start, seed):
    smp = m.sampler()
    B = len(lens)
    ct, cp = m.encode_conditions(texts[:B], proms[:B])
    kv_t, kv_p = smp.cond_kv(ct, cp)
    x_T, fm, km = m.canvas_init_known(B, lens, known, kmask)
    assert km is not None
    x = x_T.clone()
    trace = smp.sample_loop(x, fm, t_start, 0, kv_t, kv_p, seed, known=km, trace=True)
    keep = km.bool()
    xs = x_T.clone()
    for i, t in enumerate(range(t_start, 0, -1)):
        lg, _ = smp.denoise_canvas(xs, fm, t, kv_t, kv_p)
        nxt, _ = smp.posterior_sample(lg, xs, t, seed, known=km)
        free, _ = smp.posterior_sample(lg, xs, t, seed)
        assert torch.equal(nxt, torch.where(keep, x_T, free)), f"t = {t}: the known-row arm is not replacement conditioning"
        assert torch.equal(trace[i], nxt), f"t = {t}: {(trace[i] != nxt).sum().item()} ids of the fused loop differ from the step-by-step composition"
        assert torch.equal(nxt[keep], x_T[keep])          # the given ids, at every step
        xs = nxt
    assert torch.equal(x, xs)
    # and through the public call
    out, tr = m.generate_audio(texts[:B], proms[:B], n_frames=lens, steps=t_start, seed=seed, known=known, known_mask=kmask, return_trace=True)
    assert torch.equal(out, x.long()) and torch.equal(tr, trace)
    return x, x_T, keep


def test_known_frames_native_fp16_full_loop(native):
    """Prefix, gap and scattered maps, all 99 steps: the fused loop against denoise_canvas + posterior_sample(known=)."""
    cfg, texts, proms, get = native
    lens = [350, 131, cfg.canvas, 37]
    known, kmask = _known_for(lens)
    known[3], kmask[3] = known[2][:37], kmask[2][:37]            # four utterances, three kinds of map + a second scattered one
    _loop_vs_steps(get(torch.float16), texts, proms, lens, known, kmask, 99, seed=31)


@pytest.mark.parametrize("B", [4, 32])
def test_known_frames_d512_bf16_short_loop(libri, B):
    """The sampler launch that also prepares the next iteration (embedding rows + moments of the known rows): parts at 4
    utterances, quads at 32."""
    cfg, texts, proms, get = libri
    lens = _lengths(B, cfg.canvas)
    known, kmask = _known_for(lens)
    _loop_vs_steps(get(torch.bfloat16), texts, proms, lens, known, kmask, 5 if B == 4 else 3, seed=17)


def test_a_known_row_keeps_a_token_that_loses_the_draw(native):
    """Rows come in pairs with the same revealed token and the same logits, peaked on ANOTHER class, so that the kept token loses
    the Gumbel race about every second time (d3pm_sample_row.h falls back to the full routine).  The known row of a pair keeps
    its token every time; the free rows do not."""
    cfg, texts, proms, get = native
    smp = get(torch.float16).sampler()
    T, K, t = cfg.canvas, cfg.n_classes, 2
    g = torch.Generator().manual_seed(8)
    tok = torch.randint(0, 512, (T // 2,), generator=g).repeat_interleave(2)
    x_t = tok.to(torch.int32)[None].contiguous().to(DEV)
    logits = torch.zeros(1, T, K, dtype=torch.float16)
    logits[0, torch.arange(T), (tok + 17) % 1024] = 20.0
    logits = logits.to(DEV)
    known = torch.zeros(1, T, dtype=torch.uint8, device=DEV)
    known[0, 0::2] = 1
    nxt, _ = smp.posterior_sample(logits, x_t, t, seed=77, known=known)
    free, _ = smp.posterior_sample(logits, x_t, t, seed=77)
    assert torch.equal(nxt[0, 0::2], x_t[0, 0::2])
    assert torch.equal(nxt[0, 1::2], free[0, 1::2])                # the free rows draw what they drew without the map
    lost = int((free[0] != x_t[0]).sum())
    assert lost > T // 8, f"only {lost} of {T} kept tokens lose: the logits do not exercise the case"
    assert int((free[0, 0::2] != x_t[0, 0::2]).sum()) > 0 and int((nxt[0, 1::2] != x_t[0, 1::2]).sum()) > 0


# ---- equality 5 ------------------------------------------------------------------------------------------------------------------
def test_shards_and_stream_chunks_reproduce_the_unsplit_batch(libri):
    cfg, texts, proms, get = libri
    m = get(torch.bfloat16)
    B = 12
    lens = _lengths(B, cfg.canvas)
    known, kmask = _known_for(lens)
    whole = m.generate_audio(texts[:B], proms[:B], n_frames=lens, steps=4, seed=5, known=known, known_mask=kmask)
    chunked = m.generate_audio(texts[:B], proms[:B], n_frames=lens, steps=4, seed=5, known=known, known_mask=kmask, streams=2)
    assert torch.equal(chunked, whole), f"stream chunking changes {(chunked != whole).sum().item()} ids"
    lo, hi = 5, 9
    shard = m.generate_audio(texts[lo:hi], proms[lo:hi], n_frames=lens[lo:hi], steps=4, seed=5, known=known[lo:hi], known_mask=kmask[lo:hi],
                             utt0=lo, global_batch=B)
    assert torch.equal(shard, whole[lo:hi])
    _, _, km = m.canvas_init_known(B, lens, known, kmask)
    x_T = m.canvas_init_known(B, lens, known, kmask)[0]
    assert torch.equal(whole[km.bool()], x_T.long()[km.bool()])


def test_fp8_ragged_batch_equals_each_utterance_alone(libri):
    cfg, texts, proms, get = libri
    m = get(torch.bfloat16)
    lens = [1, cfg.canvas, 333, 37]
    out = m.generate_audio(texts[:4], proms[:4], n_frames=lens, steps=4, seed=7, fp8=True)
    _assert_rows_alone(m, texts, proms, lens, range(4), out, steps=4, seed=7, fp8=True)
    plain = m.generate_audio(texts[:4], proms[:4], n_frames=lens, steps=4, seed=7)
    assert not torch.equal(out, plain), "the fp8 loop returned the 16-bit loop's ids"


def test_graph_replay_refuses_per_utterance_arguments(native):
    cfg, texts, proms, get = native
    with pytest.raises(ValueError):
        get(torch.float16).generate_audio(texts[:2], proms[:2], n_frames=[10, 20], steps=2, seed=1, graph=True)


def test_wrong_canvas_shapes_are_rejected_before_the_c_abi(native):
    from vall_e.vall_e import _hip
    cfg, texts, proms, get = native
    m = get(torch.float16)
    smp = m.sampler()
    ct, cp = m.encode_conditions(texts[:2], proms[:2])
    kv_t, kv_p = smp.cond_kv(ct, cp)
    x, fm = m.canvas_init(2, [5, 9])
    for bad_fm, bad_known in ((fm[:1], None), (fm[:, :-1].contiguous(), None), (fm.to(torch.int32), None), (fm, fm[:1]), (fm, fm.bool())):
        with pytest.raises(_hip.D3PMError):
            smp.sample_loop(x, bad_fm, 2, 0, kv_t, kv_p, 1, known=bad_known)
    with pytest.raises(_hip.D3PMError):
        smp.denoise_canvas(x, fm[:1], 2, kv_t, kv_p)


# ---- against the CPU oracle ------------------------------------------------------------------------------------------------------
def _oracle_trajectory(orc, cfg, cp, ct, mask, x_T, keep, seed, utt=0):
    """Oracle.step with a mask of L frames, followed by the same replacement."""
    x, traj = x_T.clone(), []
    for t in range(cfg.timesteps - 1, 0, -1):
        u = torch.from_numpy(philox.uniform_batch(seed, t, utt, 1, cfg.canvas)[0])
        with torch.no_grad():
            x = torch.where(keep, x_T, orc.step(x, t, cp, ct, mask, u))
        traj.append(x.numpy().copy())
    return np.stack(traj)


def test_teacher_forced_audit_against_the_oracle_with_a_length_and_a_known_prefix(native):
    """One utterance of the native fp16 shape with L = 211 != 350 and a known prefix of 60 frames, teacher-forced along the
    oracle's own trajectory as tests/test_gpu_parity.py::_audit does, under that test's bounds: every id equal, or the mismatch an
    audited near-tie (gap < 0.05), and mismatches / total < 2e-3 with `total` over the FREE LIVE rows only (known rows are
    trivially equal and must not dilute the rate; padded rows are compared and audited too but not counted in `total`).
    The composed oracle (Oracle.step + replacement) was run twice on the CPU before relying on it: deterministic, and with L = 350
    and no known frames it reproduces tests/golden/native_loop.npz (traj_utt0_seed123, all 99 steps) exactly, so the harness adds
    nothing; the determinism half is repeated here."""
    cfg, sd32, texts, proms, orc = native_setup(torch.float16)
    m = native[3](torch.float16)
    smp = m.sampler()
    L, P, seed = 211, 60, 123
    with torch.no_grad():
        cp, ct = orc.conditions(texts[0], proms[0])
    kv_t, kv_p = smp.cond_kv(ct[None].to(DEV), cp[None].to(DEV))
    prefix = torch.randint(0, 1024, (P,), generator=torch.Generator().manual_seed(12))
    x_T, fm, km = m.canvas_init_known(1, [L], known=[prefix])
    mask, keep, x0 = fm[0].bool().cpu(), km[0].bool().cpu(), x_T[0].long().cpu()
    traj = _oracle_trajectory(orc, cfg, cp, ct, mask, x0, keep, seed)
    assert np.array_equal(traj, _oracle_trajectory(orc, cfg, cp, ct, mask, x0, keep, seed)), "the composed oracle is not deterministic"
    assert (traj[:, :P] == prefix.numpy()).all()
    free_live = (mask & ~keep).numpy()
    prev = x0.numpy()
    mism, audited, worst = 0, 0, 0.0
    for i, t in enumerate(range(cfg.timesteps - 1, 0, -1)):
        ref_next = traj[i]
        x = torch.from_numpy(prev.astype(np.int32))[None].to(DEV)
        lg, _ = smp.denoise_canvas(x, fm, t, kv_t, kv_p)
        nxt, _ = smp.posterior_sample(lg, x, t, seed=seed, known=km)
        got = nxt[0].cpu().numpy()
        assert np.array_equal(got[:P], prefix.numpy())
        bad = np.nonzero(got != ref_next)[0]
        if len(bad):
            xp = torch.from_numpy(prev.astype(np.int64))
            with torch.no_grad():
                post = orc.posterior(orc.logits(xp, t, cp, ct, mask), xp, t)
            u = torch.from_numpy(philox.uniform_batch(seed, t, 0, 1, cfg.canvas)[0])
            v = post.float() - torch.log(-torch.log(torch.clamp(u, min=torch.finfo(torch.float32).tiny, max=1.0)))
            for r in bad:
                gap = (v[r, ref_next[r]] - v[r, got[r]]).item()
                worst = max(worst, gap)
                audited += int(gap < 0.05)
            mism += len(bad)
        prev = ref_next
    total = 99 * int(free_live.sum())
    print(f"canvas audit: {mism} mismatches, {audited} audited near-ties, worst gap {worst:.4f}, total {total}")
    assert mism == audited, f"{mism - audited} mismatches are not near-ties (worst gap {worst})"
    assert mism / total < 2e-3


# ---- python -m vall_e ------------------------------------------------------------------------------------------------------------
def test_cli_frames_and_continue_from(built_lib, tmp_path):
    """`python -m vall_e`, pre-tokenised form, --frames 200 --continue-from: writes [1, 8, 200], level 0 begins with the prefix."""
    from vall_e import __main__ as cli
    from vall_e.vall_e import get_model
    g = torch.Generator().manual_seed(4)
    torch.save(torch.randint(0, 1024, (1, 8, 120), generator=g), tmp_path / "prompt.qnt.pt")
    prefix = torch.randint(0, 1024, (1, 8, 50), generator=g)
    torch.save(prefix, tmp_path / "prefix.qnt.pt")
    torch.manual_seed(1)
    torch.save(get_model("nar-quarter").state_dict(), tmp_path / "nar.pt")
    out = tmp_path / "out.qnt.pt"
    torch.manual_seed(0)
    cli.main([str(out), "--phonemes", "5 9 12 3", "--prompt-qnt", str(tmp_path / "prompt.qnt.pt"), "--native", "--seed", "3",
              "--nar-model", "nar-quarter", "--nar-ckpt", str(tmp_path / "nar.pt"), "--frames", "200",
              "--continue-from", str(tmp_path / "prefix.qnt.pt")])
    q = torch.load(out)
    assert tuple(q.shape) == (1, 8, 200) and q.dtype == torch.int64
    assert torch.equal(q[0, 0, :50], prefix[0, 0])
    assert 0 <= q.min() and q[:, 1:].max() < 1024

"""Block-0 QKV from a per-id table (include/d3pm_hip.h: d3pm_tuning.ln_fold, d3pm_op_embed_qkv; csrc/d3pm_api.hip build_qkv_table).

The first block of an evaluation reads x[row] = resps_emb[id] (zeros on a padded frame) and nothing else in front of norm1, so its
folded QKV projection takes n_classes + 1 distinct rows.  Under ln_fold = 1 (default) the unguided sampler loops compute them once per
call and the launch that embeds a row copies its q | k | v; ln_fold = 2 keeps the projection in every block (the launch list from
before the table).  The contract is bit identity, checked here
  * row by row: the table against d3pm_op_linear_fold on the gathered embedding rows with d3pm_op_row_stats moments, in each GEMM
    family a loop can take (64 x 64 latency tiles at M = 768, 128 x 128 tiles at M = 1152, big tiles forced at M = 1152);
  * through the loops: ids and the full trace under ln_fold = 1 and ln_fold = 2 at 2 utterances (latency kernels, moments in
    parts) and at 24 (4608 rows: big tiles, moments in quads), with a shared mask, with per-utterance canvases + known frames + key
    counts, and with the filter / nucleus sampler kernels; the guided and the reveal loop keep the projection and agree trivially;
  * that the default really drops one GEMM launch per iteration (the library's own launch counter).
The host-side half (no GPU) is in tests/test_qkv_table_api.py.
"""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_START, T_STOP = 36, 30      # 6 timesteps; t = 32 is one the launch counter brackets (every 16th)


def _cfg():
    from vall_e.vall_e import synth
    return dataclasses.replace(synth.D3PMConfig.libritts(), n_heads=8, n_layers=2, canvas=192, n_frames=150)


@pytest.fixture(scope="module")
def models(built_lib):
    from vall_e.vall_e import AR, synth
    cfg = _cfg()
    cache = {}

    def get(dtype):
        if dtype not in cache:
            m = AR.from_config(cfg)
            m.load_state_dict(synth.make_state_dict(cfg, 0))
            cache[dtype] = m.to(dtype).to(DEV)
        return cache[dtype]
    return cfg, get


@pytest.fixture(scope="module")
def conditions(models):
    """bf16 model, 24 utterances: conditions and their K/V, computed once; the first B utterances serve a batch of B."""
    from vall_e.vall_e import synth
    cfg, get = models
    m = get(torch.bfloat16)
    texts, proms = synth.make_inputs(cfg, 24, 1)
    ct, cp = m.encode_conditions(texts, proms)
    return m, texts, proms, ct, cp


def _half_revealed(x, seed):
    """live frames of x_T: about half of them carry a codec id, the rest the mask id"""
    gen = torch.Generator().manual_seed(seed)
    show = torch.rand(x.shape, generator=gen) < 0.5
    ids = torch.randint(0, 1024, x.shape, generator=gen, dtype=torch.int32)
    return torch.where(show.to(DEV) & (x != 0), ids.to(DEV), x)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_table_rows_equal_the_folded_projection_in_every_gemm_family(models, dtype):
    from vall_e.vall_e import _hip
    cfg, get = models
    m = get(dtype)
    smp = m.sampler()
    assert smp.folded and cfg.d_model == 512 and cfg.n_classes == 1025
    sd = dict(m.named_parameters())
    emb = sd["resps_emb.weight"].detach()
    wf, fs, fb = _hip.op_fold_weights(sd["blocks.0.attn.in_proj_weight"].detach(), sd["blocks.0.attn.in_proj_bias"].detach(),
                                      sd["blocks.0.norm1.weight"].detach(), sd["blocks.0.norm1.bias"].detach())
    # every id, then one padded frame (its id is not read: a zero row)
    n = cfg.n_classes + 1
    tokens = torch.cat([torch.arange(cfg.n_classes, dtype=torch.int32), torch.tensor([7], dtype=torch.int32)]).to(DEV)
    fm = torch.ones(n, dtype=torch.uint8, device=DEV)
    fm[-1] = 0
    got = _hip.op_embed_qkv(smp.shape, smp.weights, tokens, fm)
    assert got.shape == (n, 3 * cfg.d_model)
    x = torch.zeros(1536, cfg.d_model, dtype=dtype, device=DEV)      # the gathered rows, zero rows behind them
    x[:cfg.n_classes] = emb
    for name, variant, M in (("latency 64 x 64", 0, 768), ("128 x 128", 2, 1152), ("big tiles", 8, 1152)):
        with _hip.tuning(gemm_variant=variant):
            chunks = []
            for lo in range(0, n, M):
                rows = x[lo:lo + M].contiguous()
                chunks.append(_hip.op_linear_fold(rows, wf, fs, fb, _hip.op_row_stats(rows)))
            ref = torch.cat(chunks)[:n]
            bad = (ref != got).any(dim=1)
            assert not bad.any(), f"{name}: rows {bad.nonzero().flatten().tolist()[:8]} of the table differ from the projection"
            # the table itself does not depend on the family that builds it
            assert torch.equal(_hip.op_embed_qkv(smp.shape, smp.weights, tokens, fm), got), name
    # a row's projection is not trivially constant: the ids differ from each other and from the padded frame (id 0 is the synthetic
    # weights' padding row, all zeros: it IS the padded frame's row)
    assert not torch.equal(got[1], got[2]) and not torch.equal(got[1], got[-1]) and torch.equal(got[0], got[-1])
    # ids outside the classes are clamped like the embedding gather clamps them
    odd = torch.tensor([-5, 4000, 3], dtype=torch.int32, device=DEV)
    g2 = _hip.op_embed_qkv(smp.shape, smp.weights, odd, torch.ones(3, dtype=torch.uint8, device=DEV))
    assert torch.equal(g2[0], got[0]) and torch.equal(g2[1], got[cfg.n_classes - 1]) and torch.equal(g2[2], got[3])


def _run(smp, x0, fm, kv, ln_fold, loop="sample", **kw):
    from vall_e.vall_e import _hip
    x = x0.clone()
    with _hip.tuning(ln_fold=ln_fold):
        if loop == "reveal":
            tr = smp.reveal_loop(x, fm, 4, kv[0], kv[1], seed=77, trace=True, **kw)
        else:
            tr = smp.sample_loop(x, fm, T_START, T_STOP, kv[0], kv[1], seed=77, trace=True, **kw)
    return x, tr


def _same(smp, x0, fm, kv, what, **kw):
    xa, ta = _run(smp, x0, fm, kv, 1, **kw)
    xb, tb = _run(smp, x0, fm, kv, 2, **kw)
    assert torch.equal(ta, tb), f"{what}: {(ta != tb).sum().item()} ids of the trace differ between ln_fold = 1 and 2"
    assert torch.equal(xa, xb), what
    assert not torch.equal(xa, x0), what
    return xa


@pytest.mark.parametrize("B", [2, 24])
def test_loop_ids_and_trace_equal_the_projection_loop(conditions, B):
    m, _, _, ct, cp = conditions
    smp = m.sampler()
    kv = smp.cond_kv(ct[:B].contiguous(), cp[:B].contiguous())
    x, fm = m.canvas_init(B)
    assert int(fm.sum()) < fm.numel(), "the frame mask must have padded frames"
    x = _half_revealed(x, 3 + B)
    plain = _same(smp, x, fm, kv, f"B={B} plain")
    if B == 2:      # the filter and the nucleus kernels of the sampler launch gather too
        filt = _same(smp, x, fm, kv, "temperature / top-k", temperature=0.8, top_k=40)
        nuc = _same(smp, x, fm, kv, "nucleus", temperature=0.9, top_p=0.9)
        assert not torch.equal(plain, filt) and not torch.equal(plain, nuc)


def test_loop_with_per_utterance_canvas_known_frames_and_key_counts(conditions):
    m, texts, proms, ct, cp = conditions
    smp = m.sampler()
    B, lens = 3, [150, 97, 192]
    gen = torch.Generator().manual_seed(8)
    known = [torch.randint(0, 1024, (40,), generator=gen), None, torch.randint(0, 1024, (192,), generator=gen)]
    kmask = [None, None, torch.rand(192, generator=gen) < 0.3]
    x, fm, km = m.canvas_init_known(B, lens, known=known, known_mask=kmask)
    assert km is not None and fm.dim() == 2
    f, tl, pl = m.key_lengths(texts[:B], proms[:B], lens)
    keys = tuple(torch.tensor(v, dtype=torch.int32, device=DEV) for v in (f, tl, pl))
    ctk, cpk = smp.encode_conditions(*m._padded_inputs(texts[:B], proms[:B]), keys[1], keys[2])
    kv = smp.cond_kv(ctk, cpk)
    out = _same(smp, x, fm, kv, "canvas + known + keys", known=km, keys=keys)
    given = km.bool()
    assert torch.equal(out[given], x[given]), "a known frame changed"
    kv = smp.cond_kv(ct[:B].contiguous(), cp[:B].contiguous())
    _same(smp, x, fm, kv, "canvas + known", known=km)


def test_guided_and_reveal_loops_keep_the_projection(conditions):
    """Neither loop gathers from the table (their sampler launches do not), so ln_fold = 1 and 2 run the same launches."""
    m, texts, proms, ct, cp = conditions
    smp = m.sampler()
    B = 2
    x, fm = m.canvas_init(B)
    kv = smp.cond_kv(ct[:B].contiguous(), cp[:B].contiguous())
    _same(smp, x, fm, kv, "reveal", loop="reveal")
    nt, npm = m._null_conditions(texts[:B], None, 1), m._null_conditions(proms[:B], None, 2)
    ct2, cp2 = m.encode_conditions(list(texts[:B]) + nt, list(proms[:B]) + npm)
    kv2 = smp.cond_kv(ct2, cp2)
    _same(smp, _half_revealed(x, 5), fm, kv2, "guided", guidance=1.5)


def test_default_loop_launches_one_projection_less_per_iteration(conditions):
    """The library's launch counter brackets the iterations with t % 16 == 0 -- here t = 32, whose rows the sampler launch of t = 33
    prepared: ln_fold = 2 runs one GEMM launch more in it than the default, the QKV projection of block 0."""
    from vall_e.vall_e import _hip
    m, _, _, ct, cp = conditions
    smp = m.sampler()
    B = 2
    kv = smp.cond_kv(ct[:B].contiguous(), cp[:B].contiguous())
    x0, fm = m.canvas_init(B)
    counts = {}
    try:
        for ln_fold in (1, 2):
            _hip.prof_enable(_hip.K_GEMM, 256)
            _run(smp, x0, fm, kv, ln_fold)
            torch.cuda.synchronize()
            counts[ln_fold] = _hip.prof_read_class(_hip.K_GEMM)[0]
    finally:
        _hip.prof_disable()
    assert counts[1] > 0 and counts[2] - counts[1] == 1, counts

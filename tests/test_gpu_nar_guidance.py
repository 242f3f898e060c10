"""Classifier-free guidance in the NAR stage's level draw on the GPU (include/d3pm_hip.h: d3pm_nar_level_guided,
d3pm_op_nar_draw_guided; csrc/d3pm_nar_draw.hip) and the cond_drop hook of NAR.forward_backward.

  1. draw entry (f16 / bf16 / fp32; tests/nar_guidance_ref.py: 12 frames over 2 pairs, the two rows of a frame at different offsets,
     one frame cut by each half): d3pm_op_nar_draw_guided equals d3pm_op_nar_draw on the host-combined z stored in T, id for id,
     theta_out and logprob_out bit for bit -- without a cut, with top_k = 5 / top_p = 0.9, greedy, and with a known map; on the crafted
     rows the guided id is neither half's argmax; w = 0 and c == u give the ids of the conditioned half; the id lands in both halves of
     resp and a skipped frame writes nothing; logprob_out within 1.0e-4 of the fp64 log-softmax of z (the project's bound for the
     routine, tests/test_gpu_nar_draw.py case 5; measured 3.5e-7 at worst, in f16);
  2. level entry: d3pm_nar_level_guided = d3pm_nar_level on the same 2 B grids with logits_out + d3pm_op_nar_draw_guided;
  3. end to end (bf16, d = 512, where a NAR evaluation does not depend on the batch bit for bit): NAR.forward(guidance=);
  4. training (fp32, d = 128): forward_backward(cond_drop=) against the step on explicitly empty conditions and fp64 autograd
     (the rule of tests/test_gpu_nar_train.py: 2e-4 * scale + 1e-7, the loss within 1e-4).

The numbers measured on the GPU go to util.REPORT."""
import functools
import json

import numpy as np
import pytest
import torch

import guidance_ref as G
import nar_guidance_ref as R
import nar_train_ref as TR
from test_gpu_nar import build
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
TAG = dict(zip(DTYPES, IDS))
RESP_POISON, LP_POISON, THETA_POISON, HELD = -5, 777.0, 555.0, 4097
LOGPROB_TOL = 1.0e-4
T = 0.2
SEED, UTT0, LEVEL = 23, 3, 2
B, TR_MAX, K = R.BATCH, R.TR_MAX, R.N_TOKENS


def _lens(n):
    return torch.tensor(R.LENS[:n], dtype=torch.int32, device=DEV)


def _outputs(n, known, held):
    resp0 = torch.full((n, TR_MAX, 8), RESP_POISON, dtype=torch.int32)
    if known is not None:
        for half in range(n // B):
            col = resp0[half * B: (half + 1) * B, :, LEVEL + 1]
            col[:] = torch.where(known, held, col)
    lp = torch.full((B, TR_MAX, 7), LP_POISON, dtype=torch.float32, device=DEV)
    th = torch.full((B, TR_MAX), THETA_POISON, dtype=torch.float32, device=DEV)
    return resp0, resp0.to(DEV), lp, th


def _guided(grid, w, *, greedy=False, top_k=0, top_p=1.0, known=None, held=None, theta=False):
    """d3pm_op_nar_draw_guided on the 2 B grids -> (resp int32 [2 B, TR_MAX, 8] on the host, its poisoned start, logprob [B, TR_MAX],
    theta [B, TR_MAX] or None); asserts that nothing outside column LEVEL + 1 / LEVEL was written."""
    from vall_e.vall_e import _hip
    resp0, resp, lp, th = _outputs(2 * B, known, held)
    _hip.op_nar_draw_guided(grid[..., :K], _lens(2 * B), resp, LEVEL, T, SEED, w, utt0=UTT0, flags=_hip.FLAG_GREEDY if greedy else 0,
                            top_k=top_k, top_p=top_p, known=None if known is None else known.to(torch.uint8).to(DEV), logprob_out=lp,
                            theta_out=th if theta else None)
    torch.cuda.synchronize()
    resp, lp = resp.cpu(), lp.cpu()
    rest = resp.clone()
    rest[:, :, LEVEL + 1] = resp0[:, :, LEVEL + 1]
    assert torch.equal(rest, resp0), "resp changed outside the level's column"
    rest = lp.clone()
    rest[:, :, LEVEL] = LP_POISON
    assert bool((rest == LP_POISON).all()), "logprob_out changed outside the level's column"
    return resp, resp0, lp[:, :, LEVEL], th.cpu() if theta else None


def _plain(grid, *, greedy=False, top_k=0, top_p=1.0, known=None, held=None, theta=False):
    """d3pm_op_nar_draw on B utterances of the conditioned half's layout -> (ids [B, TR_MAX], logprob [B, TR_MAX], theta or None)."""
    from vall_e.vall_e import _hip
    _, resp, lp, th = _outputs(B, known, held)
    _hip.op_nar_draw(grid[..., :K], _lens(B), resp, LEVEL, T, SEED, utt0=UTT0, flags=_hip.FLAG_GREEDY if greedy else 0, top_k=top_k,
                     top_p=top_p, known=None if known is None else known.to(torch.uint8).to(DEV), logprob_out=lp,
                     theta_out=th if theta else None)
    torch.cuda.synchronize()
    return resp.cpu()[:, :, LEVEL + 1], lp.cpu()[:, :, LEVEL], th.cpu() if theta else None


def _bits(x):
    return x.contiguous().view(torch.int32)


# ---- 1. the draw entry -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_guided_draw_is_the_plain_draw_on_the_host_combined_rows(built_lib, dtype):
    c, u = R.rows(dtype)
    live = R.frames_mask()
    grid = R.grid(dtype, c, u).to(DEV)
    known = (torch.arange(TR_MAX) % 3 == 1)[None].expand(B, TR_MAX).contiguous()
    held = torch.full((B, TR_MAX), HELD, dtype=torch.int32)
    crafted = np.arange(R.N_LIVE) % 4 != 3
    worst = 0.0
    for w in R.WEIGHTS:
        assert G.exact(c, u, w).all() and G.exact_rational(c, u, w), "the host reference is exact on these inputs"
        z = R.combine(c, u, w, dtype)
        zgrid = R.plain_grid(dtype, z).to(DEV)
        ref_lp = R.log_softmax64(z)
        cases = (dict(), dict(top_k=5, top_p=0.9, theta=True), dict(greedy=True), dict(greedy=True, top_k=5, top_p=0.9, theta=True),
                 dict(known=known, held=held), dict(known=known, held=held, top_k=5, top_p=0.9, theta=True))
        for kw in cases:
            resp, resp0, lp, th = _guided(grid, w, **kw)
            want_ids, want_lp, want_th = _plain(zgrid, **kw)
            got = resp[:B, :, LEVEL + 1]
            bad = (got[live] != want_ids[live]).nonzero().reshape(-1)
            assert bad.numel() == 0, f"w {w} {kw.keys()}: {bad.numel()} ids differ, got {got[live][bad].tolist()} want {want_ids[live][bad].tolist()}"
            assert torch.equal(resp[B:, :, LEVEL + 1][live], got[live]), "the id lands in both halves of resp"
            assert torch.equal(_bits(lp[live]), _bits(want_lp[live])), f"w {w} {kw.keys()}: logprob_out differs"
            if th is not None:
                assert torch.equal(_bits(th[live]), _bits(want_th[live])), f"w {w} {kw.keys()}: theta_out differs"
                assert bool((th[~live] == THETA_POISON).all())
            # a skipped frame (outside the response, or either row outside the grid) writes nothing, in either half
            for half in (resp[:B], resp[B:]):
                assert bool((half[:, :, LEVEL + 1][~live] == resp0[:B, :, LEVEL + 1][~live]).all()), "a skipped frame was written"
            assert bool((lp[~live] == LP_POISON).all())
            ids = got[live].long().numpy()
            if "known" in kw:
                k = known[live].numpy()
                assert (ids[k] == HELD).all() and (ids[~k] != RESP_POISON).all()
                if th is not None:
                    assert np.array_equal(np.isnan(th[live].numpy()), k)
            else:
                assert (ids >= 0).all() and (ids < K).all()
                err = float(np.abs(lp[live].double().numpy() - ref_lp[np.arange(R.N_LIVE), ids]).max())
                worst = max(worst, err)
                print(f"guided logprob {TAG[dtype]} w={w} {sorted(kw)}: max |device - float64| = {err:.3e}")
                assert err <= LOGPROB_TOL, (w, kw, err)
            if kw == dict(greedy=True):
                # greedy without a cut: the argmax of z, which on the crafted rows is neither half's
                assert np.array_equal(ids, z.argmax(-1))
                assert (ids[crafted] != c.argmax(-1)[crafted]).all() and (ids[crafted] != u.argmax(-1)[crafted]).all()
    REPORT[f"nar_guidance_logprob_{TAG[dtype]}"] = {"max_abs_err_vs_float64": worst, "bound": LOGPROB_TOL}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_weight_zero_and_equal_halves_draw_from_the_conditioned_half(built_lib, dtype):
    c, u = R.rows(dtype)
    live = R.frames_mask()
    cond = R.plain_grid(dtype, c).to(DEV)
    for kw in (dict(), dict(greedy=True), dict(top_k=5, top_p=0.9, theta=True)):
        want_ids, want_lp, want_th = _plain(cond, **kw)
        runs = [(R.grid(dtype, c, u).to(DEV), 0.0)] + [(R.grid(dtype, c, c).to(DEV), w) for w in (0.5, 1.5, 3.0, 0.7, 11.3)]
        for grid, w in runs:
            resp, _, lp, th = _guided(grid, w, **kw)
            assert torch.equal(resp[:B, :, LEVEL + 1][live], want_ids[live]), (w, kw)
            assert torch.equal(resp[B:, :, LEVEL + 1][live], want_ids[live])
            assert torch.equal(_bits(lp[live]), _bits(want_lp[live])), (w, kw)
            if th is not None:
                assert torch.equal(_bits(th[live]), _bits(want_th[live]))
    # and a weight > 0 on halves that differ does move ids
    moved = _guided(R.grid(dtype, c, u).to(DEV), 1.5, greedy=True)[0][:B, :, LEVEL + 1][live]
    assert not torch.equal(moved, _plain(cond, greedy=True)[0][live])


# ---- 2. the level entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_level_entry_is_the_plain_level_followed_by_the_guided_draw(built_lib, dtype):
    from vall_e.vall_e import _hip, synth
    from vall_e.vall_e.nar import guidance_twins
    cfg, _, m = build(dtype)
    for level, n_lv in ((0, 1), (3, 4)):
        texts, proms, resps = synth.make_nar_inputs(3, 1, n_levels=n_lv)
        lens, text, prom, resp, t_max, lens_host = m._pack(*guidance_twins(texts, proms, resps))
        run = m.runner(t_max)
        Bn, tr_max = 3, resp.shape[1]
        g = _hip.Guidance(1.5)
        with torch.cuda.device(DEV):
            two = resp.clone()
            logits = run.level(lens, text, prom, two.clone(), t_max, level, T, 11, 2, 0, want_logits=True)
            lp_two, th_two = torch.zeros(Bn, tr_max, 7, device=DEV), torch.zeros(Bn, tr_max, device=DEV)
            _hip.op_nar_draw_guided(logits, lens, two, level, T, 11, 1.5, utt0=2, top_k=50, top_p=0.9, logprob_out=lp_two, theta_out=th_two)
            one, lp_one, th_one = resp.clone(), torch.zeros(Bn, tr_max, 7, device=DEV), torch.zeros(Bn, tr_max, device=DEV)
            draw = _hip.nar_draw_struct(50, _hip.nar_draw_options(50, 0.9)[1], None, lp_one, th_one)
            lg_one = run.level(lens, text, prom, one, t_max, level, T, 11, 2, 0, want_logits=True, draw=draw, guidance=g)
            # without options: the same kernel with no cut, against the draw entry without options
            bare, bare_two = resp.clone(), resp.clone()
            run.level(lens, text, prom, bare, t_max, level, T, 11, 2, 0, guidance=g)
            _hip.op_nar_draw_guided(logits, lens, bare_two, level, T, 11, 1.5, utt0=2)
        torch.cuda.synchronize()
        assert lg_one.shape == (6, t_max, cfg.n_tokens) and torch.equal(lg_one.view(torch.int16) if dtype != torch.float32 else _bits(lg_one),
                                                                         logits.view(torch.int16) if dtype != torch.float32 else _bits(logits))
        assert torch.equal(one, two), f"level {level}: {(one != two).sum().item()} ids differ"
        assert torch.equal(_bits(lp_one), _bits(lp_two)) and torch.equal(_bits(th_one), _bits(th_two))
        assert torch.equal(bare, bare_two) and torch.equal(one[:3], one[3:]) and torch.equal(bare[:3], bare[3:])
        assert not torch.equal(one[:, :, level + 1], resp[:, :, level + 1])
        for b, (_, _, tr) in enumerate(lens_host[:3]):
            assert bool(torch.isfinite(lp_one[b, :tr, level]).all()) and bool((lp_one[b, tr:] == 0).all())


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wide():
    from vall_e.vall_e import synth
    cfg, _, m = build(torch.bfloat16, synth.NARConfig(d_model=512, n_heads=8, n_layers=2))
    return m, synth.make_nar_inputs(3, 1)


@functools.lru_cache(maxsize=None)
def _wide_ids(guidance):
    m, (texts, proms, resps) = _wide()
    return m(texts, proms, resps, seed=11, guidance=guidance)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_twin_is_the_ordinary_call_on_the_empty_conditions(built_lib):
    m, (texts, proms, resps) = _wide()
    ids, logits, lens, t_max = m(texts, proms, resps, seed=11, guidance=1.5, return_logits_level=0)
    assert len(ids) == 3 and logits.shape[0] == 6 and lens.shape == (6, 3)
    assert lens[3:].tolist() == [[0, 0, len(r)] for r in resps]
    for b in range(3):
        _, alone, _, _ = m([texts[b][:0]], [proms[b][:0]], [resps[b]], seed=11, return_logits_level=0)
        tr = len(resps[b])
        assert torch.equal(logits[3 + b, 2: 2 + tr].view(torch.int16), alone[0, 2: 2 + tr].view(torch.int16)), f"twin {b}"
        _, cond, cl, _ = m([texts[b]], [proms[b]], [resps[b]], seed=11, return_logits_level=0)
        at = int(cl[0, 0] + cl[0, 1]) + 2
        assert torch.equal(logits[b, at: at + tr].view(torch.int16), cond[0, at: at + tr].view(torch.int16)), f"utterance {b}"
        assert not torch.equal(logits[b, at: at + tr], logits[3 + b, 2: 2 + tr])


def test_guidance_changes_the_ids_and_equal_twins_do_not(built_lib):
    m, (texts, proms, resps) = _wide()
    plain = m(texts, proms, resps, seed=11)
    guided = _wide_ids(1.5)
    assert all(g.shape == p.shape and g.dtype == torch.int64 for g, p in zip(guided, plain))
    assert all(torch.equal(g[:, 0], p[:, 0]) for g, p in zip(guided, plain)), "level 0 is the caller's"
    changed = [float((g[:, 1:] != p[:, 1:]).float().mean()) for g, p in zip(guided, _wide_ids(0.0))]
    print(f"guidance 1.5 against 0: share of ids of levels 1..7 that differ per utterance {changed}")
    assert all(c > 0.0 for c in changed), changed
    REPORT["nar_guidance_ids_changed_share"] = changed
    # the conditions themselves as the twins: c == u bit for bit, the ids of the call without guidance
    same = m(texts, proms, resps, seed=11, guidance=1.5, null_text_list=texts, null_proms_list=proms)
    assert _same(same, plain)


def test_guidance_zero_makes_the_launches_of_the_call_without_the_keyword(built_lib, monkeypatch):
    from vall_e.vall_e import _hip
    m, (texts, proms, resps) = _wide()
    seen = []
    level = _hip.NarRunner.level
    monkeypatch.setattr(_hip.NarRunner, "level",
                        lambda self, *a, **kw: (seen.append((a[0].shape[0], kw.get("draw"), kw.get("guidance"))), level(self, *a, **kw))[1])
    bare = m(texts, proms, resps, seed=11)
    zero = m(texts, proms, resps, seed=11, guidance=0.0, null_text_list=None, null_proms_list=None)
    assert _same(bare, zero)
    assert len(seen) == 14 and all(s == (3, None, None) for s in seen), "no twins are packed, no struct is made"
    m(texts, proms, resps, seed=11, guidance=1.5)
    assert len(seen) == 21 and all(n == 6 and d is None and g is not None for n, d, g in seen[14:])


def test_a_guided_batch_is_its_utterances_guided_alone(built_lib):
    m, (texts, proms, resps) = _wide()
    kw = dict(seed=11, guidance=1.5, top_k=50, top_p=0.9)
    batch, scores = m(texts, proms, resps, return_logprobs=True, **kw)
    for b in range(3):
        alone, s = m([texts[b]], [proms[b]], [resps[b]], utt0=b, return_logprobs=True, **kw)
        diff = int((alone[0] != batch[b]).sum())
        assert diff == 0, f"utterance {b}: {diff} ids differ alone vs inside the batch of 3"
        assert torch.equal(_bits(s[0]), _bits(scores[b])) and bool(torch.isfinite(s[0]).all()) and bool((s[0] <= 0).all())
    assert not _same(batch, _wide_ids(1.5)), "the cuts act on the guided row"
    assert _same(m(texts, proms, resps, seed=11, guidance=1.5, greedy=True), m(texts, proms, resps, seed=12, guidance=1.5, greedy=True))


def test_known_frames_come_back_in_all_levels_under_guidance(built_lib):
    m, (texts, proms, resps) = _wide()
    g = torch.Generator().manual_seed(5)
    known, mask = [], []
    for r in resps:
        k = torch.randint(0, 1024, (len(r), 8), generator=g)
        k[:, 0] = r[:, 0]
        known.append(k)
        mask.append(torch.arange(len(r)) < 5)
    out = m(texts, proms, resps, seed=11, guidance=1.5, known=known, known_mask=mask)
    free = _wide_ids(1.5)
    for b in range(3):
        assert torch.equal(out[b][:5].cpu(), known[b][:5]), f"utterance {b}: the prefix changed"
        assert torch.equal(out[b][:, 0].cpu(), resps[b][:, 0]) and not torch.equal(out[b][5:], free[b][5:])


def test_dp_helper_and_cli_pass_the_weight_through(built_lib, tmp_path):
    from vall_e import __main__ as cli, formats
    from vall_e.vall_e import AR, dp, get_model, synth
    cfg = synth.D3PMConfig.native()
    ar = AR.from_config(cfg)
    ar.load_state_dict(synth.make_state_dict(cfg, 0))
    ar = ar.half().to(DEV)
    _, _, nar = build(torch.float16)
    texts, proms = synth.make_inputs(cfg, 2, 1)
    codes = dp.generate_codes_dp(ar, nar, texts, proms, seed=5, steps=8, nar_kw=dict(guidance=1.5))
    lvl0 = ar.generate_audio(texts, proms, seed=5, steps=8)[:, : cfg.n_frames].clamp(max=1023)
    direct = nar(texts, proms, [lvl0[b].reshape(-1, 1) for b in range(2)], seed=5, utt0=0, guidance=1.5)
    assert all(torch.equal(codes[b], direct[b]) for b in range(2))
    plain = dp.generate_codes_dp(ar, nar, texts, proms, seed=5, steps=8)
    assert not torch.equal(plain, codes) and torch.equal(plain[..., 0], codes[..., 0])
    # a shard started at its global index: the null lists are cut with it
    tail = dp.generate_codes_dp(ar, nar, texts[1:], proms[1:], seed=5, steps=8,
                                nar_kw=dict(guidance=1.5, null_text_list=[t[:0] for t in texts[1:]], null_proms_list=[p[:0] for p in proms[1:]]),
                                ar_fn=lambda t, p, **k: ar.generate_audio(t, p, **{**k, "utt0": k["utt0"] + 1}),
                                nar_fn=lambda t, p, r, **k: nar(t, p, r, **{**k, "utt0": k["utt0"] + 1}))
    assert tail.shape == (1, cfg.n_frames, 8) and 0 <= tail.min() and tail.max() < 1024
    # the command line
    (tmp_path / "u.phn.txt").write_text("HH AH0 L OW1 _ W ER1 L D", encoding="utf8")
    symmap = formats.build_symmap([formats.read_phones(tmp_path / "u.phn.txt")])
    (tmp_path / "symmap.json").write_text(json.dumps(symmap), encoding="utf8")
    torch.save(torch.randint(0, 1024, (1, 8, 120), dtype=torch.int64), tmp_path / "prompt.qnt.pt")
    torch.manual_seed(1)
    torch.save(get_model("nar-quarter").state_dict(), tmp_path / "nar.pt")
    argv = [str(tmp_path / "out.qnt.pt"), "--phn-file", str(tmp_path / "u.phn.txt"), "--symmap", str(tmp_path / "symmap.json"),
            "--prompt-qnt", str(tmp_path / "prompt.qnt.pt"), "--native", "--seed", "5", "--nar-model", "nar-quarter",
            "--nar-ckpt", str(tmp_path / "nar.pt")]
    outs = []
    for extra in ([], ["--nar-guidance", "0"], ["--nar-guidance", "2"]):
        torch.manual_seed(0)
        cli.main(argv + extra)
        outs.append(torch.load(tmp_path / "out.qnt.pt"))
    assert all(o.shape == (1, 8, 350) and o.dtype == torch.int64 for o in outs)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2][:, 0], outs[0][:, 0]) and not torch.equal(outs[2], outs[0])
    assert 0 <= outs[2].min() and outs[2][:, 1:].max() < 1024


# ---- 4. the training hook -------------------------------------------------------------------------------------------------------------
LEVELS = (0, 3, 6)


def _train_model():
    from vall_e.vall_e import NAR, synth
    cfg = synth.NARConfig(d_model=128, n_heads=2, n_layers=2)
    m = NAR(cfg.n_tokens, cfg.d_model, cfg.n_heads, cfg.n_layers)
    m.load_state_dict(synth.make_nar_state_dict(cfg, 0))
    return cfg, m.float().to(DEV)


@functools.lru_cache(maxsize=None)
def _train_inputs():
    from vall_e.vall_e import synth
    return synth.make_nar_inputs(3, 1, n_levels=8)


def _step(texts, proms, resps, **kw):
    cfg, m = _train_model()
    loss = m.forward_backward(texts, proms, resps, seed=5, utt0=2, quant_levels=list(LEVELS), **kw)
    return loss, {n: p.grad.clone() for n, p in m.named_parameters()}


def _identical(a, b):
    (la, ga), (lb, gb) = a, b
    return torch.equal(la, lb) and sorted(ga) == sorted(gb) and all(torch.equal(ga[n], gb[n]) for n in ga)


def test_cond_drop_zero_is_the_step_and_one_is_the_step_on_empty_conditions(built_lib):
    t, p, r = _train_inputs()
    base = _step(t, p, r)
    for off in (0, 0.0, False, None, (0.0, 0.0)):
        assert _identical(_step(t, p, r, cond_drop=off), base), off
    empty_t, empty_p = [x[:0] for x in t], [x[:0] for x in p]
    both = _step(empty_t, empty_p, r)
    assert _identical(_step(t, p, r, cond_drop=(1.0, 1.0)), both) and _identical(_step(t, p, r, cond_drop=1), both)
    assert _identical(_step(t, p, r, cond_drop=(1.0, 0.0)), _step(empty_t, p, r))
    assert _identical(_step(t, p, r, cond_drop=(0.0, 1.0)), _step(t, empty_p, r))
    assert not torch.equal(both[0], base[0])


def test_cond_drop_decides_as_the_mirror_on_the_device(built_lib):
    from vall_e.vall_e import nar
    t, p, r = _train_inputs()
    seed, utt0, probs = 5, 2, (0.5, 0.5)
    for seed in (5, 6, 7, 8):
        _, _, dropped = nar.cond_drop_lists(t, p, seed, utt0, probs, DEV)
        assert dropped == [G.cond_drop_mirror(seed, utt0 + b, *probs) for b in range(3)], seed
    decisions = [G.cond_drop_mirror(7, utt0 + b, *probs) for b in range(3)]
    cfg, m = _train_model()
    loss = m.forward_backward(t, p, r, seed=7, utt0=utt0, quant_levels=list(LEVELS), cond_drop=probs)
    want = _step([x[:0] if d[0] else x for x, d in zip(t, decisions)], [x[:0] if d[1] else x for x, d in zip(p, decisions)], r)
    assert torch.equal(loss, want[0]) and all(torch.equal(prm.grad, want[1][n]) for n, prm in m.named_parameters())


@pytest.mark.parametrize("which", ["text", "prompt", "both"])
def test_step_on_empty_conditions_matches_fp64_autograd(built_lib, which):
    from vall_e.vall_e import synth
    cfg, m = _train_model()
    t, p, r = _train_inputs()
    if which in ("text", "both"):
        t = [x[:0] for x in t]
    if which in ("prompt", "both"):
        p = [x[:0] for x in p]
    ref_loss, ref = TR.loss_and_grads(synth.make_nar_state_dict(cfg, 0), cfg.n_heads, cfg.n_layers, t, p, r, list(LEVELS), dtype=torch.float64)
    loss = m.forward_backward(t, p, r, seed=5, quant_levels=list(LEVELS))
    print(f"empty {which}: loss {float(loss):.6f} against fp64 autograd {ref_loss:.6f}")
    assert abs(float(loss) - ref_loss) <= 1e-4, (float(loss), ref_loss)
    worst = {}
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(ref)
    for name, prm in params.items():
        want = ref[name].double()
        err = (prm.grad.detach().cpu().double() - want).abs().max().item()
        scale = want.abs().max().item()
        worst[name] = err / max(scale, 1e-30)
        assert err <= 2e-4 * scale + 1e-7, f"empty {which}: {name}: max |error| {err:.3e} vs scale {scale:.3e}"
    if which in ("text", "both"):
        assert float(m.text_emb.weight.grad.abs().max()) == 0.0, "text_emb receives exactly 0 when the text is dropped"
    if which in ("prompt", "both"):
        assert float(m.proms_emb.weight.grad.abs().max()) == 0.0
    REPORT[f"nar_cond_drop_step_empty_{which}"] = {"loss_hip": float(loss), "loss_autograd": ref_loss, "worst_relative_error": max(worst.values()),
                                                    "worst_tensor": max(worst, key=worst.get)}

"""The options of the NAR stage's level draw above the kernel (tests/test_gpu_nar_draw.py holds the kernel): d3pm_nar_level_draw,
NAR.forward(top_k=, top_p=, known=, known_mask=, return_logprobs=), dp.generate_codes_dp(nar_kw=) and the command line, on the small
model of tests/test_gpu_nar.py (d = 128, 2 heads, 2 layers)."""
import json

import numpy as np
import pytest
import torch

import nar_draw_ref as R
from test_gpu_nar import DEV, build

pytestmark = pytest.mark.gpu
LOGPROB_TOL = 1.0e-4          # the bound of tests/test_gpu_nar_draw.py case 5 and of tests/test_gpu_logprob.py
T = 0.2


def _rows(logits, lens, b):
    tt, tp, tr = (int(v) for v in lens[b])
    return logits[b, tt + tp + 2: tt + tp + 2 + tr].cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_level_entry_is_the_plain_level_followed_by_the_draw_entry(built_lib, dtype):
    from vall_e.vall_e import _hip, synth
    cfg, _, m = build(dtype)
    for level, n_lv in ((0, 1), (3, 4)):
        texts, proms, resps = synth.make_nar_inputs(3, 1, n_levels=n_lv)
        lens, text, prom, resp, t_max, lens_host = m._pack(texts, proms, resps)
        run = m.runner(t_max)
        Bn, tr_max = resp.shape[0], resp.shape[1]
        held = (torch.arange(tr_max, device=DEV) % 4 == 1).to(torch.uint8)[None].expand(Bn, tr_max).contiguous()
        resp[:, :, level + 1] = torch.where(held.bool(), torch.full_like(resp[:, :, level + 1], 7), resp[:, :, level + 1])
        with torch.cuda.device(DEV):
            logits = run.level(lens, text, prom, resp.clone(), t_max, level, T, 11, 2, 0, want_logits=True)
            two, lp_two, th_two = resp.clone(), torch.zeros(Bn, tr_max, 7, device=DEV), torch.zeros(Bn, tr_max, device=DEV)
            _hip.op_nar_draw(logits, lens, two, level, T, 11, utt0=2, top_k=50, top_p=0.9, known=held, logprob_out=lp_two, theta_out=th_two)
            one, lp_one, th_one = resp.clone(), torch.zeros(Bn, tr_max, 7, device=DEV), torch.zeros(Bn, tr_max, device=DEV)
            draw = _hip.nar_draw_struct(50, _hip.nar_draw_options(50, 0.9)[1], held, lp_one, th_one)
            run.level(lens, text, prom, one, t_max, level, T, 11, 2, 0, draw=draw)
            # a neutral struct through the new entry is the plain level
            plain, neutral = resp.clone(), resp.clone()
            run.level(lens, text, prom, plain, t_max, level, T, 11, 2, 0)
            check = _hip.check
            check(_hip.lib().d3pm_nar_level_draw(run.shape, run.weights, Bn, t_max, lens.data_ptr(), text.data_ptr(), text.shape[1], prom.data_ptr(),
                                                 prom.shape[1], neutral.data_ptr(), tr_max, level, T, 11, 2, 0, run._ws.data_ptr(), run._ws.numel(),
                                                 None, _hip.NarDraw(1.0, 0, None, None, None), _hip.stream_ptr()), "d3pm_nar_level_draw")
        torch.cuda.synchronize()
        assert torch.equal(one, two), f"level {level}: {(one != two).sum().item()} ids differ"
        assert torch.equal(lp_one.view(torch.int32), lp_two.view(torch.int32)) and torch.equal(th_one.view(torch.int32), th_two.view(torch.int32))
        assert torch.equal(neutral, plain)
        assert bool((one[:, :, level + 1][held.bool()] == 7).all()) and not torch.equal(one, plain)
        for b, (_, _, tr) in enumerate(lens_host):
            assert bool(torch.isfinite(lp_one[b, :tr, level]).all()) and bool((lp_one[b, tr:] == 0).all())


def test_default_options_are_the_call_without_keywords(built_lib, monkeypatch):
    from vall_e.vall_e import _hip, synth
    cfg, _, m = build(torch.bfloat16)
    texts, proms, resps = synth.make_nar_inputs(2, 1)
    seen = []
    level = _hip.NarRunner.level
    monkeypatch.setattr(_hip.NarRunner, "level", lambda self, *a, **kw: (seen.append(kw.get("draw")), level(self, *a, **kw))[1])
    bare = m(texts, proms, resps, seed=11)
    dflt = m(texts, proms, resps, seed=11, top_k=0, top_p=1.0, known=None, known_mask=None, return_logprobs=False)
    assert all(torch.equal(a, b) for a, b in zip(bare, dflt))
    assert len(seen) == 14 and all(d is None for d in seen)          # no struct: the entry and the kernel that know nothing of the options
    opt = m(texts, proms, resps, seed=11, top_k=1024)                    # the widest top_k cuts nothing, through the other kernel
    assert all(torch.equal(a, b) for a, b in zip(bare, opt)) and all(d is not None for d in seen[14:])


def test_a_known_recording_comes_back_and_is_scored_level_by_level(built_lib):
    from vall_e.vall_e import synth
    cfg, _, m = build(torch.bfloat16)
    texts, proms, codes = synth.make_nar_inputs(2, 3, n_levels=8)
    lvl0 = [c[:, :1] for c in codes]
    mask = [torch.ones(len(c), dtype=torch.bool) for c in codes]
    out, scores = m(texts, proms, lvl0, seed=4, known=codes, known_mask=mask, return_logprobs=True)
    worst = 0.0
    for b in range(2):
        assert torch.equal(out[b].cpu(), codes[b]) and scores[b].shape == (len(codes[b]), 7) and scores[b].dtype == torch.float32
    for l in range(7):
        out_l, logits, lens, t_max, scores_l = m(texts, proms, lvl0, seed=4, known=codes, known_mask=mask, return_logprobs=True,
                                                 return_logits_level=l)
        for b in range(2):
            assert torch.equal(scores_l[b], scores[b]) and torch.equal(out_l[b].cpu(), codes[b])
            ref = R.log_softmax64(_rows(logits, lens, b))[np.arange(len(codes[b])), codes[b][:, l + 1].numpy()]
            err = float(np.abs(scores[b][:, l].cpu().double().numpy() - ref).max())
            worst = max(worst, err)
            assert err <= LOGPROB_TOL, (l, b, err)
    print(f"teacher-forced log-probabilities: max |device - float64| = {worst:.3e}")
    # given levels hold 0: the same recording with levels 0..2 given
    out3, scores3 = m(texts, proms, [c[:, :3] for c in codes], seed=4, known=codes, known_mask=mask, return_logprobs=True)
    for b in range(2):
        assert torch.equal(out3[b].cpu(), codes[b]) and bool((scores3[b][:, :2] == 0).all())
        assert torch.equal(scores3[b][:, 2:], scores[b][:, 2:])


def test_a_known_prefix_keeps_all_its_levels_in_any_batch(built_lib):
    from vall_e.vall_e import synth
    cfg, _, m = build(torch.bfloat16)
    texts, proms, resps = synth.make_nar_inputs(3, 2)
    g = torch.Generator().manual_seed(5)
    known, mask = [], []
    for r in resps:
        k = torch.randint(0, 1024, (len(r), 8), generator=g)
        k[:, 0] = r[:, 0]
        known.append(k)
        mask.append(torch.arange(len(r)) < 5)
    kw = dict(seed=9, top_k=50, top_p=0.9)
    batch = m(texts, proms, resps, known=known, known_mask=mask, **kw)
    free = m(texts, proms, resps, **kw)
    for b in range(3):
        assert torch.equal(batch[b][:5].cpu(), known[b][:5]), f"utterance {b}: the prefix changed"
        assert torch.equal(batch[b][:, 0].cpu(), resps[b][:, 0])
        assert not torch.equal(batch[b][5:], free[b][5:])              # the later frames are conditioned on the prefix
        alone = m([texts[b]], [proms[b]], [resps[b]], known=[known[b]], known_mask=[mask[b]], utt0=b, **kw)
        diff = int((alone[0] != batch[b]).sum())
        print(f"utterance {b}: {diff} ids differ alone vs inside the batch of 3")
        assert diff == 0


def test_top_k_one_under_noise_is_the_greedy_draw(built_lib):
    """top_k = 1 keeps the classes tied at the maximum of rn(logit / T): where no row has a tie the Gumbel draw has one candidate and
    equals greedy.  The rows of the greedy run are checked for ties on the host (fp32 logits: none at this seed)."""
    from vall_e.vall_e import synth
    cfg, _, m = build(torch.float32)
    texts, proms, resps = synth.make_nar_inputs(2, 1)
    greedy = m(texts, proms, resps, sampling_temperature=T, greedy=True)
    for l in range(7):
        ids, logits, lens, t_max = m(texts, proms, resps, sampling_temperature=T, greedy=True, return_logits_level=l)
        assert all(torch.equal(a, b) for a, b in zip(ids, greedy))
        for b in range(2):
            v = R.values(_rows(logits, lens, b), T)
            assert bool(((v == v.max(-1, keepdim=True).values).sum(-1) == 1).all()), f"level {l} utterance {b}: a tied maximum, choose another seed"
    noisy = m(texts, proms, resps, sampling_temperature=T, seed=21, top_k=1)
    assert all(torch.equal(a, b) for a, b in zip(noisy, greedy))
    assert not all(torch.equal(a, b) for a, b in zip(m(texts, proms, resps, sampling_temperature=T, seed=21), greedy))


def test_dp_helper_passes_the_options_through(built_lib):
    from vall_e.vall_e import AR, dp, synth
    cfg = synth.D3PMConfig.native()
    ar = AR.from_config(cfg)
    ar.load_state_dict(synth.make_state_dict(cfg, 0))
    ar = ar.half().to(DEV)
    _, _, nar = build(torch.float16)
    texts, proms = synth.make_inputs(cfg, 3, 1)
    g = torch.Generator().manual_seed(6)
    known = [torch.randint(0, 1024, (cfg.n_frames, 8), generator=g) for _ in range(3)]
    mask = [torch.arange(cfg.n_frames) < 10 * (b + 1) for b in range(3)]
    nar_kw = dict(top_k=50, top_p=0.9, known=known, known_mask=mask, sampling_temperature=0.5)
    codes = dp.generate_codes_dp(ar, nar, texts, proms, seed=5, steps=8, nar_kw=nar_kw)
    assert codes.shape == (3, cfg.n_frames, 8)
    lvl0 = ar.generate_audio(texts, proms, seed=5, steps=8)[:, : cfg.n_frames].clamp(max=1023)
    direct = nar(texts, proms, [lvl0[b].reshape(-1, 1) for b in range(3)], seed=5, utt0=0, **nar_kw)
    for b in range(3):
        assert torch.equal(codes[b], direct[b])
        n = 10 * (b + 1)
        assert torch.equal(codes[b, :n, 1:].cpu(), known[b][:n, 1:]) and torch.equal(codes[b, :, 0], lvl0[b])
    plain = dp.generate_codes_dp(ar, nar, texts, proms, seed=5, steps=8)
    assert not torch.equal(plain, codes) and torch.equal(plain[..., 0], codes[..., 0])
    # a shard started at its global index: the per-utterance lists are cut with it
    tail = dp.generate_codes_dp(ar, nar, texts[1:], proms[1:], seed=5, steps=8, nar_kw=dict(nar_kw, known=known[1:], known_mask=mask[1:]),
                                ar_fn=lambda t, p, **k: ar.generate_audio(t, p, **{**k, "utt0": k["utt0"] + 1}),
                                nar_fn=lambda t, p, r, **k: nar(t, p, r, **{**k, "utt0": k["utt0"] + 1}))
    assert tail.shape == (2, cfg.n_frames, 8)
    for b in range(2):
        n = 10 * (b + 2)
        assert torch.equal(tail[b, :n, 1:].cpu(), known[b + 1][:n, 1:])


def test_cli_keeps_the_prefix_levels_and_saves_the_nar_logprobs(built_lib, tmp_path):
    from vall_e import __main__ as cli, formats
    from vall_e.vall_e import get_model
    (tmp_path / "u.phn.txt").write_text("HH AH0 L OW1 _ W ER1 L D", encoding="utf8")
    symmap = formats.build_symmap([formats.read_phones(tmp_path / "u.phn.txt")])
    (tmp_path / "symmap.json").write_text(json.dumps(symmap), encoding="utf8")
    torch.save(torch.randint(0, 1024, (1, 8, 120), dtype=torch.int64), tmp_path / "prompt.qnt.pt")
    X = torch.randint(0, 1024, (1, 8, 40), dtype=torch.int64, generator=torch.Generator().manual_seed(3))
    torch.save(X, tmp_path / "x.qnt.pt")
    torch.manual_seed(1)
    torch.save(get_model("nar-quarter").state_dict(), tmp_path / "nar.pt")
    argv = [str(tmp_path / "out.qnt.pt"), "--phn-file", str(tmp_path / "u.phn.txt"), "--symmap", str(tmp_path / "symmap.json"),
            "--prompt-qnt", str(tmp_path / "prompt.qnt.pt"), "--native", "--seed", "5", "--nar-model", "nar-quarter",
            "--nar-ckpt", str(tmp_path / "nar.pt"), "--continue-from", str(tmp_path / "x.qnt.pt")]
    torch.manual_seed(0)
    cli.main(argv)                                                   # as it always was: level 0 of the prefix alone survives
    old = torch.load(tmp_path / "out.qnt.pt")
    assert old.shape == (1, 8, 350) and torch.equal(old[0, 0, :40], X[0, 0]) and not torch.equal(old[0, :, :40], X[0])
    torch.manual_seed(0)
    cli.main(argv + ["--keep-prefix-levels", "--nar-logprobs", str(tmp_path / "lp.pt"), "--nar-top-k", "50", "--nar-top-p", "0.9"])
    new = torch.load(tmp_path / "out.qnt.pt")
    assert new.shape == (1, 8, 350) and new.dtype == torch.int64
    assert torch.equal(new[0, :, :40], X[0]), "the prefix lost a level"
    assert torch.equal(new[:, 0], old[:, 0]) and 0 <= new.min() and new.max() < 1024
    lp = torch.load(tmp_path / "lp.pt")
    assert lp.shape == (350, 7) and lp.dtype == torch.float32 and bool(torch.isfinite(lp).all()) and bool((lp < 0).all())
    with pytest.raises(SystemExit):
        cli.main(argv[:-2] + ["--keep-prefix-levels"])                # needs --continue-from

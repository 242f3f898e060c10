"""NAR training step on the GPU (vall_e/vall_e/nar_train.py, csrc/d3pm_nar_train.hip): the three new kernels one at a time against
fp64 autograd, then NAR.forward_backward / NAR.forward against fp64 autograd over the test reference (tests/nar_train_ref.py, pinned
to the reference's own NAR by tests/golden/nar_train_grads.npz).  Model: NARConfig(d_model=128, n_heads=2, n_layers=2) with
synth.make_nar_state_dict weights, three ragged utterances of synth.make_nar_inputs(3, 1, n_levels=8).

Bounds: a gradient or kernel output is within 2e-4 of its tensor's maximum + 1e-7 of fp64 autograd, the project's bound for its
fp32 backward kernels (tests/test_gpu_train.py); the loss within 1e-4; the fixture's samples within 5e-4 of scale."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nar_train_ref as R
from oracle import nar_oracle as N
from util import REPORT, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = (0, 3, 6)


def close(got, want, what):
    """2e-4 of the output's maximum + 1e-7; returns the error relative to that maximum."""
    want = want.double()
    err = (got.detach().cpu().double() - want).abs().max().item()
    scale = want.abs().max().item()
    assert err <= 2e-4 * scale + 1e-7, f"{what}: max |error| {err:.3e} vs scale {scale:.3e}"
    return err / max(scale, 1e-30)


def build():
    from vall_e.vall_e import NAR, synth
    cfg = synth.NARConfig(d_model=128, n_heads=2, n_layers=2)
    sd32 = synth.make_nar_state_dict(cfg, 0)
    m = NAR(cfg.n_tokens, cfg.d_model, cfg.n_heads, cfg.n_layers)
    m.load_state_dict(sd32)
    return cfg, sd32, m.float().to(DEV)


@functools.lru_cache(maxsize=None)
def inputs():
    from vall_e.vall_e import synth
    return synth.make_nar_inputs(3, 1, n_levels=8)


@functools.lru_cache(maxsize=None)
def reference(levels=LEVELS, only=None, drop=None):
    """(loss, grads) in fp64 on the CPU, computed once per case and shared: `only` = one utterance alone, drop = (seed, utt0, p)."""
    from vall_e.vall_e import synth
    cfg = synth.NARConfig(d_model=128, n_heads=2, n_layers=2)
    t, p, r = inputs()
    idx = range(3) if only is None else [only]
    t, p, r, lv = [t[b] for b in idx], [p[b] for b in idx], [r[b] for b in idx], [levels[b] for b in idx]
    masks = None
    if drop is not None:
        masks = dropout_masks(cfg, t, p, r, *drop)
    return R.loss_and_grads(synth.make_nar_state_dict(cfg, 0), cfg.n_heads, cfg.n_layers, t, p, r, lv, masks=masks, dtype=torch.float64)


def dropout_masks(cfg, t, p, r, seed, utt0, prob):
    import dropout_mirror as DM
    from vall_e.vall_e.nar_train import dropout_site
    masks = {}
    for b in range(len(t)):
        total = len(t[b]) + len(p[b]) + len(r[b]) + 2
        for layer in range(cfg.n_layers):
            for kind, width in ((0, cfg.d_model), (1, 4 * cfg.d_model), (2, cfg.d_model)):
                masks[(b, layer, kind)] = DM.z(seed, utt0 + b, dropout_site(layer, kind), (total, width), prob)
    return masks


def check_grads(m, want, what):
    worst = {}
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(want) and len(params) == 24
    for name, prm in params.items():
        assert prm.grad is not None and prm.grad.dtype == torch.float32, name
        worst[name] = close(prm.grad, want[name], f"{what}: {name}")
    return worst


# ---- 1. AdaLN backward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("d", [128, 100, 320])      # one kernel pair for every width: a multiple of the wave, a ragged one, and one wider
def test_adaln_bwd_matches_autograd_of_the_detached_form(built_lib, d, accumulate):      # than the column kernel's 256-column tile
    from vall_e.vall_e import nar_train as NT
    M = 37
    g = torch.Generator().manual_seed(d)
    x = torch.randn(M, d, generator=g) * 1.5 + 0.3
    dy = torch.randn(M, d, generator=g)
    emb = 0.3 * torch.randn(2 * d, generator=g)
    mask = torch.ones(M, dtype=torch.uint8)
    mask[torch.randperm(M, generator=g)[:9]] = 0
    dx0, demb0 = torch.randn(M, d, generator=g), torch.randn(2 * d, generator=g)

    x64, emb64 = x.double().requires_grad_(True), emb.double().requires_grad_(True)
    h = F.layer_norm(x64, (d,), eps=1e-5)
    y = emb64[:d].exp() * (2 * (1 - (0.1 * h).detach()) * h) + emb64[d:]
    (y * mask[:, None].double() * dy.double()).sum().backward()
    want_dx = x64.grad + (dx0.double() if accumulate else 0)
    want_demb = emb64.grad + demb0.double()

    def run(xx, gg):
        dx, demb = dx0.clone().to(DEV), demb0.clone().to(DEV)
        NT.adaln_bwd(xx.to(DEV), gg.to(DEV), emb.to(DEV), mask.to(DEV), dx, demb, accumulate=accumulate)
        return dx.cpu(), demb.cpu()

    dx, demb = run(x, dy)
    e1, e2 = close(dx, want_dx, "dx"), close(demb, want_demb, "demb_row")
    dead = mask == 0
    assert torch.equal(dx[dead], dx0[dead] if accumulate else torch.zeros_like(dx0[dead])), "a masked row gets 0, or keeps what it had"
    xp, dyp = x.clone(), dy.clone()
    xp[dead], dyp[dead] = 1e30, 1e30
    dx_p, demb_p = run(xp, dyp)
    assert torch.equal(dx_p, dx) and torch.equal(demb_p, demb), "a masked row is not read"
    REPORT[f"nar_train_adaln_bwd_d{d}_acc{int(accumulate)}"] = {"dx": e1, "demb_row": e2}


# ---- 2. input-assembly backward -----------------------------------------------------------------------------------------------------------
def _assembly_case(d=128, n_tokens=50):
    g = torch.Generator().manual_seed(3)
    lens_host = [(6, 9, 11), (9, 5, 14), (4, 12, 7)]
    text = [torch.randint(0, n_tokens, (a,), generator=g) for a, _, _ in lens_host]
    prom = [torch.randint(0, n_tokens, (b_, 8), generator=g) for _, b_, _ in lens_host]
    resp = [torch.randint(0, n_tokens, (c, 8), generator=g) for _, _, c in lens_host]
    text[1][:] = 7                                   # the same phoneme in every position
    resp[1][:, :] = 11                               # the same code in every frame and level
    prom[1][2:6] = prom[1][0]                        # repeated prompt frames
    absent = [8, 8, 5]                               # utterance 2: prompt levels 5 .. 7 absent
    return lens_host, text, prom, resp, absent


@pytest.mark.parametrize("n_given", [1, 7])
def test_nar_embed_bwd_matches_autograd_over_the_merged_sequence(built_lib, n_given):
    from torch.nn.utils.rnn import pad_sequence
    from vall_e.vall_e import nar_train as NT
    d, K = 128, 50
    lens_host, text, prom, resp, absent = _assembly_case(d, K)
    B = len(lens_host)
    totals = [a + b_ + c + 2 for a, b_, c in lens_host]
    t_max = max(totals) + 5
    g = torch.Generator().manual_seed(n_given)
    dx = torch.randn(B, t_max, d, generator=g)
    sd = {"text_emb.weight": torch.zeros(K, d), "proms_emb.weight": torch.zeros(8, K, d), "resps_emb.weight": torch.zeros(7, K, d),
          "sep": torch.zeros(d)}
    sd = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    for b in range(B):
        seq = N.merged_sequence(sd, text[b], prom[b][:, :absent[b]], resp[b][:, :n_given])
        assert seq.shape == (totals[b], d)
        (seq * dx[b, : totals[b]].double()).sum().backward()
    # padding of the index arrays holds a valid id: reading it would add to a table
    i32 = lambda x: x.to(torch.int32)
    lens = torch.tensor(lens_host, dtype=torch.int32).to(DEV)
    text_g = pad_sequence([i32(x) for x in text], batch_first=True, padding_value=3).contiguous().to(DEV)
    prom_g = pad_sequence([F.pad(i32(x[:, :absent[b]]), (0, 8 - absent[b]), value=-1) for b, x in enumerate(prom)], batch_first=True,
                          padding_value=3).contiguous().to(DEV)
    resp_g = pad_sequence([i32(x) for x in resp], batch_first=True, padding_value=3).contiguous().to(DEV)

    def run(grad, times=1):
        out = [torch.zeros(K, d, device=DEV), torch.zeros(8, K, d, device=DEV), torch.zeros(7, K, d, device=DEV), torch.zeros(d, device=DEV)]
        for _ in range(times):
            NT.nar_embed_bwd(lens, text_g, prom_g, resp_g, n_given, grad.to(DEV), *out)
        return [o.cpu() for o in out]

    got = run(dx)
    names = ("text_emb.weight", "proms_emb.weight", "resps_emb.weight", "sep")
    errs = {}
    for name, o in zip(names, got):
        want = sd[name].grad
        errs[name] = close(o, want, name)
        untouched = want.reshape(-1, d).abs().sum(dim=1) == 0
        assert float(o.reshape(-1, d)[untouched].abs().sum()) == 0.0, f"{name}: an untouched row moved"
    assert float(got[2][n_given:].abs().sum()) == 0.0, "response levels at or above n_given are not touched"
    poisoned = dx.clone()
    for b in range(B):
        poisoned[b, totals[b]:] = 1e30
    assert all(torch.equal(a, b_) for a, b_ in zip(run(poisoned), got)), "rows behind an utterance's total are not read"
    twice = run(dx, times=2)
    assert all(torch.equal(a, 2 * b_) for a, b_ in zip(twice, got)), "the gradients are accumulated into"
    REPORT[f"nar_train_embed_bwd_given{n_given}"] = errs


# ---- 3. loss and dlogits ------------------------------------------------------------------------------------------------------------------
def test_nar_ce_matches_cross_entropy_over_the_response_rows(built_lib):
    from vall_e.vall_e import nar_train as NT
    K, B = 203, 3                                    # a class count that is no multiple of the wave
    lens_host = [(6, 9, 11), (9, 5, 14), (4, 12, 7)]
    totals = [a + b_ + c + 2 for a, b_, c in lens_host]
    t_max, tr_max = max(totals) + 5, 14
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(B, t_max, K, generator=g) * 3
    resp = torch.randint(0, K, (B, tr_max, 8), generator=g)
    n_frames = sum(c for _, _, c in lens_host)
    lg64 = logits.double().requires_grad_(True)
    rows = torch.cat([lg64[b, totals[b] - lens_host[b][2]: totals[b]] for b in range(B)])
    targ = torch.cat([resp[b, : lens_host[b][2], LEVELS[b] + 1] for b in range(B)])
    per_row = F.cross_entropy(rows, targ, reduction="none")
    (per_row.sum() / n_frames).backward()
    lens = torch.tensor(lens_host, dtype=torch.int32).to(DEV)
    levels = torch.tensor(LEVELS, dtype=torch.int32).to(DEV)
    row_loss, dlogits = NT.nar_ce(logits.to(DEV), lens, resp.to(torch.int32).to(DEV), levels, 1.0 / n_frames)
    live = torch.zeros(B, t_max, dtype=torch.bool)
    for b in range(B):
        live[b, totals[b] - lens_host[b][2]: totals[b]] = True
    row_loss, dlogits = row_loss.cpu(), dlogits.cpu()
    # fp32 logsumexp of 203 terms of magnitude <= 15: a few ulp of a value of about 10
    assert (row_loss[live].double() - per_row.detach()).abs().max().item() <= 2e-5
    assert abs(row_loss.double().sum().item() / n_frames - F.cross_entropy(rows, targ).item()) <= 1e-5
    assert float(row_loss[~live].abs().max()) == 0.0 and float(dlogits[~live].abs().max()) == 0.0, "non-response rows are exactly 0"
    err = close(dlogits, lg64.grad, "dlogits")
    only_loss, none = NT.nar_ce(logits.to(DEV), lens, resp.to(torch.int32).to(DEV), levels, 1.0 / n_frames, want_grad=False)
    assert none is None and torch.equal(only_loss.cpu(), row_loss)
    REPORT["nar_train_ce"] = {"dlogits": err}


# ---- 4. the step --------------------------------------------------------------------------------------------------------------------------
def test_step_matches_autograd_and_the_reference_fixture(built_lib):
    cfg, sd32, m = build()
    t, p, r = inputs()
    ref_loss, ref = reference()
    loss = m.forward_backward(t, p, r, seed=5, quant_levels=list(LEVELS))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and m.loss["nll"] is loss
    assert abs(float(loss) - ref_loss) <= 1e-4, (float(loss), ref_loss)
    worst = check_grads(m, ref, "levels (0, 3, 6)")
    gold = load("nar_train_grads.npz")
    assert [int(l) for l in gold["levels"]] == list(LEVELS) and abs(float(loss) - float(gold["loss"])) <= 1e-4
    for name, prm in m.named_parameters():
        stats, rows = R.summary(name, prm.grad.cpu())
        want = gold["g/" + name]
        scale = max(np.abs(want[2:]).max(), want[1] / prm.numel(), 1e-12)
        assert np.abs(stats[2:] - want[2:]).max() <= 5e-4 * scale + 1e-9, (name, stats[2:], want[2:])
        assert abs(stats[1] - want[1]) <= 5e-4 * want[1] + 1e-9, (name, stats[1], want[1])
        if name in R.TABLES:
            assert np.array_equal(rows, gold["rows/" + name]), f"{name}: rows that no token touched stay zero"
        if name.endswith("norm.emb.weight"):
            assert float(prm.grad[[1, 2, 4, 5]].abs().max()) == 0.0, f"{name}: AdaLN rows of levels that were not drawn stay zero"
    REPORT["nar_train_step_levels_036"] = {"loss_hip": float(loss), "loss_autograd": ref_loss, "worst_relative_error": max(worst.values()),
                                           "worst_tensor": max(worst, key=worst.get)}


def test_step_with_drawn_levels_matches_the_mirror_and_autograd(built_lib):
    from vall_e.vall_e.nar_train import NARTrainer
    cfg, sd32, m = build()
    t, p, r = inputs()
    seed, utt0 = 7, 2
    loss, levels = NARTrainer(m).step(t, p, r, seed=seed, utt0=utt0)
    assert levels == R.draw_levels(seed, utt0, 3), (levels, R.draw_levels(seed, utt0, 3))
    ref_loss, ref = reference(tuple(levels))
    assert abs(float(loss) - ref_loss) <= 1e-4, (float(loss), ref_loss)
    worst = check_grads(m, ref, f"drawn levels {levels}")
    top = max(levels)
    if top < 6:
        assert float(m.resps_emb.weight.grad[top + 1:].abs().max()) == 0.0, "resps_emb levels above every l_b stay zero"
    REPORT["nar_train_step_drawn_levels"] = {"levels": levels, "loss_hip": float(loss), "loss_autograd": ref_loss,
                                             "worst_relative_error": max(worst.values()), "worst_tensor": max(worst, key=worst.get)}


# ---- 5. forward ---------------------------------------------------------------------------------------------------------------------------
def test_forward_with_eight_levels_gives_the_same_loss_and_leaves_the_gradients(built_lib):
    cfg, sd32, m = build()
    t, p, r = inputs()
    loss = m.forward_backward(t, p, r, seed=5, quant_levels=list(LEVELS))
    before = {n: prm.grad.clone() for n, prm in m.named_parameters()}
    assert m(t, p, r, seed=5, quant_levels=list(LEVELS)) == []
    assert torch.equal(m.loss["nll"], loss), (float(m.loss["nll"]), float(loss))
    assert all(torch.equal(prm.grad, before[n]) for n, prm in m.named_parameters())
    loss7 = m.forward_backward(t, p, r, seed=7, utt0=2)
    assert m(t, p, r, seed=7, utt0=2) == [] and torch.equal(m.loss["nll"], loss7), "the same drawn levels"
    fresh = build()[2]
    assert fresh(t, p, r, seed=5, quant_levels=list(LEVELS)) == [] and torch.equal(fresh.loss["nll"], loss)
    assert all(prm.grad is None for prm in fresh.parameters())


# ---- 6. batch independence ----------------------------------------------------------------------------------------------------------------
def test_batch_gradient_is_the_frame_weighted_sum_of_the_utterances_alone(built_lib):
    cfg, sd32, m = build()
    t, p, r = inputs()
    m.forward_backward(t, p, r, seed=5, utt0=4, quant_levels=list(LEVELS))
    batch = {n: prm.grad.clone() for n, prm in m.named_parameters()}
    n_frames = sum(len(x) for x in r)
    parts = {n: torch.zeros_like(g) for n, g in batch.items()}
    for b in range(3):
        one = build()[2]
        one.forward_backward([t[b]], [p[b]], [r[b]], seed=5, utt0=4 + b, quant_levels=[LEVELS[b]])
        for n, prm in one.named_parameters():
            parts[n] += prm.grad * (len(r[b]) / n_frames)
    for n in batch:
        close(batch[n], parts[n].cpu(), f"batch vs utterances alone: {n}")
    m.forward_backward(t, p, r, seed=5, utt0=4, quant_levels=list(LEVELS))      # no zeroing in between: the sum
    for n, prm in m.named_parameters():
        close(prm.grad, 2 * batch[n].cpu(), f"two calls accumulate: {n}")


def test_padding_rows_are_neither_keys_nor_producers_of_gradient(built_lib):
    """The same step on grids with 5 padding rows behind every utterance's total (masked AdaLN rows, masked keys, mask_rows in the
    walk back): the bound of the step against the same fp64 reference, and the loss of the unpadded step."""
    from vall_e.vall_e.nar_train import NARTrainer
    cfg, sd32, m = build()
    t, p, r = inputs()
    ref_loss, ref = reference()
    loss, _ = NARTrainer(m).step(t, p, r, seed=5, quant_levels=list(LEVELS), pad_rows=5)
    assert abs(float(loss) - ref_loss) <= 1e-4, (float(loss), ref_loss)
    check_grads(m, ref, "5 padding rows")
    plain = build()[2]
    assert abs(float(plain.forward_backward(t, p, r, seed=5, quant_levels=list(LEVELS))) - float(loss)) <= 1e-5


# ---- 7. one SGD step ----------------------------------------------------------------------------------------------------------------------
def test_one_sgd_step_lowers_the_loss(built_lib):
    cfg, sd32, m = build()
    t, p, r = inputs()
    opt = torch.optim.SGD([prm for n, prm in m.named_parameters() if n.startswith(("blocks.", "classifier."))], lr=0.05)
    l0 = m.forward_backward(t, p, r, seed=5, quant_levels=list(LEVELS))
    opt.step()
    for prm in m.parameters():
        prm.grad = None
    l1 = m.forward_backward(t, p, r, seed=5, quant_levels=list(LEVELS))
    REPORT["nar_train_sgd_step_loss"] = {"before": float(l0), "after": float(l1)}
    assert float(l1) < float(l0)


# ---- 8. inference is untouched ------------------------------------------------------------------------------------------------------------
def test_inference_ids_are_the_same_before_and_after_a_training_call(built_lib):
    cfg, sd32, m = build()
    t, p, r = inputs()
    r1 = [x[:, :1] for x in r]
    before = m(t, p, r1, greedy=True)
    twin = build()[2]                                # a second module with the same weights
    twin.forward_backward(t, p, r, seed=5)
    m.forward_backward(t, p, r, seed=5)
    for model in (twin, m):
        after = model(t, p, r1, greedy=True)
        assert all(torch.equal(a, b_) for a, b_ in zip(before, after))
    assert all(o.shape == (len(x), 8) for o, x in zip(before, r))


# ---- 9. dropout ---------------------------------------------------------------------------------------------------------------------------
def test_dropout_zero_is_dropout_off(built_lib):
    cfg, sd32, m = build()
    t, p, r = inputs()
    off = m.forward_backward(t, p, r, seed=5, quant_levels=list(LEVELS))
    g_off = {n: prm.grad.clone() for n, prm in m.named_parameters()}
    for prm in m.parameters():
        prm.grad = None
    zero = m.forward_backward(t, p, r, seed=5, quant_levels=list(LEVELS), dropout=0.0)
    assert torch.equal(off, zero)
    assert all(torch.equal(prm.grad, g_off[n]) for n, prm in m.named_parameters())


def test_dropout_matches_autograd_with_the_mirror_masks(built_lib):
    cfg, sd32, m = build()
    t, p, r = inputs()
    seed, utt0, prob = 11, 3, 0.1
    ref_loss, ref = reference(LEVELS, None, (seed, utt0, prob))
    assert abs(ref_loss - reference()[0]) > 1e-3, "the masks change the loss"
    loss = m.forward_backward(t, p, r, seed=seed, utt0=utt0, quant_levels=list(LEVELS), dropout=True)
    assert abs(float(loss) - ref_loss) <= 1e-4, (float(loss), ref_loss)
    worst = check_grads(m, ref, "dropout 0.1")
    # utterance 1 alone, keyed by its global index: its masks and its loss term are those it has inside the batch
    n_frames = sum(len(x) for x in r)
    share = 0.0
    for b in range(3):
        one = build()[2]
        l_b = one.forward_backward([t[b]], [p[b]], [r[b]], seed=seed, utt0=utt0 + b, quant_levels=[LEVELS[b]], dropout=prob)
        ref_b, _ = reference(LEVELS, b, (seed, utt0 + b, prob))
        assert abs(float(l_b) - ref_b) <= 1e-4, (b, float(l_b), ref_b)
        share += float(l_b) * len(r[b]) / n_frames
    assert abs(share - float(loss)) <= 1e-5, (share, float(loss))
    REPORT["nar_train_step_dropout"] = {"loss_hip": float(loss), "loss_autograd": ref_loss, "worst_relative_error": max(worst.values()),
                                        "worst_tensor": max(worst, key=worst.get)}

"""NAR training step (vall_e/vall_e/nar_train.py; include/d3pm_hip.h "NAR training step"): what can be checked without a GPU
(python -m pytest tests/test_nar_train_api.py -m "not gpu").  The three entries are declared, bound and exported and refuse bad
arguments before anything is launched (every pointer below is a made-up address: a call that got as far as a launch would not
return a refusal code); the host validation of NAR.forward_backward / NAR.forward comes before the device check; the level draw
of the numpy mirror covers 0 .. 6 and depends on (seed, utterance) alone; and the test reference (tests/nar_train_ref.py) gives the
gradients of the reference's own NAR (tests/golden/nar_train_grads.npz)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import nar_train_ref as R
from conftest import ROOT
from util import load

NAMES = ("d3pm_op_adaln_bwd_f32", "d3pm_op_nar_embed_bwd_f32", "d3pm_op_nar_ce_f32")
EMBED_POINTERS = ("lens", "text", "prom", "resp", "dx", "d_text", "d_prom", "d_resp", "d_sep")


def _codes():
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    return {name: int(value) for name, value in re.findall(r"\b(D3PM_E_[A-Z]+)\s*=\s*(-?\d+)", header)}


def _adaln_bwd(lib, **kw):
    a = dict(x=0x100000, dy=0x200000, emb_row=0x300000, row_mask=0x400000, M=37, d=128, dx=0x500000, accumulate=0, demb_row=0x600000)
    a.update(kw)
    return lib.d3pm_op_adaln_bwd_f32(a["x"], a["dy"], a["emb_row"], a["row_mask"], a["M"], a["d"], a["dx"], a["accumulate"], a["demb_row"], None)


def _embed_bwd(lib, **kw):
    a = dict(tt_max=10, tp_max=12, n_prom_levels=8, tr_max=16, resp_stride=8, n_given=1, batch=3, t_max=40, d=128, n_tokens=64)
    a.update({name: 0x100000 * (i + 1) for i, name in enumerate(EMBED_POINTERS)})
    a.update(kw)
    return lib.d3pm_op_nar_embed_bwd_f32(a["lens"], a["text"], a["tt_max"], a["prom"], a["tp_max"], a["n_prom_levels"], a["resp"], a["tr_max"],
                                         a["resp_stride"], a["n_given"], a["dx"], a["d_text"], a["d_prom"], a["d_resp"], a["d_sep"],
                                         a["batch"], a["t_max"], a["d"], a["n_tokens"], None)


def _ce(lib, **kw):
    a = dict(logits=0x100000, ldl=1024, lens=0x200000, resp=0x300000, tr_max=44, resp_stride=8, levels=0x400000, batch=3, t_max=90,
             n_tokens=1024, gscale=0.01, row_loss=0x500000, dlogits=0x600000, ldd=1024)
    a.update(kw)
    return lib.d3pm_op_nar_ce_f32(a["logits"], a["ldl"], a["lens"], a["resp"], a["tr_max"], a["resp_stride"], a["levels"], a["batch"],
                                  a["t_max"], a["n_tokens"], a["gscale"], a["row_loss"], a["dlogits"], a["ldd"], None)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
        params = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(_hip.SIGNATURES[name][1]) == params.count(",") + 1, name
        assert name in header.split("#define D3PM_ABI_VERSION")[0], "the additions are listed in the version comment"
    assert "#define D3PM_ABI_VERSION 6" in header and _hip.ABI_VERSION == 6 and built_lib.d3pm_abi_version() == 6


def test_adaln_bwd_entry_refuses_before_any_launch(built_lib):
    arg = _codes()["D3PM_E_ARG"]
    for name in ("x", "dy", "emb_row", "row_mask", "dx", "demb_row"):
        assert _adaln_bwd(built_lib, **{name: None}) == arg, name
    for name in ("M", "d"):
        for bad in (0, -4):
            assert _adaln_bwd(built_lib, **{name: bad}) == arg, (name, bad)


def test_embed_bwd_entry_refuses_before_any_launch(built_lib):
    arg = _codes()["D3PM_E_ARG"]
    for name in EMBED_POINTERS:
        assert _embed_bwd(built_lib, **{name: None}) == arg, name
    for name in ("batch", "t_max", "tt_max", "tp_max", "tr_max", "d", "n_tokens", "n_prom_levels"):
        for bad in (0, -1):
            assert _embed_bwd(built_lib, **{name: bad}) == arg, (name, bad)
    assert _embed_bwd(built_lib, n_given=0) == arg
    assert _embed_bwd(built_lib, n_given=9) == arg                          # more levels than a response row holds
    assert _embed_bwd(built_lib, n_given=4, resp_stride=3) == arg
    assert _embed_bwd(built_lib, n_prom_levels=65536) == _codes()["D3PM_E_SHAPE"]      # one grid slice per level


def test_ce_entry_refuses_before_any_launch(built_lib):
    arg = _codes()["D3PM_E_ARG"]
    for name in ("logits", "lens", "resp", "levels", "row_loss"):
        assert _ce(built_lib, **{name: None}) == arg, name
    for name in ("batch", "t_max", "tr_max"):
        for bad in (0, -1):
            assert _ce(built_lib, **{name: bad}) == arg, (name, bad)
    assert _ce(built_lib, ldl=1023) == arg and _ce(built_lib, ldd=1023) == arg      # a row stride below the class count
    assert _ce(built_lib, n_tokens=1, ldl=1, ldd=1) == arg
    assert _ce(built_lib, resp_stride=1) == arg                             # no column left for a target


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def _cpu_model():
    from vall_e.vall_e import NAR
    return NAR(1024, 128, 2, 2)


def _inputs(n=3):
    from vall_e.vall_e import synth
    return synth.make_nar_inputs(n, 1, n_levels=8)


def test_signatures_show_the_new_keywords():
    from vall_e.vall_e import NAR
    fb = inspect.signature(NAR.forward_backward).parameters
    assert [n for n in fb][:4] == ["self", "text_list", "proms_list", "resps_list"]
    for name, default in (("seed", None), ("utt0", 0), ("quant_levels", None), ("dropout", False)):
        assert fb[name].kind is inspect.Parameter.KEYWORD_ONLY and fb[name].default == default, name
    fw = inspect.signature(NAR.forward).parameters
    for name, default in (("seed", None), ("utt0", 0), ("quant_levels", None)):
        assert fw[name].kind is inspect.Parameter.KEYWORD_ONLY and fw[name].default == default, name
    assert fw["sampling_temperature"].default == 0.2


def test_every_bad_argument_is_a_value_error_before_the_device_check():
    m = _cpu_model()
    t, p, r = _inputs()
    bad_calls = [
        ((t[:2], p, r), {}),                                                 # lists of unequal length
        ((t, p[:1], r), {}),
        ((t, p, [r[0], r[1], r[2][:, :4]]), {}),                            # not all 8 levels wide
        ((t, p, [x[:, :4] for x in r]), {}),
        ((t, p, [r[0], r[1][:0], r[2]]), {}),                               # an utterance without a response frame
        ((t, p, r), dict(quant_levels=[0, 1])),                              # wrong length
        ((t, p, r), dict(quant_levels=[0, 7, 1])),                           # outside 0 .. 6
        ((t, p, r), dict(quant_levels=[0, -1, 1])),
        ((t, p, r), dict(dropout=1.0)),
        ((t, p, r), dict(dropout=-0.1)),
        ((t, p, r), dict(dropout="yes")),
    ]
    for args, kw in bad_calls:
        with pytest.raises(ValueError):
            m.forward_backward(*args, **kw)
    for args, kw in (((t[:2], p, r), {}), ((t, p, [r[0], r[1][:0], r[2]]), {}), ((t, p, r), dict(quant_levels=[0, 7, 1])),
                     ((t, p, r), dict(quant_levels=[0]))):
        with pytest.raises(ValueError):
            m(*args, **kw)
    with pytest.raises(ValueError, match="only one level"):
        m(t, p, [r[0], r[1], r[2][:, :4]])                                   # upstream's own refusal stays
    from vall_e.vall_e import NAR
    deep = NAR(1024, 64, 1, 17)
    with pytest.raises(ValueError, match="16 layers"):
        deep.forward_backward(t, p, r, dropout=True)


def test_valid_arguments_reach_no_cpu_path():
    m = _cpu_model()
    t, p, r = _inputs()
    for kw in ({}, dict(seed=3, utt0=5), dict(quant_levels=[0, 3, 6]), dict(dropout=True), dict(dropout=0.0), dict(dropout=0.25)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.forward_backward(t, p, r, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(t, p, r, quant_levels=[1, 2, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(t, p, [x[:, :1] for x in r])                                       # the inference call, as before


def test_trainer_requires_an_fp32_model_on_a_hip_device():
    from vall_e.vall_e import _hip
    from vall_e.vall_e.nar_train import NARTrainer
    with pytest.raises(_hip.D3PMError):
        NARTrainer(_cpu_model())
    with pytest.raises(_hip.D3PMError):
        NARTrainer(_cpu_model().half())


def test_dropout_argument_and_site_numbers():
    from vall_e.vall_e import nar_train as NT
    from vall_e.vall_e.train import dropout_site as cond_site
    assert NT.dropout_prob(False) == 0.0 and NT.dropout_prob(None) == 0.0 and NT.dropout_prob(True) == 0.1 and NT.dropout_prob(0.3) == 0.3
    sites = {NT.dropout_site(l, k) for l in range(16) for k in range(3)}
    assert len(sites) == 48 and NT.dropout_site(3, 2) == (2 << 8) | (3 << 4) | 2
    assert not sites & {cond_site(w, l, k) for w in (0, 1) for l in range(16) for k in range(4)}, "clear of the condition encoders' sites"
    assert NT.LEVEL_STREAM == 6


# ---- the level draw ----------------------------------------------------------------------------------------------------------------------
def test_level_draw_of_the_mirror_covers_every_level_and_depends_on_seed_and_utterance_only():
    levels = R.draw_levels(7, 0, 64)
    assert set(levels) == set(range(7)), sorted(set(levels))
    assert R.draw_levels(7, 10, 20) == levels[10:30], "a function of utt0 + b: a shard draws what the whole batch draws"
    assert [R.draw_levels(7, u, 1)[0] for u in range(64)] == levels
    assert R.draw_levels(8, 0, 64) != levels
    from oracle import philox
    u = philox.uniform_rows(7, 0, 0, 64, 4, stream=6)[:, 0]
    assert levels == [min(6, int(np.float32(v) * np.float32(7))) for v in u]
    assert not np.array_equal(u, philox.uniform_rows(7, 0, 0, 64, 4, stream=5)[:, 0]), "its own stream"


# ---- the test reference is the reference -------------------------------------------------------------------------------------------------
def test_autograd_over_the_restatement_matches_the_reference_fixture():
    """fp32 autograd over nar_train_ref.nll against the reference's own NAR (make_nar_train_grads.py): the loss within 1e-6, the
    samples and the absolute sums within 5e-4 of scale (test_gpu_train.py's bound for the same comparison); the rows of the three
    tables that received gradient are the fixture's."""
    from vall_e.vall_e import synth
    gold = load("nar_train_grads.npz")
    cfg = synth.NARConfig(d_model=128, n_heads=2, n_layers=2)
    sd32 = synth.make_nar_state_dict(cfg, 0)
    t, p, r = _inputs()
    levels = [int(l) for l in gold["levels"]]
    assert levels == [0, 3, 6]
    loss, grads = R.loss_and_grads(sd32, cfg.n_heads, cfg.n_layers, t, p, r, levels, dtype=torch.float32)
    assert abs(loss - float(gold["loss"])) <= 1e-6, (loss, float(gold["loss"]))
    assert sorted(k[2:] for k in gold.files if k.startswith("g/")) == sorted(sd32) and len(sd32) == 24
    for name in sd32:
        stats, rows = R.summary(name, grads[name])
        want = gold["g/" + name]
        scale = max(np.abs(want[2:]).max(), want[1] / grads[name].numel(), 1e-12)
        assert np.abs(stats[2:] - want[2:]).max() <= 5e-4 * scale + 1e-9, (name, stats[2:], want[2:])
        assert abs(stats[1] - want[1]) <= 5e-4 * want[1] + 1e-9, (name, stats[1], want[1])
        if name in R.TABLES:
            assert np.array_equal(rows, gold["rows/" + name]), name
    # the detach is part of the model: differentiating through f = c (1 - k h) moves to_qkv's gradient by percents
    sd = {k: v.clone().requires_grad_(True) for k, v in sd32.items()}
    orig = R.adaln
    try:
        def no_detach(x, emb_rows):
            d = x.shape[-1]
            h = torch.nn.functional.layer_norm(x, x.shape[-1:], eps=1e-5)
            return emb_rows[:, None, :d].exp() * (2 * (1 - 0.1 * h) * h) + emb_rows[:, None, d:]
        R.adaln = no_detach
        R.nll(sd, cfg.n_heads, cfg.n_layers, t, p, r, levels).backward()
    finally:
        R.adaln = orig
    name = "blocks.0.attn.block.to_qkv.weight"
    moved = (sd[name].grad - grads[name]).abs().max().item() / grads[name].abs().max().item()
    assert moved > 5e-3, moved

"""Key-padding masks in the training step (forward_backward(mask_padding=True), forward(mask_padding=True)): what can be checked
without a GPU -- the two C entries and their bindings, the host derivation of the three key counts (train.key_mask_lengths) with
the rule for a dropped condition, and the ValueErrors that come before any GPU work."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

NEW_ENTRIES = ("d3pm_op_attention_bwd_keylen_f32", "d3pm_op_attention_dropout_keylen_f32")


def _cfg():
    from vall_e.vall_e import synth
    return synth.D3PMConfig.native()


def _inputs(cfg, text_lens=(3, 60), prom_rows=(4, 500), frames=(300, 600)):
    texts = [torch.ones(n, dtype=torch.long) for n in text_lens]
    proms = [torch.zeros(n, 8, dtype=torch.long) for n in prom_rows]
    resps = [torch.ones(n, dtype=torch.long) for n in frames]
    return texts, proms, resps


def test_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
    assert built_lib.d3pm_abi_version() == 6 == _hip.ABI_VERSION      # additions only
    version_comment = header.split("#define D3PM_ABI_VERSION")[0]
    for name in NEW_ENTRIES:
        assert name in version_comment, name
    # the backward entry is the dropout backward entry with key_len in front of the dropout arguments, the forward entry likewise
    a, b = _hip.SIGNATURES["d3pm_op_attention_bwd_keylen_f32"][1], _hip.SIGNATURES["d3pm_op_attention_bwd_dropout_f32"][1]
    assert a == b[:-5] + [C.c_void_p] + b[-5:]
    a, b = _hip.SIGNATURES["d3pm_op_attention_dropout_keylen_f32"][1], _hip.SIGNATURES["d3pm_op_attention_dropout_f32"][1]
    assert a == b[:-5] + [C.c_void_p] + b[-5:]
    # the three existing entries keep their argument lists
    assert len(_hip.SIGNATURES["d3pm_op_attention_bwd_f32"][1]) == 21
    assert len(_hip.SIGNATURES["d3pm_op_attention_dropout_f32"][1]) == 18 and len(_hip.SIGNATURES["d3pm_op_attention_bwd_dropout_f32"][1]) == 25
    # what a masked key reads and writes is written down
    doc = header.split("Key-padding masks in the training step")[-1]
    assert "reads nothing" in doc and "exactly 0" in doc and "1 <= key_len[b] <= S" in doc


def test_signatures_and_docs():
    from vall_e.vall_e import AR, _hip
    from vall_e.vall_e import train as T
    for fn in (AR.forward_backward, AR.forward, T.D3PMTrainer.forward_backward):
        p = inspect.signature(fn).parameters["mask_padding"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert inspect.signature(T.attention_bwd).parameters["key_len"].default is None
    assert inspect.signature(T.attention_dropout).parameters["key_len"].default is None
    assert inspect.signature(T.D3PMTrainer._encode).parameters["key_len"].default is None
    assert inspect.signature(_hip.Sampler.training_forward).parameters["keys"].default is None
    doc = AR.generate_audio.__doc__
    assert "trained with the padding as keys" in doc and "no statement about audio quality" in doc
    assert "does not take the mask" not in doc and "forward_backward(mask_padding=True)" in doc


def test_length_derivation_and_truncation():
    from vall_e.vall_e.train import key_mask_lengths
    cfg = _cfg()
    assert (cfg.canvas, cfg.s_text, cfg.s_prompt) == (448, 50, 398)
    texts, proms, resps = _inputs(cfg)
    assert key_mask_lengths(cfg, texts, proms, resps) == ([300, 448], [3, 50], [4, 398])
    # frames count by length, not by x0 != 0: zeros inside (and at the end of) the utterance stay keys
    zeros = [torch.tensor([5, 0, 7, 0]), torch.zeros(9, dtype=torch.long)]
    assert key_mask_lengths(cfg, texts, proms, zeros)[0] == [4, 9]
    assert key_mask_lengths(cfg, texts, proms, [r.reshape(1, -1) for r in zeros])[0] == [4, 9]
    # exactly at the pads
    t2, p2, r2 = _inputs(cfg, (cfg.s_text, 1), (cfg.s_prompt, 1), (cfg.canvas, 1))
    assert key_mask_lengths(cfg, t2, p2, r2) == ([448, 1], [50, 1], [398, 1])
    assert key_mask_lengths(cfg, texts, proms, resps, mask_padding=False) is None


def test_a_dropped_condition_keeps_all_of_its_padding():
    """the rule AR._twin_key_lengths applies to the default null twin of guidance"""
    from vall_e.vall_e import AR
    from vall_e.vall_e.train import key_mask_lengths
    cfg = _cfg()
    texts, proms, resps = _inputs(cfg)
    got = key_mask_lengths(cfg, texts, proms, resps, dropped=[(True, False), (False, True)])
    assert got == ([300, 448], [cfg.s_text, 50], [4, cfg.s_prompt])
    assert key_mask_lengths(cfg, texts, proms, resps, dropped=[(True, True), (False, False)]) == ([300, 448], [50, 50], [398, 398])
    assert key_mask_lengths(cfg, texts, proms, resps, dropped=[(False, False)] * 2) == key_mask_lengths(cfg, texts, proms, resps)
    m = AR.reference_native()
    twin = m._twin_key_lengths(m.key_lengths(texts, proms, [300, 448]), None, None)
    both = key_mask_lengths(cfg, texts, proms, resps, dropped=[(True, True)] * 2)
    assert tuple(v[2:] for v in twin) == both


@pytest.mark.parametrize("case", ["empty_text", "empty_prompt", "scalar_text", "no_frames", "texts_short", "resps_short", "dropped_short"])
def test_key_mask_lengths_refuses(case):
    from vall_e.vall_e.train import key_mask_lengths
    cfg = _cfg()
    texts, proms, resps = _inputs(cfg)
    kw = {}
    if case == "empty_text":
        texts[1] = texts[1][:0]
    elif case == "empty_prompt":
        proms[0] = proms[0][:0]
    elif case == "scalar_text":
        texts[0] = torch.tensor(3)
    elif case == "no_frames":
        resps[1] = resps[1][:0]
    elif case == "texts_short":
        texts = texts[:1]
    elif case == "resps_short":
        resps = resps[:1]
    else:
        kw["dropped"] = [(False, False)]
    with pytest.raises(ValueError, match="mask_padding"):
        key_mask_lengths(cfg, texts, proms, resps, **kw)
    # an empty condition that the caller passes is refused even where cond_drop would have replaced it anyway
    if case in ("empty_text", "empty_prompt"):
        with pytest.raises(ValueError, match="mask_padding"):
            key_mask_lengths(cfg, texts, proms, resps, dropped=[(True, True)] * 2)


@pytest.mark.parametrize("bad", [1, 0, None, "yes", 1.0, (True,)], ids=repr)
def test_mask_padding_must_be_a_bool(bad):
    from vall_e.vall_e import AR
    from vall_e.vall_e.train import key_mask_lengths
    cfg = _cfg()
    texts, proms, resps = _inputs(cfg)
    with pytest.raises(ValueError, match="mask_padding must be a bool"):
        key_mask_lengths(cfg, texts, proms, resps, mask_padding=bad)
    with pytest.raises(ValueError, match="mask_padding must be a bool"):      # before the device check: the model lives on the CPU here
        AR.reference_native().forward(texts, proms, resps, mask_padding=bad)


def test_forward_rejects_on_the_host_and_valid_calls_reach_the_device_check():
    """ValueError before anything touches the GPU: the model lives on the CPU here, and a valid call raises the RuntimeError of a
    missing HIP device instead."""
    from vall_e.vall_e import AR
    m = AR.reference_native()
    texts, proms, resps = _inputs(m.cfg)
    with pytest.raises(ValueError, match="empty text"):
        m.forward([texts[0], texts[1][:0]], proms, resps, mask_padding=True)
    with pytest.raises(ValueError, match="empty prompt"):
        m.forward(texts, [proms[0][:0], proms[1]], resps, mask_padding=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.forward([texts[0], texts[1][:0]], proms, resps)      # legal without the mask
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.forward(texts, proms, resps, mask_padding=True)


def test_masked_training_kernels_have_no_scratch():
    """hipcc's resource remarks: all four arms of the two backward kernels and the dropout forward are there, none with scratch."""
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "d3pm_train.hip", "attn_bwd_"], capture_output=True,
                         text=True, check=True).stdout
    rows = [ln for ln in out.splitlines() if "VGPR" in ln]
    for kernel in ("attn_bwd_q_rows", "attn_bwd_kv_rows"):
        for arm in ("<false, false>", "<true, false>", "<false, true>", "<true, true>"):
            assert sum(kernel + arm in ln for ln in rows) == 1, (kernel, arm, out)
    out2 = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "d3pm_generic.hip", "attention_rows<float, true>"],
                          capture_output=True, text=True, check=True).stdout
    rows += [ln for ln in out2.splitlines() if "VGPR" in ln]
    assert len(rows) == 9, out + out2
    for ln in rows:
        assert re.search(r"scratch\s+0\b", ln), ln

"""Host side of the two test entries of the deduplicated loop's kernels (include/d3pm_hip.h: d3pm_op_attention_pair_segments,
d3pm_op_posterior_sample_rows; no GPU): what the kernels cannot run is refused BEFORE anything is launched, the entries add no kernel
choice of their own, and the Python wrappers check dtype, device and shape.  Every pointer handed to the library below is a made-up
address: a call that got as far as a launch would not return a refusal code."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT


def _codes():
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    return {name: int(value) for name, value in re.findall(r"\b(D3PM_E_[A-Z]+)\s*=\s*(-?\d+)", header)}


def _tuning(**fields):
    from vall_e.vall_e import _hip
    tn = _hip.Tuning()
    _hip.lib().d3pm_tuning_default(C.byref(tn))
    for name, value in fields.items():
        setattr(tn, name, value)
    return tn


def _pair(lib, tn, *, S1=64, S2=256, seg=0x50000, dtype=2, Tq=768, B=3):
    q1, q2, o1, o2, k1, v1, k2, v2 = (0x100000 * (i + 1) for i in range(8))
    return lib.d3pm_op_attention_pair_segments(dtype, q1, k1, v1, o1, S1, q2, k2, v2, o2, S2, 128, 256, 128, B, Tq, 2, 64, 0.125, seg,
                                               None if seg is None else seg + 64, None, None, C.byref(tn), None)


def test_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in ("d3pm_op_attention_pair_segments", "d3pm_op_posterior_sample_rows"):
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
    # the segment pair is the masked pair with the two segment arrays in front of the key lengths; the sampler takes what the nucleus
    # step entry takes, with a row stride and the index behind the logits and no posterior / theta outputs
    pair, seg = _hip.SIGNATURES["d3pm_op_attention_pair_keylen"][1], _hip.SIGNATURES["d3pm_op_attention_pair_segments"][1]
    assert seg == pair[:19] + [C.c_void_p, C.c_void_p] + pair[19:]
    rows = _hip.SIGNATURES["d3pm_op_posterior_sample_rows"][1]
    assert rows[0] == C.POINTER(_hip.Shape) and rows[-3:] == [C.POINTER(_hip.Nucleus), C.POINTER(_hip.Guidance), C.c_void_p]


def test_segment_pair_is_refused_where_the_plan_is_not_the_resident_pair(built_lib):
    codes = _codes()
    resident = _tuning(attn_cross_resident=5)
    # missing segment arrays are an argument error whatever the plan
    assert _pair(built_lib, resident, seg=None) == codes["D3PM_E_ARG"]
    # more text keys than one resident tile, more prompt keys than four: the planner names the tile-by-tile pair, which takes no segments
    assert _pair(built_lib, resident, S1=65) == codes["D3PM_E_SHAPE"]
    assert b"query segments" in built_lib.d3pm_last_error()
    assert _pair(built_lib, resident, S1=128) == codes["D3PM_E_SHAPE"]
    assert _pair(built_lib, resident, S2=257) == codes["D3PM_E_SHAPE"]
    assert _pair(built_lib, resident, S2=320) == codes["D3PM_E_SHAPE"]
    # the resident pair switched off, left to the automatic rule below one workgroup per CU, or moved to the 16 x 16 x 32 instruction
    assert _pair(built_lib, _tuning(attn_cross_resident=0)) == codes["D3PM_E_SHAPE"]
    assert _pair(built_lib, _tuning(attn_cross_resident=1)) == codes["D3PM_E_SHAPE"]
    assert _pair(built_lib, _tuning(attn_cross_resident=4)) == codes["D3PM_E_SHAPE"]
    # fp32 has no MFMA attention at all
    assert _pair(built_lib, resident, dtype=0) == codes["D3PM_E_SHAPE"]


def test_segment_pair_adds_no_kernel_choice_of_its_own():
    src = open(os.path.join(ROOT, "tts-with-diffusion-model_amd", "csrc", "d3pm_api.hip")).read()
    body = src[src.index("int d3pm_op_attention_pair_segments("):]
    body = body[:body.index("\n}\n")]
    assert "run_attention(" in body and "attn_cross_resident" not in body and "tune_of" not in body and "<<<" not in body


def _sample(lib, *, n_q=1, dtype=2, row_of=0x2000, guidance=None, ldl=1032, t=50, flags=0, top_p=None):
    from vall_e.vall_e import _hip
    sched = _hip.Schedule(100)
    tn = _tuning()
    shape = _hip.Shape(512, 8, 2, 768, 64, 225, 1025, 1024, 100, 2, n_q, C.pointer(tn))
    nuc = None if top_p is None else C.byref(_hip.Nucleus(1.0, 0, top_p))
    gd = None if guidance is None else C.byref(_hip.Guidance(guidance))
    return lib.d3pm_op_posterior_sample_rows(C.byref(shape), 2, 0x100000, dtype, ldl, row_of, 0x200000, 0x300000, None, None, t,
                                             C.byref(sched.c_struct), 7, 0, flags, nuc, gd, None)


def test_sampler_entry_refuses_before_any_launch(built_lib):
    from vall_e.vall_e import _hip
    codes = _codes()
    arg = codes["D3PM_E_ARG"]
    assert _sample(built_lib, row_of=None) == arg
    assert _sample(built_lib, dtype=0) == arg                     # fp32 logits
    assert b"16-bit" in built_lib.d3pm_last_error()
    assert _sample(built_lib, n_q=8) == arg
    assert _sample(built_lib, guidance=1.5) == arg
    assert _sample(built_lib, ldl=1024) == arg                     # a row stride below the class count
    assert _sample(built_lib, t=100) == arg
    assert _sample(built_lib, top_p=0.0) == arg
    assert _sample(built_lib, flags=_hip.FLAG_SEED_IN_HBM) == arg


def test_python_wrappers_check_their_tensors(built_lib):
    from vall_e.vall_e import _hip
    bf = torch.bfloat16
    q = torch.zeros(256, 128, dtype=bf)
    kt, kp = torch.zeros(2, 64, 256, dtype=bf), torch.zeros(2, 256, 256, dtype=bf)
    seg = torch.zeros(2, dtype=torch.int32)
    o1, o2 = torch.empty_like(q), torch.empty_like(q)

    def pair(**kw):
        a = dict(q1=q, k1=kt[..., :128], v1=kt[..., 128:], q2=q, k2=kp[..., :128], v2=kp[..., 128:], seg_start=seg, seg_len=seg, n_heads=2,
                 scale=0.125, out1=o1, out2=o2, capacity=128)
        a.update(kw)
        return _hip.op_attention_pair_segments(**a)

    for bad in (dict(seg_len=seg.long()), dict(seg_start=torch.zeros(3, dtype=torch.int32)), dict(out2=o2.half()), dict(q2=q[:128]),
                dict(v1=kt[..., 128:].contiguous()), dict(capacity=100), dict(capacity=384), dict(key_len=seg.long()),
                dict(key_len2=torch.zeros(1, dtype=torch.int32)), dict(k2=kp[:1, :, :128])):
        with pytest.raises(_hip.D3PMError):
            pair(**bad)

    sched = _hip.Schedule(100)
    shape = _hip.Shape(512, 8, 2, 768, 64, 225, 1025, 1024, 100, 2, 1, C.pointer(_hip.TUNING))
    x = torch.zeros(2, 768, dtype=torch.int32)
    lg = torch.zeros(1536, 1025, dtype=bf)
    idx = torch.zeros(1536, dtype=torch.int32)

    def rows(**kw):
        a = dict(logits=lg, row_of=idx, x_t=x)
        a.update(kw)
        return _hip.op_posterior_sample_rows(shape, sched, a["logits"], a["row_of"], a["x_t"], 50, 7, **{k: v for k, v in a.items()
                                                                                                      if k not in ("logits", "row_of", "x_t")})

    for bad in (dict(logits=lg.float()), dict(logits=lg[:, :1024]), dict(logits=lg[:1535]), dict(row_of=idx.long()), dict(row_of=idx[:768]),
                dict(x_t=x.long()), dict(x_t=x[:, :767]), dict(known=torch.zeros(2, 768, dtype=torch.bool)),
                dict(known=torch.zeros(1, 768, dtype=torch.uint8))):
        with pytest.raises(_hip.D3PMError):
            rows(**bad)
    for bad in (dict(temperature=0.0), dict(top_k=-1), dict(top_p=1.5), dict(guidance=-1.0)):
        with pytest.raises(ValueError):
            rows(**bad)

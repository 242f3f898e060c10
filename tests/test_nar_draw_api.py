"""Host side of the NAR stage's level draw with options (include/d3pm_hip.h: d3pm_nar_draw, d3pm_nar_level_draw, d3pm_op_nar_draw; no
GPU): the entries are declared, bound and exported; what the kernel cannot run is refused BEFORE anything is launched (every pointer
handed to the library below is a made-up address); NAR.forward validates its options before it looks for a device; and the host
reference of the GPU tests (tests/nar_draw_ref.py) satisfies the invariants the header states."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nar_draw_ref as R
from conftest import ROOT

NAMES = ("d3pm_nar_level_draw", "d3pm_op_nar_draw")


def _codes():
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    return {name: int(value) for name, value in re.findall(r"\b(D3PM_E_[A-Z]+)\s*=\s*(-?\d+)", header)}


def test_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
        params = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(_hip.SIGNATURES[name][1]) == params.count(",") + 1, name
        assert "const d3pm_nar_draw *draw, void *stream" in params          # the options sit right before the stream
    # the struct's fields in the header's order, and each entry = the entry it generalises plus the one pointer
    fields = re.search(r"typedef struct d3pm_nar_draw \{([^}]*)\} d3pm_nar_draw;", header).group(1)
    assert [f.split()[-1].lstrip("*") for f in fields.strip().rstrip(";").split(";")] == [n for n, _ in _hip.NarDraw._fields_]
    for name, base in zip(NAMES, ("d3pm_nar_level", "d3pm_op_nar_sample")):
        new, old = _hip.SIGNATURES[name][1], _hip.SIGNATURES[base][1]
        assert new[:-2] == old[:-1] and new[-1] == old[-1] and new[-2] == C.POINTER(_hip.NarDraw), name
    assert "#define D3PM_ABI_VERSION 6" in header and built_lib.d3pm_abi_version() == 6


def _draw(lib, draw, **kw):
    a = dict(dtype=2, logits=0x100000, ldl=1032, lens=0x200000, resp=0x300000, tr_max=704, resp_stride=8, t_max=704, n_tokens=1024,
             level=0, temperature=0.2, seed=7, utt0=0, flags=0, batch=3)
    a.update(kw)
    return lib.d3pm_op_nar_draw(a["dtype"], a["logits"], a["ldl"], a["lens"], a["resp"], a["tr_max"], a["resp_stride"], a["t_max"],
                                a["n_tokens"], a["level"], a["temperature"], a["seed"], a["utt0"], a["flags"], a["batch"],
                                None if draw is None else C.byref(draw), None)


def test_op_entry_refuses_before_any_launch(built_lib):
    from vall_e.vall_e import _hip
    codes = _codes()
    arg, shape = codes["D3PM_E_ARG"], codes["D3PM_E_SHAPE"]
    ok = _hip.NarDraw(0.9, 50, None, 0x400000, None)
    for name in ("logits", "lens", "resp"):
        assert _draw(built_lib, ok, **{name: None}) == arg, name
    for name in ("batch", "t_max", "tr_max", "n_tokens"):
        for bad in (0, -1):
            assert _draw(built_lib, ok, **{name: bad}) == arg, (name, bad)
    assert _draw(built_lib, ok, ldl=1023) == arg and _draw(built_lib, ok, level=7) == arg and _draw(built_lib, ok, dtype=5) == arg
    # the temperature: finite and > 0, with or without options
    for draw in (ok, None):
        for bad in (0.0, -0.2, float("nan"), float("inf")):
            assert _draw(built_lib, draw, temperature=bad) == arg, bad
    for bad in (-1, 1025, 2 ** 31 - 1):
        assert _draw(built_lib, _hip.NarDraw(1.0, bad, None, None, None)) == arg, bad
        assert b"top_k" in built_lib.d3pm_last_error()
    for bad in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert _draw(built_lib, _hip.NarDraw(bad, 0, None, None, None)) == arg, bad
        assert b"top_p" in built_lib.d3pm_last_error()
    # more tokens than a wave's registers hold: only the draw WITH options is limited
    assert _draw(built_lib, ok, n_tokens=1284, ldl=1284) == shape
    assert _draw(built_lib, _hip.NarDraw(1.0, 1284, None, None, None), n_tokens=1284, ldl=1284) == shape


def test_python_wrapper_checks_its_tensors(built_lib):
    from vall_e.vall_e import _hip
    bf = torch.bfloat16
    grid = torch.zeros(3, 20, 72, dtype=bf)
    lens = torch.zeros(3, 3, dtype=torch.int32)
    resp = torch.zeros(3, 16, 8, dtype=torch.int32)
    known = torch.zeros(3, 16, dtype=torch.uint8)
    lp = torch.zeros(3, 16, 7)
    theta = torch.zeros(3, 16)
    for bad in (dict(known=known.bool()), dict(known=known[:, :15]), dict(known=known[:2]), dict(logprob_out=lp[..., :6]),
                dict(logprob_out=lp.double()), dict(logprob_out=torch.zeros(3, 16, 8)), dict(theta_out=theta[:, :8]),
                dict(theta_out=theta.half()), dict(theta_out=theta.to("meta")), dict(logits=grid[0]), dict(resp=resp.long()), dict(level=7)):
        a = dict(logits=grid[..., :64], lens=lens, resp=resp, level=0, known=known, logprob_out=lp, theta_out=theta)
        a.update(bad)
        with pytest.raises(_hip.D3PMError):
            _hip.op_nar_draw(a["logits"], a["lens"], a["resp"], a["level"], 0.2, 7, known=a["known"], logprob_out=a["logprob_out"],
                             theta_out=a["theta_out"])
    for bad in (dict(top_k=-1), dict(top_k=65), dict(top_k=1.0), dict(top_k=True), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")),
                dict(top_p="0.9")):
        with pytest.raises(ValueError):
            _hip.op_nar_draw(grid[..., :64], lens, resp, 0, 0.2, 7, **bad)
    assert _hip.nar_draw_struct() is None and _hip.nar_draw_struct(0, 1.0, None, None, None) is None
    assert _hip.nar_draw_struct(1) is not None and _hip.nar_draw_struct(0, 0.5) is not None and _hip.nar_draw_struct(known=known) is not None


def test_forward_validates_its_options_before_it_looks_for_a_device(built_lib):
    """Every ValueError of NAR.forward's options, on a CPU model: the "no CPU path" RuntimeError comes only behind them."""
    from vall_e.vall_e import NAR, synth
    m = NAR(1024, 128, 2, 2)
    texts, proms, resps = synth.make_nar_inputs(2, 1)
    t0, t1 = len(resps[0]), len(resps[1])
    known = [torch.zeros(t0, 8, dtype=torch.long), torch.zeros(t1, 8, dtype=torch.long)]
    mask = [torch.zeros(t0, dtype=torch.bool), torch.ones(t1, dtype=torch.bool)]
    bad_calls = [
        dict(known=known),                                                     # a known without a mask
        dict(known_mask=mask),
        dict(known=known[:1], known_mask=mask),                                # list lengths
        dict(known=known, known_mask=mask[:1]),
        dict(known=[known[0][:, :7], known[1]], known_mask=mask),              # shapes
        dict(known=[known[0][:-1], known[1]], known_mask=mask),
        dict(known=[known[0].float(), known[1]], known_mask=mask),
        dict(known=[known[0][:, 0], known[1]], known_mask=mask),
        dict(known=known, known_mask=[mask[0][:-1], mask[1]]),
        dict(known=known, known_mask=[mask[0].long(), mask[1]]),
        dict(known=known, known_mask=[mask[0][:, None], mask[1]]),
        dict(top_k=-1), dict(top_k=1025), dict(top_k=2.0), dict(top_k=True),
        dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.01), dict(top_p=float("nan")), dict(top_p=float("inf")), dict(top_p="1"),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            m(texts, proms, resps, **kw)
    with pytest.raises(ValueError):
        m(texts[:1], proms, resps, top_k=5)                                    # list lengths of the inputs themselves
    # the options do not go with the 8-level training call
    _, _, resps8 = synth.make_nar_inputs(2, 1, n_levels=8)
    for kw in (dict(top_k=5), dict(top_p=0.5), dict(known=known, known_mask=mask), dict(return_logprobs=True)):
        with pytest.raises(ValueError, match="training call"):
            m(texts, proms, resps8, **kw)
    # valid options get as far as the device check, and so does a call without any
    for kw in (dict(top_k=50, top_p=0.9, known=known, known_mask=mask, return_logprobs=True), dict(top_k=1024), dict(top_p=1e-6), {}):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(texts, proms, resps, **kw)


def test_dp_helper_refuses_what_it_cannot_return():
    from vall_e.vall_e import dp

    class Stub:
        n_resp_levels, n_tokens = 7, 1024

        class cfg:
            n_frames = 4
    for kw in (dict(return_logprobs=True), dict(return_logits_level=0)):
        with pytest.raises(ValueError, match="codes alone"):
            dp.generate_codes_dp(Stub, Stub, [torch.zeros(1)], [torch.zeros(1, 8)], seed=1, nar_kw=kw)


# ---- the reference on the inputs of the GPU tests -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tokens", [1024, 37])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_reference_satisfies_the_invariants_of_the_definition(dtype, n_tokens):
    grid = R.without_dead_rows(R.draw_inputs(n_tokens, dtype), n_tokens)
    rows = torch.cat([R.draw_rows(grid, b, n_tokens) for b in range(3)])[::3]      # every third frame: all kinds of rows
    v = R.values(rows, 0.2)
    # order keys: monotone in the value, and equal exactly where the bit patterns are equal
    key = R.order_key(v, dtype)
    a, k = v.numpy()[:64].ravel(), key[:64].ravel()
    order = np.argsort(k, kind="stable")
    a, k = a[order], k[order]
    assert (a[1:] >= a[:-1]).all()
    assert ((k[1:] == k[:-1]) <= (a[1:] == a[:-1])).all()
    for top_k in (1, 2, 50, n_tokens):
        if top_k > n_tokens:
            continue
        t1 = R.theta1(v, top_k)
        vp = R.cut(v, t1)
        assert bool(((v >= torch.as_tensor(t1)[:, None]).sum(-1) >= top_k).all()), top_k      # ties at theta1 are all kept
        assert bool((torch.isfinite(vp).sum(-1) >= torch.isfinite(v).sum(-1).clamp(max=top_k)).all()), top_k
        assert bool((vp.max(-1).values == v.max(-1).values).all())
    for top_k in (0, 50):
        if top_k > n_tokens:
            continue
        vp = R.cut(v, R.theta1(v, top_k))
        p = R.softmax64(vp)
        slack = n_tokens / 2.0 ** 20 + 2.0 ** -20
        for top_p in (0.9, 0.5, 1.0 / 2048, 1.0 / 1280):
            theta = R.theta_nucleus(vp, top_p, dtype)
            assert bool((vp == torch.as_tensor(theta)[:, None]).any(-1).all()), "theta is a value of the row"
            vpp = R.cut(vp, theta)
            assert bool((vpp.max(-1).values == vp.max(-1).values).all())          # the maximum is always kept
            keep, above = (vpp > -np.inf).numpy(), (vp > torch.as_tensor(theta)[:, None]).numpy()
            p32 = float(np.float32(top_p))
            assert ((p * keep).sum(-1) >= p32 - slack).all() and ((p * above).sum(-1) < p32 + slack).all(), (top_k, top_p)
            if top_p <= 1.0 / 1280:
                assert bool(((vpp > -np.inf) == (vp == vp.max(-1, keepdim=True).values)).all())      # exactly the classes tied at the maximum
        assert np.isneginf(R.theta_nucleus(vp, 1.0, dtype)).all()
    lp = R.log_softmax64(rows)
    live = torch.isfinite(rows.float()).numpy()
    assert np.isfinite(lp[live]).all() and np.allclose(np.exp(lp).sum(-1), 1.0, atol=1e-12)

"""Classifier-free guidance in the NAR stage: what can be checked without a GPU (include/d3pm_hip.h: d3pm_nar_level_guided,
d3pm_op_nar_draw_guided).  The entries are declared, bound and exported at ABI version 6; every refusal returns its code through the
built library BEFORE anything is launched (every pointer handed over below is a made-up address); NAR.forward raises its ValueErrors
before it looks for a device; the twin packing is host-only; the cond_drop hook of NAR.forward_backward decides as
guidance_ref.cond_drop_mirror does; the host reference of the GPU tests (tests/nar_guidance_ref.py) is exact on its own inputs."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import guidance_ref as G
import nar_guidance_ref as R
from conftest import ROOT

NAMES = ("d3pm_nar_level_guided", "d3pm_op_nar_draw_guided")


def _header():
    return open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()


def _codes():
    return {name: int(value) for name, value in re.findall(r"\b(D3PM_E_[A-Z]+)\s*=\s*(-?\d+)", _header())}


def test_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = _header()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name, base in zip(NAMES, ("d3pm_nar_level_draw", "d3pm_op_nar_draw")):
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
        params = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(_hip.SIGNATURES[name][1]) == params.count(",") + 1, name
        assert re.search(r"const d3pm_nar_draw \*draw, const d3pm_guidance \*guidance,\s+void \*stream", params), name
        new, old = _hip.SIGNATURES[name][1], _hip.SIGNATURES[base][1]      # the entry it generalises plus the one pointer
        assert _hip.SIGNATURES[name][0] is C.c_int and new[:-2] == old[:-1] and new[-1] == old[-1] and new[-2] == C.POINTER(_hip.Guidance), name
    assert "#define D3PM_ABI_VERSION 6" in header and built_lib.d3pm_abi_version() == 6


def _draw(lib, draw, guide, **kw):
    a = dict(dtype=2, logits=0x100000, ldl=1032, lens=0x200000, resp=0x300000, tr_max=704, resp_stride=8, t_max=704, n_tokens=1024,
             level=0, temperature=0.2, seed=7, utt0=0, flags=0, batch=3)
    a.update(kw)
    return lib.d3pm_op_nar_draw_guided(a["dtype"], a["logits"], a["ldl"], a["lens"], a["resp"], a["tr_max"], a["resp_stride"], a["t_max"],
                                       a["n_tokens"], a["level"], a["temperature"], a["seed"], a["utt0"], a["flags"], a["batch"],
                                       None if draw is None else C.byref(draw), None if guide is None else C.byref(guide), None)


def test_draw_entry_refuses_before_any_launch(built_lib):
    from vall_e.vall_e import _hip
    codes = _codes()
    arg, shape = codes["D3PM_E_ARG"], codes["D3PM_E_SHAPE"]
    ok, g = _hip.NarDraw(0.9, 50, None, 0x400000, None), _hip.Guidance(1.5)
    # the guidance itself: a NULL struct, a negative or non-finite weight -- with and without draw options
    for draw in (ok, None):
        assert _draw(built_lib, draw, None) == arg and b"d3pm_guidance" in built_lib.d3pm_last_error()
        for bad in (-0.5, -1e-30, float("nan"), float("inf"), float("-inf")):
            assert _draw(built_lib, draw, _hip.Guidance(bad)) == arg, bad
            assert b"weight" in built_lib.d3pm_last_error()
    # anything the draw with options refuses
    for name in ("logits", "lens", "resp"):
        assert _draw(built_lib, ok, g, **{name: None}) == arg, name
    for name in ("batch", "t_max", "tr_max", "n_tokens"):
        for bad in (0, -1):
            assert _draw(built_lib, ok, g, **{name: bad}) == arg, (name, bad)
    assert _draw(built_lib, ok, g, ldl=1023) == arg and _draw(built_lib, ok, g, level=7) == arg and _draw(built_lib, ok, g, dtype=5) == arg
    for draw in (ok, None):
        for bad in (0.0, -0.2, float("nan"), float("inf")):
            assert _draw(built_lib, draw, g, temperature=bad) == arg, bad
    for bad in (-1, 1025, 2 ** 31 - 1):
        assert _draw(built_lib, _hip.NarDraw(1.0, bad, None, None, None), g) == arg, bad
        assert b"top_k" in built_lib.d3pm_last_error()
    for bad in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert _draw(built_lib, _hip.NarDraw(bad, 0, None, None, None), g) == arg, bad
        assert b"top_p" in built_lib.d3pm_last_error()
    # more tokens than a wave's registers hold: under guidance every draw is the kernel with the limit, options or none
    for draw in (ok, None, _hip.NarDraw(1.0, 0, None, None, None)):
        assert _draw(built_lib, draw, g, n_tokens=1284, ldl=1284) == shape
    # a weight of 0 is legal here: with these made-up addresses the only thing left to check is that no argument check fires first
    assert _draw(built_lib, ok, _hip.Guidance(0.0), n_tokens=1284, ldl=1284) == shape


def _level(lib, shape, weights, draw, guide, **kw):
    a = dict(batch=2, t_max=64, lens=0x200000, text=0x210000, tt_max=16, prom=0x220000, tp_max=32, resp=0x300000, tr_max=44, level=0,
             temperature=0.2, seed=7, utt0=0, flags=0, ws=0x1000000, ws_bytes=1 << 40, logits_out=None)
    a.update(kw)
    return lib.d3pm_nar_level_guided(None if shape is None else C.byref(shape), None if weights is None else C.byref(weights), a["batch"],
                                     a["t_max"], a["lens"], a["text"], a["tt_max"], a["prom"], a["tp_max"], a["resp"], a["tr_max"], a["level"],
                                     a["temperature"], a["seed"], a["utt0"], a["flags"], a["ws"], a["ws_bytes"], a["logits_out"],
                                     None if draw is None else C.byref(draw), None if guide is None else C.byref(guide), None)


def test_level_entry_refuses_before_any_launch(built_lib):
    from vall_e.vall_e import _hip
    codes = _codes()
    arg, shape_code, ws_code = codes["D3PM_E_ARG"], codes["D3PM_E_SHAPE"], codes["D3PM_E_WORKSPACE"]
    sh = _hip.NarShape(128, 2, 2, 1024, 8, 7, 2, None)
    blocks = (_hip.NarBlockWeights * 2)()
    for blk in blocks:
        for field, _ in _hip.NarBlockWeights._fields_:
            setattr(blk, field, 0x500000)
    w = _hip.NarWeights(0x600000, 0x610000, 0x620000, 0x630000, 0x640000, 0x650000, 0x660000, 2048, blocks)
    ok, g = _hip.NarDraw(0.9, 50, None, 0x400000, None), _hip.Guidance(1.5)
    for draw in (ok, None):
        assert _level(built_lib, sh, w, draw, None) == arg and b"d3pm_guidance" in built_lib.d3pm_last_error()
        for bad in (-0.5, float("nan"), float("inf")):
            assert _level(built_lib, sh, w, draw, _hip.Guidance(bad)) == arg, bad
        for bad in (0.0, -0.2, float("nan"), float("inf")):
            assert _level(built_lib, sh, w, draw, g, temperature=bad) == arg, bad
    assert _level(built_lib, sh, w, _hip.NarDraw(1.0, 1025, None, None, None), g) == arg
    assert _level(built_lib, sh, w, _hip.NarDraw(0.0, 0, None, None, None), g) == arg
    assert _level(built_lib, None, w, ok, g) == arg and _level(built_lib, sh, None, ok, g) == arg
    for name in ("lens", "text", "prom", "resp", "ws"):
        assert _level(built_lib, sh, w, ok, g, **{name: None}) == arg, name
    for name in ("batch", "t_max"):
        assert _level(built_lib, sh, w, ok, g, **{name: 0}) == arg, name
    assert _level(built_lib, sh, w, ok, g, level=7) == arg
    wide = _hip.NarShape(128, 2, 2, 1284, 8, 7, 2, None)
    for draw in (ok, None):
        assert _level(built_lib, wide, w, draw, g) == shape_code
    # the workspace is that of 2 * batch utterances: what suffices for `batch` is refused, for a weight of 0 as well
    one = built_lib.d3pm_nar_workspace_bytes(C.byref(sh), 2, 64)
    two = built_lib.d3pm_nar_workspace_bytes(C.byref(sh), 4, 64)
    assert 0 < one < two
    for guide in (g, _hip.Guidance(0.0)):
        assert _level(built_lib, sh, w, ok, guide, ws_bytes=one) == ws_code
        assert _level(built_lib, sh, w, None, guide, ws_bytes=two - 1) == ws_code


def test_python_wrappers_check_their_tensors(built_lib):
    from vall_e.vall_e import _hip
    grid = torch.zeros(4, 20, 64, dtype=torch.bfloat16)
    lens = torch.zeros(4, 3, dtype=torch.int32)
    resp = torch.zeros(4, 16, 8, dtype=torch.int32)
    known, lp, theta = torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(2, 16, 7), torch.zeros(2, 16)
    for bad in (dict(known=torch.zeros(4, 16, dtype=torch.uint8)), dict(logprob_out=torch.zeros(4, 16, 7)), dict(theta_out=torch.zeros(4, 16)),
                dict(logits=grid[:3]), dict(resp=resp[:2]), dict(lens=lens[:2]), dict(level=7)):
        a = dict(logits=grid, lens=lens, resp=resp, level=0, known=known, logprob_out=lp, theta_out=theta)
        a.update(bad)
        with pytest.raises(_hip.D3PMError):
            _hip.op_nar_draw_guided(a["logits"], a["lens"], a["resp"], a["level"], 0.2, 7, 1.5, known=a["known"], logprob_out=a["logprob_out"],
                                    theta_out=a["theta_out"])
    for bad in (-1.0, float("nan"), float("inf"), "2", True, None):
        with pytest.raises(ValueError):
            _hip.op_nar_draw_guided(grid, lens, resp, 0, 0.2, 7, bad)
    with pytest.raises(ValueError):
        _hip.op_nar_draw_guided(grid, lens, resp, 0, 0.2, 7, 1.5, top_k=65)


def test_forward_validates_guidance_before_it_looks_for_a_device(built_lib):
    from vall_e.vall_e import NAR, synth
    m = NAR(1024, 128, 2, 2)
    texts, proms, resps = synth.make_nar_inputs(2, 1)
    p = inspect.signature(NAR.forward).parameters
    assert p["guidance"].default == 0.0 and p["null_text_list"].default is None and p["null_proms_list"].default is None
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("guidance", "null_text_list", "null_proms_list"))
    bad_calls = [
        dict(guidance=-1.0), dict(guidance=float("nan")), dict(guidance=float("inf")), dict(guidance="2"), dict(guidance=True),
        dict(null_text_list=texts),                                            # null lists without guidance
        dict(null_proms_list=proms),
        dict(guidance=0.0, null_text_list=texts, null_proms_list=proms),
        dict(guidance=1.5, null_text_list=texts[:1]),                          # null lists of the wrong length
        dict(guidance=1.5, null_proms_list=proms + proms),
        dict(guidance=1.5, top_k=-1), dict(guidance=1.5, top_p=0.0),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            m(texts, proms, resps, **kw)
    with pytest.raises(ValueError):
        m(texts[:1], proms, resps, guidance=1.5)                               # list lengths of the inputs themselves
    _, _, resps8 = synth.make_nar_inputs(2, 1, n_levels=8)
    with pytest.raises(ValueError, match="training call"):
        m(texts, proms, resps8, guidance=1.5)
    # valid options get as far as the device check, and so does guidance = 0
    for kw in (dict(guidance=1.5), dict(guidance=2, null_text_list=texts, null_proms_list=proms), dict(guidance=0.5, top_k=50, top_p=0.9,
               return_logprobs=True), dict(guidance=0.0), dict(guidance=0)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(texts, proms, resps, **kw)


def test_twin_packing_is_host_only():
    from vall_e.vall_e import NAR, synth
    from vall_e.vall_e.nar import guidance_twins
    texts, proms, resps = synth.make_nar_inputs(3, 1)
    t2, p2, r2 = guidance_twins(texts, proms, resps)
    want = R.twins(texts, proms, resps)
    assert len(t2) == len(p2) == len(r2) == 6
    for got, ref in zip((t2, p2, r2), want):
        assert all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(got, ref))
    for b in range(3):
        assert t2[3 + b].shape == (0,) and p2[3 + b].shape == (0, 8) and r2[3 + b] is resps[b], "an empty text, an empty prompt, the same response"
        assert t2[b] is texts[b] and p2[b] is proms[b]
    # caller-given twins are used as they are
    t2, p2, _ = guidance_twins(texts, proms, resps, null_text_list=texts[::-1], null_proms_list=None)
    assert all(t2[3 + b] is texts[2 - b] for b in range(3)) and all(p2[3 + b].shape == (0, 8) for b in range(3))
    for kw in (dict(null_text_list=texts[:2]), dict(null_proms_list=proms[:1])):
        with pytest.raises(ValueError):
            guidance_twins(texts, proms, resps, **kw)
    # the grids of the 2 B lists: the lengths, the duplicated responses, and index arrays that are never empty
    m = NAR(1024, 128, 2, 2)
    known = [torch.full((len(r), 8), 7, dtype=torch.long) for r in resps]
    held = [torch.cat([r, k[:, 1:]], dim=1) for r, k in zip(resps, known)]        # what forward puts into the levels to come
    lens, text, prom, resp, t_max, lens_host = m._pack(*guidance_twins(texts, proms, held))
    assert lens_host == [(len(t), len(p), len(r)) for t, p, r in zip(texts, proms, resps)] + [(0, 0, len(r)) for r in resps]
    assert lens.tolist() == [list(x) for x in lens_host] and resp.shape[0] == 6 and t_max >= max(sum(x) for x in lens_host) + 2
    assert torch.equal(resp[:3], resp[3:]) and bool((resp[0, : len(resps[0]), 1:] == 7).all()), "responses and known codes in both halves"
    lens, text, prom, resp, t_max, lens_host = m._pack([t[:0] for t in texts], [p[:0] for p in proms], resps)
    assert text.shape == (3, 1) and prom.shape == (3, 1, 8) and lens_host == [(0, 0, len(r)) for r in resps]
    assert t_max >= max(len(r) for r in resps) + 2


def test_cond_drop_decisions_are_the_mirrors(monkeypatch):
    """The hook is host code around train.cond_drop_decision, which draws through d3pm_uniform on the device: here the decision is
    replaced by its numpy mirror and the wiring is checked -- keyed by (seed, utt0 + b), the text and the prompt decided apart."""
    from vall_e.vall_e import NAR, nar, synth, train
    assert "cond_drop" in inspect.signature(NAR.forward_backward).parameters
    assert inspect.signature(NAR.forward_backward).parameters["cond_drop"].default == 0.0
    texts, proms, _ = synth.make_nar_inputs(6, 1)
    asked = []

    def mirror(seed, utt, p_text, p_prompt, device):
        asked.append((seed, utt))
        return G.cond_drop_mirror(seed, utt, p_text, p_prompt)
    monkeypatch.setattr(train, "cond_drop_decision", mirror)
    for cond_drop, seed, utt0 in ((0.5, 11, 40), ((0.3, 0.7), 5, 0), ((1.0, 0.0), 2, 9), (1, 3, 1)):
        asked.clear()
        t2, p2, dropped = nar.cond_drop_lists(texts, proms, seed, utt0, cond_drop, "cpu")
        pt, pp = train.cond_drop_probs(cond_drop)
        assert asked == [(seed, utt0 + b) for b in range(6)]
        assert dropped == [G.cond_drop_mirror(seed, utt0 + b, pt, pp) for b in range(6)]
        for b, (dt, dpr) in enumerate(dropped):
            assert (t2[b].shape == (0,)) if dt else (t2[b] is texts[b]), b
            assert (p2[b].shape == (0, 8)) if dpr else (p2[b] is proms[b]), b
    assert {d for d in dropped} == {(True, True)}
    mixed = nar.cond_drop_lists(texts, proms, 11, 40, 0.5, "cpu")[2]
    assert len(set(mixed)) > 1, "six utterances at p = 0.5 with one decision: choose another seed"
    # the arguments go through train.cond_drop_probs: a bad one is a ValueError before any GPU work, on a CPU model
    m = NAR(1024, 128, 2, 2)
    _, _, resps8 = synth.make_nar_inputs(6, 1, n_levels=8)
    for bad in (True, -0.1, 1.5, (0.1,), "0.1", float("nan")):
        with pytest.raises(ValueError):
            m.forward_backward(texts, proms, resps8, cond_drop=bad)
    for fine in (0, 0.0, False, None, 0.5):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.forward_backward(texts, proms, resps8, cond_drop=fine)


def test_cli_flag_needs_the_nar_checkpoint(tmp_path):
    from vall_e import __main__ as cli
    for argv in (["--nar-guidance", "2"], ["--nar-guidance", "-1", "--nar-ckpt", str(tmp_path / "nar.pt")],
                 ["--nar-guidance", "nan", "--nar-ckpt", str(tmp_path / "nar.pt")]):
        with pytest.raises(SystemExit):
            cli.main([str(tmp_path / "out.qnt.pt")] + argv)


def test_dp_helper_cuts_the_null_lists_to_the_shard():
    from vall_e.vall_e import dp
    texts = [torch.arange(3 + b) for b in range(3)]
    proms = [torch.zeros(5 + b, 8, dtype=torch.long) for b in range(3)]
    seen = []

    class Stub:
        n_resp_levels, n_tokens, device = 7, 1024, torch.device("cpu")

        class cfg:
            n_frames = 4

    def ar_fn(t, p, **kw):
        return torch.zeros(len(t), 4, dtype=torch.long)

    def nar_fn(t, p, r, **kw):
        seen.append(kw)
        return [torch.zeros(4, 8, dtype=torch.long) for _ in t]
    nar_kw = dict(guidance=1.5, null_text_list=texts, null_proms_list=proms, top_k=5)
    out = dp.generate_codes_dp(Stub, Stub, texts, proms, seed=1, nar_kw=nar_kw, ar_fn=ar_fn, nar_fn=nar_fn)
    assert out.shape == (3, 4, 8) and seen[0]["guidance"] == 1.5 and seen[0]["top_k"] == 5 and seen[0]["utt0"] == 0
    assert all(a is b for a, b in zip(seen[0]["null_text_list"], texts)) and len(seen[0]["null_proms_list"]) == 3
    assert dp._shard_kwargs(nar_kw, 1, 3)["null_text_list"] == texts[1:] and dp._shard_kwargs(nar_kw, 1, 3)["guidance"] == 1.5
    assert len(dp._shard_kwargs(nar_kw, 1, 2)["null_proms_list"]) == 1


def test_draw_kernels_have_no_scratch():
    """hipcc's resource remarks for the draw file: the nine plain instantiations and the nine guided ones, none with scratch."""
    import subprocess
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "d3pm_nar_draw.hip"], capture_output=True, text=True,
                         check=True).stdout
    rows = [ln for ln in out.splitlines() if "VGPR" in ln]
    assert len(rows) == 18, out      # 3 dtypes x 3 filter arms, plain and guided
    for ln in rows:
        assert re.search(r"scratch\s+0\b", ln), ln


# ---- the reference on the inputs of the GPU tests -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_reference_is_exact_and_the_crafted_rows_separate_the_halves(dtype):
    assert R.N_LIVE == 12 and [len(R.live_frames(b)) for b in range(2)] == [7, 5]
    assert 7 not in R.live_frames(0) and 5 not in R.live_frames(1), "one frame cut by each half"
    offsets = [(R.LENS[b][0] + R.LENS[b][1], R.LENS[2 + b][0] + R.LENS[2 + b][1]) for b in range(2)]
    assert all(a != b for a, b in offsets), "the two rows of a frame sit at different offsets"
    c, u = R.rows(dtype)
    tdt = torch.float16 if dtype == torch.float32 else dtype
    assert np.array_equal(torch.from_numpy(c).to(tdt).float().numpy(), c) and np.array_equal(torch.from_numpy(u).to(tdt).float().numpy(), u)
    crafted = np.arange(R.N_LIVE) % 4 != 3
    for w in R.WEIGHTS:
        assert G.exact(c, u, w).all() and G.exact_rational(c, u, w), w
        z = R.combine(c, u, w, dtype)
        if dtype != torch.float32:
            assert np.array_equal(torch.from_numpy(z).to(dtype).float().numpy(), z), "z is a value of the storage type"
        zi, ci, ui = z.argmax(-1), c.argmax(-1), u.argmax(-1)
        assert (zi[crafted] != ci[crafted]).all() and (zi[crafted] != ui[crafted]).all(), w
        top2 = np.sort(z[crafted], axis=-1)[:, -2:]
        assert (top2[:, 1] > top2[:, 0]).all(), "no tied maximum on a crafted row (the noise rows may tie: the first class wins)"
    assert np.array_equal(R.combine(c, u, 0.0, dtype), c) and np.array_equal(R.combine(c, c, 3.0, dtype), c)
    g = R.grid(dtype, c, u)
    assert g.shape == (4, R.T_MAX, R.LDL) and g.dtype == dtype and bool((g[..., R.N_TOKENS:].float() > 5e4).all())
    assert np.array_equal(g[0, 9, : R.N_TOKENS].float().numpy(), c[0]) and np.array_equal(g[2, 2, : R.N_TOKENS].float().numpy(), u[0])
    assert np.array_equal(g[1, 5, : R.N_TOKENS].float().numpy(), c[7]) and np.array_equal(g[3, 11, : R.N_TOKENS].float().numpy(), u[7])
    lp = R.log_softmax64(R.combine(c, u, 1.5, dtype))
    assert np.isfinite(lp).all() and np.allclose(np.exp(lp).sum(-1), 1.0, atol=1e-12)

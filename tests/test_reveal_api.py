"""Confidence-ordered reveal (include/d3pm_hip.h: d3pm_reveal), host side: declarations and ctypes signatures, the timestep plan
against tests/reveal_ref.py, every refusal, the numpy selection on crafted scores, and the compile-time claims (no scratch in the new
kernels, the older sampler kernels at the register counts they had).  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import reveal_ref as R

NEW_ENTRIES = ("d3pm_reveal_plan", "d3pm_reveal_step", "d3pm_reveal_loop")
NAN, INF = float("nan"), float("inf")
BAD_CT = [-0.5, -1e-30, NAN, INF, -INF]


def test_reveal_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
    m = re.search(r"typedef struct d3pm_reveal \{([^}]*)\} d3pm_reveal;", header, re.S)
    assert m and re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", m.group(1))).split() == "int32_t n_steps; float choice_temperature;".split()
    assert [(n, t) for n, t in _hip.Reveal._fields_] == [("n_steps", C.c_int32), ("choice_temperature", C.c_float)]
    assert C.sizeof(_hip.Reveal) == 8 and _hip.Reveal.choice_temperature.offset == 4
    assert built_lib.d3pm_abi_version() == 6      # additions only
    version_comment = header.split("#define D3PM_ABI_VERSION")[0]
    for word in ("d3pm_reveal",) + NEW_ENTRIES:
        assert word in version_comment, word
    # the doc string says what happens to padded rows
    assert "NOT \"sampled from" in header and "final.bias" in header
    step = _hip.SIGNATURES["d3pm_reveal_step"][1]
    assert step[-5:] == [C.POINTER(_hip.Nucleus), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p] and len(step) == 19
    loop = _hip.SIGNATURES["d3pm_reveal_loop"][1]
    assert loop[-3:] == [C.POINTER(_hip.Nucleus), C.POINTER(_hip.Reveal), C.c_void_p] and len(loop) == 19


@pytest.mark.parametrize("T", [100, 200, 50])
def test_plan_against_the_reference(built_lib, T):
    from vall_e.vall_e import _hip
    sched = _hip.Schedule(T)
    cbar = R.cbar_f32(sched.cbar)
    assert (np.diff(cbar) >= 0).all(), "cbar is monotone"
    for N in (1, 2, 8, 16, T // 2, T - 2, T - 1):
        out = (C.c_int32 * N)()
        assert built_lib.d3pm_reveal_plan(C.byref(sched.c_struct), N, out) == 0
        ts = R.timesteps(T, N)
        assert list(out) == ts[:-1] and ts[-1] == 0
        assert ts[0] == T - 1 and ts[N - 1] >= 1 and all(a > b for a, b in zip(ts, ts[1:])), "strictly decreasing, T-1 first, >= 1 last"
        # the quota: the masked count reaches 0 only at the end, and never grows
        for F in (1, 5, 64, 448, 750, 1024):
            counts = R.plan(F, F, cbar, T, N)
            assert counts[-1] == 0 and all(a >= b for a, b in zip([F] + counts, counts)), (T, N, F, counts)
    N = T - 1
    out = (C.c_int32 * N)()
    assert built_lib.d3pm_reveal_plan(C.byref(sched.c_struct), N, out) == 0 and list(out) == list(range(T - 1, 0, -1))
    for N in (0, -1, T, T + 5):
        assert built_lib.d3pm_reveal_plan(C.byref(sched.c_struct), N, (C.c_int32 * 4)()) == -1 and b"n_steps" in built_lib.d3pm_last_error()
    assert built_lib.d3pm_reveal_plan(None, 4, (C.c_int32 * 4)()) == -1
    if T == 100:
        revealed = -np.diff([750] + R.plan(750, 750, cbar, 100, 16))
        print("F = 750, N = 16 reveals per step:", list(revealed))
        assert revealed.sum() == 750 and revealed.min() >= 1


def _shape(n_q=1, canvas=None):
    from vall_e.vall_e import _hip, synth
    sh = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
    sh.n_q = n_q
    if canvas is not None:
        sh.canvas = canvas
    return sh


def _step(lib, sh, sched, ct=0.0, nu=None, t=40, t_next=20, frame_mask=None, canvas=None, flags=0):
    return lib.d3pm_reveal_step(C.byref(sh), 1, None, 1, None, None, frame_mask, canvas, t, t_next, C.byref(sched.c_struct), 0, 0, flags,
                                None if nu is None else C.byref(nu), ct, None, None, None)


def _loop(lib, sh, sched, rv, nu=None, frame_mask=None, canvas=None, flags=0):
    return lib.d3pm_reveal_loop(C.byref(sh), None, 1, None, frame_mask, canvas, None, None, None, C.byref(sched.c_struct), 0, 0, flags, None, 0,
                                None, None if nu is None else C.byref(nu), None if rv is None else C.byref(rv), None)


def test_c_entries_refuse_bad_values_with_nothing_launched(built_lib):
    """Every refusal comes back with all pointers still NULL: values are checked before pointers, long before a launch."""
    from vall_e.vall_e import _hip
    lib, sched, sh = built_lib, _hip.Schedule(100), _shape()
    dummy = C.c_uint8(1)
    fm = C.addressof(dummy)
    for ct in BAD_CT:
        assert _step(lib, sh, sched, ct, frame_mask=fm) == -1 and b"choice_temperature" in lib.d3pm_last_error()
        assert _loop(lib, sh, sched, _hip.Reveal(16, ct), frame_mask=fm) == -1 and b"choice_temperature" in lib.d3pm_last_error()
    for n in (0, -3, 100, 1000):
        assert _loop(lib, sh, sched, _hip.Reveal(n, 0.0), frame_mask=fm) == -1 and b"n_steps" in lib.d3pm_last_error()
    assert _loop(lib, sh, sched, None, frame_mask=fm) == -1
    # n_q > 1 and canvas > 1024: D3PM_E_SHAPE
    assert _step(lib, _shape(n_q=8), sched, frame_mask=fm) == -4 and b"n_q" in lib.d3pm_last_error()
    assert _loop(lib, _shape(n_q=8), sched, _hip.Reveal(16, 0.0), frame_mask=fm) == -4 and b"n_q" in lib.d3pm_last_error()
    assert _step(lib, _shape(canvas=1025), sched, frame_mask=fm) == -4 and b"canvas" in lib.d3pm_last_error()
    assert _loop(lib, _shape(canvas=1025), sched, _hip.Reveal(16, 0.0), frame_mask=fm) == -4 and b"canvas" in lib.d3pm_last_error()
    # the sampling triple is checked as everywhere
    assert _step(lib, sh, sched, nu=_hip.Nucleus(0.0, 0, 1.0), frame_mask=fm) == -1 and b"temperature" in lib.d3pm_last_error()
    assert _loop(lib, sh, sched, _hip.Reveal(4, 0.0), nu=_hip.Nucleus(1.0, 0, 1.5), frame_mask=fm) == -1 and b"top_p" in lib.d3pm_last_error()
    # timesteps of a step: T > t > t_next >= 0
    for t, tn in ((0, 0), (100, 50), (40, 40), (40, 41), (40, -1)):
        assert _step(lib, sh, sched, t=t, t_next=tn, frame_mask=fm) == -1
    # the seed-in-HBM flag belongs to the captured loop
    assert _step(lib, sh, sched, frame_mask=fm, flags=4) == -1 and _loop(lib, sh, sched, _hip.Reveal(4, 0.0), frame_mask=fm, flags=4) == -1
    # good values get as far as the mask / pointer checks
    cv = _hip.Canvas(fm, None)
    for ct in (0.0, 4.5):
        assert _step(lib, sh, sched, ct) == -1 and b"exactly one of" in lib.d3pm_last_error()
        assert _step(lib, sh, sched, ct, frame_mask=fm, canvas=C.byref(cv)) == -1 and b"exactly one of" in lib.d3pm_last_error()
        assert _step(lib, sh, sched, ct, frame_mask=fm) == -1 and b"null pointer" in lib.d3pm_last_error()
        assert _step(lib, sh, sched, ct, t=1, t_next=0, canvas=C.byref(cv)) == -1 and b"null pointer" in lib.d3pm_last_error()
        for n in (1, 16, 99):
            assert _loop(lib, sh, sched, _hip.Reveal(n, ct)) == -1 and b"exactly one of" in lib.d3pm_last_error()
            assert _loop(lib, sh, sched, _hip.Reveal(n, ct), frame_mask=fm) == -1 and b"null pointer" in lib.d3pm_last_error()


def test_reveal_options_helper():
    from vall_e.vall_e import _hip
    assert _hip.reveal_options(None) is None and _hip.reveal_options(None, 0.0, 100) is None
    r = _hip.reveal_options(16, 4.5, 100)
    assert type(r) is _hip.Reveal and (r.n_steps, r.choice_temperature) == (16, 4.5)
    assert _hip.reveal_options(99, 0, 100).n_steps == 99 and _hip.reveal_options(1).n_steps == 1
    for n in (0, -1, 100, 1.5, "16", True, [16]):
        with pytest.raises(ValueError, match="reveal_steps"):
            _hip.reveal_options(n, 0.0, 100)
    for ct in BAD_CT + [True, "1", None, 1e60]:
        with pytest.raises(ValueError, match="choice_temperature"):
            _hip.reveal_options(16, ct, 100)
    with pytest.raises(ValueError, match="choice_temperature"):
        _hip.reveal_options(None, 1.0, 100)


_T = [torch.tensor([1, 2, 3])] * 2
_P = [torch.zeros(4, 8, dtype=torch.long)] * 2


def _native():
    from vall_e.vall_e import AR
    return AR.reference_native()          # parameters on the CPU


@pytest.mark.parametrize("kw", [dict(reveal_steps=n) for n in (0, -1, 100, 2.5, "8", True)] + [dict(reveal_steps=16, choice_temperature=c) for c in BAD_CT] + [
    dict(choice_temperature=1.0), dict(reveal_steps=16, steps=10), dict(reveal_steps=16, graph=True), dict(reveal_steps=16, fp8=True),
    dict(reveal_steps=16, top_p=0.0), dict(reveal_steps=16, temperature=0.0), dict(reveal_steps=16, top_k=-1),
], ids=repr)
def test_generate_audio_rejects_bad_options_on_the_host(kw):
    """ValueError before anything touches the GPU: the model lives on the CPU here, and a valid call would raise the RuntimeError of a
    missing HIP device instead."""
    with pytest.raises(ValueError):
        _native().generate_audio(_T, _P, **kw)


def test_generate_audio_rejects_an_nq_model_on_the_host():
    from vall_e.vall_e import AR, synth
    import dataclasses
    cfg = dataclasses.replace(synth.D3PMConfig.native(), n_q=8)
    with pytest.raises(ValueError, match="n_q"):
        AR.from_config(cfg).generate_audio(_T, _P, reveal_steps=16)


def test_valid_options_reach_the_device_check():
    m = _native()
    for kw in (dict(reveal_steps=16), dict(reveal_steps=1), dict(reveal_steps=99, choice_temperature=4.5), dict(reveal_steps=8, greedy=True),
               dict(reveal_steps=16, top_p=0.9, temperature=0.7, top_k=50), dict(reveal_steps=16, streams=2, return_trace=True),
               dict(reveal_steps=16, n_frames=[10, 448], known=[torch.tensor([1, 512]), None])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.generate_audio(_T, _P, **kw)


def test_signatures_take_the_two_arguments():
    from vall_e.vall_e import AR, _hip
    p = inspect.signature(AR.generate_audio).parameters
    assert p["reveal_steps"].default is None and p["choice_temperature"].default == 0.0
    assert p["reveal_steps"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (_hip.Sampler.reveal_step, _hip.Sampler.reveal_loop):
        q = inspect.signature(fn).parameters
        assert q["choice_temperature"].default == 0.0 and q["top_p"].default == 1.0 and q["known"].default is None
    assert "final.bias" in AR.generate_audio.__doc__ and "reveal_steps" in AR.generate_audio.__doc__


def test_cli_parses_the_flags(monkeypatch, tmp_path):
    """--reveal-steps / --choice-temperature reach generate_audio; a bad value is an argparse error before any model is built."""
    from vall_e import __main__ as cli
    from vall_e.vall_e import AR
    seen = {}

    class Stop(Exception):
        pass

    def fake(self, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(AR, "generate_audio", fake)
    monkeypatch.setattr(AR, "to", lambda self, *a, **k: self)
    qnt = tmp_path / "p.qnt.pt"
    torch.save(torch.zeros(1, 8, 4, dtype=torch.long), qnt)
    base = [str(tmp_path / "o.qnt.pt"), "--phonemes", "1 2 3", "--prompt-qnt", str(qnt), "--native", "--device", "cpu"]
    with pytest.raises(Stop):
        cli.main(base + ["--reveal-steps", "16", "--choice-temperature", "4.5"])
    assert seen["reveal_steps"] == 16 and seen["choice_temperature"] == 4.5
    seen.clear()
    with pytest.raises(Stop):
        cli.main(base)
    assert seen["reveal_steps"] is None and seen["choice_temperature"] == 0.0
    for bad in (["--reveal-steps", "0"], ["--reveal-steps", "8", "--choice-temperature", "-1"], ["--choice-temperature", "2"]):
        with pytest.raises(SystemExit):
            cli.main(base + bad)


def test_dp_forwards_the_two_arguments():
    from vall_e.vall_e import dp
    got = {}

    class M:
        class cfg:
            canvas, n_q = 4, 1
        device = "cpu"

        def generate_audio(self, texts, proms, **kw):
            got.update(kw)
            return torch.zeros(len(texts), 4, dtype=torch.long)

    dp.generate_audio_dp(M(), _T, _P, seed=1, reveal_steps=16, choice_temperature=2.0)
    assert got["reveal_steps"] == 16 and got["choice_temperature"] == 2.0 and got["global_batch"] == 2


# ---- the numpy selection on crafted scores ---------------------------------------------------------------------------------------
def test_order_key_is_monotone():
    v = np.array([-INF, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, INF], dtype=np.float32)
    k = R.order_key(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()


def test_selection_ties_and_quotas():
    masked = np.array([1, 1, 0, 1, 1, 1, 0, 1], bool)
    tie = np.full(8, -2.5, np.float32)
    # all scores tie: the lowest frame indices win
    assert list(R.select(tie, masked, 3)) == [0, 1, 3]
    assert list(R.select(tie, masked, 0)) == []                     # a quota of 0
    assert list(R.select(tie, masked, 6)) == [0, 1, 3, 4, 5, 7]     # the quota that takes every masked row
    assert list(R.select(tie, masked, 9)) == [0, 1, 3, 4, 5, 7]     # larger than the masked count
    s = np.array([-1.0, -3.0, 99.0, -0.5, -3.0, -0.5, 99.0, -7.0], np.float32)      # (unmasked rows carry anything: never picked)
    assert list(R.select(s, masked, 1)) == [3]                      # tie at the top: the lower index
    assert list(R.select(s, masked, 2)) == [3, 5]
    assert list(R.select(s, masked, 4)) == [0, 1, 3, 5]             # tie at the threshold (-3.0): frame 1 before frame 4
    assert list(R.select(s, masked, 5)) == [0, 1, 3, 4, 5]


def test_step_on_the_host_keeps_known_padded_and_revealed_rows():
    mask_id = 512
    x = np.array([[512, 512, 7, 512, 512, 0, 0, 0], [512, 3, 512, 512, 512, 512, 512, 0]], np.int32)
    fm = (np.arange(8)[None] < np.array([5, 7])[:, None]).astype(np.uint8)
    known = np.zeros((2, 8), np.uint8)
    known[0, 2] = 1; known[1, 1] = 1; known[1, 2] = 1          # a known row that still holds the mask id (512 doubles as a codec id)
    cand = np.arange(16, dtype=np.int32).reshape(2, 8) + 100
    score = -np.arange(16, dtype=np.float32).reshape(2, 8)
    # utterance 0: F = 4, masked 4; utterance 1: F = 5, masked 5.  keep_frac 0.5 -> keep 2 / 2 -> reveal 2 / 3
    out = R.step(x, fm, known, cand, score, mask_id, np.float32(0.5))
    assert out.tolist() == [[100, 101, 7, 512, 512, 0, 0, 0], [108, 3, 512, 111, 112, 512, 512, 0]]
    last = R.step(out, fm, known, cand, score, mask_id, np.float32(0.0))
    free = (fm != 0) & (known == 0)
    assert (last[free] != mask_id).all() and (last[~free] == x[~free]).all()
    assert R.quota(750, 750, np.float32(0.999)) == (749, 1) and R.quota(5, 3, np.float32(0.9)) == (3, 0)


# ---- compile time ----------------------------------------------------------------------------------------------------------------
_KERNELS = ("reveal_candidate_rows", "reveal_commit_prep_rows", "reveal_commit_rows", "posterior_sample_prep_rows_filtered",
            "posterior_sample_rows_filtered", "posterior_sample_prep_rows", "posterior_sample_rows", "nucleus_sample_prep_rows", "nucleus_sample_rows")


def _resources(src, flt):
    """kernel name -> [(VGPRs, scratch bytes)] over its instantiations (names the tool could not demangle are matched as substrings)."""
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), src, flt], capture_output=True, text=True, timeout=900).stdout
    res = {}
    for l in out.splitlines():
        m = re.search(r"VGPR\s+(\d+).*scratch\s+(\d+)", l)
        name = next((k for k in _KERNELS if k in l), None)
        if name is None:      # (another kernel of the file that the filter let through)
            continue
        assert m, l
        res.setdefault(name, []).append((int(m.group(1)), int(m.group(2))))
    return res, out


def test_reveal_kernels_have_no_scratch_and_the_sampler_kernels_keep_their_registers():
    """The kernels of d3pm_reveal.hip compile without scratch and at four waves per SIMD or better; d3pm_sample_row.h gained the
    shared row code, and the kernels of d3pm_sample.hip that include it report the register counts they had.  Cross-compiles, no GPU."""
    res, out = _resources("d3pm_reveal.hip", "reveal")
    # 3 dtypes x {known, not} x {plain, filtered}; 2 dtypes x {known, not}; one commit kernel -- each with kRevise off and on
    assert {k: len(v) for k, v in res.items()} == dict(reveal_candidate_rows=24, reveal_commit_prep_rows=8, reveal_commit_rows=2), out[-4000:]
    for name, rows in res.items():
        for vgpr, scratch in rows:
            assert scratch == 0 and vgpr <= 128, (name, vgpr, scratch)
    old, out = _resources("d3pm_sample.hip", "sample")
    assert all(s == 0 for rows in old.values() for _, s in rows)
    v = lambda name: {r[0] for r in old[name]}
    assert v("posterior_sample_rows") == {97} and v("posterior_sample_prep_rows") == {94}, old
    assert v("posterior_sample_rows_filtered") == {96} and v("posterior_sample_prep_rows_filtered") == {95}, old
    assert v("nucleus_sample_rows") == {106} and v("nucleus_sample_prep_rows") == {101}, old

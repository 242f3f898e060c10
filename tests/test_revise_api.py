"""Reveal with revision (include/d3pm_hip.h: d3pm_revise): what can be checked without a GPU
(python -m pytest tests/test_revise_api.py -m "not gpu").
The host reference the GPU tests compare against (tests/revise_ref.py) has the properties the definition states; the entries are
declared, bound and exported; every bad argument is refused before anything touches the GPU; the option travels through the command
line and the data-parallel wrapper; the new kernels compile without scratch."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import revise_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("d3pm_reveal_step_revise", "d3pm_reveal_loop_revise")

_T = [torch.tensor([5, 6, 7]), torch.tensor([8, 9])]
_P = [torch.zeros(4, 8, dtype=torch.long), torch.ones(6, 8, dtype=torch.long)]


def _native():
    from vall_e.vall_e import AR
    return AR.reference_native()


# ---- the host reference ------------------------------------------------------------------------------------------------------------------
def _random_step(seed, canvas=70, B=3, mask_id=512):
    g = np.random.default_rng(seed)
    _, x, fm, known, _ = V.case(1025, canvas, seed, B=B)
    score = g.standard_normal((B, canvas)).astype(np.float32) * 4
    cand = np.where(x == mask_id, g.integers(0, 500, x.shape), x).astype(np.int32)
    return x, fm, known, cand, score


@pytest.mark.parametrize("keep_frac", [0.0, 0.0625, 0.5, 0.96875])
def test_reference_step_holds_the_quota_and_touches_free_rows_only(keep_frac):
    x, fm, known, cand, score = _random_step(3)
    masked, held, free = V.kinds(x, fm, known, 512)
    out = V.step(x, fm, known, cand, score, 512, keep_frac)
    assert np.array_equal(out[~free], x[~free]), "known and padded rows keep x_t"
    for b in range(x.shape[0]):
        F = int(free[b].sum())
        assert int((out[b][free[b]] != 512).sum()) == V.hold_count(F, keep_frac)
        assert int((out[b][free[b]] == 512).sum()) == int(np.floor(F * keep_frac))
        pick = V.select(score[b], free[b], V.hold_count(F, keep_frac))
        rest = np.setdiff1d(np.flatnonzero(free[b]), pick)
        if len(pick) and len(rest):
            assert score[b][pick].min() >= score[b][rest].max(), "the selected rows are the best ones"
    kept = held & (out != 512)
    assert np.array_equal(out[kept], x[kept]), "a selected held row keeps its id"
    took = masked & (out != 512)
    assert np.array_equal(out[took], cand[took]), "a selected masked row takes cand"
    assert V.hold_count(0, keep_frac) == 0 and V.hold_count(70, 0.0) == 70 and V.hold_count(70, 0.5) == 35 and V.hold_count(7, 0.5) == 4


def test_reference_ties_go_to_the_lower_frame():
    free = np.array([1, 1, 0, 1, 1, 1, 0, 1], bool)
    assert V.select(np.zeros(8, np.float32), free, 3).tolist() == [0, 1, 3], "all tie: the lowest free frames"
    s = np.array([1, 2, 9, 2, 2, 0, 9, 2], np.float32)
    assert V.select(s, free, 2).tolist() == [1, 3] and V.select(s, free, 4).tolist() == [1, 3, 4, 7] and V.select(s, free, 5).tolist() == [0, 1, 3, 4, 7]
    assert V.select(s, free, 0).tolist() == [] and V.select(s, free, 99).tolist() == [0, 1, 3, 4, 5, 7]
    assert V.select(np.array([-0.0, 0.0, -1.0], np.float32), np.ones(3, bool), 1).tolist() == [1], "the key orders -0 below +0"


def test_reference_pinned_held_rows_are_remasked_only_under_the_quota():
    x, fm, known, cand, score = _random_step(8)
    masked, held, free = V.kinds(x, fm, known, 512)
    pinned = np.where(held, score + np.float32(1e4), score).astype(np.float32)
    seen = set()
    for keep_frac in (0.25, 0.5, 0.9375):
        out = V.step(x, fm, known, cand, pinned, 512, keep_frac)
        for b in range(x.shape[0]):
            hold, n_held = V.hold_count(int(free[b].sum()), keep_frac), int(held[b].sum())
            remasked = int((held[b] & (out[b] == 512)).sum())
            assert remasked == max(0, n_held - hold), (keep_frac, b)
            seen.add(remasked > 0)
            if hold >= n_held:      # the masked rows then compete for the rest as under d3pm_reveal
                import reveal_ref as R
                assert np.array_equal(out[b], R.step(x[b:b + 1], fm[b:b + 1], known[b:b + 1], cand[b:b + 1], score[b:b + 1], 512, keep_frac)[0])
    assert seen == {False, True}


def test_the_fp64_quota_is_the_integer_one_for_every_cbar_of_the_schedule():
    """floor((double) F * (double) float(cbar)) for all F < 2^20 and all fp16 cbar values of the 100-step table, against integer
    arithmetic on the fp16's significand and exponent."""
    from vall_e.vall_e import _hip
    bits = np.asarray(_hip.Schedule(100).cbar, dtype=np.uint16)
    assert len(bits) == 100
    F = np.arange(1 << 20, dtype=np.int64)
    for hb in np.unique(bits):
        v = float(np.array([hb], dtype=np.uint16).view(np.float16)[0])
        e, m = (int(hb) >> 10) & 31, int(hb) & 1023
        assert (int(hb) >> 15) == 0 and e < 31
        sig, sh = (m, 24) if e == 0 else (m | 1024, 25 - e)      # value = sig * 2^-sh
        assert v == sig / 2.0 ** sh
        want = (F * sig) >> sh
        got = np.floor(F.astype(np.float64) * np.float64(np.float32(v))).astype(np.int64)
        assert np.array_equal(got, want), hex(int(hb))
        assert V.hold_count(1000, np.float32(v)) == 1000 - int(want[1000])


def test_reference_plan_and_last_reveal():
    from vall_e.vall_e import _hip
    cbar = V.cbar_f32(_hip.Schedule(100).cbar)
    for N in (1, 4, 16, 99):
        p = V.plan(448, cbar, 100, N)
        ts = V.timesteps(100, N)
        assert p[-1] == 0 and all(a >= b for a, b in zip(p, p[1:])), "the masked count does not grow"
        assert p[:-1] == [int(np.floor(448 * np.float64(cbar[t]))) for t in ts[1:-1]]
    M = 9
    x0 = np.array([M, M, 3, M, 7, 0])
    free = np.array([1, 1, 1, 1, 0, 0], bool)
    trace = np.array([[1, M, M, M, 7, 0], [M, 2, M, 4, 7, 0], [5, 2, 6, 4, 7, 0]])
    assert V.last_reveal(trace, [99, 50, 1], x0, free, M).tolist() == [1, 50, 1, 50, -1, -1]
    assert V.last_reveal(trace[:1], [99], x0, free, M).tolist() == [99, 0, 0, 0, -1, -1]
    assert V.last_reveal(np.array([[1, 2, 3, 4, 7, 0]]), [99], x0, free, M).tolist() == [99, 99, -1, 99, -1, -1], "never re-masked: -1 stays"


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
    assert "#define D3PM_ABI_VERSION 6" in header and _hip.ABI_VERSION == 6 and built_lib.d3pm_abi_version() == 6
    m = re.search(r"typedef struct d3pm_revise \{([^}]*)\} d3pm_revise;", header, re.S)
    assert m and re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", m.group(1))).split() == "float hold_bonus;".split()
    assert _hip.Revise._fields_ == [("hold_bonus", C.c_float)] and C.sizeof(_hip.Revise) == 4
    version_comment = header.split("#define D3PM_ABI_VERSION")[0]
    for word in ("d3pm_revise",) + NEW_ENTRIES:
        assert word in version_comment, word
    # the step entry is d3pm_reveal_step with revise and the optional scores in front of the stream; the loop entry is
    # d3pm_reveal_loop_scored with revise in front of the scores
    a, b = _hip.SIGNATURES["d3pm_reveal_step_revise"][1], _hip.SIGNATURES["d3pm_reveal_step"][1]
    assert a == b[:-1] + [C.POINTER(_hip.Revise), C.POINTER(_hip.FrameScores), C.c_void_p]
    a, b = _hip.SIGNATURES["d3pm_reveal_loop_revise"][1], _hip.SIGNATURES["d3pm_reveal_loop_scored"][1]
    assert a == b[:-2] + [C.POINTER(_hip.Revise), C.POINTER(_hip.FrameScores), C.c_void_p]
    for words in ("hold = F_b - floor((double) F_b * (double) float(cbar[t_{i+1}]))", "score = (conf_h + hold_bonus) + lambda_i * gumbel(v)",
                  "an unselected held row is re-masked"):
        assert words in header, words


def test_the_c_entries_refuse_on_the_host(built_lib):
    """D3PM_E_ARG with a message for a null d3pm_revise and a bad hold_bonus, and what d3pm_reveal refuses: each check runs before any
    device pointer is read or anything is launched, so it can be exercised with no device at all."""
    from vall_e.vall_e import _hip, synth
    sh = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
    sched = _hip.Schedule(100)
    junk = C.c_void_p(16)
    rv = _hip.Reveal(4, 0.0)

    def step(rs, flags=0, shape=sh, ct=0.0, t=60, t_next=40):
        return built_lib.d3pm_reveal_step_revise(C.byref(shape), 1, junk, _hip.F16, junk, junk, junk, None, t, t_next, C.byref(sched.c_struct), 1, 0,
                                                 flags, None, ct, junk, junk, None if rs is None else C.byref(rs), None, None)

    def loop(rs, flags=0, shape=sh, ct=0.0, n=4):
        r = _hip.Reveal(n, ct)
        return built_lib.d3pm_reveal_loop_revise(C.byref(shape), None, 1, junk, junk, None, junk, junk, junk, C.byref(sched.c_struct), 1, 0, flags,
                                                 junk, 1 << 40, None, None, C.byref(r), None, None if rs is None else C.byref(rs), None, None)
    sh8 = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
    sh8.n_q = 8
    wide = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
    wide.canvas = 1088
    ok = _hip.Revise(0.5)
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    codes = {name: int(value) for name, value in re.findall(r"\b(D3PM_E_[A-Z]+)\s*=\s*(-?\d+)", header)}
    E_ARG, E_SHAPE = codes["D3PM_E_ARG"], codes["D3PM_E_SHAPE"]
    # (n_q > 1 and a canvas > 1024 are shape refusals of d3pm_reveal itself: the same code as from its own entry)
    assert built_lib.d3pm_reveal_loop(C.byref(sh8), None, 1, junk, junk, None, junk, junk, junk, C.byref(sched.c_struct), 1, 0, 0, junk, 1 << 40, None,
                                      None, C.byref(rv), None) == E_SHAPE
    for fn in (step, loop):
        for args, kw, word, code in (((None,), {}, "null d3pm_revise", E_ARG), ((_hip.Revise(-0.5),), {}, "hold_bonus", E_ARG),
                                     ((_hip.Revise(float("nan")),), {}, "hold_bonus", E_ARG), ((_hip.Revise(float("inf")),), {}, "hold_bonus", E_ARG),
                                     ((ok, _hip.FLAG_SEED_IN_HBM), {}, "SEED_IN_HBM", E_ARG), ((ok, 0, sh8), {}, "n_q", E_SHAPE),
                                     ((ok, 0, wide), {}, "canvas", E_SHAPE), ((ok,), dict(ct=-1.0), "choice_temperature", E_ARG),
                                     ((ok,), dict(ct=float("nan")), "choice_temperature", E_ARG)):
            assert fn(*args, **kw) == code, (fn.__name__, args, kw, built_lib.d3pm_last_error())
            assert word in built_lib.d3pm_last_error().decode(), built_lib.d3pm_last_error()
    assert step(ok, t=40, t_next=60) == E_ARG and step(ok, t=100, t_next=0) == E_ARG
    assert loop(ok, n=0) == E_ARG and loop(ok, n=100) == E_ARG
    # a null grid inside a given d3pm_frame_scores
    fs = _hip.FrameScores(None, 16)
    assert built_lib.d3pm_reveal_step_revise(C.byref(sh), 1, junk, _hip.F16, junk, junk, junk, None, 60, 40, C.byref(sched.c_struct), 1, 0, 0, None, 0.0,
                                             junk, junk, C.byref(ok), C.byref(fs), None) == E_ARG
    assert "d3pm_frame_scores" in built_lib.d3pm_last_error().decode()


# ---- host validation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), -float("inf"), True, False, "1", 1e39, (1.0,)])
def test_revise_options_refuses(bad):
    from vall_e.vall_e import _hip
    with pytest.raises(ValueError):
        _hip.revise_options(bad)


def test_revise_options_values():
    from vall_e.vall_e import _hip
    assert _hip.revise_options(None) is None and _hip.revise_options() is None
    assert _hip.revise_options(0).hold_bonus == 0.0 and _hip.revise_options(0.0).hold_bonus == 0.0, "0 is ON: equal terms"
    assert _hip.revise_options(2).hold_bonus == 2.0 and _hip.revise_options(0.1).hold_bonus == np.float32(0.1)
    assert isinstance(_hip.revise_options(0), _hip.Revise)


@pytest.mark.parametrize("kw", [dict(revise=0.0), dict(revise=1.0), dict(revise=1.0, steps=10), dict(revise=-1.0, reveal_steps=4),
                                dict(revise=float("nan"), reveal_steps=4), dict(revise=True, reveal_steps=4), dict(revise="1", reveal_steps=4),
                                dict(revise=float("inf"), reveal_steps=4), dict(revise=1.0, reveal_steps=4, fp8=True),
                                dict(revise=1.0, reveal_steps=4, graph=True), dict(revise=1.0, reveal_steps=4, guidance=1.0),
                                dict(revise=1.0, reveal_steps=4, steps=10)])
def test_generate_audio_rejects_on_the_host(kw):
    """ValueError before anything touches the GPU: the model lives on the CPU here, and a valid call raises the RuntimeError of a
    missing HIP device instead."""
    with pytest.raises(ValueError):
        _native().generate_audio(_T, _P, **kw)


def test_valid_options_reach_the_device_check_and_the_keyword_is_keyword_only():
    import dataclasses
    from vall_e.vall_e import AR, _hip, synth
    for kw in (dict(revise=0.0, reveal_steps=4), dict(revise=0, reveal_steps=4), dict(revise=2.5, reveal_steps=16, choice_temperature=1.0, top_p=0.9),
               dict(revise=0.5, reveal_steps=4, mask_padding=True, return_logprobs=True, return_trace=True, greedy=True),
               dict(revise=None, reveal_steps=4), dict(revise=None)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            _native().generate_audio(_T, _P, **kw)
    m8 = AR.from_config(dataclasses.replace(synth.D3PMConfig.native(), n_q=2))
    with pytest.raises(ValueError, match="n_q"):
        m8.generate_audio(_T, _P, revise=1.0, reveal_steps=4)
    p = inspect.signature(AR.generate_audio).parameters
    assert p["revise"].default is None and p["revise"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (_hip.Sampler.reveal_step, _hip.Sampler.reveal_loop):
        assert inspect.signature(fn).parameters["revise"].default is None, fn.__qualname__
    assert "d3pm_revise" in AR.generate_audio.__doc__


def test_cli_and_dp_forward_the_option(monkeypatch, tmp_path):
    from vall_e import __main__ as cli
    from vall_e.vall_e import AR, dp
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
        cli.main(base + ["--reveal-steps", "8", "--revise", "1.5"])
    assert seen["revise"] == 1.5 and seen["reveal_steps"] == 8
    seen.clear()
    with pytest.raises(Stop):
        cli.main(base + ["--reveal-steps", "8", "--revise"])
    assert seen["revise"] == 0.0 and isinstance(seen["revise"], float), "the bare flag: a bonus of 0"
    seen.clear()
    with pytest.raises(Stop):
        cli.main(base + ["--reveal-steps", "8"])
    assert "revise" not in seen, "the keyword reaches generate_audio only when the flag is given"
    for bad in (["--revise"], ["--revise", "1"], ["--revise", "-1", "--reveal-steps", "4"], ["--revise", "nan", "--reveal-steps", "4"]):
        with pytest.raises(SystemExit):
            cli.main(base + bad)
    got = []

    class M:
        class cfg:
            canvas, n_q = 4, 1
        device = "cpu"

        def generate_audio(self, texts, proms, **kw):
            got.append(kw)
            return torch.zeros(len(texts), 4, dtype=torch.long)

    dp.generate_audio_dp(M(), _T, _P, seed=1, reveal_steps=4, revise=0.5)
    assert got[0]["revise"] == 0.5 and got[0]["reveal_steps"] == 4 and got[0]["global_batch"] == 2


# ---- compile time ------------------------------------------------------------------------------------------------------------------------
def _listing(src, flt):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), src, flt], capture_output=True, text=True, timeout=900).stdout
    return [ln for ln in out.splitlines() if "VGPR" in ln], out


def _arm(line):
    """((dtype, known, filter), revise) of a candidate-kernel line, whichever way the tool printed the name: demangled, mangled, or what
    c++filt makes of the bf16 / known instantiations.  revise is kRevise, the last template argument."""
    m = re.search(r"rows<float, (true|false), (\d), (true|false)>", line)
    if m:
        return ("f32", m.group(1) == "true", int(m.group(2))), m.group(3) == "true"
    m = re.search(r"rowsI(DF16_|DF16b)Lb([01])ELi(\d)ELb([01])E", line)
    if m:
        return (("f16" if m.group(1) == "DF16_" else "bf16"), m.group(2) == "1", int(m.group(3))), m.group(4) == "1"
    m = re.search(r"rows<bool _Accum, bool, E, (\d), (true|false)>", line)
    assert m, line
    return ("bf16", True, int(m.group(1))), m.group(2) == "true"


def test_revise_kernels_have_no_scratch_and_the_candidate_kernel_keeps_the_occupancy():
    """hipcc's resource remarks for every instantiation of d3pm_reveal.hip, split by kRevise: no scratch anywhere, and the revise form
    of the candidate kernel -- which carries the masked row's routine AND the held row's -- runs no fewer waves per SIMD than the
    reveal form of the same dtype and arms.  Cross-compiles, no GPU."""
    rows, out = _listing("d3pm_reveal.hip", "reveal")

    def revise(ln):      # kRevise, the last template argument, demangled or mangled
        m = re.search(r"(true|false)>|Lb([01])EEEv", ln)
        assert m, ln
        return m.group(1) == "true" or m.group(2) == "1"

    count = lambda name, rv: sum(name in ln and revise(ln) == rv for ln in rows)
    # 3 dtypes x {known, not} x {plain, filtered}; 2 dtypes x {known, not}; one commit kernel -- each as reveal and as revise
    for rv in (False, True):
        assert (count("reveal_candidate_rows", rv), count("reveal_commit_prep_rows", rv), count("reveal_commit_rows", rv)) == (12, 4, 1), out[-4000:]
    assert len(rows) == 34
    for ln in rows:
        assert re.search(r"scratch\s+0\b", ln), ln
    occ = lambda ln: int(re.search(r"occ (\d+)", ln).group(1))
    arms = {_arm(ln): occ(ln) for ln in rows if "reveal_candidate_rows" in ln}
    assert all(_arm(ln)[1] == revise(ln) for ln in rows if "reveal_candidate_rows" in ln)
    mine = {arm: o for (arm, rv), o in arms.items() if rv}
    theirs = {arm: o for (arm, rv), o in arms.items() if not rv}
    assert len(arms) == 24 and len(mine) == len(theirs) == 12 and set(mine) == set(theirs)
    for arm, o in theirs.items():
        assert mine[arm] >= o, (arm, mine[arm], o)

"""Per-frame log-probability of the revealed id: what can be checked without a GPU (python -m pytest tests/test_logprob_api.py -m "not gpu").
The entries are declared, bound and exported; the C entries refuse on the host before any pointer is read; every bad argument of
generate_audio is a ValueError before anything touches the GPU and a valid one reaches the device check; the CLI forwards the keyword
only when asked; the host reference of the GPU tests (tests/logprob_ref.py) holds the bound the header states; the new kernels compile
without scratch."""
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest
import torch

import logprob_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("d3pm_frame_scores_init", "d3pm_frame_scores_step", "d3pm_sample_loop_scored", "d3pm_reveal_loop_scored")

_T = [torch.tensor([5, 6, 7]), torch.tensor([8, 9])]
_P = [torch.zeros(4, 8, dtype=torch.long), torch.ones(6, 8, dtype=torch.long)]


def _native():
    from vall_e.vall_e import AR
    return AR.reference_native()


# ---- the entries -------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
    assert "#define D3PM_ABI_VERSION 6" in header and _hip.ABI_VERSION == 6 and built_lib.d3pm_abi_version() == 6
    m = re.search(r"typedef struct d3pm_frame_scores \{([^}]*)\} d3pm_frame_scores;", header, re.S)
    assert m and re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", m.group(1))).split() == "float *logprob; int32_t *step;".split()
    assert _hip.FrameScores._fields_ == [("logprob", C.c_void_p), ("step", C.c_void_p)] and C.sizeof(_hip.FrameScores) == 16
    version_comment = header.split("#define D3PM_ABI_VERSION")[0]
    for word in ("d3pm_frame_scores",) + NEW_ENTRIES:
        assert word in version_comment, word
    # the loop entries are the guided / keyed loops with the d3pm_frame_scores pointer in front of the stream
    fs = [C.POINTER(_hip.FrameScores), C.c_void_p]
    assert _hip.SIGNATURES["d3pm_sample_loop_scored"][1] == _hip.SIGNATURES["d3pm_sample_loop_guided"][1][:-1] + fs
    assert _hip.SIGNATURES["d3pm_reveal_loop_scored"][1] == _hip.SIGNATURES["d3pm_reveal_loop_keys"][1][:-1] + fs
    for text in ("logprob = z_j - m - logf(S)", "z_mask_id = -inf", "rn16(fmaf(w, float(c_k) - float(u_k), float(c_k)))", "1.0e-4",
                 "not necessarily to the id the loop returns"):
        assert text in header, text


def test_the_c_entries_refuse_on_the_host(built_lib):
    """Each check runs before any pointer is read or anything is launched, so it can be exercised with no device at all."""
    from vall_e.vall_e import _hip, synth
    E_ARG, E_SHAPE = -1, -4
    sh = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
    sh2 = _hip.make_shape(dataclasses.replace(synth.D3PMConfig.native(), n_q=2), torch.float16)
    sched = _hip.Schedule(100)
    junk = C.c_void_p(16)
    ok, no_lp, no_st = _hip.FrameScores(16, 16), _hip.FrameScores(None, 16), _hip.FrameScores(16, None)
    by = lambda v: None if v is None else C.byref(v)

    def init(fs, shape=sh, fm=junk, cv=None):
        return built_lib.d3pm_frame_scores_init(C.byref(shape), 1, junk, fm, by(cv), by(fs), None)

    def step(fs, shape=sh, dtype=_hip.F16, row_of=None, gd=None, t=5, ldl=1025):
        return built_lib.d3pm_frame_scores_step(C.byref(shape), 1, junk, dtype, ldl, row_of, by(gd), junk, t, by(fs), None)

    def loop(fs, shape=sh, flags=0, f8=None, keys=None, gd=None):
        return built_lib.d3pm_sample_loop_scored(C.byref(shape), None, f8, 1, junk, junk, None, 3, 0, junk, junk, junk, C.byref(sched.c_struct), 1, 0,
                                                 flags, junk, 1 << 40, None, None, by(keys), by(gd), by(fs), None)

    def reveal(fs, shape=sh, flags=0):
        rv = _hip.Reveal(4, 0.0)
        return built_lib.d3pm_reveal_loop_scored(C.byref(shape), None, 1, junk, junk, None, junk, junk, junk, C.byref(sched.c_struct), 1, 0, flags,
                                                 junk, 1 << 40, None, None, C.byref(rv), None, by(fs), None)
    cv = _hip.Canvas(16, None)
    for fn in (init, step, loop, reveal):
        for fs, word in ((None, "d3pm_frame_scores"), (no_lp, "d3pm_frame_scores"), (no_st, "d3pm_frame_scores")):
            assert fn(fs) == E_ARG and word in built_lib.d3pm_last_error().decode(), fn.__name__
        assert fn(ok, sh2) == E_SHAPE and "n_q" in built_lib.d3pm_last_error().decode(), fn.__name__
    assert init(ok, fm=junk, cv=cv) == E_ARG and init(ok, fm=None) == E_ARG, "exactly one of frame_mask and canvas"
    gd = _hip.Guidance(1.5)
    assert step(ok, row_of=junk, gd=gd) == E_ARG and "guidance" in built_lib.d3pm_last_error().decode()
    assert step(ok, row_of=junk, dtype=_hip.F32) == E_ARG and "16-bit" in built_lib.d3pm_last_error().decode()
    assert step(ok, gd=_hip.Guidance(float("nan"))) == E_ARG and step(ok, t=0) == E_ARG and step(ok, ldl=1024) == E_ARG and step(ok, dtype=7) == E_ARG
    for fn in (loop, reveal):
        assert fn(ok, flags=_hip.FLAG_SEED_IN_HBM) == E_ARG and "SEED_IN_HBM" in built_lib.d3pm_last_error().decode()
    assert loop(ok, f8=junk, keys=_hip.Keys(None, None, None)) == E_ARG and "fp8" in built_lib.d3pm_last_error().decode()
    assert loop(ok, f8=junk, gd=gd) == E_ARG and "fp8" in built_lib.d3pm_last_error().decode()
    assert loop(ok, gd=_hip.Guidance(-1.0)) == E_ARG and "finite" in built_lib.d3pm_last_error().decode()


# ---- host validation ---------------------------------------------------------------------------------------------------------------------
def test_keywords_and_defaults():
    from vall_e.vall_e import AR, _hip
    p = inspect.signature(AR.generate_audio).parameters
    assert p["return_logprobs"].default is False and p["return_logprobs"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (_hip.Sampler.sample_loop, _hip.Sampler.reveal_loop):
        assert inspect.signature(fn).parameters["scores"].default is None, fn.__qualname__
    assert hasattr(_hip.Sampler, "frame_scores_init") and hasattr(_hip.Sampler, "frame_scores_step")
    from vall_e.vall_e.ar_discrete import FrameScores
    assert FrameScores._fields == ("logprob", "step")
    from vall_e.vall_e import dp
    assert "return_logprobs" not in inspect.signature(dp.generate_audio_dp).parameters, "dp.py stays as it is"


@pytest.mark.parametrize("kw", [dict(return_logprobs=1), dict(return_logprobs="yes"), dict(return_logprobs=None), dict(return_logprobs=0),
                                dict(return_logprobs=True, graph=True)])
def test_generate_audio_rejects_on_the_host(kw):
    """ValueError before anything touches the GPU: the model lives on the CPU here, and a valid call raises the RuntimeError of a
    missing HIP device instead."""
    with pytest.raises(ValueError, match="return_logprobs"):
        _native().generate_audio(_T, _P, **kw)


def test_an_n_q_model_is_refused_and_valid_options_reach_the_device_check():
    from vall_e.vall_e import AR, synth
    m2 = AR.from_config(dataclasses.replace(synth.D3PMConfig.native(), n_q=2))
    with pytest.raises(ValueError, match="n_q"):
        m2.generate_audio(_T, _P, return_logprobs=True)
    for kw in (dict(), dict(return_trace=True), dict(n_frames=[30, 20], known=[torch.tensor([1, 2]), None], top_p=0.9, temperature=0.8, top_k=40),
               dict(greedy=True, steps=5, utt0=3, global_batch=8, streams=2), dict(guidance=1.5, mask_padding=True), dict(fp8=True),
               dict(reveal_steps=4, choice_temperature=1.0)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            _native().generate_audio(_T, _P, return_logprobs=True, **kw)


def test_cli_forwards_the_keyword_only_with_the_flag(monkeypatch, tmp_path):
    from vall_e import __main__ as cli
    from vall_e.vall_e import AR
    from vall_e.vall_e.ar_discrete import FrameScores
    seen = []

    def fake(self, **kw):
        seen.append(kw)
        ids = torch.arange(self.cfg.canvas)
        if kw.get("return_logprobs"):
            return ids, FrameScores(-torch.arange(self.cfg.canvas, dtype=torch.float32), torch.arange(self.cfg.canvas, dtype=torch.int32))
        return ids

    monkeypatch.setattr(AR, "generate_audio", fake)
    monkeypatch.setattr(AR, "to", lambda self, *a, **k: self)
    qnt = tmp_path / "p.qnt.pt"
    torch.save(torch.zeros(1, 8, 4, dtype=torch.long), qnt)
    base = [str(tmp_path / "o.qnt.pt"), "--phonemes", "1 2 3", "--prompt-qnt", str(qnt), "--native", "--device", "cpu"]
    cli.main(base)
    assert "return_logprobs" not in seen[0], "existing calls are keyword for keyword what they were"
    out = tmp_path / "lp.pt"
    cli.main(base + ["--logprobs", str(out), "--frames", "9"])
    assert seen[1]["return_logprobs"] is True and set(seen[1]) == set(seen[0]) | {"return_logprobs", "n_frames", "known"}
    scalars = lambda kw: {k: v for k, v in kw.items() if k not in ("return_logprobs", "n_frames", "known", "text_list", "proms_list")}
    assert scalars(seen[1]) == scalars(seen[0])
    saved = torch.load(out)
    assert set(saved) == {"logprob", "step"} and saved["logprob"].dtype == torch.float32 and saved["step"].dtype == torch.int32
    assert saved["step"].tolist() == list(range(9)) and saved["logprob"].tolist() == [-float(i) for i in range(9)], "the first n_frames frames"


# ---- the host reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1025, 257])
@pytest.mark.parametrize("scale", [0.8, 4.0, 12.0])
def test_the_definition_in_fp32_sits_inside_the_bound(K, scale):
    """The definition with serial fp32 summation against float64 on 400 rows per case: far inside the 1.0e-4 the header states."""
    g = np.random.default_rng(K + int(scale * 10))
    l = (g.standard_normal((400, K)) * scale).astype(np.float32)
    ids = R.other_ids(400, K, seed=K)
    ref = R.logprob64(l, K // 2, ids)
    assert np.isfinite(ref).all() and (ref < 0).all()
    err = np.abs(R.logprob32_serial(l, K // 2, ids).astype(np.float64) - ref).max()
    assert err < 0.25 * R.TOL, err
    # the mask class is outside the sum: raising its logit moves nothing
    l2 = l.copy()
    l2[:, K // 2] = 30.0
    assert np.array_equal(R.logprob64(l2, K // 2, ids), ref)


def test_reference_helpers():
    l, x, fm, known = R.cases(2, 37, 257, seed=1)
    free = R.free_masked(x, fm, known, 128)
    assert l.shape == (2, 37, 257) and free.sum() >= 20 and (fm[1, -5:] == 0).all() and fm[0].all() and known.sum() > 0
    assert (x[fm == 0] == 0).all() and (x[known != 0] != 128).all() and not free[known != 0].any() and not free[fm == 0].any()
    trace = np.array([[128, 128, 5, 9], [128, 7, 128, 9], [3, 7, 6, 9]])
    step = R.first_reveal(trace, [99, 98, 97], None, np.array([True, True, True, False]), 128)
    assert step.tolist() == [97, 98, 99, -1], "the FIRST entry that is not the mask, -1 off the free masked rows"
    assert R.first_reveal(trace[:1], [99], None, np.array([True, True, True, True]), 128).tolist() == [0, 0, 99, 99]


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_have_no_scratch():
    """hipcc's resource remarks for every instantiation of d3pm_logprob.hip: 3 dtypes x (plain, guided) x class count + 2 dtypes x
    indexed x class count + the init kernel; none of them spills."""
    import subprocess
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "d3pm_logprob.hip"], capture_output=True, text=True,
                         check=True, timeout=900).stdout
    rows = [ln for ln in out.splitlines() if "VGPR" in ln]
    assert len(rows) == 17, out
    for ln in rows:
        assert re.search(r"scratch\s+0\b", ln), ln
        assert int(re.search(r"VGPR\s+(\d+)", ln).group(1)) <= 64 and int(re.search(r"occ (\d+)", ln).group(1)) >= 8, ln

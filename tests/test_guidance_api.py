"""Classifier-free guidance: what can be checked without a GPU (python -m pytest tests/test_guidance_api.py -m "not gpu").
The host reference the GPU tests compare against (tests/guidance_ref.py) is exact on the tests' inputs; the crafted logits
separate the guided row from both of its sources; the entries are declared, bound and exported; every bad argument is a ValueError
before anything touches the GPU; the cond_drop decision is a function of (seed, utterance) mirrored from oracle/philox.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import guidance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("d3pm_posterior_sample_guided", "d3pm_sample_loop_guided")
WS = (0.5, 1.5, 2.0, 3.0)      # dyadic weights only: w * d is then a short product and the reference is exact


def _native():
    from vall_e.vall_e import AR
    return AR.reference_native()


_T = [torch.tensor([5, 6, 7]), torch.tensor([8, 9])]
_P = [torch.zeros(4, 8, dtype=torch.long), torch.ones(6, 8, dtype=torch.long)]


# ---- the host reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [np.float16, "bfloat16"])
@pytest.mark.parametrize("K", [1025, 257])
def test_reference_is_exact_on_the_tests_inputs(grid, K):
    c, u = R.crafted(74, K, seed=K + 3, dtype=grid)
    assert np.array_equal(R.on_grid(c, grid), c) and np.array_equal(R.on_grid(u, grid), u)
    for w in WS:
        assert R.exact(c, u, w).all(), "w * float32(c - u) + c is exact in fp64: one rounding to fp32, as the fma"
        assert R.exact_rational(c, u, w, n=1500, seed=int(w * 4))
        z = R.combine(c, u, w)
        assert z.dtype == np.float16 and np.isfinite(z.astype(np.float32)).all()
        assert np.array_equal(R.combine(c, c, w), R.rn16(c)), "c == u: z = rn16(c) exactly"
        assert np.array_equal(R.combine(c, u, 0.0), R.rn16(c))


def test_reference_against_rational_arithmetic_with_one_rounding():
    """combine == rn16(round_to_fp32(w (c - u)_fp32 + c)) computed with Fractions, element by element, on a small block."""
    from fractions import Fraction
    c, u = R.crafted(8, 257, seed=1)
    for w in (0.5, 3.0):
        z = R.combine(c, u, w)
        for i, j in [(i, j) for i in range(8) for j in range(0, 257, 9)]:
            d = np.float32(np.float64(c[i, j]) - np.float64(u[i, j]))
            exact = Fraction(w) * Fraction(float(d)) + Fraction(float(c[i, j]))
            f32 = np.float32(float(exact))      # float(Fraction) rounds once to fp64; exact here (asserted above), then once to fp32
            assert Fraction(float(np.float64(float(exact)))) == exact
            assert z[i, j] == np.float16(f32)


@pytest.mark.parametrize("K", [1025, 257])
def test_crafted_rows_separate_the_guided_id_from_both_sources(K):
    c, u = R.crafted(74, K, seed=K + 3)
    assert not np.array_equal(c[:37], c[37:]) and not np.array_equal(u[:37], u[37:]), "the two utterances have distinct twins"
    for w in (0.5, 1.5, 3.0):
        z = R.combine(c, u, w).astype(np.float32).argmax(-1)
        assert (z != c.argmax(-1)).mean() >= 0.5 and (z != u.argmax(-1)).mean() >= 0.5
        swapped = R.combine(u, c, w).astype(np.float32).argmax(-1)
        neighbour = R.combine(c, np.roll(u, 1, axis=0), w).astype(np.float32).argmax(-1)
        assert (swapped != z).mean() >= 0.5 and (neighbour != z).mean() >= 0.5


# ---- the entries -------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
    assert "#define D3PM_ABI_VERSION 6" in header and _hip.ABI_VERSION == 6 and built_lib.d3pm_abi_version() == 6
    m = re.search(r"typedef struct d3pm_guidance \{([^}]*)\} d3pm_guidance;", header, re.S)
    assert m and re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", m.group(1))).split() == "float weight;".split()
    assert _hip.Guidance._fields_ == [("weight", C.c_float)] and C.sizeof(_hip.Guidance) == 4
    version_comment = header.split("#define D3PM_ABI_VERSION")[0]
    for word in ("d3pm_guidance",) + NEW_ENTRIES:
        assert word in version_comment, word
    # the loop entry is d3pm_sample_loop_keys with the d3pm_guidance pointer in front of the stream
    a, b = _hip.SIGNATURES["d3pm_sample_loop_guided"][1], _hip.SIGNATURES["d3pm_sample_loop_keys"][1]
    assert a == b[:-1] + [C.POINTER(_hip.Guidance), C.c_void_p]
    assert "fmaf(w, float(c_j) - float(u_j), float(c_j))" in header and "2 * max(regime_batch, batch)" in header


def test_the_c_entries_refuse_on_the_host(built_lib):
    """D3PM_E_ARG with a message for a null d3pm_guidance, a bad weight, n_q > 1, fp8 weights and the seed-in-HBM flag: each check
    runs before any pointer is read or anything is launched, so it can be exercised with no device at all."""
    from vall_e.vall_e import _hip, synth
    sh = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
    sched = _hip.Schedule(100)
    junk = C.c_void_p(16)

    def step(gd, flags=0, shape=sh):
        return built_lib.d3pm_posterior_sample_guided(C.byref(shape), 1, junk, _hip.F16, junk, junk, None, 5, C.byref(sched.c_struct), 1, 0, flags,
                                                      None, None if gd is None else C.byref(gd), None)

    def loop(gd, flags=0, f8=None, shape=sh):
        return built_lib.d3pm_sample_loop_guided(C.byref(shape), None, f8, 1, junk, junk, None, 3, 0, junk, junk, junk, C.byref(sched.c_struct), 1,
                                                 0, flags, junk, 1 << 40, None, None, None, None if gd is None else C.byref(gd), None)
    sh8 = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
    sh8.n_q = 8
    ok = _hip.Guidance(1.5)
    for fn in (step, loop):
        for args, word in (((None,), "null d3pm_guidance"), ((_hip.Guidance(-0.5),), "finite"), ((_hip.Guidance(float("nan")),), "finite"),
                           ((_hip.Guidance(float("inf")),), "finite"), ((ok, _hip.FLAG_SEED_IN_HBM), "SEED_IN_HBM"), ((ok, 0) + ((None,) if fn is loop else ()) + (sh8,), "n_q")):
            assert fn(*args) == -1, (fn.__name__, args)
            assert word in built_lib.d3pm_last_error().decode(), built_lib.d3pm_last_error()
    assert loop(ok, 0, junk) == -1 and "fp8" in built_lib.d3pm_last_error().decode()


# ---- host validation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), -float("inf"), True, False, "1", None, 1e39])
def test_guidance_options_refuses(bad):
    from vall_e.vall_e import _hip
    with pytest.raises(ValueError):
        _hip.guidance_options(bad)


def test_guidance_options_values():
    from vall_e.vall_e import _hip
    assert _hip.guidance_options(0) is None and _hip.guidance_options(0.0) is None and _hip.guidance_options() is None
    assert _hip.guidance_options(2).weight == 2.0 and _hip.guidance_options(0.1).weight == np.float32(0.1)


@pytest.mark.parametrize("kw", [dict(guidance=-1.0), dict(guidance=float("nan")), dict(guidance=True), dict(guidance="2"),
                                dict(null_text_list=_T), dict(null_proms_list=_P), dict(guidance=0.0, null_text_list=_T),
                                dict(guidance=1.0, null_text_list=_T[:1]), dict(guidance=1.0, null_proms_list=_P + _P),
                                dict(guidance=1.0, graph=True), dict(guidance=1.0, fp8=True), dict(guidance=1.0, reveal_steps=4)])
def test_generate_audio_rejects_on_the_host(kw):
    """ValueError before anything touches the GPU: the model lives on the CPU here, and a valid call raises the RuntimeError of a
    missing HIP device instead."""
    with pytest.raises(ValueError):
        _native().generate_audio(_T, _P, **kw)


def test_an_n_q_model_is_refused_and_valid_options_reach_the_device_check():
    import dataclasses
    from vall_e.vall_e import AR, synth
    m8 = AR.from_config(dataclasses.replace(synth.D3PMConfig.native(), n_q=2))
    with pytest.raises(ValueError, match="n_q"):
        m8.generate_audio(_T, _P, guidance=1.0)
    for kw in (dict(guidance=1.5), dict(guidance=2, null_text_list=_T, null_proms_list=[None, _P[0]]), dict(guidance=0.5, mask_padding=True, top_p=0.9)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            _native().generate_audio(_T, _P, **kw)


def test_null_twins_and_their_key_counts():
    m = _native()
    cfg = m.cfg
    nt, npm = m._null_conditions(_T, None, 1), m._null_conditions(_P, [None, _P[0]], 2)
    assert [tuple(t.shape) for t in nt] == [(0,), (0,)] and nt[0].dtype == _T[0].dtype
    assert tuple(npm[0].shape) == (0, 8) and npm[1] is _P[0]
    f, t, p = m._twin_key_lengths(([37, 300], [3, 2], [4, 6]), [None, torch.tensor([1, 2, 3, 4])], None)
    assert f == [37, 300, 37, 300], "a twin has its partner's frames"
    assert t == [3, 2, cfg.s_text, 4], "the empty null keeps all of its padding as keys, a caller-given one its own length"
    assert p == [4, 6, cfg.s_prompt, cfg.s_prompt]


def test_p_sample_and_sampler_arguments():
    from vall_e.vall_e import AR, _hip
    for fn, names in ((AR.generate_audio, ("guidance", "null_text_list", "null_proms_list")), (AR.p_sample, ("guidance", "null_logits")),
                      (_hip.Sampler.sample_loop, ("guidance",)), (_hip.Sampler.posterior_sample, ("guidance", "null_logits")),
                      (AR.forward_backward, ("cond_drop",))):
        p = inspect.signature(fn).parameters
        for n in names:
            assert n in p, (fn.__qualname__, n)
    p = inspect.signature(AR.generate_audio).parameters
    assert p["guidance"].default == 0.0 and p["null_text_list"].default is None and p["guidance"].kind is inspect.Parameter.KEYWORD_ONLY
    m = _native()
    lg = torch.zeros(1, m.cfg.canvas, 1025)
    x = torch.zeros(1, m.cfg.canvas, dtype=torch.long)
    for kw in (dict(guidance=1.0), dict(null_logits=lg), dict(guidance=-1.0, null_logits=lg)):
        with pytest.raises(ValueError):
            m.p_sample(lg, torch.tensor([5]), x, **kw)


def test_cli_and_dp_forward_the_weight(monkeypatch, tmp_path):
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
        cli.main(base + ["--guidance", "1.5"])
    assert seen["guidance"] == 1.5
    seen.clear()
    with pytest.raises(Stop):
        cli.main(base)
    assert seen["guidance"] == 0.0
    for bad in (["--guidance", "-1"], ["--guidance", "nan"], ["--guidance", "2", "--reveal-steps", "4"]):
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

    dp.generate_audio_dp(M(), _T, _P, seed=1, guidance=2.0, null_text_list=_T)
    assert got[0]["guidance"] == 2.0 and got[0]["global_batch"] == 2 and len(got[0]["null_text_list"]) == 2


# ---- the training hook -------------------------------------------------------------------------------------------------------------------
def test_cond_drop_probabilities_and_the_mirrored_decision():
    from oracle import philox
    from vall_e.vall_e import train
    assert train.COND_DROP_STREAM == R.COND_DROP_STREAM == 5, "streams 0..4 and 16..23 are taken"
    assert train.cond_drop_probs(0) == train.cond_drop_probs(False) == train.cond_drop_probs(None) == train.cond_drop_probs(0.0) == (0.0, 0.0)
    assert train.cond_drop_probs(0.25) == (0.25, 0.25) and train.cond_drop_probs((0.1, 1.0)) == (0.1, 1.0) and train.cond_drop_probs(1) == (1.0, 1.0)
    for bad in (True, -0.1, 1.5, (0.1,), (0.1, 0.2, 0.3), (0.1, True), "0.1", float("nan"), (0.5, float("inf"))):
        with pytest.raises(ValueError):
            train.cond_drop_probs(bad)
    assert train.cond_drop_decision(3, 7, 0.0, 0.0, "cpu") == (False, False), "p = 0 draws nothing: no device needed"
    # the mirror: words 0 and 1 of (group 0, row utt, t 0, stream 5); a function of (seed, utt); p = 1 always, p = 0 never
    u = philox.uniform_rows(11, 0, 40, 3, 4, stream=5)
    for i in range(3):
        assert R.cond_drop_mirror(11, 40 + i, 0.5, 0.5) == (bool(u[i, 0] < 0.5), bool(u[i, 1] < 0.5))
        assert R.cond_drop_mirror(11, 40 + i, 1.0, 0.0) == (True, False) and R.cond_drop_mirror(11, 40 + i, 0.0, 1.0) == (False, True)
    d = np.array([R.cond_drop_mirror(5, utt, 0.3, 0.7) for utt in range(2000)])
    assert abs(d[:, 0].mean() - 0.3) < 0.04 and abs(d[:, 1].mean() - 0.7) < 0.04, d.mean(0)
    both = (d[:, 0] & d[:, 1]).mean()
    assert abs(both - 0.21) < 0.04, "the two decisions come from different words"
    assert not np.array_equal(d, np.array([R.cond_drop_mirror(6, utt, 0.3, 0.7) for utt in range(2000)]))
    assert not np.array_equal(philox.uniform_rows(11, 0, 40, 3, 4, stream=5), philox.uniform_rows(11, 0, 40, 3, 4, stream=3))


def test_guided_kernels_have_no_scratch():
    """hipcc's resource remarks for every guided instantiation: no scratch, and the reference-class-count kernels keep at least the
    four waves per SIMD of the unguided sampler."""
    import subprocess
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "d3pm_sample.hip", "guided_sample"], capture_output=True,
                         text=True, check=True).stdout
    rows = [ln for ln in out.splitlines() if "VGPR" in ln]
    assert len(rows) == 20, out      # 3 dtypes x known x class count, and 2 dtypes x known x class count with the preparation
    for ln in rows:
        assert re.search(r"scratch\s+0\b", ln), ln
        assert int(re.search(r"occ (\d+)", ln).group(1)) >= 4, ln

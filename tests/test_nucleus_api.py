"""The nucleus (top-p) cut on the x0-logits of the D3PM sampler, host side: the C-ABI additions (d3pm_nucleus and the two *_nucleus
entries), their refusal of bad values before anything else is touched, the keywords of AR.generate_audio / AR.p_sample, the CLI
flag, the forwarding by the data-parallel layer, the definition itself on rows whose answer is known without trusting an exp, and the
compile-time claims (no scratch anywhere, the kernels without a filter at the register counts they had).  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import nucleus_ref as R

NEW_ENTRIES = ("d3pm_posterior_sample_nucleus", "d3pm_sample_loop_nucleus")
NAN, INF = float("nan"), float("inf")
BAD_P = [0.0, -0.5, -0.0, 1.0000001, 1.5, NAN, INF, -INF]


def test_nucleus_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
    m = re.search(r"typedef struct d3pm_nucleus \{([^}]*)\} d3pm_nucleus;", header, re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "float temperature; int32_t top_k; float top_p;"
    assert [(n, t) for n, t in _hip.Nucleus._fields_] == [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float)]
    assert C.sizeof(_hip.Nucleus) == 12 and _hip.Nucleus.top_k.offset == 4 and _hip.Nucleus.top_p.offset == 8
    # additions only: the version stays, d3pm_sampling keeps its two fields, and the additions are listed in the version comment
    assert built_lib.d3pm_abi_version() == 6
    m = re.search(r"typedef struct d3pm_sampling \{([^}]*)\} d3pm_sampling;", header, re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "float temperature; int32_t top_k;"
    assert C.sizeof(_hip.Sampling) == 8 and len(_hip.Sampling._fields_) == 2
    version_comment = header.split("#define D3PM_ABI_VERSION")[0]
    for word in ("d3pm_nucleus",) + NEW_ENTRIES:
        assert word in version_comment, word
    # the step entry: the _sampling one with the triple and a theta output in front of the stream; the loop entry: the triple
    step = _hip.SIGNATURES["d3pm_posterior_sample_sampling"][1]
    assert _hip.SIGNATURES["d3pm_posterior_sample_nucleus"][1] == step[:-2] + [C.POINTER(_hip.Nucleus), C.c_void_p] + step[-1:]
    loop = _hip.SIGNATURES["d3pm_sample_loop_sampling"][1]
    assert _hip.SIGNATURES["d3pm_sample_loop_nucleus"][1] == loop[:-2] + [C.POINTER(_hip.Nucleus)] + loop[-1:]


def _shape(n_q=1):
    from vall_e.vall_e import _hip, synth
    sh = _hip.make_shape(synth.D3PMConfig.native(), torch.float16)
    sh.n_q = n_q
    return sh


def _step(lib, sh, nu, theta=None):
    return lib.d3pm_posterior_sample_nucleus(C.byref(sh), 1, None, 1, None, None, None, 40, None, 0, 0, 0, None,
                                             None if nu is None else C.byref(nu), theta, None)


def _loop(lib, sh, nu, frame_mask, canvas=None):
    return lib.d3pm_sample_loop_nucleus(C.byref(sh), None, None, 1, None, frame_mask, canvas, 9, 0, None, None, None, None, 0, 0, 0,
                                        None, 0, None, None if nu is None else C.byref(nu), None)


@pytest.mark.parametrize("p", BAD_P)
def test_c_entries_refuse_a_bad_top_p_before_anything_else(built_lib, p):
    """D3PM_E_ARG with a message that names top_p, from both entries, with every pointer still NULL: values are checked before
    pointers, and long before a launch (there is no GPU here)."""
    from vall_e.vall_e import _hip
    sh = _shape()
    dummy = C.c_uint8(1)
    for tau, k in ((1.0, 0), (0.7, 50)):
        nu = _hip.Nucleus(tau, k, p)
        assert _step(built_lib, sh, nu) == -1
        assert b"top_p" in built_lib.d3pm_last_error() and b"d3pm_posterior_sample_nucleus" in built_lib.d3pm_last_error()
        assert _loop(built_lib, sh, nu, C.addressof(dummy)) == -1
        assert b"top_p" in built_lib.d3pm_last_error() and b"d3pm_sample_loop_nucleus" in built_lib.d3pm_last_error()
    # the two older numbers are still checked by the new entries
    assert _step(built_lib, sh, _hip.Nucleus(0.0, 0, 0.9)) == -1 and b"temperature" in built_lib.d3pm_last_error()
    assert _loop(built_lib, sh, _hip.Nucleus(1.0, 1026, 0.9), C.addressof(dummy)) == -1 and b"top_k" in built_lib.d3pm_last_error()


def test_c_entries_accept_good_values_up_to_the_pointer_checks(built_lib):
    from vall_e.vall_e import _hip
    sh = _shape()
    dummy = C.c_uint8(1)
    cv = _hip.Canvas(C.addressof(dummy), None)
    for nu in (None, _hip.Nucleus(1.0, 0, 1.0), _hip.Nucleus(1.0, 0, 0.9), _hip.Nucleus(0.7, 50, 0.5), _hip.Nucleus(1.3, 1025, 2.0 ** -11),
               _hip.Nucleus(1.0, 0, 1e-30)):
        assert _step(built_lib, sh, nu) == -1 and b"null pointer" in built_lib.d3pm_last_error()
        assert _loop(built_lib, sh, nu, None) == -1 and b"exactly one of" in built_lib.d3pm_last_error()
        assert _loop(built_lib, sh, nu, C.addressof(dummy), C.byref(cv)) == -1 and b"exactly one of" in built_lib.d3pm_last_error()
        assert _loop(built_lib, sh, nu, C.addressof(dummy)) == -1 and b"null pointer" in built_lib.d3pm_last_error()
        assert _loop(built_lib, sh, nu, None, C.byref(cv)) == -1 and b"null pointer" in built_lib.d3pm_last_error()


def test_nucleus_options_helper():
    from vall_e.vall_e import _hip
    assert _hip.nucleus_options() is None and _hip.nucleus_options(1.0, 0, 1.0, 1025) is None and _hip.nucleus_options(1, 0, 1) is None
    s = _hip.nucleus_options(0.7, 50, 1.0, 1025)          # top_p == 1: what sampling_options returns
    assert type(s) is _hip.Sampling and s.top_k == 50 and s.temperature == C.c_float(0.7).value
    n = _hip.nucleus_options(0.7, 50, 0.9, 1025)
    assert type(n) is _hip.Nucleus and (n.temperature, n.top_k, n.top_p) == (C.c_float(0.7).value, 50, C.c_float(0.9).value)
    n = _hip.nucleus_options(top_p=0.5)
    assert type(n) is _hip.Nucleus and (n.temperature, n.top_k, n.top_p) == (1.0, 0, 0.5)
    # (1e-60 is 0 as a float; 1 + 1e-12 is > 1 as given, though 1 as a float)
    for p in BAD_P + [True, False, "0.9", None, [0.9], 1e-60, 1.0 + 1e-12]:
        with pytest.raises(ValueError, match="top_p"):
            _hip.nucleus_options(1.0, 0, p, 1025)
    with pytest.raises(ValueError, match="temperature"):
        _hip.nucleus_options(0.0, 0, 0.9, 1025)
    with pytest.raises(ValueError, match="top_k"):
        _hip.nucleus_options(1.0, 1026, 0.9, 1025)
    # sampling_options keeps its signature and behaviour
    assert list(inspect.signature(_hip.sampling_options).parameters) == ["temperature", "top_k", "n_classes"]
    assert _hip.sampling_options(1.0, 0, 1025) is None and type(_hip.sampling_options(0.7, 0, 1025)) is _hip.Sampling


_T = [torch.tensor([1, 2, 3])] * 2
_P = [torch.zeros(4, 8, dtype=torch.long)] * 2


def _native():
    from vall_e.vall_e import AR
    return AR.reference_native()          # parameters on the CPU


@pytest.mark.parametrize("kw", [dict(top_p=p) for p in BAD_P] + [
    dict(top_p=True), dict(top_p="0.9"), dict(top_p=None), dict(top_p=0.9, temperature=0.0), dict(top_p=0.9, top_k=-1),
    dict(top_p=0.9, graph=True), dict(top_p=0.5, top_k=50, graph=True),          # the graph path never ignores the option
], ids=repr)
def test_generate_audio_and_p_sample_reject_bad_options_on_the_host(kw):
    """ValueError before anything touches the GPU: the model lives on the CPU here, and a valid call would raise the RuntimeError of
    a missing HIP device instead."""
    m = _native()
    with pytest.raises(ValueError):
        m.generate_audio(_T, _P, **kw)
    if "graph" not in kw:
        with pytest.raises(ValueError):
            m.p_sample(torch.zeros(1, 448, 1025), torch.tensor([40]), torch.zeros(1, 448, dtype=torch.int64), **kw)


def test_valid_options_reach_the_device_check():
    m = _native()
    for kw in (dict(top_p=0.9), dict(top_p=1.0, graph=True), dict(top_p=0.5, temperature=0.7, top_k=50), dict(top_p=2.0 ** -11),
               dict(top_p=0.99, n_frames=[10, 448], known=[torch.tensor([1, 512]), None])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.generate_audio(_T, _P, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.p_sample(torch.zeros(1, 448, 1025), torch.tensor([40]), torch.zeros(1, 448, dtype=torch.int64), top_p=0.9)


def test_signatures_take_top_p():
    from vall_e.vall_e import AR, _hip
    for fn in (AR.generate_audio, AR.p_sample):
        p = inspect.signature(fn).parameters
        assert p["top_p"].default == 1.0 and p["top_p"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(_hip.Sampler.posterior_sample).parameters
    assert p["top_p"].default == 1.0 and p["want_theta"].default is False
    assert inspect.signature(_hip.Sampler.sample_loop).parameters["top_p"].default == 1.0


def test_cli_parses_the_flag(monkeypatch, tmp_path):
    """--top-p reaches AR.generate_audio; a bad value is an argparse error (exit status 2) before a model is built."""
    import vall_e.__main__ as cli
    from vall_e import formats
    from vall_e.vall_e import AR
    seen = {}

    class Fake:
        class cfg:
            n_frames = 6
        phone_symmap = {}

        def to(self, *_):
            return self

        def generate_audio(self, **kw):
            seen.update(kw)
            return torch.arange(448)

    monkeypatch.setattr(AR, "reference_native", classmethod(lambda cls: seen.update(built=True) or Fake()))
    monkeypatch.setattr(formats, "load_quants", lambda p: torch.zeros(5, 8, dtype=torch.long))
    monkeypatch.setattr(formats, "save_quants", lambda resps, path: seen.update(saved=tuple(resps.shape)))
    base = ["--native", "--phonemes", "1 2 3", "--prompt-qnt", "p.qnt.pt", str(tmp_path / "o.qnt.pt")]
    cli.main(base + ["--top-p", "0.9"])
    assert seen["top_p"] == 0.9 and seen["temperature"] == 1.0 and seen["top_k"] == 0 and seen["saved"] == (6, 1)
    seen.clear()
    cli.main(base)
    assert seen["top_p"] == 1.0
    seen.clear()
    cli.main(base + ["--top-p", "0.5", "--top-k", "3", "--temperature", "0.7", "--frames", "4"])
    assert (seen["top_p"], seen["top_k"], seen["temperature"], seen["n_frames"]) == (0.5, 3, 0.7, [4])
    for bad in (["--top-p", "0"], ["--top-p", "-0.1"], ["--top-p", "1.01"], ["--top-p", "nan"], ["--top-p", "inf"], ["--top-p", "x"]):
        seen.clear()
        with pytest.raises(SystemExit) as e:
            cli.main(base + bad)
        assert e.value.code == 2 and not seen, bad


def test_dp_forwards_top_p():
    from vall_e.vall_e import dp

    class Model:
        class cfg:
            canvas, n_frames = 16, 12
        device = torch.device("cpu")

    log = []

    def gen(texts, proms, *, seed, utt0, top_p, temperature=1.0, top_k=0, n_frames=None):
        log.append((utt0, top_p, top_k))
        return torch.zeros(len(texts), 16, dtype=torch.long)

    texts = [torch.tensor([i]) for i in range(3)]
    dp.generate_audio_dp(Model(), texts, texts, seed=3, generate_fn=gen, top_p=0.9, top_k=7)
    assert log == [(0, 0.9, 7)]


# ---- the definition --------------------------------------------------------------------------------------------------------------
def _exp_variants():
    """np.exp and the same nudged by a few float32 ulps either way: what holds for all of them does not hang on exp's last bit
    (the maximum's exp(0) stays exactly 1, as it does for every exp)."""
    def nudged(n):
        def f(x):
            e = np.exp(x).astype(np.float32)
            for _ in range(abs(n)):
                e = np.where(x == 0, e, np.nextafter(e, np.float32(np.inf if n > 0 else 0.0))).astype(np.float32)
            return e
        return f
    return [np.exp, nudged(3), nudged(-3)]


def test_definition_ties_at_the_maximum():
    """top_p <= 1/1280: Q <= K 2^20, so the target is at most 2^20 = q of ONE maximal class: exactly the classes tied at the maximum
    are kept -- the ids top_k = 1 gives."""
    g = np.random.default_rng(0)
    for K in (1025, 777, 1280):
        l = (g.standard_normal((48, K)) * 3).astype(np.float16).astype(np.float32)
        l[0] = 1.5                                 # all tied
        l[1, 10:20] = 12.5                         # ten tied at the top
        l[2, ::2] = 0.0; l[2, 1::2] = -0.0; l[2, 7] = -3.0      # signed zeros at the top
        l[3, 5:] = R.NEG_INF
        for p in (2.0 ** -11, 1.0 / 1280, 1e-30):
            for exp in _exp_variants():
                got = R.host_nucleus(l, 1.0, 0, p, exp)
                assert np.array_equal(got, R.host_filter(l, 1.0, 1)), (K, p)
        assert np.isfinite(R.host_nucleus(l, 1.0, 0, 2.0 ** -11)[1]).sum() == 10
        assert np.isfinite(R.host_nucleus(l, 1.0, 0, 2.0 ** -11)[2]).sum() == K - 1


@pytest.mark.parametrize("K", [1025, 777, 64])
def test_definition_two_level_rows(K):
    cases = R.two_level_cases(K)
    assert len(cases) >= 4
    for row, top_p, kept, theta in cases:
        for exp in _exp_variants():
            th = R.nucleus_theta(row[None], top_p, exp)[0]
            assert th == theta, (K, top_p, th, theta)
            got = np.flatnonzero(np.isfinite(R.cut_at(row[None], [th])[0]))
            assert np.array_equal(got, kept)
        # the composition rule: the nucleus acts on z'', here after a top-k that keeps the same classes
        z2 = R.host_filter(row[None], 1.0, len(kept))
        assert np.array_equal(R.host_nucleus(row[None], 1.0, len(kept), top_p), R.cut_at(z2, R.nucleus_theta(z2, top_p)))


def test_definition_signed_zeros_and_the_slack():
    K = 1025
    # zeros as the LOWER level: 4 classes at 2.0, 300 at +0, 300 at -0, the rest -inf.  w = trunc(exp(-2) 2^20) ~ 141 909, so
    # Q ~ 4.19 M + 2 x 42.57 M = 89.3 M.  top_p = 0.5: the target 44.7 M is reached by the keys >= key(+0) (46.8 M), so theta = +0
    # -- and the cut, on VALUES, keeps the -0 classes as well.  The margins are millions of units: no exp's last bit matters.
    row = np.full(K, R.NEG_INF, dtype=np.float32)
    row[:4] = 2.0; row[4:304] = 0.0; row[304:604] = -0.0
    for exp in _exp_variants():
        th = R.nucleus_theta(row[None], 0.5, exp)[0]
        assert th == 0.0 and not np.signbit(th), "theta is +0: its key is the largest one that reaches the target"
        assert np.isfinite(R.cut_at(row[None], [th])[0]).sum() == 604, "-0 >= +0 on values: both zeros stand"
        th = R.nucleus_theta(row[None], 0.95, exp)[0]          # needs the -0 classes' mass as well
        assert th == 0.0 and np.signbit(th)
        assert np.isfinite(R.cut_at(row[None], [th])[0]).sum() == 604
        th = R.nucleus_theta(row[None], 0.04, exp)[0]          # 4 2^20 / Q ~ 0.047: the upper level alone
        assert th == 2.0 and np.isfinite(R.cut_at(row[None], [th])[0]).sum() == 4
    # the slack of the contract, on random rows: |sum_S q / Q - sum_S softmax| <= K / 2^20 + 2^-20 for the kept set, so the kept
    # mass is >= top_p - eps and the mass strictly above theta is < top_p + eps; theta is one of the row's values
    g = np.random.default_rng(1)
    l = (g.standard_normal((256, K)) * 3).astype(np.float16).astype(np.float32)
    l[::4] *= 4.0
    eps = K / 2.0 ** 20 + 2.0 ** -20
    assert eps <= 1.0e-3
    for tau, k, p in ((1.0, 0, 0.9), (0.7, 50, 0.5), (1.3, 0, 0.99)):
        z2 = R.host_filter(l, tau, k)
        th = R.nucleus_theta(z2, p)
        assert (z2 == th[:, None]).any(-1).all()
        sm = torch.softmax(torch.from_numpy(z2).double(), -1).numpy()
        ge = np.where(z2 >= th[:, None], sm, 0).sum(-1)
        gt = np.where(z2 > th[:, None], sm, 0).sum(-1)
        assert (ge >= p - eps).all() and (gt < p + eps).all(), (tau, k, p, ge.min(), gt.max())


# ---- compile time ----------------------------------------------------------------------------------------------------------------
def test_sampler_kernels_have_no_scratch_and_the_unfiltered_ones_keep_their_registers():
    """Every sampler kernel of d3pm_sample.hip, in all three arms, compiles without scratch; the kernels without a filter report the
    register counts they had (97 VGPRs stand-alone, 94 with the next iteration's preparation); the nucleus arm exists as kernels of
    its own, next to the unchanged *_filtered ones.  Cross-compiles, no GPU."""
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "d3pm_sample.hip", "sample"],
                         capture_output=True, text=True, timeout=900).stdout
    rows = [l for l in out.splitlines() if "posterior_sample" in l or "nucleus_sample" in l]
    res = {}
    for l in rows:
        m = re.search(r"VGPR\s+(\d+).*scratch\s+(\d+)", l)
        assert m and int(m.group(2)) == 0, f"a sampler kernel with scratch: {l}"
        assert int(m.group(1)) <= 128, f"a sampler kernel below four waves per SIMD: {l}"
        kind = ("nucleus" if "nucleus_sample" in l else "filtered" if "_filtered" in l else "plain") + ("_prep" if "prep_rows" in l else "")
        res.setdefault(kind, []).append(int(m.group(1)))
    # 3 dtypes x {known, not} stand-alone, 2 dtypes x {known, not} with the preparation
    assert {k: len(v) for k, v in res.items()} == dict(plain=6, filtered=6, nucleus=6, plain_prep=4, filtered_prep=4, nucleus_prep=4), out[-4000:]
    assert set(res["plain"]) == {97} and set(res["plain_prep"]) == {94}, res
    assert set(res["filtered"]) == {96} and set(res["filtered_prep"]) == {95}, "the top-k-only kernels are the ones they were"

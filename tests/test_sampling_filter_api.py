"""Temperature and top-k on the x0-logits of the D3PM sampler, host side: the C-ABI additions (d3pm_sampling and the two
*_sampling entries), their refusal of bad values before anything else is touched, the keywords of AR.generate_audio / AR.p_sample,
the CLI flags, the forwarding by the data-parallel layer, and the compile-time claims (no scratch, the kernels without the filter arm
still there under their names).  No GPU."""
import ctypes as C
import datetime
import os
import re
import socket
import subprocess

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

NEW_ENTRIES = ("d3pm_posterior_sample_sampling", "d3pm_sample_loop_sampling")


def test_sampling_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
    # the struct: float temperature, then int32 top_k, nothing else -- in the header and in ctypes
    m = re.search(r"typedef struct d3pm_sampling \{([^}]*)\} d3pm_sampling;", header, re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "float temperature; int32_t top_k;"
    assert [(n, t) for n, t in _hip.Sampling._fields_] == [("temperature", C.c_float), ("top_k", C.c_int32)]
    assert C.sizeof(_hip.Sampling) == 8 and _hip.Sampling.temperature.offset == 0 and _hip.Sampling.top_k.offset == 4
    # additions only: the version and the pinned struct of the canvas entries stay
    assert built_lib.d3pm_abi_version() == 6 and C.sizeof(_hip.Canvas) == 2 * C.sizeof(C.c_void_p)
    assert "d3pm_sampling" in header.split("#define D3PM_ABI_VERSION")[0], "the additions are listed in the version comment"
    # the step entry is the known-frame entry plus the struct; the loop entry the fp8 canvas loop plus a shared mask and the struct
    known = _hip.SIGNATURES["d3pm_posterior_sample_known"][1]
    assert _hip.SIGNATURES["d3pm_posterior_sample_sampling"][1] == known[:-1] + [C.POINTER(_hip.Sampling)] + known[-1:]
    loop = _hip.SIGNATURES["d3pm_sample_loop_fp8_canvas"][1]
    assert _hip.SIGNATURES["d3pm_sample_loop_sampling"][1] == loop[:5] + [C.c_void_p] + loop[5:-1] + [C.POINTER(_hip.Sampling)] + loop[-1:]


def _shape(n_q=1):
    from vall_e.vall_e import _hip, synth
    cfg = synth.D3PMConfig.native()
    sh = _hip.make_shape(cfg, torch.float16)
    sh.n_q = n_q
    return sh


BAD = [(0.0, 0), (-1.0, 0), (float("nan"), 0), (float("inf"), 0), (-float("inf"), 5), (1.0, -1), (1.0, 1026), (0.7, 5000)]


@pytest.mark.parametrize("tau,k", BAD)
def test_c_entries_refuse_bad_values_before_anything_else(built_lib, tau, k):
    """D3PM_E_ARG with a message that names the number, from both entries, with every pointer still NULL: the values are checked
    before the pointers are, and long before a launch (there is no GPU here)."""
    from vall_e.vall_e import _hip
    sh, sm = _shape(), _hip.Sampling(tau, k)
    rc = built_lib.d3pm_posterior_sample_sampling(C.byref(sh), 1, None, _hip.F16, None, None, None, 40, None, 0, 0, 0, None, C.byref(sm), None)
    assert rc == -1
    msg = built_lib.d3pm_last_error()
    assert (b"temperature" in msg) if not (tau > 0 and tau < float("inf")) else (b"top_k" in msg), msg
    dummy = C.c_uint8(1)
    rc = built_lib.d3pm_sample_loop_sampling(C.byref(sh), None, None, 1, None, C.addressof(dummy), None, 9, 0, None, None, None, None, 0, 0, 0,
                                             None, 0, None, C.byref(sm), None)
    assert rc == -1
    msg = built_lib.d3pm_last_error()
    assert b"temperature" in msg or b"top_k" in msg, msg


def test_c_entries_accept_good_values_up_to_the_pointer_checks(built_lib):
    """Valid options (the neutral pair, NULL, the extremes 1 and n_classes) pass the value check and fail at the NEXT one: the null
    pointers.  The loop entry wants exactly one of frame_mask / canvas."""
    from vall_e.vall_e import _hip
    sh = _shape()
    for sm in (None, _hip.Sampling(1.0, 0), _hip.Sampling(0.5, 1), _hip.Sampling(1.3, 1025), _hip.Sampling(1e-3, 50)):
        ref = None if sm is None else C.byref(sm)
        assert built_lib.d3pm_posterior_sample_sampling(C.byref(sh), 1, None, _hip.F16, None, None, None, 40, None, 0, 0, 0, None, ref, None) == -1
        assert b"null pointer" in built_lib.d3pm_last_error()
    dummy = C.c_uint8(1)
    cv = _hip.Canvas(C.addressof(dummy), None)
    args = (9, 0, None, None, None, None, 0, 0, 0, None, 0, None, None, None)
    assert built_lib.d3pm_sample_loop_sampling(C.byref(sh), None, None, 1, None, None, None, *args) == -1
    assert b"exactly one of" in built_lib.d3pm_last_error()
    assert built_lib.d3pm_sample_loop_sampling(C.byref(sh), None, None, 1, None, C.addressof(dummy), C.byref(cv), *args) == -1
    assert b"exactly one of" in built_lib.d3pm_last_error()
    assert built_lib.d3pm_sample_loop_sampling(C.byref(sh), None, None, 1, None, None, C.byref(cv), *args) == -1
    assert b"null pointer" in built_lib.d3pm_last_error()


def test_sampling_options_helper():
    from vall_e.vall_e import _hip
    assert _hip.sampling_options() is None and _hip.sampling_options(1.0, 0, 1025) is None and _hip.sampling_options(1, 0) is None
    s = _hip.sampling_options(0.7, 50, 1025)
    assert isinstance(s, _hip.Sampling) and s.top_k == 50 and s.temperature == C.c_float(0.7).value
    assert _hip.sampling_options(1.0, 1025, 1025).top_k == 1025          # {1, K} is not neutral: it takes the filter arm
    for tau, k in BAD + [("1", 0), (None, 0), (1.0, 2.5), (1.0, "3"), (True, 0), (1.0, True), (1e-60, 0), (1e60, 0)]:
        with pytest.raises(ValueError):
            _hip.sampling_options(tau, k, 1025)


_T = [torch.tensor([1, 2, 3])] * 2
_P = [torch.zeros(4, 8, dtype=torch.long)] * 2


def _native():
    from vall_e.vall_e import AR
    return AR.reference_native()          # parameters on the CPU


@pytest.mark.parametrize("kw", [dict(temperature=t, top_k=k) for t, k in BAD] + [
    dict(temperature="hot"), dict(top_k=1.5), dict(top_k=None),
    dict(temperature=0.7, graph=True), dict(top_k=50, graph=True),          # the graph path never ignores the options
])
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
    for kw in (dict(temperature=0.7), dict(top_k=50), dict(temperature=1.3, top_k=1025), dict(temperature=1.0, top_k=0, graph=True),
               dict(temperature=0.5, top_k=1, n_frames=[10, 448], known=[torch.tensor([1, 512]), None])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.generate_audio(_T, _P, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.p_sample(torch.zeros(1, 448, 1025), torch.tensor([40]), torch.zeros(1, 448, dtype=torch.int64), temperature=0.7, top_k=50)


def test_cli_parses_the_flags(monkeypatch, tmp_path):
    """--temperature / --top-k reach AR.generate_audio; a bad value is an argparse error (exit status 2) before a model is built."""
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

    monkeypatch.setattr(AR, "reference_native", classmethod(lambda cls: Fake()))
    monkeypatch.setattr(formats, "load_quants", lambda p: torch.zeros(5, 8, dtype=torch.long))
    monkeypatch.setattr(formats, "save_quants", lambda resps, path: seen.update(saved=tuple(resps.shape)))
    base = ["--native", "--phonemes", "1 2 3", "--prompt-qnt", "p.qnt.pt", str(tmp_path / "o.qnt.pt")]
    cli.main(base + ["--temperature", "0.7", "--top-k", "50"])
    assert seen["temperature"] == 0.7 and seen["top_k"] == 50 and seen["saved"] == (6, 1)
    seen.clear()
    cli.main(base)
    assert seen["temperature"] == 1.0 and seen["top_k"] == 0
    seen.clear()
    cli.main(base + ["--top-k", "3", "--frames", "4"])
    assert seen["top_k"] == 3 and seen["n_frames"] == [4]
    for bad in (["--temperature", "0"], ["--temperature", "nan"], ["--top-k", "-2"], ["--top-k", "1026"], ["--top-k", "x"]):
        seen.clear()
        with pytest.raises(SystemExit) as e:
            cli.main(base + bad)
        assert e.value.code == 2 and not seen, bad


# ---- data-parallel forwarding over gloo --------------------------------------------------------------------------------------
CANVAS = 16


class _FakeModel:
    class cfg:
        canvas, n_frames = CANVAS, 12
    device = torch.device("cpu")


class _FakeNAR:
    n_resp_levels, n_tokens = 7, 1024


def _recording_generate(log):
    def fn(texts, proms, *, seed, utt0, temperature, top_k, n_frames=None):
        log.append((utt0, temperature, top_k))
        rows = []
        for b, t in enumerate(texts):
            g = torch.Generator().manual_seed(seed * 1000 + utt0 + b + 7 * top_k)
            rows.append(torch.randint(0, 1024, (CANVAS,), generator=g) + int(t[0]))
        return torch.stack(rows) if len(rows) > 1 else rows[0]
    return fn


def _fake_nar(texts, proms, resps, *, seed, utt0):
    return [torch.cat([r.long(), torch.full((r.shape[0], 7), utt0 + b)], dim=-1) for b, r in enumerate(resps)]


def _run(dp, n_utts, rank, world):
    texts = [torch.tensor([i]) for i in range(n_utts)]
    log, log2 = [], []
    grid = dp.generate_audio_dp(_FakeModel(), texts, texts, seed=3, generate_fn=_recording_generate(log), temperature=0.7, top_k=50)
    codes = dp.generate_codes_dp(_FakeModel(), _FakeNAR(), texts, texts, seed=3, ar_fn=_recording_generate(log2), nar_fn=_fake_nar,
                                 temperature=1.3, top_k=9, n_frames=12)
    lo, hi = dp.shard_bounds(n_utts, world, rank)
    # every rank that has utterances hands both numbers on, unsliced (they are per call, not per utterance)
    assert log == ([(lo, 0.7, 50)] if hi > lo else []) and log2 == ([(lo, 1.3, 9)] if hi > lo else [])
    return grid, codes


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n_utts, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from vall_e.vall_e import dp
    q.put((rank,) + _run(dp, n_utts, rank, world))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_utts", [(2, 5), (3, 2)])
def test_dp_forwards_the_sampling_keywords(world, n_utts):
    from vall_e.vall_e import dp
    single, single_codes = _run(dp, n_utts, 0, 1)
    assert single.shape == (n_utts, CANVAS) and single_codes.shape == (n_utts, 12, 8)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_utts, q), daemon=True) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r, grid, codes in got:
        assert torch.equal(grid, single) and torch.equal(codes, single_codes), r


def test_real_generate_audio_signature_takes_what_dp_forwards():
    import inspect
    from vall_e.vall_e import AR
    for fn in (AR.generate_audio, AR.p_sample):
        p = inspect.signature(fn).parameters
        assert p["temperature"].default == 1.0 and p["top_k"].default == 0
        assert p["temperature"].kind is p["top_k"].kind is inspect.Parameter.KEYWORD_ONLY


# ---- compile time ----------------------------------------------------------------------------------------------------------------
def test_sampler_kernels_compile_without_scratch_and_keep_the_unfiltered_arms():
    """Every instantiation of the two sampler kernels -- with and without the filter arm -- compiles without scratch (the k-th
    largest search keeps its keys in registers), and each unfiltered instantiation still exists under its own name next to a
    *_filtered one (the neutral options launch it).  Cross-compiles, no GPU."""
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "d3pm_sample.hip", "posterior_sample"],
                         capture_output=True, text=True, timeout=900).stdout
    rows = [l for l in out.splitlines() if "posterior_sample" in l]
    plain = [l for l in rows if "_filtered" not in l]
    filt = [l for l in rows if "_filtered" in l]
    # 3 dtypes x {known, not} for the stand-alone kernel, 2 dtypes x {known, not} for the one with the next iteration's prep
    assert len(plain) == 10 and len(filt) == 10, out[-3000:]
    for l in rows:
        m = re.search(r"VGPR\s+(\d+).*scratch\s+(\d+)", l)
        assert m and int(m.group(2)) == 0, f"a sampler kernel with scratch: {l}"
        assert int(m.group(1)) <= 128, f"a sampler kernel below four waves per SIMD: {l}"

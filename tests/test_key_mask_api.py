"""Key-padding masks (include/d3pm_hip.h: d3pm_keys; AR.generate_audio(mask_padding=True)): what can be checked without a GPU --
the derivation of the three key counts, the ValueErrors before any GPU work, the C symbols and their Python bindings."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

NEW_ENTRIES = ("d3pm_encode_conditions_keys", "d3pm_denoise_step_keys", "d3pm_sample_loop_keys", "d3pm_reveal_loop_keys",
               "d3pm_op_attention_pair_keylen")
_T = [torch.tensor([1, 2, 3]), torch.tensor([4, 5])]
_P = [torch.zeros(4, 8, dtype=torch.long)] * 2


def _native():
    from vall_e.vall_e import AR
    return AR.reference_native()          # parameters on the CPU


def test_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
    m = re.search(r"typedef struct d3pm_keys \{([^}]*)\} d3pm_keys;", header, re.S)
    assert m and re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", m.group(1))).split() == "const int32_t *frames, *text, *prompt;".split()
    assert [(n, t) for n, t in _hip.Keys._fields_] == [("frames", C.c_void_p), ("text", C.c_void_p), ("prompt", C.c_void_p)]
    assert C.sizeof(_hip.Keys) == 24
    assert built_lib.d3pm_abi_version() == 6      # additions only
    version_comment = header.split("#define D3PM_ABI_VERSION")[0]
    for word in ("d3pm_keys",) + NEW_ENTRIES:
        assert word in version_comment, word
    # each *_keys entry is the generalised entry's argument list with the d3pm_keys pointer in front of the stream
    for new, old in (("d3pm_encode_conditions_keys", "d3pm_encode_conditions"), ("d3pm_denoise_step_keys", "d3pm_denoise_step_canvas"),
                     ("d3pm_sample_loop_keys", "d3pm_sample_loop_nucleus"), ("d3pm_reveal_loop_keys", "d3pm_reveal_loop")):
        a, b = _hip.SIGNATURES[new][1], _hip.SIGNATURES[old][1]
        assert a == b[:-1] + [C.POINTER(_hip.Keys), C.c_void_p], new
    a, b = _hip.SIGNATURES["d3pm_op_attention_pair_keylen"][1], _hip.SIGNATURES["d3pm_op_attention_pair"][1]
    assert a == b[:-2] + [C.c_void_p, C.c_void_p] + b[-2:]
    # the contract that cannot be checked on the device is written down
    assert "leading ones" in header and "1 <= frames[b] <= canvas" in header


def test_length_derivation_and_truncation():
    from vall_e.vall_e import _hip
    f, t, p = _hip.key_lengths([37, 448, 1], [20, 50, 77], [100, 398, 1000], canvas=448, s_text=50, s_prompt=398)
    assert (f, t, p) == ([37, 448, 1], [20, 50, 50], [100, 398, 398])
    m = _native()
    cfg = m.cfg
    texts = [torch.ones(3, dtype=torch.long), torch.ones(cfg.s_text + 9, dtype=torch.long)]
    proms = [torch.zeros(4, 8, dtype=torch.long), torch.zeros(cfg.s_prompt + 1, 8, dtype=torch.long)]
    assert m.key_lengths(texts, proms) == ([cfg.n_frames] * 2, [3, cfg.s_text], [4, cfg.s_prompt])
    assert m.key_lengths(texts, proms, 17)[0] == [17, 17]
    assert m.key_lengths(texts, proms, [5, cfg.canvas])[0] == [5, cfg.canvas]


@pytest.mark.parametrize("bad", [dict(n_frames=[0, 3]), dict(n_frames=[3, 449]), dict(text_lens=[0, 3]), dict(prompt_lens=[3, 0]),
                                 dict(n_frames=[3])], ids=repr)
def test_key_lengths_refuses(bad):
    from vall_e.vall_e import _hip
    kw = dict(n_frames=[3, 4], text_lens=[3, 4], prompt_lens=[3, 4])
    kw.update(bad)
    with pytest.raises(ValueError, match="mask_padding"):
        _hip.key_lengths(kw["n_frames"], kw["text_lens"], kw["prompt_lens"], 448, 50, 398)


@pytest.mark.parametrize("kw,texts,proms", [
    (dict(graph=True), _T, _P), (dict(fp8=True), _T, _P),
    (dict(), [torch.tensor([1, 2]), torch.zeros(0, dtype=torch.long)], _P),
    (dict(), _T, [torch.zeros(4, 8, dtype=torch.long), torch.zeros(0, 8, dtype=torch.long)]),
    (dict(n_frames=[5, 0]), _T, _P),
], ids=["graph", "fp8", "empty_text", "empty_prompt", "no_frames"])
def test_generate_audio_rejects_on_the_host(kw, texts, proms):
    """ValueError before anything touches the GPU: the model lives on the CPU here, and a valid call raises the RuntimeError of a
    missing HIP device instead."""
    with pytest.raises(ValueError):
        _native().generate_audio(texts, proms, mask_padding=True, **kw)


def test_an_empty_text_is_legal_without_the_mask_and_valid_options_reach_the_device_check():
    m = _native()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.generate_audio([torch.tensor([1, 2]), torch.zeros(0, dtype=torch.long)], _P)
    for kw in (dict(), dict(n_frames=[10, 448]), dict(reveal_steps=4, top_p=0.9), dict(streams=2, greedy=True), dict(return_trace=True),
               dict(n_frames=[10, 448], known=[torch.tensor([1, 512]), None])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.generate_audio(_T, _P, mask_padding=True, **kw)


def test_signatures_and_docs():
    from vall_e.vall_e import AR, _hip
    p = inspect.signature(AR.generate_audio).parameters
    assert p["mask_padding"].default is False and p["mask_padding"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (_hip.Sampler.denoise_canvas, _hip.Sampler.sample_loop, _hip.Sampler.reveal_loop):
        assert inspect.signature(fn).parameters["keys"].default is None
    q = inspect.signature(_hip.Sampler.encode_conditions).parameters
    assert q["text_len"].default is None and q["prom_len"].default is None
    q = inspect.signature(_hip.op_attention_pair).parameters
    assert q["key_len"].default is None and q["key_len2"].default is None
    assert "trained with the padding as keys" in AR.generate_audio.__doc__


def test_make_keys_validates_on_the_host():
    from vall_e.vall_e import _hip
    cpu = torch.device("cpu")
    ok = torch.ones(2, dtype=torch.int32)
    ks = _hip.make_keys((ok, None, ok), 2, cpu)
    assert ks.frames == ok.data_ptr() and ks.text is None and ks.prompt == ok.data_ptr()
    assert _hip.make_keys(None, 2, cpu) is None
    for bad in ((ok, ok), (ok.long(), None, None), (None, torch.ones(3, dtype=torch.int32), None), (None, None, torch.ones(4, dtype=torch.int32)[::2]),
                (None, None, [1, 2])):
        with pytest.raises(_hip.D3PMError, match="keys"):
            _hip.make_keys(bad, 2, cpu)


def test_cli_and_dp_forward_the_flag(monkeypatch, tmp_path):
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
        cli.main(base + ["--mask-padding"])
    assert seen["mask_padding"] is True
    seen.clear()
    with pytest.raises(Stop):
        cli.main(base)
    assert seen["mask_padding"] is False
    got = {}

    class M:
        class cfg:
            canvas, n_q = 4, 1
        device = "cpu"

        def generate_audio(self, texts, proms, **kw):
            got.update(kw)
            return torch.zeros(len(texts), 4, dtype=torch.long)

    dp.generate_audio_dp(M(), _T, _P, seed=1, mask_padding=True)
    assert got["mask_padding"] is True and got["global_batch"] == 2


def test_masked_kernels_have_no_scratch():
    """hipcc's resource remarks for the masked instantiations (a `true` template argument): no scratch, and the pipelined walk
    keeps its three waves per SIMD."""
    import subprocess
    for src, pat in (("d3pm_mfma_attn32.hip", r"attn32p_hd64|attn32_hd64|attn32_cross_hd64"), ("d3pm_mfma_attn.hip", r"attn_cross_hd64")):
        out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), src, pat], capture_output=True, text=True, check=True).stdout
        rows = [ln for ln in out.splitlines() if "VGPR" in ln]
        masked = [ln for ln in rows if re.search(r"Lb1E", ln) or "true" in ln.split("VGPR")[0]]
        assert masked, out
        for ln in rows:
            assert re.search(r"scratch\s+0\b", ln), ln
        for ln in masked:
            if "attn32p_hd64" in ln:
                assert re.search(r"occ 3\b", ln), ln

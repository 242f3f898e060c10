"""ctypes binding of libd3pm_hip.so (C ABI in include/d3pm_hip.h).

There is deliberately no CPU fallback: if the shared library is missing the import of the
sampler fails loudly (build it with `python -c "import __graft_entry__ as g; g.build()"`).
PyTorch is used only to own device memory and to provide the current HIP stream.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from numbers import Integral

import numpy as np
import torch

F32, F16, BF16 = 0, 1, 2
ABI_VERSION = 6
FLAG_GREEDY, FLAG_FORCE_GENERIC, FLAG_SEED_IN_HBM = 1, 2, 4
K_GEMM, K_ATTN, K_SAMPLE, K_LN, K_GEMM_LN, K_ALL = 0, 1, 2, 3, 4, 5

_DTYPES = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
_LIB_DIR = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "lib"))
LIB_PATH = os.environ.get("D3PM_HIP_LIB") or os.path.join(_LIB_DIR, "libd3pm_hip.so")


class Tuning(C.Structure):
    """d3pm_tuning (include/d3pm_hip.h): schedule choices, every value bit-identical.  The C library keeps no state: a
    pointer to one of these travels in the shape structs.  `TUNING` below is this module's default instance."""
    _fields_ = [(n, C.c_int32) for n in ("gemm_variant", "gemm_persist_slots", "lat_tile", "attn_query_groups",
                                         "attn_pair_sequential", "attn_cross_resident", "row_panel", "workspace_alias",
                                         "regime_batch", "ln_fold")] + \
               [("prof", C.c_void_p)]


class Shape(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d_model", "n_heads", "n_layers", "canvas", "s_text", "s_prompt",
                                         "n_classes", "mask_id", "timesteps", "dtype", "n_q")] + [("tuning", C.POINTER(Tuning))]


_BLOCK_FIELDS = ("norm1_w", "norm1_b", "attn_in_w", "attn_in_b", "attn_out_w", "attn_out_b", "norm2_w", "norm2_b",
                 "norm22_w", "norm22_b", "cross_in_w", "cross_in_b", "cross_out_w", "cross_out_b", "norm3_w",
                 "norm3_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "tfc_w", "tfc_b")


class BlockWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _BLOCK_FIELDS]


class FoldBlock(C.Structure):
    """d3pm_fold_block: a block's LayerNorms folded into the projections they feed (filled by d3pm_fold_build)."""
    _fields_ = [(n, C.c_void_p) for n in ("qkv_w", "qkv_s", "qkv_b", "q2_w", "q2_s", "q2_b")]


class Weights(C.Structure):
    _fields_ = [("resps_emb", C.c_void_p), ("time_emb", C.c_void_p), ("final_w", C.c_void_p),
                ("final_b", C.c_void_p), ("blocks", C.POINTER(BlockWeights)), ("fold", C.POINTER(FoldBlock))]


_ENC_LAYER_FIELDS = ("in_w", "in_b", "out_w", "out_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b", "norm1_w", "norm1_b",
                     "norm2_w", "norm2_b")


class EncoderLayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _ENC_LAYER_FIELDS]


class EncoderWeights(C.Structure):
    _fields_ = [("layers", C.POINTER(EncoderLayerWeights)), ("n_layers", C.c_int32), ("n_heads", C.c_int32),
                ("d_ff", C.c_int32), ("mlp_hidden", C.c_int32), ("fc1_w", C.c_void_p), ("fc1_b", C.c_void_p),
                ("fc2_w", C.c_void_p), ("fc2_b", C.c_void_p)]


class CondWeights(C.Structure):
    _fields_ = [("text_emb", C.c_void_p), ("proms_emb", C.c_void_p), ("pe_text0", C.c_void_p),
                ("pe_prompt", C.c_void_p), ("n_levels", C.c_int32), ("text_encoder", EncoderWeights),
                ("prompt_encoder", EncoderWeights)]


class NarShape(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d_model", "n_heads", "n_layers", "n_tokens", "n_prom_levels", "n_resp_levels",
                                         "dtype")] + [("tuning", C.POINTER(Tuning))]


_NAR_BLOCK_FIELDS = ("attn_norm_emb", "to_qkv_w", "to_out_w", "to_out_b", "ffn_norm_emb", "ffn0_w", "ffn0_b", "ffn3_w",
                     "ffn3_b")


class NarBlockWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _NAR_BLOCK_FIELDS]


class NarWeights(C.Structure):
    _fields_ = [("text_emb", C.c_void_p), ("proms_emb", C.c_void_p), ("resps_emb", C.c_void_p), ("sep", C.c_void_p),
                ("classifier_w", C.c_void_p), ("classifier_b", C.c_void_p), ("pe", C.c_void_p), ("pe_rows", C.c_int32),
                ("blocks", C.POINTER(NarBlockWeights))]


class Canvas(C.Structure):
    """d3pm_canvas: per-utterance frame masks and the optional known-frame map, both device uint8 [batch][canvas]."""
    _fields_ = [("frame_mask", C.c_void_p), ("known", C.c_void_p)]


class Keys(C.Structure):
    """d3pm_keys: per-utterance key counts (device int32 [batch] each, or NULL) of the DiT self-attention (frames), of the text
    cross-attention / text encoder (text) and of the prompt cross-attention / prompt encoder (prompt) -- include/d3pm_hip.h."""
    _fields_ = [("frames", C.c_void_p), ("text", C.c_void_p), ("prompt", C.c_void_p)]


def key_lengths(n_frames, text_lens, prompt_lens, canvas, s_text, s_prompt):
    """The three key counts of `mask_padding` from per-utterance lengths (host ints): frames[b] = L_b, text[b] = min(len(text_b),
    s_text), prompt[b] = min(rows(prom_b), s_prompt) -> three lists of ints.  ValueError for an utterance without a frame, a
    phoneme or a prompt frame (a softmax over no key is undefined), or with more frames than the canvas."""
    n_frames, text_lens, prompt_lens = [int(v) for v in n_frames], [int(v) for v in text_lens], [int(v) for v in prompt_lens]
    if not (len(n_frames) == len(text_lens) == len(prompt_lens)):
        raise ValueError(f"mask_padding: {len(n_frames)} frame counts, {len(text_lens)} texts and {len(prompt_lens)} prompts")
    for b, (f, t, p) in enumerate(zip(n_frames, text_lens, prompt_lens)):
        if not 1 <= f <= canvas:
            raise ValueError(f"mask_padding: utterance {b} has {f} frames, outside 1..{canvas}")
        if t < 1:
            raise ValueError(f"mask_padding: utterance {b} has an empty text")
        if p < 1:
            raise ValueError(f"mask_padding: utterance {b} has an empty prompt")
    return n_frames, [min(t, s_text) for t in text_lens], [min(p, s_prompt) for p in prompt_lens]


def _key_array(t, name, B, device):
    """One d3pm_keys member: None, or a contiguous int32 [B] tensor on `device` (the values are read by the kernels only)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B,) or t.device != device or not t.is_contiguous():
        raise D3PMError(f"keys.{name} must be a contiguous int32 [{B}] tensor on {device}")
    return t


def make_keys(keys, B, device):
    """keys: None, or (frames, text, prompt) -- each None or int32 [B] on the device -> a Keys struct that keeps its tensors alive."""
    if keys is None:
        return None
    if not isinstance(keys, (tuple, list)) or len(keys) != 3:
        raise D3PMError("keys must be a (frames, text, prompt) triple of int32 [B] device tensors (None = that attention is not masked)")
    kept = tuple(_key_array(t, n, B, device) for t, n in zip(keys, ("frames", "text", "prompt")))
    ks = Keys(*(None if t is None else t.data_ptr() for t in kept))
    ks._keep = kept
    return ks


class Sampling(C.Structure):
    """d3pm_sampling: temperature and top-k on the x0-logits of the D3PM sampler (include/d3pm_hip.h)."""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32)]


def sampling_options(temperature=1.0, top_k=0, n_classes=None):
    """Host validation of the two sampling options (ValueError, before any GPU work) -> a Sampling struct, or None for the neutral
    pair (temperature 1, top_k 0), which runs the entries and the kernels that know nothing of the filter."""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)):
        raise ValueError(f"temperature must be a number, got {temperature!r}")
    tau = float(temperature)
    if not (math.isfinite(tau) and tau > 0.0) or not math.isfinite(C.c_float(tau).value) or C.c_float(tau).value <= 0.0:
        raise ValueError(f"temperature must be finite and > 0, got {temperature!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, Integral):
        raise ValueError(f"top_k must be an int, got {top_k!r}")
    k = int(top_k)
    if k < 0 or (n_classes is not None and k > n_classes):
        raise ValueError(f"top_k must be 0 (off) or 1..{n_classes}, got {k}")
    tau = C.c_float(tau).value
    if tau == 1.0 and k == 0:
        return None
    return Sampling(tau, k)


class Nucleus(C.Structure):
    """d3pm_nucleus: d3pm_sampling plus the nucleus (top-p) cut behind it (include/d3pm_hip.h)."""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float)]


def nucleus_options(temperature=1.0, top_k=0, top_p=1.0, n_classes=None):
    """Host validation of the three sampling options (ValueError, before any GPU work) -> None for the neutral triple (1, 0, 1), what
    sampling_options returns when top_p == 1 (the entries and kernels that know nothing of the nucleus), a Nucleus struct otherwise."""
    smp = sampling_options(temperature, top_k, n_classes)
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)):
        raise ValueError(f"top_p must be a number, got {top_p!r}")
    p = float(top_p)
    if not (math.isfinite(p) and 0.0 < p <= 1.0) or not 0.0 < C.c_float(p).value <= 1.0:
        raise ValueError(f"top_p must be finite, > 0 and <= 1 (1 = off), got {top_p!r}")
    p = C.c_float(p).value
    if p == 1.0:
        return smp
    return Nucleus(1.0, 0, p) if smp is None else Nucleus(smp.temperature, smp.top_k, p)


class NarDraw(C.Structure):
    """d3pm_nar_draw: the options of the NAR stage's level draw (include/d3pm_hip.h)."""
    _fields_ = [("top_p", C.c_float), ("top_k", C.c_int32), ("known", C.c_void_p), ("logprob_out", C.c_void_p), ("theta_out", C.c_void_p)]


def nar_draw_options(top_k=0, top_p=1.0, n_tokens=None):
    """Host validation of the NAR draw's two filter options (ValueError, before any GPU work) -> (top_k, top_p as the float the
    library receives)."""
    if isinstance(top_k, bool) or not isinstance(top_k, Integral):
        raise ValueError(f"top_k must be an int, got {top_k!r}")
    k = int(top_k)
    if k < 0 or (n_tokens is not None and k > n_tokens):
        raise ValueError(f"top_k must be 0 (off) or 1..{n_tokens}, got {k}")
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)):
        raise ValueError(f"top_p must be a number, got {top_p!r}")
    p = float(top_p)
    if not (math.isfinite(p) and 0.0 < p <= 1.0) or not 0.0 < C.c_float(p).value <= 1.0:
        raise ValueError(f"top_p must be finite, > 0 and <= 1 (1 = off), got {top_p!r}")
    return k, C.c_float(p).value


def nar_draw_struct(top_k=0, top_p=1.0, known=None, logprob_out=None, theta_out=None):
    """-> None for the neutral options (the entries and the kernel that know nothing of them), else a NarDraw over the tensors'
    addresses (the caller keeps the tensors alive over the call)."""
    if top_k == 0 and top_p == 1.0 and known is None and logprob_out is None and theta_out is None:
        return None
    return NarDraw(top_p, top_k, _p(known), _p(logprob_out), _p(theta_out))


class Guidance(C.Structure):
    """d3pm_guidance: the weight w of classifier-free guidance, z = rn16(fmaf(w, c - u, c)) (include/d3pm_hip.h)."""
    _fields_ = [("weight", C.c_float)]


def guidance_options(guidance=0.0):
    """Host validation of the guidance weight (ValueError, before any GPU work) -> None for 0 (the entries and kernels that know
    nothing of guidance), a Guidance struct otherwise."""
    if isinstance(guidance, bool) or not isinstance(guidance, (int, float)):
        raise ValueError(f"guidance must be a number, got {guidance!r}")
    w = float(guidance)
    if not (math.isfinite(w) and w >= 0.0) or not math.isfinite(C.c_float(w).value):
        raise ValueError(f"guidance must be finite and >= 0 (0 = off), got {guidance!r}")
    w = C.c_float(w).value
    return None if w == 0.0 else Guidance(w)


class Reveal(C.Structure):
    """d3pm_reveal: the confidence-ordered reveal schedule, N denoiser evaluations (include/d3pm_hip.h)."""
    _fields_ = [("n_steps", C.c_int32), ("choice_temperature", C.c_float)]


def reveal_options(reveal_steps, choice_temperature=0.0, timesteps=None):
    """Host validation of the reveal schedule's two numbers (ValueError, before any GPU work) -> a Reveal struct, or None when
    reveal_steps is None (the D3PM loop; a choice_temperature other than 0 then has nothing to act on and is refused)."""
    if isinstance(choice_temperature, bool) or not isinstance(choice_temperature, (int, float)):
        raise ValueError(f"choice_temperature must be a number, got {choice_temperature!r}")
    ct = float(choice_temperature)
    if not (math.isfinite(ct) and ct >= 0.0) or not math.isfinite(C.c_float(ct).value):
        raise ValueError(f"choice_temperature must be finite and >= 0, got {choice_temperature!r}")
    if reveal_steps is None:
        if ct != 0.0:
            raise ValueError("choice_temperature without reveal_steps")
        return None
    if isinstance(reveal_steps, bool) or not isinstance(reveal_steps, Integral):
        raise ValueError(f"reveal_steps must be an int, got {reveal_steps!r}")
    n = int(reveal_steps)
    if n < 1 or (timesteps is not None and n > timesteps - 1):
        raise ValueError(f"reveal_steps must be in 1..{None if timesteps is None else timesteps - 1}, got {n}")
    return Reveal(n, C.c_float(ct).value)


class Revise(C.Structure):
    """d3pm_revise: the reveal schedule whose held frames compete again in every step (include/d3pm_hip.h)."""
    _fields_ = [("hold_bonus", C.c_float)]


def revise_options(revise=None):
    """Host validation of the revise option (ValueError, before any GPU work) -> None for None (the entries and kernels that know
    nothing of it), a Revise struct for a real number >= 0: the hold bonus, 0 included."""
    if revise is None:
        return None
    if isinstance(revise, bool) or not isinstance(revise, (int, float)):
        raise ValueError(f"revise must be None or a number (the hold bonus), got {revise!r}")
    hb = float(revise)
    if not (math.isfinite(hb) and hb >= 0.0) or not math.isfinite(C.c_float(hb).value):
        raise ValueError(f"revise (the hold bonus) must be finite and >= 0, got {revise!r}")
    return Revise(C.c_float(hb).value)


class FrameScores(C.Structure):
    """d3pm_frame_scores: the two device grids [batch][canvas] of the per-frame log-probability (include/d3pm_hip.h)."""
    _fields_ = [("logprob", C.c_void_p), ("step", C.c_void_p)]


class ScheduleC(C.Structure):
    _fields_ = [("timesteps", C.c_int32), ("d", C.POINTER(C.c_uint16)), ("c", C.POINTER(C.c_uint16)),
                ("dbar", C.POINTER(C.c_uint16)), ("cbar", C.POINTER(C.c_uint16))]


_lib = None

# name -> (restype, argtypes); every symbol include/d3pm_hip.h declares
SIGNATURES = {
    "d3pm_abi_version": (C.c_int, []),
    "d3pm_last_error": (C.c_char_p, []),
    "d3pm_schedule_build": (C.c_int, [C.c_int] + [C.POINTER(C.c_uint16)] * 5),
    "d3pm_workspace_bytes": (C.c_size_t, [C.POINTER(Shape), C.c_int]),
    "d3pm_film_table": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_void_p]),
    "d3pm_fold_bytes": (C.c_size_t, [C.POINTER(Shape)]),
    "d3pm_fold_build": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_size_t, C.POINTER(FoldBlock), C.c_void_p]),
    "d3pm_op_row_stats": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "d3pm_op_linear_stats": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_linear_fold": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_dedup_index": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11),
    "d3pm_op_dedup_index_align": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11),
    "d3pm_op_linear_live": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_linear_live_est": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_linear_live_rows": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_int, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_embed_qkv_bytes": (C.c_size_t, [C.POINTER(Shape), C.c_int]),
    "d3pm_op_embed_qkv": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "d3pm_op_fold_weights": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "d3pm_cond_kv": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_int] + [C.c_void_p] * 5),
    "d3pm_cond_workspace_bytes": (C.c_size_t, [C.POINTER(Shape), C.POINTER(CondWeights), C.c_int]),
    "d3pm_encode_conditions": (C.c_int, [C.POINTER(Shape), C.POINTER(CondWeights), C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "d3pm_encode_conditions_keys": (C.c_int, [C.POINTER(Shape), C.POINTER(CondWeights), C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(Keys), C.c_void_p]),
    "d3pm_denoise_step_keys": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_int, C.c_void_p, C.POINTER(Canvas), C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_uint32, C.POINTER(Keys), C.c_void_p]),
    "d3pm_sample_loop_keys": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.POINTER(Canvas), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.POINTER(Nucleus), C.POINTER(Keys), C.c_void_p]),
    "d3pm_reveal_loop_keys": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Canvas),
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(Nucleus), C.POINTER(Reveal), C.POINTER(Keys),
                                        C.c_void_p]),
    "d3pm_op_attention_pair_keylen": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_posterior_sample_guided": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Canvas),
                                               C.c_int, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(Nucleus),
                                               C.POINTER(Guidance), C.c_void_p]),
    "d3pm_sample_loop_guided": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.POINTER(Canvas), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.POINTER(Nucleus), C.POINTER(Keys), C.POINTER(Guidance), C.c_void_p]),
    "d3pm_frame_scores_init": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Canvas), C.POINTER(FrameScores),
                                         C.c_void_p]),
    "d3pm_frame_scores_step": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(Guidance), C.c_void_p,
                                         C.c_int, C.POINTER(FrameScores), C.c_void_p]),
    "d3pm_sample_loop_scored": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.POINTER(Canvas), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.POINTER(Nucleus), C.POINTER(Keys), C.POINTER(Guidance), C.POINTER(FrameScores),
                                          C.c_void_p]),
    "d3pm_reveal_loop_scored": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Canvas),
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                          C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(Nucleus), C.POINTER(Reveal), C.POINTER(Keys),
                                          C.POINTER(FrameScores), C.c_void_p]),
    "d3pm_reveal_step_revise": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(Canvas), C.c_int, C.c_int, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                          C.POINTER(Nucleus), C.c_float, C.c_void_p, C.c_void_p, C.POINTER(Revise), C.POINTER(FrameScores),
                                          C.c_void_p]),
    "d3pm_reveal_loop_revise": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Canvas),
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                          C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(Nucleus), C.POINTER(Reveal), C.POINTER(Keys),
                                          C.POINTER(Revise), C.POINTER(FrameScores), C.c_void_p]),
    "d3pm_denoise_step": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]),
    "d3pm_posterior_sample": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p]),
    "d3pm_sample_loop": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScheduleC), C.c_uint64,
                                   C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "d3pm_denoise_step_canvas": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_int, C.c_void_p, C.POINTER(Canvas), C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]),
    "d3pm_posterior_sample_known": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_void_p]),
    "d3pm_sample_loop_canvas": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_int, C.c_void_p, C.POINTER(Canvas), C.c_int,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScheduleC), C.c_uint64,
                                          C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "d3pm_sample_loop_fp8_canvas": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_int, C.c_void_p,
                                              C.POINTER(Canvas), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_void_p]),
    "d3pm_posterior_sample_sampling": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                                 C.c_void_p, C.POINTER(Sampling), C.c_void_p]),
    "d3pm_sample_loop_sampling": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                            C.POINTER(Canvas), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.POINTER(Sampling), C.c_void_p]),
    "d3pm_posterior_sample_nucleus": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                                C.c_void_p, C.POINTER(Nucleus), C.c_void_p, C.c_void_p]),
    "d3pm_sample_loop_nucleus": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                           C.POINTER(Canvas), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.POINTER(Nucleus), C.c_void_p]),
    "d3pm_reveal_plan": (C.c_int, [C.POINTER(ScheduleC), C.c_int, C.POINTER(C.c_int32)]),
    "d3pm_reveal_step": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(Canvas), C.c_int, C.c_int, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.POINTER(Nucleus), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "d3pm_reveal_loop": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Canvas),
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(Nucleus), C.POINTER(Reveal), C.c_void_p]),
    "d3pm_q_sample": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_void_p]),
    "d3pm_denoise_step_fp8": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]),
    "d3pm_sample_loop_fp8": (C.c_int, [C.POINTER(Shape), C.POINTER(Weights), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScheduleC),
                                       C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "d3pm_op_quantize_mx": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "d3pm_op_layernorm_mx": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "d3pm_op_layernorm_mx_pair": (C.c_int, [C.c_int] + [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "d3pm_op_linear_mx": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_ce_loss_rows": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "d3pm_uniform": (C.c_int, [C.c_uint64, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "d3pm_nar_workspace_bytes": (C.c_size_t, [C.POINTER(NarShape), C.c_int, C.c_int]),
    "d3pm_nar_level": (C.c_int, [C.POINTER(NarShape), C.POINTER(NarWeights), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64,
                                 C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "d3pm_nar_level_draw": (C.c_int, [C.POINTER(NarShape), C.POINTER(NarWeights), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64,
                                      C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(NarDraw), C.c_void_p]),
    "d3pm_nar_level_guided": (C.c_int, [C.POINTER(NarShape), C.POINTER(NarWeights), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64,
                                        C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(NarDraw),
                                        C.POINTER(Guidance), C.c_void_p]),
    "d3pm_op_linear": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_attention": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                    C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_attention_keylen": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                           C.c_void_p, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_attention_gather": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                           C.c_void_p, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_attention_gather_pool": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_attention_pair": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_float, C.POINTER(Tuning), C.c_void_p]),
    "d3pm_op_attention_pair_segments": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Tuning),
                                                  C.c_void_p]),
    "d3pm_op_posterior_sample_rows": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.POINTER(ScheduleC), C.c_uint64, C.c_uint32, C.c_uint32,
                                                C.POINTER(Nucleus), C.POINTER(Guidance), C.c_void_p]),
    "d3pm_op_nar_embed": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "d3pm_op_adaln": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "d3pm_op_nar_sample": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_float, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]),
    "d3pm_op_nar_draw": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_float, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(NarDraw), C.c_void_p]),
    "d3pm_op_nar_draw_guided": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_float, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(NarDraw), C.POINTER(Guidance),
                                          C.c_void_p]),
    "d3pm_op_layernorm": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_float, C.c_void_p]),
    "d3pm_op_linear_rowpanel": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "d3pm_op_cond_embed": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p]),
    "d3pm_op_matmul_f32": (C.c_int, [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "d3pm_op_colsum_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p]),
    "d3pm_op_act_bwd_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "d3pm_op_mask_rows_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "d3pm_op_layernorm_bwd_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "d3pm_op_attention_bwd_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "d3pm_op_ce_bwd_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                     C.c_int, C.c_void_p]),
    "d3pm_op_embed_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "d3pm_op_embed_bwd_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p]),
    "d3pm_op_dropout_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                      C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]),
    "d3pm_op_attention_dropout_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint64, C.c_uint32,
                                                C.c_uint32, C.c_void_p]),
    "d3pm_op_attention_bwd_dropout_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                    C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_uint32,
                                                    C.c_uint32, C.c_void_p]),
    "d3pm_op_attention_dropout_keylen_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_float, C.c_uint64,
                                                       C.c_uint32, C.c_uint32, C.c_void_p]),
    "d3pm_op_attention_bwd_keylen_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                   C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_uint64,
                                                   C.c_uint32, C.c_uint32, C.c_void_p]),
    "d3pm_op_adaln_bwd_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p]),
    "d3pm_op_nar_embed_bwd_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                            C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_void_p]),
    "d3pm_op_nar_ce_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "d3pm_tuning_default": (None, [C.POINTER(Tuning)]),
    "d3pm_prof_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "d3pm_prof_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double)]),
    "d3pm_prof_read_class": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double)]),
    "d3pm_prof_destroy": (C.c_int, [C.c_void_p]),
}

TUNING = Tuning()        # filled by d3pm_tuning_default when the library loads
TUNING_FIELDS = tuple(n for n, _ in Tuning._fields_ if n != "prof")


def _load(path, signatures):
    if not os.path.isfile(path):
        raise RuntimeError(f"{path} is missing: the HIP extension has not been built "
                           "(run __graft_entry__.build()); there is no CPU fallback")
    handle = C.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    if handle.d3pm_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{os.path.basename(path)} ABI version mismatch")
    return handle


def lib():
    """The loaded library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, SIGNATURES)
        _lib.d3pm_tuning_default(C.byref(TUNING))
    return _lib


class D3PMError(RuntimeError):
    pass


def check(rc: int, what: str):
    if rc != 0:
        raise D3PMError(f"{what} failed with code {rc}: {lib().d3pm_last_error().decode()}")


def dtype_code(dtype: torch.dtype) -> int:
    try:
        return _DTYPES[dtype]
    except KeyError:
        raise D3PMError(f"unsupported model dtype {dtype}") from None


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


class Schedule:
    """Host-side fp16 schedule scalars (d3pm_schedule_build)."""

    def __init__(self, timesteps: int):
        self.timesteps = timesteps
        self.betas = np.zeros(timesteps + 1, np.uint16)
        self.d, self.c, self.dbar, self.cbar = (np.zeros(timesteps, np.uint16) for _ in range(4))
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
        check(lib().d3pm_schedule_build(timesteps, p(self.betas), p(self.d), p(self.c), p(self.dbar), p(self.cbar)),
              "d3pm_schedule_build")
        self.c_struct = ScheduleC(timesteps, p(self.d), p(self.c), p(self.dbar), p(self.cbar))


def make_shape(cfg, dtype: torch.dtype, tuning: "Tuning | None" = None) -> Shape:
    lib()                                             # TUNING holds the library's defaults from here on
    return Shape(cfg.d_model, cfg.n_heads, cfg.n_layers, cfg.canvas, cfg.s_text, cfg.s_prompt, cfg.n_classes,
                 cfg.mask_id, cfg.timesteps, dtype_code(dtype), getattr(cfg, "n_q", 1),
                 C.pointer(tuning if tuning is not None else TUNING))


class DeviceWeights:
    """Pointer table over tensors that stay owned by the caller (an nn.Module's parameters)."""

    def __init__(self, tensors: dict, n_layers: int):
        self._keep = []

        def ptr(key):
            t = tensors[key]
            if not (t.is_cuda and t.is_contiguous()):
                raise D3PMError(f"weight {key} must be a contiguous device tensor")
            self._keep.append(t)
            return t.data_ptr()

        self.blocks = (BlockWeights * n_layers)()
        # n_q > 1: resps_emb.weight is [n_q, K, d] and final.{weight, bias} are [n_q * K, d] / [n_q * K], both contiguous -- the
        # layouts d3pm_weights documents
        names = {"norm1_w": "norm1.weight", "norm1_b": "norm1.bias", "attn_in_w": "attn.in_proj_weight",
                 "attn_in_b": "attn.in_proj_bias", "attn_out_w": "attn.out_proj.weight",
                 "attn_out_b": "attn.out_proj.bias", "norm2_w": "norm2.weight", "norm2_b": "norm2.bias",
                 "norm22_w": "norm22.weight", "norm22_b": "norm22.bias", "cross_in_w": "cross_attn.in_proj_weight",
                 "cross_in_b": "cross_attn.in_proj_bias", "cross_out_w": "cross_attn.out_proj.weight",
                 "cross_out_b": "cross_attn.out_proj.bias", "norm3_w": "norm3.weight", "norm3_b": "norm3.bias",
                 "fc1_w": "mlp.fc1.weight", "fc1_b": "mlp.fc1.bias", "fc2_w": "mlp.fc2.weight",
                 "fc2_b": "mlp.fc2.bias", "tfc_w": "timestep_fc.weight", "tfc_b": "timestep_fc.bias"}
        for i in range(n_layers):
            for field, key in names.items():
                setattr(self.blocks[i], field, ptr(f"blocks.{i}.{key}"))
        self.c_struct = Weights(ptr("resps_emb.weight"), ptr("time_emb.weight"), ptr("final.weight"),
                                ptr("final.bias"), self.blocks, None)
        self.fold_blocks = self.fold_storage = None

    def build_fold(self, shape: "Shape", device):
        """The LayerNorm-folded projection tables (d3pm_fold_build): W o gamma for the QKV and the merged cross-attention query
        projection of every block plus their fp32 column vectors (fc1's FiLM-folded copy depends on the timestep and is rebuilt
        inside every denoiser evaluation).  Shapes that do not qualify (fp32, d_model not a multiple of 256) keep fold = NULL."""
        need = lib().d3pm_fold_bytes(C.byref(shape))
        if need == 0:
            return False
        self.fold_storage = torch.empty(need, dtype=torch.uint8, device=device)
        self.fold_blocks = (FoldBlock * shape.n_layers)()
        check(lib().d3pm_fold_build(C.byref(shape), C.byref(self.c_struct), _p(self.fold_storage), need, self.fold_blocks,
                                    stream_ptr()), "d3pm_fold_build")
        self.c_struct.fold = self.fold_blocks
        return True


class Fp8BlockWeights(C.Structure):
    _fields_ = [("attn_in_w8", C.c_void_p), ("attn_in_scale", C.c_void_p), ("cross_in_w8", C.c_void_p),
                ("cross_in_scale", C.c_void_p), ("fc1_w8", C.c_void_p), ("fc1_scale", C.c_void_p),
                ("fc2_w8", C.c_void_p), ("fc2_scale", C.c_void_p)]


class DeviceFp8Weights:
    """Block-scaled e4m3 copies (quantize_mx) of the LayerNorm-fed projections -- and of fc2 unless `fc2=False` -- of every
    block for the fp8 fast path."""

    def __init__(self, tensors: dict, n_layers: int, d_model: int, fc2: bool = True):
        self._keep = []
        self.blocks = (Fp8BlockWeights * n_layers)()
        which = [("attn_in", "attn.in_proj_weight", None), ("cross_in", "cross_attn.in_proj_weight", d_model), ("fc1", "mlp.fc1.weight", None)]
        if fc2:
            which.append(("fc2", "mlp.fc2.weight", None))
        for i in range(n_layers):
            for field, key, rows in which:
                w = tensors[f"blocks.{i}.{key}"]
                codes, scale = quantize_mx(w[:rows] if rows else w)
                self._keep += [codes, scale]
                setattr(self.blocks[i], field + "_w8", codes.data_ptr())
                setattr(self.blocks[i], field + "_scale", scale.data_ptr())


class DeviceCondWeights:
    """Pointer tables of the two condition encoders (+ embeddings and position tables)."""

    def __init__(self, tensors: dict, cfg, pe_text0: torch.Tensor, pe_prompt: torch.Tensor):
        self._keep = [pe_text0, pe_prompt]

        def ptr(key):
            t = tensors[key]
            if not (t.is_cuda and t.is_contiguous()):
                raise D3PMError(f"weight {key} must be a contiguous device tensor")
            self._keep.append(t)
            return t.data_ptr()

        names = {"in_w": "self_attn.in_proj_weight", "in_b": "self_attn.in_proj_bias", "out_w": "self_attn.out_proj.weight",
                 "out_b": "self_attn.out_proj.bias", "lin1_w": "linear1.weight", "lin1_b": "linear1.bias",
                 "lin2_w": "linear2.weight", "lin2_b": "linear2.bias", "norm1_w": "norm1.weight", "norm1_b": "norm1.bias",
                 "norm2_w": "norm2.weight", "norm2_b": "norm2.bias"}

        def encoder(name, mult):
            layers = (EncoderLayerWeights * cfg.cond_layers)()
            for j in range(cfg.cond_layers):
                for field, key in names.items():
                    setattr(layers[j], field, ptr(f"{name}.0.layers.{j}.{key}"))
            self._keep.append(layers)
            return EncoderWeights(layers, cfg.cond_layers, cfg.cond_heads, cfg.cond_ff, mult * cfg.d_model,
                                  ptr(f"{name}.1.fc1.weight"), ptr(f"{name}.1.fc1.bias"), ptr(f"{name}.1.fc2.weight"),
                                  ptr(f"{name}.1.fc2.bias"))

        self.c_struct = CondWeights(ptr("text_emb.weight"), ptr("proms_emb.weight"), pe_text0.data_ptr(),
                                    pe_prompt.data_ptr(), cfg.n_levels, encoder("encodertext", 2), encoder("encoder2", 3))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _require(t, name, shape, dtypes, device):
    """The C ABI takes raw pointers and derives every extent from the shape struct: a tensor of another shape, dtype,
    layout or device would be read / written out of bounds without any error, so it is rejected here."""
    if not isinstance(t, torch.Tensor):
        raise D3PMError(f"{name}: expected a tensor, got {type(t).__name__}")
    if tuple(t.shape) != tuple(shape):
        raise D3PMError(f"{name}: shape {tuple(t.shape)} != expected {tuple(shape)}")
    if t.dtype not in dtypes:
        raise D3PMError(f"{name}: dtype {t.dtype} not in {tuple(dtypes)}")
    if t.device != device:
        raise D3PMError(f"{name}: on {t.device}, the sampler lives on {device}")
    if not t.is_contiguous():
        raise D3PMError(f"{name}: must be contiguous")


class Sampler:
    """Thin object API over the C entry points for one (shape, weights) pair."""

    def __init__(self, cfg, tensors: dict, dtype: torch.dtype, device, pe_text0=None, pe_prompt=None):
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.shape = make_shape(cfg, dtype)
        self.n_q = max(1, getattr(cfg, "n_q", 1))       # quantizer levels generated jointly (> 1: this build's extension)
        self.weights = DeviceWeights(tensors, cfg.n_layers)
        self._tensors, self._fp8 = tensors, None
        # fp8 fast path: also run fc2 on MX operands (fc1's GELU epilogue then writes the hidden layer in that format).  On: measured
        # on MI355X (profiles/round3_h_ab_mx_fp8_gemm.txt) fc1 + fc2 take 52.5 + 38.1 us per block against 60.1 + 45.0 us with a
        # 16-bit hidden layer and 65.8 + 45.0 us in bf16; the logits error vs the bf16 path grows from 3.1 % to 3.7 %, the
        # teacher-forced id agreement stays at 0.9993 (tests/test_gpu_parity.py); False keeps fc2 a 16-bit GEMM
        self.fp8_fc2 = True
        self.cond_weights = (DeviceCondWeights(tensors, cfg, pe_text0, pe_prompt)
                             if pe_text0 is not None and "encodertext.1.fc1.weight" in tensors else None)
        self._cond_ws = None
        self.schedule = Schedule(cfg.timesteps)
        self._ws = {}
        self._graphs = {}
        self.film = torch.empty((cfg.timesteps + 1, cfg.n_layers, 2 * cfg.d_model), dtype=dtype, device=self.device)
        check(lib().d3pm_film_table(C.byref(self.shape), C.byref(self.weights.c_struct), _p(self.film), stream_ptr()),
              "d3pm_film_table")
        # LayerNorm folded into the projections (include/d3pm_hip.h: d3pm_fold_block; tuning field ln_fold picks it per call)
        self.folded = self.weights.build_fold(self.shape, self.device)

    def fp8_weights(self) -> DeviceFp8Weights:
        """e4m3 weight copies for the fp8 fast path, quantised on first use."""
        if self._fp8 is None:
            if self.cfg.d_model != 512 or self.dtype == torch.float32:
                raise D3PMError("the fp8 fast path needs d_model = 512 and a 16-bit model dtype")
            self._fp8 = DeviceFp8Weights(self._tensors, self.cfg.n_layers, self.cfg.d_model, fc2=self.fp8_fc2)
        return self._fp8

    def workspace(self, batch: int, slot: int = 0) -> torch.Tensor:
        """Scratch for one in-flight call; `slot` separates calls that run concurrently on different streams."""
        need = lib().d3pm_workspace_bytes(C.byref(self.shape), batch)
        if need == 0:
            raise D3PMError("d3pm_workspace_bytes: " + lib().d3pm_last_error().decode())
        ws = self._ws.get(slot)
        if ws is None or ws.numel() < need:
            ws = self._ws[slot] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def encode_conditions(self, text: torch.Tensor, prompt: torch.Tensor, text_len=None, prom_len=None):
        """text int32 [B,S_t] (zero padded), prompt int32 [B,S_p,n_levels] (-1 = level absent) ->
        (cond_text [B,S_t,d], cond_prompt [B,S_p,d]) through d3pm_encode_conditions.  text_len / prom_len: int32 [B] on the device
        or None -- the valid rows of each utterance, the only keys of that encoder's self-attention (d3pm_encode_conditions_keys);
        the ids behind a length are not read by the library (those rows are embedded as padding), so they may hold anything."""
        if self.cond_weights is None:
            raise D3PMError("this sampler was bound without condition-encoder weights")
        cfg, B = self.cfg, text.shape[0]
        assert text.shape == (B, cfg.s_text) and prompt.shape == (B, cfg.s_prompt, cfg.n_levels)
        ks = make_keys((None, text_len, prom_len), B, self.device) if (text_len is not None or prom_len is not None) else None
        text, prompt = text.to(torch.int32).contiguous(), prompt.to(torch.int32).contiguous()
        need = lib().d3pm_cond_workspace_bytes(C.byref(self.shape), C.byref(self.cond_weights.c_struct), B)
        if self._cond_ws is None or self._cond_ws.numel() < need:
            self._cond_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        ct = torch.empty((B, cfg.s_text, cfg.d_model), dtype=self.dtype, device=self.device)
        cp = torch.empty((B, cfg.s_prompt, cfg.d_model), dtype=self.dtype, device=self.device)
        if ks is not None:
            check(lib().d3pm_encode_conditions_keys(C.byref(self.shape), C.byref(self.cond_weights.c_struct), B, _p(text),
                                                    _p(prompt), _p(ct), _p(cp), _p(self._cond_ws), self._cond_ws.numel(),
                                                    C.byref(ks), stream_ptr()), "d3pm_encode_conditions_keys")
            return ct, cp
        check(lib().d3pm_encode_conditions(C.byref(self.shape), C.byref(self.cond_weights.c_struct), B, _p(text),
                                           _p(prompt), _p(ct), _p(cp), _p(self._cond_ws), self._cond_ws.numel(),
                                           stream_ptr()), "d3pm_encode_conditions")
        return ct, cp

    def cond_kv(self, cond_text: torch.Tensor, cond_prompt: torch.Tensor):
        """cond_text [B,S_t,d], cond_prompt [B,S_p,d] -> per-layer K|V tensors [L,B,S,2d]."""
        cfg, B = self.cfg, cond_text.shape[0]
        assert cond_text.shape == (B, cfg.s_text, cfg.d_model) and cond_prompt.shape == (B, cfg.s_prompt, cfg.d_model)
        cond_text, cond_prompt = cond_text.to(self.dtype).contiguous(), cond_prompt.to(self.dtype).contiguous()
        kv_t = torch.empty((cfg.n_layers, B, cfg.s_text, 2 * cfg.d_model), dtype=self.dtype, device=self.device)
        kv_p = torch.empty((cfg.n_layers, B, cfg.s_prompt, 2 * cfg.d_model), dtype=self.dtype, device=self.device)
        check(lib().d3pm_cond_kv(C.byref(self.shape), C.byref(self.weights.c_struct), B, _p(cond_text),
                                 _p(cond_prompt), _p(kv_t), _p(kv_p), stream_ptr()), "d3pm_cond_kv")
        return kv_t, kv_p

    def _check_grid(self, x, frame_mask=None, name="x_t"):
        cfg = self.cfg
        tail = (cfg.canvas,) if self.n_q == 1 else (cfg.canvas, self.n_q)
        if not isinstance(x, torch.Tensor) or x.dim() != 1 + len(tail):
            raise D3PMError(f"{name}: expected an int32 [B, {', '.join(map(str, tail))}] token grid")
        _require(x, name, (x.shape[0],) + tail, (torch.int32,), self.device)
        if x.shape[0] < 1:
            raise D3PMError(f"{name}: empty batch")
        if frame_mask is not None:
            _require(frame_mask, "frame_mask", (cfg.canvas,), (torch.uint8,), self.device)
        return x.shape[0]

    def _check_canvas(self, B, frame_mask, known=None):
        """The per-utterance calls: frame_mask uint8 [B, canvas] (a shared [canvas] mask is repeated per utterance) and the
        known-frame map, uint8 [B, canvas] or None -> the d3pm_canvas struct (keeps its tensors alive)."""
        cfg = self.cfg
        if isinstance(frame_mask, torch.Tensor) and frame_mask.dim() == 1:
            _require(frame_mask, "frame_mask", (cfg.canvas,), (torch.uint8,), self.device)
            frame_mask = frame_mask[None].expand(B, cfg.canvas).contiguous()
        _require(frame_mask, "frame_mask", (B, cfg.canvas), (torch.uint8,), self.device)
        if known is not None:
            _require(known, "known", (B, cfg.canvas), (torch.uint8,), self.device)
        cv = Canvas(frame_mask.data_ptr(), None if known is None else known.data_ptr())
        cv._keep = (frame_mask, known)
        return cv

    def _check_kv(self, kv_t, kv_p, B):
        cfg = self.cfg
        _require(kv_t, "kv_text", (cfg.n_layers, B, cfg.s_text, 2 * cfg.d_model), (self.dtype,), self.device)
        _require(kv_p, "kv_prompt", (cfg.n_layers, B, cfg.s_prompt, 2 * cfg.d_model), (self.dtype,), self.device)

    def denoise(self, x_t, frame_mask, t, kv_t, kv_p, *, want_logits=True, want_hidden=False, only_layers=-1,
                flags=0, fp8=False):
        cfg = self.cfg
        B = self._check_grid(x_t, frame_mask)
        self._check_kv(kv_t, kv_p, B)
        ws = self.workspace(B)
        logits = torch.empty((B, cfg.canvas) + self._lvl() + (cfg.n_classes,), dtype=self.dtype, device=self.device) if want_logits else None
        hidden = torch.empty((B, cfg.canvas, cfg.d_model), dtype=self.dtype, device=self.device) if want_hidden else None
        if fp8:
            check(lib().d3pm_denoise_step_fp8(C.byref(self.shape), C.byref(self.weights.c_struct),
                                              C.cast(self.fp8_weights().blocks, C.c_void_p), B, _p(x_t), _p(frame_mask), int(t),
                                              _p(self.film), _p(kv_t), _p(kv_p), _p(ws), ws.numel(), _p(logits), _p(hidden),
                                              only_layers, flags, stream_ptr()), "d3pm_denoise_step_fp8")
            return logits, hidden
        check(lib().d3pm_denoise_step(C.byref(self.shape), C.byref(self.weights.c_struct), B, _p(x_t), _p(frame_mask),
                                      int(t), _p(self.film), _p(kv_t), _p(kv_p), _p(ws), ws.numel(), _p(logits),
                                      _p(hidden), only_layers, flags, stream_ptr()), "d3pm_denoise_step")
        return logits, hidden

    def denoise_canvas(self, x_t, frame_mask, t, kv_t, kv_p, *, want_logits=True, want_hidden=False, only_layers=-1, flags=0, keys=None):
        """`denoise` with one frame mask per utterance, uint8 [B, canvas] (d3pm_denoise_step_canvas).  keys: None or the (frames,
        text, prompt) key counts of make_keys (d3pm_denoise_step_keys)."""
        cfg = self.cfg
        B = self._check_grid(x_t)
        cv = self._check_canvas(B, frame_mask)
        self._check_kv(kv_t, kv_p, B)
        ks = make_keys(keys, B, self.device)
        ws = self.workspace(B)
        logits = torch.empty((B, cfg.canvas) + self._lvl() + (cfg.n_classes,), dtype=self.dtype, device=self.device) if want_logits else None
        hidden = torch.empty((B, cfg.canvas, cfg.d_model), dtype=self.dtype, device=self.device) if want_hidden else None
        if ks is not None:
            check(lib().d3pm_denoise_step_keys(C.byref(self.shape), C.byref(self.weights.c_struct), B, _p(x_t), C.byref(cv),
                                               int(t), _p(self.film), _p(kv_t), _p(kv_p), _p(ws), ws.numel(), _p(logits),
                                               _p(hidden), only_layers, flags, C.byref(ks), stream_ptr()), "d3pm_denoise_step_keys")
            return logits, hidden
        check(lib().d3pm_denoise_step_canvas(C.byref(self.shape), C.byref(self.weights.c_struct), B, _p(x_t), C.byref(cv),
                                             int(t), _p(self.film), _p(kv_t), _p(kv_p), _p(ws), ws.numel(), _p(logits),
                                             _p(hidden), only_layers, flags, stream_ptr()), "d3pm_denoise_step_canvas")
        return logits, hidden

    def _lvl(self):
        return () if self.n_q == 1 else (self.n_q,)

    def posterior_sample(self, logits, x_t, t, seed, utt0=0, flags=0, want_posterior=False, known=None, temperature=1.0, top_k=0,
                         top_p=1.0, want_theta=False, guidance=0.0, null_logits=None):
        """known: uint8 [B, canvas] or None -- frames that keep x_t instead of being drawn (d3pm_posterior_sample_known).
        guidance (> 0) with null_logits (the logits of the same rows under the null condition, shape and dtype of `logits`): the
        draw runs on rn16(fmaf(guidance, logits - null_logits, logits)) (d3pm_posterior_sample_guided; ids only: no posterior, no theta).
        temperature / top_k: d3pm_sampling (d3pm_posterior_sample_sampling); the neutral pair takes the entries without them.
        top_p: d3pm_nucleus (d3pm_posterior_sample_nucleus); 1 takes the entries without it.  want_theta: a third result, the nucleus
        threshold of every row as float32 in the shape of x_t (-inf where top_p is 1, NaN for a known frame)."""
        cfg = self.cfg
        smp = nucleus_options(temperature, top_k, top_p, cfg.n_classes)
        gd = guidance_options(guidance)
        if (gd is None) != (null_logits is None):
            raise ValueError("guidance and null_logits go together: a weight > 0 needs the null logits, and they need a weight")
        if gd is not None and (want_posterior or want_theta or self.n_q > 1):
            raise ValueError("the guided draw returns ids only (no posterior, no theta) and is defined for n_q = 1")
        B = self._check_grid(x_t)
        if known is not None:
            _require(known, "known", (B, cfg.canvas), (torch.uint8,), self.device)
        logits = logits.contiguous() if isinstance(logits, torch.Tensor) else logits
        _require(logits, "logits", (B, cfg.canvas) + self._lvl() + (cfg.n_classes,), tuple(_DTYPES), self.device)
        x_next = torch.empty_like(x_t)
        if gd is not None:
            _require(null_logits, "null_logits", tuple(logits.shape), (logits.dtype,), self.device)
            both = torch.cat([logits, null_logits.contiguous()], 0)      # [2B, canvas, K]: the null twins behind the conditioned rows
            cv = None
            if known is not None:
                cv = Canvas(None, known.data_ptr())
            nuc = self._as_nucleus(smp)
            check(lib().d3pm_posterior_sample_guided(C.byref(self.shape), B, _p(both), dtype_code(both.dtype), _p(x_t), _p(x_next),
                                                     None if cv is None else C.byref(cv), int(t), C.byref(self.schedule.c_struct), seed,
                                                     utt0, flags, None if nuc is None else C.byref(nuc), C.byref(gd), stream_ptr()),
                  "d3pm_posterior_sample_guided")
            return x_next, None
        post = torch.empty((B, cfg.canvas) + self._lvl() + (cfg.n_classes,), dtype=torch.int16, device=self.device) if want_posterior else None
        if want_theta or isinstance(smp, Nucleus):
            theta = torch.empty(x_t.shape, dtype=torch.float32, device=self.device) if want_theta else None
            nuc = smp if isinstance(smp, Nucleus) else None if smp is None else Nucleus(smp.temperature, smp.top_k, 1.0)
            check(lib().d3pm_posterior_sample_nucleus(C.byref(self.shape), B, _p(logits), dtype_code(logits.dtype), _p(x_t),
                                                      _p(x_next), _p(known), int(t), C.byref(self.schedule.c_struct), seed, utt0,
                                                      flags, _p(post), None if nuc is None else C.byref(nuc), _p(theta), stream_ptr()),
                  "d3pm_posterior_sample_nucleus")
            return (x_next, post, theta) if want_theta else (x_next, post)
        if smp is not None:
            check(lib().d3pm_posterior_sample_sampling(C.byref(self.shape), B, _p(logits), dtype_code(logits.dtype), _p(x_t),
                                                       _p(x_next), _p(known), int(t), C.byref(self.schedule.c_struct), seed, utt0,
                                                       flags, _p(post), C.byref(smp), stream_ptr()), "d3pm_posterior_sample_sampling")
            return x_next, post
        if known is not None:
            check(lib().d3pm_posterior_sample_known(C.byref(self.shape), B, _p(logits), dtype_code(logits.dtype), _p(x_t),
                                                    _p(x_next), _p(known), int(t), C.byref(self.schedule.c_struct), seed, utt0,
                                                    flags, _p(post), stream_ptr()), "d3pm_posterior_sample_known")
            return x_next, post
        check(lib().d3pm_posterior_sample(C.byref(self.shape), B, _p(logits), dtype_code(logits.dtype), _p(x_t),
                                          _p(x_next), int(t), C.byref(self.schedule.c_struct), seed, utt0, flags,
                                          _p(post), stream_ptr()), "d3pm_posterior_sample")
        return x_next, post

    def _check_scores(self, scores, B):
        """scores: a (logprob float32, step int32) pair of preallocated [B, canvas] tensors on the device -> the d3pm_frame_scores
        struct (keeps its tensors alive)."""
        if self.n_q != 1:
            raise ValueError("frame scores are defined for n_q = 1")
        if not isinstance(scores, (tuple, list)) or len(scores) != 2:
            raise D3PMError("scores must be a (logprob float32, step int32) pair of [B, canvas] device tensors")
        logprob, step = scores
        _require(logprob, "scores.logprob", (B, self.cfg.canvas), (torch.float32,), self.device)
        _require(step, "scores.step", (B, self.cfg.canvas), (torch.int32,), self.device)
        fs = FrameScores(logprob.data_ptr(), step.data_ptr())
        fs._keep = (logprob, step)
        return fs

    def new_scores(self, B):
        """A (logprob, step) pair for `scores=`: float32 / int32 [B, canvas] on the sampler's device (contents set by the library)."""
        return (torch.empty((B, self.cfg.canvas), dtype=torch.float32, device=self.device),
                torch.empty((B, self.cfg.canvas), dtype=torch.int32, device=self.device))

    def frame_scores_init(self, x, frame_mask, scores, known=None):
        """d3pm_frame_scores_init on the canvas x a loop is about to start from: step = 0 on the free masked rows, -1 elsewhere, logprob
        = 0.  frame_mask uint8 [canvas] or [B, canvas]; known uint8 [B, canvas] or None; scores as for sample_loop."""
        per_utt = known is not None or (isinstance(frame_mask, torch.Tensor) and frame_mask.dim() == 2)
        B = self._check_grid(x, None if per_utt else frame_mask, "x")
        cv = self._check_canvas(B, frame_mask, known) if per_utt else None
        fs = self._check_scores(scores, B)
        check(lib().d3pm_frame_scores_init(C.byref(self.shape), B, _p(x), None if per_utt else _p(frame_mask), C.byref(cv) if per_utt else None,
                                           C.byref(fs), stream_ptr()), "d3pm_frame_scores_init")

    def frame_scores_step(self, logits, x_next, t, scores, *, row_of=None, guidance=0.0, null_logits=None):
        """d3pm_frame_scores_step behind one sampler step: the rows of `scores` with step 0 whose x_next is no longer the mask id get the
        log-probability of that id under `logits` (the evaluation at t) and step = t.  logits [B, canvas, n_classes] (any of the three
        dtypes); guidance (> 0) with null_logits as for posterior_sample; row_of int32 [B * canvas] with logits [B * canvas,
        n_classes] (16-bit, a view with a wider row stride allowed): row r reads logits[row_of[r]], clamped into the rows."""
        cfg = self.cfg
        gd = guidance_options(guidance)
        if (gd is None) != (null_logits is None):
            raise ValueError("guidance and null_logits go together: a weight > 0 needs the null logits, and they need a weight")
        B = self._check_grid(x_next, None, "x_next")
        fs = self._check_scores(scores, B)
        rows = B * cfg.canvas
        if row_of is not None:
            if not isinstance(logits, torch.Tensor) or tuple(logits.shape) != (rows, cfg.n_classes) or logits.dtype not in _DTYPES or \
                    logits.device != self.device or logits.stride(1) != 1 or logits.stride(0) < cfg.n_classes:
                raise D3PMError(f"logits must be a [{rows}, {cfg.n_classes}] tensor on {self.device} with unit column stride")
            _require_int32([("row_of", row_of, (rows,))], self.device)
            ldl = logits.stride(0)
        else:
            logits = logits.contiguous() if isinstance(logits, torch.Tensor) else logits
            _require(logits, "logits", (B, cfg.canvas, cfg.n_classes), tuple(_DTYPES), self.device)
            ldl = cfg.n_classes
            if gd is not None:
                _require(null_logits, "null_logits", tuple(logits.shape), (logits.dtype,), self.device)
                logits = torch.cat([logits, null_logits.contiguous()], 0)      # [2B, canvas, K]: the null twins behind the conditioned rows
        check(lib().d3pm_frame_scores_step(C.byref(self.shape), B, _p(logits), dtype_code(logits.dtype), int(ldl), _p(row_of),
                                           None if gd is None else C.byref(gd), _p(x_next), int(t), C.byref(fs), stream_ptr()),
              "d3pm_frame_scores_step")

    def sample_loop(self, x, frame_mask, t_start, t_stop, kv_t, kv_p, seed, utt0=0, flags=0, trace=False, slot=0,
                    fp8=False, known=None, temperature=1.0, top_k=0, top_p=1.0, keys=None, guidance=0.0, scores=None):
        """frame_mask uint8 [canvas] (shared by the batch) runs d3pm_sample_loop(_fp8); a per-utterance mask [B, canvas] and / or a
        known-frame map `known` (uint8 [B, canvas]; `x` already carries the given ids) run the *_canvas entries.  temperature /
        top_k other than the neutral (1, 0) run d3pm_sample_loop_sampling, which covers the four of them; top_p other than 1 runs
        d3pm_sample_loop_nucleus, which takes the same arguments.  keys: None or the (frames, text, prompt) key counts of make_keys
        (d3pm_sample_loop_keys, which covers all of the above but fp8).  guidance > 0 (classifier-free guidance,
        d3pm_sample_loop_guided): kv_t / kv_p hold 2B utterances -- the null twins behind the conditioned ones -- and so do the three
        arrays of `keys`; x, frame_mask, known and the trace stay those of B utterances.  No fp8, no n_q > 1.
        scores: None (the branches above, untouched) or a (logprob float32, step int32) pair of preallocated [B, canvas] tensors
        (new_scores) that d3pm_sample_loop_scored fills with the per-frame log-probability of the revealed ids (n_q = 1; it covers
        every combination above)."""
        cfg = self.cfg
        smp = nucleus_options(temperature, top_k, top_p, cfg.n_classes)
        gd = guidance_options(guidance)
        if keys is not None and fp8:
            raise ValueError("the fp8 fast path takes no key mask")
        if gd is not None and (fp8 or self.n_q > 1):
            raise ValueError("guidance does not combine with " + ("fp8=True" if fp8 else "an n_q > 1 model"))
        per_utt = known is not None or (isinstance(frame_mask, torch.Tensor) and frame_mask.dim() == 2)
        B = self._check_grid(x, None if per_utt else frame_mask, "x")
        cv = self._check_canvas(B, frame_mask, known) if per_utt else None
        fs = None if scores is None else self._check_scores(scores, B)
        eval_B = B if gd is None else 2 * B
        self._check_kv(kv_t, kv_p, eval_B)
        ks = make_keys(keys, eval_B, self.device)
        ws = self.workspace(eval_B, slot)
        tr = torch.empty((t_start - t_stop, B, cfg.canvas) + self._lvl(), dtype=torch.int32, device=self.device) if trace else None
        if fs is not None:
            nuc = self._as_nucleus(smp)
            check(lib().d3pm_sample_loop_scored(C.byref(self.shape), C.byref(self.weights.c_struct),
                                                C.cast(self.fp8_weights().blocks, C.c_void_p) if fp8 else None, B, _p(x),
                                                None if per_utt else _p(frame_mask), C.byref(cv) if per_utt else None,
                                                int(t_start), int(t_stop), _p(self.film), _p(kv_t), _p(kv_p),
                                                C.byref(self.schedule.c_struct), seed, utt0, flags, _p(ws), ws.numel(), _p(tr),
                                                None if nuc is None else C.byref(nuc), None if ks is None else C.byref(ks),
                                                None if gd is None else C.byref(gd), C.byref(fs), stream_ptr()), "d3pm_sample_loop_scored")
            return tr
        if gd is not None:
            nuc = self._as_nucleus(smp)
            check(lib().d3pm_sample_loop_guided(C.byref(self.shape), C.byref(self.weights.c_struct), None, B, _p(x),
                                                None if per_utt else _p(frame_mask), C.byref(cv) if per_utt else None,
                                                int(t_start), int(t_stop), _p(self.film), _p(kv_t), _p(kv_p),
                                                C.byref(self.schedule.c_struct), seed, utt0, flags, _p(ws), ws.numel(), _p(tr),
                                                None if nuc is None else C.byref(nuc), None if ks is None else C.byref(ks), C.byref(gd),
                                                stream_ptr()), "d3pm_sample_loop_guided")
            return tr
        if ks is not None:
            nuc = self._as_nucleus(smp)
            check(lib().d3pm_sample_loop_keys(C.byref(self.shape), C.byref(self.weights.c_struct), None, B, _p(x),
                                              None if per_utt else _p(frame_mask), C.byref(cv) if per_utt else None,
                                              int(t_start), int(t_stop), _p(self.film), _p(kv_t), _p(kv_p),
                                              C.byref(self.schedule.c_struct), seed, utt0, flags, _p(ws), ws.numel(), _p(tr),
                                              None if nuc is None else C.byref(nuc), C.byref(ks), stream_ptr()), "d3pm_sample_loop_keys")
            return tr
        if smp is not None:
            name = "d3pm_sample_loop_nucleus" if isinstance(smp, Nucleus) else "d3pm_sample_loop_sampling"
            check(getattr(lib(), name)(C.byref(self.shape), C.byref(self.weights.c_struct),
                                       C.cast(self.fp8_weights().blocks, C.c_void_p) if fp8 else None, B, _p(x),
                                       None if per_utt else _p(frame_mask), C.byref(cv) if per_utt else None,
                                       int(t_start), int(t_stop), _p(self.film), _p(kv_t), _p(kv_p),
                                       C.byref(self.schedule.c_struct), seed, utt0, flags, _p(ws), ws.numel(), _p(tr),
                                       C.byref(smp), stream_ptr()), name)
            return tr
        if per_utt and fp8:
            check(lib().d3pm_sample_loop_fp8_canvas(C.byref(self.shape), C.byref(self.weights.c_struct),
                                                    C.cast(self.fp8_weights().blocks, C.c_void_p), B, _p(x), C.byref(cv),
                                                    int(t_start), int(t_stop), _p(self.film), _p(kv_t), _p(kv_p),
                                                    C.byref(self.schedule.c_struct), seed, utt0, flags, _p(ws), ws.numel(), _p(tr),
                                                    stream_ptr()), "d3pm_sample_loop_fp8_canvas")
            return tr
        if per_utt:
            check(lib().d3pm_sample_loop_canvas(C.byref(self.shape), C.byref(self.weights.c_struct), B, _p(x), C.byref(cv),
                                                int(t_start), int(t_stop), _p(self.film), _p(kv_t), _p(kv_p),
                                                C.byref(self.schedule.c_struct), seed, utt0, flags, _p(ws), ws.numel(), _p(tr),
                                                stream_ptr()), "d3pm_sample_loop_canvas")
            return tr
        if fp8:
            check(lib().d3pm_sample_loop_fp8(C.byref(self.shape), C.byref(self.weights.c_struct),
                                             C.cast(self.fp8_weights().blocks, C.c_void_p), B, _p(x), _p(frame_mask),
                                             int(t_start), int(t_stop), _p(self.film), _p(kv_t), _p(kv_p),
                                             C.byref(self.schedule.c_struct), seed, utt0, flags, _p(ws), ws.numel(), _p(tr),
                                             stream_ptr()), "d3pm_sample_loop_fp8")
            return tr
        check(lib().d3pm_sample_loop(C.byref(self.shape), C.byref(self.weights.c_struct), B, _p(x), _p(frame_mask),
                                     int(t_start), int(t_stop), _p(self.film), _p(kv_t), _p(kv_p),
                                     C.byref(self.schedule.c_struct), seed, utt0, flags, _p(ws), ws.numel(), _p(tr),
                                     stream_ptr()), "d3pm_sample_loop")
        return tr

    def reveal_plan(self, n_steps):
        """The timesteps t_0 .. t_{N-1} of the reveal schedule (d3pm_reveal_plan) as a list of ints."""
        rv = reveal_options(n_steps, 0.0, self.schedule.timesteps)
        out = (C.c_int32 * rv.n_steps)()
        check(lib().d3pm_reveal_plan(C.byref(self.schedule.c_struct), rv.n_steps, out), "d3pm_reveal_plan")
        return list(out)

    @staticmethod
    def _as_nucleus(smp):
        return smp if smp is None or isinstance(smp, Nucleus) else Nucleus(smp.temperature, smp.top_k, 1.0)

    def reveal_step(self, logits, x_t, frame_mask, t, t_next, seed, utt0=0, flags=0, known=None, temperature=1.0, top_k=0, top_p=1.0,
                    choice_temperature=0.0, x_next=None, revise=None, scores=None):
        """One step of the reveal schedule (d3pm_reveal_step) on the logits of the evaluation at `t`, followed by `t_next` (0 = the
        last step) -> (x_next, cand, score): cand int32 / score float32 [B, canvas] hold a value only where x_t was a masked free
        row (the other entries are 0).  frame_mask uint8 [canvas] or [B, canvas]; known uint8 [B, canvas] or None.  x_next: the grid
        to store into (x_t itself for an in-place step), default a new one.
        revise: None, or the hold bonus (a number >= 0) of d3pm_revise (d3pm_reveal_step_revise): the free rows that hold an id
        compete again, cand / score then hold a value on every free row, and x_next may receive the mask id.  scores (with revise
        only): the (logprob, step) pair whose entries the commit resets on the rows it re-masks."""
        cfg = self.cfg
        smp = self._as_nucleus(nucleus_options(temperature, top_k, top_p, cfg.n_classes))
        reveal_options(1, choice_temperature)
        rs = revise_options(revise)
        if scores is not None and rs is None:
            raise ValueError("reveal_step takes scores only with revise")
        per_utt = known is not None or (isinstance(frame_mask, torch.Tensor) and frame_mask.dim() == 2)
        B = self._check_grid(x_t, None if per_utt else frame_mask)
        cv = self._check_canvas(B, frame_mask, known) if per_utt else None
        logits = logits.contiguous() if isinstance(logits, torch.Tensor) else logits
        _require(logits, "logits", (B, cfg.canvas, cfg.n_classes), tuple(_DTYPES), self.device)
        if x_next is None:
            x_next = torch.empty_like(x_t)
        else:
            _require(x_next, "x_next", tuple(x_t.shape), (torch.int32,), self.device)
        cand = torch.zeros((B, cfg.canvas), dtype=torch.int32, device=self.device)
        score = torch.zeros((B, cfg.canvas), dtype=torch.float32, device=self.device)
        head = (C.byref(self.shape), B, _p(logits), dtype_code(logits.dtype), _p(x_t), _p(x_next), None if per_utt else _p(frame_mask),
                C.byref(cv) if per_utt else None, int(t), int(t_next), C.byref(self.schedule.c_struct), seed, utt0, flags,
                None if smp is None else C.byref(smp), float(choice_temperature), _p(cand), _p(score))
        if rs is not None:
            fs = None if scores is None else self._check_scores(scores, B)
            check(lib().d3pm_reveal_step_revise(*head, C.byref(rs), None if fs is None else C.byref(fs), stream_ptr()), "d3pm_reveal_step_revise")
        else:
            check(lib().d3pm_reveal_step(*head, stream_ptr()), "d3pm_reveal_step")
        return x_next, cand, score

    def reveal_loop(self, x, frame_mask, n_steps, kv_t, kv_p, seed, utt0=0, flags=0, trace=False, slot=0, known=None, temperature=1.0,
                    top_k=0, top_p=1.0, choice_temperature=0.0, keys=None, scores=None, revise=None):
        """The reveal schedule in n_steps denoiser evaluations (d3pm_reveal_loop), in place on x; masks and known frames as for
        sample_loop.  keys: None or the (frames, text, prompt) key counts of make_keys (d3pm_reveal_loop_keys).  scores: None or the
        (logprob, step) pair of sample_loop (d3pm_reveal_loop_scored).  revise: None or the hold
        bonus (a number >= 0) of d3pm_revise (d3pm_reveal_loop_revise, which covers keys and scores): every step may re-mask frames.
        -> the trace int32 [n_steps, B, canvas] (x after every step) or None."""
        cfg = self.cfg
        smp = self._as_nucleus(nucleus_options(temperature, top_k, top_p, cfg.n_classes))
        rv = reveal_options(n_steps, choice_temperature, self.schedule.timesteps)
        if rv is None:
            raise ValueError("reveal_loop needs n_steps")
        if self.n_q != 1:
            raise ValueError("the reveal schedule is defined for n_q = 1")
        per_utt = known is not None or (isinstance(frame_mask, torch.Tensor) and frame_mask.dim() == 2)
        B = self._check_grid(x, None if per_utt else frame_mask, "x")
        cv = self._check_canvas(B, frame_mask, known) if per_utt else None
        self._check_kv(kv_t, kv_p, B)
        ws = self.workspace(B, slot)
        fs = None if scores is None else self._check_scores(scores, B)
        tr = torch.empty((rv.n_steps, B, cfg.canvas), dtype=torch.int32, device=self.device) if trace else None
        ks = make_keys(keys, B, self.device)
        rs = revise_options(revise)
        head = (C.byref(self.shape), C.byref(self.weights.c_struct), B, _p(x), None if per_utt else _p(frame_mask), C.byref(cv) if per_utt else None,
                _p(self.film), _p(kv_t), _p(kv_p), C.byref(self.schedule.c_struct), seed, utt0, flags, _p(ws), ws.numel(), _p(tr),
                None if smp is None else C.byref(smp), C.byref(rv))
        kp, fp = None if ks is None else C.byref(ks), None if fs is None else C.byref(fs)
        if rs is not None:
            check(lib().d3pm_reveal_loop_revise(*head, kp, C.byref(rs), fp, stream_ptr()), "d3pm_reveal_loop_revise")
        elif fs is not None:
            check(lib().d3pm_reveal_loop_scored(*head, kp, fp, stream_ptr()), "d3pm_reveal_loop_scored")
        elif ks is not None:
            check(lib().d3pm_reveal_loop_keys(*head, kp, stream_ptr()), "d3pm_reveal_loop_keys")
        else:
            check(lib().d3pm_reveal_loop(*head, stream_ptr()), "d3pm_reveal_loop")
        return tr

    def ce_loss_rows(self, logits, targets, frame_mask):
        """fp32 [B, canvas] cross-entropy rows of masked logits against masked targets (d3pm_ce_loss_rows)."""
        B = self._check_grid(targets, frame_mask, "targets")
        logits = logits.contiguous() if isinstance(logits, torch.Tensor) else logits
        _require(logits, "logits", (B, self.cfg.canvas, self.cfg.n_classes), tuple(_DTYPES), self.device)
        out = torch.empty((B, self.cfg.canvas), dtype=torch.float32, device=self.device)
        check(lib().d3pm_ce_loss_rows(C.byref(self.shape), B, _p(logits), dtype_code(logits.dtype), _p(targets),
                                      _p(frame_mask), _p(out), stream_ptr()), "d3pm_ce_loss_rows")
        return out

    def training_forward(self, x0, frame_mask, kv_t, kv_p, seed, utt0=0, timesteps=None, keys=None):
        """The training-side forward of AR.forward (ar_discrete.py:655-693) for utterances that share one frame mask:
        sum over t = 1 .. timesteps-1 of mean_rows CE(denoiser(q_sample(x0, t)), x0 * mask), divided by mask.sum().
        keys: None or the (frames, text, prompt) key counts of make_keys -- every evaluation then runs through d3pm_denoise_step_keys.
        Returns (loss fp32 [B], logits of the last step [B, canvas, K] with padded frames zeroed)."""
        T = self.schedule.timesteps if timesteps is None else int(timesteps)
        fm = frame_mask.to(torch.uint8)
        live = fm.bool()
        targets = (x0 * fm.to(x0.dtype)[None, :]).to(torch.int32).contiguous()
        total = torch.zeros(x0.shape[0], dtype=torch.float32, device=self.device)
        logits = None
        for t in range(1, T):
            x_t = self.q_sample(x0, fm, t, seed, utt0)
            if keys is None:
                logits, _ = self.denoise(x_t, fm, t, kv_t, kv_p)
            else:
                logits, _ = self.denoise_canvas(x_t, fm, t, kv_t, kv_p, keys=keys)
            total += self.ce_loss_rows(logits, targets, fm).mean(dim=1)
        if logits is not None:
            logits = logits * live[None, :, None].to(logits.dtype)
        return total / live.sum().to(torch.float32), logits

    def sample_loop_graphed(self, x, frame_mask, t_start, t_stop, kv_t, kv_p, seed, utt0=0, flags=0):
        """The same loop replayed from a captured HIP graph: one launch instead of ~50 per iteration, for the
        launch-bound regime (one or two utterances).  The graph is captured once per (batch, step range, utt0,
        flags) over static buffers; the seed lives in HBM (D3PM_FLAG_SEED_IN_HBM) so that a replay can draw new
        noise.  `x` is updated in place like sample_loop does."""
        B = x.shape[0]
        key = (B, int(t_start), int(t_stop), int(utt0), int(flags))
        ent = self._graphs.get(key)
        if ent is None:
            st = {"x": torch.empty_like(x), "mask": torch.empty_like(frame_mask), "kv_t": torch.empty_like(kv_t),
                  "kv_p": torch.empty_like(kv_p), "seed": torch.zeros(1, dtype=torch.int64, device=self.device)}
            for k, v in (("x", x), ("mask", frame_mask), ("kv_t", kv_t), ("kv_p", kv_p)):
                st[k].copy_(v)
            fl = int(flags) | FLAG_SEED_IN_HBM
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):          # eager warm-up on the capture stream: lazy module load, func attributes
                self.sample_loop(st["x"], st["mask"], t_start, max(t_start - 1, t_stop), st["kv_t"], st["kv_p"],
                                 st["seed"].data_ptr(), utt0=utt0, flags=fl, slot=("graph",) + key)
            torch.cuda.current_stream(self.device).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self.sample_loop(st["x"], st["mask"], t_start, t_stop, st["kv_t"], st["kv_p"], st["seed"].data_ptr(),
                                 utt0=utt0, flags=fl, slot=("graph",) + key)
            ent = self._graphs[key] = (graph, st)
        graph, st = ent
        st["x"].copy_(x)
        st["mask"].copy_(frame_mask)
        st["kv_t"].copy_(kv_t)
        st["kv_p"].copy_(kv_p)
        st["seed"].fill_(int(seed))
        graph.replay()
        x.copy_(st["x"])

    def q_sample(self, x0, frame_mask, t, seed, utt0=0):
        self._check_grid(x0, frame_mask, "x0")
        out = torch.empty_like(x0)
        check(lib().d3pm_q_sample(C.byref(self.shape), x0.shape[0], _p(x0), _p(out), _p(frame_mask), int(t),
                                  C.byref(self.schedule.c_struct), seed, utt0, stream_ptr()), "d3pm_q_sample")
        return out


FAMILY_AUTO, FAMILY_GENERIC, FAMILY_MFMA = 0, 1, 2


def op_linear(x, w, bias=None, *, act=0, r1=None, r2=None, row_mask=None, mask_period=1, family=0, out=None,
              ldy=None):
    """y = epilogue(x @ w.T + bias) through d3pm_op_linear; x [M,K], w [N,K] contiguous device tensors."""
    M, K = x.shape
    N = w.shape[0]
    ldy = N if ldy is None else ldy
    y = torch.zeros((M, ldy), dtype=x.dtype, device=x.device) if out is None else out
    check(lib().d3pm_op_linear(dtype_code(x.dtype), family, _p(x), x.stride(0), _p(w), _p(bias), _p(y), ldy, _p(r1),
                               _p(r2), 0 if r1 is None else r1.stride(0), _p(row_mask), mask_period, M, N, K, act,
                               C.byref(TUNING), stream_ptr()), "d3pm_op_linear")
    return y[:, :N]


def mx_scale_bytes(amax: torch.Tensor) -> torch.Tensor:
    """e8m0 byte of a block's absolute maximum (csrc/d3pm_mx.hip: mx_scale_byte): the smallest power of two 2^(byte - 127)
    with amax / scale <= 448, exact integer arithmetic on the fp32 bits."""
    bits = amax.float().contiguous().view(torch.int32)
    e = (bits >> 23) - 8 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)
    return e.clamp(1, 254).to(torch.uint8)


def quantize_mx(w: torch.Tensor):
    """[N, K] (K a multiple of 128) -> (uint8 e4m3 codes [N, K], uint8 e8m0 scales [N, 4, K // 128]); blocks of 32 along K.
    The weight side of the fp8 path (host / torch arithmetic; torch's float8_e4m3fn is the OCP format gfx950 computes in); the
    device-side quantisers (d3pm_op_quantize_mx, d3pm_op_layernorm_mx, the MX epilogue) apply the same rule."""
    N, K = w.shape
    assert K % 128 == 0
    wf = w.float().reshape(N, K // 128, 4, 32)
    sb = mx_scale_bytes(wf.abs().amax(dim=-1))                       # [N, K/128, 4]
    inv = torch.exp2(127.0 - sb.float())
    codes = (wf * inv[..., None]).to(torch.float8_e4m3fn).view(torch.uint8).reshape(N, K)
    return codes.contiguous(), sb.permute(0, 2, 1).contiguous()


def dequantize_mx(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 values of an MX tensor (codes [N, K], scales [N, 4, K // 128]): exact."""
    N, K = codes.shape
    sc = torch.exp2(scales.permute(0, 2, 1).float() - 127.0)        # [N, K/128, 4]
    return (codes.view(torch.float8_e4m3fn).float().reshape(N, K // 128, 4, 32) * sc[..., None]).reshape(N, K)


def _mx_pair(M, K, device, out):
    """(codes [M, K], scales [M, 4, K // 128]): `out` where the caller brings the pair (contiguous uint8 of those shapes), else new."""
    if out is None:
        return (torch.empty((M, K), dtype=torch.uint8, device=device), torch.empty((M, 4, K // 128), dtype=torch.uint8, device=device))
    c, s = out
    assert c.dtype == s.dtype == torch.uint8 and c.shape == (M, K) and s.shape == (M, 4, K // 128) and c.is_contiguous() and s.is_contiguous()
    return c, s


def op_quantize_mx(x, *, out=None):
    """x [M, K] (row stride x.stride(0)) -> (codes, scales); out = (codes, scales) to write into."""
    M, K = x.shape
    x8, sx = _mx_pair(M, K, x.device, out)
    check(lib().d3pm_op_quantize_mx(dtype_code(x.dtype), _p(x), x.stride(0), _p(x8), _p(sx), M, K, stream_ptr()), "d3pm_op_quantize_mx")
    return x8, sx


def op_layernorm_mx(x, w, b, film=None, eps=1e-6, *, out=None):
    M, d = x.shape
    y8, sx = _mx_pair(M, d, x.device, out)
    check(lib().d3pm_op_layernorm_mx(dtype_code(x.dtype), _p(x), _p(y8), _p(sx), _p(w), _p(b), _p(film), M, d, eps,
                                     stream_ptr()), "d3pm_op_layernorm_mx")
    return y8, sx


def op_layernorm_mx_pair(x, w, b, w2, b2, film=None, eps=1e-6, *, out=None, out2=None):
    """Two LayerNorms of the same rows in one launch (the sampler's norm2 | norm22): ((codes, scales), (codes_2, scales_2));
    FiLM applies to the first."""
    M, d = x.shape
    y8, sx = _mx_pair(M, d, x.device, out)
    y8_2, sx_2 = _mx_pair(M, d, x.device, out2)
    check(lib().d3pm_op_layernorm_mx_pair(dtype_code(x.dtype), _p(x), _p(y8), _p(sx), _p(w), _p(b), _p(film), _p(w2), _p(b2), _p(y8_2),
                                          _p(sx_2), M, d, eps, stream_ptr()), "d3pm_op_layernorm_mx_pair")
    return (y8, sx), (y8_2, sx_2)


def op_linear_mx(x8, sx, w8, sw, bias, out_dtype, *, act=0, r1=None, row_mask=None, mask_period=1, mx_out=False, out=None, ldy=None,
                 out8=None, out_scales=None):
    """16-bit result [M, N], or with mx_out=True the result as (codes [M, N], scales [M, 4, N // 128]).  out / ldy: the 16-bit
    result goes to `out` with row stride ldy; out8 / out_scales: the MX result goes there (either one implies mx_out; the library
    refuses one without the other)."""
    M, K = x8.shape
    N = w8.shape[0]
    mx_out = mx_out or out8 is not None or out_scales is not None
    if mx_out:
        given = out8 is not None or out_scales is not None
        y8 = out8 if given else torch.empty((M, N), dtype=torch.uint8, device=x8.device)
        sy = out_scales if given else torch.empty((M, 4, N // 128), dtype=torch.uint8, device=x8.device)
        y = out
        ldy = N if ldy is None else ldy
    else:
        y8 = sy = None
        ldy = N if ldy is None else ldy
        y = torch.empty((M, ldy), dtype=out_dtype, device=x8.device) if out is None else out
    check(lib().d3pm_op_linear_mx(dtype_code(out_dtype), _p(x8), x8.stride(0), _p(sx), _p(w8), _p(sw), _p(bias), _p(y), ldy, _p(r1),
                                  0 if r1 is None else r1.stride(0), _p(row_mask), mask_period, _p(y8), _p(sy), M, N, K, act,
                                  C.byref(TUNING), stream_ptr()), "d3pm_op_linear_mx")
    return (y8, sy) if mx_out else y[:, :N]


def op_attention(q, k, v, n_heads, scale, *, family=0, key_len=None):
    """q [B,Tq,d], k/v [B,S,d] (views with arbitrary row stride allowed) -> [B,Tq,d].  key_len: int32 [B] on the device, the valid
    keys of each utterance (1 .. S, the caller's contract: the library cannot check device values); keys behind them are masked."""
    B, Tq, d = q.shape
    S = k.shape[1]
    assert k.stride(1) == v.stride(1) and q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    assert q.stride(0) == Tq * q.stride(1) and k.stride(0) == S * k.stride(1) and v.stride(0) == S * v.stride(1)
    o = torch.empty((B, Tq, d), dtype=q.dtype, device=q.device)
    if key_len is None:
        check(lib().d3pm_op_attention(dtype_code(q.dtype), family, _p(q), q.stride(1), _p(k), _p(v), k.stride(1), _p(o), d,
                                      B, Tq, S, n_heads, d // n_heads, float(scale), C.byref(TUNING), stream_ptr()),
              "d3pm_op_attention")
        return o
    if key_len.dtype != torch.int32 or key_len.shape != (B,) or key_len.device != q.device or not key_len.is_contiguous():
        raise D3PMError(f"key_len must be a contiguous int32 [{B}] tensor on {q.device}")
    check(lib().d3pm_op_attention_keylen(dtype_code(q.dtype), family, _p(q), q.stride(1), _p(k), _p(v), k.stride(1), _p(o), d,
                                         B, Tq, S, n_heads, d // n_heads, float(scale), _p(key_len), C.byref(TUNING), stream_ptr()),
          "d3pm_op_attention_keylen")
    return o


def op_attention_gather(q, k, v, key_row, seg_start, seg_len, n_heads, scale, out, *, key_len=None):
    """The self-attention of the deduplicated loop (d3pm_op_attention_gather): q / out [rows, d], where utterance b owns the seg_len[b]
    rows (any count from 1 up to the capacity) from row seg_start[b] (any row); k / v [kv_rows, d], views of one packed pool that share a row stride; key j of
    utterance b is row key_row[b, j] of them (int32 [B, S], clamped into the pool by the kernel).  Writes `out` in place (rows no segment
    owns keep what they hold) and returns it.  The query capacity per utterance handed to the launch is rows rounded down to 128."""
    rows, d = q.shape
    B, S = key_row.shape
    dev = q.device
    if k.shape != v.shape or k.shape[1] != d or out.shape != q.shape or out.dtype != q.dtype or k.dtype != q.dtype or v.dtype != q.dtype:
        raise D3PMError("op_attention_gather: q / out [rows, d] and k / v [kv_rows, d] of one dtype")
    if k.stride(0) != v.stride(0) or any(t.stride(1) != 1 for t in (q, k, v, out)) or any(t.device != dev for t in (k, v, out, key_row)):
        raise D3PMError("op_attention_gather: k and v share a row stride; unit column strides; one device")
    ints = [("key_row", key_row, (B, S)), ("seg_start", seg_start, (B,)), ("seg_len", seg_len, (B,))]
    if key_len is not None:
        ints.append(("key_len", key_len, (B,)))
    for name, t, shape in ints:
        if t.dtype != torch.int32 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise D3PMError(f"{name} must be a contiguous int32 {list(shape)} tensor on {dev}")
    check(lib().d3pm_op_attention_gather(dtype_code(q.dtype), _p(q), q.stride(0), _p(k), _p(v), k.stride(0), k.shape[0], _p(key_row),
                                         _p(seg_start), _p(seg_len), _p(out), out.stride(0), B, rows // 128 * 128, S, n_heads, d // n_heads,
                                         float(scale), _p(key_len), C.byref(TUNING), stream_ptr()), "d3pm_op_attention_gather")
    return out


def op_attention_gather_pool(q, k, v, key_row, seg_key, seg_start, seg_len, n_heads, scale, out, *, pool_rows, qblocks_grid, pool_src=None,
                             key_len=None):
    """op_attention_gather with an utterance's distinct k | v rows pooled in LDS (d3pm_op_attention_gather_pool): seg_key int32 [B, S] names
    key j of utterance b as row seg_key[b, j] - seg_start[b] of its pool (clamped into the segment), pool row r being row
    pool_src[seg_start[b] + r] of k / v (int32 [any]; None: row seg_start[b] + r), clamped into them.  An utterance with more than
    pool_rows rows walks key_row instead.  The caller promises that both name rows with the same bytes.  qblocks_grid: 128-query blocks
    per (utterance, head) in the grid."""
    rows, d = q.shape
    B, S = key_row.shape
    dev = q.device
    if k.shape != v.shape or k.shape[1] != d or out.shape != q.shape or out.dtype != q.dtype or k.dtype != q.dtype or v.dtype != q.dtype:
        raise D3PMError("op_attention_gather_pool: q / out [rows, d] and k / v [kv_rows, d] of one dtype")
    if k.stride(0) != v.stride(0) or any(t.stride(1) != 1 for t in (q, k, v, out)) or any(t.device != dev for t in (k, v, out, key_row)):
        raise D3PMError("op_attention_gather_pool: k and v share a row stride; unit column strides; one device")
    ints = [("key_row", key_row, (B, S)), ("seg_key", seg_key, (B, S)), ("seg_start", seg_start, (B,)), ("seg_len", seg_len, (B,))]
    if key_len is not None:
        ints.append(("key_len", key_len, (B,)))
    if pool_src is not None:
        ints.append(("pool_src", pool_src, tuple(pool_src.shape[:1])))
    for name, t, shape in ints:
        if t.dtype != torch.int32 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise D3PMError(f"{name} must be a contiguous int32 {list(shape)} tensor on {dev}")
    check(lib().d3pm_op_attention_gather_pool(dtype_code(q.dtype), _p(q), q.stride(0), _p(k), _p(v), k.stride(0), k.shape[0], _p(key_row),
                                              _p(seg_start), _p(seg_len), _p(out), out.stride(0), B, rows // 128 * 128, S, n_heads, d // n_heads,
                                              float(scale), _p(key_len), _p(seg_key), _p(pool_src), int(pool_rows), int(qblocks_grid),
                                              C.byref(TUNING), stream_ptr()), "d3pm_op_attention_gather_pool")
    return out


def op_attention_pair(q1, k1, v1, q2, k2, v2, n_heads, scale, *, key_len=None, key_len2=None):
    """The text / prompt cross-attention pair of a block as one launch: q1, q2 [B,Tq,d]; k1 / v1 [B,S1,d], k2 / v2 [B,S2,d] (K / V
    views of one packed [.., 2d] cache row allowed) -> (o1, o2) [B,Tq,d].  key_len / key_len2: int32 [B] on the device, the valid
    keys of each utterance in problem 1 / 2 (1 <= value <= S1 / S2; keys behind them are masked out), or None
    (d3pm_op_attention_pair_keylen)."""
    B, Tq, d = q1.shape
    S1, S2 = k1.shape[1], k2.shape[1]
    for t in (q1, q2, k1, v1, k2, v2):
        assert t.stride(2) == 1
    assert q1.stride(1) == q2.stride(1) and k1.stride(1) == v1.stride(1) == k2.stride(1) == v2.stride(1)
    assert q1.stride(0) == Tq * q1.stride(1) and q2.stride(0) == Tq * q2.stride(1)
    assert k1.stride(0) == S1 * k1.stride(1) and k2.stride(0) == S2 * k2.stride(1)
    o1 = torch.empty((B, Tq, d), dtype=q1.dtype, device=q1.device)
    o2 = torch.empty_like(o1)
    if key_len is not None or key_len2 is not None:
        for name, kl in (("key_len", key_len), ("key_len2", key_len2)):
            if kl is not None and (not isinstance(kl, torch.Tensor) or kl.dtype != torch.int32 or kl.shape != (B,) or kl.device != q1.device
                                   or not kl.is_contiguous()):
                raise D3PMError(f"{name} must be a contiguous int32 [{B}] tensor on {q1.device}")
        check(lib().d3pm_op_attention_pair_keylen(dtype_code(q1.dtype), _p(q1), _p(k1), _p(v1), _p(o1), S1, _p(q2), _p(k2), _p(v2), _p(o2),
                                                  S2, q1.stride(1), k1.stride(1), d, B, Tq, n_heads, d // n_heads, float(scale),
                                                  _p(key_len), _p(key_len2), C.byref(TUNING), stream_ptr()), "d3pm_op_attention_pair_keylen")
        return o1, o2
    check(lib().d3pm_op_attention_pair(dtype_code(q1.dtype), _p(q1), _p(k1), _p(v1), _p(o1), S1, _p(q2), _p(k2), _p(v2), _p(o2), S2,
                                       q1.stride(1), k1.stride(1), d, B, Tq, n_heads, d // n_heads, float(scale), C.byref(TUNING),
                                       stream_ptr()), "d3pm_op_attention_pair")
    return o1, o2


def _require_int32(pairs, dev):
    for name, t, shape in pairs:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
            raise D3PMError(f"{name} must be a contiguous int32 {list(shape)} tensor on {dev}")


def op_attention_pair_segments(q1, k1, v1, q2, k2, v2, seg_start, seg_len, n_heads, scale, out1, out2, capacity, *, key_len=None,
                               key_len2=None):
    """The cross pair of the deduplicated loop (d3pm_op_attention_pair_segments): q1 / q2 / out1 / out2 [rows, d], where utterance b owns
    the seg_len[b] rows (any count from 1 up to `capacity`) from row seg_start[b] (any row); k1 / v1 [B, S1, d], k2 / v2 [B, S2, d] as in
    op_attention_pair; key_len / key_len2 int32 [B] or None.  Writes out1 / out2 in place (rows no segment owns keep what they hold)
    and returns them.  The kernel is the planner's choice under the current tuning; a plan that takes no segments raises D3PMError."""
    if q1.dim() != 2 or k1.dim() != 3 or k2.dim() != 3:
        raise D3PMError("op_attention_pair_segments: q / out [rows, d] and k / v [B, S, d]")
    rows, d = q1.shape
    B, S1, S2 = k1.shape[0], k1.shape[1], k2.shape[1]
    dev = q1.device
    same = (q2, out1, out2)
    if any(t.shape != q1.shape for t in same) or k1.shape != v1.shape or k2.shape != v2.shape or k2.shape[0] != B or k1.shape[2] != d or k2.shape[2] != d:
        raise D3PMError("op_attention_pair_segments: q1 / q2 / out1 / out2 [rows, d], k1 / v1 [B, S1, d], k2 / v2 [B, S2, d]")
    tensors = (q1, q2, out1, out2, k1, v1, k2, v2)
    if any(t.dtype != q1.dtype or t.device != dev or t.stride(-1) != 1 for t in tensors):
        raise D3PMError("op_attention_pair_segments: one dtype, one device, unit column strides")
    if q1.stride(0) != q2.stride(0) or out1.stride(0) != out2.stride(0) or len({t.stride(1) for t in (k1, v1, k2, v2)}) != 1 or \
            k1.stride(0) != S1 * k1.stride(1) or v1.stride(0) != S1 * v1.stride(1) or k2.stride(0) != S2 * k2.stride(1) or v2.stride(0) != S2 * v2.stride(1):
        raise D3PMError("op_attention_pair_segments: q1 / q2, out1 / out2 and the four K / V views share their row strides; K / V batches are dense")
    if not isinstance(capacity, int) or capacity <= 0 or capacity % 128 or capacity > rows:
        raise D3PMError(f"op_attention_pair_segments: capacity {capacity!r} must be a multiple of 128 within the {rows} rows")
    ints = [("seg_start", seg_start, (B,)), ("seg_len", seg_len, (B,))]
    ints += [(n, t, (B,)) for n, t in (("key_len", key_len), ("key_len2", key_len2)) if t is not None]
    _require_int32(ints, dev)
    check(lib().d3pm_op_attention_pair_segments(dtype_code(q1.dtype), _p(q1), _p(k1), _p(v1), _p(out1), S1, _p(q2), _p(k2), _p(v2), _p(out2), S2,
                                                q1.stride(0), k1.stride(1), out1.stride(0), B, capacity, n_heads, d // n_heads, float(scale),
                                                _p(seg_start), _p(seg_len), _p(key_len), _p(key_len2), C.byref(TUNING), stream_ptr()),
          "d3pm_op_attention_pair_segments")
    return out1, out2


def op_posterior_sample_rows(shape, schedule, logits, row_of, x_t, t, seed, *, utt0=0, flags=0, known=None, temperature=1.0, top_k=0,
                             top_p=1.0, guidance=0.0, want_second=False):
    """The sampler launch of the deduplicated loop on its own (d3pm_op_posterior_sample_rows): x_t int32 [B, shape.canvas]; logits
    [B * canvas, n_classes] f16 / bf16 (a view with a wider row stride allowed); row_of int32 [B * canvas]: canvas row r draws from
    logits[row_of[r]] (clamped into the rows by the kernel).  known uint8 [B, canvas] or None.  Returns x_next, or (x_next, second)
    with want_second, the second output being what the loop writes into its trace.  `schedule` a Schedule; guidance is refused by the
    library (the deduplicated launch has no guided form)."""
    if not isinstance(x_t, torch.Tensor) or x_t.dim() != 2 or x_t.shape[1] != shape.canvas or x_t.dtype != torch.int32 or not x_t.is_contiguous():
        raise D3PMError(f"x_t must be a contiguous int32 [B, {shape.canvas}] tensor")
    dev, rows = x_t.device, x_t.numel()
    if not isinstance(logits, torch.Tensor) or tuple(logits.shape) != (rows, shape.n_classes) or logits.dtype not in (torch.float16, torch.bfloat16) or \
            logits.device != dev or logits.stride(1) != 1 or logits.stride(0) < shape.n_classes:
        raise D3PMError(f"logits must be a float16 / bfloat16 [{rows}, {shape.n_classes}] tensor on {dev} with unit column stride")
    _require_int32([("row_of", row_of, (rows,))], dev)
    if known is not None:
        _require(known, "known", tuple(x_t.shape), (torch.uint8,), dev)
    smp = nucleus_options(temperature, top_k, top_p, shape.n_classes)
    nuc = None if smp is None else smp if isinstance(smp, Nucleus) else Nucleus(smp.temperature, smp.top_k, 1.0)
    gd = guidance_options(guidance)
    x_next = torch.empty_like(x_t)
    second = torch.empty_like(x_t) if want_second else None
    check(lib().d3pm_op_posterior_sample_rows(C.byref(shape), x_t.shape[0], _p(logits), dtype_code(logits.dtype), logits.stride(0), _p(row_of),
                                              _p(x_t), _p(x_next), _p(second), _p(known), int(t), C.byref(schedule.c_struct), seed, utt0, flags,
                                              None if nuc is None else C.byref(nuc), None if gd is None else C.byref(gd), stream_ptr()),
          "d3pm_op_posterior_sample_rows")
    return (x_next, second) if want_second else x_next


def _require_table(t, name, shape, dtype, dev, min_rows=None):
    """A contiguous table of `dtype` on `dev`; with min_rows the leading extent may be anything from min_rows up."""
    ok = isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and t.is_contiguous() and t.dim() == len(shape) and \
        tuple(t.shape[1:]) == tuple(shape[1:]) and (t.shape[0] >= min_rows if min_rows is not None else t.shape[0] == shape[0])
    if not ok:
        lead = [f">= {min_rows}"] + list(shape[1:]) if min_rows is not None else list(shape)
        raise D3PMError(f"{name} must be a contiguous {dtype} {lead} tensor on {dev}")


def op_nar_embed(lens, text, prom, resp, n_given, w_text, w_prom, w_resp, sep, pe, t_max, *, x=None, row_mask=None, key_len=None):
    """The NAR stage's input assembly on its own (d3pm_op_nar_embed): lens int32 [B, 3]; text int32 [B, tt_max]; prom int32
    [B, tp_max, n_prom_levels] (-1 = level absent); resp int32 [B, tr_max, resp_stride], levels 0 .. n_given - 1 summed; tables of one
    float dtype: w_text [n_tokens, d], w_prom [n_prom_levels, n_tokens, d], w_resp [>= n_given, n_tokens, d], sep [d], pe [>= t_max, d].
    Returns (x [B, t_max, d], row_mask uint8 [B, t_max], key_len int32 [B]); each may be handed in (a contiguous view of a larger
    buffer is fine: nothing outside the view is written)."""
    if not isinstance(lens, torch.Tensor) or lens.dim() != 2 or lens.shape[1] != 3 or lens.shape[0] == 0:
        raise D3PMError("lens must be an int32 [B, 3] tensor")
    if not isinstance(w_text, torch.Tensor) or w_text.dim() != 2 or w_text.dtype not in _DTYPES:
        raise D3PMError(f"w_text must be a [n_tokens, d] tensor of one of {tuple(_DTYPES)}")
    if not all(isinstance(t, torch.Tensor) and t.dim() == n for t, n in ((text, 2), (prom, 3), (resp, 3))):
        raise D3PMError("text [B, tt_max], prom [B, tp_max, n_prom_levels] and resp [B, tr_max, resp_stride] must be tensors")
    B, dev, dtype = lens.shape[0], lens.device, w_text.dtype
    (n_tokens, d), levels, stride = w_text.shape, prom.shape[2], resp.shape[2]
    if not isinstance(n_given, int) or not isinstance(t_max, int) or t_max <= 0 or not 1 <= n_given <= stride:
        raise D3PMError(f"op_nar_embed: t_max {t_max!r} must be positive and n_given {n_given!r} within 1 .. {stride}")
    _require_int32([("lens", lens, (B, 3)), ("text", text, (B, text.shape[1])), ("prom", prom, (B, prom.shape[1], levels)),
                    ("resp", resp, (B, resp.shape[1], stride))], dev)
    _require_table(w_text, "w_text", (n_tokens, d), dtype, dev)
    _require_table(w_prom, "w_prom", (levels, n_tokens, d), dtype, dev)
    _require_table(w_resp, "w_resp", (n_given, n_tokens, d), dtype, dev, min_rows=n_given)
    _require_table(sep, "sep", (d,), dtype, dev)
    _require_table(pe, "pe", (t_max, d), dtype, dev, min_rows=t_max)
    x = torch.empty((B, t_max, d), dtype=dtype, device=dev) if x is None else x
    row_mask = torch.empty((B, t_max), dtype=torch.uint8, device=dev) if row_mask is None else row_mask
    key_len = torch.empty((B,), dtype=torch.int32, device=dev) if key_len is None else key_len
    _require(x, "x", (B, t_max, d), (dtype,), dev)
    _require(row_mask, "row_mask", (B, t_max), (torch.uint8,), dev)
    _require_int32([("key_len", key_len, (B,))], dev)
    check(lib().d3pm_op_nar_embed(dtype_code(dtype), _p(lens), _p(text), text.shape[1], _p(prom), prom.shape[1], levels, _p(resp), resp.shape[1],
                                  stride, n_given, _p(w_text), _p(w_prom), _p(w_resp), _p(sep), _p(pe), _p(x), _p(row_mask), _p(key_len), B,
                                  t_max, d, n_tokens, stream_ptr()), "d3pm_op_nar_embed")
    return x, row_mask, key_len


def op_adaln(x, emb_row, row_mask, *, out=None):
    """AdaLN of the NAR stage on its own (d3pm_op_adaln): x [M, d] with dense rows, emb_row [2 d] = (log gamma | beta) of one level,
    row_mask uint8 [M]; returns y [M, d] (or `out`), rows with a zero mask entry zero.  The addresses go to the library as they are:
    a view whose storage offset breaks the 16-byte alignment of x, out or emb_row takes the scalar kernel at d = 512 / 1024."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype not in _DTYPES or not x.is_contiguous() or x.numel() == 0:
        raise D3PMError(f"x must be a contiguous [M, d] tensor of one of {tuple(_DTYPES)}")
    M, d = x.shape
    dev = x.device
    _require(emb_row, "emb_row", (2 * d,), (x.dtype,), dev)
    _require(row_mask, "row_mask", (M,), (torch.uint8,), dev)
    out = torch.empty_like(x) if out is None else out
    _require(out, "out", (M, d), (x.dtype,), dev)
    check(lib().d3pm_op_adaln(dtype_code(x.dtype), _p(x), _p(out), _p(emb_row), _p(row_mask), M, d, stream_ptr()), "d3pm_op_adaln")
    return out


def _nar_draw_extents(logits, lens, resp, level):
    """The tensor checks the two draw entries share -> (B, t_max, n_tokens, ldl, device)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3 or logits.dtype not in _DTYPES or logits.numel() == 0:
        raise D3PMError(f"logits must be a [B, t_max, n_tokens] tensor of one of {tuple(_DTYPES)}")
    B, t_max, n_tokens = logits.shape
    dev, ldl = logits.device, logits.stride(1)
    if logits.stride(2) != 1 or ldl < n_tokens or logits.stride(0) != t_max * ldl:
        raise D3PMError("logits: unit column stride, a row stride >= n_tokens, utterances t_max rows apart")
    if not isinstance(resp, torch.Tensor) or resp.dim() != 3:
        raise D3PMError("resp must be an int32 [B, tr_max, resp_stride] tensor")
    _require_int32([("lens", lens, (B, 3)), ("resp", resp, (B, resp.shape[1], resp.shape[2]))], dev)
    if not isinstance(level, int) or not 0 <= level < resp.shape[2] - 1:
        raise D3PMError(f"level {level!r} must be within 0 .. {resp.shape[2] - 2}")
    return B, t_max, n_tokens, ldl, dev


def op_nar_sample(logits, lens, resp, level, temperature, seed, *, utt0=0, flags=0):
    """The NAR stage's level draw on its own (d3pm_op_nar_sample): logits [B, t_max, n_tokens] of a float dtype (a view with a wider
    row stride allowed, dense in t), lens int32 [B, 3], resp int32 [B, tr_max, resp_stride]: column level + 1 of every response frame
    inside the grid is written in place; returns resp.  flags: FLAG_GREEDY."""
    B, t_max, n_tokens, ldl, dev = _nar_draw_extents(logits, lens, resp, level)
    check(lib().d3pm_op_nar_sample(dtype_code(logits.dtype), _p(logits), ldl, _p(lens), _p(resp), resp.shape[1], resp.shape[2], t_max,
                                   n_tokens, level, float(temperature), seed, utt0, flags, B, stream_ptr()), "d3pm_op_nar_sample")
    return resp


def op_nar_draw(logits, lens, resp, level, temperature, seed, *, utt0=0, flags=0, top_k=0, top_p=1.0, known=None, logprob_out=None,
                theta_out=None):
    """op_nar_sample with the draw options (d3pm_op_nar_draw): top_k / top_p as nar_draw_options checks them; known uint8 [B, tr_max]
    (a frame with a non-zero byte keeps the id resp holds); logprob_out float32 [B, tr_max, resp_stride - 1], column `level` of every
    response frame inside the grid written; theta_out float32 [B, tr_max].  With every option at its default this is op_nar_sample's
    launch.  Returns resp."""
    B, t_max, n_tokens, ldl, dev = _nar_draw_extents(logits, lens, resp, level)
    top_k, top_p = nar_draw_options(top_k, top_p, n_tokens)
    tr_max = resp.shape[1]
    if known is not None:
        _require(known, "known", (B, tr_max), (torch.uint8,), dev)
    if logprob_out is not None:
        _require(logprob_out, "logprob_out", (B, tr_max, resp.shape[2] - 1), (torch.float32,), dev)
    if theta_out is not None:
        _require(theta_out, "theta_out", (B, tr_max), (torch.float32,), dev)
    draw = nar_draw_struct(top_k, top_p, known, logprob_out, theta_out)
    check(lib().d3pm_op_nar_draw(dtype_code(logits.dtype), _p(logits), ldl, _p(lens), _p(resp), tr_max, resp.shape[2], t_max, n_tokens,
                                 level, float(temperature), seed, utt0, flags, B, None if draw is None else C.byref(draw), stream_ptr()),
          "d3pm_op_nar_draw")
    return resp


def op_nar_draw_guided(logits, lens, resp, level, temperature, seed, guidance, *, utt0=0, flags=0, top_k=0, top_p=1.0, known=None,
                       logprob_out=None, theta_out=None):
    """op_nar_draw under classifier-free guidance (d3pm_op_nar_draw_guided): logits [2 B, t_max, n_tokens], lens [2 B, 3] and resp
    [2 B, tr_max, resp_stride] hold the B utterances and behind them their null twins; the draw runs on rn<T>(fmaf(guidance, c - u, c))
    and writes the id into both halves of resp.  known / logprob_out / theta_out are [B, ...].  guidance: a finite weight >= 0 (0 is
    legal here and draws from the conditioned half).  Returns resp."""
    B2, t_max, n_tokens, ldl, dev = _nar_draw_extents(logits, lens, resp, level)
    if B2 % 2:
        raise D3PMError(f"guided logits hold 2 * batch utterances, got {B2}")
    B = B2 // 2
    guidance_options(guidance)
    gd = Guidance(float(guidance))
    top_k, top_p = nar_draw_options(top_k, top_p, n_tokens)
    tr_max = resp.shape[1]
    if known is not None:
        _require(known, "known", (B, tr_max), (torch.uint8,), dev)
    if logprob_out is not None:
        _require(logprob_out, "logprob_out", (B, tr_max, resp.shape[2] - 1), (torch.float32,), dev)
    if theta_out is not None:
        _require(theta_out, "theta_out", (B, tr_max), (torch.float32,), dev)
    draw = nar_draw_struct(top_k, top_p, known, logprob_out, theta_out)
    check(lib().d3pm_op_nar_draw_guided(dtype_code(logits.dtype), _p(logits), ldl, _p(lens), _p(resp), tr_max, resp.shape[2], t_max, n_tokens,
                                        level, float(temperature), seed, utt0, flags, B, None if draw is None else C.byref(draw),
                                        C.byref(gd), stream_ptr()), "d3pm_op_nar_draw_guided")
    return resp


def stats_buffer(M: int, parts: int, device) -> torch.Tensor:
    """Storage of the row moments in the library's layout [ceil(M / 16), parts, 16, 2] (include/d3pm_hip.h: d3pm_op_row_stats)."""
    return torch.zeros(((M + 15) // 16, parts, 16, 2), dtype=torch.float32, device=device)


def stats_rows(st: torch.Tensor, M: int) -> torch.Tensor:
    """The same moments as [M, parts, 2] (row-major view for tests)."""
    return st.permute(0, 2, 1, 3).reshape(-1, st.shape[1], 2)[:M]


def op_row_stats(x, *, stats=None):
    """[M, d] 16-bit rows -> the fp32 partial (sum, sum of squares) per 32-column part, in the library's layout (stats_buffer).
    stats: a preallocated moment buffer (tests)."""
    M, d = x.shape
    st = stats_buffer(M, d // 32, x.device) if stats is None else stats
    check(lib().d3pm_op_row_stats(dtype_code(x.dtype), _p(x), x.stride(0), M, d, _p(st), stream_ptr()), "d3pm_op_row_stats")
    return st


def op_linear_stats(x, w, bias, r1, *, r2=None, row_mask=None, mask_period=1, out=None, stats=None):
    """(y, stats): y = residual epilogue of d3pm_op_linear, stats = the moments of the rows of y (layout of stats_buffer).
    out: a preallocated y [M, N] (any row stride; it may be r1); stats: a preallocated moment buffer (tests)."""
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=x.dtype, device=x.device) if out is None else out
    st = stats_buffer(M, N // 32, x.device) if stats is None else stats
    check(lib().d3pm_op_linear_stats(dtype_code(x.dtype), _p(x), x.stride(0), _p(w), _p(bias), _p(y), y.stride(0), _p(r1), _p(r2), r1.stride(0),
                                     _p(row_mask), mask_period, M, N, K, _p(st), C.byref(TUNING), stream_ptr()), "d3pm_op_linear_stats")
    return y, st


def op_dedup_index(tokens, frame_mask, n_classes, table=None, seg_align=128):
    """Row deduplication index of tokens / frame_mask [batch, canvas] (d3pm_op_dedup_index_align): dict of seg_start, seg_len [batch], m_live [1],
    row_of, cid [batch * canvas] (int32), cmask [batch * canvas] (uint8) and, with `table` [n_classes, d], x [batch * canvas, d] and its
    moments `stats` (fp32, the library's layout).  Rows the index does not define keep the sentinels they are created with here.
    seg_align: 128 = an utterance owns its class count rounded up to 128 rows (d3pm_op_dedup_index); 1 = the count itself, the dense
    segments the sampler loop runs on; anything else is refused by the library."""
    batch, canvas = tokens.shape
    n, dev = batch * canvas, tokens.device
    i32 = lambda k, fill: torch.full((k,), fill, dtype=torch.int32, device=dev)      # noqa: E731
    out = {"seg_start": i32(batch, -1), "seg_len": i32(batch, -1), "m_live": i32(1, -1), "row_of": i32(n, -1), "cid": i32(n, -7),
           "cmask": torch.full((n,), 7, dtype=torch.uint8, device=dev)}
    scratch = i32(n + batch, 0)
    d, dt = 0, BF16 if table is None else dtype_code(table.dtype)
    if table is not None:
        d = table.shape[1]
        out["x"] = torch.full((n, d), 3.0, dtype=table.dtype, device=dev)
        out["stats"] = torch.full((((n + 15) // 16) * 16 * (d // 32) * 2,), 5.0, dtype=torch.float32, device=dev)
    check(lib().d3pm_op_dedup_index_align(dt, _p(tokens), _p(frame_mask), batch, canvas, n_classes, d, int(seg_align), _p(table),
                                          _p(out["seg_start"]), _p(out["seg_len"]), _p(out["m_live"]), _p(out["row_of"]), _p(out["cid"]),
                                          _p(out["cmask"]), _p(out.get("x")), _p(out.get("stats")), _p(scratch), stream_ptr()),
          "d3pm_op_dedup_index_align")
    return out


def op_linear_live(x, w, bias, y, m_live, x2=None, r1=None, row_mask=None, act=0, fold_s=None, fold_b=None, stats_in=None, stats_out=None,
                   m_est=None, rows_est=None):
    """y [M, N] (written in place: only the tiles that hold a row < m_live[0]) = the projection of d3pm_op_linear_live; M = x.shape[0]
    is the capacity.  m_est: the host's estimate of m_live (d3pm_op_linear_live_est; 0 = none).  rows_est: the estimate that sizes big
    tiles (d3pm_op_linear_live_rows; 0 = none).  The schedule is the module's TUNING."""
    M, K = x.shape
    N = w.shape[0]
    args = (dtype_code(x.dtype), _p(x), _p(x2), x.stride(0), _p(w), _p(bias), _p(y), y.stride(0), _p(r1),
            r1.stride(0) if r1 is not None else 0, _p(row_mask), row_mask.numel() if row_mask is not None else 1, M, N, K, act,
            _p(fold_s), _p(fold_b), _p(stats_in), _p(stats_out), _p(m_live))
    if rows_est is not None:
        check(lib().d3pm_op_linear_live_rows(*args, int(m_est or 0), int(rows_est), C.byref(TUNING), stream_ptr()), "d3pm_op_linear_live_rows")
    elif m_est is None:
        check(lib().d3pm_op_linear_live(*args, C.byref(TUNING), stream_ptr()), "d3pm_op_linear_live")
    else:
        check(lib().d3pm_op_linear_live_est(*args, int(m_est), C.byref(TUNING), stream_ptr()), "d3pm_op_linear_live_est")
    return y


def op_fold_weights(w, bias, gamma, beta, film=None):
    """(Wf [N, K] in w's dtype, fold_s [N] fp32, fold_b [N] fp32) of one LayerNorm-fed projection (d3pm_op_fold_weights)."""
    N, K = w.shape
    wf = torch.empty_like(w)
    fs = torch.empty(N, dtype=torch.float32, device=w.device)
    fb = torch.empty(N, dtype=torch.float32, device=w.device)
    check(lib().d3pm_op_fold_weights(dtype_code(w.dtype), _p(w), _p(bias), _p(gamma), _p(beta), _p(film), N, K, _p(wf), _p(fs), _p(fb),
                                     stream_ptr()), "d3pm_op_fold_weights")
    return wf, fs, fb


def op_linear_fold(x, wf, fold_s, fold_b, stats, *, act=0, eps=1e-6, out=None):
    """act(LN-folded projection) of the raw rows x [M, K] with their moments `stats` (d3pm_op_linear_fold).
    out: a preallocated y [M, N] with any row stride (tests)."""
    M, K = x.shape
    N = wf.shape[0]
    y = torch.empty((M, N), dtype=x.dtype, device=x.device) if out is None else out
    check(lib().d3pm_op_linear_fold(dtype_code(x.dtype), _p(x), x.stride(0), _p(wf), _p(fold_s), _p(fold_b), _p(stats), eps, _p(y), y.stride(0),
                                    M, N, K, act, C.byref(TUNING), stream_ptr()), "d3pm_op_linear_fold")
    return y


def op_embed_qkv(shape, weights, tokens, frame_mask):
    """The block-0 q | k | v rows [n, 3 d_model] of `tokens` int32 [n] under `frame_mask` uint8 [n], gathered from the per-id table the
    sampler loop builds under ln_fold = 1 (d3pm_op_embed_qkv).  shape: Shape, weights: DeviceWeights with build_fold done."""
    n = tokens.numel()
    need = lib().d3pm_op_embed_qkv_bytes(C.byref(shape), n)
    if need == 0:
        raise D3PMError("d3pm_op_embed_qkv: needs a 16-bit model, d_model a multiple of 256 and n_q <= 1")
    dtype = {v: k for k, v in _DTYPES.items()}[shape.dtype]
    storage = torch.empty(need, dtype=torch.uint8, device=tokens.device)
    q = torch.empty((n, shape.d_model), dtype=dtype, device=tokens.device)
    kv = torch.empty((n, 2 * shape.d_model), dtype=dtype, device=tokens.device)
    check(lib().d3pm_op_embed_qkv(C.byref(shape), C.byref(weights.c_struct), _p(tokens), _p(frame_mask), n, _p(storage), need, _p(q),
                                  _p(kv), stream_ptr()), "d3pm_op_embed_qkv")
    return torch.cat([q, kv], dim=1)


def op_layernorm(x, w, b, film=None, eps=1e-6):
    y = torch.empty_like(x)
    check(lib().d3pm_op_layernorm(dtype_code(x.dtype), _p(x), _p(y), _p(w), _p(b), _p(film), x.shape[0], x.shape[1],
                                  eps, stream_ptr()), "d3pm_op_layernorm")
    return y


def op_linear_rowpanel(x, w, bias, r1, ln_w, ln_b, *, x2=None, ln2_w=None, ln2_b=None, film=None, row_mask=None, eps=1e-6, mx=False):
    """Projection onto the residual stream + the LayerNorm(s) of the new rows in one launch (include/d3pm_hip.h).
    Returns (y, ln_y, ln2_y | None); with mx=True the LayerNorm rows come back in the block-scaled fp8 format:
    (y, (codes, scales), (codes2, scales2) | None)."""
    M, K = x.shape
    if not (tuple(w.shape) == (512, K) and tuple(r1.shape) == (M, 512) and x.stride(1) == 1 and w.is_contiguous() and r1.is_contiguous()):
        raise ValueError("op_linear_rowpanel: x [M,K], w [512,K], r1 [M,512]")
    if x2 is not None and (x2.shape != x.shape or x2.stride() != x.stride()):
        raise ValueError("op_linear_rowpanel: x2 must look like x")
    y = torch.empty_like(r1)
    if mx:
        ln_y = torch.empty((M, 512), dtype=torch.uint8, device=x.device)
        ln2_y = torch.empty_like(ln_y) if ln2_w is not None else None
        sx = torch.empty((M, 4, 4), dtype=torch.uint8, device=x.device)
        sx2 = torch.empty_like(sx) if ln2_w is not None else None
    else:
        ln_y = torch.empty_like(r1)
        ln2_y = torch.empty_like(r1) if ln2_w is not None else None
        sx = sx2 = None
    check(lib().d3pm_op_linear_rowpanel(dtype_code(x.dtype), _p(x), _p(x2), x.stride(0), _p(w), _p(bias), _p(y), _p(r1), _p(row_mask),
                                        0 if row_mask is None else row_mask.numel(), M, K, _p(ln_w), _p(ln_b), _p(ln_y),
                                        _p(ln2_w), _p(ln2_b), _p(ln2_y), _p(film), eps, _p(sx), _p(sx2), stream_ptr()),
          "d3pm_op_linear_rowpanel")
    if mx:
        return y, (ln_y, sx), ((ln2_y, sx2) if ln2_w is not None else None)
    return y, ln_y, ln2_y


class NarRunner:
    """Pointer tables + workspace of the stock NAR model (d3pm_nar_level)."""

    def __init__(self, cfg, tensors: dict, dtype: torch.dtype, device, pe: torch.Tensor):
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        lib()
        self.shape = NarShape(cfg.d_model, cfg.n_heads, cfg.n_layers, cfg.n_tokens, cfg.n_prom_levels, cfg.n_resp_levels,
                              dtype_code(dtype), C.pointer(TUNING))
        self._keep = [pe]

        def ptr(key):
            t = tensors[key]
            if not (t.is_cuda and t.is_contiguous()):
                raise D3PMError(f"weight {key} must be a contiguous device tensor")
            self._keep.append(t)
            return t.data_ptr()

        self.blocks = (NarBlockWeights * cfg.n_layers)()
        names = {"attn_norm_emb": "attn.norm.emb.weight", "to_qkv_w": "attn.block.to_qkv.weight",
                 "to_out_w": "attn.block.to_out.weight", "to_out_b": "attn.block.to_out.bias",
                 "ffn_norm_emb": "ffn.norm.emb.weight", "ffn0_w": "ffn.block.0.weight", "ffn0_b": "ffn.block.0.bias",
                 "ffn3_w": "ffn.block.3.weight", "ffn3_b": "ffn.block.3.bias"}
        for i in range(cfg.n_layers):
            for field, key in names.items():
                setattr(self.blocks[i], field, ptr(f"blocks.{i}.{key}"))
        self.weights = NarWeights(ptr("text_emb.weight"), ptr("proms_emb.weight"), ptr("resps_emb.weight"), ptr("sep"),
                                  ptr("classifier.weight"), ptr("classifier.bias"), pe.data_ptr(), pe.shape[0], self.blocks)
        self._ws = None

    def level(self, lens, text, prom, resp, t_max, level, temperature, seed, utt0=0, flags=0, want_logits=False, draw=None,
              guidance=None):
        """One quantizer level for the whole batch; `resp` [B, tr_max, n_resp_levels+1] int32 is updated in place.  draw: None = the
        draw without options (d3pm_nar_level), else a NarDraw (d3pm_nar_level_draw) whose tensors the caller keeps alive.
        guidance: a Guidance struct = d3pm_nar_level_guided: the arrays hold the B // 2 utterances and behind them their null twins, the
        draw's arrays are [B // 2, ...] and the logits returned are those of all B."""
        cfg, B = self.cfg, lens.shape[0]
        need = lib().d3pm_nar_workspace_bytes(C.byref(self.shape), B, t_max)
        if need == 0:
            raise D3PMError("d3pm_nar_workspace_bytes: " + lib().d3pm_last_error().decode())
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        logits = torch.empty((B, t_max, cfg.n_tokens), dtype=self.dtype, device=self.device) if want_logits else None
        if guidance is not None:
            if B % 2:
                raise D3PMError(f"a guided level holds 2 * batch utterances, got {B}")
            check(lib().d3pm_nar_level_guided(C.byref(self.shape), C.byref(self.weights), B // 2, t_max, _p(lens), _p(text), text.shape[1],
                                              _p(prom), prom.shape[1], _p(resp), resp.shape[1], int(level), float(temperature), seed,
                                              utt0, flags, _p(self._ws), self._ws.numel(), _p(logits),
                                              None if draw is None else C.byref(draw), C.byref(guidance), stream_ptr()),
                  "d3pm_nar_level_guided")
            return logits
        if draw is not None:
            check(lib().d3pm_nar_level_draw(C.byref(self.shape), C.byref(self.weights), B, t_max, _p(lens), _p(text), text.shape[1],
                                            _p(prom), prom.shape[1], _p(resp), resp.shape[1], int(level), float(temperature), seed,
                                            utt0, flags, _p(self._ws), self._ws.numel(), _p(logits), C.byref(draw), stream_ptr()),
                  "d3pm_nar_level_draw")
            return logits
        check(lib().d3pm_nar_level(C.byref(self.shape), C.byref(self.weights), B, t_max, _p(lens), _p(text), text.shape[1],
                                   _p(prom), prom.shape[1], _p(resp), resp.shape[1], int(level), float(temperature), seed,
                                   utt0, flags, _p(self._ws), self._ws.numel(), _p(logits), stream_ptr()), "d3pm_nar_level")
        return logits


def uniform(seed: int, t: int, row0: int, rows: int, n_classes: int, stream_id: int, device) -> torch.Tensor:
    out = torch.empty((rows, n_classes), dtype=torch.float32, device=device)
    check(lib().d3pm_uniform(seed, t, row0, rows, n_classes, stream_id, _p(out), stream_ptr()), "d3pm_uniform")
    return out


# ---- schedule choices: fields of this module's default Tuning (what every Sampler / NarRunner / op_* call passes) --------------
def set_gemm_variant(v: int):
    if v not in (0, 2, 3, 4, 5, 6, 7, 8):
        raise D3PMError(f"gemm_variant {v}: not a shipped schedule (include/d3pm_hip.h)")
    lib()
    TUNING.gemm_variant = v


def set_attn_query_groups(v: int):
    if v not in (0, 1, 2, 4, 32, 33):
        raise D3PMError(f"attn_query_groups {v}: not a shipped schedule (include/d3pm_hip.h)")
    lib()
    TUNING.attn_query_groups = v


def set_attn_pair_sequential(v):
    """0 / False never, 1 auto (default), 2 / True always."""
    lib()
    TUNING.attn_pair_sequential = 2 if v is True else int(v)


def set_lat_tile(v: int):
    lib()
    TUNING.lat_tile = int(v)


def set_row_panel(mask: int):
    lib()
    TUNING.row_panel = int(mask)


def set_attn_cross_resident(v):
    """0 / False never, 1 auto (default), 2 / True always, 3 one query block per workgroup."""
    lib()
    TUNING.attn_cross_resident = 2 if v is True else int(v)


def set_gemm_persist_slots(v: int):
    lib()
    TUNING.gemm_persist_slots = int(v)


def set_workspace_alias(v: bool):
    lib()
    TUNING.workspace_alias = 1 if v else 0


# (ln_fold = 3, the every-row arm of the row deduplication, and 4, its big-tiles-in-every-iteration arm, are A/B values: set_tuning_field /
# bench.py --tune take them, tuning() does not)
_TUNING_VALUES = {"gemm_variant": (0, 2, 3, 4, 5, 6, 7, 8, 9, 10), "attn_query_groups": (0, 1, 2, 4, 32, 33), "lat_tile": (0, 1, 2, 3),
                  "attn_pair_sequential": (0, 1, 2), "attn_cross_resident": (0, 1, 2, 3, 4, 5), "workspace_alias": (0, 1), "ln_fold": (0, 1, 2)}


@contextlib.contextmanager
def tuning(**fields):
    """`with _hip.tuning(attn_query_groups=32, row_panel=0): ...` -- schedule choices for the calls made inside the block; the
    module's default Tuning is restored on exit, also when the body raises, so no test or caller can leak a schedule."""
    lib()
    for name, value in fields.items():
        if name not in TUNING_FIELDS:
            raise D3PMError(f"unknown tuning field {name!r}: one of {TUNING_FIELDS}")
        ok = _TUNING_VALUES.get(name)
        if ok is not None and int(value) not in ok:
            raise D3PMError(f"{name} = {value}: not a shipped schedule (include/d3pm_hip.h)")
    saved = {name: getattr(TUNING, name) for name in fields}
    try:
        for name, value in fields.items():
            setattr(TUNING, name, int(value))
        yield TUNING
    finally:
        for name, value in saved.items():
            setattr(TUNING, name, value)


def reset_tuning():
    """Back to the library's defaults (d3pm_tuning_default); an attached profiler stays attached."""
    prof = TUNING.prof
    lib().d3pm_tuning_default(C.byref(TUNING))
    TUNING.prof = prof



def set_tuning_field(name: str, value: int):
    """bench.py --tune name=value"""
    if name not in TUNING_FIELDS:
        raise D3PMError(f"unknown tuning field {name!r}: one of {TUNING_FIELDS}")
    lib()
    setattr(TUNING, name, int(value))


# ---- timing hooks: a d3pm_prof handle attached to the default Tuning ------------------------------------------------------
def prof_enable(kclass: int, max_events: int):
    prof_disable()
    h = C.c_void_p()
    check(lib().d3pm_prof_create(kclass, max_events, C.byref(h)), "d3pm_prof_create")
    TUNING.prof = h.value


def prof_read():
    if not TUNING.prof:
        return 0, 0.0, 0.0, 0.0
    n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
    check(lib().d3pm_prof_read(TUNING.prof, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), "d3pm_prof_read")
    return n.value, ms.value, fl.value, by.value


def prof_read_class(kclass: int):
    """(launches, total ms, algorithmic flops, algorithmic bytes) of one kernel class; does not reset.  Zeros when no
    profiler is attached (bench.py --no-kernel-events)."""
    if not TUNING.prof:
        return 0, 0.0, 0.0, 0.0
    n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
    check(lib().d3pm_prof_read_class(TUNING.prof, kclass, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), "d3pm_prof_read_class")
    return n.value, ms.value, fl.value, by.value


def prof_disable():
    if TUNING.prof:
        lib().d3pm_prof_destroy(TUNING.prof)
        TUNING.prof = None


def profiling() -> bool:
    return bool(TUNING.prof)


import atexit  # noqa: E402

atexit.register(lambda: prof_disable() if _lib is not None else None)      # a process that exits with a profiler attached frees its events

"""Data-parallel sharding of utterances over the GPUs of one node.

Utterances are independent (weights replicated, one Philox row block per *global* utterance index),
so the batch is split contiguously over ranks with no data-path collective; the only exchange is one
all-gather of the generated int32 token grid at the end (RCCL over xGMI when the backend is "nccl";
gloo in the CPU tests).  Results are independent of the number of ranks: the noise rows are keyed by the global utterance
index, every GEMM schedule is bit-compatible with every other, and the one choice that is not -- the instruction shape of the
attention kernels, picked by batch size -- is made for the GLOBAL batch on every rank (`global_batch=`, d3pm_tuning.regime_batch).
tests/test_gpu_batch_sweep.py holds a shard against the unsplit batch bit for bit.
The reference has no multi-GPU inference (its only distributed code is DeepSpeed DP training,
/root/reference/vall_e/train.py:29-31); this module is new in the build.
"""
from __future__ import annotations

from numbers import Integral
from typing import Callable, Optional, Sequence

import torch
import torch.distributed as dist


def shard_bounds(n_items: int, world: int, rank: int) -> tuple[int, int]:
    """Contiguous split; the first n_items % world ranks get one extra utterance."""
    base, extra = divmod(n_items, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


_PER_UTTERANCE = ("n_frames", "known", "known_mask", "null_text_list", "null_proms_list")


def _shard_kwargs(kw: dict, lo: int, hi: int) -> dict:
    """Per-utterance keyword arguments of AR.generate_audio (a sequence n_frames, known, known_mask) cut to the shard."""
    out = dict(kw)
    for name in _PER_UTTERANCE:
        v = out.get(name)
        if v is not None and not isinstance(v, Integral):
            out[name] = list(v[lo:hi])
    return out


def generate_audio_dp(model, text_list: Sequence[torch.Tensor], proms_list: Sequence[torch.Tensor], *, seed: int,
                      group=None, generate_fn: Optional[Callable] = None, **kw) -> torch.Tensor:
    """Every rank passes the same global lists and gets back the same int64 [B, canvas] grid ([B, canvas, n_q] for a model
    built with n_q > 1).  Keyword arguments that are per call (steps, greedy, fp8, temperature, top_k, top_p, reveal_steps, choice_temperature, revise, mask_padding, ...) go to every
    rank as they are (mask_padding derives its key counts from the shard's own texts, prompts and n_frames); the per-utterance ones (a sequence n_frames, known, known_mask) are cut to the rank's shard."""
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank(group) if world > 1 else 0
    B = len(text_list)
    lo, hi = shard_bounds(B, world, rank)
    fn = generate_fn or model.generate_audio
    if generate_fn is None:
        kw = dict(kw, global_batch=B)          # a shard takes the attention kernels of the unsplit batch: same ids at any rank count
    if hi > lo:
        local = fn(list(text_list[lo:hi]), list(proms_list[lo:hi]), seed=seed, utt0=lo, **_shard_kwargs(kw, lo, hi))
        local = local.reshape(hi - lo, -1).to(torch.int32)
    else:
        local = None
    n_q = max(1, getattr(model.cfg, "n_q", 1))
    shape = (-1, model.cfg.canvas) if n_q == 1 else (-1, model.cfg.canvas, n_q)
    if world == 1:
        return local.long().reshape(shape)
    canvas = model.cfg.canvas * n_q
    dev = local.device if local is not None else model.device
    per = -(-B // world)                                   # padded shard so one fixed-size all-gather suffices
    send = torch.zeros((per, canvas), dtype=torch.int32, device=dev)
    if local is not None:
        send[: hi - lo] = local
    recv = torch.empty((world * per, canvas), dtype=torch.int32, device=dev)
    dist.all_gather_into_tensor(recv, send, group=group)
    parts = []
    for r in range(world):
        a, b = shard_bounds(B, world, r)
        parts.append(recv[r * per: r * per + (b - a)])
    return torch.cat(parts).long().reshape(shape)


def generate_codes_dp(ar, nar, text_list: Sequence[torch.Tensor], proms_list: Sequence[torch.Tensor], *, seed: int,
                      group=None, ar_fn: Optional[Callable] = None, nar_fn: Optional[Callable] = None,
                      nar_kw: Optional[dict] = None, **kw) -> torch.Tensor:
    """Both stages of the reference's inference script (/root/reference/vall_e/__main__.py:60-71) sharded the same way:
    every rank runs the D3PM stage and then the NAR stage (levels 1..7) for its contiguous slice of the utterances --
    noise keyed by the global utterance index in both -- and ONE all-gather returns the int64 [B, n_frames, 8] codes
    to every rank.  No collective sits between the stages: a rank's NAR input is its own D3PM output.
    With a sequence `n_frames` (one length per utterance) the NAR stage sees utterance b's own L_b frames and the result is
    [B, max L, 8], zero beyond L_b.
    nar_kw: keyword options of the NAR stage (NAR.forward: sampling_temperature, greedy, top_k, top_p, known, known_mask, guidance,
    null_text_list, null_proms_list); the per-utterance lists among them (known, known_mask, the null lists) are cut to the rank's
    shard like those of the D3PM stage.  The result is the
    codes alone, so return_logprobs is not taken here."""
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank(group) if world > 1 else 0
    B = len(text_list)
    lo, hi = shard_bounds(B, world, rank)
    levels = nar.n_resp_levels + 1
    nf = kw.get("n_frames")
    lens = [int(ar.cfg.n_frames if nf is None else nf)] * B if nf is None or isinstance(nf, Integral) else [int(v) for v in nf]
    if len(lens) != B:
        raise ValueError(f"n_frames has {len(lens)} entries for {B} utterances")
    n_frames = max(lens)
    nar_kw = dict(nar_kw or {})
    if nar_kw.get("return_logprobs") or nar_kw.get("return_logits_level") is not None:
        raise ValueError("generate_codes_dp returns the codes alone: call the NAR model itself for its log-probabilities or logits")
    gen = ar_fn or ar.generate_audio
    fill = nar_fn or nar
    if ar_fn is None:
        kw = dict(kw, global_batch=B)
    local = None
    if hi > lo:
        texts, proms = list(text_list[lo:hi]), list(proms_list[lo:hi])
        lvl0 = gen(texts, proms, seed=seed, utt0=lo, **_shard_kwargs(kw, lo, hi)).reshape(hi - lo, -1)
        resps = [lvl0[b][: lens[lo + b]].clamp(max=nar.n_tokens - 1).reshape(-1, 1) for b in range(hi - lo)]
        full = fill(texts, proms, resps, seed=seed, utt0=lo, **_shard_kwargs(nar_kw, lo, hi))
        local = torch.zeros((hi - lo, n_frames, levels), dtype=torch.int32, device=full[0].device)
        for b, f in enumerate(full):
            local[b, : lens[lo + b]] = f.reshape(lens[lo + b], levels).to(torch.int32)
    if world == 1:
        return local.long()
    dev = local.device if local is not None else ar.device
    per = -(-B // world)
    send = torch.zeros((per, n_frames, levels), dtype=torch.int32, device=dev)
    if local is not None:
        send[: hi - lo] = local
    recv = torch.empty((world * per, n_frames, levels), dtype=torch.int32, device=dev)
    dist.all_gather_into_tensor(recv, send, group=group)
    parts = []
    for r in range(world):
        a, b = shard_bounds(B, world, r)
        parts.append(recv[r * per: r * per + (b - a)])
    return torch.cat(parts).long()

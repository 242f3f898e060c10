"""Drop-in `NAR`: the stock non-autoregressive VALL-E model that fills quantizer levels 1..7 once the D3PM sampler
has produced level 0 (the step right after the hot path: /root/reference/vall_e/__main__.py:36-38,
SURVEY.md §8f row 1).

Same surface as the reference's /root/reference/vall_e/vall_e/nar.py `class NAR(Base)`: ctor
`NAR(n_tokens, d_model=512, n_heads=8, n_layers=12, p_dropout=0.1)` (base.py:316-323), state-dict key layout
(base.py:336-360), `forward(text_list, proms_list, resps_list, sampling_temperature=0.2) -> [LongTensor[t, 8]]`.
Every level runs in HIP behind `d3pm_nar_level`; PyTorch stores the weights.  Sampling uses a Philox Gumbel-max instead of
torch's multinomial stream (`seed=`).  The training branch (nar.py:53-74: responses of 8 levels) computes the loss in HIP as well
(`forward`), and `forward_backward` adds the gradient of every parameter to `.grad` (nar_train.py: fp32 models).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch
from torch import Tensor, nn

from . import _hip
from .ar_discrete import SymmapState
from .synth import NARConfig


def _sinusoid_table(n: int, d_model: int, dtype: torch.dtype) -> Tensor:
    """base.py:38-89: omega computed in fp32, then it follows the module dtype (.half() rounds it)."""
    half = d_model // 2
    omega = torch.exp(-math.log(1e4) * (torch.arange(half, dtype=torch.float32) / half)).to(dtype)
    ang = omega[None, :] * torch.arange(n)[:, None]
    return torch.cat([ang.sin(), ang.cos()], dim=-1)


class _Table(nn.Module):
    def __init__(self, *shape):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(*shape))


class _AdaLNParams(nn.Module):
    def __init__(self, d, n_levels):
        super().__init__()
        self.emb = nn.Embedding(n_levels, 2 * d)
        nn.init.zeros_(self.emb.weight)


class _AttnParams(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.to_qkv = nn.Linear(d, 3 * d, bias=False)
        self.to_out = nn.Linear(d, d)


class _Prenorm(nn.Module):
    def __init__(self, block, d, n_levels):
        super().__init__()
        self.block = block
        self.norm = _AdaLNParams(d, n_levels)


class _BlockParams(nn.Module):
    """Parameter container with upstream's names (base.py:197-222); never called."""

    def __init__(self, d, n_levels):
        super().__init__()
        self.attn = _Prenorm(_AttnParams(d), d, n_levels)
        self.ffn = _Prenorm(nn.Sequential(nn.Linear(d, 4 * d), nn.GELU(), nn.Dropout(0.0), nn.Linear(4 * d, d)), d, n_levels)


def guidance_twins(text_list, proms_list, resps_list, null_text_list=None, null_proms_list=None):
    """The 2 B lists of a guided call (include/d3pm_hip.h: d3pm_nar_level_guided): behind the B utterances their null twins -- the empty
    text `text[:0]` and the empty prompt `prom[:0]` unless the caller gives others, which are used as they are -- each with the
    response of its utterance (the same tensor).  Host only: nothing here reads a tensor's contents.  ValueError for lists of
    the wrong length."""
    B = len(resps_list)
    if not (len(text_list) == len(proms_list) == B):
        raise ValueError(f"{len(text_list)} texts, {len(proms_list)} prompts and {B} responses")
    for name, given in (("null_text_list", null_text_list), ("null_proms_list", null_proms_list)):
        if given is not None and len(given) != B:
            raise ValueError(f"{name} has {len(given)} entries for {B} utterances")
    null_text = [t[:0] for t in text_list] if null_text_list is None else list(null_text_list)
    null_proms = [p[:0] for p in proms_list] if null_proms_list is None else list(null_proms_list)
    return list(text_list) + null_text, list(proms_list) + null_proms, list(resps_list) + list(resps_list)


def cond_drop_lists(text_list, proms_list, seed, utt0, cond_drop, device):
    """The texts and prompts of a training step under cond_drop = p or (p_text, p_prompt) (train.cond_drop_probs): utterance b loses
    its text and / or its prompt (replaced by the empty one) by train.cond_drop_decision(seed, utt0 + b, ...), a function of (seed,
    utt) alone -- Philox stream 5, the D3PM stage's rule.  -> (texts, prompts, [(dropped text?, dropped prompt?)])."""
    from . import train
    p_text, p_prompt = train.cond_drop_probs(cond_drop)
    texts, proms, dropped = [], [], []
    for b, (t, p) in enumerate(zip(text_list, proms_list)):
        dt, dp_ = train.cond_drop_decision(seed, utt0 + b, p_text, p_prompt, device)
        texts.append(t[:0] if dt else t)
        proms.append(p[:0] if dp_ else p)
        dropped.append((dt, dp_))
    return texts, proms, dropped


class NAR(SymmapState, nn.Module):
    n_resp_levels = 7
    n_prom_levels = 8
    pad_rows_to_tiles = True      # _pack: round the padded grid up so that batch * t_max is a multiple of 192 (big-tile GEMMs)

    def __init__(self, n_tokens: int = 1024, d_model: int = 512, n_heads: int = 8, n_layers: int = 12, p_dropout: float = 0.1):
        super().__init__()
        self.cfg = NARConfig(d_model=d_model, n_heads=n_heads, n_layers=n_layers, n_tokens=n_tokens)
        self.n_tokens = n_tokens
        self.text_emb = _Table(n_tokens, d_model)
        self.proms_emb = _Table(self.n_prom_levels, n_tokens, d_model)
        self.resps_emb = _Table(self.n_resp_levels, n_tokens, d_model)
        self.sep = nn.Parameter(torch.randn(d_model))
        self.blocks = nn.ModuleList([_BlockParams(d_model, self.n_resp_levels) for _ in range(n_layers)])
        self.classifier = nn.Linear(d_model, n_tokens)
        self._runner = None
        self._runner_key = None
        self._init_symmaps()

    @property
    def dtype(self):
        return self.classifier.weight.dtype

    @property
    def device(self):
        return self.classifier.weight.device

    def runner(self, t_max: int) -> _hip.NarRunner:
        self._no_cpu_path()
        sd = dict(self.named_parameters())
        key = (self.dtype, self.device, tuple((k, v.data_ptr(), v._version) for k, v in sd.items()))
        if self._runner is None or self._runner_key != key or self._runner.weights.pe_rows < t_max:
            rows = max(2048, t_max)
            pe = _sinusoid_table(rows, self.cfg.d_model, self.dtype).to(self.device).contiguous()
            with torch.cuda.device(self.device):
                self._runner = _hip.NarRunner(self.cfg, {k: v.detach() for k, v in sd.items()}, self.dtype, self.device, pe)
            self._runner_key = key
        return self._runner

    def _pack(self, text_list, proms_list, resps_list):
        """Ragged lists -> padded int32 grids on the model's device.  The lengths come from the tensors' shapes (host
        integers): nothing here reads device memory back, so a batch that is already on the GPU (the D3PM stage's output)
        is packed without a single synchronisation."""
        import torch.nn.functional as F
        from torch.nn.utils.rnn import pad_sequence
        dev = self.device
        lens_host = [(len(t), len(p), len(r)) for t, p, r in zip(text_list, proms_list, resps_list)]
        i32 = lambda x: x.to(device=dev, dtype=torch.int32, non_blocking=True)
        text = pad_sequence([i32(t) for t in text_list], batch_first=True)
        # absent prompt levels are -1 (they contribute nothing), padded prompt rows are 0 like upstream's zero padding
        prom = pad_sequence([F.pad(i32(p), (0, self.n_prom_levels - p.shape[-1]), value=-1) for p in proms_list], batch_first=True)
        resp = pad_sequence([F.pad(i32(r), (0, self.n_resp_levels + 1 - r.shape[-1])) for r in resps_list], batch_first=True)
        # a batch without a single phoneme or without a single prompt frame (dropped conditions, null twins alone) keeps one padding
        # column / row: the index arrays the kernels take are never empty, and nothing reads past an utterance's own length
        if text.shape[1] == 0:
            text = text.new_zeros((text.shape[0], 1))
        if prom.shape[1] == 0:
            prom = prom.new_zeros((prom.shape[0], 1, self.n_prom_levels))
        lens = torch.tensor(lens_host, dtype=torch.int32).to(dev, non_blocking=True)
        t_max = max(a + b_ + c for a, b_, c in lens_host) + 2
        if self.pad_rows_to_tiles:
            # t_max is the padded grid's row count per utterance (rows past an utterance's own length are masked padding): a few more
            # of them make batch * t_max a multiple of 192, so the projections run as big-tile GEMMs (192 x 128) instead of
            # one 128 x 128 tile per workgroup -- same bits (the schedules accumulate in the same order)
            step = 192 // math.gcd(len(lens_host), 192)
            padded = -(-t_max // step) * step
            if padded * 100 <= t_max * 103:
                t_max = padded
        return lens, text.contiguous(), prom.contiguous(), resp.contiguous(), t_max, lens_host

    def _no_cpu_path(self):
        if self.device.type != "cuda":
            raise RuntimeError("the NAR levels run on MI355X only: move the model to a HIP device; there is no CPU path")

    @torch.no_grad()
    def forward_backward(self, text_list: Sequence[Tensor], proms_list: Sequence[Tensor], resps_list: Sequence[Tensor], *,
                         seed: Optional[int] = None, utt0: int = 0, quant_levels=None, dropout=False, cond_drop=0.0) -> Tensor:
        """One training step's loss and gradients (nar.py:53-74, base.py:403-488; nar_train.py): resps_list [t, 8] each.  Utterance b
        takes the level l_b = quant_levels[b], or the draw of (seed, utt0 + b) (seed=None: one from torch.randint, as generate_audio
        does); levels 0 .. l_b go in and level l_b + 1 is the target.  nll = the mean cross-entropy over all response frames of the
        call; its gradient is ADDED to `.grad` (fp32) of every parameter.  dropout: False = eval arithmetic, True = upstream's
        p = 0.1 at its three sites per block, a number = that probability.  Returns the fp32 scalar loss and sets
        `self.loss = {"nll": loss}`, where upstream's gather_attribute("loss") reads it.
        cond_drop: p or (p_text, p_prompt) -- per utterance the text and / or the prompt is replaced by the empty one (the null twin of
        forward(guidance=...)) before packing, decided by train.cond_drop_decision(seed, utt0 + b, ...): Philox stream 5, the D3PM
        stage's rule, a function of (seed, utt) alone; 0 / False (default) is the step without it, bit for bit.  Data parallel: each rank's loss is the mean
        over its own frames and train.all_reduce_gradients averages the ranks, as DeepSpeed does upstream.
        ValueError before any GPU work: lists of unequal length, a response that is not 8 levels wide or is empty, quant_levels of
        the wrong length or outside 0 .. 6, a dropout outside [0, 1), a cond_drop that is no probability or pair of them."""
        from . import nar_train, train
        nar_train.validate(text_list, proms_list, resps_list, quant_levels=quant_levels, dropout=dropout, n_layers=self.cfg.n_layers)
        p_text, p_prompt = train.cond_drop_probs(cond_drop)
        self._no_cpu_path()
        if p_text > 0.0 or p_prompt > 0.0:
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            with torch.cuda.device(self.device):
                text_list, proms_list, _ = cond_drop_lists(text_list, proms_list, seed, utt0, (p_text, p_prompt), self.device)
        loss, _ = nar_train.NARTrainer(self).step(text_list, proms_list, resps_list, seed=seed, utt0=utt0, quant_levels=quant_levels,
                                                  dropout=dropout)
        self.loss = {"nll": loss}
        return loss

    def _check_known(self, resps_list, known, known_mask):
        """ValueError for a known / known_mask pair that does not fit the responses; nothing here reads a tensor's contents."""
        if (known is None) != (known_mask is None):
            raise ValueError("known and known_mask go together: give both or neither")
        if known is None:
            return
        if len(known) != len(resps_list) or len(known_mask) != len(resps_list):
            raise ValueError(f"known has {len(known)} and known_mask {len(known_mask)} entries for {len(resps_list)} utterances")
        for b, (r, k, m) in enumerate(zip(resps_list, known, known_mask)):
            if not isinstance(k, Tensor) or k.dim() != 2 or tuple(k.shape) != (r.shape[0], self.n_resp_levels + 1) or k.is_floating_point():
                raise ValueError(f"known[{b}] must be an integer [{r.shape[0]}, {self.n_resp_levels + 1}] tensor of codes, got "
                                 f"{tuple(k.shape) if isinstance(k, Tensor) else type(k).__name__}")
            if not isinstance(m, Tensor) or m.dtype != torch.bool or tuple(m.shape) != (r.shape[0],):
                raise ValueError(f"known_mask[{b}] must be a bool [{r.shape[0]}] tensor")

    @torch.no_grad()
    def forward(self, text_list: Sequence[Tensor], proms_list: Sequence[Tensor], resps_list: Sequence[Tensor],
                sampling_temperature: float = 0.2, *, seed: Optional[int] = None, greedy: bool = False, utt0: int = 0,
                return_logits_level: Optional[int] = None, quant_levels=None, top_k: int = 0, top_p: float = 1.0, known=None,
                known_mask=None, return_logprobs: bool = False, guidance: float = 0.0, null_text_list=None, null_proms_list=None):
        """resps_list: [t, l] with the levels already known (l = 1 after the D3PM stage) -> [LongTensor[t, 8]].
        l = 8 is upstream's training call (nar.py:53-74): the loss of forward_backward(..., seed=, utt0=, quant_levels=) without
        gradients goes to `self.loss = {"nll": loss}` and [] is returned.

        Options of the level draw (include/d3pm_hip.h: d3pm_nar_draw; with all of them at their defaults the call makes the launches it
        makes without them):
          top_k, top_p     every level draws from the top_k largest of its rn(logit / sampling_temperature) (0 = off, ties kept) and
                           from the smallest set of them that carries the share top_p of the softmax mass (1 = off).
          known, known_mask  per utterance a [t, 8] tensor of codes and a bool [t]: at a frame whose mask is set, levels l .. 7 of the
                           result are known's and the later levels are conditioned on them; levels < l of `known` are ignored (those
                           of resps_list stand).  Both or neither.
          return_logprobs  -> (codes, [FloatTensor[t, 7]]): column c = the model's log-probability (its own logits: no temperature, no
                           cut) of the level c + 1 code that stands in the result, drawn or known; 0 in the columns of levels that
                           were given.
          guidance         w > 0: classifier-free guidance in every level's draw (include/d3pm_hip.h: d3pm_nar_level_guided).  Each
                           level is one evaluation of 2 B utterances -- behind the B of the call their null twins, `text[:0]` and
                           `prom[:0]` with the same response, or null_text_list / null_proms_list as they are -- and frame f draws from
                           rn(fmaf(w, c - u, c)) of its two rows; top_k / top_p, known, return_logprobs (the log-softmax of the guided
                           logits), greedy and utt0 act on that row, and the noise is that of the call without guidance.  The
                           results are those of the B utterances; return_logits_level returns the grid of all 2 B.  0 (default) is
                           the call without it, launch for launch.  Meaningful for weights trained with the conditions dropped some of
                           the time (forward_backward(cond_drop=...)); no statement about audio quality is made.
        ValueError before any GPU work: lists of unequal length, a known / known_mask of the wrong shape or one without the other,
        top_k / top_p out of range, a guidance that is not finite and >= 0, null lists without guidance or of the wrong length, and
        any of these options together with the 8-level training call."""
        levels = {r.shape[-1] for r in resps_list}
        if len(levels) > 1:
            raise ValueError(f"Please give only one level, got {levels}.")
        n_given = next(iter(levels))
        options = top_k != 0 or top_p != 1.0 or known is not None or known_mask is not None or return_logprobs
        guide = _hip.guidance_options(guidance)
        if guide is None and (null_text_list is not None or null_proms_list is not None):
            raise ValueError("null_text_list / null_proms_list belong to guidance: give a weight > 0 with them")
        if guide is not None and n_given == self.n_resp_levels + 1:
            raise ValueError("guidance belongs to the inference call: the responses have all 8 levels, which is the training call")
        if guide is not None:
            guidance_twins(text_list, proms_list, resps_list, null_text_list, null_proms_list)      # the lists' lengths
        if options:
            if n_given == self.n_resp_levels + 1:
                raise ValueError("top_k / top_p / known / known_mask / return_logprobs belong to the inference call: the responses "
                                 "have all 8 levels, which is the training call")
            if not (len(text_list) == len(proms_list) == len(resps_list)):
                raise ValueError(f"{len(text_list)} texts, {len(proms_list)} prompts and {len(resps_list)} responses")
            top_k, top_p = _hip.nar_draw_options(top_k, top_p, self.n_tokens)
            self._check_known(resps_list, known, known_mask)
        if n_given == self.n_resp_levels + 1:
            from . import nar_train
            nar_train.validate(text_list, proms_list, resps_list, quant_levels=quant_levels)
            self._no_cpu_path()
            loss, _ = nar_train.NARTrainer(self).step(text_list, proms_list, resps_list, seed=seed, utt0=utt0, quant_levels=quant_levels,
                                                      backward=False)
            self.loss = {"nll": loss}
            return []
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        held = None
        if known is not None:
            # the known codes go into the levels the stage has yet to fill, at the masked frames alone: _pack carries them into `resp`,
            # where the draw leaves them and the next level's input assembly reads them
            dev = self.device
            resps_list = [torch.cat([r.to(dev), (k.to(dev)[:, n_given:] * m.to(dev)[:, None]).to(r.dtype)], dim=1)
                          for r, k, m in zip(resps_list, known, known_mask)]
        B = len(resps_list)
        if guide is not None:
            # (after the known codes went into the responses: both halves carry them)
            text_list, proms_list, resps_list = guidance_twins(text_list, proms_list, resps_list, null_text_list, null_proms_list)
        lens, text, prom, resp, t_max, lens_host = self._pack(text_list, proms_list, resps_list)
        run = self.runner(t_max)
        flags = _hip.FLAG_GREEDY if greedy else 0
        logits = None
        with torch.cuda.device(self.device):
            if known is not None:
                from torch.nn.utils.rnn import pad_sequence
                held = pad_sequence([m.to(device=self.device, dtype=torch.uint8) for m in known_mask], batch_first=True).contiguous()
            logprob = torch.zeros((B, resp.shape[1], self.n_resp_levels), dtype=torch.float32, device=self.device) if return_logprobs else None
            draw = _hip.nar_draw_struct(top_k, top_p, held, logprob) if options else None
            for level in range(n_given - 1, self.n_resp_levels):
                lg = run.level(lens, text, prom, resp, t_max, level, sampling_temperature, seed, utt0, flags,
                               want_logits=(return_logits_level == level), draw=draw, guidance=guide)
                if lg is not None:
                    logits = lg
        out = [resp[b, : lens_host[b][2]].long() for b in range(B)]
        if return_logprobs:
            scores = [logprob[b, : lens_host[b][2]] for b in range(B)]
            return (out, logits, lens, t_max, scores) if return_logits_level is not None else (out, scores)
        return (out, logits, lens, t_max) if return_logits_level is not None else out

"""Drop-in `AR` model of the discrete-diffusion (D3PM, absorbing state) codec-token sampler.

Same public surface as the reference's /root/reference/vall_e/vall_e/ar_discrete.py `class AR`
(ctor signature :205, `generate_audio` :696, `p_sample` :401, `q_sample` :467, `timesteps`,
state-dict key layout :210-240) but the reverse process runs in hand-written HIP kernels for
gfx950 behind the C ABI of include/d3pm_hip.h.  PyTorch only stores the weights, runs the two
small once-per-utterance condition encoders (:216-230, 0.3 % of the reference's time) and provides
the HIP stream.  There is no CPU or eager fallback for the diffusion loop.

Differences from upstream, all opt-in or strictly more general:
  * the ctor honours its arguments (upstream overrides them with d=32,H=16,L=8,steps=100, :207-238);
    `AR.reference_native()` builds exactly the upstream shape;
  * batches: upstream only works for one utterance (:699); here B utterances are B independent
    runs (per-utterance Philox noise stream), returned as [B, canvas];
  * noise comes from a counter-based Philox stream (`seed=`) instead of the CPU Mersenne generator;
  * the 630 MB of dense transition tables are replaced by their 4 fp16 scalars per step.
"""
from __future__ import annotations

import math
from collections import namedtuple
from numbers import Integral
from typing import Optional, Sequence, Union

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _hip
from .synth import MASK_ID, N_CLASSES, D3PMConfig

# generate_audio(return_logprobs=True): logprob float32 and step int32, [B, canvas] each (include/d3pm_hip.h: d3pm_frame_scores)
FrameScores = namedtuple("FrameScores", ("logprob", "step"))


class _Mlp(nn.Module):
    """timm-style Mlp (fc1 -> act -> fc2); state-dict keys fc1.*, fc2.* as upstream's timm import."""

    def __init__(self, d_in, d_hidden, d_out, act):
        super().__init__()
        self.fc1 = nn.Linear(d_in, d_hidden)
        self.act = act
        self.fc2 = nn.Linear(d_hidden, d_out)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _LevelSumEmbedding(nn.Module):
    """Prompt embedding: sum over quantizer levels of per-level tables (base.py:244-274)."""

    def __init__(self, n_levels, n_tokens, d):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(n_levels, n_tokens, d))

    def forward(self, codes: Tensor) -> Tensor:
        """codes int64 [..., S, l<=n_levels] -> [..., S, d]; fp32 sum, one rounding (the one-hot
        contraction upstream accumulates the <= 8 non-zero terms in fp32)."""
        w = self.weight
        out = torch.zeros(codes.shape[:-1] + (w.shape[-1],), dtype=torch.float32, device=w.device)
        for lvl in range(codes.shape[-1]):
            out += F.embedding(codes[..., lvl], w[lvl]).float()
        return out.to(w.dtype)


class _DiTBlockParams(nn.Module):
    """Parameter container with upstream's names (ar_discrete.py:103-124).  Never called: the
    block forward is the HIP path.  cross_attn2 is kept so upstream state dicts load strictly."""

    def __init__(self, d, heads):
        super().__init__()
        self.norm1 = nn.LayerNorm(d, eps=1e-6)
        self.attn = nn.MultiheadAttention(d, heads)
        self.norm2 = nn.LayerNorm(d, eps=1e-6)
        self.cross_attn = nn.MultiheadAttention(d, heads)
        self.norm22 = nn.LayerNorm(d, eps=1e-6)
        self.cross_attn2 = nn.MultiheadAttention(d, heads)
        self.norm3 = nn.LayerNorm(d, eps=1e-6)
        self.mlp = _Mlp(d, 4 * d, d, nn.GELU())
        self.timestep_fc = nn.Linear(d, 2 * d)

    def forward(self, *a, **k):
        raise RuntimeError("DiT blocks execute inside libd3pm_hip.so; call AR.generate_audio")


def _sinusoid_table(n: int, d_model: int, dtype: torch.dtype) -> Tensor:
    """[n, d] host table [sin | cos] as upstream's SinusodialEmbedding yields it (ar_discrete.py:41-72):
    omega is *computed* in fp16, then follows the module dtype (`.half()` keeps it, `.float()` widens
    the fp16 values) and the angles / sin / cos are evaluated in that dtype."""
    half = d_model // 2
    omega = torch.exp(-math.log(1e4) * (torch.arange(half, dtype=torch.float16) / half)).to(dtype)
    ang = omega[None, :] * torch.arange(n)[:, None]
    return torch.cat([ang.sin(), ang.cos()], dim=-1)


class SymmapState:
    """`phone_symmap` / `spkr_symmap` as the reference's export attaches them to the trained module
    (/root/reference/vall_e/export.py:18-19; read back as `ar.phone_symmap` at /root/reference/vall_e/__main__.py:56).
    Upstream ships them inside a whole-module pickle; here they ride in the state dict under one extra key,
    `_symmaps`, present only when a map is set -- so a state dict exported upstream (no such key) loads strictly,
    and a state dict saved here loads upstream after `sd.pop("_symmaps", None)`."""
    SYMMAP_KEY = "_symmaps"

    def _init_symmaps(self):
        self.phone_symmap: dict = {}      # {phone symbol: id >= 1}, data.py:125-127
        self.spkr_symmap: dict = {}       # {speaker name: id >= 0}, data.py:133-134

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        sd = super().state_dict(*args, destination=destination, prefix=prefix, keep_vars=keep_vars)
        if self.phone_symmap or self.spkr_symmap:
            sd[prefix + self.SYMMAP_KEY] = {"phone_symmap": dict(self.phone_symmap), "spkr_symmap": dict(self.spkr_symmap)}
        return sd

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        state_dict = dict(state_dict)
        maps = state_dict.pop(self.SYMMAP_KEY, None)
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        if maps is not None:
            self.phone_symmap = dict(maps.get("phone_symmap", {}))
            self.spkr_symmap = dict(maps.get("spkr_symmap", {}))
        return out

    @classmethod
    def load_exported(cls, path, **ctor):
        """A checkpoint written by tools/convert_upstream_pickle.py (run once in the upstream environment on the
        whole-module pickle of /root/reference/vall_e/export.py:20): {"state_dict", "phone_symmap", "spkr_symmap"}."""
        blob = torch.load(path, map_location="cpu")
        model = cls(**ctor) if ctor else cls.reference_native() if hasattr(cls, "reference_native") else cls()
        model.load_state_dict(blob["state_dict"])
        model.phone_symmap = dict(blob.get("phone_symmap") or {})
        model.spkr_symmap = dict(blob.get("spkr_symmap") or {})
        return model


class AR(SymmapState, nn.Module):
    n_resp_levels = 1
    num_classes = N_CLASSES

    def __init__(self, d_model=512, n_steps=100, n_tokens=1024, max_n_levels=8, n_heads=8, num_layers=6, *,
                 canvas: int = 448, n_frames: int = 350, s_text: int = 50, s_prompt: int = 398, n_q: int = 1):
        """Positional arguments as upstream (ar_discrete.py:205).  `n_q` > 1 is this build's extension (SURVEY.md section 8d
        config 2, BASELINE.json configs[1] "x 8 quantizers"; upstream generates level 0 only and leaves levels 1..7 to the NAR
        model): the D3PM then denoises all n_q quantizer levels of a frame jointly -- token grids [B, canvas, n_q], a frame's
        input = the sum of its level embeddings (`resps_emb.weight` [n_q, K, d]), `final` has n_q * K outputs, and every
        (frame, level) is sampled like a level-0 token.  n_q = 1 is the upstream model, bit for bit."""
        super().__init__()
        if n_tokens + 1 != N_CLASSES:
            raise ValueError("the absorbing-state tables assume 1024 codec ids + 1 mask id")
        if not 1 <= n_q <= 16:
            raise ValueError("n_q must be in 1..16")
        self.cfg = D3PMConfig(d_model=d_model, n_heads=n_heads, n_layers=num_layers, canvas=canvas, n_frames=n_frames,
                              s_text=s_text, s_prompt=s_prompt, timesteps=n_steps, n_levels=max_n_levels, n_q=n_q)
        self.n_resp_levels = n_q
        cfg, d = self.cfg, d_model
        self.timesteps = n_steps                       # read at call time, like upstream (:750)
        self.text_emb = nn.Embedding(N_CLASSES, d, padding_idx=0)
        self.proms_emb = _LevelSumEmbedding(max_n_levels, N_CLASSES, d)
        self.resps_emb = nn.Embedding(N_CLASSES, d, padding_idx=0) if n_q == 1 else _LevelSumEmbedding(n_q, N_CLASSES, d)
        self.time_emb = nn.Embedding(n_steps + 1, d)
        self.token_emb = nn.Embedding(N_CLASSES, d)    # unused upstream too; kept for state-dict parity

        def encoder(mult):
            layer = nn.TransformerEncoderLayer(d_model=d, nhead=cfg.cond_heads, dim_feedforward=cfg.cond_ff, dropout=0.0)
            return nn.Sequential(nn.TransformerEncoder(layer, num_layers=cfg.cond_layers, enable_nested_tensor=False),
                                 _Mlp(d, d * mult, d, nn.SiLU()))

        self.encodertext = encoder(2)
        self.encoder2 = encoder(3)
        self.blocks = nn.ModuleList([_DiTBlockParams(d, n_heads) for _ in range(num_layers)])
        self.final = nn.Linear(d, n_q * N_CLASSES)
        self._pe_cache = {}
        self.eps = 1.0e-6
        self._sampler = None
        self._sampler_key = None
        self.loop_streams = 1     # >1: the batch is cut into that many independent chunks on separate HIP streams
        self._streams = []
        self._init_symmaps()

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def reference_native(cls) -> "AR":
        """The only shape upstream's class can build: d=32, 16 heads, 8 blocks, 100 steps."""
        return cls(d_model=32, n_steps=100, n_tokens=1024, max_n_levels=8, n_heads=16, num_layers=8)

    @classmethod
    def from_config(cls, cfg: D3PMConfig) -> "AR":
        return cls(cfg.d_model, cfg.timesteps, cfg.n_classes - 1, cfg.n_levels, cfg.n_heads, cfg.n_layers,
                   canvas=cfg.canvas, n_frames=cfg.n_frames, s_text=cfg.s_text, s_prompt=cfg.s_prompt, n_q=cfg.n_q)

    @property
    def dtype(self) -> torch.dtype:
        return self.final.weight.dtype

    @property
    def device(self) -> torch.device:
        return self.final.weight.device

    def _pe(self):
        """(pe_text0 [1,d], pe_prompt [S_p,d]) in the model dtype on the model device, built on the host."""
        key = (self.dtype, self.device)
        if key not in self._pe_cache:
            self._pe_cache[key] = (_sinusoid_table(1, self.cfg.d_model, self.dtype).to(self.device),
                                   _sinusoid_table(self.cfg.s_prompt, self.cfg.d_model, self.dtype).to(self.device))
        return self._pe_cache[key]

    # ------------------------------------------------------------------ HIP sampler plumbing
    def sampler(self) -> _hip.Sampler:
        """(Re)binds the C-ABI pointer tables when weights moved or changed dtype."""
        if self.device.type != "cuda":
            raise RuntimeError("the D3PM sampler runs on MI355X only: move the model to a HIP device "
                               "(model.to('cuda')); there is no CPU path")
        sd = {k: v for k, v in self.named_parameters()}
        key = (self.dtype, self.device, tuple((k, v.data_ptr(), v._version) for k, v in sd.items()))
        if self._sampler is None or self._sampler_key != key:
            with torch.cuda.device(self.device):
                pe_text0, pe_prompt = self._pe()
                self._sampler = _hip.Sampler(self.cfg, {k: v.detach() for k, v in sd.items()}, self.dtype, self.device,
                                             pe_text0.contiguous(), pe_prompt.contiguous())
            self._sampler_key = key
        return self._sampler

    # ------------------------------------------------------------------ conditioning (torch-ROCm)
    @staticmethod
    def _pad_rows(x: Tensor, n: int) -> Tensor:
        if x.shape[0] >= n:
            return x[:n]
        return F.pad(x, [0, 0] * (x.dim() - 1) + [0, n - x.shape[0]])

    def _padded_inputs(self, text_list, proms_list):
        cfg, dev = self.cfg, self.device
        text = torch.stack([self._pad_rows(t.to(dev).long(), cfg.s_text) for t in text_list])           # [B,S_t]
        prom = torch.stack([self._pad_rows(p.to(dev).long(), cfg.s_prompt) for p in proms_list])        # [B,S_p,l]
        return text, prom

    def encode_conditions(self, text_list: Sequence[Tensor], proms_list: Sequence[Tensor], text_len=None, prom_len=None):
        """-> (cond_text [B,S_t,d], cond_prompt [B,S_p,d]) through the HIP condition encoders
        (d3pm_encode_conditions).  Same statements as upstream (:711-746): zero pad / truncate, embed, text gets
        PE(position 0) on every phoneme (the x.shape[0] quirk at :89), the prompt true positions; two post-norm
        encoder layers + Mlp.  Prompts with fewer than n_levels quantizer levels: the missing levels add nothing.
        text_len / prom_len (int32 [B] on the device, or None): the rows of each utterance that are keys of the encoder's
        self-attention (generate_audio(mask_padding=True)); upstream has every padded row as a key."""
        text, prom = self._padded_inputs(text_list, proms_list)
        if prom.shape[-1] < self.cfg.n_levels:
            prom = F.pad(prom, (0, self.cfg.n_levels - prom.shape[-1]), value=-1)
        with torch.cuda.device(self.device):
            return self.sampler().encode_conditions(text, prom, text_len, prom_len)

    def key_lengths(self, text_list, proms_list, n_frames: Union[int, Sequence[int], None] = None):
        """The key counts of generate_audio(mask_padding=True) as three lists of B ints (host arithmetic only): frames[b] = the live
        frames of utterance b, text[b] = min(len(text_b), s_text), prompt[b] = min(rows(prom_b), s_prompt).  ValueError for an
        empty text or prompt and for a frame count outside 1..canvas."""
        cfg, B = self.cfg, len(text_list)
        if n_frames is None or isinstance(n_frames, Integral):
            frames = [cfg.n_frames if n_frames is None else int(n_frames)] * B
        else:
            frames = [int(v) for v in n_frames]
        return _hip.key_lengths(frames, [int(t.shape[0]) if t.dim() else 0 for t in text_list],
                                [int(p.shape[0]) if p.dim() else 0 for p in proms_list], cfg.canvas, cfg.s_text, cfg.s_prompt)

    def encode_conditions_torch(self, text_list: Sequence[Tensor], proms_list: Sequence[Tensor]):
        """The same encoders on PyTorch-ROCm modules (tests cross-check the HIP path against it)."""
        text, prom = self._padded_inputs(text_list, proms_list)
        pe_text0, pe_prompt = self._pe()
        ct = self.text_emb(text) + pe_text0
        cp = self.proms_emb(prom) + pe_prompt
        # sequence-first batches: per-utterance arithmetic is what upstream's unbatched call does
        ct = self.encodertext(ct.transpose(0, 1)).transpose(0, 1)
        cp = self.encoder2(cp.transpose(0, 1)).transpose(0, 1)
        return ct.contiguous(), cp.contiguous()

    def canvas_init(self, batch: int, n_frames: Union[int, Sequence[int], None] = None):
        """x_T: `n_frames` mask ids then zeros; the frame mask is fixed for the whole loop (:699-709).  An int (or None: the
        constructor's n_frames) gives the mask every utterance shares, uint8 [canvas]; a sequence of `batch` ints gives utterance
        b its own `n_frames[b]` live frames and a mask uint8 [batch, canvas]."""
        cfg = self.cfg
        if n_frames is not None and not isinstance(n_frames, Integral):
            x, frame_mask, _ = self.canvas_init_known(batch, n_frames)
            return x, frame_mask
        n_frames = cfg.n_frames if n_frames is None else int(n_frames)
        if not 0 < n_frames <= cfg.canvas:
            raise ValueError(f"n_frames must be in 1..{cfg.canvas}")
        shape = (batch, cfg.canvas) if cfg.n_q == 1 else (batch, cfg.canvas, cfg.n_q)
        x = torch.zeros(shape, dtype=torch.int32, device=self.device)
        x[:, :n_frames] = MASK_ID
        frame_mask = (x[0].reshape(cfg.canvas, -1)[:, 0] != 0).to(torch.uint8)
        return x, frame_mask

    def canvas_init_known(self, batch: int, n_frames: Union[int, Sequence[int], None] = None, known=None, known_mask=None):
        """Per-utterance canvases (include/d3pm_hip.h: d3pm_canvas) -> (x_T int32 [batch, canvas(, n_q)], frame mask uint8
        [batch, canvas], known-frame map uint8 [batch, canvas] or None when no frame is given).
        Utterance b has L_b = n_frames[b] live frames (an int or None: the same for all).  known[b] (or None) is an int tensor
        [n] -- [n, n_q] for a model built with n_q > 1 -- of codec ids 0 .. 1023 for frames 0 .. n - 1, and known_mask[b] (or None) a
        bool [n] that marks which of them are given; without a mask all n are, i.e. a known[b] shorter than L_b is a prefix to
        continue.  x_T carries the given ids, the mask id on the other live frames and zeros on the padding.  Ids are taken
        verbatim: 512 is upstream's mask id (1025 // 2) and doubles as a codec id there, so a known 512 is legal and stays 512.
        Everything is validated here, on the host (ValueError); the kernels check nothing."""
        cfg = self.cfg
        if n_frames is None or isinstance(n_frames, Integral):
            lens = [cfg.n_frames if n_frames is None else int(n_frames)] * batch
        else:
            lens = [int(v) for v in n_frames]
        if len(lens) != batch:
            raise ValueError(f"n_frames has {len(lens)} entries for {batch} utterances")
        for L in lens:
            if not 0 < L <= cfg.canvas:
                raise ValueError(f"n_frames must be in 1..{cfg.canvas}, got {L}")
        if known is None and known_mask is not None:
            raise ValueError("known_mask without known")
        for name, lst in (("known", known), ("known_mask", known_mask)):
            if lst is not None and len(lst) != batch:
                raise ValueError(f"{name} has {len(lst)} entries for {batch} utterances")
        x = torch.zeros((batch, cfg.canvas, cfg.n_q), dtype=torch.int32)
        frame_mask = torch.zeros((batch, cfg.canvas), dtype=torch.uint8)
        kmap = torch.zeros((batch, cfg.canvas), dtype=torch.uint8)
        for b, L in enumerate(lens):
            x[b, :L] = MASK_ID
            frame_mask[b, :L] = 1
            ids = None if known is None else known[b]
            if ids is None:
                if known_mask is not None and known_mask[b] is not None:
                    raise ValueError(f"known_mask[{b}] without known[{b}]")
                continue
            ids = torch.as_tensor(ids).detach().cpu()
            if ids.is_floating_point() or ids.dtype == torch.bool or ids.dim() not in (1, 2):
                raise ValueError(f"known[{b}] must be an integer tensor [n] or [n, n_q]")
            ids = ids.long().reshape(ids.shape[0], -1)
            if ids.shape[1] != cfg.n_q:
                raise ValueError(f"known[{b}] must give all {cfg.n_q} level(s) of a frame, got {ids.shape[1]}")
            given = torch.ones(ids.shape[0], dtype=torch.bool)
            if known_mask is not None and known_mask[b] is not None:
                given = torch.as_tensor(known_mask[b]).detach().cpu().reshape(-1).bool()
                if given.shape[0] != ids.shape[0]:
                    raise ValueError(f"known_mask[{b}] has {given.shape[0]} entries for {ids.shape[0]} known frames")
            at = given.nonzero().reshape(-1)
            if at.numel() == 0:
                continue
            if int(at.max()) >= L:
                raise ValueError(f"known[{b}] gives frame {int(at.max())}, at or beyond the utterance's {L} live frames")
            vals = ids[at]
            if int(vals.min()) < 0 or int(vals.max()) > N_CLASSES - 2:
                raise ValueError(f"known[{b}] holds an id outside 0..{N_CLASSES - 2}")
            x[b, at] = vals.to(torch.int32)
            kmap[b, at] = 1
        if cfg.n_q == 1:
            x = x[:, :, 0]
        dev = self.device
        return x.contiguous().to(dev), frame_mask.to(dev), (kmap.to(dev) if bool(kmap.any()) else None)

    def _null_conditions(self, like, given, dims):
        """The null twins' texts (dims 1) or prompts (dims 2): the caller's entries, the empty condition where there is none."""
        def empty(ref):
            ref = torch.as_tensor(ref)
            return ref.new_zeros((0,)) if dims == 1 else ref.new_zeros((0,) + tuple(ref.shape[1:]) if ref.dim() == 2 else (0, self.cfg.n_levels))
        return [empty(ref) if given is None or given[b] is None else given[b] for b, ref in enumerate(like)]

    def _twin_key_lengths(self, key_lens, null_text_list, null_proms_list):
        """The key counts of B utterances -> those of the 2B of a guided call: a twin has its partner's frames; an empty null text /
        prompt keeps all of its padding as keys (it has nothing else), a caller-given one its own length."""
        cfg = self.cfg
        frames, text, prompt = (list(v) for v in key_lens)

        def lens(given, cap):
            out = []
            for b in range(len(frames)):
                n = 0 if given is None or given[b] is None else int(given[b].shape[0]) if given[b].dim() else 0
                out.append(min(n, cap) if n > 0 else cap)
            return out
        return frames + frames, text + lens(null_text_list, cfg.s_text), prompt + lens(null_proms_list, cfg.s_prompt)

    # ------------------------------------------------------------------ the hot path
    @torch.no_grad()
    def generate_audio(self, text_list, proms_list, resps_list=None, *, steps: Optional[int] = None,
                       n_frames: Union[int, Sequence[int], None] = None, seed: Optional[int] = None, greedy: bool = False,
                       utt0: int = 0, return_trace: bool = False, flags: int = 0, streams: Optional[int] = None,
                       graph: Optional[bool] = None, fp8: bool = False, global_batch: Optional[int] = None,
                       known: Optional[Sequence[Optional[Tensor]]] = None,
                       known_mask: Optional[Sequence[Optional[Tensor]]] = None, temperature: float = 1.0, top_k: int = 0,
                       top_p: float = 1.0, reveal_steps: Optional[int] = None, choice_temperature: float = 0.0,
                       mask_padding: bool = False, guidance: float = 0.0,
                       null_text_list: Optional[Sequence[Tensor]] = None, null_proms_list: Optional[Sequence[Tensor]] = None,
                       return_logprobs: bool = False, revise: Optional[float] = None):
        """Reverse diffusion for len(text_list) utterances.  Positional behaviour as upstream:
        one utterance -> int64 [canvas] (squeezed, untrimmed; rows >= n_frames are sampled from
        final.bias and meaningless); with n_q > 1 (constructor) [canvas, n_q] / [B, canvas, n_q].  `resps_list` is ignored, as
        upstream ignores it (:699).
        `n_frames` may be a sequence of B ints: utterance b then has n_frames[b] live frames and is exactly the one-utterance run
        `generate_audio([text_b], [prom_b], n_frames=n_frames[b], utt0=utt0 + b, global_batch=...)`, bit for bit.  `known` /
        `known_mask` give frames the caller already has (canvas_init_known: ids, and which of them are given; a known[b] shorter
        than the utterance with no mask is a prefix to continue): they are revealed context from the first iteration on and
        come back unchanged; every other frame draws the noise it would have drawn without them.  The result stays [B, canvas],
        untrimmed: the caller trims with its own lengths.
        `fp8=True` is the fast configuration of BASELINE.json configs[4]: the QKV, cross-attention query, fc1 and fc2
        projections run on the block-scaled fp8 matrix instruction (e4m3 codes, one power-of-two scale per 32 elements;
        d_model = 512, 16-bit model, batch * canvas a multiple of 192); the reference has no such mode.
        `global_batch`: the size of the logical batch these utterances are a shard of (vall_e/vall_e/dp.py passes it; the stream
        chunks below do too).  The attention kernels come in two instruction shapes that are picked by batch size and accumulate
        in different orders; with the global batch given, a shard takes the kernels of the unsplit batch, so the ids of an
        utterance do not depend on how the batch was split (d3pm_tuning.regime_batch).
        `temperature` (finite, > 0) and `top_k` (0 = off, else 1 .. 1025) shape how sharply every reverse step draws
        (include/d3pm_hip.h: d3pm_sampling): each row's x0-logits become rn16(rn16(l) / temperature), everything below the top_k-th
        largest of them (ties kept) becomes -inf, and the posterior draw runs on that -- inside the sampler launch, with the noise
        every class would have had anyway; the same ids as filtering the logits on the host between d3pm_denoise_step and
        d3pm_posterior_sample.  All 1025 classes take part alike; with n_q > 1 every level's logits are filtered on their own.  They
        compose with greedy, n_frames, known frames, fp8, utt0 / global_batch and stream chunks; the defaults (1, 0) run the loop
        that knows nothing of them.  Bad values are a ValueError before any GPU work.  The NAR stage keeps its own
        `sampling_temperature`.
        `top_p` (finite, 0 < top_p <= 1; 1 = off) is the nucleus cut behind them (include/d3pm_hip.h: d3pm_nucleus): of a row's
        logits after temperature and top_k, the draw keeps the smallest set of the largest ones that carries the share top_p of the
        softmax mass (measured in units of 2^-20 of the largest class's weight, ties at the threshold all kept) and sends the rest to
        -inf, per row and per step, inside the same launch.  The kept mass sits within 1.0e-3 of what the definition in exact
        arithmetic keeps; the ids are exactly those of the unfiltered sampler on logits cut at the kernel's threshold.  It composes
        with everything top_k composes with; `top_p <= 1/1280` draws what `top_k = 1` draws.
        `graph=True` replays the loop from a captured HIP graph (seed read from HBM, identical results).  Off by
        default: measured on MI355X one utterance takes 66.6 ms replayed and 66.3 ms launched eagerly -- the ~5000
        kernels of a reverse process are bound by their own ~10 us latency at M = 768 rows, not by launch overhead.  The graph cache is keyed on batch, step range, utt0 and flags, not on sampling options:
        `graph=True` with a temperature / top_k / top_p other than (1, 0, 1) raises ValueError, like the per-utterance arguments.
        `reveal_steps=N` (1 .. timesteps - 1; None = the loop above, untouched) runs the confidence-ordered reveal schedule instead
        (include/d3pm_hip.h: d3pm_reveal): N denoiser evaluations at timesteps spread over timesteps - 1 .. 1, each followed by a step
        that reveals the masked frames the model is most sure of -- as many as leave the share cbar[next timestep] of the utterance's
        free frames masked -- with the candidate id drawn by Gumbel-max from the x0-logits (mask class excluded; temperature / top_k /
        top_p apply to them as above; greedy takes the argmax).  `choice_temperature` (>= 0, default 0) adds Gumbel noise, annealed
        with cbar, to the confidence that orders the frames.  Known frames come back unchanged and frames beyond n_frames stay 0:
        they are NOT sampled from final.bias as on the default path.  It composes with n_frames sequences, known / known_mask,
        temperature / top_k / top_p, greedy, utt0 / global_batch, streams and return_trace (the trace then has N entries);
        with `steps`, graph=True, fp8=True or an n_q > 1 model it raises ValueError before any GPU work.  No statement about audio
        quality is made for it.
        `mask_padding=True` (default False: upstream's behaviour, untouched) keeps an utterance from attending to its own padding
        (include/d3pm_hip.h: d3pm_keys): the keys of every DiT self-attention are its n_frames[b] live frames, the keys of the text /
        prompt cross-attention and of the text / prompt encoder are its min(len(text_b), s_text) phonemes / min(rows(prom_b),
        s_prompt) prompt frames; a masked key has probability exactly 0.  Padded rows stay queries and are sampled as ever, so the
        result keeps its shape.  No padded row is then a key of a live one: the live rows are what the model computes at canvas =
        n_frames[b], s_text = len(text_b), s_prompt = rows(prom_b), within accumulation order (1e-3 of the oracle in fp32; bit for
        bit only on the generic kernels: the MFMA kernels tile by the padded counts and padded query rows share waves with live
        ones, so the last bits, and with them an occasional id, can still differ between two paddings).  It composes with
        n_frames sequences, known / known_mask, temperature / top_k / top_p, reveal_steps, greedy, utt0 / global_batch, streams,
        return_trace and n_q > 1; an empty text or prompt, graph=True and fp8=True raise ValueError before any GPU work.  The
        synthetic and the upstream weights were trained with the padding as keys: no statement about audio quality is made for it.
        Weights for this mode come from the training step with the same mask, forward_backward(mask_padding=True) (forward takes
        it too, for the evaluation-only loss).
        `guidance=w` (finite, >= 0; 0 = the loop above, untouched) is classifier-free guidance (include/d3pm_hip.h: d3pm_guidance):
        every reverse step evaluates the denoiser for 2B utterances in one evaluation -- each utterance and its null twin, which has
        the same canvas but no phonemes and no prompt frames (the empty text and prompt, zero padded like any other) -- and the
        sampler launch draws from rn16(fmaf(w, cond - null, cond)) of the two logit rows, with everything else (temperature / top_k /
        top_p, posterior, noise) as without it.  `null_text_list` / `null_proms_list` (B entries each; None = the empty one) give
        a caller-chosen "negative" condition per utterance instead.  The result, the trace and the noise keys stay those of B
        utterances.  It composes with n_frames sequences, known / known_mask, temperature / top_k / top_p, greedy, utt0 /
        global_batch (counted in logical utterances), streams (a chunk carries its twins), return_trace, steps and mask_padding
        (the default null twin keeps all of its padding as keys: it has nothing else; a caller-given null keeps its own lengths;
        its frames are its partner's); with graph=True, fp8=True, reveal_steps or an n_q > 1 model it raises ValueError before any
        GPU work, as do a negative, non-finite or bool weight and null lists without guidance or of the wrong length.  Guidance
        is meaningful for weights trained with the conditions dropped some of the time (forward_backward(cond_drop=...)); no
        statement about audio quality is made for the synthetic or the upstream weights.
        `return_logprobs=True` (default False: the loops above, untouched) also returns how sure the model was of every frame it
        revealed (include/d3pm_hip.h: d3pm_frame_scores): the result becomes (ids, scores), or (ids, trace, scores) with return_trace,
        where scores is the named pair FrameScores(logprob float32, step int32), [B, canvas] each and squeezed like ids for one
        utterance.  step is -1 for a frame that was padding, known or already an id when the loop started, else the timestep of the
        evaluation that revealed the frame (0: still masked); logprob is the model's log-probability of the id the frame took in
        that iteration among the codec ids -- log-softmax of that evaluation's logits (under guidance: of the guided logits) with the
        mask class removed, and WITHOUT temperature / top_k / top_p, so the number compares across sampling options and is always
        finite; 0.0 where step < 1.  On the default path a revealed frame is still redrawn every iteration and may, rarely, change
        later: logprob belongs to the id taken at `step`.  One short launch more per iteration; the ids are bit for bit those of
        the call without it.  It composes with everything the two loops compose with -- n_frames, known / known_mask, temperature /
        top_k / top_p, greedy, mask_padding, guidance, fp8, steps, reveal_steps, utt0 / global_batch and streams; a value that is
        not a bool, graph=True or an n_q > 1 model raise ValueError before any GPU work.  To regenerate the least sure frames call
        again with known = ids and known_mask = logprob >= threshold.
        `revise=bonus` (a finite number >= 0; None = the reveal loop above, untouched) lets later steps of the reveal schedule re-mask
        frames the model has come to doubt (include/d3pm_hip.h: d3pm_revise).  In every step the free frames that already hold an id
        compete again for their place: such a frame's score is the model's log-probability of its id on THIS evaluation's logits
        (as return_logprobs defines it: mask class removed, no temperature / top_k / top_p, always finite) plus `bonus`, plus the
        same order noise a masked frame gets; masked frames are scored as before, bit for bit.  After the step that is followed by
        timestep t' an utterance with F free frames holds F - floor(F * cbar[t']) ids on them, the frames that come first in the
        order among ALL free frames; a held frame that does not is re-masked and may be revealed again later, with another id.
        bonus = 0 lets held and masked frames compete on equal terms; a bonus larger than any |log-probability| pins every held
        frame.  With return_logprobs, step / logprob describe the LAST time a frame left the mask.  It needs reveal_steps (ValueError
        before any GPU work without it, as for a bool, a negative or a non-finite value) and composes with everything reveal_steps
        composes with: n_frames sequences, known / known_mask, temperature / top_k / top_p, choice_temperature, greedy,
        mask_padding, utt0 / global_batch, streams, return_trace and return_logprobs.  No statement about audio quality is made
        for it."""
        if len(text_list) != len(proms_list) or len(text_list) == 0:
            raise ValueError("text_list and proms_list must be non-empty and of equal length")
        B = len(text_list)
        if not isinstance(return_logprobs, bool):
            raise ValueError(f"return_logprobs must be a bool, got {return_logprobs!r}")
        if return_logprobs:
            for name, bad in (("graph=True", bool(graph)), ("an n_q > 1 model", self.cfg.n_q > 1)):
                if bad:
                    raise ValueError(f"return_logprobs does not combine with {name}")
        guided = _hip.guidance_options(guidance) is not None      # host validation before any GPU work
        if not guided and (null_text_list is not None or null_proms_list is not None):
            raise ValueError("null_text_list / null_proms_list without guidance")
        if guided:
            for name, bad in (("graph=True", bool(graph)), ("fp8=True", bool(fp8)), ("reveal_steps", reveal_steps is not None),
                              ("an n_q > 1 model", self.cfg.n_q > 1)):
                if bad:
                    raise ValueError(f"guidance does not combine with {name}")
            for name, lst in (("null_text_list", null_text_list), ("null_proms_list", null_proms_list)):
                if lst is not None and len(lst) != B:
                    raise ValueError(f"{name} has {len(lst)} entries for {B} utterances")
        key_lens = None
        if mask_padding:
            for name, bad in (("graph=True", bool(graph)), ("fp8=True", bool(fp8))):
                if bad:
                    raise ValueError(f"mask_padding does not combine with {name}")
            key_lens = self.key_lengths(text_list, proms_list, n_frames)      # host validation before any GPU work
        filtered = _hip.nucleus_options(temperature, top_k, top_p, N_CLASSES) is not None      # host validation before any GPU work
        if filtered and graph:
            raise ValueError("graph=True replays a loop captured per (batch, step range, utt0, flags): temperature / top_k / top_p run "
                             "on the eager loop only")
        rv = _hip.reveal_options(reveal_steps, choice_temperature, self.timesteps)
        if rv is not None:
            for name, bad in (("steps", steps is not None), ("graph=True", bool(graph)), ("fp8=True", bool(fp8)), ("an n_q > 1 model", self.cfg.n_q > 1)):
                if bad:
                    raise ValueError(f"reveal_steps does not combine with {name}")
        if _hip.revise_options(revise) is not None and rv is None:      # host validation before any GPU work
            raise ValueError("revise needs reveal_steps: it is an option of the reveal schedule")
        per_utt = known is not None or known_mask is not None or not (n_frames is None or isinstance(n_frames, Integral))
        if per_utt:
            if graph:
                raise ValueError("graph=True replays static buffers captured per (batch, step range): per-utterance n_frames / "
                                 "known frames run on the eager loop only")
            x, frame_mask, kmap = self.canvas_init_known(B, n_frames, known, known_mask)      # host validation before any GPU work
        smp = self.sampler()
        t_start = (self.timesteps - 1) if steps is None else steps
        if not 0 < t_start < smp.schedule.timesteps:
            raise ValueError(f"steps must be in 1..{smp.schedule.timesteps - 1}")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())       # follows torch.manual_seed
        n_streams = max(1, min(B, self.loop_streams if streams is None else streams))
        regime = max(int(global_batch), B) if global_batch else (B if n_streams > 1 else 0)
        if guided:
            # the null twins: utterance B + b of every evaluation.  regime_batch keeps counting logical utterances (the library doubles
            # it for the loop); the encoders run once over all 2B utterances under the doubled count
            regime = max(regime, B)
            text_list = list(text_list) + self._null_conditions(text_list, null_text_list, 1)
            proms_list = list(proms_list) + self._null_conditions(proms_list, null_proms_list, 2)
            if key_lens is not None:
                key_lens = self._twin_key_lengths(key_lens, null_text_list, null_proms_list)
        with torch.cuda.device(self.device), _hip.tuning(regime_batch=regime):
            keys = None      # d3pm_keys: (frames, text, prompt), int32 [B] on the device ([2B] under guidance)
            if key_lens is not None:
                keys = tuple(torch.tensor(v, dtype=torch.int32, device=self.device) for v in key_lens)
            if guided:      # the encoders see all 2B utterances at once, under the count the loop's evaluations run with
                with _hip.tuning(regime_batch=2 * regime):
                    cond_text, cond_prompt = self.encode_conditions(text_list, proms_list, *(keys[1:] if keys else ()))
            else:
                cond_text, cond_prompt = self.encode_conditions(text_list, proms_list, *(keys[1:] if keys else ()))

            def chunk(t, lo, hi):      # under guidance a chunk carries its twins: rows [lo, hi) and [B + lo, B + hi) of a 2B-long array
                return torch.cat([t[lo:hi], t[B + lo:B + hi]], 0) if guided else t[lo:hi]

            def chunk_keys(lo, hi):
                return None if keys is None else tuple(chunk(k, lo, hi) for k in keys)
            if not per_utt:
                x, frame_mask, kmap = self.canvas_init(B, n_frames) + (None,)
            fl = flags | (_hip.FLAG_GREEDY if greedy else 0)
            scores = smp.new_scores(B) if return_logprobs else None      # (logprob, step), [B, canvas]: a stream chunk gets its slice

            def scored(lo=0, hi=B):      # the keywords reach the loops only when asked for
                kw = {} if scores is None else {"scores": tuple(g[lo:hi] for g in scores)}
                if revise is not None:
                    kw["revise"] = revise
                return kw
            use_graph = bool(graph)
            if fp8 and (use_graph or (n_streams > 1 and not return_trace)):
                raise ValueError("fp8=True runs on the single-stream eager loop only (no graph replay, no stream chunks)")
            use_graph = use_graph and not return_trace and not _hip.profiling()
            if use_graph:
                kv_t, kv_p = smp.cond_kv(cond_text, cond_prompt)
                trace = None
                smp.sample_loop_graphed(x, frame_mask, t_start, 0, kv_t, kv_p, seed, utt0, fl)
            elif n_streams == 1 or return_trace:
                kv_t, kv_p = smp.cond_kv(cond_text, cond_prompt)
                if rv is not None:
                    trace = smp.reveal_loop(x, frame_mask, rv.n_steps, kv_t, kv_p, seed, utt0, fl, trace=return_trace, known=kmap,
                                            temperature=temperature, top_k=top_k, top_p=top_p, choice_temperature=rv.choice_temperature,
                                            keys=keys, **scored())
                else:
                    trace = smp.sample_loop(x, frame_mask, t_start, 0, kv_t, kv_p, seed, utt0, fl, trace=return_trace, fp8=fp8, known=kmap,
                                            temperature=temperature, top_k=top_k, top_p=top_p, keys=keys, guidance=guidance, **scored())
            else:
                # utterances are independent: chunks of the batch run the whole loop on their own stream so that
                # the short kernels of one chunk fill the ramp-up / epilogue bubbles of the others
                trace = None
                while len(self._streams) < n_streams:
                    self._streams.append(torch.cuda.Stream(device=self.device))
                cur = torch.cuda.current_stream()
                bounds = [(B * i) // n_streams for i in range(n_streams + 1)]
                for i in range(n_streams):
                    lo, hi = bounds[i], bounds[i + 1]
                    st = self._streams[i]
                    st.wait_stream(cur)
                    with torch.cuda.stream(st):
                        kv_t, kv_p = smp.cond_kv(chunk(cond_text, lo, hi), chunk(cond_prompt, lo, hi))
                        if rv is not None:
                            smp.reveal_loop(x[lo:hi], frame_mask[lo:hi] if per_utt else frame_mask, rv.n_steps, kv_t, kv_p, seed, utt0 + lo, fl,
                                            slot=i, known=None if kmap is None else kmap[lo:hi], temperature=temperature, top_k=top_k,
                                            top_p=top_p, choice_temperature=rv.choice_temperature, keys=chunk_keys(lo, hi), **scored(lo, hi))
                        else:
                            smp.sample_loop(x[lo:hi], frame_mask[lo:hi] if per_utt else frame_mask, t_start, 0, kv_t, kv_p, seed, utt0 + lo, fl,
                                            slot=i, known=None if kmap is None else kmap[lo:hi], temperature=temperature, top_k=top_k,
                                            top_p=top_p, keys=chunk_keys(lo, hi), guidance=guidance, **scored(lo, hi))
                        for t_ in (kv_t, kv_p, cond_text, cond_prompt, x) + (scores or ()):
                            t_.record_stream(st)
                for i in range(n_streams):
                    cur.wait_stream(self._streams[i])
        out = x.long()
        out = out[0] if B == 1 else out
        if return_logprobs:
            fs = FrameScores(*(g[0] if B == 1 else g for g in scores))
            return (out, trace, fs) if return_trace else (out, fs)
        return (out, trace) if return_trace else out

    # ------------------------------------------------------------------ upstream method names
    @torch.no_grad()
    def p_sample(self, model_logits: Tensor, t: Tensor, x: Tensor, *, seed: int = 0, utt0: int = 0, temperature: float = 1.0,
                 top_k: int = 0, top_p: float = 1.0, guidance: float = 0.0, null_logits: Optional[Tensor] = None):
        """One reverse transition from x0-logits [B,T,K] at step t[0] (ar_discrete.py:401-420).
        Returns (sample int64 [B,T], softmax(logits)) like upstream (the softmax of the logits as given: `temperature` / `top_k` /
        `top_p`, as in generate_audio, act on the draw only).  `guidance` (> 0) with `null_logits` [B,T,K], the logits of the same
        rows under the null condition, draws from rn16(fmaf(guidance, logits - null_logits, logits)) (the one-step entry of
        generate_audio(guidance=...)).  Bad values are a ValueError before any GPU work."""
        _hip.nucleus_options(temperature, top_k, top_p, N_CLASSES)
        if (_hip.guidance_options(guidance) is None) != (null_logits is None):
            raise ValueError("guidance and null_logits go together")
        smp = self.sampler()
        x_next, _ = smp.posterior_sample(model_logits, x.to(torch.int32).contiguous(), int(t.reshape(-1)[0]), seed, utt0,
                                         temperature=temperature, top_k=top_k, top_p=top_p, guidance=guidance, null_logits=null_logits)
        return x_next.long(), F.softmax(model_logits, dim=-1)

    @torch.no_grad()
    def q_sample(self, x_start: Tensor, t: Tensor, mask: Tensor, *, seed: int = 0, utt0: int = 0):
        """Forward noising q(x_t | x_0) (ar_discrete.py:467-487)."""
        smp = self.sampler()
        fm = mask.to(torch.uint8).contiguous()
        return smp.q_sample(x_start.to(torch.int32).contiguous(), fm, int(t.reshape(-1)[0]), seed, utt0).long()

    def forward_backward(self, text_list, proms_list, resps_list, *, seed: Optional[int] = None, timesteps: Optional[int] = None,
                         dropout=False, utt0: int = 0, cond_drop=0.0, mask_padding: bool = False):
        """The training step's compute (reference: `engine.backward(engine(...))`, utils/engines.py:144-147 over
        ar_discrete.py:588-694): the loss of `forward` AND its gradient for every parameter the forward reads, accumulated
        into `param.grad` by the HIP backward kernels (vall_e/vall_e/train.py; fp32 model).  Follow it with
        `train.all_reduce_gradients(self)` under torch.distributed and any torch.optim step.  Returns the loss.
        dropout=True applies the dropout the reference's condition encoders apply in train mode (p = 0.1 / 0.01,
        ar_discrete.py:216-230) from a Philox mask keyed by (seed, utterance, site); a (p_layer, p_mlp) pair sets other
        probabilities; the default False is eval-mode arithmetic (`self.training` is not consulted).  Upstream's masks come
        from torch's global generator, a stream that is not reproduced.  utt0: global index of the first utterance (a
        data-parallel rank passes its shard offset), which keys the q_sample noise and the masks.
        cond_drop: p or (p_text, p_prompt) -- the probability with which an utterance's text / prompt is replaced by the empty one
        for this step (the null condition of generate_audio(guidance=...): what classifier-free guidance needs the weights to
        have seen); decided per utterance from (seed, utt0 + b) on Philox stream 5; 0 (default) is the step without it.
        mask_padding=True trains the model generate_audio(mask_padding=True) evaluates: an utterance's padding is no key of any
        attention -- the DiT self-attention keeps its first min(len(resps_b), canvas) frames, the text / prompt cross-attention
        and the two encoders its min(len(text_b), s_text) phonemes / min(rows(prom_b), s_prompt) prompt frames; a condition that
        cond_drop replaced keeps all of its padding, as the default null twin of guidance does.  Masked keys get probability 0
        and gradient 0, padded rows stay queries; loss and gradients are those of the model at the truncated shape, scaled as
        DESIGN.md "Key masks in the training step" states.  It composes with dropout (no draw changes), cond_drop and utt0; an
        empty text or prompt, or a mask_padding that is not a bool, is a ValueError before any GPU work.  False (default) is the
        step without it, launch for launch."""
        from .train import D3PMTrainer
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        loss, _ = D3PMTrainer(self).forward_backward(text_list, proms_list, resps_list, seed=seed, timesteps=timesteps, dropout=dropout,
                                                     utt0=utt0, cond_drop=cond_drop, mask_padding=mask_padding)
        return loss

    @torch.no_grad()
    def forward(self, text_list, proms_list, resps_list=None, spkr_name=None, *, seed: Optional[int] = None, mask_padding: bool = False):
        """Training-side forward, evaluation only (forward half; ar_discrete.py:588-694): for every
        utterance, x_0 = the target codes zero-padded / truncated to the canvas, mask = (x_0 != 0), and
            loss = sum_{t=1}^{timesteps-1} mean_canvas CE(final(blocks(q_sample(x_0, t))) * mask, x_0 * mask) / mask.sum().
        Sets `self.loss` (mean over the utterances; upstream indexes `[0]` throughout, so for one utterance this is its
        value) and returns the masked logits of the last step of the last utterance, `[canvas, n_classes]`, as upstream.
        q_sample draws Philox stream 1 keyed by `seed` instead of torch.rand.  No autograd graph is built: gradients come from
        `forward_backward` (hand-written backward kernels), not from torch.autograd.
        mask_padding=True evaluates the loss forward_backward(mask_padding=True) trains (in every dtype forward runs in): the keys
        of every attention are the utterance's own frames, phonemes and prompt frames (train.key_mask_lengths; d3pm_keys), padded
        rows stay queries and the returned logits keep their shape.  An empty text or prompt is a ValueError before any GPU work."""
        if resps_list is None or not (len(text_list) == len(proms_list) == len(resps_list)) or len(text_list) == 0:
            raise ValueError("text_list, proms_list and resps_list must be non-empty and of equal length")
        from .train import key_mask_lengths
        key_lens = key_mask_lengths(self.cfg, text_list, proms_list, resps_list, mask_padding=mask_padding)      # host validation first
        smp = self.sampler()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        losses, last = [], None
        with torch.cuda.device(self.device):
            for b, (text, prom, resps) in enumerate(zip(text_list, proms_list, resps_list)):
                r = resps.reshape(-1).to(self.device).long()[: self.cfg.canvas]
                x0 = F.pad(r, (0, self.cfg.canvas - r.shape[0])).to(torch.int32)[None].contiguous()
                frame_mask = (x0[0] != 0).to(torch.uint8)
                keys = None      # (frames, text, prompt) of this utterance, int32 [1] on the device
                if key_lens is not None:
                    keys = tuple(torch.tensor([v[b]], dtype=torch.int32, device=self.device) for v in key_lens)
                cond_text, cond_prompt = self.encode_conditions([text], [prom], *(keys[1:] if keys else ()))
                kv_t, kv_p = smp.cond_kv(cond_text, cond_prompt)
                loss, logits = smp.training_forward(x0, frame_mask, kv_t, kv_p, seed, utt0=b, timesteps=self.timesteps, keys=keys)
                losses.append(loss[0])
                last = logits[0]
        self.loss = torch.stack(losses).mean()
        return last

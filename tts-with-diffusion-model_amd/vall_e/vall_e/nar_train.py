"""Training step of the stock NAR model on MI355X: the loss of the training branch of `NAR.forward` and the gradient of every
parameter, from hand-written HIP kernels.

Reference: the reference's vall_e/vall_e/nar.py:53-74 (one quantizer level l_b per utterance; levels 0 .. l_b of the response go in,
level l_b + 1 is the target) and base.py:403-488 (`[text | sep | prompt | sep | response]` assembly :427-435, AdaLN blocks :136-234,
classifier :440, cross-entropy over the response rows :445-488), differentiated by torch autograd inside `engine.backward`.

Here: `NARTrainer` replays that forward op by op through the C ABI on fp32 tensors (d3pm_op_nar_embed, d3pm_op_adaln, the generic
family of d3pm_op_linear, d3pm_op_attention_keylen) with a stash per block, and walks the stash backwards through the kernels of
csrc/d3pm_train.hip (`linear_bwd`, `act_bwd`, `attention_bwd(..., key_len=total)`, `mask_rows`) and the three of
csrc/d3pm_nar_train.hip (`adaln_bwd`, `nar_embed_bwd`, `nar_ce`).  Gradients accumulate in fp32 into `param.grad` of EVERY parameter
of the module (all of them are read), which is what torch.optim and `train.all_reduce_gradients` consume.

The utterances of a call run one after the other, each on its own grid of total_b = t_text + t_prompt + t_b + 2 rows (no padding),
with its own level: the AdaLN row and the number of summed response levels are per utterance.  The loss is the mean over all
response frames of the call, so utterance b enters with the weight t_b / N and the result does not depend on how a batch is cut
beyond the order of the sums.

Level: l_b = min(6, int(float32(u) * float32(7))) with u the first uniform of the Philox key (seed; group 0, row utt0 + b, t 0,
stream 6) drawn through d3pm_uniform -- a function of (seed, utt0 + b) alone, so data-parallel ranks agree with one process over the
whole batch (upstream draws torch.randint(0, 7, (B,)) from the global generator); `quant_levels=[...]` overrides it.

AdaLN detach: upstream's AdaLN is y = exp(log_gamma) * (c (1 - (k h).detach()) h) + beta (base.py:154); the detach is part of the
model and `adaln_bwd` treats f = c (1 - k h) as a constant.

Dropout: off by default (eval arithmetic, the way `AR.forward_backward` started).  `dropout=True` is upstream's p = 0.1 at its three
sites per block -- on the attention branch after `to_out(...) * m` (kind 0), after the GELU (kind 1), on the FFN branch after
`block.3` (kind 2) -- and `dropout=p` another probability in [0, 1).  The masks come from the stream of the condition encoders'
dropout (d3pm_op_dropout_f32), keyed by (seed, utt0 + b, site) with site = (2 << 8) | (layer << 4) | kind and indexed by the row
inside the utterance times the width plus the column, so they do not depend on the batch; the backward pass regenerates them.
"""
from __future__ import annotations

import ctypes as C
import numbers
from typing import Optional, Sequence

import torch

from . import _hip
from . import train as T

LEVEL_STREAM = 6          # Philox stream of the level draw (0 .. 5 and 16 .. 23 are taken: DESIGN.md section 7)
DROPOUT_TRAIN = 0.1       # p_dropout of the reference's NAR (base.py:320)
DROPOUT_WHICH = 2         # the `which` field of the NAR's dropout sites (0 / 1 are the D3PM stage's two condition encoders)
N_LEVELS = 7              # levels 0 .. 6 can be drawn (nar.py:56)

_ptr = T._ptr


def dropout_prob(dropout) -> float:
    """The `dropout` argument -> p: False / None -> 0, True -> the reference's 0.1, a number in [0, 1) -> itself."""
    if dropout is None or dropout is False:
        return 0.0
    if dropout is True:
        return DROPOUT_TRAIN
    if not isinstance(dropout, numbers.Real) or not 0.0 <= float(dropout) < 1.0:
        raise ValueError(f"dropout: expected True / False or a probability in [0, 1), got {dropout!r}")
    return float(dropout)


def dropout_site(layer: int, kind: int) -> int:
    """Site number in the mask stream: kind 0 attention branch after to_out(...) * m, 1 after the GELU, 2 FFN branch after block.3."""
    return (DROPOUT_WHICH << 8) | (layer << 4) | kind


def validate(text_list, proms_list, resps_list, *, quant_levels=None, dropout=False, n_layers=1, width=N_LEVELS + 1) -> float:
    """Host validation of a training call, before any GPU work; returns the dropout probability.  ValueError: lists of unequal
    length or empty, a response that is not `width` levels wide, an empty response (upstream raises there too, base.py:446),
    quant_levels of the wrong length or outside 0 .. 6, a dropout outside [0, 1), dropout with more than 16 layers (the site
    number has four bits for the layer)."""
    B = len(resps_list)
    if B == 0 or not (len(text_list) == len(proms_list) == B):
        raise ValueError(f"expected as many texts and prompts as responses and at least one: {len(text_list)} texts, "
                         f"{len(proms_list)} prompts, {B} responses")
    for b, r in enumerate(resps_list):
        if r.dim() != 2 or r.shape[-1] != width:
            raise ValueError(f"the training step takes responses of {width} levels [t, {width}], utterance {b} has shape {tuple(r.shape)}")
        if r.shape[0] == 0:
            raise ValueError("Cannot compute loss given empty targ_list.")
    if quant_levels is not None:
        levels = [int(l) for l in quant_levels]
        if len(levels) != B or not all(0 <= l < N_LEVELS for l in levels):
            raise ValueError(f"quant_levels: expected {B} levels within 0 .. {N_LEVELS - 1}, got {list(quant_levels)!r}")
    p = dropout_prob(dropout)
    if p > 0.0 and n_layers > 16:
        raise ValueError(f"dropout: the mask stream numbers at most 16 layers, the model has {n_layers}")
    return p


def draw_levels(seed: int, utt0: int, batch: int, device) -> list:
    """l_b = min(6, int(float32(u) * float32(7))), u = word 0 of Philox key (seed; group 0, row utt0 + b, t 0, stream 6)."""
    u = _hip.uniform(T._seed(seed), 0, int(utt0), batch, 4, LEVEL_STREAM, device)[:, 0].cpu()
    return (u * torch.tensor(float(N_LEVELS), dtype=torch.float32)).to(torch.int64).clamp(max=N_LEVELS - 1).tolist()


def adaln_bwd(x, dy, emb_row, row_mask, dx, demb_row, accumulate=True):
    """d3pm_op_adaln_bwd_f32: x / dy / dx [M, d] dense, emb_row / demb_row [2 d] (demb_row accumulated into), row_mask uint8 [M]."""
    M, d = x.shape
    for t_, n_ in ((x, "x"), (dy, "dy"), (dx, "dx"), (emb_row, "emb_row"), (demb_row, "demb_row")):
        if not T._f32(t_, n_).is_contiguous():
            raise _hip.D3PMError(f"adaln_bwd: {n_} must be contiguous")
    assert dy.shape == x.shape == dx.shape and emb_row.numel() == 2 * d == demb_row.numel() and row_mask.numel() == M
    _hip.check(_hip.lib().d3pm_op_adaln_bwd_f32(_ptr(x), _ptr(dy), _ptr(emb_row), _ptr(row_mask), M, d, _ptr(dx), 1 if accumulate else 0,
                                                _ptr(demb_row), _hip.stream_ptr()), "d3pm_op_adaln_bwd_f32")


def nar_embed_bwd(lens, text, prom, resp, n_given, dx, d_text, d_prom, d_resp, d_sep):
    """d3pm_op_nar_embed_bwd_f32: the grids of _hip.op_nar_embed, dx [B, t_max, d]; the four table gradients are accumulated into."""
    B, t_max, d = dx.shape
    for t_, n_ in ((dx, "dx"), (d_text, "d_text"), (d_prom, "d_prom"), (d_resp, "d_resp"), (d_sep, "d_sep")):
        if not T._f32(t_, n_).is_contiguous():
            raise _hip.D3PMError(f"nar_embed_bwd: {n_} must be contiguous")
    n_tokens = d_text.shape[0]
    assert d_text.shape == (n_tokens, d) and d_prom.shape == (prom.shape[2], n_tokens, d) and d_resp.shape[0] >= n_given and \
        d_resp.shape[1:] == (n_tokens, d) and d_sep.shape == (d,) and lens.shape == (B, 3)
    _hip.check(_hip.lib().d3pm_op_nar_embed_bwd_f32(_ptr(lens), _ptr(text), text.shape[1], _ptr(prom), prom.shape[1], prom.shape[2], _ptr(resp),
                                                    resp.shape[1], resp.shape[2], int(n_given), _ptr(dx), _ptr(d_text), _ptr(d_prom),
                                                    _ptr(d_resp), _ptr(d_sep), B, t_max, d, n_tokens, _hip.stream_ptr()),
               "d3pm_op_nar_embed_bwd_f32")


def nar_ce(logits, lens, resp, levels, gscale, want_grad=True):
    """d3pm_op_nar_ce_f32: logits [B, t_max, K] (dense), lens int32 [B, 3], resp int32 [B, tr_max, stride], levels int32 [B] on the
    device -> (row_loss [B, t_max], dlogits [B, t_max, K] = (softmax - onehot) * gscale on the response rows and 0 elsewhere, or None)."""
    B, t_max, K = logits.shape
    if not T._f32(logits, "logits").is_contiguous():
        raise _hip.D3PMError("nar_ce: logits must be contiguous")
    assert lens.shape == (B, 3) and levels.shape == (B,) and levels.dtype == torch.int32 and resp.dim() == 3
    row_loss = torch.empty((B, t_max), dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits) if want_grad else None
    _hip.check(_hip.lib().d3pm_op_nar_ce_f32(_ptr(logits), K, _ptr(lens), _ptr(resp), resp.shape[1], resp.shape[2], _ptr(levels), B, t_max, K,
                                             float(gscale), _ptr(row_loss), _ptr(dlogits), K, _hip.stream_ptr()), "d3pm_op_nar_ce_f32")
    return row_loss, dlogits


class NARTrainer:
    """Loss + gradients of the training branch of NAR.forward for a model in fp32 on a HIP device."""

    def __init__(self, model):
        if model.dtype != torch.float32 or model.device.type != "cuda":
            raise _hip.D3PMError("NAR training runs in fp32 on a HIP device: model.float().to('cuda')")
        self.model = model
        self._pe = None

    def _pe_table(self, rows: int) -> torch.Tensor:
        if self._pe is None or self._pe.shape[0] < rows or self._pe.device != self.model.device:
            from .nar import _sinusoid_table
            self._pe = _sinusoid_table(max(2048, rows), self.model.cfg.d_model, torch.float32).to(self.model.device).contiguous()
        return self._pe

    # ---- one utterance: forward with a stash -----------------------------------------------------------------
    def _forward(self, grids, t_max, level, drop):
        """grids = (lens [1, 3], text, prom, resp) of one utterance; drop = (p, seed, utt).  -> (logits [t_max, K], stash)."""
        m, cfg = self.model, self.model.cfg
        lens, text, prom, resp = grids
        p, seed, utt = drop
        d, H, n = cfg.d_model, cfg.n_heads, t_max
        scale = (1.0 / (d // H)) ** 0.5
        G = _hip.FAMILY_GENERIC
        lin = lambda x, w, b, **kw: _hip.op_linear(x, w, b, family=G, **kw)
        x, mask, key_len = _hip.op_nar_embed(lens, text, prom, resp, level + 1, m.text_emb.weight, m.proms_emb.weight, m.resps_emb.weight,
                                             m.sep, self._pe_table(t_max), t_max)
        x, mask = x.view(n, d), mask.view(n)
        blocks = []
        for i, blk in enumerate(m.blocks):
            att, ffn = blk.attn.block, blk.ffn.block
            s = {"x": x}
            # x1 = (x + dropout(to_out(attention(AdaLN_a(x) * m)) * m)) * m
            s["ha"] = _hip.op_adaln(x, blk.attn.norm.emb.weight[level], mask)
            s["qkv"] = lin(s["ha"], att.to_qkv.weight, None)
            qkv = s["qkv"].view(1, n, 3 * d)
            s["att"] = _hip.op_attention(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], H, scale, family=G, key_len=key_len).view(n, d)
            if p > 0:
                o = lin(s["att"], att.to_out.weight, att.to_out.bias, row_mask=mask, mask_period=n)
                x1 = T.dropout(o, p, seed, utt, dropout_site(i, 0), residual=x)
            else:
                x1 = lin(s["att"], att.to_out.weight, att.to_out.bias, r1=x, row_mask=mask, mask_period=n)
            s["x1"] = x1
            # x = (x1 + dropout(block.3(dropout(gelu(block.0(AdaLN_f(x1) * m)))))) * m
            s["hf"] = _hip.op_adaln(x1, blk.ffn.norm.emb.weight[level], mask)
            s["u"] = lin(s["hf"], ffn[0].weight, ffn[0].bias)
            s["g"] = lin(s["hf"], ffn[0].weight, ffn[0].bias, act=T.GELU)
            if p > 0:
                T.dropout(s["g"], p, seed, utt, dropout_site(i, 1), out=s["g"])      # the stash keeps the dropped hidden: block.3's input
                o = lin(s["g"], ffn[3].weight, ffn[3].bias, row_mask=mask, mask_period=n)
                x = T.dropout(o, p, seed, utt, dropout_site(i, 2), residual=x1)
            else:
                x = lin(s["g"], ffn[3].weight, ffn[3].bias, r1=x1, row_mask=mask, mask_period=n)
            blocks.append(s)
        logits = lin(x, m.classifier.weight, m.classifier.bias, row_mask=mask, mask_period=n)
        return logits, {"x_last": x, "mask": mask, "key_len": key_len, "blocks": blocks}

    # ---- one utterance: the walk back ------------------------------------------------------------------------
    def _backward(self, grids, t_max, level, drop, stash, dlogits, padded):
        m, cfg = self.model, self.model.cfg
        lens, text, prom, resp = grids
        p, seed, utt = drop
        d, H, n = cfg.d_model, cfg.n_heads, t_max
        scale = (1.0 / (d // H)) ** 0.5
        mask, key_len = stash["mask"], stash["key_len"]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dlogits.device)
        g = T._grad
        dx = new(n, d)
        T.linear_bwd(stash["x_last"], m.classifier.weight, dlogits, g(m.classifier.weight), g(m.classifier.bias), dx)
        for i in reversed(range(len(m.blocks))):
            blk, s = m.blocks[i], stash["blocks"][i]
            att, ffn = blk.attn.block, blk.ffn.block
            if padded:
                T.mask_rows(dx, mask)                                          # x = (...) * m at the end of the block
            # ---- x = x1 + dropout2(block.3(dropout1(gelu(block.0(hf)))))
            do = T.dropout(dx, p, seed, utt, dropout_site(i, 2)) if p > 0 else dx      # a copy: dx goes on as the residual's gradient
            dg = new(n, 4 * d)
            T.linear_bwd(s["g"], ffn[3].weight, do, g(ffn[3].weight), g(ffn[3].bias), dg)
            if p > 0:
                T.dropout(dg, p, seed, utt, dropout_site(i, 1), out=dg)
            du = T.act_bwd(s["u"], dg, T.GELU)
            dh = new(n, d)
            T.linear_bwd(s["hf"], ffn[0].weight, du, g(ffn[0].weight), g(ffn[0].bias), dh)
            adaln_bwd(s["x1"], dh, blk.ffn.norm.emb.weight[level], mask, dx, g(blk.ffn.norm.emb.weight)[level])
            if padded:
                T.mask_rows(dx, mask)                                          # x1 = (...) * m
            # ---- x1 = x + dropout0(to_out(attention(qkv(ha))) * m)
            do = T.dropout(dx, p, seed, utt, dropout_site(i, 0)) if p > 0 else dx
            datt = new(n, d)
            T.linear_bwd(s["att"], att.to_out.weight, do, g(att.to_out.weight), g(att.to_out.bias), datt)
            qkv, dqkv = s["qkv"].view(1, n, 3 * d), new(1, n, 3 * d)
            T.attention_bwd(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], datt.view(1, n, d), dqkv[..., :d], dqkv[..., d:2 * d],
                            dqkv[..., 2 * d:], H, scale, key_len=key_len)
            T.linear_bwd(s["ha"], att.to_qkv.weight, dqkv.view(n, 3 * d), g(att.to_qkv.weight), None, dh)
            adaln_bwd(s["x"], dh, blk.attn.norm.emb.weight[level], mask, dx, g(blk.attn.norm.emb.weight)[level])
        nar_embed_bwd(lens, text, prom, resp, level + 1, dx.view(1, n, d), g(m.text_emb.weight), g(m.proms_emb.weight),
                      g(m.resps_emb.weight), g(m.sep))

    @torch.no_grad()
    def step(self, text_list: Sequence[torch.Tensor], proms_list: Sequence[torch.Tensor], resps_list: Sequence[torch.Tensor], *,
             seed: Optional[int] = None, utt0: int = 0, quant_levels=None, dropout=False, backward: bool = True, pad_rows: int = 0):
        """nll = sum over the response frames of the call of CE(classifier(x)[row], resps[b][f][l_b + 1]) / N, N = sum_b t_b; with
        backward=True its gradient is added to `param.grad` of every parameter (fp32; created as zeros where missing).
        pad_rows: extra padding rows behind every utterance's total (they are neither keys nor producers of gradient; the result is
        the same).  Returns (loss fp32 scalar tensor, levels list)."""
        m = self.model
        p = validate(text_list, proms_list, resps_list, quant_levels=quant_levels, dropout=dropout, n_layers=m.cfg.n_layers)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        B = len(resps_list)
        n_frames = sum(int(r.shape[0]) for r in resps_list)
        with torch.cuda.device(m.device):
            levels = [int(l) for l in quant_levels] if quant_levels is not None else draw_levels(seed, utt0, B, m.device)
            if backward:
                for prm in m.parameters():
                    T._grad(prm)
            total = torch.zeros((), dtype=torch.float32, device=m.device)
            for b in range(B):
                lens, text, prom, resp, _, lens_host = m._pack([text_list[b]], [proms_list[b]], [resps_list[b]])
                t_max = sum(lens_host[0]) + 2 + int(pad_rows)
                grids, drop = (lens, text, prom, resp), (p, seed, utt0 + b)
                logits, stash = self._forward(grids, t_max, levels[b], drop)
                level_t = torch.tensor([levels[b]], dtype=torch.int32, device=m.device)
                row_loss, dlogits = nar_ce(logits.view(1, t_max, -1), lens, resp, level_t, 1.0 / n_frames, want_grad=backward)
                total += row_loss.sum()
                if backward:
                    self._backward(grids, t_max, levels[b], drop, stash, dlogits.view(t_max, -1), pad_rows > 0)
        return total / n_frames, levels

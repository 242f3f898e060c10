"""Training step of the D3PM model on MI355X: loss AND parameter gradients of `AR.forward` from hand-written HIP kernels,
plus the data-parallel gradient all-reduce.

Reference: the training forward /root/reference/vall_e/vall_e/ar_discrete.py:588-694 (for t = 1 .. timesteps-1: q_sample ->
DiT blocks :126-161 -> final Linear :776 -> masked cross-entropy :683-690, summed over t and divided by mask.sum()), its
gradient by torch autograd inside `engine.backward`, and DeepSpeed's data-parallel all-reduce of the gradients
(/root/reference/vall_e/utils/engines.py:144-147; /root/reference/vall_e/train.py:29-31 initialises the NCCL group).

Here: `forward_backward` replays the forward op by op through the C ABI with a stash of every op input, then walks the stash
backwards through the `d3pm_op_*_bwd_f32` kernels (csrc/d3pm_train.hip); gradients are accumulated into `param.grad`
(fp32), exactly what an optimizer from torch.optim consumes.  `all_reduce_gradients` is one bucketed all-reduce over
`torch.distributed` (backend "nccl" = RCCL over xGMI on the GPU box; "gloo" in the CPU tests).

Scope: the F32 precision mode (fp32 weights and activations).  Gradients flow into every parameter the denoiser forward
reads -- the DiT blocks (cross_attn2 and token_emb are dead upstream and stay gradient-free), `final`, `resps_emb`, `time_emb`
via `timestep_fc` -- and, through the cached cross-attention K / V, into the two condition encoders (ar_discrete.py:216-230:
two post-norm TransformerEncoder layers + a SiLU Mlp each) and their embeddings `text_emb` (padding row 0 excluded, as
nn.Embedding(padding_idx=0) does) and `proms_emb`.

Dropout: by default the step is the eval-mode forward (`model.eval()`), which is how the gradient fixtures were generated
(tests/golden/make_golden.py gen_grads).  The reference trains with dropout active inside both condition encoders
(ar_discrete.py:216-230): p = 0.1 at the four sites of each TransformerEncoderLayer (attention probabilities, after the
self-attention out_proj, the FFN hidden after the ReLU, after linear2) and drop = 0.01 at the two of its Mlp (after the SiLU,
after fc2); the DiT blocks have dropout 0 (:109,123).  `forward_backward(dropout=True)` applies those six sites, and
`dropout=(p_layer, p_mlp)` other probabilities.  The masks come from a counter-based Philox stream keyed by (seed, utterance,
site) (include/d3pm_hip.h, DESIGN.md "Dropout mask stream"), drawn once per utterance per call as upstream's encoders run once
per forward, and regenerated in the backward pass rather than stored.  Upstream draws them from torch's global generator; that
stream itself is not reproduced.  The argument is explicit on purpose: `model.training` is not consulted (a freshly built
nn.Module is in train mode, and honouring the flag would change what every existing caller computes).

Key masks: `forward_backward(mask_padding=True)` trains the model `generate_audio(mask_padding=True)` evaluates -- the keys of every
attention of the step are the utterance's own frames, phonemes and prompt frames (`key_mask_lengths`, host arithmetic), through the
masked forward ops and the masked backward kernels (`attn_bwd_q_rows` / `attn_bwd_kv_rows` with the KEYS arm).  A masked key has
probability 0 and gradient 0, padded rows stay queries, and the dropout stream keeps its padded indexing; the step equals the model
at the truncated shape (DESIGN.md "Key masks in the training step").  The default False is the step without it, launch for launch.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from . import _hip

GELU, RELU, SILU = 1, 2, 3


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(t: torch.Tensor, name: str):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise _hip.D3PMError(f"{name}: the training ops take fp32 device tensors")
    return t


def matmul(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, *, ta=False, tb=False, beta=0.0, row_mask=None, period=1):
    """out[M, N] = beta * out + op(a) @ op(b) through d3pm_op_matmul_f32 (2-D fp32 views, any strides)."""
    for t_, n_ in ((a, "a"), (b, "b"), (out, "out")):
        _f32(t_, n_)
    A = a.t() if ta else a
    Bm = b.t() if tb else b
    M, K = A.shape
    K2, N = Bm.shape
    assert K == K2 and tuple(out.shape) == (M, N) and out.stride(1) == 1
    _hip.check(_hip.lib().d3pm_op_matmul_f32(_ptr(A), A.stride(0), A.stride(1), _ptr(Bm), Bm.stride(0), Bm.stride(1), _ptr(out),
                                             out.stride(0), M, N, K, float(beta), _ptr(row_mask), period, _hip.stream_ptr()),
               "d3pm_op_matmul_f32")
    return out


def colsum(x: torch.Tensor, out: torch.Tensor, beta=1.0):
    assert x.stride(1) == 1 and out.numel() == x.shape[1]
    _hip.check(_hip.lib().d3pm_op_colsum_f32(_ptr(_f32(x, "x")), x.stride(0), x.shape[0], x.shape[1], _ptr(_f32(out, "out")), float(beta),
                                             _hip.stream_ptr()), "d3pm_op_colsum_f32")


def linear_bwd(x, w, dy, dw, db, dx=None, dx_beta=0.0):
    """y = x @ w.T + b:  dw += dy.T @ x, db += colsum(dy), dx = dx_beta * dx + dy @ w."""
    matmul(dy, x, dw, ta=True, beta=1.0)
    if db is not None:
        colsum(dy, db, 1.0)
    if dx is not None:
        matmul(dy, w, dx, beta=dx_beta)
    return dx


def act_bwd(u, dm, act=GELU):
    du = torch.empty_like(u)
    _hip.check(_hip.lib().d3pm_op_act_bwd_f32(_ptr(_f32(u, "u")), _ptr(_f32(dm, "dm")), _ptr(du), u.numel(), act, _hip.stream_ptr()),
               "d3pm_op_act_bwd_f32")
    return du


def mask_rows(x, mask):
    _hip.check(_hip.lib().d3pm_op_mask_rows_f32(_ptr(_f32(x, "x")), x.stride(0), x.shape[0], x.shape[1], _ptr(mask), mask.numel(),
                                                _hip.stream_ptr()), "d3pm_op_mask_rows_f32")


def layernorm_bwd(x, dout, w, b, dx, dw, db, film=None, dfilm=None, eps=1e-6, accumulate=True):
    M, d = x.shape
    _hip.check(_hip.lib().d3pm_op_layernorm_bwd_f32(_ptr(_f32(x, "x")), _ptr(_f32(dout, "dout")), _ptr(w), _ptr(b), _ptr(film), float(eps), M,
                                                    d, _ptr(_f32(dx, "dx")), 1 if accumulate else 0, _ptr(dw), _ptr(db), _ptr(dfilm),
                                                    _hip.stream_ptr()), "d3pm_op_layernorm_bwd_f32")


def _key_len(key_len, B, device):
    if key_len.dtype != torch.int32 or key_len.shape != (B,) or key_len.device != device or not key_len.is_contiguous():
        raise _hip.D3PMError(f"key_len must be a contiguous int32 [{B}] tensor on {device}")
    return key_len


def attention_bwd(q, k, v, do, dq, dk, dv, n_heads, scale, beta_kv=0.0, drop=None, key_len=None):
    """q [B,Tq,d], k / v [B,S,d] views (row strides free), do [B,Tq,d]; dq / dk / dv views of the same shapes.  drop = (p, seed,
    utt0, site): the backward pass of attention_dropout with those arguments.  key_len (int32 [B] on the device, 1 .. S, or None):
    the backward pass of the masked forward (d3pm_op_attention_bwd_keylen_f32) -- keys behind key_len[b] are not read and their
    dk / dv rows receive 0 (beta_kv * old); None launches the entries without it."""
    B, Tq, d = q.shape
    S = k.shape[1]
    hd = d // n_heads
    stats = torch.empty(B * n_heads * Tq * 2, dtype=torch.float32, device=q.device)
    assert k.stride(1) == v.stride(1) and dk.stride(1) == dv.stride(1)
    if key_len is not None:
        p, seed, utt0, site = (0.0, 0, 0, 0) if drop is None else drop
        _hip.check(_hip.lib().d3pm_op_attention_bwd_keylen_f32(
            _ptr(_f32(q, "q")), q.stride(1), _ptr(_f32(k, "k")), _ptr(_f32(v, "v")), k.stride(1), _ptr(_f32(do, "do")), do.stride(1), _ptr(dq),
            dq.stride(1), _ptr(dk), _ptr(dv), dk.stride(1), _ptr(stats), B, Tq, S, n_heads, hd, float(scale), float(beta_kv),
            _ptr(_key_len(key_len, B, q.device)), float(p), _seed(seed), utt0, site, _hip.stream_ptr()), "d3pm_op_attention_bwd_keylen_f32")
        return
    if drop is not None:
        p, seed, utt0, site = drop
        _hip.check(_hip.lib().d3pm_op_attention_bwd_dropout_f32(
            _ptr(_f32(q, "q")), q.stride(1), _ptr(_f32(k, "k")), _ptr(_f32(v, "v")), k.stride(1), _ptr(_f32(do, "do")), do.stride(1), _ptr(dq),
            dq.stride(1), _ptr(dk), _ptr(dv), dk.stride(1), _ptr(stats), B, Tq, S, n_heads, hd, float(scale), float(beta_kv), float(p),
            _seed(seed), utt0, site, _hip.stream_ptr()), "d3pm_op_attention_bwd_dropout_f32")
        return
    _hip.check(_hip.lib().d3pm_op_attention_bwd_f32(_ptr(q), q.stride(1), _ptr(k), _ptr(v), k.stride(1), _ptr(do), do.stride(1), _ptr(dq),
                                                    dq.stride(1), _ptr(dk), _ptr(dv), dk.stride(1), _ptr(stats), B, Tq, S, n_heads, hd,
                                                    float(scale), float(beta_kv), _hip.stream_ptr()), "d3pm_op_attention_bwd_f32")


def attention_dropout(q, k, v, n_heads, scale, p, seed, utt0, site, key_len=None):
    """softmax(scale q k^T) with probability dropout, times v (d3pm_op_attention_dropout_f32): q [B,Tq,d], k / v [B,S,d] views
    (row strides free); utterance b draws its mask with utt0 + b.  key_len (int32 [B] on the device, 1 .. S, or None): keys behind
    key_len[b] are outside the softmax and draw nothing, every other key keeps its draw (d3pm_op_attention_dropout_keylen_f32).
    -> [B,Tq,d]."""
    B, Tq, d = q.shape
    S = k.shape[1]
    assert k.stride(1) == v.stride(1) and q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    assert q.stride(0) == Tq * q.stride(1) and k.stride(0) == S * k.stride(1) and v.stride(0) == S * v.stride(1)
    o = torch.empty((B, Tq, d), dtype=torch.float32, device=q.device)
    if key_len is not None:
        _hip.check(_hip.lib().d3pm_op_attention_dropout_keylen_f32(
            _ptr(_f32(q, "q")), q.stride(1), _ptr(_f32(k, "k")), _ptr(_f32(v, "v")), k.stride(1), _ptr(o), d, B, Tq, S, n_heads,
            d // n_heads, float(scale), _ptr(_key_len(key_len, B, q.device)), float(p), _seed(seed), utt0, site, _hip.stream_ptr()),
            "d3pm_op_attention_dropout_keylen_f32")
        return o
    _hip.check(_hip.lib().d3pm_op_attention_dropout_f32(_ptr(_f32(q, "q")), q.stride(1), _ptr(_f32(k, "k")), _ptr(_f32(v, "v")), k.stride(1),
                                                        _ptr(o), d, B, Tq, S, n_heads, d // n_heads, float(scale), float(p), _seed(seed),
                                                        utt0, site, _hip.stream_ptr()), "d3pm_op_attention_dropout_f32")
    return o


def dropout(x, p, seed, utt, site, *, residual=None, out=None):
    """out = (residual +) x * z over the 2-D view x (d3pm_op_dropout_f32; row strides free, `out=x` works in place), z the
    mask factor of (seed, utt, site) at each logical index r * cols + c.  Also the backward pass of the site, on the gradient."""
    M, N = x.shape
    y = torch.empty((M, N), dtype=torch.float32, device=x.device) if out is None else out
    for t_ in (x, y) + (() if residual is None else (residual,)):
        assert t_.stride(1) == 1 and tuple(t_.shape) == (M, N)
    _hip.check(_hip.lib().d3pm_op_dropout_f32(_ptr(_f32(x, "x")), x.stride(0), _ptr(residual), 0 if residual is None else residual.stride(0),
                                              _ptr(_f32(y, "out")), y.stride(0), M, N, float(p), _seed(seed), utt, site, _hip.stream_ptr()),
               "d3pm_op_dropout_f32")
    return y


def _seed(seed: int) -> int:
    return int(seed) & 0xFFFFFFFFFFFFFFFF


DROPOUT_TRAIN = (0.1, 0.01)      # (p_layer, p_mlp): nn.TransformerEncoderLayer's default and the Mlp's drop (ar_discrete.py:216-230)
MLP_LAYER = 15                   # the `layer` field of the Mlp's two sites


def dropout_probs(dropout) -> tuple:
    """The `dropout` argument of forward_backward -> (p_layer, p_mlp): False / None -> (0, 0), True -> the reference's
    (0.1, 0.01), a pair of numbers -> itself.  Each p must lie in [0, 1); anything else raises ValueError."""
    if dropout is None or dropout is False:
        return 0.0, 0.0
    if dropout is True:
        return DROPOUT_TRAIN
    if not isinstance(dropout, (tuple, list)) or len(dropout) != 2 or \
            not all(isinstance(p, numbers.Real) and not isinstance(p, bool) for p in dropout):
        raise ValueError(f"dropout: expected True / False or a (p_layer, p_mlp) pair of numbers, got {dropout!r}")
    p_layer, p_mlp = float(dropout[0]), float(dropout[1])
    for p in (p_layer, p_mlp):
        if not 0.0 <= p < 1.0:
            raise ValueError(f"dropout: every probability must lie in [0, 1), got {dropout!r}")
    return p_layer, p_mlp


COND_DROP_STREAM = 5      # Philox stream of the condition-drop decision (0..4 and 16..23 are taken: DESIGN.md section 7)


def cond_drop_probs(cond_drop) -> tuple:
    """The `cond_drop` argument of forward_backward -> (p_text, p_prompt): False / None / 0 -> (0, 0), a number p -> (p, p), a
    (p_text, p_prompt) pair -> itself.  Every probability lies in [0, 1] (1 = always dropped)."""
    if cond_drop is None or cond_drop is False:
        return 0.0, 0.0
    if isinstance(cond_drop, numbers.Real) and not isinstance(cond_drop, bool):
        pair = (cond_drop, cond_drop)
    elif isinstance(cond_drop, (tuple, list)) and len(cond_drop) == 2 and \
            all(isinstance(p, numbers.Real) and not isinstance(p, bool) for p in cond_drop):
        pair = tuple(cond_drop)
    else:
        raise ValueError(f"cond_drop: expected a probability or a (p_text, p_prompt) pair of numbers, got {cond_drop!r}")
    p_text, p_prompt = float(pair[0]), float(pair[1])
    for p in (p_text, p_prompt):
        if not (math.isfinite(p) and 0.0 <= p <= 1.0):
            raise ValueError(f"cond_drop: every probability must lie in [0, 1], got {cond_drop!r}")
    return p_text, p_prompt


def cond_drop_decision(seed: int, utt: int, p_text: float, p_prompt: float, device) -> tuple:
    """(drop text?, drop prompt?) of global utterance `utt`: u = words 0 and 1 of Philox key (seed; group 0, row utt, t 0, stream 5)
    drawn through d3pm_uniform; a condition is dropped <=> u < p (fp32 u in [0, 1) against the fp32 probability).  A function of
    (seed, utt) alone, so data-parallel ranks agree with one process over the whole batch.  p = 0 draws nothing."""
    if p_text == 0.0 and p_prompt == 0.0:
        return False, False
    u = _hip.uniform(_seed(seed), 0, int(utt), 1, 4, COND_DROP_STREAM, device)[0].cpu()
    return bool(u[0] < torch.tensor(p_text, dtype=torch.float32)), bool(u[1] < torch.tensor(p_prompt, dtype=torch.float32))


def key_mask_lengths(cfg, text_list, proms_list, resps_list, dropped=None, mask_padding=True):
    """Host side of `mask_padding` in the training step (no GPU work): the key counts of every utterance as three lists of ints,
    (frames, text, prompt) with frames[b] = min(len(resps_b), canvas) -- counted by length, a code 0 inside the utterance stays a
    key --, text[b] = min(len(text_b), s_text) and prompt[b] = min(rows(prom_b), s_prompt): the numbers of _hip.key_lengths.
    dropped (or None): per utterance the (text dropped?, prompt dropped?) pair of cond_drop_decision -- a dropped condition keeps
    all of its padding as keys (s_text / s_prompt), the rule AR._twin_key_lengths applies to the default null twin of guidance.
    mask_padding=False returns None.  ValueError: a mask_padding that is not a bool, lists of different lengths, an utterance
    without a frame, a phoneme or a prompt frame (what the caller passes: validation comes before the drop)."""
    if not isinstance(mask_padding, bool):
        raise ValueError(f"mask_padding must be a bool, got {mask_padding!r}")
    if not mask_padding:
        return None
    B = len(text_list)
    if not (B == len(proms_list) == len(resps_list)) or (dropped is not None and len(dropped) != B):
        raise ValueError(f"mask_padding: {B} texts, {len(proms_list)} prompts, {len(resps_list)} targets"
                         + ("" if dropped is None else f", {len(dropped)} drop decisions"))

    def rows(t):
        return int(t.shape[0]) if t.dim() else 0
    frames, text, prompt = _hip.key_lengths([min(int(r.numel()), cfg.canvas) for r in resps_list], [rows(t) for t in text_list],
                                            [rows(p) for p in proms_list], cfg.canvas, cfg.s_text, cfg.s_prompt)
    for b, (drop_text, drop_prompt) in enumerate(dropped or ()):
        if drop_text:
            text[b] = cfg.s_text
        if drop_prompt:
            prompt[b] = cfg.s_prompt
    return frames, text, prompt


def dropout_site(which: int, layer: int, kind: int) -> int:
    """Site number of the mask stream: which 0 text / 1 prompt encoder; layer 0 .. cond_layers - 1 with kind 0 attention
    probabilities, 1 after out_proj, 2 FFN hidden, 3 after linear2; layer MLP_LAYER with kind 0 after SiLU, 1 after fc2."""
    return (which << 8) | (layer << 4) | kind


def ce_bwd(logits, targets, frame_mask, gscale):
    rows, K = logits.shape
    out = torch.empty_like(logits)
    _hip.check(_hip.lib().d3pm_op_ce_bwd_f32(_ptr(_f32(logits, "logits")), logits.stride(0), _ptr(targets), _ptr(frame_mask),
                                             frame_mask.numel(), rows, K, float(gscale), _ptr(out), out.stride(0), _hip.stream_ptr()),
               "d3pm_op_ce_bwd_f32")
    return out


def embed(tok, mask, table):
    rows, d = tok.numel(), table.shape[1]
    y = torch.empty((rows, d), dtype=torch.float32, device=table.device)
    _hip.check(_hip.lib().d3pm_op_embed_f32(_ptr(tok), _ptr(mask), 0 if mask is None else mask.numel(), _ptr(_f32(table, "table")), _ptr(y),
                                            rows, d, table.shape[0], _hip.stream_ptr()), "d3pm_op_embed_f32")
    return y


def embed_bwd(tok, mask, dy, dtable, padding_idx=0):
    _hip.check(_hip.lib().d3pm_op_embed_bwd_f32(_ptr(tok), _ptr(mask), 0 if mask is None else mask.numel(), _ptr(_f32(dy, "dy")),
                                                _ptr(_f32(dtable, "dtable")), tok.numel(), dy.shape[1], dtable.shape[0], padding_idx,
                                                _hip.stream_ptr()), "d3pm_op_embed_bwd_f32")


def _grad(p: torch.nn.Parameter) -> torch.Tensor:
    if p.grad is None:
        p.grad = torch.zeros_like(p, dtype=torch.float32)
    return p.grad


class D3PMTrainer:
    """Loss + gradients of AR.forward for a model in fp32 on a HIP device."""

    def __init__(self, model):
        if model.dtype != torch.float32 or model.device.type != "cuda":
            raise _hip.D3PMError("training runs in the F32 precision mode on a HIP device: model.float().to('cuda')")
        self.model = model

    # ---- condition encoders (once per utterance) with a stash ------------------------------------------------
    def _encode(self, which, tokens, drop=(0.0, 0.0, 0, 0), key_len=None):
        """which 0: text int32 [S_t]; 1: prompt int32 [S_p, n_levels] -> (cond [S, d], stash).  drop = (p_layer, p_mlp, seed,
        utt): the six dropout sites (module docstring); a site with p = 0 is the eval-mode op.  The stash keeps the dropped
        tensors that the weight gradients read (linear2's and fc2's inputs).  key_len (int32 [1] on the device, or None): the rows
        that are keys of the encoder's self-attention (mask_padding); every row stays a query."""
        p_layer, p_mlp, seed, utt = drop
        m, cfg = self.model, self.model.cfg
        d = cfg.d_model
        G = _hip.FAMILY_GENERIC
        lin = lambda x, w, b, **kw: _hip.op_linear(x, w, b, family=G, **kw)
        pe_text0, pe_prompt = m._pe()
        enc = m.encodertext if which == 0 else m.encoder2
        rows = tokens.shape[0]
        x = torch.empty((rows, d), dtype=torch.float32, device=m.device)
        table = m.text_emb.weight if which == 0 else m.proms_emb.weight
        pe = pe_text0 if which == 0 else pe_prompt
        _hip.check(_hip.lib().d3pm_op_cond_embed(_hip.F32, which, _ptr(tokens), cfg.n_levels, _ptr(table), _ptr(pe.contiguous()), _ptr(x), rows,
                                                 cfg.s_prompt, d, cfg.n_classes, _hip.stream_ptr()), "d3pm_op_cond_embed")
        H = cfg.cond_heads
        scale = (1.0 / (d // H)) ** 0.5
        layers = []
        for l, layer in enumerate(enc[0].layers):
            s = {"x": x}
            s["qkv"] = lin(x, layer.self_attn.in_proj_weight, layer.self_attn.in_proj_bias)
            qkv = s["qkv"].view(1, rows, 3 * d)
            q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
            if p_layer > 0:                 # t1 = x + dropout1(out_proj(attention with dropped probabilities))
                s["att"] = attention_dropout(q, k, v, H, scale, p_layer, seed, utt, dropout_site(which, l, 0), key_len=key_len).view(rows, d)
                s["t1"] = dropout(lin(s["att"], layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias), p_layer, seed, utt,
                                  dropout_site(which, l, 1), residual=x)
            else:
                s["att"] = _hip.op_attention(q, k, v, H, scale, family=G, key_len=key_len).view(rows, d)
                s["t1"] = lin(s["att"], layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias, r1=x)
            s["x1"] = _hip.op_layernorm(s["t1"], layer.norm1.weight, layer.norm1.bias, eps=1e-5)
            s["ff"] = lin(s["x1"], layer.linear1.weight, layer.linear1.bias, act=RELU)
            if p_layer > 0:                 # t2 = x1 + dropout2(linear2(dropout(relu(linear1(x1)))))
                dropout(s["ff"], p_layer, seed, utt, dropout_site(which, l, 2), out=s["ff"])
                s["t2"] = dropout(lin(s["ff"], layer.linear2.weight, layer.linear2.bias), p_layer, seed, utt, dropout_site(which, l, 3),
                                  residual=s["x1"])
            else:
                s["t2"] = lin(s["ff"], layer.linear2.weight, layer.linear2.bias, r1=s["x1"])
            x = _hip.op_layernorm(s["t2"], layer.norm2.weight, layer.norm2.bias, eps=1e-5)
            layers.append(s)
        mlp = enc[1]
        top = {"x": x, "u": lin(x, mlp.fc1.weight, mlp.fc1.bias), "h": lin(x, mlp.fc1.weight, mlp.fc1.bias, act=SILU)}
        if p_mlp > 0:                       # drop1 after the SiLU
            dropout(top["h"], p_mlp, seed, utt, dropout_site(which, MLP_LAYER, 0), out=top["h"])
        cond = lin(top["h"], mlp.fc2.weight, mlp.fc2.bias)
        if p_mlp > 0:                       # drop2 after fc2
            dropout(cond, p_mlp, seed, utt, dropout_site(which, MLP_LAYER, 1), out=cond)
        return cond, {"which": which, "tokens": tokens, "layers": layers, "top": top, "drop": drop, "key_len": key_len}

    def _encode_backward(self, stash, dcond):
        m, cfg = self.model, self.model.cfg
        d, H = cfg.d_model, cfg.cond_heads
        scale = (1.0 / (d // H)) ** 0.5
        which, tokens, top = stash["which"], stash["tokens"], stash["top"]
        enc = m.encodertext if which == 0 else m.encoder2
        rows = tokens.shape[0]
        dev = dcond.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        p_layer, p_mlp, seed, utt = stash["drop"]
        mlp = enc[1]
        if p_mlp > 0:                                            # drop2 (a copy: the caller keeps dcond)
            dcond = dropout(dcond, p_mlp, seed, utt, dropout_site(which, MLP_LAYER, 1))
        dh = new(rows, top["h"].shape[1])
        linear_bwd(top["h"], mlp.fc2.weight, dcond, _grad(mlp.fc2.weight), _grad(mlp.fc2.bias), dh)
        if p_mlp > 0:                                            # drop1
            dropout(dh, p_mlp, seed, utt, dropout_site(which, MLP_LAYER, 0), out=dh)
        du = act_bwd(top["u"], dh, SILU)
        dx = new(rows, d)
        linear_bwd(top["x"], mlp.fc1.weight, du, _grad(mlp.fc1.weight), _grad(mlp.fc1.bias), dx)
        for l, layer, s in reversed([(l, layer, s) for l, (layer, s) in enumerate(zip(enc[0].layers, stash["layers"]))]):
            dt2 = new(rows, d)                                   # x = LN(t2; norm2), t2 = x1 + linear2(relu(linear1(x1)))
            layernorm_bwd(s["t2"], dx, layer.norm2.weight, layer.norm2.bias, dt2, _grad(layer.norm2.weight), _grad(layer.norm2.bias),
                          eps=1e-5, accumulate=False)
            # dropout2 (a copy: dt2 goes on to collect the residual branch's gradient)
            dl2 = dropout(dt2, p_layer, seed, utt, dropout_site(which, l, 3)) if p_layer > 0 else dt2
            dff = new(rows, s["ff"].shape[1])
            linear_bwd(s["ff"], layer.linear2.weight, dl2, _grad(layer.linear2.weight), _grad(layer.linear2.bias), dff)
            if p_layer > 0:                                      # dropout on the FFN hidden
                dropout(dff, p_layer, seed, utt, dropout_site(which, l, 2), out=dff)
            # relu'(u) = [u > 0] = [relu(u) > 0]; with dropout s["ff"] is the dropped hidden, which keeps the sign where kept,
            # and dff is already 0 where dropped
            dpre = act_bwd(s["ff"], dff, RELU)
            linear_bwd(s["x1"], layer.linear1.weight, dpre, _grad(layer.linear1.weight), _grad(layer.linear1.bias), dt2, dx_beta=1.0)
            dt1 = new(rows, d)                                   # x1 = LN(t1; norm1), t1 = x + out_proj(attention)
            layernorm_bwd(s["t1"], dt2, layer.norm1.weight, layer.norm1.bias, dt1, _grad(layer.norm1.weight), _grad(layer.norm1.bias),
                          eps=1e-5, accumulate=False)
            do = dropout(dt1, p_layer, seed, utt, dropout_site(which, l, 1)) if p_layer > 0 else dt1     # dropout1 (a copy)
            datt = new(rows, d)
            linear_bwd(s["att"], layer.self_attn.out_proj.weight, do, _grad(layer.self_attn.out_proj.weight),
                       _grad(layer.self_attn.out_proj.bias), datt)
            qkv, dqkv = s["qkv"].view(1, rows, 3 * d), new(1, rows, 3 * d)
            attention_bwd(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], datt.view(1, rows, d), dqkv[..., :d], dqkv[..., d:2 * d],
                          dqkv[..., 2 * d:], H, scale, drop=(p_layer, seed, utt, dropout_site(which, l, 0)) if p_layer > 0 else None,
                          key_len=stash["key_len"])
            dx = dt1                                             # residual branch; the in-projection adds its part
            linear_bwd(s["x"], layer.self_attn.in_proj_weight, dqkv.view(rows, 3 * d), _grad(layer.self_attn.in_proj_weight),
                       _grad(layer.self_attn.in_proj_bias), dx, dx_beta=1.0)
        if which == 0:
            embed_bwd(tokens, None, dx, _grad(m.text_emb.weight), padding_idx=0)
        else:
            gp = _grad(m.proms_emb.weight)
            for lvl in range(tokens.shape[1]):
                embed_bwd(tokens[:, lvl].contiguous(), None, dx, gp[lvl], padding_idx=-1)

    # ---- one denoiser evaluation with a stash ---------------------------------------------------------------
    def _forward(self, x_t, fm, t, kv_t, kv_p, film, keys=(None, None, None)):
        """keys: the (frames, text, prompt) key counts of mask_padding, int32 [1] on the device each (None = that attention has every
        padded row as a key, the step without the mask)."""
        k_frames, k_text, k_prompt = keys
        m, cfg = self.model, self.model.cfg
        d, H = cfg.d_model, cfg.n_heads
        scale = (1.0 / (d // H)) ** 0.5
        G = _hip.FAMILY_GENERIC
        lin = lambda x, w, b, **kw: _hip.op_linear(x, w, b, family=G, **kw)
        x = embed(x_t.reshape(-1), fm, m.resps_emb.weight)
        stash = []
        for l, blk in enumerate(m.blocks):
            s = {"xin": x}
            s["h1"] = _hip.op_layernorm(x, blk.norm1.weight, blk.norm1.bias)
            s["qkv"] = lin(s["h1"], blk.attn.in_proj_weight, blk.attn.in_proj_bias)
            qkv = s["qkv"].view(1, -1, 3 * d)
            s["att"] = _hip.op_attention(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], H, scale, family=G, key_len=k_frames).view(-1, d)
            s["x1"] = lin(s["att"], blk.attn.out_proj.weight, blk.attn.out_proj.bias, r1=x)
            s["h2"] = _hip.op_layernorm(s["x1"], blk.norm2.weight, blk.norm2.bias)
            s["h22"] = _hip.op_layernorm(s["x1"], blk.norm22.weight, blk.norm22.bias)
            wq, bq = blk.cross_attn.in_proj_weight[:d], blk.cross_attn.in_proj_bias[:d]
            s["qt"], s["qp"] = lin(s["h2"], wq, bq), lin(s["h22"], wq, bq)
            s["at"] = _hip.op_attention(s["qt"].view(1, -1, d), kv_t[l][..., :d], kv_t[l][..., d:], H, scale, family=G,
                                        key_len=k_text).view(-1, d)
            s["ap"] = _hip.op_attention(s["qp"].view(1, -1, d), kv_p[l][..., :d], kv_p[l][..., d:], H, scale, family=G,
                                        key_len=k_prompt).view(-1, d)
            wo, bo = blk.cross_attn.out_proj.weight, blk.cross_attn.out_proj.bias
            ot = lin(s["at"], wo, bo)
            s["x2"] = lin(s["ap"], wo, bo, r1=s["x1"], r2=ot)
            s["film"] = film[t, l].contiguous()
            s["h3"] = _hip.op_layernorm(s["x2"], blk.norm3.weight, blk.norm3.bias, film=s["film"])
            s["u"] = lin(s["h3"], blk.mlp.fc1.weight, blk.mlp.fc1.bias)
            s["g"] = lin(s["h3"], blk.mlp.fc1.weight, blk.mlp.fc1.bias, act=GELU)
            x = lin(s["g"], blk.mlp.fc2.weight, blk.mlp.fc2.bias, r1=s["x2"], row_mask=fm, mask_period=fm.numel())
            stash.append(s)
        logits = lin(x, m.final.weight, m.final.bias)
        return x, logits, stash

    def _backward(self, x_t, fm, t, kv_t, kv_p, cond_t, cond_p, dcond_t, dcond_p, x_last, logits, stash, targets, gscale,
                  keys=(None, None, None)):
        k_frames, k_text, k_prompt = keys
        m, cfg = self.model, self.model.cfg
        d, H = cfg.d_model, cfg.n_heads
        scale = (1.0 / (d // H)) ** 0.5
        n = x_last.shape[0]
        dev = x_last.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        dlogits = ce_bwd(logits, targets, fm, gscale)
        dx = new(n, d)
        linear_bwd(x_last, m.final.weight, dlogits, _grad(m.final.weight), _grad(m.final.bias), dx)
        temb = m.time_emb.weight[t:t + 1]
        for l in reversed(range(len(m.blocks))):
            blk, s = m.blocks[l], stash[l]
            mask_rows(dx, fm)                                                     # x = (...) * mask at the end of the block
            # ---- x3 = x2 + fc2(gelu(fc1(LN3 + FiLM)))
            dg = new(n, 4 * d)
            linear_bwd(s["g"], blk.mlp.fc2.weight, dx, _grad(blk.mlp.fc2.weight), _grad(blk.mlp.fc2.bias), dg)
            du = act_bwd(s["u"], dg, GELU)
            dh3 = new(n, d)
            linear_bwd(s["h3"], blk.mlp.fc1.weight, du, _grad(blk.mlp.fc1.weight), _grad(blk.mlp.fc1.bias), dh3)
            dfilm = torch.zeros(2 * d, dtype=torch.float32, device=dev)
            layernorm_bwd(s["x2"], dh3, blk.norm3.weight, blk.norm3.bias, dx, _grad(blk.norm3.weight), _grad(blk.norm3.bias),
                          film=s["film"], dfilm=dfilm)
            # film = timestep_fc(time_emb[t])
            dfilm2 = dfilm.view(1, 2 * d)
            linear_bwd(temb, blk.timestep_fc.weight, dfilm2, _grad(blk.timestep_fc.weight), _grad(blk.timestep_fc.bias),
                       _grad(m.time_emb.weight)[t:t + 1], dx_beta=1.0)
            # ---- x2 = x1 + out(at) + out(ap), both through cross_attn.out_proj
            wo = blk.cross_attn.out_proj.weight
            gwo, gbo = _grad(wo), _grad(blk.cross_attn.out_proj.bias)
            dat, dap = new(n, d), new(n, d)
            linear_bwd(s["at"], wo, dx, gwo, gbo, dat)
            linear_bwd(s["ap"], wo, dx, gwo, gbo, dap)
            gin_w, gin_b = _grad(blk.cross_attn.in_proj_weight), _grad(blk.cross_attn.in_proj_bias)
            wq, wkv = blk.cross_attn.in_proj_weight[:d], blk.cross_attn.in_proj_weight[d:]
            for q_name, h_name, datt, kv, cond, dcond, norm, k_len in (("qt", "h2", dat, kv_t[l], cond_t, dcond_t, blk.norm2, k_text),
                                                                      ("qp", "h22", dap, kv_p[l], cond_p, dcond_p, blk.norm22, k_prompt)):
                S = kv.shape[1]
                dq, dkv = new(1, n, d), new(1, S, 2 * d)
                attention_bwd(s[q_name].view(1, n, d), kv[..., :d], kv[..., d:], datt.view(1, n, d), dq, dkv[..., :d], dkv[..., d:], H, scale,
                              key_len=k_len)
                dq2, dkv2 = dq.view(n, d), dkv.view(S, 2 * d)
                dh = new(n, d)
                linear_bwd(s[h_name], wq, dq2, gin_w[:d], gin_b[:d], dh)
                linear_bwd(cond, wkv, dkv2, gin_w[d:], gin_b[d:], dcond, dx_beta=1.0)
                layernorm_bwd(s["x1"], dh, norm.weight, norm.bias, dx, _grad(norm.weight), _grad(norm.bias))
            # ---- x1 = xin + attn.out_proj(self-attention(LN1))
            datt = new(n, d)
            linear_bwd(s["att"], blk.attn.out_proj.weight, dx, _grad(blk.attn.out_proj.weight), _grad(blk.attn.out_proj.bias), datt)
            qkv, dqkv = s["qkv"].view(1, n, 3 * d), new(1, n, 3 * d)
            attention_bwd(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], datt.view(1, n, d), dqkv[..., :d], dqkv[..., d:2 * d],
                          dqkv[..., 2 * d:], H, scale, key_len=k_frames)
            dh1 = new(n, d)
            linear_bwd(s["h1"], blk.attn.in_proj_weight, dqkv.view(n, 3 * d), _grad(blk.attn.in_proj_weight), _grad(blk.attn.in_proj_bias), dh1)
            layernorm_bwd(s["xin"], dh1, blk.norm1.weight, blk.norm1.bias, dx, _grad(blk.norm1.weight), _grad(blk.norm1.bias))
            mask_rows(dx, fm)                                                     # x * mask at the start of the block
        embed_bwd(x_t.reshape(-1), fm, dx, _grad(m.resps_emb.weight), padding_idx=0)

    @torch.no_grad()
    def forward_backward(self, text_list: Sequence[torch.Tensor], proms_list: Sequence[torch.Tensor], resps_list: Sequence[torch.Tensor],
                         *, seed: int = 0, timesteps: Optional[int] = None, dropout=False, utt0: int = 0, cond_drop=0.0,
                         mask_padding: bool = False):
        """The loss of AR.forward (mean over the utterances) and its gradient, accumulated into `param.grad`.
        cond_drop: p or (p_text, p_prompt) -- per utterance the text and / or the prompt is replaced by the empty one (no phonemes /
        no prompt frames, zero padded like any other: the null condition of generate_audio(guidance=...)) with that probability;
        a replaced condition still flows through its encoder, whose gradients accumulate as ever.  The decision is a function of
        (seed, utt0 + b) (cond_drop_decision); 0 / False (default) is the step without it, bit for bit.
        dropout: False (default) = eval-mode arithmetic; True = the reference's train-mode condition encoders (p 0.1 in the
        encoder layers, 0.01 in the Mlp); a (p_layer, p_mlp) pair = those probabilities (dropout_probs; module docstring).
        utt0: global index of this call's first utterance -- utterance b keys its q_sample noise and its dropout masks with
        utt0 + b, so data-parallel ranks that pass their shard offset draw what one process over the whole batch would.
        mask_padding: True keeps an utterance from attending to its own padding, as generate_audio(mask_padding=True) does: the keys
        of every DiT self-attention are its first min(len(resps_b), canvas) frames, those of the text / prompt cross-attention and
        of the two encoders' self-attention its min(len(text_b), s_text) phonemes / min(rows(prom_b), s_prompt) prompt frames
        (key_mask_lengths); a text or prompt that cond_drop replaced keeps all of its padding as keys, the rule of the null twin
        of guidance.  A masked key has probability 0 and receives no gradient; padded rows stay queries.  The step is then the
        model at the truncated shape: loss = (L / C) loss' + (T - 1) (C - L) ln(K) / (C L'), every gradient (L / C) times that
        model's (DESIGN.md "Key masks in the training step").  An empty text or prompt is a ValueError before any GPU work.
        False (default) is the step without it: the same launches.
        Returns (loss fp32 scalar tensor, [(dcond_text, dcond_prompt)] per utterance)."""
        p_layer, p_mlp = dropout_probs(dropout)
        p_text, p_prompt = cond_drop_probs(cond_drop)
        masked = key_mask_lengths(self.model.cfg, text_list, proms_list, resps_list, mask_padding=mask_padding) is not None
        m, cfg = self.model, self.model.cfg
        smp = m.sampler()
        T = m.timesteps if timesteps is None else int(timesteps)
        B = len(text_list)
        losses, dconds = [], []
        with torch.cuda.device(m.device):
            for b, (text, prom, resps) in enumerate(zip(text_list, proms_list, resps_list)):
                r = resps.reshape(-1).to(m.device).long()[: cfg.canvas]
                x0 = F.pad(r, (0, cfg.canvas - r.shape[0])).to(torch.int32)[None].contiguous()
                fm = (x0[0] != 0).to(torch.uint8)
                n_live = int(fm.sum().item())
                targets = (x0[0] * fm.to(torch.int32)).contiguous()
                drop_text, drop_prompt = cond_drop_decision(seed, utt0 + b, p_text, p_prompt, m.device)
                keys = (None, None, None)
                if masked:      # one-element int32 tensors: the ops of this utterance run with B = 1
                    lens = key_mask_lengths(cfg, [text], [prom], [resps], dropped=[(drop_text, drop_prompt)])
                    keys = tuple(torch.tensor(v, dtype=torch.int32, device=m.device) for v in lens)
                if drop_text:
                    text = text[:0]
                if drop_prompt:
                    prom = prom[:0]
                text_p, prom_p = m._padded_inputs([text], [prom])
                prom_p = prom_p[0].to(torch.int32)
                if prom_p.shape[-1] < cfg.n_levels:
                    prom_p = F.pad(prom_p, (0, cfg.n_levels - prom_p.shape[-1]), value=-1)
                drop = (p_layer, p_mlp, seed, utt0 + b)
                cond_t2, st_t = self._encode(0, text_p[0].to(torch.int32).contiguous(), drop, keys[1])
                cond_p2, st_p = self._encode(1, prom_p.contiguous(), drop, keys[2])
                kv_t, kv_p = smp.cond_kv(cond_t2[None], cond_p2[None])
                dcond_t, dcond_p = torch.zeros_like(cond_t2), torch.zeros_like(cond_p2)
                gscale = 1.0 / (cfg.canvas * max(n_live, 1) * B)
                total = torch.zeros((), dtype=torch.float32, device=m.device)
                for t in range(1, T):
                    x_t = smp.q_sample(x0, fm, t, seed, utt0 + b)
                    x_last, logits, stash = self._forward(x_t, fm, t, kv_t, kv_p, smp.film, keys)
                    total += smp.ce_loss_rows(logits.view(1, cfg.canvas, cfg.n_classes), targets.view(1, -1), fm).mean()
                    self._backward(x_t, fm, t, kv_t, kv_p, cond_t2, cond_p2, dcond_t, dcond_p, x_last, logits, stash, targets, gscale, keys)
                self._encode_backward(st_t, dcond_t)
                self._encode_backward(st_p, dcond_p)
                losses.append(total / max(n_live, 1))
                dconds.append((dcond_t, dcond_p))
        loss = torch.stack(losses).mean()
        m.loss = loss
        return loss, dconds


def all_reduce_gradients(model, *, bucket_bytes: int = 64 << 20, average: bool = True):
    """Data-parallel gradient reduction (the reference: DeepSpeed inside engine.backward / step, utils/engines.py:144-147):
    every parameter's .grad summed over the ranks of the default process group in buckets of <= `bucket_bytes` -- one flat
    buffer per bucket, one all-reduce each (backend "nccl" = RCCL over xGMI; ring all-reduce is per-link bound, so a few
    large messages instead of one per tensor) -- then divided by the world size.  A parameter that has a gradient on some
    rank but not on this one contributes zeros, so all ranks issue identical collectives; a parameter without a gradient
    on EVERY rank (upstream's dead `cross_attn2` / `token_emb` tensors) is left out and keeps `.grad = None`, exactly as at
    world size 1 -- otherwise weight decay would touch it in data-parallel runs only (one small MAX all-reduce of the
    has-gradient bitmask decides that).  `model` is any nn.Module: the NAR after `NAR.forward_backward` works the same way (every
    parameter of it has a gradient on every rank; each rank's loss is the mean over its own frames and the ranks are averaged)."""
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size() == 1:
        return 0
    world = dist.get_world_size()
    params = [p for p in model.parameters() if p.requires_grad]
    if not params:
        return 0
    has = torch.tensor([1 if p.grad is not None else 0 for p in params], dtype=torch.int32, device=params[0].device)
    dist.all_reduce(has, op=dist.ReduceOp.MAX)
    params = [p for p, h in zip(params, has.tolist()) if h]
    n_coll, i = 1, 0
    while i < len(params):
        bucket, size = [], 0
        while i < len(params) and (not bucket or size + params[i].numel() * 4 <= bucket_bytes):
            bucket.append(params[i])
            size += params[i].numel() * 4
            i += 1
        flat = torch.cat([(_grad(p) if p.grad is not None else torch.zeros_like(p, dtype=torch.float32)).reshape(-1).float()
                          for p in bucket])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        if average:
            flat /= world
        off = 0
        for p in bucket:
            k = p.numel()
            if p.grad is None:
                p.grad = torch.zeros_like(p, dtype=torch.float32)
            p.grad.copy_(flat[off:off + k].view_as(p))
            off += k
        n_coll += 1
    return n_coll

"""TEST INFRASTRUCTURE -- functional torch restatement of the stock NAR model's training step (the reference's
vall_e/vall_e/nar.py:53-74 and base.py:403-488), for autograd in fp32 or fp64 on the CPU.

Differences from oracle/nar_oracle.py:level_logits, which restates the inference branch:
  * a quantizer level per utterance: utterance b sums response levels 0 .. l_b, normalises with AdaLN row l_b and is scored
    against level l_b + 1 of its own response;
  * `adaln` keeps upstream's `(k h).detach()` (base.py:154).  nar_oracle.adaln omits it, which is harmless for inference and
    wrong for a gradient: never differentiate that one;
  * optional dropout factors injected at upstream's three sites per block (PrenormResidual.dropout of the attention branch,
    the nn.Dropout after the GELU, PrenormResidual.dropout of the FFN branch), as tensors [total_b, width] per utterance.

Pinned to the reference by tests/golden/make_nar_train_grads.py (loss and every gradient of the reference's own NAR in train
mode, p_dropout = 0) and, without the reference, by tests/test_nar_train_api.py against the committed fixture.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import nar_oracle as N


def adaln(x, emb_rows):
    """AdaLN.forward with a level per utterance: x [b, t, d], emb_rows [b, 2d] = (log gamma | beta) of each utterance's level."""
    d = x.shape[-1]
    log_g, beta = emb_rows[:, None, :d], emb_rows[:, None, d:]
    h = F.layer_norm(x, x.shape[-1:], eps=N.ADALN_EPS)
    h = N.ADALN_C * (1 - (N.ADALN_K * h).detach()) * h
    return log_g.exp() * h + beta


def _factors(masks, b_count, layer, kind, T, width, ref):
    """Dropout factors [b, T, width] of one site (ones where nothing was injected; padded rows are zero downstream anyway)."""
    z = torch.ones((b_count, T, width), dtype=ref.dtype)
    for b in range(b_count):
        zb = masks.get((b, layer, kind))
        if zb is not None:
            z[b, : zb.shape[0]] = zb.to(ref.dtype)
    return z


def nll(sd, n_heads: int, n_layers: int, text_list, proms_list, resps_list, levels, masks=None):
    """The training loss: resps_list [t_b, 8] each, levels[b] in 0 .. 6 -> mean over all response rows of the call of
    CE(classifier(x)[row], resps[b][f][levels[b] + 1]).  masks: {(b, layer, kind): factors [total_b, width]} or None."""
    dtype = sd["classifier.weight"].dtype
    prev = [r[:, : l + 1] for r, l in zip(resps_list, levels)]
    targ = [r[:, l + 1] for r, l in zip(resps_list, levels)]
    xs = [N.merged_sequence(sd, t, p, r) for t, p, r in zip(text_list, proms_list, prev)]
    lens = [len(x) for x in xs]
    B, T = len(xs), max(lens)
    x = torch.stack([F.pad(z, (0, 0, 0, T - len(z))) for z in xs])
    m = torch.stack([(torch.arange(T) < n) for n in lens]).unsqueeze(-1).to(dtype)
    x = x + N.sinusoid_pe(T, x.shape[-1], dtype)[None]
    lv = torch.as_tensor(list(levels))
    d = x.shape[-1]
    drop = (lambda h, i, kind: h) if not masks else (lambda h, i, kind: h * _factors(masks, B, i, kind, T, h.shape[-1], h))
    for i in range(n_layers):
        pa, pf = f"blocks.{i}.attn", f"blocks.{i}.ffn"
        x = (x + drop(N.attention(sd, pa + ".block", adaln(x, sd[pa + ".norm.emb.weight"][lv]) * m, m, n_heads), i, 0)) * m
        h = adaln(x, sd[pf + ".norm.emb.weight"][lv]) * m
        h = drop(F.gelu(F.linear(h, sd[pf + ".block.0.weight"], sd[pf + ".block.0.bias"])), i, 1)
        h = drop(F.linear(h, sd[pf + ".block.3.weight"], sd[pf + ".block.3.bias"]), i, 2)
        x = (x + h) * m
    h = F.linear(x, sd["classifier.weight"], sd["classifier.bias"]) * m
    rows = torch.cat([h[b, lens[b] - len(r): lens[b]] for b, r in enumerate(resps_list)])
    return F.cross_entropy(rows, torch.cat(targ))


def loss_and_grads(sd32, n_heads, n_layers, text_list, proms_list, resps_list, levels, masks=None, dtype=torch.float64):
    """(loss float, {name: gradient}) by autograd over `nll` with the weights cast to `dtype`."""
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd32.items()}
    loss = nll(sd, n_heads, n_layers, text_list, proms_list, resps_list, levels, masks)
    loss.backward()
    return float(loss.detach()), {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in sd.items()}


def draw_levels(seed: int, utt0: int, batch: int):
    """Numpy mirror of the level draw: l_b = min(6, int(float32(u) * float32(7))), u = word 0 of Philox key (seed; group 0,
    row utt0 + b, t 0, stream 6) from oracle/philox.py."""
    import numpy as np
    from oracle import philox
    u = philox.uniform_rows(seed & 0xFFFFFFFFFFFFFFFF, 0, utt0, batch, 4, stream=6)[:, 0]
    return [min(6, int(np.float32(v) * np.float32(7))) for v in u]


TABLES = ("text_emb.weight", "proms_emb.weight", "resps_emb.weight")


def summary(name, grad):
    """What the fixture keeps of one gradient: (stats [10] = sum, absolute sum, 8 strided samples; rows or None).  For the three
    embedding tables `rows` are the indices of the non-zero rows of the gradient viewed as [-1, d] and the samples are taken from
    those rows only (a strided sample of a whole table would land on untouched rows)."""
    g = grad.detach().double()
    flat, rows = g.reshape(-1), None
    if name in TABLES:
        g2 = g.reshape(-1, g.shape[-1])
        rows = torch.nonzero(g2.abs().sum(dim=1) != 0).reshape(-1)
        flat = g2[rows].reshape(-1)
    idx = torch.linspace(0, flat.numel() - 1, 8).long()
    stats = torch.cat([torch.stack([g.sum(), g.abs().sum()]), flat[idx]])
    return stats.numpy(), (None if rows is None else rows.numpy())

"""Host-side mirror of the condition encoders' train-mode dropout under a key mask (tests/test_gpu_train_key_mask.py), beside
tests/dropout_mirror.py: the oracle runs at the truncated shape (only the live rows exist), while the kernels index the mask
stream by the padded extents -- r * cols + c over [S_pad][cols], (h * S_pad + i) * S_pad + j over the attention probabilities.
So every site's factors are drawn at the padded extents and sliced to the live rows and keys."""
import torch
import torch.nn.functional as F

from dropout_mirror import z
from oracle import d3pm_oracle as O


def masked_mirror_encoder(seed, utt, p_layer, p_mlp, pads):
    """O.cond_encoder on the live rows x [S_live, d] with the six dropout sites of train mode; pads = (s_text, s_prompt) of the
    padded model, the extents the device draws at."""
    from vall_e.vall_e.train import MLP_LAYER, dropout_site

    def enc(sd, name, x, shape):
        which = 0 if name == "encodertext" else 1
        S, d = x.shape
        S_pad = pads[which]
        assert S <= S_pad
        H = shape.cond_heads
        hd = d // H

        def drop(t, layer, kind, p):      # an [S_live][cols] activation: rows of the [S_pad][cols] draw
            if p == 0:
                return t
            return t * z(seed, utt, dropout_site(which, layer, kind), (S_pad, t.shape[1]), p)[:S].to(t.dtype)

        def drop_probs(P, layer, p):      # [H][S_live][S_live] probabilities: live queries and keys of the [H][S_pad][S_pad] draw
            if p == 0:
                return P
            return P * z(seed, utt, dropout_site(which, layer, 0), (H, S_pad, S_pad), p)[:, :S, :S].to(P.dtype)

        for j in range(shape.cond_layers):
            pf = f"{name}.0.layers.{j}"
            qkv = F.linear(x, sd[pf + ".self_attn.in_proj_weight"], sd[pf + ".self_attn.in_proj_bias"])
            qh, kh, vh = (t.reshape(S, H, hd).transpose(0, 1) for t in qkv.split(d, dim=-1))
            P = drop_probs(torch.softmax((qh * hd ** -0.5) @ kh.transpose(-1, -2), dim=-1), j, p_layer)
            att = (P @ vh).transpose(0, 1).reshape(S, d)
            x = O._ln(sd, pf + ".norm1", x + drop(O._lin(sd, pf + ".self_attn.out_proj", att), j, 1, p_layer), 1e-5)
            ff = drop(F.relu(O._lin(sd, pf + ".linear1", x)), j, 2, p_layer)
            x = O._ln(sd, pf + ".norm2", x + drop(O._lin(sd, pf + ".linear2", ff), j, 3, p_layer), 1e-5)
        h = drop(F.silu(O._lin(sd, f"{name}.1.fc1", x)), MLP_LAYER, 0, p_mlp)
        return drop(O._lin(sd, f"{name}.1.fc2", h), MLP_LAYER, 1, p_mlp)
    return enc

"""Host-side mirrors of the training step's condition-encoder dropout, shared by the GPU training tests
(tests/test_gpu_train_dropout.py, tests/test_gpu_train_kernels.py, tests/test_gpu_train_d512.py): the mask factors of one
(seed, utterance, site) from the numpy Philox mirror (tests/test_train_dropout_api.py:mask_z), and the oracle's condition
encoder with the six train-mode dropout sites applied with those masks."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import d3pm_oracle as O
from test_train_dropout_api import mask_z


def z(seed, utt, site, shape, p):
    """fp32 factors (0 or 1 / (1 - p)) of the logical elements of a tensor of `shape`, row-major."""
    return torch.from_numpy(mask_z(seed, utt, site, int(np.prod(shape)), p).reshape(shape))


def mirror_encoder(seed, utt, p_layer, p_mlp):
    """O.cond_encoder with the six dropout sites of train mode, masks from the mirror; the attention written out."""
    from vall_e.vall_e.train import MLP_LAYER, dropout_site

    def enc(sd, name, x, shape):
        which = 0 if name == "encodertext" else 1
        S, d = x.shape
        H = shape.cond_heads
        hd = d // H

        def drop(t, layer, kind, p):
            return t if p == 0 else t * z(seed, utt, dropout_site(which, layer, kind), tuple(t.shape), p).to(t.dtype)

        for j in range(shape.cond_layers):
            pf = f"{name}.0.layers.{j}"
            qkv = F.linear(x, sd[pf + ".self_attn.in_proj_weight"], sd[pf + ".self_attn.in_proj_bias"])
            qh, kh, vh = (t.reshape(S, H, hd).transpose(0, 1) for t in qkv.split(d, dim=-1))
            P = drop(torch.softmax((qh * hd ** -0.5) @ kh.transpose(-1, -2), dim=-1), j, 0, p_layer)
            att = (P @ vh).transpose(0, 1).reshape(S, d)
            x = O._ln(sd, pf + ".norm1", x + drop(O._lin(sd, pf + ".self_attn.out_proj", att), j, 1, p_layer), 1e-5)
            ff = drop(F.relu(O._lin(sd, pf + ".linear1", x)), j, 2, p_layer)
            x = O._ln(sd, pf + ".norm2", x + drop(O._lin(sd, pf + ".linear2", ff), j, 3, p_layer), 1e-5)
        h = drop(F.silu(O._lin(sd, f"{name}.1.fc1", x)), MLP_LAYER, 0, p_mlp)
        return drop(O._lin(sd, f"{name}.1.fc2", h), MLP_LAYER, 1, p_mlp)
    return enc

"""TEST INFRASTRUCTURE -- host reference of classifier-free guidance in the NAR stage's level draw (include/d3pm_hip.h:
d3pm_nar_level_guided; csrc/d3pm_nar_draw.hip), beside guidance_ref.py, whose construction it uses.  No GPU here.

  combine   z = rn<T>(fmaf(w, float(c) - float(u), float(c))) evaluated without an fma (guidance_ref._parts: the fp32 difference, the
            product exact in fp64, one rounding of the fp64 sum to fp32), then the LAST rounding to the storage type T: to fp16 for
            f16, guidance_ref.on_grid for bf16, nothing for fp32.  Exact only where guidance_ref.exact holds: dyadic weights and
            logits on a 16-bit grid (also for the fp32 arm), which the tests assert on their own inputs.
  grids     the padded grids of the draw tests: 2 pairs, utterance 2 + b the twin of b, with different t_text / t_prompt in the two
            halves so that a frame's two rows sit at different offsets; 12 frames are drawn, one is cut by the grid in the
            conditioned half and one in the twin's half.  The rows are guidance_ref.crafted; every other row of the grid is noise
            and the pad columns hold 60000, so a kernel that reads a neighbour's row or a pad column lands on another id.
  twins     what NAR.forward packs under guidance, restated: lengths, duplicated responses."""
import numpy as np
import torch

import guidance_ref as G

N_TOKENS = 1024
LDL = N_TOKENS + 8
PAD = 60000.0
T_MAX = 16
TR_MAX = 9
# (t_text, t_prompt, t_response): the utterances, then their twins.  Pair 0: rows 9 + f against 2 + f, frame 7 of the conditioned half
# is row 16 = T_MAX (cut).  Pair 1: rows 5 + f against 11 + f, frame 5 of the twin is row 16 (cut).
LENS = ((3, 4, 8), (2, 1, 6), (0, 0, 8), (5, 4, 6))
BATCH = 2
WEIGHTS = (0.5, 1.5, 3.0)
GRID_OF = {torch.float16: np.float16, torch.bfloat16: "bfloat16", torch.float32: np.float16}      # fp32 logits on a 16-bit grid too


def live_frames(b):
    """The frames of pair b that the guided draw writes: inside the response and both rows inside the grid."""
    (tt, tp, tr), (nt, npr, _) = LENS[b], LENS[BATCH + b]
    return [f for f in range(tr) if tt + tp + 2 + f < T_MAX and nt + npr + 2 + f < T_MAX]


def frames_mask():
    m = torch.zeros(BATCH, TR_MAX, dtype=torch.bool)
    for b in range(BATCH):
        m[b, live_frames(b)] = True
    return m


N_LIVE = sum(len(live_frames(b)) for b in range(BATCH))


def combine(c, u, w, dtype):
    """fp32 numpy arrays (values exact in `dtype`) -> the guided row as fp32 values exact in `dtype`."""
    c64, _, prod = G._parts(c, u, w)
    z = (prod + c64).astype(np.float32)
    if dtype == torch.float16:
        return z.astype(np.float16).astype(np.float32)
    if dtype == torch.bfloat16:
        return G.on_grid(z, "bfloat16")
    return z


def rows(dtype, seed=3, same=False):
    """(c, u): fp32 numpy [N_LIVE, N_TOKENS] on the grid of `dtype`, live frame after live frame.  same: u = c."""
    c, u = G.crafted(N_LIVE, N_TOKENS, seed, GRID_OF[dtype])
    return (c, c.copy()) if same else (c, u)


def grid(dtype, c, u, seed=5):
    """-> logits [2 BATCH, T_MAX, LDL] of `dtype` with the rows c / u at the live frames of the two halves."""
    g = np.random.default_rng(seed)
    full = (g.standard_normal((2 * BATCH, T_MAX, LDL)) * 2.0).astype(np.float32)
    full[..., N_TOKENS:] = PAD
    at = 0
    for b in range(BATCH):
        (tt, tp, _), (nt, npr, _) = LENS[b], LENS[BATCH + b]
        for f in live_frames(b):
            full[b, tt + tp + 2 + f, :N_TOKENS] = c[at]
            full[BATCH + b, nt + npr + 2 + f, :N_TOKENS] = u[at]
            at += 1
    return torch.from_numpy(full).to(dtype)


def plain_grid(dtype, z, seed=5):
    """-> logits [BATCH, T_MAX, LDL] of `dtype`: the conditioned half's layout with the host-combined rows z at the live frames."""
    return grid(dtype, z, z, seed)[:BATCH].contiguous()


def log_softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def twins(text_list, proms_list, resps_list, null_text_list=None, null_proms_list=None):
    """The 2 B lists NAR.forward packs under guidance: the utterances, then per utterance the null text (default: empty), the null
    prompt (default: no frames) and the SAME response."""
    nt = [t[:0] for t in text_list] if null_text_list is None else list(null_text_list)
    npr = [p[:0] for p in proms_list] if null_proms_list is None else list(null_proms_list)
    return list(text_list) + nt, list(proms_list) + npr, list(resps_list) + list(resps_list)

"""The confidence-ordered reveal schedule of include/d3pm_hip.h (d3pm_reveal) in numpy: timesteps, quota, order key, selection, one
step, and the float64 mirror of the candidate / score of a row.  Shared by tests/test_reveal_api.py (CPU) and
tests/test_gpu_reveal.py; not a test module."""
import numpy as np

import nucleus_ref as NR

NEG_INF = float("-inf")
FLT_MIN = 1.17549435e-38


def timesteps(T, N):
    """t_i = (T-1) - floor(i (T-1) / N), i = 0 .. N-1, then t_N = 0."""
    assert 1 <= N <= T - 1
    return [(T - 1) - (i * (T - 1)) // N for i in range(N)] + [0]


def cbar_f32(cbar_bits):
    """fp16 bit patterns of the schedule -> the float32 values the quota is defined on."""
    return np.asarray(cbar_bits, dtype=np.uint16).view(np.float16).astype(np.float32)


def keep_fraction(cbar, T, N, i):
    """float(cbar[t_{i+1}]) of step i; 0 for the last step."""
    ts = timesteps(T, N)
    return np.float32(cbar[ts[i + 1]]) if i + 1 < N else np.float32(0.0)


def quota(F, masked_now, keep_frac):
    """-> (keep, reveal): keep = min(masked_now, floor((double) F * (double) keep_frac))."""
    keep = min(int(masked_now), int(np.floor(np.float64(F) * np.float64(np.float32(keep_frac)))))
    return keep, int(masked_now) - keep


def plan(F, masked0, cbar, T, N):
    """The masked count of an utterance with F free rows, masked0 of them masked at the start, after every step."""
    out, m = [], int(masked0)
    for i in range(N):
        m, _ = quota(F, m, keep_fraction(cbar, T, N, i))
        out.append(m)
    return out


def order_key(score):
    """The monotone uint32 image of the fp32 bits: unsigned order = order of the values."""
    u = np.asarray(score, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def select(score, masked, n_reveal):
    """Frame indices (sorted) of the n_reveal masked rows that come first in the order: key descending, frame index ascending."""
    idx = np.flatnonzero(masked)
    key = order_key(np.asarray(score, dtype=np.float32)[idx])
    first = idx[np.lexsort((idx, -key.astype(np.int64)))]      # last key of lexsort is the primary one
    return np.sort(first[:max(0, min(int(n_reveal), len(idx)))])


def step(x_t, frame_mask, known, cand, score, mask_id, keep_frac):
    """One step on the host for a batch: x_t int [B, canvas], frame_mask [B, canvas] (or [canvas]), known [B, canvas] or None,
    cand / score [B, canvas] as the device reports them -> x_next."""
    x_t = np.asarray(x_t)
    B, canvas = x_t.shape
    fm = np.broadcast_to(np.asarray(frame_mask) != 0, (B, canvas))
    kn = np.zeros((B, canvas), bool) if known is None else np.asarray(known) != 0
    out = x_t.copy()
    for b in range(B):
        free = fm[b] & ~kn[b]
        masked = free & (x_t[b] == mask_id)
        _, n_rev = quota(int(free.sum()), int(masked.sum()), keep_frac)
        pick = select(score[b], masked, n_rev)
        out[b, pick] = np.asarray(cand)[b, pick]
    return out


# ---- the candidate and the score of a row ---------------------------------------------------------------------------------------
def filtered_logits(l, mask_id, tau=1.0, k=0, top_p=1.0):
    """z''' [rows, K] float32: z = rn16(l), class mask_id -> -inf, then temperature / top-k / top-p as nucleus_ref defines them."""
    z = np.asarray(l, dtype=np.float32).astype(np.float16).astype(np.float32).copy()
    z[..., mask_id] = NEG_INF
    return NR.host_nucleus(z, tau, k, top_p)


def gumbel64(u):
    u = np.clip(np.asarray(u, dtype=np.float64), FLT_MIN, 1.0)
    return -np.log(-np.log(u))


def log_softmax64(z3):
    z = np.asarray(z3, dtype=np.float64)
    m = z.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))


def first_argmax(v):
    """First-index argmax per row."""
    return np.argmax(v, axis=-1)      # numpy returns the first maximal index


def mirror_candidates(z3, u=None):
    """float64 mirror: -> (cand [rows], runner-up [rows], gap [rows]) of z''' + gumbel(u) (u None: greedy, of z''' itself)."""
    v = np.asarray(z3, dtype=np.float64) + (0.0 if u is None else gumbel64(u))
    best = first_argmax(v)
    r = np.arange(v.shape[0])
    top = v[r, best]
    w = v.copy()
    w[r, best] = NEG_INF
    second = first_argmax(w)
    return best, second, top - w[r, second]

"""The reveal schedule with revision of include/d3pm_hip.h (d3pm_revise) in numpy: the quota, the selection among ALL free rows, one
step, the plan of masked counts, the `step` grid a trace implies, and the row-level inputs the GPU tests share.  Host only.  Shared by
tests/test_revise_api.py (CPU) and tests/test_gpu_revise.py; not a test module."""
import numpy as np

import reveal_ref as R

order_key = R.order_key
timesteps = R.timesteps
cbar_f32 = R.cbar_f32


def hold_count(F, keep_frac):
    """How many free rows of an utterance with F of them hold an id after a step: F - floor((double) F * (double) float(keep_frac))."""
    return int(F) - int(np.floor(np.float64(F) * np.float64(np.float32(keep_frac))))


def select(score, free, n_hold):
    """Frame indices (sorted) of the n_hold free rows that come first in the order: key descending, frame index ascending."""
    idx = np.flatnonzero(free)
    key = order_key(np.asarray(score, dtype=np.float32)[idx])
    first = idx[np.lexsort((idx, -key.astype(np.int64)))]      # last key of lexsort is the primary one
    return np.sort(first[:max(0, min(int(n_hold), len(idx)))])


def step(x_t, frame_mask, known, cand, score, mask_id, keep_frac):
    """One step on the host for a batch: x_t int [B, canvas], frame_mask [B, canvas] (or [canvas]), known [B, canvas] or None,
    cand / score [B, canvas] as the device reports them -> x_next.  A selected free row takes cand (a held row's cand is its own id),
    an unselected free row takes mask_id, every other row keeps x_t."""
    x_t = np.asarray(x_t)
    B, canvas = x_t.shape
    fm = np.broadcast_to(np.asarray(frame_mask) != 0, (B, canvas))
    kn = np.zeros((B, canvas), bool) if known is None else np.asarray(known) != 0
    out = x_t.copy()
    for b in range(B):
        free = fm[b] & ~kn[b]
        pick = select(score[b], free, hold_count(int(free.sum()), keep_frac))
        out[b, free] = mask_id
        out[b, pick] = np.asarray(cand)[b, pick]
    return out


def plan(F, cbar, T, N):
    """The masked count of an utterance with F free rows after every step: floor(F cbar[t_{i+1}]), 0 after the last one --
    whatever the canvas looked like before."""
    return [int(F) - hold_count(F, R.keep_fraction(cbar, T, N, i)) for i in range(N)]


def last_reveal(trace, ts, x0, free, mask_id):
    """The `step` grid as the definition states it, from a trace [n][...] whose entry i is x after the step at timestep ts[i] and the
    canvas x0 the loop started from: -1 off the free masked rows of x0; a row that goes id -> mask gets 0 (also from -1); a row with 0
    that leaves the mask gets ts[i].  At the end: the timestep of the LAST time a row left the mask."""
    trace, x0 = np.asarray(trace), np.asarray(x0)
    step_ = np.where(free & (x0 == mask_id), 0, -1).astype(np.int32)
    prev = x0
    for i in range(trace.shape[0]):
        cur = trace[i]
        step_ = np.where(free & (prev != mask_id) & (cur == mask_id), 0, step_)
        step_ = np.where((step_ == 0) & (cur != mask_id), ts[i], step_).astype(np.int32)
        prev = cur
    return step_


def case(K, canvas, seed, B=3, held=0.3, with_known=True):
    """Ragged batch of B utterances (lengths canvas, 2/3 and 1/3 of it): logits float32 [B, canvas, K] of the randn * 3 kind with every
    fifth row constant, x_t int32 with the share `held` of the rows holding an id, known rows on utterances 0 and 1 (one of them a
    known mask id, which is legal and is not a masked row), 0 on the padded rows.
    -> logits, x_t, frame_mask uint8, known uint8 (or None), lens"""
    g = np.random.default_rng(seed)
    mask_id = K // 2
    lens = [canvas, max(1, (2 * canvas) // 3), max(1, canvas // 3)][:B]
    logits = (g.standard_normal((B, canvas, K)) * 3).astype(np.float32)
    logits[:, 0::5] = 0.75
    fm = (np.arange(canvas)[None] < np.asarray(lens)[:, None]).astype(np.uint8)
    ids = g.integers(0, min(K, 1024), (B, canvas))
    ids = np.where(ids == mask_id, ids + 1, ids)
    x = np.where(g.random((B, canvas)) < held, ids, mask_id)
    known = np.zeros((B, canvas), np.uint8)
    if with_known:
        known[0, : max(1, canvas // 8)] = 1
        if B > 1:
            known[1, 1::7] = 1
        known &= fm
        x = np.where(known != 0, (ids + 3) % min(K, 1024), x)
        if B > 1 and known[1, 1]:
            x[1, 1] = mask_id
    x = np.where(fm != 0, x, 0).astype(np.int32)
    return logits, x, fm, (known if with_known else None), lens


def kinds(x, fm, known, mask_id):
    """-> (masked, held, free) bool arrays: the free rows of x, split by whether they hold the mask id."""
    x, fm = np.asarray(x), np.asarray(fm) != 0
    free = fm & ~(np.zeros_like(fm) if known is None else np.asarray(known) != 0)
    masked = free & (x == mask_id)
    return masked, free & ~masked, free

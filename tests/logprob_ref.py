"""TEST INFRASTRUCTURE -- host reference of the per-frame log-probability (include/d3pm_hip.h: d3pm_frame_scores).

logprob64(logits, mask_id, ids) is the definition in float64: z_k = rn16(float(l_k)), the mask class removed, log_softmax at the id.
cases(...) builds the row-level inputs the GPU tests share: a frame mask with a padded tail, a known map, x_t cycling through masked,
masked, revealed and known rows; state(...) says what d3pm_frame_scores_init must write for them."""
import numpy as np

TOL = 1.0e-4      # the bound of the header: the reveal score's, same three roundings and a sum of <= 1280 terms


def rn16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def logprob64(logits, mask_id, ids):
    """logits [rows, K] (any float array: the values as stored), ids [rows] -> float64 [rows]: log_softmax over the classes but mask_id
    of z = rn16(logits), taken at ids."""
    z = rn16(logits).astype(np.float64)
    z[:, mask_id] = -np.inf
    m = z.max(-1, keepdims=True)
    ls = z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))
    return ls[np.arange(z.shape[0]), np.asarray(ids)]


def logprob32_serial(logits, mask_id, ids):
    """The same in fp32 with a serial sum in ascending class: what any fp32 implementation of the definition gives up to summation order."""
    z = rn16(logits).astype(np.float32)
    z[:, mask_id] = -np.inf
    m = z.max(-1)
    s = np.zeros(z.shape[0], dtype=np.float32)
    for k in range(z.shape[1]):
        s = (s + np.exp(z[:, k] - m).astype(np.float32)).astype(np.float32)
    zj = z[np.arange(z.shape[0]), np.asarray(ids)]
    return ((zj - m).astype(np.float32) - np.log(s).astype(np.float32)).astype(np.float32)


def cases(B, canvas, K, seed, scale=3.0):
    """-> logits float32 [B, canvas, K] (randn * scale, every fifth row constant), x_t int32 [B, canvas], frame_mask uint8 [B, canvas]
    (the last utterance has a padded tail), known uint8 [B, canvas].  Rows cycle r % 4: 0 and 1 masked, 2 already revealed, 3 known;
    padded rows hold 0."""
    g = np.random.default_rng(seed)
    mask_id = K // 2
    logits = (g.standard_normal((B, canvas, K)) * scale).astype(np.float32)
    logits[:, 0::5] = 0.75
    lens = [canvas] * (B - 1) + [max(1, (3 * canvas) // 4)]
    fm = (np.arange(canvas)[None] < np.asarray(lens)[:, None]).astype(np.uint8)
    ids = g.integers(0, min(K, 1024), (B, canvas))
    ids = np.where(ids == mask_id, ids + 1, ids)
    r = np.arange(B * canvas).reshape(B, canvas)
    x = np.where(r % 4 >= 2, ids, mask_id)
    known = ((r % 4 == 3) & (fm != 0)).astype(np.uint8)
    x = np.where(fm != 0, x, 0).astype(np.int32)
    return logits, x, fm, known


def free_masked(x, fm, known, mask_id):
    return (np.asarray(fm) != 0) & (np.asarray(known) == 0) & (np.asarray(x) == mask_id)


def other_ids(shape, K, seed):
    """random codec ids, never the mask id"""
    g = np.random.default_rng(seed)
    ids = g.integers(0, min(K, 1024), shape)
    return np.where(ids == K // 2, ids + 1, ids).astype(np.int32)


def first_reveal(trace, ts, x0, free, mask_id):
    """step as the definition states it, from a trace [n][...] whose entry i is x after the iteration at timestep ts[i]: -1 off the free
    masked rows of x0, else the timestep of the first entry whose id is not the mask (0: none)."""
    trace = np.asarray(trace)
    step = np.where(free, 0, -1).astype(np.int32)
    for i in range(trace.shape[0] - 1, -1, -1):
        step = np.where(free & (trace[i] != mask_id), ts[i], step)
    return step

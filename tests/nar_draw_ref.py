"""Host reference of the NAR stage's level draw with options (include/d3pm_hip.h: d3pm_nar_draw; csrc/d3pm_nar_draw.hip), beside
nar_mirror.py, whose inputs and rounding it uses (draw_inputs, draw_rows, DRAW_LENS, rn).  No GPU here.

  values        v = rn<T>(float(logit) / float32(temperature)): what the draw compares, fp32 numbers exact in the storage type T
  order_key     the unsigned key of a value in its own storage type (16 bits of the f16 / bf16 pattern, 32 bits of an fp32): negative
                values reverse, the others move above them
  theta1        the top_k-th largest v of every row counted with multiplicity (top_k = 0: -inf)
  cut           v >= theta ? v : -inf, per row, compared on values
  masses        q = (uint32) (float32 exp(v' - max v') * 2^20) and Q = sum q.  The device's expf may sit an fp32 step from numpy's, so a q
                here may differ from the device's by one unit: the GPU tests take the device's theta and check it against the float64
                softmax within the header's bound; the theta below is the definition on THESE q
  theta_nucleus the value of the largest key c with (double) mass(c) >= (double) float32(top_p) * (double) Q
  log_softmax64 float64 log-softmax of float(logits)

Rows that are -inf throughout are outside the top-p contract (masses and theta_nucleus refuse them)."""
import numpy as np
import torch

from nar_mirror import DRAW_LENS, draw_frames, draw_inputs, draw_rows, rn  # noqa: F401  (the tests take them from here)

KEY_BITS = {torch.float16: 16, torch.bfloat16: 16, torch.float32: 32}
SCALE = np.float32(1048576.0)


def values(rows: torch.Tensor, temperature: float) -> torch.Tensor:
    """rows [n, K] of a storage type T -> fp32 [n, K], every element exact in T."""
    return rn(torch.from_numpy(rows.float().numpy() / np.float32(temperature)), rows.dtype)


def order_key(v: torch.Tensor, dtype) -> np.ndarray:
    """fp32 values exact in `dtype` -> uint64 keys whose unsigned order is the order of the values (-0 below +0)."""
    if dtype == torch.float32:
        u = v.contiguous().numpy().view(np.uint32).astype(np.uint64)
    else:
        u = v.to(dtype).contiguous().view(torch.int16).numpy().view(np.uint16).astype(np.uint64)
    bits = KEY_BITS[dtype]
    top, full = np.uint64(1 << (bits - 1)), np.uint64((1 << bits) - 1)
    return np.where(u & top != 0, ~u & full, u | top)


def theta1(v: torch.Tensor, top_k: int) -> np.ndarray:
    n, K = v.shape
    if top_k == 0:
        return np.full(n, -np.inf, dtype=np.float32)
    assert 1 <= top_k <= K
    return -np.sort(-v.numpy(), axis=-1)[:, top_k - 1]


def cut(v: torch.Tensor, theta) -> torch.Tensor:
    theta = torch.as_tensor(np.asarray(theta, dtype=np.float32))[:, None]
    return torch.where(v >= theta, v, torch.full_like(v, -np.inf))


def masses(vp: torch.Tensor):
    a = vp.numpy()
    m = a.max(axis=-1, keepdims=True)
    assert np.isfinite(m).all(), "a row that is -inf throughout is outside the top-p contract"
    q = (np.exp((a - m).astype(np.float32)).astype(np.float32) * SCALE).astype(np.uint32).astype(np.uint64)
    return q, q.sum(axis=-1)


def theta_nucleus(vp: torch.Tensor, top_p: float, dtype) -> np.ndarray:
    """Per row of v' (the values behind the top-k cut): theta, -inf for top_p = 1."""
    n, K = vp.shape
    if not np.float32(top_p) < np.float32(1.0):
        return np.full(n, -np.inf, dtype=np.float32)
    q, Q = masses(vp)
    key = order_key(vp, dtype)
    order = np.argsort(-key.astype(np.int64), axis=-1, kind="stable")          # keys descending (< 2^33: exact in int64)
    ks, qs, vs = (np.take_along_axis(x, order, axis=-1) for x in (key, q, vp.numpy()))
    cum = np.cumsum(qs, axis=-1)
    target = np.float64(np.float32(top_p)) * Q.astype(np.float64)
    theta = np.empty(n, dtype=np.float32)
    for r in range(n):
        # mass(c) for c = a key of the row is the cumulated q up to the LAST slot that holds this key
        last = np.nonzero(np.append(ks[r, 1:] != ks[r, :-1], True))[0]
        ok = last[cum[r, last].astype(np.float64) >= target[r]]
        theta[r] = vs[r, ok[0]]
    return theta


def log_softmax64(rows: torch.Tensor) -> np.ndarray:
    z = rows.float().double().numpy()
    m = z.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def softmax64(vp: torch.Tensor) -> np.ndarray:
    z = vp.double().numpy()
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def without_dead_rows(grid: torch.Tensor, n_tokens: int) -> torch.Tensor:
    """The grid with every response row that is -inf throughout replaced by its predecessor (the top-p inputs)."""
    out = grid.clone()
    for b, (tt, tp, _) in enumerate(DRAW_LENS):
        base = tt + tp + 2
        for f in range(draw_frames(b)):
            if bool(torch.isinf(out[b, base + f, :n_tokens].float()).all()):
                out[b, base + f, :n_tokens] = out[b, base + f - 1, :n_tokens]
    return out

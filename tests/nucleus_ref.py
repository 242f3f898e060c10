"""The nucleus (top-p) definition of include/d3pm_hip.h (d3pm_nucleus) in numpy, and the crafted rows whose answer is known without
trusting the last bit of any exp.  Shared by tests/test_nucleus_api.py (CPU) and tests/test_gpu_nucleus.py; not a test module."""
import numpy as np

NEG_INF = float("-inf")
UNIT = 1048576.0      # 2^20: q of the row maximum


def host_filter(l, tau, k):
    """Temperature and top-k as d3pm_sampling defines them, in numpy: l any float array [..., K] -> float32 array of the fp16 values
    z'' = (z' >= theta ? z' : -inf), z' = rn16(rn16(l) / tau) (an IEEE fp32 division), theta = the k-th largest z' (k = 0: no cut)."""
    z = np.asarray(l, dtype=np.float32).astype(np.float16).astype(np.float32)
    z = (z / np.float32(tau)).astype(np.float16).astype(np.float32)
    if k > 0:
        theta = -np.sort(-z, axis=-1)[..., k - 1:k]
        z = np.where(z >= theta, z, np.float32(NEG_INF)).astype(np.float32)
    return z


def order_key(z):
    """The 16-bit key of an fp16 value whose unsigned order is the order of the values (-0 just below +0)."""
    u = np.asarray(z, dtype=np.float32).astype(np.float16).view(np.uint16).astype(np.uint32)
    return np.where(u & 0x8000, ~u & 0xFFFF, u | 0x8000).astype(np.uint32)


def key_value(c):
    c = np.asarray(c, dtype=np.uint32)
    u = np.where(c & 0x8000, c & 0x7FFF, ~c & 0xFFFF).astype(np.uint16)
    return u.view(np.float16).astype(np.float32)


def quanta(z2, exp=np.exp):
    """q_j = (uint32)(expf(z''_j - m) * 2^20), truncated.  `exp` is whatever float32 exp the caller trusts; the device has its own."""
    z2 = np.asarray(z2, dtype=np.float32)
    m = z2.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = exp((z2 - m).astype(np.float32)).astype(np.float32)
    return np.floor(e * np.float32(UNIT)).astype(np.int64)


def nucleus_theta(z2, top_p, exp=np.exp):
    """theta per row: the value of the LARGEST key c with (double) mass(c) >= (double) top_p * (double) Q, mass(c) the sum of the q_j
    with key_j >= c.  Built bit by bit from the top, as the header says it may be (mass is monotone in c)."""
    z2 = np.asarray(z2, dtype=np.float32)
    flat = z2.reshape(-1, z2.shape[-1])
    q = quanta(flat, exp)
    key = order_key(flat).astype(np.int64)
    rhs = np.float64(np.float32(top_p)) * q.sum(-1).astype(np.float64)
    c = np.zeros(flat.shape[0], dtype=np.int64)
    for bit in (1 << b for b in range(15, -1, -1)):
        cand = c | bit
        mass = np.where(key >= cand[:, None], q, 0).sum(-1)
        c = np.where(mass.astype(np.float64) >= rhs, cand, c)
    return key_value(c).reshape(z2.shape[:-1])


def cut_at(z2, theta):
    """z''' = z'' >= theta ? z'' : -inf, compared on values."""
    z2 = np.asarray(z2, dtype=np.float32)
    th = np.asarray(theta, dtype=np.float32)[..., None]
    return np.where(z2 >= th, z2, np.float32(NEG_INF)).astype(np.float32)


def host_nucleus(l, tau, k, top_p, exp=np.exp):
    z2 = host_filter(l, tau, k)
    return cut_at(z2, nucleus_theta(z2, top_p, exp)) if top_p < 1.0 else z2


# ---- rows whose kept set is known without the last bit of exp ----------------------------------------------------------------------
# a classes at m, b classes at m - delta, the rest -inf (or absent from the mass: q = 0).  q of the upper level is exactly 2^20 each;
# q of the lower level is w = trunc(exp(-delta) 2^20), known to within a few units.  The upper level alone is the nucleus iff
# a 2^20 >= top_p Q, Q = a 2^20 + b w.  (a, b, top_p) below miss or clear that by far more than a + b units plus 16 units of doubt
# about every w (checked by two_level_cases itself, in float64), so the kept set does not depend on how exp rounds.
TWO_LEVEL = [      # (a, b, m, delta, top_p, upper level alone?)
    (1, 1, 3.0, 1.0, 0.5, True),
    (1, 1, 3.0, 1.0, 0.9, False),
    (3, 100, 0.5, 1.0, 0.05, True),
    (3, 100, 0.5, 1.0, 0.5, False),
    (7, 40, -2.0, 2.5, 0.6, True),
    (7, 40, -2.0, 2.5, 0.75, False),
    (64, 900, 10.0, 4.0, 0.75, True),
    (64, 900, 10.0, 4.0, 0.85, False),
]


def two_level_row(K, a, b, m, delta, seed):
    """One row of K classes: a of them at m, b at m - delta, the rest -inf, at positions drawn from `seed`."""
    assert a + b <= K
    pos = np.random.default_rng(seed).permutation(K)
    row = np.full(K, NEG_INF, dtype=np.float32)
    row[pos[:a]] = m
    row[pos[a:a + b]] = m - delta
    assert np.array_equal(row, row.astype(np.float16).astype(np.float32)), "m and m - delta must be fp16 values"
    return row, pos[:a], pos[a:a + b]


def two_level_cases(K):
    """-> list of (row [K] float32, top_p, kept class ids (sorted), theta) for every TWO_LEVEL entry that fits K classes."""
    out = []
    for i, (a, b, m, delta, top_p, upper_alone) in enumerate(TWO_LEVEL):
        if a + b > K:
            continue
        w = np.exp(-np.float64(delta)) * UNIT
        p32 = np.float64(np.float32(top_p))
        gap = a * UNIT - p32 * (a * UNIT + b * w)
        doubt = p32 * b * 16.0 + a + b          # 16 units of doubt about each w, a + b units of margin on top
        assert (gap > doubt) if upper_alone else (gap < -doubt), (a, b, top_p, gap, doubt)
        row, up, low = two_level_row(K, a, b, m, delta, seed=100 + i)
        kept = np.sort(up if upper_alone else np.concatenate([up, low]))
        out.append((row, top_p, kept, np.float32(m if upper_alone else m - delta)))
    return out

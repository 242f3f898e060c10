"""TEST INFRASTRUCTURE -- host reference of classifier-free guidance (include/d3pm_hip.h: d3pm_guidance).

combine(c, u, w) is the definition  z = rn16(fmaf(w, float(c) - float(u), float(c)))  evaluated without an fma: the difference is
rounded to fp32 once (it is exact in fp64), the product w * d of two fp32 numbers is exact in fp64, and for 16-bit logits and dyadic
w the sum with c is exact in fp64 too, so one rounding to fp32 gives what the fma gives.  exact(c, u, w) checks that last step on
the caller's own inputs (TwoSum error term == 0), exact_rational does it in rational arithmetic on a sample."""
from fractions import Fraction

import numpy as np

from oracle import philox

COND_DROP_STREAM = 5


def rn16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def _parts(c, u, w):
    c64, u64 = np.asarray(c, dtype=np.float32).astype(np.float64), np.asarray(u, dtype=np.float32).astype(np.float64)
    d = (c64 - u64).astype(np.float32)                       # the fp32 subtraction: one rounding of an exact fp64 difference
    prod = np.float64(np.float32(w)) * d.astype(np.float64)  # 24 x 24 bits: exact in fp64
    return c64, d, prod


def combine(c, u, w):
    """fp16 array: float32(w * float64(float32(float64(c) - float64(u))) + float64(c)), then one rounding to fp16."""
    c64, _, prod = _parts(c, u, w)
    return (prod + c64).astype(np.float32).astype(np.float16)


def exact(c, u, w):
    """True where prod + c is exact in fp64 (TwoSum error 0): there float32(prod + c) IS fmaf(w, d, c)."""
    c64, _, prod = _parts(c, u, w)
    s = prod + c64
    bb = s - prod
    err = (prod - (s - bb)) + (c64 - bb)
    return err == 0.0


def exact_rational(c, u, w, n=2000, seed=0):
    """The same statement in rational arithmetic on n sampled elements: w * d + c as a Fraction equals the fp64 sum."""
    c64, d, prod = _parts(c, u, w)
    flat = np.random.default_rng(seed).integers(0, c64.size, n)
    cf, df, sf = c64.reshape(-1)[flat], d.reshape(-1)[flat], (prod + c64).reshape(-1)[flat]
    fw = Fraction(float(np.float32(w)))
    return all(fw * Fraction(float(dv)) + Fraction(float(cv)) == Fraction(float(sv)) for cv, dv, sv in zip(cf, df, sf))


def crafted(rows, K, seed, dtype=np.float16):
    """Seeded logits (c, u), float32 arrays of values on the grid of `dtype` ('bfloat16' or a numpy dtype), every row's twin its own:
    on three rows in four the conditioned row peaks at class a with b close behind, the null row agrees at a and sits far below at
    b -- so the guided row's argmax is b, neither argmax(c) nor argmax(u) (= a) for every w >= 0.5; the others are unrelated noise.
    A kernel that ignores u, swaps the halves or reads a neighbour's twin lands on another id."""
    g = np.random.default_rng(seed)
    c = (g.standard_normal((rows, K)) * 0.8).astype(np.float32)
    u = c + (g.standard_normal((rows, K)) * 0.1).astype(np.float32)
    r = np.arange(rows)
    a = g.integers(0, K, rows)
    b = (a + 1 + g.integers(0, K - 1, rows)) % K
    plain = r % 4 == 3
    u[plain] = (g.standard_normal((int(plain.sum()), K)) * 0.8).astype(np.float32)
    cr = r[~plain]
    c[cr, a[cr]] = 5.0; u[cr, a[cr]] = 5.0
    c[cr, b[cr]] = 4.5; u[cr, b[cr]] = 2.0
    return on_grid(c, dtype), on_grid(u, dtype)


def on_grid(x, dtype):
    """float32 values rounded to the grid of a 16-bit dtype ('bfloat16': round to nearest even on the top 16 bits)."""
    x = np.asarray(x, dtype=np.float32)
    if dtype == "bfloat16":
        b = x.view(np.uint32).astype(np.uint64)
        b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
        return b.astype(np.uint32).view(np.float32)
    return x.astype(dtype).astype(np.float32)


def cond_drop_mirror(seed, utt, p_text, p_prompt):
    """(drop text?, drop prompt?) of global utterance `utt`: words 0 and 1 of Philox key (seed; group 0, row utt, t 0, stream 5),
    dropped <=> u < p in fp32 (vall_e/vall_e/train.py: cond_drop_decision draws the same words through d3pm_uniform)."""
    u = philox.uniform_rows(seed, 0, utt, 1, 4, stream=COND_DROP_STREAM)[0]
    return bool(u[0] < np.float32(p_text)), bool(u[1] < np.float32(p_prompt))

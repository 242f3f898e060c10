"""Host definition of the block-scaled fp8 ("MX") format and the expected outputs of the exact MX tests (tests/test_gpu_mx_exact.py;
checked on the CPU against the package's own torch quantiser by tests/test_mx_ref.py).

The format, from the text of include/d3pm_hip.h (d3pm_op_quantize_mx) and nothing else:

    blocks   32 consecutive elements of a row;
    scale    of a block = the smallest power of two with absmax / scale <= 448, stored as the byte e with scale = 2^(e - 127),
             clamped to [1, 254].  Found here by SEARCH over the 254 candidate bytes in float64 -- not by arithmetic on the bits of
             the maximum, which is how the kernels (mx_scale_byte) and the package's torch quantiser (_hip.mx_scale_bytes) do it;
    codes    OCP e4m3: round(x / scale) to nearest, ties to even, onto the table of the 127 non-negative finite e4m3 values
             (subnormals included) built below from the format's definition, the sign kept (-0 keeps its sign bit);
    layout   codes [rows][K], scales [rows][4][K / 128]: scales[m][g][s] belongs to elements [128 s + 32 g, 128 s + 32 g + 32).

inf and NaN inputs are not defined by the header and are not part of any test.

Dyadic operands (as tests/gemm_exact_ref.py): x and w are j * 2^e with |j| <= 4 and one e in [-2, 2] per block, every block's
maximum equal to 4 * 2^e.  The block scale is then 2^(e - 6) and the codes are 64 j: the quantiser round-trips the values exactly,
every product is a multiple of the quantum 2^-4, and while sum |x||w| + |bias| + |r1| stays below 2^22 quanta every partial sum of any
order is exact in an fp32 accumulator.  What the GEMM stores is then decided by its epilogue alone."""
import math

import torch

from gemm_exact_ref import epilogue_chain

E4M3_MAX = 448.0
# value of code c = (e << 3) | m, 0 <= c <= 126: e = 0 -> m 2^-9 (subnormal), else (1 + m / 8) 2^(e - 7); 0x7F is the NaN code
E4M3 = torch.tensor([(c & 7) * 2.0 ** -9 if c >> 3 == 0 else (1 + (c & 7) / 8) * 2.0 ** ((c >> 3) - 7) for c in range(127)], dtype=torch.float64)
assert E4M3[126] == E4M3_MAX and bool((E4M3[1:] > E4M3[:-1]).all())
_THRESHOLDS = E4M3_MAX * torch.exp2(torch.arange(1, 254, dtype=torch.float64) - 127)      # the largest maximum byte 1 .. 253 can hold
X_EXP = W_EXP = (-2, 2)
J_MAX = 4
QUANTUM = 2.0 ** (2 * X_EXP[0])      # of a product
BIAS_STEP, R1_STEP, ADD_RANGE = 4, 8, 127      # bias = 4 j q, r1 = 8 j q, |j| <= 127: representable in both 16-bit types
EXACT_QUANTA = 2 ** 22


def scale_bytes(amax):
    """float64 block maxima (finite, >= 0) -> uint8: the first byte e in 1 .. 254 with amax / 2^(e - 127) <= 448."""
    amax = amax.double()
    assert bool(torch.isfinite(amax).all()) and bool((amax >= 0).all())
    return (1 + torch.searchsorted(_THRESHOLDS, amax.contiguous(), right=False)).to(torch.uint8)      # the bytes that are too small, counted


def codes_of(q):
    """float64 q = x / scale, |q| <= 448 -> uint8 e4m3 codes, round to nearest even on the table."""
    a = q.double().abs().contiguous()
    assert bool((a <= E4M3_MAX).all())
    lo = (torch.searchsorted(E4M3, a, right=True) - 1).clamp(0, 126)
    hi = (lo + 1).clamp_max(126)
    dlo, dhi = a - E4M3[lo], E4M3[hi] - a
    up = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    code = torch.where(up, hi, lo)
    neg = torch.signbit(q.double())
    return (code | (neg.long() << 7)).to(torch.uint8)


def values_of(codes):
    """uint8 e4m3 codes -> float64"""
    c = codes.long()
    assert bool(((c & 0x7F) != 0x7F).all()), "the NaN code"
    v = E4M3[c & 0x7F]
    return torch.where((c & 0x80) != 0, -v, v)


def quantize(x):
    """[rows, K] finite values (any float type) -> (codes uint8 [rows, K], scales uint8 [rows, 4, K // 128])"""
    rows, K = x.shape
    assert K % 128 == 0
    xd = x.double().reshape(rows, K // 128, 4, 32)
    sb = scale_bytes(xd.abs().amax(dim=-1))                                     # [rows, K / 128, 4]
    q = xd / torch.exp2(sb.double() - 127)[..., None]                           # exact: a power of two
    return codes_of(q).reshape(rows, K), sb.permute(0, 2, 1).contiguous()


def dequantize(codes, scales):
    """float64 values of (codes [rows, K], scales [rows, 4, K // 128])"""
    rows, K = codes.shape
    sc = torch.exp2(scales.permute(0, 2, 1).double() - 127)
    return (values_of(codes).reshape(rows, K // 128, 4, 32) * sc[..., None]).reshape(rows, K)


def planted_blocks(dtype):
    """[(name, 32 float64 values exactly representable in `dtype`)]: the edge cases of the quantiser, one block each."""
    f16 = dtype == torch.float16
    small = [0.0078125] * 31
    top = 65504.0 if f16 else (2.0 - 2.0 ** -7) * 2.0 ** 127
    out = [("zero_block", [0.0] * 32),
           ("minus_zero_block", [-0.0] * 32),
           ("minus_zero_beside_values", [-0.0, 1.0, -0.0, -3.0] * 8)]
    for E in (-3, 0, 5):
        out += [(f"max_1.75_2^{E}", [1.75 * 2.0 ** E] + small),                 # on the boundary: the smaller scale, code 448
                (f"max_-1.75_2^{E}", small + [-1.75 * 2.0 ** E]),
                (f"max_1.8125_2^{E}", [1.8125 * 2.0 ** E] + small),             # just above: the next power of two
                (f"tie_17_19_32_2^{E}", [17 * 2.0 ** E, 19 * 2.0 ** E, 32 * 2.0 ** E, -17 * 2.0 ** E, -19 * 2.0 ** E] + [2.0 ** E] * 27)]
    out += [("largest_finite", [top, -top, top / 2, 1.0] * 8),
            ("largest_finite_alone", [0.0] * 31 + [-top])]
    if f16:
        out += [("f16_subnormals", [k * 2.0 ** -24 for k in range(1, 33)]),
                ("f16_subnormals_top", [-(1023 - k) * 2.0 ** -24 for k in range(32)]),
                ("f16_subnormal_beside_normal", [2.0 ** -24, 2.0 ** -14, -2.0 ** -24, 3 * 2.0 ** -24] * 8)]
    else:      # bf16 carries fp32's exponent range: blocks whose scale is clamped at byte 1 (2^-126)
        out += [("bf16_subnormals", [k * 2.0 ** -133 for k in range(1, 33)]),                     # below 2^-126 altogether
                ("bf16_subnormals_top", [-(127 - k) * 2.0 ** -133 for k in range(32)]),
                ("bf16_clamped_normal", [1.5 * 2.0 ** -125, -2.0 ** -126, 2.0 ** -133, 1.75 * 2.0 ** -118] * 8),   # 448 2^-126: still byte 1
                ("bf16_first_unclamped", [1.8125 * 2.0 ** -118, 2.0 ** -126, -2.0 ** -133, 2.0 ** -120] * 8)]
    blocks = [(n, torch.tensor(v, dtype=torch.float64)) for n, v in out]
    for n, v in blocks:
        assert v.shape == (32,) and torch.equal(v.to(dtype).double(), v), n
    return blocks


def quantiser_operand(M, K, dtype, seed):
    """[M, K] of `dtype`: blocks of very different magnitude (2^-12 .. 2^12), the planted blocks in the first blocks of the tensor (as
    many as it holds, row-major over [M, K / 32]) and, from five rows on, an all-zero row behind them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).double() * torch.exp2(torch.randint(-12, 13, (M, K // 32), generator=g).double()).repeat_interleave(32, dim=1)
    x = x.to(dtype).double().reshape(M * (K // 32), 32)
    blocks = planted_blocks(dtype)
    for i, (_, v) in enumerate(blocks[:x.shape[0]]):
        x[i] = v
    x = x.reshape(M, K)
    if M >= 5:
        x[M - 2] = 0.0
    return x.to(dtype)


def _dyadic(rows, K, g):
    j = torch.randint(-J_MAX, J_MAX + 1, (rows, K // 32, 32), generator=g).double()
    at = torch.randint(0, 32, (rows, K // 32, 1), generator=g)
    j.scatter_(2, at, (torch.randint(0, 2, (rows, K // 32, 1), generator=g) * 2 - 1).double() * J_MAX)      # every block's maximum is 4
    e = torch.randint(X_EXP[0], X_EXP[1] + 1, (rows, K // 32, 1), generator=g).double()
    return (j * torch.exp2(e)).reshape(rows, K)


def dyadic_mx_operands(M, N, K, seed):
    """dict: x [M, K], w [N, K] float64 (see the module text) with their MX form (x8, sx, w8, sw), bias [N] and r1 [M, N] float64 on
    the grid of both 16-bit types, acc = x @ w.T in float64.  Asserts the round trip and the exactness bound."""
    g = torch.Generator().manual_seed(seed)
    x, w = _dyadic(M, K, g), _dyadic(N, K, g)
    bias = torch.randint(-ADD_RANGE, ADD_RANGE + 1, (N,), generator=g).double() * (BIAS_STEP * QUANTUM)
    r1 = torch.randint(-ADD_RANGE, ADD_RANGE + 1, (M, N), generator=g).double() * (R1_STEP * QUANTUM)
    bound = (x.abs() @ w.abs().T + bias.abs() + r1.abs()).max().item() / QUANTUM
    assert bound < EXACT_QUANTA, f"a partial sum could reach {bound} quanta: not exact in fp32 in every order"
    x8, sx = quantize(x)
    w8, sw = quantize(w)
    assert torch.equal(dequantize(x8, sx), x) and torch.equal(dequantize(w8, sw), w), "the operands do not round-trip"
    for t in (bias, r1):
        assert torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)
    return dict(x=x, w=w, x8=x8, sx=sx, w8=w8, sw=sw, bias=bias, r1=r1, acc=x @ w.T, bound=bound)


def expected_16bit(x, w, bias, dtype, r1=None, row_mask=None, mask_period=1):
    """The 16-bit epilogue of the MX GEMM is the 16-bit kernels' (epilogue_store): the same rounding chain on the exact products."""
    out = epilogue_chain(x, w, bias, dtype, r1=r1, row_mask=row_mask, mask_period=mask_period)
    assert bool(torch.isfinite(out.double()).all())
    return out


def expected_mx(x, w, bias):
    """The MX-output epilogue without activation: v = acc + bias is exact in fp32, so the stored block is the quantiser's of v."""
    v = x.double() @ w.double().T
    if bias is not None:
        v = v + bias.double()      # (-0 bias under an all-zero row: 0 + -0 = +0 in fp32 and here alike)
    return quantize(v)


def gelu_tanh64(v):
    """The tanh form of GELU as csrc/d3pm_mx.hip states it, v / (1 + 2^(-2 log2(e) sqrt(2 / pi) (v + 0.044715 v^3))), in float64 with
    the mathematical constants."""
    k = 2.0 * math.log2(math.e) * math.sqrt(2.0 / math.pi)
    return v / (1.0 + torch.exp2(-k * (v + 0.044715 * v ** 3)))


def boundary_distance(amax):
    """Relative distance of a block maximum from the nearest point where the scale byte changes (1.75 2^E, E any integer);
    inf for a maximum of 0 or one in the clamped range of byte 1."""
    a = amax.double()
    m, _ = torch.frexp(a)                           # a = m 2^e, m in [0.5, 1): the boundary of the binade is m = 0.875
    d = (m - 0.875).abs() / 0.875
    d = torch.minimum(d, (m - 0.4375).abs() / 0.4375)      # and the one below, for m just above 0.5
    return torch.where(a <= _THRESHOLDS[0], torch.full_like(d, float("inf")), d)


# ---- the cases of tests/test_gpu_mx_exact.py ----------------------------------------------------------------------------------------
QUANT_K, QUANT_M = (128, 384, 512, 640, 1152), (1, 5, 384)
LN_M = (1, 5, 37, 1023)
# M x N x K of the GEMM tests.  Tiles: 192 x 128 (gemm_variant 8; 512 slots) or 192 x 256 (variant 6; 256 slots); the XCD split
# deals tiles_total / 8 tiles to each of 8 XCDs and the remainder `tr` to the first ones.
GEMM_SHAPES = [(192, 128, 512),        # one tile: seven of the eight XCDs have none
               (192, 384, 512),        # 3 tiles of 192 x 128: tr = 3, the `tr != 0` arm
               (576, 640, 1024),       # 15 tiles of 192 x 128: tq = 1, tr = 7; two scale chunks
               (384, 512, 2048),       # 8 tiles of 192 x 128 / 4 of 192 x 256 (tr = 4); four scale chunks
               (6336, 2048, 512)]      # 528 tiles against 512 slots / 264 against 256: some workgroups walk across a tile boundary
TIGHT_SHAPE = (192, 384, 512)          # also runs with ldx = K, ldy = ldr = N
MASK_PERIOD = 7


def mx_tile(M, N, K, variant):
    """(TM, TN) of the tile gemm_variant 6 / 8 pins, None where mx_linear_supported refuses the shape under it (csrc/d3pm_mx.hip,
    mx_geometry); variant 0 runs every shape of GEMM_SHAPES."""
    tm, tn = {6: (192, 256), 8: (192, 128)}[variant]
    return (tm, tn) if M % tm == 0 and N % tn == 0 and K % 512 == 0 else None


# ---- GELU (tanh form) behind the MX-output epilogue -----------------------------------------------------------------------------------
U = 2.0 ** -24                   # half an ulp of fp32, relative: one correctly rounded fp32 operation
TINY = 4 * 2.0 ** -149
GELU_K = 2.0 * math.log2(math.e) * math.sqrt(2.0 / math.pi)
SWEEP_MARGIN = 2.0 ** -12        # relative distance every block maximum of the sweep keeps from a scale boundary


def gelu_tanh_delta(v, g):
    """|fp32 result of the MX epilogue's GELU - gelu_tanh64(v)| for an exact 16-bit v, from the operations of csrc/d3pm_mx.hip:
      p = fma(fl(v v), c1, c0), u' = fl(v p) with c0 = fl(-k), c1 = fl(fl(-k) fl(0.044715)): both terms of p have the same sign, so
          p = p_exact (1 + e) with |e| <= U (c0, or 3 U for c1) + U (v v) + U (fma) <= 5 U, and u' = u (1 + e'), |e'| <= 6 U;
      E' = v_exp_f32(u'): 1 ulp, i.e. within 2 U relative of 2^u' = 2^u 2^(u e') -> E' = E (1 + a), |a| <= 6 U |u| ln 2 + 2 U;
      d  = fl(1 + E') = (1 + E) (1 + b), |b| <= |a| E / (1 + E) + U;
      r  = v_rcp_f32(d): 1 ulp, within 2 U relative of 1 / d;  out = fl(v r): U.
    The 1-ulp accuracy of v_exp_f32 and v_rcp_f32 is the figure of the CDNA ISA guide's instruction descriptions.  Relative error of
    out <= |b| + 3 U to first order; the factor (1 + 2^-10) covers the higher orders (|a| < 2^-15 over [-8, 8]: |u| <= 71.2).
    (+ TINY where v r is an fp32 subnormal)."""
    u = GELU_K * (v.abs() + 0.044715 * v.abs() ** 3)
    E = torch.exp2(-GELU_K * (v + 0.044715 * v ** 3))
    a = 6 * U * u * math.log(2.0) + 2 * U
    b = a * (E / (1.0 + E)) + U
    return g.abs() * (b + 3 * U) * (1 + 2.0 ** -10) + TINY


def gelu_sweep_bias(dtype, bound=8.0):
    """Every finite value of the 16-bit type in [-bound, bound] as a bias vector whose length is a multiple of 256: blocks of 31
    consecutive values of the sweep and one anchor.  The anchor repeats the block's value of largest |gelu| unless that maximum
    lies within SWEEP_MARGIN of a scale boundary; then it is a larger neighbour of that value whose |gelu| does not.  Returns
    (bias [N] of dtype, N); the caller asserts the margin with `boundary_distance`."""
    from gemm_exact_ref import finite_values
    vals = finite_values(dtype, bound)
    nb = (vals.numel() + 30) // 31
    nb = (nb * 32 + 255) // 256 * 256 // 32
    body = torch.cat([vals, vals[:nb * 31 - vals.numel()]]).view(nb, 31)
    gd = gelu_tanh64(body.double()).abs()
    arg = gd.argmax(dim=1, keepdim=True)
    a = body.gather(1, arg)[:, 0].double()
    anchor, best = a.clone(), boundary_distance(gd.amax(dim=1))
    for k in range(1, 17):
        cand = (a * (1 + k / 8)).clamp(-bound, bound).to(dtype).double()
        gm = torch.maximum(gd.amax(dim=1), gelu_tanh64(cand).abs())
        take = (best <= SWEEP_MARGIN) & (boundary_distance(gm) > SWEEP_MARGIN)
        anchor = torch.where(take, cand, anchor)
        best = torch.where(take, boundary_distance(gm), best)
    bias = torch.cat([body, anchor.to(dtype)[:, None]], dim=1).reshape(-1)
    return bias, bias.numel()

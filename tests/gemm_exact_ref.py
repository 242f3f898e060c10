"""Host side of the exact GEMM tests (tests/test_gpu_gemm_edges.py; checked on the CPU by tests/test_gemm_exact_ref.py).

Dyadic operands.  Every operand is a small integer times a fixed power of two, so every product x[m][k] * w[n][k] is an integer
multiple of one quantum q = 2^(x_exp + w_exp), and so are bias, R1 and R2.  While K * max|x| * max|w| + max|bias| stays below 2^24 in
units of q, every partial sum of every summation order is an integer below 2^24 times q: the fp32 accumulator of any GEMM family, tile
geometry or k-split holds it exactly, and so does the fp32 `acc + bias`.  What a kernel stores is then decided by the rounding points of
its epilogue alone, which are the project's numerical specification (csrc/d3pm_generic.hip, linear_tiled):

    v = rn(acc + bias);  v = rn(act(v));  r = R1  or  rn(R1 + R2);  v = rn(r + v);  y = v * mask

`epilogue_chain` evaluates exactly that from the float64 product; a kernel has to reproduce it bit for bit on every element.

Guards.  `guarded` places a [rows, cols] view with row stride `ld` in a storage that is prefilled with a NaN pattern and holds at least
one full tile of rows (>= 192) in front of and behind the view, beside the ld - cols pad columns.  `assert_untouched` compares
everything outside the view with the pattern as integers.  A stray store lands inside the allocation and is seen; a stray load that
reaches a stored element brings a NaN into the result."""
import torch

GUARD_ROWS = 192                       # the tallest GEMM tile
NAN_BITS = {torch.float16: 0x7E55, torch.bfloat16: 0x7FD5, torch.float32: 0x7FC55555, torch.uint8: 0xA5}
_INT_VIEW = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}
SIG_BITS = {torch.float16: 11, torch.bfloat16: 8}
X_RANGE, X_EXP, W_RANGE, W_EXP = 4, -2, 2, -3
# (step, range) in units of the product quantum: value = step * j, |j| <= range, j and step * range representable in the type.
# The bias lifts acc + bias past the significand of the type, R1 and R2 have different steps so that R1 + R2 needs rounding too.
ADDENDS = {torch.bfloat16: {"bias": (16, 127), "r1": (8, 127), "r2": (1, 127)},
           torch.float16: {"bias": (128, 127), "r1": (16, 1023), "r2": (1, 1023)}}
# moments: integers of magnitude <= 64 in all, so that 512 squares of a row sum below 2^24 (and need no rounding in either type)
MOMENT_NNZ, MOMENT_X, MOMENT_BIAS, MOMENT_R = 24, 2, 4, 6


def exactness_bound(K, dtype, moments=False):
    """The largest |partial sum| any summation order of acc + bias can meet, in units of the product quantum."""
    if moments:
        return MOMENT_NNZ * MOMENT_X + MOMENT_BIAS
    step, rng = ADDENDS[dtype]["bias"]
    return K * X_RANGE * W_RANGE + step * rng


def dyadic_operands(M, N, K, dtype, seed, moments=False):
    """x [M, K], w [N, K], bias [N], r1, r2 [M, N] of `dtype` on the CPU (see the module text).  moments = True: integers, every row of w
    with MOMENT_NNZ entries of +-1, so that |x . w + bias + r1 + r2| <= 24 * 2 + 4 + 6 + 6 = 64 by construction."""
    assert exactness_bound(K, dtype, moments) < 2 ** 24, "a partial sum could leave the exact range of the fp32 accumulator"
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()      # noqa: E731
    if moments:
        assert K >= MOMENT_NNZ
        x = ri(-MOMENT_X, MOMENT_X, M, K)
        w = torch.zeros(N, K, dtype=torch.float64)
        cols = torch.rand(N, K, generator=g).argsort(dim=1)[:, :MOMENT_NNZ]
        w.scatter_(1, cols, ri(0, 1, N, MOMENT_NNZ) * 2 - 1)
        out = (x, w, ri(-MOMENT_BIAS, MOMENT_BIAS, N), ri(-MOMENT_R, MOMENT_R, M, N), ri(-MOMENT_R, MOMENT_R, M, N))
    else:
        q = 2.0 ** (X_EXP + W_EXP)
        a = ADDENDS[dtype]
        add = lambda name, *s: ri(-a[name][1], a[name][1], *s) * (a[name][0] * q)      # noqa: E731
        out = (ri(-X_RANGE, X_RANGE, M, K) * 2.0 ** X_EXP, ri(-W_RANGE, W_RANGE, N, K) * 2.0 ** W_EXP, add("bias", N), add("r1", M, N),
               add("r2", M, N))
    cast = tuple(t.to(dtype) for t in out)
    assert all(torch.equal(c.double(), t) for c, t in zip(cast, out)), "an operand is not representable in the storage type"
    return cast


def epilogue_chain(x, w, bias, dtype, act="none", r1=None, r2=None, row_mask=None, mask_period=1, swap_residual_order=False):
    """The stored rows [M, N] of `dtype` that the specification gives for exact products (module text); operands on the CPU.
    swap_residual_order is the WRONG chain rn(rn(R1 + v) + R2), kept for the mutation check of the tests."""
    rn = lambda t: t.to(dtype).double()      # noqa: E731   (a value below 2^24 quanta passes through fp32 unchanged: one rounding)
    acc = x.double() @ w.double().T
    v = rn(acc + (bias.double() if bias is not None else 0.0))
    if act == "relu":
        v = torch.clamp_min(v, 0.0)
    else:
        assert act == "none"
    if r1 is not None:
        if r2 is None:
            v = rn(r1.double() + v)
        elif swap_residual_order:
            v = rn(rn(r1.double() + v) + r2.double())
        else:
            v = rn(rn(r1.double() + r2.double()) + v)
    else:
        assert r2 is None
    if row_mask is not None:
        M = x.shape[0]
        v = v * (row_mask[torch.arange(M) % mask_period] != 0).double()[:, None]      # -v * 0 = -0, as in the kernels
    return v.to(dtype)


def part_moments(y, part=32):
    """float64 (sum, sum of squares) of every `part` columns of the stored rows y: [M, N / part, 2]."""
    M, N = y.shape
    yd = y.double().reshape(M, N // part, part)
    return torch.stack([yd.sum(-1), (yd * yd).sum(-1)], dim=-1)


def _filled(numel, dtype, device):
    return torch.full((numel,), NAN_BITS[dtype], dtype=torch.int32, device=device).to(_INT_VIEW[dtype]).view(dtype)


def guarded(rows, cols, ld, dtype, guard_rows=GUARD_ROWS, device="cpu", fill=None):
    """(storage, view): view [rows, cols] with row stride ld inside a 1-d `storage` of (rows + 2 guard_rows) * ld elements that holds the
    NaN pattern of the type everywhere; `fill` [rows, cols] is copied into the view."""
    assert ld >= cols and guard_rows >= GUARD_ROWS
    storage = _filled((rows + 2 * guard_rows) * ld, dtype, device)
    view = storage.view(-1, ld)[guard_rows:guard_rows + rows, :cols]
    if fill is not None:
        view.copy_(fill)
    return storage, view


def guarded_flat(shape, dtype, guard=4096, device="cpu", fill=None):
    """The same for a contiguous buffer of any shape (a bias, a mask, an fp32 moment buffer): `guard` elements on either side."""
    numel = 1
    for s in shape:
        numel *= s
    storage = _filled(numel + 2 * guard, dtype, device)
    view = storage[guard:guard + numel].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return storage, view


def outside(storage, view):
    """bool [storage.numel()]: True where an element of the storage does not belong to the view."""
    idx = torch.arange(storage.numel()).as_strided(tuple(view.shape), tuple(view.stride()), view.storage_offset() - storage.storage_offset())
    out = torch.ones(storage.numel(), dtype=torch.bool)
    out[idx.reshape(-1)] = False
    return out


def assert_untouched(storage, view, what="", also=None):
    """Everything of `storage` outside `view` still holds the pattern (compared as integers).  also: bool of the view's shape, elements
    INSIDE the view that must hold the pattern too (moment slots of rows that do not exist)."""
    ints = storage.detach().cpu().view(_INT_VIEW[storage.dtype]).to(torch.int64)
    mask = 0xFFFF if storage.dtype in SIG_BITS else 0xFF if storage.dtype == torch.uint8 else 0xFFFFFFFF
    bad = ((ints & mask) != NAN_BITS[storage.dtype]) & outside(storage, view)
    if also is not None:
        inner = view.detach().cpu().contiguous().view(_INT_VIEW[storage.dtype]).to(torch.int64)
        hit = ((inner & mask) != NAN_BITS[storage.dtype]) & also
        assert not hit.any(), f"{what}: {int(hit.sum())} slots inside the buffer that belong to no row were written, first at {hit.nonzero()[0].tolist()}"
    if bad.any():
        first = int(bad.nonzero()[0])
        rel = first - (view.storage_offset() - storage.storage_offset())
        ld = view.stride(0) if view.dim() >= 2 else 1
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the view were written; the first lies {rel} elements from the view's "
                             f"origin (row {rel // ld if ld else 0}, column {rel % ld if ld else rel}, row stride {ld})")


def rn16(x, dtype):
    """float64 -> the 16-bit type with ONE rounding to nearest even (torch converts through fp32, which rounds twice): the fp32
    intermediate is rounded to odd -- truncated towards zero, lowest bit set when inexact -- which the second rounding cannot confuse."""
    f = x.to(torch.float32)
    b = f.view(torch.int32)
    b = torch.where(f.double().abs() > x.abs(), b - 1, b)
    b = torch.where(b.view(torch.float32).double() != x, b | 1, b)
    return b.view(torch.float32).to(dtype)


def ulp_steps(a, b):
    """Representable steps of the (common) 16-bit type between a and b."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


def finite_values(dtype, bound=8.0):
    """Every finite value of the 16-bit type in [-bound, bound], subnormals and both zeros included."""
    top = int(torch.tensor(bound, dtype=dtype).view(torch.int16))
    pos = torch.arange(top + 1, dtype=torch.int32)
    return torch.cat([pos, pos | 0x8000]).to(torch.int16).view(dtype)


# ---- the cases of tests/test_gpu_gemm_edges.py: (M, N, K, the epilogues with R1 apply) per GEMM family ----
SHAPES = {
    "k128": [(129, 136, 64, True), (257, 72, 192, True), (5, 4096, 64, True), (127, 1025, 128, False)],
    "panel64": [(33, 520, 256, True), (97, 200, 512, True), (65, 1025, 256, False)],
    "big": [(192, 512, 256, True), (384, 512, 384, True)],
}
MOMENT_SHAPES = [(200, 512, 64), (1000, 512, 256), (384, 512, 256)]
FOLD_SHAPES = {"k128": (129, 136, 256), "panel64": (33, 520, 256), "big": (192, 512, 512)}
BK, KC = 64, 256      # csrc/d3pm_plan.h


def k128_ok(M, N, K, ldx, ldy, ldr=None):
    """csrc/d3pm_plan.cpp k128_ok for 16-bit operands at 16-byte aligned addresses (ldr: None = no residual)."""
    return K >= BK and K % BK == 0 and ldx % 8 == 0 and ldy % 8 == 0 and (ldr is None or (ldr % 8 == 0 and N % 8 == 0)) and M * N >= 128 * 128


def panel64_ok(M, N, K, ldx, ldy, ldr=None):
    return N >= 16 and K >= KC and K % KC == 0 and ldx % 8 == 0 and ldy % 8 == 0 and (ldr is None or (ldr % 8 == 0 and N % 8 == 0))


def big_tile(M, N, K, variant):
    """the geometry gemm_variant 6 / 7 / 8 forces where the shape is made of its whole tiles, else None (d3pm_plan.cpp big_tile)"""
    tm, tn = {6: (192, 256), 7: (96, 512), 8: (192, 128), 9: (96, 128), 10: (128, 128)}[variant]
    return (tm, tn) if K >= 4 * BK and K % (2 * BK) == 0 and M % tm == 0 and N % tn == 0 else None

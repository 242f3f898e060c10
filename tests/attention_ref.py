"""The attention contract of d3pm_kernels.h (AttnArgs) in float64, and the crafted inputs whose answer is known per key.  Shared by
tests/test_attention_ref_api.py (CPU) and tests/test_gpu_attention_exact.py; not a test module.

Layouts: q [B, Tq, H * 64], k / v [B, S, H * 64] torch tensors of a 16-bit type on the CPU (head_dim is 64 throughout), probability
matrices [B, H, Tq, S] in float64.

Three kinds of input:
  * selector inputs -- the softmax is one-hot far below fp32 rounding, so every schedule must return one V row unchanged;
  * probe values -- V is a slice of the identity, so the output IS the probability matrix the kernel used, one 64-key block per launch;
  * flat / steered scores -- N(0, sigma^2) inputs, optionally with one coordinate that moves the scores of whole 64-key tiles by a
    chosen log2-domain offset (the deferred running maximum of the flash kernels moves when a tile exceeds it by 2^8).

The bound on a recovered probability (`probability_bound`, `check_probabilities`) is derived from the contract
    P = rn(softmax(rn(rn(q * scale) . k))),  O = rn(P . V),  rn = round to the storage type, unit roundoff u (2^-9 bf16, 2^-12 fp16)
and from nothing a kernel returned.  With A_i = max_j scale * sum_c |q_ic| |k_jc|:
  * rn(q * scale) moves every score of query i by at most u A_i, the 16-bit score (generic family) by at most u |s_ij| <= u A_i more.
    The MFMA family rounds q * scale * log2(e) instead and keeps fp32 scores: one of the two terms.  So |ds_ij| <= 2 u A_i.
  * p_ij = e^s_ij / sum_j e^s_ij with every exponent off by at most 2 u A_i in either direction is off by at most the factor
    e^(4 u A_i), i.e. relatively by e^(2 * 2 u A_i) - 1.
  * rn of P, rn of the output and the ratio against a sum of equally perturbed terms (the flash kernels divide the rounded
    probabilities by a sum of rounded -- or, on the 32 x 32 x 16 instruction, unrounded -- ones) add at most 4 u.
  => |p^_ij - p_ij| <= (e^(4 u A_i) - 1 + 4 u) p_ij.
This holds where the 16-bit P register is a normal number.  The flash kernels hold 2^(s_ij - m_ref) with m_ref <= the row maximum,
so the register is >= p_ij / max_j p_ij: entries with p_ij >= 2^-12 max_j p_ij are in this "relative class" for fp16 (bf16 has
fp32's exponent range).  Smaller entries must merely stay small: p^_ij <= 2^-11 max_j p_ij.  Where the NORMALISED p_ij is below
twice the smallest normal number of the storage type, rn(P) of the generic family and rn(O) of every family are subnormal
roundings with an absolute error of half a quantum each: one quantum (2^-24 fp16) is added to both classes there.
float32 (generic family only, the key-mask test): u = 2^-24 and the fp32 arithmetic is no longer negligible -- the 64-term FMA
chain moves a score by at most (64 + 2) u A_i, expf (1 ulp = 2 u) enters numerator and denominator, the sum of S terms goes over
ceil(S / 64) additions per lane and 6 shuffle steps: (e^(2 * 66 u A_i) - 1) + (4 + 4 + ceil(S / 64) + 6) u.
"""
import math

import torch

HD = 64
TILE = 64
LOG2E = 1.4426950408889634
K_DEFER = 8.0          # the flash kernels raise their running reference when a tile exceeds it by 2^8


def unit_roundoff(dtype) -> float:
    return {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12, torch.float32: 2.0 ** -24}[dtype]


def subnormal_quantum(dtype) -> float:
    return {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24, torch.float32: 2.0 ** -149}[dtype]


def smallest_normal(dtype) -> float:
    return float(torch.finfo(dtype).tiny)


def heads(x: torch.Tensor) -> torch.Tensor:
    """[B, T, H * 64] of any float type -> float64 [B, H, T, 64] (exact upcast)."""
    B, T, d = x.shape
    return x.to(torch.float64).view(B, T, d // HD, HD).transpose(1, 2)


def unheads(x: torch.Tensor) -> torch.Tensor:
    """[B, H, T, 64] -> [B, T, H * 64]."""
    B, H, T, hd = x.shape
    return x.transpose(1, 2).reshape(B, T, H * hd)


def _key_mask(key_len, B, S):
    """bool [B, 1, 1, S]: key j of utterance b is valid."""
    if key_len is None:
        return torch.ones(B, 1, 1, S, dtype=torch.bool)
    kl = torch.as_tensor(key_len, dtype=torch.int64).view(B, 1, 1, 1)
    return torch.arange(S).view(1, 1, 1, S) < kl


def scores_fp64(q, k, scale):
    """scale * q . k per head in float64, natural-log domain: [B, H, Tq, S]."""
    return (heads(q) @ heads(k).transpose(-1, -2)) * float(scale)


def softmax_fp64(q, k, scale, key_len=None):
    """P [B, H, Tq, S] in float64 from the 16-bit (or fp32) inputs upcast: no other rounding.  Masked keys get exactly 0."""
    s = scores_fp64(q, k, scale)
    s = s.masked_fill(~_key_mask(key_len, s.shape[0], s.shape[-1]), float("-inf"))
    return torch.softmax(s, dim=-1)


def attention_fp64(q, k, v, scale, key_len=None):
    """softmax_fp64 . V in float64: [B, Tq, H * 64]."""
    return unheads(softmax_fp64(q, k, scale, key_len) @ heads(v))


# ---- selector inputs ------------------------------------------------------------------------------------------------------
def selector_order(Tq: int, S: int, reverse: bool = False) -> torch.Tensor:
    """pi(i) = i mod S, or S - 1 - (i mod S): the key that query i selects."""
    pi = torch.arange(Tq) % S
    return S - 1 - pi if reverse else pi


def selector_inputs(B, H, Tq, S, dtype, seed, reverse=False):
    """K rows = +-4 sign codes drawn independently per (utterance, head); query i = K row pi(i).  Every value is exact in fp16 and
    bf16.  Returns (q, k, pi, gap): gap [B, H, Tq] is the log2-domain distance between the selected key's score and the next one
    from the float64 scores at `scale` = 1 / 8 (inf for S = 1)."""
    g = torch.Generator().manual_seed(seed)
    k = (torch.randint(0, 2, (B, S, H * HD), generator=g).to(torch.float32) * 8.0 - 4.0).to(dtype)
    pi = selector_order(Tq, S, reverse)
    q = k[:, pi, :].clone()
    s = scores_fp64(q, k, 0.125) * LOG2E
    top = torch.topk(s, min(2, S), dim=-1).values
    sel = torch.gather(s, -1, pi.view(1, 1, Tq, 1).expand(B, H, Tq, 1))[..., 0]
    gap = sel - top[..., 1] if S > 1 else torch.full_like(sel, float("inf"))
    assert torch.equal(sel, top[..., 0]), "a selector query does not score highest on its own key"
    return q, k, pi, gap


# ---- probe values ---------------------------------------------------------------------------------------------------------
def probe_values(B, S, H, blk, dtype):
    """V[b, j, h * 64 + c] = 1 where j // 64 == blk and j % 64 == c, else 0: the output of a launch is then the block `blk` of the
    probability matrix, O[b, i, h * 64 + c] = P[b, h, i, 64 blk + c], rounded once to the storage type."""
    v = torch.zeros(B, S, H, HD, dtype=dtype)
    j = torch.arange(blk * TILE, min((blk + 1) * TILE, S))
    v[:, j, :, j - blk * TILE] = 1
    return v.view(B, S, H * HD)


def n_blocks(S: int) -> int:
    return (S + TILE - 1) // TILE


def recover_probabilities(run, B, S, H, dtype):
    """run(v) -> O [B, Tq, H * 64] (any device) for v = probe_values(.., blk, ..), once per 64-key block -> float64 [B, H, Tq, S]: the
    normalised probability every key had in the launch."""
    cols = []
    for blk in range(n_blocks(S)):
        o = run(probe_values(B, S, H, blk, dtype))
        cols.append(heads(o.detach().cpu()))
    return torch.cat(cols, dim=-1)[..., :S]


# ---- flat and steered scores ----------------------------------------------------------------------------------------------
def flat_inputs(B, H, Tq, S, dtype, seed, sigma=0.7):
    """q, k ~ N(0, sigma^2) rounded to `dtype`: a nearly flat softmax (a key carries about 1 / S of the mass)."""
    g = torch.Generator().manual_seed(seed)
    q = (sigma * torch.randn(B, Tq, H * HD, generator=g)).to(dtype)
    k = (sigma * torch.randn(B, S, H * HD, generator=g)).to(dtype)
    return q, k


FAMILIES = {                       # log2-domain step of the scores from one 64-key tile to the next (the first entry: tile 0 itself)
    "all_negative": [-60.0, 0.0, 0.0, 0.0, 0.0],
    "falling": [-7.5] * 5,
    "rising_under": [7.5] * 5,
    "rising_over": [8.5] * 5,
    "up_then_down": [8.5, 8.5, -12.0, -12.0, -12.0],
}
STEER_Q = 8.0                      # the constant in the steered coordinate of q (exact in both types)


def steered_inputs(family, B, H, Tq, S, dtype, seed, scale=0.125, sigma=0.5):
    """Flat inputs whose coordinate 0 of every head is steered: q holds STEER_Q, k a per-tile constant, so the float64 log2-domain
    score of key j is offset[j // 64] plus the flat part's noise (a few units).  Returns (q, k, offsets): the offsets actually
    obtained after the 16-bit rounding of k, one per tile."""
    q, k = flat_inputs(B, H, Tq, S, dtype, seed, sigma)
    want = torch.tensor(FAMILIES[family][:n_blocks(S)], dtype=torch.float64).cumsum(0)
    kc = (want / (STEER_Q * scale * LOG2E)).to(dtype)
    q = q.view(B, Tq, H, HD).clone()
    k = k.view(B, S, H, HD).clone()
    q[..., 0] = STEER_Q
    k[..., 0] = kc[torch.arange(S) // TILE].view(1, S, 1)
    got = kc.to(torch.float64) * (STEER_Q * scale * LOG2E)
    return q.view(B, Tq, H * HD), k.view(B, S, H * HD), got


def steps_on_intended_side(family, offsets) -> bool:
    """Every tile-to-tile step of the realised offsets lies on the same side of the deferral threshold as the intended one."""
    want = FAMILIES[family][1:len(offsets)]
    got = (offsets[1:] - offsets[:-1]).tolist()
    return all((g > K_DEFER) == (w > K_DEFER) and (g < 0) == (w < 0) for g, w in zip(got, want))


# ---- the bound ------------------------------------------------------------------------------------------------------------
def probability_bound(q, k, scale, dtype, key_len=None):
    """The relative tolerance of the module docstring per query: float64 [B, H, Tq, 1]."""
    u = unit_roundoff(dtype)
    a = (heads(q).abs() @ heads(k).abs().transpose(-1, -2)) * float(scale)
    B, S = a.shape[0], a.shape[-1]
    a = a.masked_fill(~_key_mask(key_len, B, S), 0.0).amax(dim=-1, keepdim=True)
    if dtype == torch.float32:
        return torch.expm1(2.0 * (HD + 2) * u * a) + (4 + 4 + n_blocks(S) + 6) * u
    return torch.expm1(4.0 * u * a) + 4.0 * u


class Report:
    """What check_probabilities found: worst_ratio = max |p^ - p| / tolerance over the relative class (<= 1 passes) at `worst_at` =
    (b, h, i, j); frac_relative = share of the entries in that class; small_violations = entries of the small class above their cap;
    row_sum_err = max |sum_j p^_ij - 1| and its limit S u."""

    def __init__(self, worst_ratio, worst_at, frac_relative, small_violations, row_sum_err, row_sum_limit):
        self.worst_ratio, self.worst_at, self.frac_relative = worst_ratio, worst_at, frac_relative
        self.small_violations, self.row_sum_err, self.row_sum_limit = small_violations, row_sum_err, row_sum_limit

    @property
    def ok(self):
        return self.worst_ratio <= 1.0 and self.small_violations == 0 and self.row_sum_err <= self.row_sum_limit

    def __str__(self):
        return (f"worst error / bound {self.worst_ratio:.3f} at (b, h, i, j) = {self.worst_at}, {self.frac_relative:.2%} of the entries in "
                f"the relative class, {self.small_violations} small entries above their cap, row sums off by {self.row_sum_err:.2e} "
                f"(limit {self.row_sum_limit:.2e})")


def check_probabilities(p_hat, p_ref, rel, dtype) -> Report:
    """p_hat (recovered, float64) against p_ref (softmax_fp64) under rel (probability_bound).  Never raises: the caller asserts on
    the report, and a mutation test asserts on WHERE it failed."""
    u, quantum, tiny = unit_roundoff(dtype), subnormal_quantum(dtype), smallest_normal(dtype)
    pmax = p_ref.amax(dim=-1, keepdim=True)
    relative = p_ref >= 2.0 ** -12 * pmax
    floor = torch.where(p_ref < 2.0 * tiny, quantum, 0.0)
    err = (p_hat - p_ref).abs()
    ratio = torch.where(relative, err / (rel * p_ref + floor), torch.zeros_like(err))
    ratio = torch.where(torch.isfinite(p_hat), ratio, torch.full_like(ratio, float("inf")))
    flat = int(ratio.argmax())
    at = tuple(int(x) for x in torch.unravel_index(torch.tensor(flat), ratio.shape))
    small_bad = int(((~relative) & ~(p_hat <= 2.0 ** -11 * pmax + floor)).sum())
    S = p_ref.shape[-1]
    return Report(float(ratio.flatten()[flat]), at, float(relative.double().mean()), small_bad,
                  float((p_hat.sum(-1) - 1.0).abs().max()), S * u)


# ---- the contract on the CPU, with the mistakes a kernel can make ------------------------------------------------------------
MUTATIONS = ("drop_last_key", "double_last_key", "shift_keys_in_last_tile", "swap_value_tiles", "no_rescale")


def _rn(x, dtype):
    return x.to(dtype).to(torch.float32)


def emulate(q, k, v, scale, dtype, order="eager", mutation=None):
    """The contract with its 16-bit rounding points and fp32 accumulation on the CPU -> O [B, Tq, H * 64] of `dtype`.
    order "eager": P = rn(softmax(rn(rn(q scale) . k))), O = rn(P . V) -- the generic family.
    order "tiled": 64-key tiles with a deferred running maximum, q pre-scaled by scale * log2(e), fp32 scores, un-normalised 16-bit
    probabilities, fp32 row sum divided out at the end -- the flash kernels.
    mutation: one of MUTATIONS (swap_value_tiles exchanges tiles 0 and 1; no_rescale exists in the tiled order only)."""
    assert mutation is None or mutation in MUTATIONS
    qh, kh, vh = (heads(t).to(torch.float32) for t in (q, k, v))
    S = kh.shape[2]
    last0 = (n_blocks(S) - 1) * TILE
    k_idx, v_idx = torch.arange(S), torch.arange(S)
    if mutation == "drop_last_key":
        k_idx, v_idx = k_idx[:-1], v_idx[:-1]
    elif mutation == "double_last_key":
        k_idx, v_idx = torch.cat([k_idx, k_idx[-1:]]), torch.cat([v_idx, v_idx[-1:]])
    elif mutation == "shift_keys_in_last_tile":
        k_idx = torch.where(k_idx >= last0, (k_idx + 1).clamp(max=S - 1), k_idx)
    elif mutation == "swap_value_tiles":
        assert S >= 2 * TILE
        v_idx = torch.cat([v_idx[TILE:2 * TILE], v_idx[:TILE], v_idx[2 * TILE:]])
    kh, vh = kh[:, :, k_idx], vh[:, :, v_idx]
    n = kh.shape[2]
    if order == "eager":
        assert mutation != "no_rescale"
        s = _rn(_rn(qh * scale, dtype) @ kh.transpose(-1, -2), dtype)
        p = _rn(torch.softmax(s, dim=-1), dtype)
        return unheads(p @ vh).to(dtype)
    assert order == "tiled"
    s = _rn(qh * (scale * LOG2E), dtype) @ kh.transpose(-1, -2)
    m = l = acc = None
    for t0 in range(0, n, TILE):
        st, vt = s[..., t0:t0 + TILE], vh[:, :, t0:t0 + TILE]
        mx = st.amax(dim=-1, keepdim=True)
        if t0 == 0:
            m, l, acc = mx, torch.zeros_like(mx), torch.zeros(*mx.shape[:-1], HD)
        elif bool((mx - m > K_DEFER).any()):
            delta = (mx - m).clamp(min=0.0)
            if mutation != "no_rescale":
                alpha = torch.exp2(-delta)
                l, acc = l * alpha, acc * alpha
            m = m + delta
        p = _rn(torch.exp2(st - m), dtype)
        l = l + p.sum(-1, keepdim=True)
        acc = acc + p @ vt
    return unheads(acc / l).to(dtype)

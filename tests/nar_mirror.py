"""Host-side mirrors of the three kernels of the stock NAR stage (csrc/d3pm_nar.hip), beside key_mask_mirror.py and attention_ref.py:
plain torch / numpy restatements of the rule each kernel's comment documents, and the inputs the kernel tests run them on
(tests/test_gpu_nar_kernels.py on the GPU, tests/test_nar_mirror.py for the mirrors themselves).  No GPU here.

  embed_mirror   nar_embed_rows: text rows rn(W_text[id] + pe[pos]); a sep row at pos == tt and at pos == tt + 1 + tp; prompt / response
                 rows rn(rn(acc) + pe[pos]) with acc the fp32 sum over the levels in ascending order (a prompt level with a code < 0 is
                 skipped); ids clamped into [0, n_tokens - 1]; rows at or past `total` zero; row_mask = pos < total; key_len = total.
  adaln_mirror   adaln_rows: row mean and variance in float64 (two passes, eps = 1e-5), then the kernel's chain with every rounding to
                 the storage type: h, k h, 1 - ., c ., . h, exp(log gamma), g a, + beta.  Masked rows zero.
  draw_mirror    nar_sample_rows: z = rn(float(logit) / float32(T)); greedy = first index of the maximum; otherwise the first-index
                 argmax of z + gumbel(u) in float64 with u from oracle/philox.py, and the margin between the best and the second best.

rn() is the round-to-nearest-even conversion to the storage type; for fp32 it does nothing."""
import math

import numpy as np
import torch

from oracle import nar_oracle as N
from oracle import philox

ADALN_K, ADALN_C, ADALN_EPS = 0.1, 2.0, 1e-5
STORAGE_EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}


def rn(v: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 values after a store in `dtype`, back in fp32."""
    assert v.dtype == torch.float32
    return v if dtype == torch.float32 else v.to(dtype).float()


# ---- nar_embed_rows ---------------------------------------------------------------------------------------------------------------
def embed_mirror(lens, text, prom, resp, n_given, w_text, w_prom, w_resp, sep, pe, t_max):
    """lens [B, 3], text [B, tt_max], prom [B, tp_max, L], resp [B, tr_max, stride] integer tensors; tables of one dtype T.
    Returns (x [B, t_max, d] of T, row_mask uint8 [B, t_max], key_len int32 [B]).  Slots past an utterance's own lengths and
    response columns from n_given on are never looked at."""
    dtype, (n_tokens, d) = w_text.dtype, w_text.shape
    B = lens.shape[0]
    x = torch.zeros(B, t_max, d, dtype=dtype)
    row_mask = torch.zeros(B, t_max, dtype=torch.uint8)
    key_len = torch.zeros(B, dtype=torch.int32)

    def level_sum(table, codes, skip_negative):           # codes [t, l] -> rn(acc) [t, d], acc in fp32, levels ascending
        acc = torch.zeros(codes.shape[0], d, dtype=torch.float32)
        for l in range(codes.shape[1]):
            rows = table[l][codes[:, l].clamp(0, n_tokens - 1)].float()
            acc = torch.where((codes[:, l] >= 0)[:, None], acc + rows, acc) if skip_negative else acc + rows
        return rn(acc, dtype)

    for b in range(B):
        tt, tp, tr = (int(v) for v in lens[b])
        total = tt + tp + tr + 2
        key_len[b] = total
        row_mask[b, :min(total, t_max)] = 1
        rows = torch.cat([w_text[text[b, :tt].long().clamp(0, n_tokens - 1)].float(), sep[None].float(),
                          level_sum(w_prom, prom[b, :tp].long(), True), sep[None].float(),
                          level_sum(w_resp, resp[b, :tr, :n_given].long(), False)])
        n = min(total, t_max)
        x[b, :n] = rn(rows[:n] + pe[:n].float(), dtype).to(dtype)
    return x, row_mask, key_len


EMBED_LENS = ((1, 1, 1), (7, 9, 13), (4, 6, 5), (3, 2, 4))      # total 5, 31 (= t_max - 5), 17, 11
EMBED_MAX = (10, 12, 16)                                        # tt_max, tp_max, tr_max: above every utterance's own lengths
EMBED_TOKENS, EMBED_LEVELS, EMBED_STRIDE = 64, 8, 8


def embed_inputs(d, dtype, n_given, poison=9999):
    """The ragged batch of four of the embedding tests.  Every code slot the kernel must not read holds `poison`, an id far outside
    the tables: text / prompt / response slots past an utterance's own lengths and response columns from n_given on."""
    g = torch.Generator().manual_seed(1000 + d)
    K, L = EMBED_TOKENS, EMBED_LEVELS
    tables = dict(w_text=torch.randn(K, d, generator=g), w_prom=torch.randn(L, K, d, generator=g),
                  w_resp=torch.randn(EMBED_STRIDE - 1, K, d, generator=g), sep=torch.randn(d, generator=g))
    tables = {k: v.to(dtype) for k, v in tables.items()}
    B = len(EMBED_LENS)
    tt_max, tp_max, tr_max = EMBED_MAX
    text = torch.full((B, tt_max), poison, dtype=torch.int32)
    prom = torch.full((B, tp_max, L), poison, dtype=torch.int32)
    resp = torch.full((B, tr_max, EMBED_STRIDE), poison, dtype=torch.int32)
    for b, (tt, tp, tr) in enumerate(EMBED_LENS):
        text[b, :tt] = torch.randint(0, K, (tt,), generator=g, dtype=torch.int32)
        prom[b, :tp] = torch.randint(0, K, (tp, L), generator=g, dtype=torch.int32)
        resp[b, :tr, :n_given] = torch.randint(0, K, (tr, n_given), generator=g, dtype=torch.int32)
    # ids outside the table are clamped: below zero and above n_tokens - 1, in the text and in the response (in the prompt a
    # negative code means "level absent", so only the upper side can be clamped there)
    text[1, 2], text[1, 5], text[2, 0] = -3, K, 1000
    resp[1, 4, 0], resp[1, 7, n_given - 1], resp[2, 1, 0] = -1, K + 5, -2 ** 31
    prom[1, 3, 2] = K
    # whole prompt levels absent: utterance 2 has four levels, utterance 3 only level 0 and level 5; one row of utterance 1 has none
    prom[2, :6, 4:] = -1
    prom[3, :2, 1:5] = -1
    prom[3, :2, 6:] = -1
    prom[1, 6, :] = -1
    t_max = max(sum(l) + 2 for l in EMBED_LENS) + 5
    pe = N.sinusoid_pe(t_max, d, torch.float32).to(dtype)
    return dict(lens=torch.tensor(EMBED_LENS, dtype=torch.int32), text=text, prom=prom, resp=resp, n_given=n_given, pe=pe, t_max=t_max,
                **tables)


def repoison(inp, poison):
    """The same inputs with another value in every slot that must not be read."""
    out = dict(inp)
    for name in ("text", "prom", "resp"):
        out[name] = inp[name].clone()
    for b, (tt, tp, tr) in enumerate(EMBED_LENS):
        out["text"][b, tt:] = poison
        out["prom"][b, tp:] = poison
        out["resp"][b, tr:] = poison
        out["resp"][b, :, inp["n_given"]:] = poison
    return out


# ---- adaln_rows / adaln_rows_vec ---------------------------------------------------------------------------------------------------
def adaln_mirror(x, emb_row, row_mask, *, stats=torch.float64, rstd_ulps=0, eps=ADALN_EPS):
    """x [M, d], emb_row [2 d] of one storage type T, row_mask [M].  16-bit T: the kernel's chain in fp32 with every rounding, the row
    moments from float64 (stats=torch.float32: from fp32 sums, rstd_ulps: rstd moved by that many fp32 steps -- the two knobs of the
    mirror-against-mirror measurement).  fp32 T: the whole expression in float64, nothing rounded; returns float64."""
    dtype, (M, d) = x.dtype, x.shape
    live = row_mask.bool()[:, None]
    xs = x.to(stats)
    mean = xs.mean(-1, keepdim=True)
    var = ((xs - mean) ** 2).mean(-1, keepdim=True)
    if dtype == torch.float32:
        xd, e = x.double(), emb_row.double()
        h = (xd - mean.double()) / torch.sqrt(var.double() + eps)
        y = e[:d].exp() * (ADALN_C * (1 - ADALN_K * h) * h) + e[d:]
        return torch.where(live, y, torch.zeros_like(y))
    mean32 = mean.float()
    rstd32 = (1.0 / torch.sqrt(var.double() + eps)).float() if stats == torch.float64 else torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    if rstd_ulps:
        r = rstd32.numpy()
        for _ in range(abs(rstd_ulps)):
            r = np.nextafter(r, np.float32(math.inf if rstd_ulps > 0 else 0.0))
        rstd32 = torch.from_numpy(r)
    k, c, one = (torch.tensor(v, dtype=torch.float32) for v in (ADALN_K, ADALN_C, 1.0))
    h = rn((x.float() - mean32) * rstd32, dtype)
    a = rn(k * h, dtype)
    a = rn(one - a, dtype)
    a = rn(c * a, dtype)
    a = rn(a * h, dtype)
    gam = rn(torch.exp(emb_row[:d].float()), dtype)
    y = rn(rn(gam * a, dtype) + emb_row[d:].float(), dtype)
    return torch.where(live, y, torch.zeros_like(y)).to(dtype)


ADALN_ROWS = 1027      # M = 1 and M = 5 are the leading rows of the same tensor
ADALN_LEVEL = 3        # the row of the [8][2 d] table the tests hand to the kernel
SMALL_SIGMA = 1e-2


def adaln_row_kinds(M=ADALN_ROWS):
    """kind per row: 0 = sigma in [0.5, 3.5] and |mean| <= 10; 1 = sigma 1e-2 (eps = 1e-5 is 10 % of the variance); 2 = mean = 100 sigma
    (one-pass variance in fp32 would cancel); 3 = constant (h = 0).  The first five rows hold one of each and a masked one."""
    kind = torch.zeros(M, dtype=torch.int64)
    kind[1], kind[2], kind[3] = 1, 2, 3
    kind[64:96] = 1
    kind[128:136] = 2
    kind[200:204] = 3
    kind[M - 1] = 1                                     # the last row of the ragged last workgroup can see eps too
    mask = torch.ones(M, dtype=torch.uint8)
    mask[4] = 0
    mask[7::4] = 0                                      # about a quarter of the rows
    mask[M - 1] = 1
    return kind, mask


def adaln_inputs(d, dtype):
    """x [1027, d], the [8][2 d] table and the row mask of the AdaLN tests."""
    g = torch.Generator().manual_seed(2000 + d)
    M = ADALN_ROWS
    kind, mask = adaln_row_kinds(M)
    sigma = 0.5 + 3.0 * torch.rand(M, generator=g)
    mean = 20.0 * torch.rand(M, generator=g) - 10.0
    sigma = torch.where(kind == 1, torch.full_like(sigma, SMALL_SIGMA), sigma)
    mean = torch.where(kind == 1, mean * 5e-3, mean)                       # |mean| <= 0.05: sixteen-bit storage still resolves sigma
    sigma = torch.where(kind == 2, torch.full_like(sigma, 0.25), sigma)
    mean = torch.where(kind == 2, 100.0 * sigma, mean)
    x = mean[:, None] + sigma[:, None] * torch.randn(M, d, generator=g)
    const = (torch.round(mean * 4) / 4)[:, None].expand(M, d)              # a short constant: its fp32 row sum is exact
    x = torch.where((kind == 3)[:, None], const, x)
    table = (0.3 * torch.randn(8, 2 * d, generator=g)).to(dtype)
    # exp(log gamma) is the one transcendental per column, and one rounded value of it serves a whole column: a device expf one fp32
    # step away from torch's must not be able to move it, so a log gamma whose exponential sits within 4 fp32 steps of a rounding
    # boundary of the storage type is nudged away
    while dtype != torch.float32:
        lg = table[:, :d]
        near = exp_near_boundary(lg, dtype)
        if not near.any():
            break
        lg[near] = (lg[near].float() * 1.01 + 1e-3).to(dtype)
    return x.to(dtype), table, mask, kind


def exp_near_boundary(lg, dtype, steps=4):
    e = torch.exp(lg.double())
    at = e.float().to(dtype)
    return ((e * (1.0 + steps * 2.0 ** -24)).float().to(dtype) != at) | ((e * (1.0 - steps * 2.0 ** -24)).float().to(dtype) != at)


def lp_error(got, ref, dtype):
    """(share of elements whose bits differ, worst error in storage ulps under the scale of test_gpu_kernels.assert_close_lp)."""
    differ = (got != ref).float().mean().item()
    ref32 = ref.float()
    scale = ref32.abs().clamp_min(ref32.abs().max() * 1e-3)
    worst = ((got.float() - ref32).abs() / scale).max().item() / STORAGE_EPS[dtype]
    return differ, worst


# ---- nar_sample_rows --------------------------------------------------------------------------------------------------------------
def gumbel64(u: np.ndarray) -> np.ndarray:
    u = np.clip(u.astype(np.float64), np.finfo(np.float32).tiny, 1.0)
    return -np.log(-np.log(u))


def draw_values(logits, temperature, *, greedy=False, seed=0, level=0, utt=0, rounded=True, fp32_noise=False):
    """The values the draw compares, float64 [tr, n_tokens]: z, or z + gumbel(u)."""
    tr, n_tokens = logits.shape
    z = torch.from_numpy(logits.float().numpy() / np.float32(temperature))
    if rounded:
        z = rn(z, logits.dtype)
    if greedy:
        return z.double().numpy()
    u = philox.uniform_rows(seed, level, utt * 65536, tr, n_tokens, N.STREAM_NAR)
    if fp32_noise:
        ut = torch.clamp(torch.from_numpy(u), min=torch.finfo(torch.float32).tiny, max=1.0)
        return (z - torch.log(-torch.log(ut))).double().numpy()
    return z.double().numpy() + gumbel64(u)


def draw_mirror(logits, temperature, **how):
    """logits [tr, n_tokens] of a storage type T, the response rows of utterance `utt` (= utt0 + b).  Returns (ids int64 [tr],
    margin float64 [tr] between the best and the second best value).  rounded=False leaves z = float(logit) / T unrounded;
    fp32_noise=True evaluates z + gumbel(u) in fp32 with the oracle's own torch expression instead of float64 (the two switches of
    the comparison with oracle.nar_oracle.sample_gumbel)."""
    v = draw_values(logits, temperature, **how)
    tr, n_tokens = v.shape
    ids = np.argmax(v, axis=-1)                      # the first index of the maximum
    if n_tokens > 1:
        top = np.partition(v, n_tokens - 2, axis=-1)[:, -2:]
        with np.errstate(invalid="ignore"):
            margin = np.nan_to_num(top[:, 1] - top[:, 0], nan=0.0, posinf=np.inf)      # -inf - -inf: no margin at all
    else:
        margin = np.full(tr, np.inf)
    return ids.astype(np.int64), margin


def margin_ulps(logits, temperature, **how):
    """The margin of every row in fp32 steps of the winning value's magnitude."""
    v = draw_values(logits, temperature, **how)
    _, margin = draw_mirror(logits, temperature, **how)
    return margin / np.spacing(np.abs(v.max(axis=-1)).astype(np.float32)).astype(np.float64)


DRAW_TR, DRAW_TR_MAX, DRAW_CUT = (700, 1, 333), 704, 5
DRAW_LENS = ((3, 4, 700), (2, 1, 1), (5, 6, 333))
DRAW_T_MAX = DRAW_LENS[0][0] + DRAW_LENS[0][1] + 2 + DRAW_TR[0] - DRAW_CUT      # the last 5 frames of utterance 0 are outside the grid
DRAW_PAD, DRAW_PAD_VALUE, DRAW_TEMPERATURE = 8, 60000.0, 0.2
DRAW_SEEDS = (23, 1023)       # Philox seeds of the Gumbel tests: no row of the inputs within 64 fp32 steps of a tie (test_nar_mirror.py)
DRAW_RUNS = ((23, 0), (23, 5), (1023, 0))      # (seed, level) of every Gumbel launch


def draw_frames(b):
    """Frames of utterance b whose grid row exists."""
    tt, tp, tr = DRAW_LENS[b]
    return min(tr, DRAW_T_MAX - (tt + tp + 2))


def draw_inputs(n_tokens, dtype, special=True):
    """The padded logits grid [3, t_max, n_tokens + 8] of the draw tests: randn * 3 on the response rows, +60000 in the pad columns
    (a read past n_tokens wins the race), other random numbers on every row that is no response row.  With special=True (the greedy test) some rows
    carry a duplicated maximum at two classes that different lanes own in different passes (the first must win), constant rows,
    -inf classes, one row that is -inf throughout, and every fifth row a pair of neighbouring logits on top (rounding_pairs)."""
    g = torch.Generator().manual_seed(3000 + n_tokens)
    ldl = n_tokens + DRAW_PAD
    grid = 3.0 * torch.randn(len(DRAW_LENS), DRAW_T_MAX, ldl, generator=g)
    hi, lo = (700, 3) if n_tokens > 700 else (n_tokens - 1, 1)
    for b, (tt, tp, tr) in enumerate(DRAW_LENS):
        n = draw_frames(b)
        rows = 3.0 * torch.randn(n, n_tokens, generator=g)
        if special and n > 1:
            f = torch.arange(n)
            dup = f % 7 == 2
            rows[dup, hi] = 40.0
            rows[dup, lo] = 40.0
            rows[f % 11 == 5] = 1.25
            rows[(f % 13 == 6)[:, None] & (torch.arange(n_tokens) % 3 == 0)[None]] = -math.inf
            rows[f == 17] = -math.inf
        grid[b, tt + tp + 2: tt + tp + 2 + n, :n_tokens] = rows
    grid[:, :, n_tokens:] = DRAW_PAD_VALUE
    grid = grid.to(dtype)
    if special:
        # rows on which the rounding of logit / T decides: the largest logit a sits at a later class than its predecessor a' in the
        # storage type, and rn(a / T) == rn(a' / T) -- the rounded rule names the earlier class, argmax(logit / T) the later one
        # (fp32 rounds nothing: there the later class wins under both)
        pairs = rounding_pairs(dtype)
        for b, (tt, tp, tr) in enumerate(DRAW_LENS):
            for f in range(0, draw_frames(b), 5):
                if f % 7 == 2 or f % 11 == 5 or f % 13 == 6 or f == 17 or draw_frames(b) == 1:
                    continue
                first, later = (130 + f % 50, 900 - f % 37) if n_tokens > 900 else (2, 4)
                grid[b, tt + tp + 2 + f, first], grid[b, tt + tp + 2 + f, later] = pairs[f % len(pairs)]
    return grid


def rounding_pairs(dtype, temperature=DRAW_TEMPERATURE, lo=26.0, hi=31.0):
    """(a', a): neighbouring values of the storage type above every randn * 3 logit whose quotients by T round to one value."""
    if dtype == torch.float32:
        a = torch.arange(lo, hi, 0.125)
        return list(zip(np.nextafter(a.numpy(), np.float32(0)).tolist(), a.tolist()))
    step = STORAGE_EPS[dtype] * 16.0                         # the spacing of the storage type in [16, 32)
    a = torch.arange(lo + step, hi, step, dtype=torch.float64)
    z = lambda t: rn(torch.from_numpy(t.float().numpy() / np.float32(temperature)), dtype)
    same = z(a) == z(a - step)
    assert same.sum() >= 8, "no neighbouring logits whose quotients collide"
    return [(float(v - step), float(v)) for v in a[same][:: max(1, int(same.sum()) // 16)]]


def draw_rows(grid, b, n_tokens):
    tt, tp, _ = DRAW_LENS[b]
    return grid[b, tt + tp + 2: tt + tp + 2 + draw_frames(b), :n_tokens]

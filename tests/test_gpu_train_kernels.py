"""Kernel-level checks of the training step's fp32 building blocks (csrc/d3pm_train.hip and the generic fp32 forward ops the
trainer replays, csrc/d3pm_generic.hip) at the LibriTTS shapes -- d = 512, 8 denoiser heads of width 64, 16 encoder heads of
width 32, FFN K = 2048, 768-row canvas, cross-attention onto 50 / 225 keys -- and at the edges where such kernels go wrong
(one key, key counts off the 64-lane grid, Tq != S, batch > 1, masked rows, padding ids).  Every result is compared with a
plain float64 torch evaluation of the same operation (autograd for the gradients).

Bounds.  u = 2^-24 is the fp32 unit roundoff.  A sum of n fp32 terms carries a rounding error of at most
gamma_n * sum |terms| (gamma_n = n u / (1 - n u)) in the worst case; the kernels' errors are not adversarial, and the
probabilistic analysis of Higham & Mary (SIAM J. Sci. Comput. 41(5), 2019, Thm. 3.1) bounds them by lam * sqrt(n) * u *
sum |terms| with probability >= 1 - 2 exp(-lam^2 / 2) per result.  LAM = 8 (failure probability < 3e-14 per element) is
used throughout; every bound below is that term plus the few roundings of the epilogue, evaluated element by element in fp64
from the same inputs.  A kernel that drops a term, mis-scales or mis-indexes errs by about one term's size, far above it."""
import math

import pytest
import torch
import torch.nn.functional as F

from dropout_mirror import z as _z
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
LAM = 8.0
SEED = (0xDEADBEEF << 32) | 77


def _sum_err(n, abs_terms):
    """Probabilistic fp32 rounding bound of a sum of n terms whose absolute values sum to abs_terms (module docstring)."""
    return LAM * math.sqrt(n) * U * abs_terms


def _guarded(rows, cols, ld, B=1):
    """A [B, rows, cols] view with row stride ld into NaN-filled storage, plus the storage: ld - cols pad columns per row and
    64 trailing elements the call must leave alone (and, where nothing is accumulated, a read of the output poisons it)."""
    store = torch.full((B * rows * ld + 64,), float("nan"), dtype=torch.float32, device=DEV)
    return store[:B * rows * ld].view(B, rows, ld)[..., :cols], store


def _untouched(store, view):
    """Every element of `store` outside `view` still holds the NaN it was filled with."""
    idx = torch.arange(store.numel(), device=DEV).as_strided(view.shape, view.stride(), view.storage_offset())
    written = torch.zeros(store.numel(), dtype=torch.bool, device=DEV)
    written[idx.reshape(-1)] = True
    return bool(torch.isnan(store[~written]).all())


# ---- 1./2. attention forward (generic fp32) and backward, with and without probability dropout ------------------------------
ATTN_SHAPES = [(1, 8, 64, 768, 768), (1, 8, 64, 768, 50), (1, 8, 64, 768, 225), (2, 16, 32, 225, 225), (1, 16, 32, 50, 50),
               (1, 8, 64, 100, 1), (2, 8, 64, 65, 130)]
PAD = 8          # extra columns per row of every gradient buffer: a write past a slice lands there


def _attn_inputs(B, H, hd, Tq, S, g):
    """q / k / v laid out as the trainer passes them: self-attention (Tq == S) as column slices of one [B, T, 3d] projection,
    cross-attention as a contiguous [B, Tq, d] query and column slices of a [B, S, 2d] K | V cache row."""
    d = H * hd
    if Tq == S:
        qkv = torch.randn(B, S, 3 * d, generator=g).to(DEV)
        return qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    q = torch.randn(B, Tq, d, generator=g).to(DEV)
    kv = torch.randn(B, S, 2 * d, generator=g).to(DEV)
    return q, kv[..., :d], kv[..., d:]


def _attn_ref(q, k, v, H, scale, Z=None):
    """softmax(scale q k^T) (o Z) @ v in float64; q [B,Tq,d], k / v [B,S,d], Z [B,H,Tq,S]."""
    B, Tq, d = q.shape
    hd = d // H
    qh, kh, vh = (t.reshape(B, -1, H, hd).transpose(1, 2) for t in (q, k, v))
    P = torch.softmax((qh * scale) @ kh.transpose(-1, -2), dim=-1)
    if Z is not None:
        P = P * Z
    return (P @ vh).transpose(1, 2).reshape(B, Tq, d)


def _grad_buffers(B, Tq, S, d, self_attn):
    """dq / dk / dv views in the trainer's layout (self: slices of one [B, T, 3d] buffer; cross: dq [B, Tq, d], dk / dv slices
    of [B, S, 2d]) with PAD guard columns per row; -> (views, [(storage, views in it)])."""
    if self_attn:
        buf, st = _guarded(S, 3 * d, 3 * d + PAD, B)
        return (buf[..., :d], buf[..., d:2 * d], buf[..., 2 * d:]), [(st, buf)]
    dq, st_q = _guarded(Tq, d, d + PAD, B)
    dkv, st_kv = _guarded(S, 2 * d, 2 * d + PAD, B)
    return (dq, dkv[..., :d], dkv[..., d:]), [(st_q, dq), (st_kv, dkv)]


@pytest.mark.parametrize("B,H,hd,Tq,S", ATTN_SHAPES)
def test_generic_f32_attention_forward_matches_float64(B, H, hd, Tq, S):
    from vall_e.vall_e import _hip
    g = torch.Generator().manual_seed(B * 7 + H + hd + Tq + S)
    q, k, v = _attn_inputs(B, H, hd, Tq, S, g)
    scale = hd ** -0.5
    o = _hip.op_attention(q, k, v, H, scale, family=_hip.FAMILY_GENERIC)
    ref = _attn_ref(q.double(), k.double(), v.double(), H, scale)
    err = (o.double() - ref).abs().max().item() / ref.abs().max().item()
    REPORT[f"train_kernels_attn_fwd_B{B}_H{H}_hd{hd}_Tq{Tq}_S{S}"] = err
    assert err <= 1e-5, err


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("B,H,hd,Tq,S", ATTN_SHAPES)
def test_attention_backward_matches_autograd(B, H, hd, Tq, S, drop):
    from vall_e.vall_e import train as T
    d, p, utt0 = H * hd, 0.1, 3
    site = T.dropout_site(1, 1, 0)
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(B * 7 + H + hd + Tq + S + 1)
    q, k, v = _attn_inputs(B, H, hd, Tq, S, g)
    do = torch.randn(B, Tq, d, generator=g).to(DEV)
    Z = torch.stack([_z(SEED, utt0 + b, site, (H, Tq, S), p) for b in range(B)]).double().to(DEV) if drop else None
    ref = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
    _attn_ref(*ref, H, scale, Z).backward(do.double())
    if drop:
        o = T.attention_dropout(q, k, v, H, scale, p, SEED, utt0, site)
        o_ref = _attn_ref(q.double(), k.double(), v.double(), H, scale, Z)
        assert (o.double() - o_ref).abs().max().item() <= 1e-5 * o_ref.abs().max().item()
    errs = {}
    for beta in (0.0, 1.0):
        # beta 0: every buffer starts NaN (a read of dK / dV would poison the result); beta 1: dK / dV start random
        (dq, dk, dv), stores = _grad_buffers(B, Tq, S, d, Tq == S)
        old_k = torch.randn(B, S, d, generator=g).to(DEV)
        old_v = torch.randn(B, S, d, generator=g).to(DEV)
        if beta:
            dk.copy_(old_k)
            dv.copy_(old_v)
        T.attention_bwd(q, k, v, do, dq, dk, dv, H, scale, beta_kv=beta, drop=(p, SEED, utt0, site) if drop else None)
        for store, view in stores:
            assert _untouched(store, view), "a write outside the gradient slices"
        for name, got, r, old in (("dq", dq, ref[0], None), ("dk", dk, ref[1], old_k), ("dv", dv, ref[2], old_v)):
            want = r.grad if old is None else r.grad + beta * old.double()
            scale_ = r.grad.abs().max().item()      # 0 for dq / dk at S = 1 (softmax of one key): then the kernel must give 0
            err = (got.double() - want).abs().max().item()
            errs[f"{name}_beta{int(beta)}"] = err / max(scale_, 1e-30)
            assert err <= 2e-5 * scale_, (name, beta, err, scale_)
    REPORT[f"train_kernels_attn_bwd_{'drop' if drop else 'plain'}_B{B}_H{H}_hd{hd}_Tq{Tq}_S{S}"] = errs


# ---- 3. generic fp32 linear forward and linear_bwd -------------------------------------------------------------------------
LIN_SHAPES = [(1536, 512), (2048, 512), (512, 2048), (1025, 512)]
M_LIN = 768


def _act64(v, act):
    return {0: lambda t: t, 1: F.gelu, 2: F.relu, 3: F.silu}[act](v)


@pytest.mark.parametrize("epi", ["plain", "r1", "r1r2", "mask"])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("N,K", LIN_SHAPES)
def test_generic_f32_linear_matches_float64(N, K, act, epi):
    """y = [mask] * (r1 + r2 + act(x w^T + b)).  Bound per element: the K + 1 term sum of x w^T + b (LAM sqrt(K + 1) u sum |terms|),
    carried through the activation (|act'| <= 1.13 for GELU, 1.1 for SiLU, 1 otherwise), plus 8 u (|pre| + |act|) for the
    activation's own evaluation (erff / expf are within 2 ulp; 1 + erf cancels, hence the |pre| term) and 4 u (|r1| + |r2| + |y|)
    for the roundings of the residual adds."""
    from vall_e.vall_e import _hip
    g = torch.Generator().manual_seed(N + K + act)
    x = torch.randn(M_LIN, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV)
    b = (torch.randn(N, generator=g) * 0.1).to(DEV)
    r1 = torch.randn(M_LIN, N, generator=g).to(DEV) if epi in ("r1", "r1r2") else None
    r2 = torch.randn(M_LIN, N, generator=g).to(DEV) if epi == "r1r2" else None
    period = 100
    mask = (torch.rand(period, generator=g) < 0.7).to(torch.uint8).to(DEV) if epi == "mask" else None
    y = _hip.op_linear(x, w, b, act=act, r1=r1, r2=r2, row_mask=mask, mask_period=period, family=_hip.FAMILY_GENERIC)
    pre = x.double() @ w.double().t() + b.double()
    a = _act64(pre, act)
    ref = a.clone()
    res = torch.zeros_like(ref)
    if r1 is not None:
        ref = ref + r1.double() + (r2.double() if r2 is not None else 0.0)
        res = r1.double().abs() + (r2.double().abs() if r2 is not None else 0.0)
    slope = {0: 1.0, 1: 1.13, 2: 1.0, 3: 1.1}[act]
    terms = x.double().abs() @ w.double().abs().t() + b.double().abs()
    bound = slope * _sum_err(K + 1, terms) + 8 * U * (pre.abs() + a.abs()) + 4 * U * (res + ref.abs())
    if mask is not None:
        live = mask.bool().repeat(M_LIN // period + 1)[:M_LIN]
        assert bool((y[~live] == 0).all()), "masked rows must be exactly zero"
        y, ref, bound = y[live], ref[live], bound[live]
    err = (y.double() - ref).abs()
    REPORT[f"train_kernels_linear_N{N}_K{K}_act{act}_{epi}"] = (err / bound).max().item()
    assert bool((err <= bound).all()), f"worst error / bound {(err / bound).max().item():.3g}"


@pytest.mark.parametrize("dx_beta", [0.0, 1.0])
@pytest.mark.parametrize("N,K", LIN_SHAPES)
def test_linear_bwd_matches_float64(N, K, dx_beta):
    """dw += dy^T x (M-term sums), db += colsum(dy) (M terms), dx = dx_beta dx + dy w (N terms); each bounded by its sum's
    LAM sqrt(n + 1) u (sum |terms| + |old|) plus one rounding of the result."""
    from vall_e.vall_e import train as T
    g = torch.Generator().manual_seed(N * 3 + K + int(dx_beta))
    x = torch.randn(M_LIN, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV)
    dy = torch.randn(M_LIN, N, generator=g).to(DEV)
    dw0, db0 = torch.randn(N, K, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    dx0 = torch.randn(M_LIN, K, generator=g).to(DEV)
    dw, db = dw0.clone(), db0.clone()
    dx, store = _guarded(M_LIN, K, K + PAD)
    dx = dx[0]
    if dx_beta:
        dx.copy_(dx0)
    T.linear_bwd(x, w, dy, dw, db, dx, dx_beta=dx_beta)
    assert _untouched(store, dx)
    X, W, DY = x.double(), w.double(), dy.double()
    worst = {}
    for name, got, ref, terms, n in (
            ("dw", dw, dw0.double() + DY.t() @ X, DY.abs().t() @ X.abs() + dw0.double().abs(), M_LIN),
            ("db", db, db0.double() + DY.sum(0), DY.abs().sum(0) + db0.double().abs(), M_LIN),
            ("dx", dx, dx_beta * dx0.double() + DY @ W, DY.abs() @ W.abs() + dx_beta * dx0.double().abs(), N)):
        bound = _sum_err(n + 1, terms) + U * ref.abs()
        err = (got.double() - ref).abs()
        worst[name] = (err / bound).max().item()
        assert bool((err <= bound).all()), (name, worst[name])
    REPORT[f"train_kernels_linear_bwd_N{N}_K{K}_beta{int(dx_beta)}"] = worst


# ---- 4. LayerNorm (+ FiLM) backward ------------------------------------------------------------------------------------------
def _ln_rows(kind, M, d, g):
    """random rows; rows with |mean| / sigma ~ 100; near-constant rows (sigma ~ 1e-3 around 0.5); or the three interleaved."""
    r = torch.randn(M, d, generator=g, dtype=torch.float64)
    if kind == "offset":
        return (100.0 * torch.sign(torch.randn(M, 1, generator=g, dtype=torch.float64)) + r).float()
    if kind == "flat":
        return (0.5 + 1e-3 * r).float()
    if kind == "mixed":
        return torch.stack([_ln_rows(("random", "offset", "flat")[i % 3], 1, d, g)[0] for i in range(M)])
    return r.float()


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("M", [1, 5, 768, 771])
@pytest.mark.parametrize("d", [32, 512])
def test_layernorm_bwd_matches_autograd(d, M, film, accumulate, eps):
    """First-order error bound, element by element, from the fp32 evaluation order of layernorm_bwd_rows: the row mean carries
    e_mu <= LAM sqrt(d) u mean|x|, so xhat = (x - mean) rstd carries e_xh <= rstd e_mu + LAM sqrt(d) u |xh| + 4 u |xh| (the
    variance sum and the sqrt / divide feed rstd); g = dy w; the row means mg, mgx of g and g xhat carry LAM sqrt(d) u of their
    sums of |terms| plus mean(|g| e_xh); dx = rstd (g - mg - xh mgx) adds 4 u of its |terms| and the relative error of rstd.
    The parameter gradients are fp32 atomic sums over M rows: LAM sqrt(M + 1) u (sum |terms| + |old|) plus sum |dy| e_xh."""
    from vall_e.vall_e import train as T
    g = torch.Generator().manual_seed(d * 1000 + M * 4 + 2 * film + accumulate)
    worst = {}
    for kind in ("random", "offset", "flat", "mixed"):
        x = _ln_rows(kind, M, d, g).to(DEV)
        w = (1.0 + 0.1 * torch.randn(d, generator=g)).to(DEV)
        b = (0.1 * torch.randn(d, generator=g)).to(DEV)
        fl = (0.2 * torch.randn(2 * d, generator=g)).to(DEV) if film else None
        go = torch.randn(M, d, generator=g).to(DEV)
        dx0, dw0, db0 = (torch.randn(M, d, generator=g).to(DEV), torch.randn(d, generator=g).to(DEV),
                         torch.randn(d, generator=g).to(DEV))
        df0 = torch.randn(2 * d, generator=g).to(DEV)
        dx, dw, db, df = dx0.clone(), dw0.clone(), db0.clone(), df0.clone() if film else None
        T.layernorm_bwd(x, go, w, b, dx, dw, db, film=fl, dfilm=df, eps=eps, accumulate=accumulate)
        X = x.double().requires_grad_(True)
        Wt, Bt = w.double().requires_grad_(True), b.double().requires_grad_(True)
        Ft = fl.double().requires_grad_(True) if film else None
        y = F.layer_norm(X, (d,), Wt, Bt, eps)
        out = y * (1 + Ft[:d]) + Ft[d:] if film else y
        out.backward(go.double())
        # the error bound (docstring), fp64
        with torch.no_grad():
            Xd = x.double()
            mu = Xd.mean(1, keepdim=True)
            rstd = 1.0 / torch.sqrt(((Xd - mu) ** 2).mean(1, keepdim=True) + eps)
            xh = (Xd - mu) * rstd
            dyv = go.double() * (1 + fl.double()[:d]) if film else go.double()
            gg = dyv * w.double()
            mgx = (gg * xh).mean(1, keepdim=True)
            s = LAM * math.sqrt(d) * U
            e_mu = s * Xd.abs().mean(1, keepdim=True) + U * mu.abs()
            e_rstd = s + 4 * U                                   # relative: the variance sum, sqrt and divide
            e_xh = rstd * e_mu + (2 * U + e_rstd) * xh.abs()
            e_mg = (s + 3 * U) * gg.abs().mean(1, keepdim=True)
            e_mgx = (s + 4 * U) * (gg * xh).abs().mean(1, keepdim=True) + (gg.abs() * e_xh).mean(1, keepdim=True)
            terms = gg.abs() + gg.mean(1, keepdim=True).abs() + (xh * mgx).abs()
            bnd = {"dx": rstd * (e_mg + e_xh * mgx.abs() + xh.abs() * e_mgx + 6 * U * terms) + e_rstd * rstd * terms}
            if accumulate:
                bnd["dx"] = bnd["dx"] + U * (dx0.double().abs() + X.grad.abs())
            sm = LAM * math.sqrt(M + 1) * U
            bnd["dw"] = (sm + 3 * U) * ((dyv * xh).abs().sum(0) + dw0.double().abs()) + (dyv.abs() * e_xh).sum(0)
            bnd["db"] = (sm + 2 * U) * (dyv.abs().sum(0) + db0.double().abs())
            want = {"dx": X.grad + (dx0.double() if accumulate else 0.0), "dw": dw0.double() + Wt.grad, "db": db0.double() + Bt.grad}
            got = {"dx": dx, "dw": dw, "db": db}
            if film:
                gy = go.double().abs()
                yv = xh * w.double() + b.double()
                bnd["dfilm"] = (sm + 3 * U) * (torch.cat([(gy * yv.abs()).sum(0), gy.sum(0)]) + df0.double().abs()) + \
                    torch.cat([(gy * e_xh * w.double().abs()).sum(0), torch.zeros(d, dtype=torch.float64, device=DEV)])
                want["dfilm"] = df0.double() + Ft.grad
                got["dfilm"] = df
        for name in got:
            err = (got[name].double() - want[name]).abs()
            r = (err / bnd[name]).max().item()
            worst[f"{kind}_{name}"] = r
            assert bool((err <= bnd[name]).all()), (kind, name, r)
    REPORT[f"train_kernels_layernorm_bwd_d{d}_M{M}_film{int(film)}_acc{int(accumulate)}_eps{eps:g}"] = max(worst.values())


# ---- 5. activation backward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["gelu", "relu", "silu"])
def test_act_bwd_matches_autograd(act):
    from vall_e.vall_e import train as T
    code = {"gelu": T.GELU, "relu": T.RELU, "silu": T.SILU}[act]
    g = torch.Generator().manual_seed(code)
    u = torch.cat([torch.linspace(-30, 30, 60001, dtype=torch.float64).float(), (torch.rand(4096, generator=g) * 60 - 30),
                   torch.tensor([0.0, -0.0, 1e-30, -1e-30, 30.0, -30.0])])
    dm = torch.randn(u.numel(), generator=g)
    du = T.act_bwd(u.to(DEV), dm.to(DEV), code).cpu().double()
    U64 = u.double().requires_grad_(True)
    {"gelu": F.gelu, "relu": F.relu, "silu": F.silu}[act](U64).backward(dm.double())
    if act == "relu":                                            # exact, with relu'(0) = 0 as torch has it
        assert torch.equal(du, U64.grad), (du - U64.grad).abs().max().item()
        assert bool((du[u == 0] == 0).all())
        return
    # GELU / SiLU: the derivative is O(1) and its fp32 evaluation from erff / expf (within 2 ulp) stays within 1e-6 of it,
    # |err| <= 1e-6 |dM| element by element, as long as no factor is formed by cancellation: GELU's 1 + erf(u / sqrt 2) for
    # u << 0 is multiplied by 0.5 and meets u pdf(u) of the same small size; SiLU's 1 - sigmoid(u) must be sigmoid(-u), since
    # 1 + e^-u near u = 17 rounds by up to 2^-24 and u times that is 1.5e-6
    err = (du - U64.grad).abs()
    REPORT[f"train_kernels_act_bwd_{act}"] = (err / dm.double().abs()).max().item()
    assert bool((err <= 1e-6 * dm.double().abs()).all()), (err / dm.double().abs()).max().item()


# ---- 6. cross-entropy backward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [1.0, 30.0])
def test_ce_bwd_matches_autograd(gain):
    """d/dlogits of sum_rows CE(logits * mask, targets * mask) * gscale.  Bound per element: softmax p_j = exp(l_j - max) / sum
    is within u (|l_j - max| + 4) relative of exact (the subtraction's rounding goes through exp; expf 2 ulp; divide), the
    K-term positive sum adds LAM sqrt(K) u plus the p-weighted error of its terms; the result adds one rounding of p - [target]
    and of the gscale product.  Below FLT_MIN = 2^-126 fp32 has no normal numbers: p and p * gscale may flush to 0 there, so
    each contributes at most FLT_MIN of absolute error (2 FLT_MIN in all)."""
    from vall_e.vall_e import train as T
    rows, K = 768, 1025
    g = torch.Generator().manual_seed(int(gain))
    logits = torch.randn(rows, K, generator=g) * gain
    logits[7] = 0.25                                              # all-equal row
    logits[8] = torch.randn(K, generator=g)
    logits[8, 3] = 40.0                                           # peaked far from its target
    targets = torch.randint(0, K, (rows,), generator=g, dtype=torch.int32)
    targets[8] = 1000
    targets[0], targets[1], targets[2] = 0, 1024, 1024
    fm = torch.ones(rows, dtype=torch.uint8)
    fm[700:] = 0                                                  # padding tail
    fm[torch.randperm(700, generator=g)[:50]] = 0                 # and holes
    fm[[0, 1, 7, 8]] = 1
    fm[2] = 0                                                     # a masked row whose target is 1024
    tg = targets * fm.to(torch.int32)
    gscale = 1.0 / (rows * int(fm.sum()))
    dl = T.ce_bwd(logits.to(DEV), tg.to(DEV), fm.to(DEV), gscale).cpu().double()
    L = logits.double().requires_grad_(True)
    mk = fm.double()[:, None]
    (F.cross_entropy(L * mk, tg.long(), reduction="sum") * gscale).backward()
    ref = L.grad
    assert bool((dl[fm == 0] == 0).all()), "masked rows must get no gradient"
    with torch.no_grad():
        Ld = logits.double()
        p = torch.softmax(Ld, dim=1)
        rel = U * ((Ld - Ld.max(1, keepdim=True).values).abs() + 4)
        s_rel = (p * rel).sum(1, keepdim=True) + LAM * math.sqrt(K) * U
        bound = gscale * p * (rel + s_rel + U) + 2 * U * ref.abs() + 2 * 2.0 ** -126
    live = fm.bool()
    err = (dl - ref).abs()[live]
    REPORT[f"train_kernels_ce_bwd_gain{gain:g}"] = (err / bound[live]).max().item()
    assert bool((err <= bound[live]).all()), (err / bound[live]).max().item()


# ---- 7. embedding backward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", ["one_token", "mix"])
@pytest.mark.parametrize("padding_idx", [0, -1])
@pytest.mark.parametrize("period", [0, 100, 768])
def test_embed_bwd_matches_index_add(tokens, padding_idx, period):
    """dTable[tok] += mask * dY over rows with 0 <= tok < n_classes and tok != padding_idx, into one level of a 3-level table (as
    the prompt embedding's levels are): the neighbouring levels stay untouched.  fp32 atomic sums of up to 768 rows: LAM
    sqrt(n + 1) u (sum |terms| + |old|)."""
    from vall_e.vall_e import train as T
    rows, d, n = 768, 512, 1025
    g = torch.Generator().manual_seed(period + 3 * (padding_idx + 1) + (tokens == "mix"))
    if tokens == "one_token":
        tok = torch.full((rows,), 7, dtype=torch.int32)
    else:
        tok = torch.randint(0, n, (rows,), generator=g, dtype=torch.int32)
        tok[::5] = torch.randint(0, 4, (len(tok[::5]),), generator=g, dtype=torch.int32)      # repeats, and ids 0 / 1 often
        tok[3::11] = -1                                           # absent levels
    mask = (torch.rand(period, generator=g) < 0.75).to(torch.uint8) if period else None
    dy = torch.randn(rows, d, generator=g)
    big = torch.randn(3, n, d, generator=g)
    base = big.clone()
    dev_big = big.to(DEV)
    T.embed_bwd(tok.to(DEV), None if mask is None else mask.to(DEV), dy.to(DEV), dev_big[1], padding_idx=padding_idx)
    got = dev_big.cpu().double()
    assert torch.equal(got[0], base[0].double()) and torch.equal(got[2], base[2].double()), "write outside the table"
    live = (tok >= 0) & (tok < n) & (tok != padding_idx)
    if mask is not None:
        live &= mask.bool().repeat(rows // period + 1)[:rows]
    idx = tok[live].long()
    ref = base[1].double().index_add(0, idx, dy[live].double())
    cnt = torch.zeros(n, dtype=torch.float64).index_add(0, idx, torch.ones(len(idx), dtype=torch.float64))
    terms = base[1].double().abs().index_add(0, idx, dy[live].double().abs())
    bound = LAM * torch.sqrt(cnt + 1)[:, None] * U * terms
    err = (got[1] - ref).abs()
    untouched = cnt == 0
    assert torch.equal(got[1][untouched], base[1].double()[untouched]), "rows without a live token must not change"
    if padding_idx >= 0:
        assert torch.equal(got[1][padding_idx], base[1][padding_idx].double())
    REPORT[f"train_kernels_embed_bwd_{tokens}_pad{padding_idx}_period{period}"] = (err / bound.clamp_min(1e-300)).max().item()
    assert bool((err <= bound).all()), (err / bound.clamp_min(1e-300)).max().item()

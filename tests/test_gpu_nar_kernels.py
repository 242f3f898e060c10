"""The three kernels of the stock NAR stage (csrc/d3pm_nar.hip), each launched alone through its test entry (include/d3pm_hip.h:
d3pm_op_nar_embed, d3pm_op_adaln, d3pm_op_nar_sample) and compared with the host mirror of the rule its comment documents
(tests/nar_mirror.py; tests/test_nar_mirror.py pins the mirrors to the oracle on the CPU).

  * nar_embed_rows: bit for bit, every storage type, both block sizes (d = 128: 64 threads; 512 / 1024: 256).
  * adaln_rows, adaln_rows_vec<T, 1> (d = 512), adaln_rows_vec<T, 2> (d = 1024): masked rows, the sentinel row and finiteness exactly;
    against the mirror (float64 row moments) at most 1e-3 of the elements of a case may differ in bits and none by 64 storage ulps or
    more.  The kernel's moments are fp32 sums in another order and its rsqrtf may sit one fp32 step away, which flips the rounding of h
    on a few elements: the mirror alone, float64 moments against fp32 moments and against rstd moved by one fp32 step, stays under 3e-4
    differing on these very inputs (tests/test_nar_mirror.py asserts it).  A case is one (type, d, alignment): the M = 1027 launch; the
    M = 1 and M = 5 launches run the leading rows of the same tensor and must reproduce them bit for bit (a row's result does not
    depend on how many rows the launch has), so they stand under the same comparison.  The same tensor through 16-byte aligned
    addresses (vec kernel) and through views 4 bytes further on (scalar kernel) must satisfy the same two conditions against each other.
  * nar_sample_rows: greedy ids equal the mirror's exactly (first index on ties across lanes and passes, constant rows, -inf
    classes, the rounding of logit / T, which decides 150 rows of the 16-bit inputs); Gumbel ids equal the mirror's, a differing id
    excused only where the mirror's own margin is within 8 fp32 steps of the winning value (two logf and one add), one row per
    case at the most -- and no row of these inputs is within 64 (tests/test_nar_mirror.py), so the excuse is never needed here.

The numbers measured on the GPU go to util.REPORT."""
import numpy as np
import pytest
import torch

import nar_mirror as NM
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
TAG = dict(zip(DTYPES, IDS))
SENTINEL = -7.0
DIFFER_CAP, ULP_CAP = 1e-3, 64.0


def _dev(inp):
    return {k: v.to(DEV) if isinstance(v, torch.Tensor) else v for k, v in inp.items()}


# ---- nar_embed_rows ---------------------------------------------------------------------------------------------------------------
def _embed_launch(inp, t_max):
    """One launch into buffers that end in a sentinel row / entry; returns (x, row_mask, key_len, the three whole buffers)."""
    from vall_e.vall_e import _hip
    B, d, dtype = inp["lens"].shape[0], inp["w_text"].shape[1], inp["w_text"].dtype
    xb = torch.full((B * t_max + 1, d), SENTINEL, dtype=dtype, device=DEV)
    mb = torch.full((B * t_max + 1,), 7, dtype=torch.uint8, device=DEV)
    kb = torch.full((B + 1,), -77, dtype=torch.int32, device=DEV)
    a = _dev(inp)
    x, m, k = _hip.op_nar_embed(a["lens"], a["text"], a["prom"], a["resp"], a["n_given"], a["w_text"], a["w_prom"], a["w_resp"], a["sep"],
                                a["pe"], t_max, x=xb[:B * t_max].view(B, t_max, d), row_mask=mb[:B * t_max].view(B, t_max), key_len=kb[:B])
    torch.cuda.synchronize()
    return x.cpu(), m.cpu(), k.cpu(), (xb.cpu(), mb.cpu(), kb.cpu())


def _sentinels_intact(bufs):
    xb, mb, kb = bufs
    return bool((xb[-1] == SENTINEL).all()) and int(mb[-1]) == 7 and int(kb[-1]) == -77


@pytest.mark.parametrize("n_given", [1, 4, 7])
@pytest.mark.parametrize("d", [128, 512, 1024])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_embed_rows_equal_the_mirror_bit_for_bit(built_lib, dtype, d, n_given):
    inp = NM.embed_inputs(d, dtype, n_given)
    t_max = inp["t_max"]
    want_x, want_m, want_k = NM.embed_mirror(**inp)
    x, m, k, bufs = _embed_launch(inp, t_max)
    assert torch.equal(m, want_m) and torch.equal(k, want_k)
    assert torch.equal(x, want_x), f"{int((x != want_x).any(-1).sum())} rows differ: {(x != want_x).any(-1).nonzero().tolist()[:8]}"
    assert not x[m == 0].any() and int((m == 0).sum()) > 0, "padding rows must be exactly zero"
    assert _sentinels_intact(bufs)
    # nothing past an utterance's own lengths, and no response column from n_given on, is read: other poison, same output
    x2, m2, k2, bufs2 = _embed_launch(NM.repoison(inp, -4321), t_max)
    assert torch.equal(x2, x) and torch.equal(m2, m) and torch.equal(k2, k) and _sentinels_intact(bufs2)
    # a grid shorter than the longest utterance: t_max rows of it are written, key_len still reports its total, nothing behind the grid
    short = 20
    assert max(sum(l) + 2 for l in NM.EMBED_LENS) > short
    cut = dict(inp, t_max=short)
    want_x, want_m, want_k = NM.embed_mirror(**cut)
    x3, m3, k3, bufs3 = _embed_launch(inp, short)
    assert torch.equal(x3, want_x) and torch.equal(m3, want_m) and torch.equal(k3, want_k) and torch.equal(k3, k)
    assert bool(m3[1].all()) and _sentinels_intact(bufs3)


# ---- adaln_rows / adaln_rows_vec ---------------------------------------------------------------------------------------------------
def _adaln_launch(x, table, mask, M, shift):
    """x[:M] through the entry; shift = the number of elements every address (x, y, emb_row) sits behind a 256-byte aligned one."""
    from vall_e.vall_e import _hip
    d, dtype = x.shape[1], x.dtype
    xb = torch.zeros(shift + M * d, dtype=dtype, device=DEV)
    xb[shift:] = x[:M].reshape(-1).to(DEV)
    tb = torch.zeros(shift + table.numel(), dtype=dtype, device=DEV)
    tb[shift:] = table.reshape(-1).to(DEV)
    yb = torch.full((shift + (M + 1) * d,), SENTINEL, dtype=dtype, device=DEV)
    xv, yv = xb[shift:].view(M, d), yb[shift: shift + M * d].view(M, d)
    emb = tb[shift:].view(table.shape)[NM.ADALN_LEVEL]
    assert xv.data_ptr() % 16 == (shift * x.element_size()) % 16 == yv.data_ptr() % 16 == emb.data_ptr() % 16
    _hip.op_adaln(xv, emb, mask[:M].to(DEV), out=yv)
    torch.cuda.synchronize()
    assert bool((yb[shift + M * d:] == SENTINEL).all()), "the row behind M was written"
    return yv.cpu()


def _adaln_case(dtype, d, shift, what):
    """The three launches of one case against the mirror; returns the M = 1027 output."""
    x, table, mask, kind = NM.adaln_inputs(d, dtype)
    ref = NM.adaln_mirror(x, table[NM.ADALN_LEVEL], mask)
    full = None
    for M in (NM.ADALN_ROWS, 5, 1):
        y = _adaln_launch(x, table, mask, M, shift)
        assert torch.isfinite(y.float()).all(), (what, M)
        assert not y[mask[:M] == 0].any(), (what, M, "masked rows must be exactly zero")
        if full is None:
            full = y
        assert torch.equal(y, full[:M]), (what, M, "a row's result depends on the number of rows")
    differ, worst = NM.lp_error(full, ref, dtype)
    by_kind = {k: NM.lp_error(full[(kind == k) & mask.bool()], ref[(kind == k) & mask.bool()], dtype)[0] for k in range(4)}
    REPORT[f"nar_adaln_{what}"] = {"differing": differ, "worst_ulp": worst, "differing_by_row_kind": by_kind}
    print(f"adaln {what}: {differ:.2e} of the elements differ from the mirror, worst {worst:.1f} ulp; by row kind {by_kind}")
    assert differ <= DIFFER_CAP, f"{what}: {differ:.2e} of the elements differ from the mirror"
    assert worst < ULP_CAP, f"{what}: worst element off by {worst:.1f} ulp"
    return full


@pytest.mark.parametrize("d", [512, 1024])
@pytest.mark.parametrize("dtype", DTYPES[1:], ids=IDS[1:])
def test_adaln_vec_and_scalar_kernels_against_the_mirror_and_each_other(built_lib, dtype, d):
    """16-byte aligned addresses take adaln_rows_vec<T, d / 512>; the same tensors 4 bytes further on take adaln_rows."""
    vec = _adaln_case(dtype, d, 0, f"{TAG[dtype]}_d{d}_vec")
    scalar = _adaln_case(dtype, d, 4 // vec.element_size(), f"{TAG[dtype]}_d{d}_scalar_offset4")
    differ, worst = NM.lp_error(vec, scalar, dtype)
    REPORT[f"nar_adaln_{TAG[dtype]}_d{d}_vec_vs_scalar"] = {"differing": differ, "worst_ulp": worst}
    print(f"adaln {TAG[dtype]} d={d} vec vs scalar: {differ:.2e} differing, worst {worst:.1f} ulp")
    assert differ <= DIFFER_CAP and worst < ULP_CAP, (differ, worst)


@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("dtype", DTYPES[1:], ids=IDS[1:])
def test_adaln_scalar_kernel_at_other_widths(built_lib, dtype, d):
    _adaln_case(dtype, d, 0, f"{TAG[dtype]}_d{d}_scalar")


def test_adaln_fp32_against_float64(built_lib):
    """fp32 rounds nothing: the scalar kernel against the whole expression in float64 under the fp32 criterion of test_gpu_kernels.py
    (1e-4 of the output scale)."""
    d = 512
    x, table, mask, kind = NM.adaln_inputs(d, torch.float32)
    ref = NM.adaln_mirror(x, table[NM.ADALN_LEVEL], mask)
    full = None
    for M in (NM.ADALN_ROWS, 5, 1):
        y = _adaln_launch(x, table, mask, M, 0)
        assert torch.isfinite(y).all() and not y[mask[:M] == 0].any()
        full = y if full is None else full
        assert torch.equal(y, full[:M])
    err = (full.double() - ref).abs().max().item() / ref.abs().max().item()
    small = (kind == 1) & mask.bool()
    err_small = (full.double() - ref)[small].abs().max().item() / ref[small].abs().max().item()
    REPORT["nar_adaln_f32_d512_scalar"] = {"max_err_over_scale": err, "max_err_over_scale_sigma_1e-2_rows": err_small}
    print(f"adaln f32 d=512: max error {err:.2e} of the output scale; sigma = 1e-2 rows {err_small:.2e} of theirs")
    assert err <= 1e-4 and err_small <= 1e-4, (err, err_small)


# ---- nar_sample_rows --------------------------------------------------------------------------------------------------------------
RESP_SENTINEL = -5


def _draw_launch(grid, n_tokens, level, seed, *, greedy=False, only=None, utt0=0):
    """One launch over the padded grid (or over utterance `only` alone); returns resp [B, tr_max, 8] on the host."""
    from vall_e.vall_e import _hip
    sel = slice(None) if only is None else slice(only, only + 1)
    lens = torch.tensor(NM.DRAW_LENS, dtype=torch.int32)[sel].contiguous().to(DEV)
    resp = torch.full((lens.shape[0], NM.DRAW_TR_MAX, 8), RESP_SENTINEL, dtype=torch.int32, device=DEV)
    _hip.op_nar_sample(grid[sel][..., :n_tokens], lens, resp, level, NM.DRAW_TEMPERATURE, seed, utt0=utt0,
                       flags=_hip.FLAG_GREEDY if greedy else 0)
    torch.cuda.synchronize()
    return resp.cpu()


def _only_the_column(resp, level, utts=(0, 1, 2)):
    """Column level + 1 of the frames inside the grid holds ids, every other slot the sentinel; returns the ids per utterance."""
    ids = []
    for i, b in enumerate(utts):
        n = NM.draw_frames(b)
        col = resp[i, :n, level + 1]
        assert bool((col != RESP_SENTINEL).all()), f"utterance {b}: {int((col == RESP_SENTINEL).sum())} frames not written"
        rest = resp[i].clone()
        rest[:n, level + 1] = RESP_SENTINEL
        assert bool((rest == RESP_SENTINEL).all()), f"utterance {b}: a slot outside column {level + 1} of its {n} frames changed"
        ids.append(col.numpy().astype(np.int64))
    return ids


@pytest.mark.parametrize("n_tokens", [1024, 1023, 6])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_greedy_draw_equals_the_mirror(built_lib, dtype, n_tokens):
    grid = NM.draw_inputs(n_tokens, dtype)
    assert NM.draw_frames(0) == NM.DRAW_TR[0] - NM.DRAW_CUT
    level = 2
    ids = _only_the_column(_draw_launch(grid.to(DEV), n_tokens, level, 0, greedy=True), level)
    for b in range(3):
        want, _ = NM.draw_mirror(NM.draw_rows(grid, b, n_tokens), NM.DRAW_TEMPERATURE, greedy=True)
        bad = np.nonzero(ids[b] != want)[0]
        assert bad.size == 0, f"utterance {b}: {bad.size} ids differ, first frames {bad[:8].tolist()}: got {ids[b][bad[:8]].tolist()} want {want[bad[:8]].tolist()}"
        assert ids[b].max() < n_tokens


@pytest.mark.parametrize("n_tokens", [1024, 1023, 6])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gumbel_draw_equals_the_mirror(built_lib, dtype, n_tokens):
    grid = NM.draw_inputs(n_tokens, dtype, special=False)
    dev = grid.to(DEV)
    got, smallest, mismatches, excused = {}, np.inf, 0, 0
    for seed, level in NM.DRAW_RUNS:
        got[seed, level] = _only_the_column(_draw_launch(dev, n_tokens, level, seed), level)
        for b in range(3):
            rows = NM.draw_rows(grid, b, n_tokens)
            want, _ = NM.draw_mirror(rows, NM.DRAW_TEMPERATURE, seed=seed, level=level, utt=b)
            ulps = NM.margin_ulps(rows, NM.DRAW_TEMPERATURE, seed=seed, level=level, utt=b)
            smallest = min(smallest, float(ulps.min()))
            bad = got[seed, level][b] != want
            mismatches += int(bad.sum())
            excused += int((bad & (ulps <= 8)).sum())
            assert got[seed, level][b].max() < n_tokens
    REPORT[f"nar_draw_{TAG[dtype]}_k{n_tokens}"] = {"id_mismatches": mismatches, "excused": excused, "smallest_margin_fp32_ulps": smallest,
                                                  "rows": 3 * sum(NM.draw_frames(b) for b in range(3))}
    print(f"draw {TAG[dtype]} n_tokens={n_tokens}: {mismatches} ids differ from the mirror ({excused} within 8 ulp); smallest margin {smallest:.1f} ulp")
    assert mismatches == excused and excused <= 1, (mismatches, excused)
    (s0, l0), (_, l5), (s1, _) = NM.DRAW_RUNS
    # another level draws other noise into another column; another seed draws other noise
    assert l0 != l5 and not all(np.array_equal(a, c) for a, c in zip(got[s0, l0], got[s0, l5]))
    assert not all(np.array_equal(a, c) for a, c in zip(got[s0, l0], got[s1, l0]))
    # utterance 2 alone at utt0 = 2 draws what it draws inside the batch at utt0 = 0
    alone = _only_the_column(_draw_launch(dev, n_tokens, l0, s0, only=2, utt0=2), l0, utts=(2,))
    assert np.array_equal(alone[0], got[s0, l0][2])

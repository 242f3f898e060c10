"""The NAR stage's level draw with options (csrc/d3pm_nar_draw.hip) through its test entry d3pm_op_nar_draw (include/d3pm_hip.h:
d3pm_nar_draw), on the padded grids of the draw tests (tests/nar_mirror.py: pad columns of 60000, frames cut by the grid, duplicated
maxima, constant rows, -inf classes) in f32 / f16 / bf16 at n_tokens 1024, 37 (no multiple of 4, fewer groups than lanes) and 1280 (the
limit).  Nothing here has a tolerance but the log-probability (1.0e-4, the bound of d3pm_frame_scores) and the distance of the kept
mass from top_p (the header's n_tokens / 2^20 + 2^-20):

  1. neutral options + logprob_out: the ids of d3pm_op_nar_sample, bit for bit (greedy and every Gumbel run of DRAW_RUNS);
  2. top_k in {1, 2, 50, n_tokens} (50 not at 37 tokens, where the entry refuses it) at temperature 0.2 and 1: the ids of
     d3pm_op_nar_sample(temperature = 1) on the host-filtered v' stored in T; a duplicated maximum survives top_k = 1 at both classes
     and the first wins under greedy;
  3. top_p: the ids of the unfiltered entry on the host values cut at the theta the device reports; theta is a value of the row; the
     kept mass of the float64 softmax sits within the slack of top_p from either side; top_p = 1/2048 gives the ids of top_k = 1;
  4. known frames keep the code they hold, every other frame draws what it draws without `known`, theta_out is NaN exactly there;
  5. logprob_out at the id that stands in resp equals the float64 log-softmax of float(logits) within 1.0e-4, known frames included,
     and does not depend on temperature / top_k / top_p, bit for bit;
  6. every launch below leaves resp, logprob_out and theta_out untouched outside the frames of the grid and outside the level's column;
  7. refusals return their codes and write nothing.

The numbers measured on the GPU go to util.REPORT."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import nar_draw_ref as R
import nar_mirror as NM
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
TAG = dict(zip(DTYPES, IDS))
TOKENS = [1024, 37, 1280]
RESP_POISON, LP_POISON, THETA_POISON = -5, 777.0, 555.0
HELD = 4097                       # the code of the known frames of case 4: no id the draw can write
LOGPROB_TOL = 1.0e-4
B, TR_MAX = len(NM.DRAW_LENS), NM.DRAW_TR_MAX


@functools.lru_cache(maxsize=None)
def _grid(n_tokens, dtype, special, alive=False):
    g = NM.draw_inputs(n_tokens, dtype, special=special)
    return R.without_dead_rows(g, n_tokens) if alive else g


@functools.lru_cache(maxsize=None)
def _grid_dev(n_tokens, dtype, special, alive=False):
    return _grid(n_tokens, dtype, special, alive).to(DEV)


def _frames_mask():
    m = torch.zeros(B, TR_MAX, dtype=torch.bool)
    for b in range(B):
        m[b, :NM.draw_frames(b)] = True
    return m


def _rows_of(grid, n_tokens):
    """The response rows inside the grid, utterance after utterance: [sum frames, n_tokens] in the order of _frames_mask()."""
    return torch.cat([NM.draw_rows(grid, b, n_tokens) for b in range(B)])


def _with_rows(grid, n_tokens, rows):
    """The grid with its response rows replaced (pad columns and every other row as they are)."""
    out, at = grid.clone(), 0
    for b, (tt, tp, _) in enumerate(NM.DRAW_LENS):
        n = NM.draw_frames(b)
        out[b, tt + tp + 2: tt + tp + 2 + n, :n_tokens] = rows[at: at + n].to(grid.dtype)
        at += n
    return out


def _sample(dev_grid, n_tokens, level, seed, temperature, greedy):
    """d3pm_op_nar_sample -> ids int64 [sum frames]."""
    from vall_e.vall_e import _hip
    lens = torch.tensor(NM.DRAW_LENS, dtype=torch.int32, device=DEV)
    resp = torch.full((B, TR_MAX, 8), RESP_POISON, dtype=torch.int32, device=DEV)
    _hip.op_nar_sample(dev_grid[..., :n_tokens], lens, resp, level, temperature, seed, flags=_hip.FLAG_GREEDY if greedy else 0)
    torch.cuda.synchronize()
    return resp.cpu()[:, :, level + 1][_frames_mask()].long().numpy()


def _draw(dev_grid, n_tokens, level, seed, temperature, greedy, *, top_k=0, top_p=1.0, known=None, held=None, logprob=False, theta=False):
    """d3pm_op_nar_draw over the whole padded grid with every output pre-filled with poison; asserts that nothing outside the frames of
    the grid and outside column level + 1 (resp) / level (logprob_out) was written (case 6) and returns (ids [sum frames], logprob
    [sum frames] or None, theta [sum frames] or None).  known: bool [B, TR_MAX]; held: int32 [B, TR_MAX] codes put into column
    level + 1 before the launch (where known)."""
    from vall_e.vall_e import _hip
    lens = torch.tensor(NM.DRAW_LENS, dtype=torch.int32, device=DEV)
    resp0 = torch.full((B, TR_MAX, 8), RESP_POISON, dtype=torch.int32)
    if known is not None:
        resp0[:, :, level + 1] = torch.where(known, held, resp0[:, :, level + 1])
    resp = resp0.to(DEV)
    lp = torch.full((B, TR_MAX, 7), LP_POISON, dtype=torch.float32, device=DEV) if logprob else None
    th = torch.full((B, TR_MAX), THETA_POISON, dtype=torch.float32, device=DEV) if theta else None
    _hip.op_nar_draw(dev_grid[..., :n_tokens], lens, resp, level, temperature, seed, flags=_hip.FLAG_GREEDY if greedy else 0, top_k=top_k,
                     top_p=top_p, known=None if known is None else known.to(torch.uint8).to(DEV), logprob_out=lp, theta_out=th)
    torch.cuda.synchronize()
    inside = _frames_mask()
    resp = resp.cpu()
    rest = resp.clone()
    rest[:, :, level + 1][inside] = resp0[:, :, level + 1][inside]
    assert torch.equal(rest, resp0), "resp changed outside the frames of the grid or outside the level's column"
    ids = resp[:, :, level + 1][inside].long().numpy()
    if known is not None:
        k = known[inside].numpy()
        assert np.array_equal(ids[k], held[inside].long().numpy()[k]), "a known frame lost the code it held"
        assert (ids[~k] != RESP_POISON).all()
    else:
        assert (ids != RESP_POISON).all(), "a frame inside the grid was not written"
    out_lp = out_th = None
    if logprob:
        lp = lp.cpu()
        rest = lp.clone()
        rest[:, :, level][inside] = LP_POISON
        assert bool((rest == LP_POISON).all()), "logprob_out changed outside the frames of the grid or outside the level's column"
        out_lp = lp[:, :, level][inside].numpy()
    if theta:
        th = th.cpu()
        assert bool((th[~inside] == THETA_POISON).all()), "theta_out changed outside the frames of the grid"
        out_th = th[inside].numpy()
    return ids, out_lp, out_th


def _report_diff(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} ids differ, first frames {bad[:8].tolist()}: got {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}"


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tokens", TOKENS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_neutral_options_draw_what_the_plain_entry_draws(built_lib, dtype, n_tokens):
    special = _grid_dev(n_tokens, dtype, True)
    ids, lp, _ = _draw(special, n_tokens, 2, 0, NM.DRAW_TEMPERATURE, True, logprob=True)
    _report_diff(ids, _sample(special, n_tokens, 2, 0, NM.DRAW_TEMPERATURE, True), "greedy")
    assert ids.max() < n_tokens and (lp != LP_POISON).all()
    plain = _grid_dev(n_tokens, dtype, False)
    for seed, level in NM.DRAW_RUNS:
        ids, _, _ = _draw(plain, n_tokens, level, seed, NM.DRAW_TEMPERATURE, False, logprob=True)
        _report_diff(ids, _sample(plain, n_tokens, level, seed, NM.DRAW_TEMPERATURE, False), f"seed {seed} level {level}")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tokens", TOKENS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_top_k_equals_the_plain_entry_on_host_filtered_values(built_lib, dtype, n_tokens):
    seed, level = NM.DRAW_RUNS[1]
    for special, greedy in ((True, True), (False, False)):
        grid, dev = _grid(n_tokens, dtype, special), _grid_dev(n_tokens, dtype, special)
        rows = _rows_of(grid, n_tokens)
        for temperature in (NM.DRAW_TEMPERATURE, 1.0):
            v = R.values(rows, temperature)
            for top_k in (1, 2, 50, n_tokens):
                if top_k > n_tokens:
                    continue
                vp = R.cut(v, R.theta1(v, top_k))
                want = _sample(_with_rows(grid, n_tokens, vp).to(DEV), n_tokens, level, seed, 1.0, greedy)
                got, _, _ = _draw(dev, n_tokens, level, seed, temperature, greedy, top_k=top_k)
                _report_diff(got, want, f"top_k {top_k} T {temperature} greedy {greedy}")
                if special and top_k == 1 and temperature == 1.0:
                    # rows with a duplicated maximum that no later rule of draw_inputs overwrote: both classes kept, the first wins
                    hi, lo = (700, 3) if n_tokens > 700 else (n_tokens - 1, 1)
                    f = torch.cat([torch.arange(NM.draw_frames(b)) for b in range(B)])
                    many = torch.cat([torch.full((NM.draw_frames(b),), NM.draw_frames(b) > 1) for b in range(B)])
                    dup = ((f % 7 == 2) & (f % 11 != 5) & (f % 13 != 6) & (f != 17) & many).numpy()
                    assert dup.sum() > 50
                    assert bool((torch.isfinite(vp[dup]).sum(-1) == 2).all()) and bool(torch.isfinite(vp[dup][:, [hi, lo]]).all())
                    assert (got[dup] == lo).all()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tokens", TOKENS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_top_p_cuts_at_a_value_of_the_row_that_holds_the_mass(built_lib, dtype, n_tokens):
    seed, level = NM.DRAW_RUNS[0]
    slack = n_tokens / 2.0 ** 20 + 2.0 ** -20
    grid, dev = _grid(n_tokens, dtype, True, True), _grid_dev(n_tokens, dtype, True, True)
    rows = _rows_of(grid, n_tokens)
    v = R.values(rows, NM.DRAW_TEMPERATURE)
    worst_low, worst_high = np.inf, -np.inf
    for top_k in (0, 50):
        if top_k > n_tokens:
            continue
        vp = R.cut(v, R.theta1(v, top_k))
        p = R.softmax64(vp)
        for greedy in (True, False):
            only_max, _, _ = _draw(dev, n_tokens, level, seed, NM.DRAW_TEMPERATURE, greedy, top_k=1)
            for top_p in (0.9, 0.5, 1.0 / 2048):
                got, _, theta = _draw(dev, n_tokens, level, seed, NM.DRAW_TEMPERATURE, greedy, top_k=top_k, top_p=top_p, theta=True)
                th = torch.from_numpy(theta)[:, None]
                assert bool((vp == th).any(-1).all()), "theta is not a value of its row"
                want = _sample(_with_rows(grid, n_tokens, R.cut(vp, theta)).to(DEV), n_tokens, level, seed, 1.0, greedy)
                _report_diff(got, want, f"top_k {top_k} top_p {top_p} greedy {greedy}")
                p32 = float(np.float32(top_p))
                kept, above = (p * (vp >= th).numpy()).sum(-1), (p * (vp > th).numpy()).sum(-1)
                worst_low, worst_high = min(worst_low, float((kept - p32).min())), max(worst_high, float((above - p32).max()))
                assert (kept >= p32 - slack).all(), (top_k, top_p, float((kept - p32).min()))
                assert (above < p32 + slack).all(), (top_k, top_p, float((above - p32).max()))
                if top_p == 1.0 / 2048:
                    _report_diff(got, only_max, f"top_p 1/2048 against top_k 1, greedy {greedy}")
                # the same call without theta_out draws the same ids
                if top_p == 0.9:
                    again, _, _ = _draw(dev, n_tokens, level, seed, NM.DRAW_TEMPERATURE, greedy, top_k=top_k, top_p=top_p)
                    _report_diff(again, got, "without theta_out")
    # theta_out alone takes the nucleus arm with nothing cut: -inf everywhere, the ids of the plain entry
    got, _, theta = _draw(dev, n_tokens, level, seed, NM.DRAW_TEMPERATURE, False, theta=True)
    assert np.isneginf(theta).all()
    _report_diff(got, _sample(dev, n_tokens, level, seed, NM.DRAW_TEMPERATURE, False), "theta_out alone")
    REPORT[f"nar_draw_top_p_{TAG[dtype]}_k{n_tokens}"] = {"kept_minus_top_p_min": worst_low, "above_minus_top_p_max": worst_high, "slack": slack}
    print(f"top-p {TAG[dtype]} n_tokens={n_tokens}: kept - top_p >= {worst_low:.3e}, above - top_p <= {worst_high:.3e}, slack {slack:.3e}")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tokens", TOKENS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_known_frames_keep_their_code_and_move_no_other_frame(built_lib, dtype, n_tokens):
    seed, level = NM.DRAW_RUNS[2]
    dev = _grid_dev(n_tokens, dtype, True, True)
    known = (torch.arange(TR_MAX) % 3 == 0)[None].expand(B, TR_MAX).contiguous()
    held = torch.full((B, TR_MAX), HELD, dtype=torch.int32)
    inside = _frames_mask()
    k = known[inside].numpy()
    for kw in (dict(top_k=min(50, n_tokens), top_p=0.9), dict()):
        free, _, th_free = _draw(dev, n_tokens, level, seed, NM.DRAW_TEMPERATURE, False, theta=True, **kw)
        got, _, th = _draw(dev, n_tokens, level, seed, NM.DRAW_TEMPERATURE, False, known=known, held=held, theta=True, **kw)
        assert (got[k] == HELD).all()
        _report_diff(got[~k], free[~k], "frames that are not known")
        assert np.array_equal(np.isnan(th), k), "theta_out must be NaN exactly on the known frames"
        assert np.array_equal(th[~k], th_free[~k])
        # without theta_out and without logprob_out a known frame leaves before it reads its row
        got2, _, _ = _draw(dev, n_tokens, level, seed, NM.DRAW_TEMPERATURE, False, known=known, held=held, **kw)
        _report_diff(got2, got, "known frames without theta_out")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tokens", TOKENS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_logprob_is_the_log_softmax_of_the_rows_own_logits(built_lib, dtype, n_tokens):
    seed, level = NM.DRAW_RUNS[1]
    grid, dev = _grid(n_tokens, dtype, True), _grid_dev(n_tokens, dtype, True)
    rows = _rows_of(grid, n_tokens)
    ref = R.log_softmax64(rows)
    alive = torch.isfinite(rows.float()).any(-1).numpy()          # (a row that is -inf throughout has no log-softmax)
    inside = _frames_mask()
    known = (torch.arange(TR_MAX) % 3 == 0)[None].expand(B, TR_MAX).contiguous()
    held = torch.randint(0, n_tokens, (B, TR_MAX), generator=torch.Generator().manual_seed(9), dtype=torch.int32)
    k = known[inside].numpy()
    worst = 0.0

    def check(ids, lp, what):
        nonlocal worst
        want = ref[np.arange(len(ids)), ids]
        fin = alive & np.isfinite(want)
        assert np.isfinite(lp[fin]).all(), what
        err = float(np.abs(lp[fin] - want[fin]).max())
        worst = max(worst, err)
        print(f"logprob {TAG[dtype]} n_tokens={n_tokens} {what}: max |device - float64| = {err:.3e}")
        assert err <= LOGPROB_TOL, (what, err)
        dead = alive & np.isneginf(want)                            # a held id whose own logit is -inf
        assert np.isneginf(lp[dead]).all(), what

    ids, lp, _ = _draw(dev, n_tokens, level, seed, NM.DRAW_TEMPERATURE, False, logprob=True)
    check(ids, lp, "drawn")
    ids_k, lp_k, _ = _draw(dev, n_tokens, level, seed, NM.DRAW_TEMPERATURE, False, known=known, held=held, logprob=True)
    assert np.array_equal(ids_k[k], held[inside].long().numpy()[k]) and np.array_equal(ids_k[~k], ids[~k])
    check(ids_k, lp_k, "known every third frame")
    assert np.array_equal(lp_k[~k].view(np.uint32), lp[~k].view(np.uint32))
    # the value is a function of the row and of the id alone: the ids of a filtered draw, held as known under other options
    ids_f, lp_f, _ = _draw(dev, n_tokens, level, seed, 0.7, False, top_k=min(50, n_tokens), top_p=0.5, logprob=True)
    check(ids_f, lp_f, "top_k 50, top_p 0.5, T 0.7")
    everything = torch.ones(B, TR_MAX, dtype=torch.bool)
    held_f = torch.zeros(B, TR_MAX, dtype=torch.int32)
    held_f[inside] = torch.from_numpy(ids_f).to(torch.int32)
    for kw in (dict(), dict(top_k=1), dict(top_p=0.9, top_k=7)):
        for temperature in (1.0, NM.DRAW_TEMPERATURE):
            ids_h, lp_h, _ = _draw(dev, n_tokens, level, seed, temperature, True, known=everything, held=held_f, logprob=True, **kw)
            assert np.array_equal(ids_h, ids_f)
            same = lp_h.view(np.uint32)[alive] == lp_f.view(np.uint32)[alive]
            assert same.all(), f"the log-probability moved with {kw} T {temperature} on {int((~same).sum())} frames"
    REPORT[f"nar_draw_logprob_{TAG[dtype]}_k{n_tokens}"] = {"max_abs_err_vs_float64": worst, "bound": LOGPROB_TOL}


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_codes_and_write_nothing(built_lib):
    from vall_e.vall_e import _hip
    n_tokens = 1284
    logits = torch.zeros(1, 12, n_tokens, dtype=torch.bfloat16, device=DEV)
    lens = torch.tensor([[2, 3, 5]], dtype=torch.int32, device=DEV)
    resp = torch.full((1, 6, 8), RESP_POISON, dtype=torch.int32, device=DEV)
    lp = torch.full((1, 6, 7), LP_POISON, dtype=torch.float32, device=DEV)
    th = torch.full((1, 6), THETA_POISON, dtype=torch.float32, device=DEV)

    def call(top_p, top_k, n=n_tokens, temperature=0.2):
        d = _hip.NarDraw(top_p, top_k, None, lp.data_ptr(), th.data_ptr())
        return built_lib.d3pm_op_nar_draw(2, logits.data_ptr(), n_tokens, lens.data_ptr(), resp.data_ptr(), 6, 8, 12, n, 0, temperature, 7, 0, 0, 1,
                                          C.byref(d), None)
    E_ARG, E_SHAPE = -1, -4
    assert call(0.9, 50) == E_SHAPE and call(1.0, 0) == E_SHAPE                    # (logprob_out / theta_out make the call non-neutral)
    for top_k in (-1, 1025):
        assert call(1.0, top_k, n=1024) == E_ARG
    for top_p in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(top_p, 0, n=1024) == E_ARG
    for temperature in (0.0, -1.0, float("nan"), float("inf")):
        assert call(0.9, 50, n=1024, temperature=temperature) == E_ARG
    torch.cuda.synchronize()
    assert bool((resp == RESP_POISON).all()) and bool((lp == LP_POISON).all()) and bool((th == THETA_POISON).all())
    assert call(0.9, 50, n=1024) == 0                                              # the same buffers, accepted: the refusals were the options'
    torch.cuda.synchronize()
    assert bool((resp[0, :5, 1] >= 0).all()) and bool((resp[0, 5] == RESP_POISON).all())

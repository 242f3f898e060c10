"""The deduplicated sampler loop with the projections onto the residual stream on tiles sized to the estimated distinct rows
(csrc/d3pm_api.hip sample_loop_impl, csrc/d3pm_sequence.h LoopPlan::rows_est, csrc/d3pm_plan.cpp plan_distinct_rows / big_tile).

Every big-tile geometry gives the same bits, so ids and the trace of every iteration must agree byte for byte between ln_fold = 1 (the
estimate on, latency list on), 4 (the estimate on, big tiles in every iteration) and 3 (every row, no estimate).  16 utterances x 768
frames, d = 512, two layers is the smallest batch whose out-projections take big tiles: its capacity of 12 288 rows is the first
shipped threshold, so every big-tile iteration there runs its producers on 96 x 128 tiles -- entered from the latency list, at the end
of the schedule, and from a canvas of 768 distinct ids per utterance, where the live rows are the capacity, far above the estimate,
and the ids are still those of every row.  The thresholds themselves -- 96 x 128 tiles up to 12 288 estimated rows, 128 x 128 up to
16 384, 192 x 128 beyond -- are crossed at 32 utterances, in runs of five iterations around each, with the estimate recomputed here
from the sampler's schedule so that the test cannot pass without the crossing inside the run."""
import contextlib
import dataclasses
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANVAS = 768
SHORT96, SHORT128 = 12288, 16384      # live_short96_rows() / live_short128_rows(), pinned with the planner in tests/test_live_tiles_plan_api.py


def _cfg():
    from vall_e.vall_e import synth
    return dataclasses.replace(synth.D3PMConfig.libritts(), n_heads=8, n_layers=2, canvas=CANVAS, n_frames=700)


@contextlib.contextmanager
def _ln_fold(value):
    """3 and 4 are A/B values of the library; the `tuning` context manager lists the shipped schedules only"""
    from vall_e.vall_e import _hip
    saved = _hip.TUNING.ln_fold
    _hip.set_tuning_field("ln_fold", value)
    try:
        yield
    finally:
        _hip.set_tuning_field("ln_fold", saved)


@pytest.fixture(scope="module")
def setup(built_lib):
    from vall_e.vall_e import AR, synth
    cfg = _cfg()
    m = AR.from_config(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, 0))
    m = m.to(torch.bfloat16).to(DEV)
    smp = m.sampler()
    cache = {}

    def get(batch):
        if batch not in cache:
            texts, proms = synth.make_inputs(cfg, batch, 1)
            cache[batch] = smp.cond_kv(*m.encode_conditions(texts, proms))
        return cache[batch]
    cbar = smp.schedule.cbar.view(np.float16).astype(np.float32)      # cbar[t], the index sample_loop_impl reads

    def estimate(batch, t):      # plan_distinct_rows
        r = float(np.float32(CANVAS) * (np.float32(1.0) - cbar[t]))
        distinct = cfg.n_classes * (1.0 - math.exp(-r / cfg.n_classes)) if r > 0 else 0.0
        return batch * min(CANVAS, 2 + math.ceil(distinct))
    return cfg, m, smp, get, estimate


def _arms(smp, x0, fm, kv, t_start, t_stop, arms, what):
    out = {}
    for ln_fold in arms:
        x = x0.clone()
        with _ln_fold(ln_fold):
            tr = smp.sample_loop(x, fm, t_start, t_stop, kv[0], kv[1], seed=91, trace=True)
        torch.cuda.synchronize()
        out[ln_fold] = (x, tr)
    xa, ta = out[arms[0]]
    for ln_fold in arms[1:]:
        xb, tb = out[ln_fold]
        per_iter = (ta != tb).flatten(1).sum(dim=1).tolist()
        assert torch.equal(ta, tb), f"{what}: ids of the trace that differ between ln_fold = {arms[0]} and {ln_fold}, per iteration: {per_iter}"
        assert torch.equal(xa, xb), (what, ln_fold)
    print(what, "ids changed by the run:", int((xa != x0).sum()))
    return xa


def _distinct_canvas(batch):
    gen = torch.Generator().manual_seed(2)
    ids = torch.stack([torch.randperm(CANVAS, generator=gen) for _ in range(batch)]).to(torch.int32).to(DEV)      # 768 live rows per utterance
    return ids, torch.ones(CANVAS, dtype=torch.uint8, device=DEV)


def _crossing(cfg, estimate, batch, bound):
    """(t_start, t_stop, estimates) of five iterations whose third is the first with an estimate above `bound`"""
    t_x = max(t for t in range(1, cfg.timesteps) if estimate(batch, t) > bound)
    t_start, t_stop = t_x + 2, t_x - 3
    est = [estimate(batch, t) for t in range(t_start, t_stop, -1)]
    assert t_stop >= 0 and t_start < cfg.timesteps and est == sorted(est) and est[0] < est[1] <= bound < est[2] < est[3], (bound, est)
    return t_start, t_stop, est


@pytest.mark.parametrize("bound", [SHORT96, SHORT128])
def test_32_utterances_across_a_threshold(setup, bound):
    cfg, m, smp, get, estimate = setup
    B = 32
    t_start, t_stop, est = _crossing(cfg, estimate, B, bound)
    print("estimate passes", bound, "inside t =", t_start, "..", t_stop + 1, "estimates:", est)
    x, fm = m.canvas_init(B)
    out = _arms(smp, x, fm, get(B), t_start, t_stop, (1, 4, 3), f"32 utterances across {bound}")
    assert not torch.equal(out, x)


def test_16_utterances_at_the_end_of_the_schedule(setup):
    cfg, m, smp, get, estimate = setup
    B = 16
    assert all(0 < estimate(B, t) < B * CANVAS == SHORT96 for t in range(1, cfg.timesteps))      # 96 x 128 wherever tiles are big
    x, fm = m.canvas_init(B)
    out = _arms(smp, x, fm, get(B), 3, 0, (1, 4, 3), "16 utterances, t = 3 .. 1")
    assert not torch.equal(out, x)


def test_16_utterances_from_the_latency_list_to_96_row_tiles(setup):
    cfg, m, smp, get, estimate = setup
    B = 16
    # plan_live_rows, the estimate of the latency rule: the last iteration within 3840 rows and the four behind it
    cbar = smp.schedule.cbar.view(np.float16).astype(np.float32)
    live_rows = lambda t: B * min(CANVAS, 2 + math.ceil(max(float(np.float32(CANVAS) * (np.float32(1.0) - cbar[t])), 0.0)))      # noqa: E731
    t_sw = min(t for t in range(1, cfg.timesteps) if live_rows(t) <= 3840)
    assert all(0 < estimate(B, t) <= SHORT96 for t in range(t_sw - 3, t_sw + 2)), [estimate(B, t) for t in range(t_sw - 3, t_sw + 2)]
    x, fm = m.canvas_init(B)
    _arms(smp, x, fm, get(B), t_sw + 1, t_sw - 3, (1, 4, 3), "16 utterances, latency list -> 96 x 128")


def test_16_utterances_every_id_distinct(setup):
    cfg, m, smp, get, estimate = setup
    B = 16
    ids, ones = _distinct_canvas(B)                   # 12 288 live rows under an estimate of about 6 000
    assert estimate(B, 40) < 0.6 * B * CANVAS
    _arms(smp, ids, ones, get(B), 40, 37, (1, 4, 3), "16 utterances, every id distinct")


def test_32_utterances_every_id_distinct(setup):
    cfg, m, smp, get, estimate = setup
    B = 32
    t0 = _crossing(cfg, estimate, B, SHORT96)[0]      # two iterations on 96-row tiles, then 128-row ones: 24 576 live rows on both
    ids, ones = _distinct_canvas(B)
    _arms(smp, ids, ones, get(B), t0, t0 - 3, (1, 4), "32 utterances, every id distinct")

"""The self-attention of the deduplicated sampler loop in the iterations that expect few rows per utterance (csrc/d3pm_sequence.h
LoopPlan::seg_est, csrc/d3pm_plan.cpp attn_pool_rows, attn32p_hd64 POOL in csrc/d3pm_mfma_attn32.hip).

At the shape of tests/test_gpu_live_regime.py (16 utterances x 768 frames, d = 512, two layers) a reverse process is run from the top of
the schedule across both boundaries the host decides per iteration -- pooled -> gathered self-attention, and further down latency
GEMMs -> big tiles -- under ln_fold = 1 (everything on), 4 (the gathered attention and big tiles in every iteration) and 3 (every row):
ids and the trace of every iteration must agree byte for byte.  Which iterations are pooled is read from the planner itself
(tests/few_rows_plan_table.cpp, linked host-only, fed with the schedule the sampler uses), so the test cannot pass without pooled
iterations being followed by gathered ones.  A second case starts at the top from a canvas of 768 distinct ids per utterance: every
estimate is wrong, every pooled workgroup finds its utterance beyond the pool and walks the row index, and the ids are those of
ln_fold = 4."""
import os
import subprocess

import numpy as np
import pytest
import torch

import test_gpu_live_regime as LR

pytestmark = pytest.mark.gpu
DEV, B, CANVAS = LR.DEV, LR.B, LR.CANVAS


@pytest.fixture(scope="module")
def setup(built_lib, tmp_path_factory):
    from vall_e.vall_e import AR, synth
    cfg = LR._cfg()
    cache = {}

    def get(dtype):
        if dtype not in cache:
            m = AR.from_config(cfg)
            m.load_state_dict(synth.make_state_dict(cfg, 0))
            m = m.to(dtype).to(DEV)
            texts, proms = synth.make_inputs(cfg, B, 1)
            smp = m.sampler()
            cache[dtype] = (m, smp, smp.cond_kv(*m.encode_conditions(texts, proms)))
        return cache[dtype]

    tmp = tmp_path_factory.mktemp("few_rows_loop")
    plan_o, main_o, exe = (str(tmp / n) for n in ("d3pm_plan.o", "few_rows_plan_table.o", "few_rows_plan_table"))
    subprocess.run(LR.HOST_ONLY + ["-c", os.path.join(LR.CSRC, "d3pm_plan.cpp"), "-o", plan_o], check=True, timeout=600)
    subprocess.run(LR.HOST_ONLY + ["-c", os.path.join(LR.ROOT, "tests", "few_rows_plan_table.cpp"), "-o", main_o], check=True, timeout=600)
    subprocess.run([LR.HIPCC, plan_o, main_o, "-o", exe], check=True, timeout=600)
    cbar = get(torch.bfloat16)[1].schedule.cbar.view(np.float16).astype(np.float64)      # cbar[t], the index sample_loop_impl reads
    out = subprocess.run([exe, str(B), str(CANVAS)] + [repr(float(c)) for c in cbar], check=True, capture_output=True, text=True, timeout=600).stdout
    lines = [dict(kv.split("=", 1) for kv in line.split()[1:]) for line in out.splitlines()]
    bound = next(f for f in lines if "ATTN_32P_POOL" in f)
    iters = [f for f in lines if "latency" in f]
    assert len(iters) == cfg.timesteps
    pooled = [int(f["kernel"]) == int(bound["ATTN_32P_POOL"]) for f in iters]
    latency = [int(f["latency"]) == 1 for f in iters]
    return cfg, get, pooled, latency


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_ids_do_not_change_across_the_boundaries(setup, dtype):
    cfg, get, pooled, latency = setup
    m, smp, kv = get(dtype)
    t0 = cfg.timesteps - 1
    t_pool = min(t for t in range(cfg.timesteps) if pooled[t])        # the last pooled iteration
    t_lat = min(t for t in range(cfg.timesteps) if latency[t])        # the last iteration on the latency GEMMs
    assert pooled[t0] and all(pooled[t] for t in range(t_pool, t0 + 1)) and 3 <= t_lat < t_pool - 1 <= t0 - 3, (t_pool, t_lat)
    t_stop = t_lat - 3
    kinds = ["pool" if pooled[t] else "gather+panel64" if latency[t] else "gather+big" for t in range(t0, t_stop, -1)]
    print("iterations", t0, "..", t_stop + 1, {k: kinds.count(k) for k in dict.fromkeys(kinds)})
    assert kinds == sorted(kinds, key=["pool", "gather+panel64", "gather+big"].index) and kinds.count("gather+panel64") >= 2 and kinds.count("gather+big") == 2
    x, fm = m.canvas_init(B)
    out, _ = LR._arms(smp, x, fm, kv, t0, t_stop, (1, 4, 3), f"from the top across both boundaries {dtype}")
    assert not torch.equal(out, x)
    # ... and a run whose first, unprepared iteration is the first gathered one, entered from below the boundary
    LR._arms(smp, x, fm, kv, t_pool - 1, t_pool - 3, (1, 4), f"below the pool {dtype}")


def test_a_wrong_estimate_falls_back_to_the_row_index(setup):
    cfg, get, pooled, latency = setup
    m, smp, kv = get(torch.bfloat16)
    t0 = cfg.timesteps - 1
    assert pooled[t0] and pooled[t0 - 1] and pooled[t0 - 2]      # estimate: a few rows per utterance
    gen = torch.Generator().manual_seed(3)
    ids = torch.stack([torch.randperm(CANVAS, generator=gen) for _ in range(B)]).to(torch.int32).to(DEV)      # 768 live rows per utterance
    fm = torch.ones(CANVAS, dtype=torch.uint8, device=DEV)
    LR._arms(smp, ids, fm, kv, t0, t0 - 3, (1, 4), "every id distinct at the top of the schedule")

"""The host's bound on the live rows of a deduplicated iteration and the launch plans under it (csrc/d3pm_plan.cpp: plan_live_rows,
live_latency_rows, LinearArgs::m_est), pinned without a GPU.

tests/live_rows_plan_table.cpp links the planner host-only, as tests/launch_plan_table.cpp does.  Checked: the estimate is monotone in t
for a cosine schedule and stays within [2 * batch, batch * canvas]; with an estimate within the bound R every projection of a block -- the
dual cross-attention out-projection included -- plans onto gemm_mfma_panel64 with an epilogue its launcher instantiates and a grid that
covers min(M, m_est) rows; with no estimate, or one above R, the plans are the big-tile ones pinned in tests/test_launch_plan_api.py."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tts-with-diffusion-model_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST_ONLY = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", CSRC]
BATCH, CANVAS, T = 32, 768, 100
PROJECTIONS = ("qkv", "out", "q2", "cross", "fc1", "fc2")      # cross = both cross-attention out-projections in one launch
PANEL_TM = {0: 64, 1: 96, 2: 32}


def cosine_cbar(timesteps):
    """1 - alpha_bar of the cosine schedule (s = 0.008): the probability that a frame of x_t is still masked"""
    f = lambda i: math.cos((i / (timesteps + 1) + 0.008) / 1.008 * math.pi / 2) ** 2      # noqa: E731
    return [1.0 - f(t + 1) / f(0) for t in range(timesteps)]


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split()[1:])


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("live_rows_plan")
    plan_o, main_o, exe = (str(tmp / n) for n in ("d3pm_plan.o", "live_rows_plan_table.o", "live_rows_plan_table"))
    subprocess.run(HOST_ONLY + ["-c", os.path.join(CSRC, "d3pm_plan.cpp"), "-o", plan_o], check=True, timeout=600)
    subprocess.run(HOST_ONLY + ["-c", os.path.join(ROOT, "tests", "live_rows_plan_table.cpp"), "-o", main_o], check=True, timeout=600)
    subprocess.run([HIPCC, plan_o, main_o, "-o", exe], check=True, timeout=600)
    cbar = cosine_cbar(T)
    out = subprocess.run([exe, str(BATCH), str(CANVAS)] + [repr(c) for c in cbar + [0.0, 1.0, -0.25, 1.5]], check=True, capture_output=True,
                         text=True, timeout=600).stdout
    t = {"est": [], "latency": [], "linear": {}, "R": None}
    for line in out.splitlines():
        kind, f = line.split()[0], _fields(line)
        if kind == "bound":
            t["R"] = int(f["R"])
        elif kind == "est":
            t["est"].append(int(f["rows"]))
            t["latency"].append(int(f["latency"]))
        elif kind == "linear":
            t["linear"][(f["case"], int(f["B"]), int(f["m_est"]))] = f
    return t


def test_estimate_is_monotone_and_bounded(table):
    est, edge = table["est"][:T], table["est"][T:]
    print("R", table["R"], "estimate at t = 99, 90, 80, 70, 60, 50, 1:", [est[t] for t in (99, 90, 80, 70, 60, 50, 1)])
    assert all(est[t] >= est[t + 1] for t in range(T - 1)), "fewer masked frames at a smaller t: the estimate must not shrink"
    assert all(2 * BATCH <= e <= BATCH * CANVAS for e in est + edge)
    cbar = cosine_cbar(T)
    for t in range(T):      # batch * min(canvas, 2 + ceil(canvas * (1 - cbar_t))), in the library's fp32
        revealed = np.float32(CANVAS) * (np.float32(1.0) - np.float32(cbar[t]))
        assert est[t] == BATCH * min(CANVAS, 2 + math.ceil(max(float(revealed), 0.0))), t
    # cbar = 0 (nothing masked), 1 (all masked), and values outside [0, 1] stay inside the bounds
    assert edge == [BATCH * CANVAS, 2 * BATCH, BATCH * CANVAS, 2 * BATCH]
    # the regime rule is the comparison with R, and the top of a reverse process is a latency iteration at this shape
    assert table["latency"][:T] == [int(e <= table["R"]) for e in est]
    assert table["latency"][T - 1] == 1 and table["latency"][1] == 0


@pytest.mark.parametrize("utterances", [11, 16, 32])
def test_an_estimate_within_the_bound_plans_the_latency_family(table, utterances):
    R, M = table["R"], utterances * 768
    for m_est in sorted({1, 64, 385, R // 2, R}):
        for name in PROJECTIONS:
            f = table["linear"][(name, utterances, m_est)]
            assert f["kernel"] == "panel64" and f["listed"] == "1", (name, m_est, f)
            geom, tm = int(f["geom"]), int(f["tm"])
            assert tm == PANEL_TM[geom] and int(f["tn"]) == 64
            rows = min(M, m_est)
            assert int(f["grid"]) == -(-rows // tm) * -(-int(f["N"]) // 64), (name, m_est, f)      # the tile count of min(M, m_est)
            assert int(f["tiles_total"]) == -(-M // tm) * int(f["n_tiles"])                         # the capacity's
            if name == "cross":
                assert f["form"] == "1" and geom == 2                                               # CROSS_OUT_PANEL64_DUAL, 32 x 64


@pytest.mark.parametrize("utterances", [16, 32])
def test_without_an_estimate_the_plans_are_the_big_tile_ones(table, utterances):
    grids = {16: dict(qkv=512, out=256, q2=512, cross=256, fc1=512, fc2=256), 32: dict(qkv=512, out=512, q2=512, cross=512, fc1=512, fc2=512)}
    R, M = table["R"], utterances * 768
    for name in PROJECTIONS:
        f0 = table["linear"][(name, utterances, 0)]
        assert (f0["kernel"], f0["tm"], f0["tn"], int(f0["grid"])) == ("big", "192", "128", grids[utterances][name]), (name, f0)
        assert int(f0["epi"]) & 256 and f0["listed"] == "1"                                         # EPI_QUADS
        if name == "cross":
            assert f0["form"] == "2"                                                                 # CROSS_OUT_BIG_DUAL
        for m_est in (R + 1, M + 5):      # an estimate above the bound changes nothing
            f = dict(table["linear"][(name, utterances, m_est)])
            assert f.pop("m_est") == str(m_est)
            assert f == {k: v for k, v in f0.items() if k != "m_est"}, (name, m_est)

"""The self-attention plan of the deduplicated loop under the host's per-utterance row estimate (csrc/d3pm_plan.cpp: plan_attention
with AttnArgs::seg_est, attn_pool_rows), pinned without a GPU.

tests/few_rows_plan_table.cpp links the planner host-only, as tests/live_rows_plan_table.cpp does.  Checked: an estimate of 1 .. P rows
per utterance (P = attn_pool_rows(), read from the library) names the pooled kernel with a grid of ceil(seg_est / 128) query blocks per
(utterance, head), the pool of P rows and an LDS total inside a workgroup's 160 KiB; no estimate, an estimate above P, a call without
the segment key index or without gathered keys plan exactly as before; the new kernel value is appended to the enum; over a cosine
schedule the top of a reverse process is pooled and the pooled iterations are exactly those whose estimate is within P."""
import os
import subprocess

import pytest

from test_live_rows_plan_api import cosine_cbar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tts-with-diffusion-model_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST_ONLY = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", CSRC]
BATCH, CANVAS, T, HEADS = 32, 768, 100, 8
STATIC_LDS, LDS_LIMIT = 48 * 1024, 160 * 1024


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split()[1:])


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("few_rows_plan")
    plan_o, main_o, exe = (str(tmp / n) for n in ("d3pm_plan.o", "few_rows_plan_table.o", "few_rows_plan_table"))
    subprocess.run(HOST_ONLY + ["-c", os.path.join(CSRC, "d3pm_plan.cpp"), "-o", plan_o], check=True, timeout=600)
    subprocess.run(HOST_ONLY + ["-c", os.path.join(ROOT, "tests", "few_rows_plan_table.cpp"), "-o", main_o], check=True, timeout=600)
    subprocess.run([HIPCC, plan_o, main_o, "-o", exe], check=True, timeout=600)
    out = subprocess.run([exe, str(BATCH), str(CANVAS)] + [repr(c) for c in cosine_cbar(T)], check=True, capture_output=True, text=True,
                         timeout=600).stdout
    t = {"iter": [], "attn": {}}
    for line in out.splitlines():
        kind, f = line.split()[0], _fields(line)
        if kind == "bound":
            t.update({k: int(v) for k, v in f.items()})
        elif kind == "iter":
            t["iter"].append({k: int(v) for k, v in f.items()})
        elif kind == "attn":
            t["attn"][(f["case"], int(f["B"]), int(f["seg_est"]))] = {k: int(v) for k, v in f.items() if k != "case"}
    return t


def test_the_pooled_kernel_is_appended_to_the_enum(table):
    assert table["ATTN_32P"] == 1 and table["ATTN_32P_POOL"] == 7      # behind ATTN_TILES = 6: the older table programs print the values


def test_the_pool_fits_a_workgroup_at_the_loop_shape(table):
    P = table["P"]
    assert P >= 1 and STATIC_LDS + 4 * CANVAS + 256 * P <= LDS_LIMIT


@pytest.mark.parametrize("case", ["loop", "masked"])
@pytest.mark.parametrize("utterances", [16, 32])
def test_an_estimate_within_the_pool_names_the_pooled_kernel(table, utterances, case):
    P = table["P"]
    for seg_est in sorted({1, 2, 127, P}):
        f = table["attn"][(case, utterances, seg_est)]
        assert f["kernel"] == table["ATTN_32P_POOL"], (seg_est, f)
        assert f["masked"] == int(case == "masked")
        assert f["n_qblocks"] == -(-seg_est // 128) and f["grid"] == -(-seg_est // 128) * HEADS * utterances
        assert f["pool_rows"] == P and f["lds"] == 4 * CANVAS + 256 * P
        assert f["total_lds"] == STATIC_LDS + f["lds"] <= LDS_LIMIT


@pytest.mark.parametrize("case", ["loop", "masked", "no_seg_key", "no_gather"])
@pytest.mark.parametrize("utterances", [16, 32])
def test_nothing_changes_without_a_usable_estimate(table, utterances, case):
    P = table["P"]
    f0 = dict(table["attn"][(case, utterances, 0)])
    assert f0.pop("seg_est") == 0
    assert f0["kernel"] == table["ATTN_32P"] and f0["pool_rows"] == 0 and f0["n_qblocks"] == CANVAS // 128
    assert f0["grid"] == CANVAS // 128 * HEADS * utterances and f0["lds"] == (0 if case == "no_gather" else 4 * CANVAS)
    every = [1, 2, 127, P, P + 1, 2 * P, 768, 100000]
    for seg_est in (every if case in ("no_seg_key", "no_gather") else [P + 1, 2 * P, 768, 100000]):
        f = dict(table["attn"][(case, utterances, seg_est)])
        assert f.pop("seg_est") == seg_est
        assert f == f0, (case, seg_est)


def test_the_longest_gathered_canvas_still_fits(table):
    f = table["attn"][("long", 32, table["P"])]
    assert f["kernel"] == table["ATTN_32P_POOL"] and f["lds"] == 4 * 4096 + 256 * table["P"] and f["total_lds"] <= LDS_LIMIT


def test_a_pool_named_by_the_caller(table):
    fits, too_big = table["attn"][("named384", 2, 0)], table["attn"][("named512", 2, 0)]
    assert fits["kernel"] == table["ATTN_32P_POOL"] and fits["pool_rows"] == 384 and fits["n_qblocks"] == 1 and fits["grid"] == 8 * 2
    assert fits["lds"] == 4 * 512 + 256 * 384 and fits["total_lds"] <= LDS_LIMIT
    assert too_big["kernel"] == table["ATTN_32P"] and too_big["pool_rows"] == 0 and too_big["lds"] == 4 * 512      # 178 KiB: the gathered kernel


def test_the_pooled_iterations_of_a_reverse_process(table):
    P, it = table["P"], table["iter"]
    assert len(it) == T and [i["t"] for i in it] == list(range(T))
    for i in it:
        assert i["seg_est"] == -(-i["rows"] // BATCH)
        assert (i["kernel"] == table["ATTN_32P_POOL"]) == (i["seg_est"] <= P), i
        assert i["grid"] == (-(-i["seg_est"] // 128) if i["seg_est"] <= P else CANVAS // 128) * HEADS * BATCH
    pooled = [i["t"] for i in it if i["kernel"] == table["ATTN_32P_POOL"]]
    print("P", P, "pooled iterations", pooled[0] if pooled else None, "..", pooled[-1] if pooled else None)
    assert it[T - 1]["kernel"] == table["ATTN_32P_POOL"] and it[1]["kernel"] == table["ATTN_32P"]
    assert pooled == list(range(pooled[0], T)), "the estimate grows as t falls: the pooled iterations are the top of the schedule"

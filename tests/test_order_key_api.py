"""The order-key map of csrc/d3pm_order_key.h -- the one map behind the row cuts of both stages (filter_row / nucleus_row) and the
reveal order -- walked on the host, without a GPU.

tests/order_key_table.cpp includes that header alone, is built host-only like tests/live_tiles_plan_table.cpp and prints one line of
counts per storage type: f16 and bf16 over all 65 536 keys, fp32 over its edge patterns (+-0, +-inf, +-denorm_min, +-1, +-FLT_MAX)
and a fixed-seed sample of 2^20 patterns."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tts-with-diffusion-model_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST_ONLY = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", CSRC]
NON_NAN = {"f16": 63490, "bf16": 65282}      # 2 * (exponents below all-ones) * 2^mantissa + the two infinities


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("order_key")
    obj, exe = str(tmp / "order_key_table.o"), str(tmp / "order_key_table")
    subprocess.run(HOST_ONLY + ["-c", os.path.join(ROOT, "tests", "order_key_table.cpp"), "-o", obj], check=True, timeout=600)
    subprocess.run([HIPCC, obj, "-o", exe], check=True, timeout=600)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    print(out)
    return {line.split()[0]: {k: int(v) for k, v in (kv.split("=", 1) for kv in line.split()[1:])} for line in out.splitlines()}


def test_the_program_includes_the_header_alone():
    src = open(os.path.join(ROOT, "tests", "order_key_table.cpp")).read()
    assert [l for l in src.splitlines() if l.startswith("#include \"")] == ['#include "d3pm_order_key.h"']
    hdr = open(os.path.join(CSRC, "d3pm_order_key.h")).read()
    assert [l for l in hdr.splitlines() if l.startswith("#include")] == ['#include "d3pm_common.h"']


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_every_16_bit_key(table, name):
    t = table[name]
    assert t["keys"] == 65536 and t["nan"] == 65536 - NON_NAN[name]
    assert t["roundtrip_bad"] == 0          # order_key(order_value(k)) == k for every key whose value is not NaN
    assert t["decreasing"] == 0             # values are non-decreasing in the key
    assert t["equal_pairs"] == 1 and t["zero_pairs"] == 1      # two distinct keys with one value: those of -0 and +0, and no others
    assert t["below_one"] == 0 and t["key0_nan"] == 1          # every non-NaN value has a key >= 1: an empty slot's key 0 sits below all
    assert t["top_nan"] == 1                # the all-ones key is NaN (theta of a row that is -inf throughout)
    assert (t["key_neg_zero"], t["key_pos_zero"]) == (0x7FFF, 0x8000)
    assert 1 <= t["key_neg_inf"] < t["key_neg_zero"] < t["key_pos_zero"] < t["key_pos_inf"] < 0xFFFF
    assert t["key_pos_inf"] - t["key_neg_inf"] + 1 == NON_NAN[name]      # the non-NaN keys are one contiguous run


def test_fp32_edges_and_sample(table):
    t = table["f32"]
    assert t["edge"] == 10 and t["edge_bad"] == 0 and t["edge_order_bad"] == 0
    assert t["sample"] == 1 << 20 and t["sample_bad"] == 0 and t["sample_order_bad"] == 0
    assert 0 < t["nan"] < t["sample"] // 64      # 2^-8 of the patterns are NaNs: the sample met some and was not made of them
    assert t["key0_nan"] == 1 and t["top_nan"] == 1
    assert (t["key_neg_zero"], t["key_pos_zero"]) == (0x7FFFFFFF, 0x80000000)

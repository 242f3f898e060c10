"""Which kernel a projection or an attention call runs on (csrc/d3pm_plan.cpp), pinned without a GPU.

The planner is host code without a kernel, so tests/launch_plan_table.cpp links against it after a `hipcc --cuda-host-only` compile and
prints its choices; this module compiles both once, runs the program and reads its lines.  Pinned: the automatic choices of the
d = 512, 768-frame model in bf16 (DESIGN.md section 3 lists them), the edges the folded LayerNorm's format decision depends on, and the
attention regimes.  The sweep has no expected table: it checks properties every plan must have by itself, and every (family, epilogue,
geometry) it meets must be a `case` of that family's launcher -- a plan the dispatch switch does not have would otherwise only show
on a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tts-with-diffusion-model_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST_ONLY = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", CSRC]
EPI = dict(EPI_GELU=1, EPI_R1=2, EPI_R2=4, EPI_MASK=8, EPI_RELU=16, EPI_SILU=32, EPI_LNF=64, EPI_STATS=128, EPI_QUADS=256)


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split()[1:])


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("launch_plan")
    plan_o, main_o, exe = (str(tmp / n) for n in ("d3pm_plan.o", "launch_plan_table.o", "launch_plan_table"))
    subprocess.run(HOST_ONLY + ["-c", os.path.join(CSRC, "d3pm_plan.cpp"), "-o", plan_o], check=True, timeout=600)
    subprocess.run(HOST_ONLY + ["-c", os.path.join(ROOT, "tests", "launch_plan_table.cpp"), "-o", main_o], check=True, timeout=600)
    # the program walks the real launch sequence and loop plan: the two other host-only units of the library are linked with it, named
    # to the linker in a response file beside the program's own object
    program_o, unit_o = main_o, [str(tmp / n) for n in ("d3pm_sequence.o", "d3pm_schedule.o")]
    for obj in unit_o:
        subprocess.run(HOST_ONLY + ["-c", os.path.join(CSRC, os.path.basename(obj)[:-2] + ".cpp"), "-o", obj], check=True, timeout=600)
    (tmp / "objects.rsp").write_text("\n".join(f'"{o}"' for o in [program_o] + unit_o))
    main_o = "@" + str(tmp / "objects.rsp")
    subprocess.run([HIPCC, plan_o, main_o, "-o", exe], check=True, timeout=600)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=600).stdout
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "llvm-nm")
    t = {"linear": {}, "attn": {}, "cross": {}, "seen": set(), "violations": [], "sweep": None,
         "symbols": subprocess.run([nm, plan_o], check=True, capture_output=True, text=True).stdout}
    t.update({"sequence_symbols": subprocess.run([nm, unit_o[0]], check=True, capture_output=True, text=True).stdout,
              "program_symbols": subprocess.run([nm, program_o], check=True, capture_output=True, text=True).stdout,
              "block": {}, "step": {}, "plan": {}, "est": {}})
    for line in out.splitlines():
        kind, f = line.split()[0], _fields(line)
        if kind == "linear":
            t["linear"][f["case"]] = f
        elif kind == "attn":
            t["attn"][(f["case"], int(f["B"]))] = f
        elif kind == "cross":
            t["cross"][int(f["case"])] = int(f["form"])
        elif kind == "seen":
            t["seen"].add((int(f["family"]), int(f["epi"]), int(f["geom"])))
        elif kind == "violation":
            t["violations"].append(line)
        elif kind == "sweep":
            t["sweep"] = {k: int(v) for k, v in f.items()}
        elif kind == "block":
            t["block"][(f["case"], int(f["l"]))] = int(f["launches"])
        elif kind == "step":
            t["step"].setdefault((f["case"], int(f["l"])), []).append(f)
        elif kind == "plan":
            t["plan"][f["case"]] = {k: int(v) for k, v in f.items() if k != "case"}
        elif kind == "est":
            t["est"][int(f["t"])] = (int(f["rows"]), int(f["m_est"]))
    return t


def test_the_planner_holds_no_kernel(table):
    """A kernel in d3pm_plan.cpp would make its host-only object refer to the device code it does not carry (and the link above fail)."""
    assert "__hip_fatbin" not in table["symbols"] and "__hipRegister" not in table["symbols"]
    src = open(os.path.join(CSRC, "d3pm_plan.cpp")).read() + open(os.path.join(CSRC, "d3pm_plan.h")).read()
    src = re.sub(r"//[^\n]*", "", src)      # the comments may speak of launches
    assert "__global__" not in src and "<<<" not in src and not re.search(r"\bhip[A-Z]\w*\(", src)
    # ... and the same three checks for the launch sequence and the loop plan (csrc/d3pm_sequence.{h,cpp})
    assert "__hip_fatbin" not in table["sequence_symbols"] and "__hipRegister" not in table["sequence_symbols"]
    src = open(os.path.join(CSRC, "d3pm_sequence.cpp")).read() + open(os.path.join(CSRC, "d3pm_sequence.h")).read()
    src = re.sub(r"//[^\n]*", "", src)
    assert "__global__" not in src and "<<<" not in src and not re.search(r"\bhip[A-Z]\w*\(", src)
    # the program that walks them defines no function of the library (namespace d3pm, or the C ABI) itself: it would test a copy
    defined = [ln.split()[-1] for ln in table["program_symbols"].splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"]
    assert "main" in defined and not [s for s in defined if s.startswith("d3pm_")], defined
    ours = ("carve", "fold_plan", "loop_plan", "fold_features", "plan_linear", "plan_attention", "plan_cross_out", "set_error")
    assert not [s for s in defined if any(f"4d3pm{len(n)}{n}" in s for n in ours)], defined


BIG, GLDS = "big 192x128", "128glds 128x128"
P64, P96, P32 = "panel64 64x64", "panel64 96x64", "panel64 32x64"
# utterances -> (QKV 1536 x 512, out 512 x 512, merged q 1024 x 512, fc1 2048 x 512, fc2 512 x 2048, final 1025 x 512), each (kernel tile, grid)
AUTO = {
    1: ((P96, 192), (P32, 192), (P64, 192), (P96, 256), (P32, 192), (P64, 204)),
    2: ((P96, 384), (P64, 192), (P96, 256), (P96, 512), (P64, 192), (P64, 408)),
    3: ((GLDS, 216), (GLDS, 72), (GLDS, 144), (GLDS, 288), (GLDS, 72), (GLDS, 162)),
    8: ((BIG, 384), (GLDS, 192), (BIG, 256), (BIG, 512), (BIG, 128), (GLDS, 432)),
    10: ((BIG, 480), (GLDS, 240), (BIG, 320), (BIG, 512), (BIG, 160), (GLDS, 540)),
    11: ((BIG, 512), (GLDS, 264), (BIG, 352), (BIG, 512), (BIG, 176), (GLDS, 594)),
    16: ((BIG, 512), (BIG, 256), (BIG, 512), (BIG, 512), (BIG, 256), (GLDS, 864)),
    32: ((BIG, 512), (BIG, 512), (BIG, 512), (BIG, 512), (BIG, 512), (GLDS, 1728)),
}


def _choice(f):
    return (f["kernel"] if f["kernel"] == "generic" else f"{f['kernel']} {f['tile']}", int(f["grid"]))


@pytest.mark.parametrize("utterances", sorted(AUTO))
def test_automatic_projection_choices_at_768_frames(table, utterances):
    got = tuple(_choice(table["linear"][f"{name}/{utterances}"]) for name in ("qkv", "out", "q2", "fc1", "fc2", "final"))
    print(utterances, got)
    assert got == AUTO[utterances]


def test_projection_edges(table):
    lin = table["linear"]
    assert _choice(lin["qkv_table"]) == (P64, 432)          # the block-0 table projection, 1152 x 1536 x 512
    # M * N < 128^2 keeps a projection off the MFMA family: fold_plan then answers FOLD_NONE
    assert _choice(lin["out_rows16"])[0] == "generic" and _choice(lin["out_rows31"])[0] == "generic"
    assert _choice(lin["out_rows32"]) == (P64, 8)
    assert _choice(lin["native_qkv"])[0] == "generic"       # the upstream-native 448 x 96 x 32


@pytest.mark.parametrize("utterances", [8, 10, 11, 16, 32])
def test_fold_format_follows_the_tiles(table, utterances):
    """Quads need every moment-touching projection of folded_block on big tiles: so at 16 and 32 utterances, not at 8 .. 11 (the
    out-projections leave the chip too idle for big tiles there), where the moments travel as 32-column parts."""
    on_big = {name: table["linear"][f"fold_{name}/{utterances}"]["kernel"] == "big" for name in ("qkv", "out", "q2", "cross", "fc1", "fc2")}
    print(utterances, on_big, "cross-out form", table["cross"][utterances])
    if utterances >= 16:
        assert all(on_big.values()) and table["cross"][utterances] == 2      # CROSS_OUT_BIG_DUAL
    else:
        assert not on_big["out"] and not on_big["cross"] and table["cross"][utterances] == 0
        assert on_big["qkv"] and on_big["q2"] and on_big["fc1"] and on_big["fc2"]


def test_self_attention_choices(table):
    at = table["attn"]
    f = at[("self", 10)]
    assert (f["kernel"], f["qg"], f["pair"], f["grid"]) == ("attn_mfma_hd64", "1", "0", "960")
    assert (at[("self", 11)]["kernel"], at[("self", 11)]["grid"]) == ("attn32p_hd64", "528")
    assert (at[("self", 32)]["kernel"], at[("self", 32)]["grid"], at[("self", 32)]["masked"]) == ("attn32p_hd64", "1536", "0")
    assert at[("self_plain_walk", 32)]["kernel"] == "attn32_hd64"
    # a shard of four utterances of a batch of 32 takes the kernel of the whole batch
    assert (at[("self_regime32", 4)]["kernel"], at[("self_regime32", 4)]["grid"]) == ("attn32p_hd64", "192")
    f = at[("self_keylen_keeps", 32)]
    assert (f["kernel"], f["masked"]) == ("attn32p_hd64", "1")
    f = at[("self_keylen", 32)]
    assert (f["kernel"], f["qg"], f["pair"], f["grid"]) == ("attn_mfma_hd64", "2", "0", "1536")


def test_cross_attention_pair_choices(table):
    at = table["attn"]
    f = at[("cross", 1)]
    assert (f["kernel"], f["qg"], f["pair"], f["grid"], f["n_first"]) == ("attn_mfma_hd64", "1", "0", "192", "96")
    f = at[("cross", 10)]
    assert (f["kernel"], f["qg"], f["pair"], f["grid"]) == ("attn_mfma_hd64", "1", "1", "960")
    f = at[("cross", 11)]
    assert (f["kernel"], f["n_qsplit"], f["grid"], f["lds"]) == ("attn32_cross_hd64", "3", "264", "81920")
    f = at[("cross", 32)]
    assert (f["kernel"], f["n_qsplit"], f["grid"]) == ("attn32_cross_hd64", "1", "256")
    assert at[("cross_resident16", 32)]["kernel"] == "attn_cross_hd64"
    assert at[("cross_split", 1)]["kernel"] == "attn_split_hd64"


def test_sweep_properties(table):
    """Epilogue in the family's table, grid > 0, LDS <= 160 KiB, quads only on big tiles, a dual on geometry >= 2, ... (the program)."""
    print(table["sweep"])
    assert table["violations"] == []
    assert table["sweep"]["violations"] == 0 and table["sweep"]["planned"] > 50000 and table["sweep"]["attention"] > 5000


def _switch_cases(source, function):
    """The EPI values of the `case` labels of `function`'s dispatch switch, read from the launcher's source."""
    src = open(os.path.join(CSRC, source)).read()
    m = re.search(r"^int " + function + r"\(.*?^}\n", src, re.S | re.M)
    assert m, (source, function)
    vals = set()
    for expr in re.findall(r"\bcase ([^:]+):", m.group(0)):
        if re.fullmatch(r"(?:\s*(?:EPI_\w+|0)\s*\|?)+", expr):
            vals.add(eval(expr, {}, EPI))
    return vals


def test_every_plan_of_the_sweep_is_a_case_of_its_launcher(table):
    cases = {0: _switch_cases("d3pm_mfma_gemm.hip", "mfma_linear"), 1: _switch_cases("d3pm_mfma_gemm_big.hip", "big_linear"),
             2: _switch_cases("d3pm_mfma_gemm_lat.hip", "panel64_linear"), 3: _switch_cases("d3pm_mfma_gemm_big.hip", "big_dual"),
             4: _switch_cases("d3pm_mfma_gemm_lat.hip", "panel64_dual")}
    assert [len(cases[k]) for k in range(5)] == [12, 15, 10, 3, 2]
    seen = {k: {e for fam, e, _ in table["seen"] if fam == k} for k in range(5)}
    for k in range(5):
        assert seen[k] <= cases[k], (k, sorted(seen[k] - cases[k]))
        assert seen[k] == cases[k], (k, sorted(cases[k] - seen[k]))      # and the sweep reached every instantiated epilogue
    assert {g for fam, _, g in table["seen"] if fam == 1} == {1, 2, 3} and {g for fam, _, g in table["seen"] if fam == 2} == {0, 1, 2}
    assert {g for fam, _, g in table["seen"] if fam == 3} == {2, 3} and {g for fam, _, g in table["seen"] if fam == 4} == {2}


# ---- the launches of a folded block and the plan of a sampler loop (csrc/d3pm_sequence.{h,cpp}), walked by the program ----
# d = 512, 8 heads, 6 layers, 768 frames, 50 + 225 condition keys, 1025 classes, bf16, default tuning, the 100-step schedule
FOLD_NONE, FOLD_PARTS, FOLD_QUADS = 0, 1, 2
PROJECTIONS = ("qkv", "out", "q2", "fc1", "fc2")


def _block(table, case, l):
    steps = table["step"][(case, l)]
    assert len(steps) == table["block"][(case, l)] and [int(s["i"]) for s in steps] == list(range(len(steps)))
    return {s["name"]: s for s in steps}, [s["name"] for s in steps]


@pytest.mark.parametrize("utterances,per_block", [(2, 8), (8, 9), (16, 8), (32, 8)])
def test_launches_of_a_block(table, utterances, per_block):
    """folded_block as the loop launches it: block 0 reads its QKV rows from the table (one launch fewer), every other block projects."""
    case = f"b{utterances}"
    assert [table["block"][(case, l)] for l in range(6)] == [per_block - 1] + [per_block] * 5
    first, order0 = _block(table, case, 0)
    by_name, order = _block(table, case, 1)
    print(case, order)
    assert order[0] == "qkv" and order0 == order[1:] and "qkv" not in first
    cross = by_name["cross"]
    if utterances == 2:
        assert all(by_name[n]["kernel"] == "panel64" for n in PROJECTIONS)
        assert (cross["kind"], cross["kernel"], cross["form"]) == ("dual", "panel64", "1")
    elif utterances == 8:
        # two launches: o_text onto ws.h with no epilogue bit, then o_prompt + x + h with the moments
        text = by_name["cross_text"]
        assert (text["kind"], text["epi"]) == ("linear", "0") and order.index("cross_text") + 1 == order.index("cross")
        assert (cross["kind"], int(cross["epi"])) == ("linear", EPI["EPI_R2"] | EPI["EPI_STATS"])
    else:
        for n in PROJECTIONS:
            assert (by_name[n]["kernel"], by_name[n]["tile"]) == ("big", "192x128") and int(by_name[n]["epi"]) & EPI["EPI_QUADS"], n
        assert (cross["kind"], cross["kernel"], cross["tile"], cross["form"]) == ("dual", "big", "192x128", "2")
        assert int(cross["epi"]) & EPI["EPI_QUADS"]


def test_one_iteration_is_49_launches(table):
    """6 blocks of 8 launches, block 0 without its QKV projection, the final projection and the sampler launch."""
    assert sum(table["block"][("b32", l)] for l in range(6)) + 1 + 1 == 49


@pytest.mark.parametrize("utterances", [16, 32])
def test_latency_launch_list(table, utterances):
    """With the dedup index set and an estimate of 64 live rows: every projection on the 32 x 64 panel64 tile, the panel64 dual, and
    the two attention kernels of the deduplicated loop."""
    for l in (0, 1):
        by_name, order = _block(table, f"lat{utterances}", l)
        for n in PROJECTIONS[1 if l == 0 else 0:]:
            assert (by_name[n]["kernel"], by_name[n]["tile"], by_name[n]["live"]) == ("panel64", "32x64", "1"), (l, n)
        cross = by_name["cross"]
        assert (cross["kind"], cross["kernel"], cross["form"]) == ("dual", "panel64", "1")      # CROSS_OUT_PANEL64_DUAL
        assert (by_name["self_attn"]["kernel"], by_name["self_attn"]["segments"], by_name["self_attn"]["gather"]) == ("attn32p_hd64", "1", "1")
        assert (by_name["cross_attn"]["kernel"], by_name["cross_attn"]["segments"]) == ("attn32_cross_hd64", "1")


def _plan(fold, table, dedup, latency=None):
    first, last = latency if latency else (-1, -1)
    return dict(fold=fold, table=int(table), dedup=int(dedup), latency=int(latency is not None), first=first, last=last,
                count=first - last + 1 if latency else 0)


LOOP_PLANS = {
    "b32": _plan(FOLD_QUADS, True, True, (99, 74)),      # exactly 26 latency iterations
    "b16": _plan(FOLD_QUADS, True, True, (99, 62)),      # exactly 38
    "b8": _plan(FOLD_PARTS, True, False),
    "b2": _plan(FOLD_PARTS, True, False),
    # 32 utterances otherwise
    "ln_fold4": _plan(FOLD_QUADS, True, True),
    "ln_fold3": _plan(FOLD_QUADS, True, False),
    "ln_fold2": _plan(FOLD_QUADS, False, False),
    "ln_fold0": _plan(FOLD_NONE, False, False),
    "fp8": _plan(FOLD_NONE, False, False),
    "force_generic": _plan(FOLD_NONE, False, False),
    "known": _plan(FOLD_QUADS, True, True),
    "guided": _plan(FOLD_QUADS, False, False),
    "n_q8": _plan(FOLD_QUADS, False, False),
    "one_iteration": _plan(FOLD_QUADS, False, False),
}


@pytest.mark.parametrize("case", sorted(LOOP_PLANS))
def test_loop_plan(table, case):
    print(case, table["plan"][case])
    assert table["plan"][case] == LOOP_PLANS[case]
    assert LOOP_PLANS["b32"]["count"] == 26 and LOOP_PLANS["b16"]["count"] == 38


def test_live_row_estimates_at_the_switch(table):
    """The numbers of d3pm_plan.cpp's comment on D3PM_LIVE_LATENCY_ROWS: t = 74 is the last latency iteration of 32 utterances."""
    assert table["est"][74] == (3776, 3776) and table["est"][73] == (4064, 0)


def test_ln_fold_codes_are_read_in_one_function():
    """The integer codes of d3pm_tuning.ln_fold are compared with a number in fold_features (d3pm_plan.cpp) and nowhere else."""
    hits = {}
    for name in sorted(os.listdir(CSRC)):
        for m in re.finditer(r"ln_fold\s*(==|!=)\s*[0-9]", re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())):
            hits.setdefault(name, []).append(m.group(0))
    assert list(hits) == ["d3pm_plan.cpp"] and len(hits["d3pm_plan.cpp"]) == 5, hits

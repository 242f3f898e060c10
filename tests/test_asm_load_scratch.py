"""The GEMM kernels that issue `global_load_*` from inline asm and wait for them with a hand-counted vmcnt must not spill in their
folded-LayerNorm instantiations (EPI_LNF: the row moments in flight across the epilogue; EPI_STATS: the moments they leave).  hipcc
takes an asm destination register as valid once the statement is issued; a spill would store it stale and the load would land in
a register that by then holds something else.  The list of sources is found by grepping for the idiom, so a new file that adopts it
is covered without editing this test.  Cross-compiles for gfx950, no GPU."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tts-with-diffusion-model_amd", "csrc")
EPI_LNF, EPI_STATS = 64, 128


def _asm_load_sources():
    out = []
    for p in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        src = open(p).read()
        if re.search(r'asm\s+volatile\s*\(\s*"global_load_\w+', src) and re.search(r"s_waitcnt vmcnt\(", src):
            out.append(os.path.basename(p))
    return out


def test_the_idiom_is_found():
    assert "d3pm_mfma_gemm_big.hip" in _asm_load_sources()


@pytest.mark.parametrize("src", _asm_load_sources())
def test_folded_instantiations_compile_without_scratch(src):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), src], capture_output=True, text=True,
                         timeout=1500).stdout
    checked = 0
    for line in out.splitlines():
        m = re.search(r"I(?:DF16_|DF16b)Li(\d+)E", line)     # first template argument after the 16-bit type: the EPI bits
        if not m or not int(m.group(1)) & (EPI_LNF | EPI_STATS):
            continue
        r = re.search(r"scratch\s+(\d+)", line)
        assert r and int(r.group(1)) == 0, f"{src}: folded instantiation with scratch: {line}"
        checked += 1
    if src == "d3pm_mfma_gemm_big.hip":
        # 16-bit types x geometries x (LNF, LNF + GELU, R1 / R2 / R1 + mask + STATS) x (parts, quads), + the dual out-projection
        assert checked >= 60, out[-2000:]

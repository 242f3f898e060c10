#!/usr/bin/env python3
"""Are the kernels of a csrc file the ones another revision compiled?  Cross-compiles each named file for gfx950 to assembly (device
only; no GPU needed) in the working tree and in a checkout of REV, and compares every kernel's body by symbol: the lines from its
`_Z...:` label to its `.Lfunc_end`, comments stripped.  Exit status 1 if a kernel differs, is missing or is new.

    python tools/kernel_bodies.py [--rev HEAD] d3pm_sample.hip d3pm_reveal.hip d3pm_logprob.hip"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "tts-with-diffusion-model_amd"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden", "--cuda-device-only", "-S"]


def bodies(tree, name, tmp, tag):
    out = os.path.join(tmp, f"{tag}_{name}.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(tree, PKG, "csrc", name), "-o", out], check=True)
    text = open(out).read()
    found = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        m = re.search(r"^" + re.escape(sym) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
        assert m, sym
        lines = (re.sub(r"\s*;.*", "", l).rstrip() for l in m.group(1).splitlines())
        found[sym] = [l for l in lines if l]
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("files", nargs="+")
    args = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        ref = os.path.join(tmp, "ref")
        os.makedirs(ref)
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.rev, PKG + "/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", ref], input=tar, check=True)
        jobs = [(tree, name, tag) for name in args.files for tree, tag in ((ref, "ref"), (ROOT, "new"))]
        with ThreadPoolExecutor(min(len(jobs), 8)) as pool:
            res = list(pool.map(lambda j: bodies(j[0], j[1], tmp, j[2]), jobs))
        for k, name in enumerate(args.files):
            old, new = res[2 * k], res[2 * k + 1]
            differ = sorted(s for s in old.keys() | new.keys() if old.get(s) != new.get(s))
            print(f"{name}: {len(old)} kernels at {args.rev}, {len(new)} here, {len(differ)} differ")
            for s in differ:
                print("   ", "missing here" if s not in new else "new here" if s not in old else "body differs", s)
            bad += len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

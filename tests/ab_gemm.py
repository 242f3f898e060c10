"""Interleaved A/B of GEMM schedules inside one process: medians over alternating repetitions.
arguments: <variant>[m<big mode>] ...   variants: 2 = 128x128 persistent (round-1 default), 6 = 192x256 big tile,
7 = 96x512 big tile, 8 = 192x128 big tile, 9 = the five-slab ring; big modes: 1 hand-placed reads (shipped), 0 compiler-placed reads,
9 = deferred stores, 2049 = all DMA pieces at the top of a k-step (all: same results).  The probe builds with parts of the kernel
removed and the clock read-out (m17 .. m465, m257 in profiles/round2_a_ab_gemm.txt and round4_gemm_clock_under_load.txt) existed up
to commit 4442690 and can be recovered from there."""
import math, statistics, sys, torch
sys.path[:0] = ["tts-with-diffusion-model_amd", "."]
import __graft_entry__ as g
g.build_ab()                       # libd3pm_hip_ab.so (include/d3pm_hip_ab.h): big modes other than 1 and the ring are not in the product
from vall_e.vall_e import _hip
_hip.use_ab_library()
DEV, dtype = "cuda", torch.bfloat16
ARMS = [(int(a.split("m")[0]), int(a.split("m")[1]) if "m" in a else 1) for a in (sys.argv[1:] or ["2", "6", "7", "8", "0"])]
for arm in ARMS:
    if arm[1] not in (0, 1, 9, 2049):
        sys.exit(f"v{arm[0]}m{arm[1]}: big mode {arm[1]} is not built any more (0, 1, 9, 2049 are; see the docstring)")


def timeit(f, n=10):
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


shapes = [("qkv", 24576, 1536, 512, 0, False), ("merged-q", 49152, 512, 512, 0, False), ("proj", 24576, 512, 512, 0, True),
          ("fc1+gelu", 24576, 2048, 512, 1, False), ("fc2+res", 24576, 512, 2048, 0, True)]
for name, M, N, K, act, res in shapes:
    x = torch.randn(M, K, device=DEV).to(dtype); w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(dtype)
    b = torch.randn(N, device=DEV).to(dtype); y = torch.empty(M, N, device=DEV, dtype=dtype)
    r = torch.randn(M, N, device=DEV).to(dtype) if res else None
    f = lambda: _hip.op_linear(x, w, b, act=act, r1=r, family=_hip.FAMILY_MFMA, out=y, ldy=N)
    res_t = {a: [] for a in ARMS}
    outs = {}
    for rep in range(7):
        for arm in ARMS:
            _hip.set_gemm_ring(arm[0] == 9); _hip.set_gemm_variant(0 if arm[0] == 9 else arm[0]); _hip.set_gemm_big_mode(arm[1])
            res_t[arm].append(timeit(f))
            if rep == 0:
                outs[arm] = y.clone()
    ref = next(iter(outs.values()))
    same = all(torch.equal(ref, o) for o in outs.values())
    line = f"{name:9s}"
    for arm in ARMS:
        t = statistics.median(res_t[arm])
        line += f" | v{arm[0]}m{arm[1]}: {t:6.1f} us {2 * M * N * K / t / 1e6:6.0f} TF/s"
    print(line + f" | bit-identical: {same}", flush=True)
_hip.set_gemm_variant(0); _hip.set_gemm_big_mode(1); _hip.set_gemm_ring(False)

"""Interleaved A/B of GEMM schedules inside one process: medians over alternating repetitions.
arguments: <variant> ...   d3pm_tuning.gemm_variant: 2 = 128x128 persistent (round-1 default), 6 = 192x256 big tile, 7 = 96x512 big tile,
8 = 192x128 big tile, 0 = the automatic choice (all: same results).  The five-slab ring and the big-tile modes other than the shipped
one (compiler-placed reads, deferred stores, all DMA pieces at the top of a k-step) existed up to commit d54b189, the probe builds
with parts of the kernel removed up to commit 4442690; their figures are in profiles/ (round2_a_ab_gemm.txt and later)."""
import math, statistics, sys, torch
sys.path[:0] = ["tts-with-diffusion-model_amd", "."]
from vall_e.vall_e import _hip
DEV, dtype = "cuda", torch.bfloat16
ARMS = [int(a) for a in (sys.argv[1:] or ["2", "6", "7", "8", "0"])]


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
            _hip.set_gemm_variant(arm)
            res_t[arm].append(timeit(f))
            if rep == 0:
                outs[arm] = y.clone()
    ref = next(iter(outs.values()))
    same = all(torch.equal(ref, o) for o in outs.values())
    line = f"{name:9s}"
    for arm in ARMS:
        t = statistics.median(res_t[arm])
        line += f" | v{arm}: {t:6.1f} us {2 * M * N * K / t / 1e6:6.0f} TF/s"
    print(line + f" | bit-identical: {same}", flush=True)
_hip.set_gemm_variant(0)

"""Interleaved timing of the schedules of the MFMA self-attention kernel (not a test): python tests/ab_attn.py [arm ...]
Arms (d3pm_tuning.attn_query_groups): the shipped kernel (QG 2) and QG 1; both give the same bits, which is asserted.  QG 3, hand-placed
fragment reads (164) and K / V by direct-to-LDS DMA (228) existed up to commit d54b189, the builds with parts of the kernel removed
(101 .. 160) and the occupancy probes (201 / 202) up to commit 4442690; their figures are in profiles/."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tts-with-diffusion-model_amd"), ROOT]
from vall_e.vall_e import _hip  # noqa: E402

DEV = "cuda:0"
B, T, H, d = 32, 768, 8, 512
torch.manual_seed(0)
qkv = torch.randn(B, T, 3 * d, device=DEV).to(torch.bfloat16)
q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]


def timeit(fn, reps=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


ARMS = [(2, "shipped (QG 2)"), (1, "QG 1")]
arms = [int(a) for a in sys.argv[1:]] or [a for a, _ in ARMS]
names = dict(ARMS)
for arm in arms:
    if arm not in names:
        sys.exit(f"arm {arm} is not built any more ({', '.join(str(a) for a in names)} are; see the docstring)")
flops = 4.0 * B * H * T * T * 64
ref = None
for arm in arms:
    _hip.set_attn_query_groups(arm)
    o = _hip.op_attention(q, k, v, H, 0.125, family=_hip.FAMILY_MFMA)      # every arm must give the shipped kernel's bits
    ref = o.clone() if ref is None else ref
    assert torch.equal(o, ref), f"arm {arm}: output differs from the first arm"
    t = timeit(lambda: _hip.op_attention(q, k, v, H, 0.125, family=_hip.FAMILY_MFMA))
    print("%-28s %7.1f us  %6.0f TFLOP/s-equivalent" % (names.get(arm, str(arm)), t, flops / t / 1e6), flush=True)
_hip.set_attn_query_groups(0)

"""Row moments of the folded LayerNorm in the quad format (csrc/d3pm_mfma_tile.h EpiFold, d3pm_api.hip fold_plan).

When every projection of the folded sequence runs on big tiles (d = 512, throughput batches) the producers leave one (sum, sum of
squares) per 128 columns instead of one per 32, summed in the order every consumer used to sum the 32-column parts.  At one or two
utterances (panel64) and mid-size batches (128 x 128 tiles) the sequence keeps the parts.  Checked here:
  * one folded denoiser evaluation at batches {1, 2, 3, 8, 11, 32} is bit-identical to one utterance of it evaluated alone under the
    same attention regime -- a one-utterance evaluation runs the part format throughout, so every mixture of formats and kernel
    families gives the same bits;
  * folded projections the MFMA family cannot take (batch x canvas < 32 at d = 512, < 64 at d = 256) no longer fail or read stale
    moments: the evaluation takes the LayerNorm launches and agrees with ln_fold = 0.
"""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(cfg, dtype):
    from vall_e.vall_e import AR, synth
    m = AR.from_config(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, 0))
    return m.to(dtype).to(DEV)


def _canvas(m, cfg, B, seed):
    x, fm = m.canvas_init(B)
    gen = torch.Generator().manual_seed(seed)
    live = torch.rand(B, cfg.canvas, generator=gen) < 0.5
    ids = torch.randint(0, 1024, (B, cfg.canvas), generator=gen, dtype=torch.int32)
    return torch.where(live.to(DEV) & (x != 0), ids.to(DEV), x), fm


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_folded_denoiser_is_bit_identical_across_moment_formats(built_lib, dtype):
    from vall_e.vall_e import _hip, synth
    cfg = synth.D3PMConfig.libritts()
    m = _model(cfg, dtype)
    smp = m.sampler()
    assert smp.folded
    texts, proms = synth.make_inputs(cfg, 32, 1)
    ct, cp = m.encode_conditions(texts, proms)
    x, fm = _canvas(m, cfg, 32, 9)
    for B in (1, 2, 3, 8, 11, 32):
        kv_t, kv_p = smp.cond_kv(ct[:B].contiguous(), cp[:B].contiguous())
        with _hip.tuning(regime_batch=B):
            lg = smp.denoise(x[:B].contiguous(), fm, 40, kv_t, kv_p)[0].clone()
        k = B - 1                                   # the last utterance, alone, told the batch it belongs to
        kv_t1, kv_p1 = smp.cond_kv(ct[k:k + 1].contiguous(), cp[k:k + 1].contiguous())
        with _hip.tuning(regime_batch=B):
            lg1 = smp.denoise(x[k:k + 1].contiguous(), fm, 40, kv_t1, kv_p1)[0]
        assert torch.equal(lg1, lg[k:k + 1]), f"batch {B}: utterance {k} alone differs from the batch"


@pytest.mark.parametrize("d", [256, 512])
@pytest.mark.parametrize("rows", [16, 32, 48])
def test_small_folded_sequences_agree_with_the_layernorm_launches(built_lib, d, rows):
    """at batch x canvas below the MFMA family's minimum the folded sequence used to hand its producers to
    the generic GEMM, which ignores stats_out, so the consumers read stale moments (or the consumer launch failed with
    D3PM_E_SHAPE).  Now the whole evaluation takes the LayerNorm launches there."""
    from vall_e.vall_e import _hip, synth
    dtype = torch.float16
    cfg = dataclasses.replace(synth.D3PMConfig.libritts(), d_model=d, n_heads=8, n_layers=2, canvas=16, n_frames=12, s_prompt=32)
    m = _model(cfg, dtype)
    smp = m.sampler()
    B = rows // cfg.canvas
    texts, proms = synth.make_inputs(cfg, B, 1)
    ct, cp = m.encode_conditions(texts, proms)
    kv_t, kv_p = smp.cond_kv(ct, cp)
    x, fm = _canvas(m, cfg, B, 4)
    lg_f = smp.denoise(x, fm, 40, kv_t, kv_p)[0].clone()
    with _hip.tuning(ln_fold=0):
        lg_u = smp.denoise(x, fm, 40, kv_t, kv_p)[0].clone()
    assert torch.isfinite(lg_f.float()).all()
    assert (lg_f.float() - lg_u.float()).abs().max().item() < 8e-3

"""Host side of the block-0 QKV table (include/d3pm_hip.h: d3pm_tuning.ln_fold value 2, d3pm_workspace_bytes): no GPU needed.
The device side is tests/test_gpu_qkv_table.py."""
import ctypes as C

import pytest
import torch


def _align(v):
    return (v + 255) & ~255


def _workspace_before_the_table(cfg, batch, es=2):
    """d3pm_workspace_bytes as it was before the table (aliased layout, n_q = 1, 16-bit, d a multiple of 256): x, h, h2, the shared
    qkv | mlp | logits region, att, the row moments, the fp8 scale slot, fc1's folded copy and its two fp32 vectors."""
    n, d, L = batch * cfg.canvas, cfg.d_model, cfg.n_layers
    ldl = (cfg.n_classes + 7) & ~7
    total = 3 * _align(n * d * es) + _align(max(n * 4 * d * es, n * ldl * es)) + _align(n * d * es)
    total += _align(((n + 15) & ~15) * (d // 32) * 2 * 4) + _align(2 * n * (d // 32))
    total += _align(L * 4 * d * d * es) + 2 * _align(L * 4 * d * 4)
    return total


def test_ln_fold_2_is_a_shipped_value(built_lib):
    from vall_e.vall_e import _hip
    assert _hip.TUNING.ln_fold == 1
    with _hip.tuning(ln_fold=2) as t:
        assert t.ln_fold == 2
    assert _hip.TUNING.ln_fold == 1
    with pytest.raises(_hip.D3PMError):
        with _hip.tuning(ln_fold=3):
            pass
    assert _hip.ABI_VERSION == 6 and built_lib.d3pm_abi_version() == 6
    assert "d3pm_op_embed_qkv" in _hip.SIGNATURES and "d3pm_op_embed_qkv_bytes" in _hip.SIGNATURES


@pytest.mark.parametrize("batch", [1, 4, 32])
def test_workspace_is_the_same_for_every_ln_fold_and_grew(built_lib, batch):
    from vall_e.vall_e import _hip, synth
    cfg = synth.D3PMConfig.libritts()
    sizes = []
    for ln_fold in (0, 1, 2):
        tn = _hip.Tuning()
        built_lib.d3pm_tuning_default(C.byref(tn))
        tn.ln_fold = ln_fold
        sizes.append(built_lib.d3pm_workspace_bytes(C.byref(_hip.make_shape(cfg, torch.bfloat16, tn)), batch))
    assert sizes[0] == sizes[1] == sizes[2] > 0
    before = _workspace_before_the_table(cfg, batch)
    n, d, mt = batch * cfg.canvas, cfg.d_model, 1152      # 1026 table rows padded to a multiple of 192 and of 128
    grew = _align(mt * d * 2) + _align(mt * (d // 32) * 2 * 4) + _align(mt * 3 * d * 2) + _align(n * d * 2)
    assert sizes[1] == before + grew, (sizes[1], before, grew)
    # an fp32 model and an n_q = 8 model have no table: nothing to pay for
    assert built_lib.d3pm_op_embed_qkv_bytes(C.byref(_hip.make_shape(cfg, torch.float32)), 16) == 0
    assert built_lib.d3pm_op_embed_qkv_bytes(C.byref(_hip.make_shape(synth.D3PMConfig.libritts_8q(), torch.bfloat16)), 16) == 0
    assert built_lib.d3pm_op_embed_qkv_bytes(C.byref(_hip.make_shape(cfg, torch.bfloat16)), 16) > mt * 4 * d * 2


def test_loop_refuses_the_workspace_size_from_before_the_table(built_lib):
    """The size check comes before the first launch, so the call needs no device: every pointer below is a placeholder that the
    library does not dereference before it returns D3PM_E_WORKSPACE."""
    from vall_e.vall_e import _hip, synth
    cfg = synth.D3PMConfig.libritts()
    sh = _hip.make_shape(cfg, torch.bfloat16)
    batch = 2
    blocks = (_hip.BlockWeights * cfg.n_layers)()
    w = _hip.Weights(256, 256, 256, 256, blocks, None)
    sched = _hip.Schedule(cfg.timesteps)
    fake = C.c_void_p(256)
    old = _workspace_before_the_table(cfg, batch)
    assert old < built_lib.d3pm_workspace_bytes(C.byref(sh), batch)
    rc = built_lib.d3pm_sample_loop(C.byref(sh), C.byref(w), batch, fake, fake, 10, 0, fake, fake, fake, C.byref(sched.c_struct), 1, 0, 0,
                                    fake, old, None, None)
    assert rc == -2, (rc, built_lib.d3pm_last_error())      # D3PM_E_WORKSPACE
    assert b"workspace" in built_lib.d3pm_last_error()

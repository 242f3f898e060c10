"""Training-step dropout of the condition encoders, host side (no GPU): the C-ABI entries, the `dropout=` argument parser, and
a numpy mirror of the mask stream (include/d3pm_hip.h "Dropout of the two condition encoders"; DESIGN.md "Dropout mask stream"),
which the GPU tests (tests/test_gpu_train_dropout.py) compare the kernels against bit for bit."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import philox

STREAM_DROPOUT = 3
NEW_ENTRIES = ("d3pm_op_dropout_f32", "d3pm_op_attention_dropout_f32", "d3pm_op_attention_bwd_dropout_f32")


def mask_u(seed: int, utt: int, site: int, n: int) -> np.ndarray:
    """fp32 uniforms of logical elements 0 .. n-1: counter (idx >> 2, utt, site, 3), word idx & 3, (word >> 8) 2^-24."""
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox.philox4x32_10(g, utt, site, STREAM_DROPOUT, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = np.stack(words, axis=-1).reshape(-1)[:n]
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def mask_z(seed: int, utt: int, site: int, n: int, p: float) -> np.ndarray:
    """The factor of each element: s = 1 / (1 - p) in fp32 where u >= p (kept), 0 where dropped."""
    p32 = np.float32(p)
    s = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(mask_u(seed, utt, site, n) >= p32, s, np.float32(0.0)).astype(np.float32)


def test_new_entries_are_declared_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _hip.SIGNATURES, name
        assert hasattr(built_lib, name), name


def test_dropout_probs_parses_the_argument():
    from vall_e.vall_e.train import dropout_probs
    assert dropout_probs(False) == (0.0, 0.0)
    assert dropout_probs(None) == (0.0, 0.0)
    assert dropout_probs(True) == (0.1, 0.01)
    assert dropout_probs((0.2, 0.0)) == (0.2, 0.0)
    assert dropout_probs([0, 0.5]) == (0.0, 0.5)
    assert dropout_probs((np.float32(0.25), 0.125)) == (0.25, 0.125)


@pytest.mark.parametrize("bad", [(-0.1, 0.01), (0.1, 1.0), (1.5, 0.0), (0.1, -1e-9), (float("nan"), 0.0), (0.1,), (0.1, 0.1, 0.1),
                                 ("0.1", 0.01), (True, 0.0), "00", 0.1, 1, {"p": 0.1}, (None, 0.0)])
def test_dropout_probs_rejects_out_of_range_and_malformed(bad):
    from vall_e.vall_e.train import dropout_probs
    with pytest.raises(ValueError):
        dropout_probs(bad)


def test_dropout_site_layout():
    from vall_e.vall_e.train import MLP_LAYER, dropout_site
    assert dropout_site(0, 0, 0) == 0
    assert dropout_site(0, 1, 3) == 0x13
    assert dropout_site(1, MLP_LAYER, 1) == 0x1F1


@pytest.mark.parametrize("p", [0.01, 0.1, 0.5])
def test_mirror_keep_rate(p):
    n = 1_000_000
    keep = int((mask_u(2024, 0, 0x101, n) >= np.float32(p)).sum())
    sigma = (n * p * (1 - p)) ** 0.5
    assert abs(keep - n * (1 - p)) < 5 * sigma, (keep, n * (1 - p), sigma)
    z = mask_z(2024, 0, 0x101, 1000, p)
    assert set(np.unique(z).tolist()) <= {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}


def test_mirror_keys_give_different_masks():
    n, p = 4096, 0.1
    base = mask_z(7, 0, 0x12, n, p)
    for seed, utt, site in ((7, 0, 0x13), (7, 0, 0x112), (7, 1, 0x12), (8, 0, 0x12), (7 | (1 << 40), 0, 0x12)):
        other = mask_z(seed, utt, site, n, p)
        assert not np.array_equal(base, other), (seed, utt, site)
    assert np.array_equal(base, mask_z(7, 0, 0x12, n, p))
    # a prefix of a longer draw is the shorter draw (the index is logical, not tied to the extent)
    assert np.array_equal(mask_z(7, 0, 0x12, 1001, p), base[:1001])

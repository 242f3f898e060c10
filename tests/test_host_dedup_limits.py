"""The shape limits of d3pm_op_dedup_index_align (include/d3pm_hip.h) are refused on the host, before anything is launched: no GPU needed.
dedup_embed_rows keeps the prefix of the utterance counts in 48 KiB of LDS, so a batch above 12283 is D3PM_E_SHAPE with a message."""
import ctypes as C

import numpy as np
import pytest

E_ARG, E_SHAPE = -1, -4
MAX_BATCH = 12 * 1024 - 5


def _call(lib, batch, canvas, n_classes=1025, seg_align=1):
    buf = np.zeros(64, np.int32)      # never read or written: every case below is refused before the first launch
    p = C.c_void_p(buf.ctypes.data)
    return lib.d3pm_op_dedup_index_align(1, p, p, batch, canvas, n_classes, 512, seg_align, None, p, p, p, p, p, p, None, None, p, None)


@pytest.mark.parametrize("batch", [MAX_BATCH + 2, 12288, 3 * 8192])      # 12285 and 12288: multiples of 3, so batch * 128 is one of 384
def test_batch_above_the_lds_prefix_is_refused(built_lib, batch):
    assert batch > MAX_BATCH and batch * 128 % 384 == 0
    assert _call(built_lib, batch, 128) == E_SHAPE
    assert f"at most {MAX_BATCH} utterances".encode() in built_lib.d3pm_last_error()


def test_the_other_shape_rules_are_refused_first(built_lib):
    assert _call(built_lib, 3, 100) == E_SHAPE and b"multiple of 128" in built_lib.d3pm_last_error()
    assert _call(built_lib, 4, 128) == E_SHAPE and b"multiple of 384" in built_lib.d3pm_last_error()
    assert _call(built_lib, 3, 128, n_classes=4096) == E_SHAPE and b"at most 4095 classes" in built_lib.d3pm_last_error()
    assert _call(built_lib, 3, 128, seg_align=64) == E_ARG

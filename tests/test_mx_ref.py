"""tests/mx_ref.py (the MX format written from the header's text: scale by search, codes by a table) against the package's torch
quantiser (_hip.quantize_mx / mx_scale_bytes / dequantize_mx: arithmetic on the fp32 bits, torch's float8_e4m3fn cast), without a
GPU.  The two hosts share no code; they must agree bit for bit on everything the GPU tests feed the kernels, so that a disagreement
on the GPU is the kernel's."""
import pytest
import torch

import gemm_exact_ref as R
import mx_ref as X

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]


def _hip():
    from vall_e.vall_e import _hip
    return _hip


def _same(x, what):
    c, s = X.quantize(x)
    rc, rs = _hip().quantize_mx(x)
    assert torch.equal(s, rs), f"{what}: {int((s != rs).sum())} scale bytes differ"
    assert torch.equal(c, rc), f"{what}: {int((c != rc).sum())} codes differ"
    assert int((c & 0x7F).max()) <= 0x7E, f"{what}: the NaN code"
    # (as fp32: the largest bf16 value, 255 x 2^120, rounds to the code of 256 at scale 2^120, which fp32 cannot hold)
    assert torch.equal(X.dequantize(c, s).float(), _hip().dequantize_mx(c, s)), what
    return c, s


def test_the_code_table_is_torchs_e4m3():
    codes = torch.arange(256, dtype=torch.uint8)
    finite = (codes & 0x7F) != 0x7F
    assert torch.equal(X.values_of(codes[finite]), codes[finite].view(torch.float8_e4m3fn).double())
    assert torch.equal(X.codes_of(X.values_of(codes[finite])), codes[finite])      # -0 keeps its sign bit (0x80)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_random_blocky_operands_and_the_quantiser_cases_of_the_gpu_tests(dtype):
    for K in X.QUANT_K:
        for M in X.QUANT_M:
            _same(X.quantiser_operand(M, K, dtype, 7 * K + M), f"{M}x{K}")
    g = torch.Generator().manual_seed(5)
    _same(torch.randn(64, 1024, generator=g) * torch.exp2(torch.randint(-40, 40, (64, 32), generator=g).float()).repeat_interleave(32, dim=1), "fp32 blocky")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_planted_block_and_what_it_must_give(dtype):
    blocks = X.planted_blocks(dtype)
    n = (len(blocks) + 3) // 4
    x = torch.zeros(n * 4, 32, dtype=torch.float64)
    for i, (_, v) in enumerate(blocks):
        x[i] = v
    c, s = _same(x.reshape(n, 128).to(dtype), "planted")
    assert torch.equal(X.quantiser_operand(384, 128, dtype, 0).reshape(-1, 32)[:len(blocks)].double(), x[:len(blocks)]), "M = 384 holds every case"
    c, s = c.reshape(-1, 32), s.permute(0, 2, 1).reshape(-1)
    at = {name: i for i, (name, _) in enumerate(blocks)}
    assert s[at["zero_block"]] == 1 and bool((c[at["zero_block"]] == 0).all())
    assert s[at["minus_zero_block"]] == 1 and bool((c[at["minus_zero_block"]] == 0x80).all())
    assert c[at["minus_zero_beside_values"]][:4].tolist() == [0x80, 0x70, 0x80, 0xFC] and s[at["minus_zero_beside_values"]] == 127 + 1 - 8
    for E in (-3, 0, 5):
        assert s[at[f"max_1.75_2^{E}"]] == 127 + E - 8 and c[at[f"max_1.75_2^{E}"]][0] == 0x7E            # 448
        assert s[at[f"max_-1.75_2^{E}"]] == 127 + E - 8 and c[at[f"max_-1.75_2^{E}"]][31] == 0xFE
        assert s[at[f"max_1.8125_2^{E}"]] == 127 + E - 7 and c[at[f"max_1.8125_2^{E}"]][0] == 0x76        # 232: halfway between 224 and 240
        # 32 2^E -> scale 2^(E - 3), code 256; 17 and 19 -> 136 and 152, halfway on the grid of 16: to the even codes 128 and 160
        assert s[at[f"tie_17_19_32_2^{E}"]] == 127 + E - 3 and c[at[f"tie_17_19_32_2^{E}"]][:5].tolist() == [0x70, 0x72, 0x78, 0xF0, 0xF2]
    top = at["largest_finite"]
    assert s[top] == (15 if dtype == torch.float16 else 127) + 127 - 7 and c[top][0] == 0x78 and c[top][1] == 0xF8
    if dtype == torch.bfloat16:
        assert s[at["bf16_subnormals"]] == 1 and s[at["bf16_subnormals_top"]] == 1 and s[at["bf16_clamped_normal"]] == 1
        assert c[at["bf16_clamped_normal"]][3] == 0x7E and s[at["bf16_first_unclamped"]] == 2
        assert bool((c[at["bf16_subnormals_top"]] != 0x80).all()), "127 2^-133 is 2^-126 x 0.99: not zero at the clamped scale"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_finite_16_bit_value_as_a_block_maximum(dtype):
    """All 65 536 bit patterns, the finite ones each as the maximum of a block of its own (the rest of the block: a half, a
    sixteenth and an eleventh of it, rounded to the type)."""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    v = torch.where(torch.isfinite(v), v, torch.zeros_like(v)).double()
    assert torch.equal(X.scale_bytes(v.abs()), _hip().mx_scale_bytes(v.abs().float()))
    x = torch.zeros(65536, 32, dtype=torch.float64)
    x[:, 5], x[:, 6], x[:, 7], x[:, 8] = v, (v / 2).to(dtype).double(), (-v / 16).to(dtype).double(), (v / 11).to(dtype).double()
    c, s = _same(x.reshape(512, 4096).to(dtype), "block maxima")
    assert torch.equal(s.permute(0, 2, 1).reshape(-1), X.scale_bytes(x.to(dtype).double().abs().amax(dim=1)))


def test_dyadic_operands_of_every_gemm_shape_are_exact_in_fp32():
    """The round trip and the bound are asserted by dyadic_mx_operands; fp32 x @ w.T equals float64 in the natural and in a permuted
    k order, both hosts agree on the operands, and the expected outputs of the two epilogues are what torch's own types give."""
    for (M, N, K) in X.GEMM_SHAPES:
        o = X.dyadic_mx_operands(M, N, K, M + N + K)
        assert o["bound"] < X.EXACT_QUANTA
        x32, w32 = o["x"].float(), o["w"].float()
        assert torch.equal((x32 @ w32.T).double(), o["acc"])
        perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
        assert torch.equal((x32[:, perm] @ w32[:, perm].T).double(), o["acc"])
        rc, rs = _hip().quantize_mx(x32)
        assert torch.equal(rc, o["x8"]) and torch.equal(rs, o["sx"])
        if M * N <= 576 * 640:
            for dtype in DTYPES:
                mask = (torch.arange(X.MASK_PERIOD) % 3 != 1).to(torch.uint8)
                got = X.expected_16bit(o["x"], o["w"], o["bias"], dtype, r1=o["r1"], row_mask=mask, mask_period=X.MASK_PERIOD)
                eager = (o["r1"].to(dtype) + ((x32 @ w32.T) + o["bias"].float()).to(dtype)) * (mask[torch.arange(M) % X.MASK_PERIOD] != 0).to(dtype)[:, None]
                assert torch.equal(got.view(torch.int16), eager.view(torch.int16))
            c, s = X.expected_mx(o["x"], o["w"], o["bias"])
            rc, rs = _hip().quantize_mx((x32 @ w32.T) + o["bias"].float())
            assert torch.equal(c, rc) and torch.equal(s, rs)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_gelu_sweep_keeps_every_block_maximum_off_the_scale_boundaries(dtype):
    bias, N = X.gelu_sweep_bias(dtype)
    assert N % 256 == 0
    vals = R.finite_values(dtype)
    seen = torch.zeros(65536, dtype=torch.bool)
    seen[bias.view(torch.int16).long() & 0xFFFF] = True
    assert bool(seen[vals.view(torch.int16).long() & 0xFFFF].all()), "a value of the sweep is missing"
    v = bias.double()
    g = X.gelu_tanh64(v)
    gm, arg = g.abs().view(-1, 32).max(dim=1)
    delta = X.gelu_tanh_delta(v, g).view(-1, 32).gather(1, arg[:, None])[:, 0]
    dist = X.boundary_distance(gm)
    assert bool((dist > X.SWEEP_MARGIN).all()), f"{int((dist <= X.SWEEP_MARGIN).sum())} block maxima within the margin of a boundary"
    assert bool((dist * gm > 16 * delta).all()), "the margin does not cover the error bound of the kernel's GELU"
    # the bound itself: far below the e4m3 grid, and the tanh form is the one the source states (within 5e-4 of the erf form)
    assert bool((X.gelu_tanh_delta(v, g) <= g.abs() * 2.0 ** -15 + X.TINY).all())
    erf_form = 0.5 * v * torch.special.erfc(-v / 2.0 ** 0.5)
    assert float((g - erf_form).abs().max()) < 5e-4


def test_boundary_distance():
    d = X.boundary_distance(torch.tensor([1.75, 7.0, 3.5 * (1 + 2.0 ** -10), 1.0, 0.0, 448 * 2.0 ** -126, 0.9999], dtype=torch.float64))
    assert d[0] == 0 and d[1] == 0 and abs(float(d[2]) - 2.0 ** -10) < 1e-12 and abs(float(d[3]) - 1 / 7) < 1e-12 and d[4] == float("inf") and d[5] == float("inf")
    assert abs(float(d[6]) - (0.9999 - 0.875) / 0.875) < 1e-9

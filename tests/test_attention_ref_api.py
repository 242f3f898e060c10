"""tests/attention_ref.py on the CPU: the crafted inputs have the properties the GPU tests rely on, a faithful emulation of the
contract passes the derived bound in both evaluation orders, and each of the mistakes the bound is meant to catch fails it -- at the
key where the mistake was made.  No GPU, no library."""
import pytest
import torch

import attention_ref as R

DTYPES = [torch.float16, torch.bfloat16]
B, H = 2, 2
SCALE = 0.125


def _recover(q, k, dtype, order, mutation=None):
    S = k.shape[1]
    return R.recover_probabilities(lambda v: R.emulate(q, k, v, SCALE, dtype, order, mutation), B, S, H, dtype)


def _report(q, k, dtype, order, mutation=None):
    return R.check_probabilities(_recover(q, k, dtype, order, mutation), R.softmax_fp64(q, k, SCALE), R.probability_bound(q, k, SCALE, dtype),
                                 dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("S", [1, 33, 64, 65, 130, 256, 768])
def test_selector_inputs_are_one_hot_far_below_fp32_rounding(dtype, S):
    for reverse in (False, True):
        q, k, pi, gap = R.selector_inputs(B, H, max(S, 16), S, dtype, seed=S, reverse=reverse)
        assert float(gap.min()) >= 40.0, float(gap.min())
        assert torch.equal(q.float().abs(), torch.full_like(q.float(), 4.0)) and torch.equal(k.float().abs(), torch.full_like(k.float(), 4.0))
        assert float((R.scores_fp64(q, k, SCALE) * R.LOG2E).max()) < 200.0           # well inside fp32 (and inside fp16 in natural units: 128)
        p = R.softmax_fp64(q, k, SCALE)
        assert torch.equal(p.argmax(-1), pi.view(1, 1, -1).expand(B, H, -1))
        assert float((p.amax(-1) - 1.0).abs().max()) < 2.0 ** -39


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_probe_values_return_the_probability_matrix(dtype):
    S, Tq = 130, 7
    q, k = R.flat_inputs(B, H, Tq, S, dtype, seed=1)
    p = R.softmax_fp64(q, k, SCALE)
    got = R.recover_probabilities(lambda v: R.attention_fp64(q, k, v, SCALE), B, S, H, dtype)
    assert got.shape == p.shape and float((got - p).abs().max()) < 1e-15
    for blk in range(R.n_blocks(S)):
        v = R.probe_values(B, S, H, blk, dtype)
        assert int(v.sum()) == B * H * (min(64, S - 64 * blk))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("S", [65, 130, 256])
def test_flat_inputs_are_all_in_the_relative_class_and_the_bound_is_a_few_percent(dtype, S):
    q, k = R.flat_inputs(B, H, 64, S, dtype, seed=S)
    p = R.softmax_fp64(q, k, SCALE)
    assert bool((p >= 2.0 ** -12 * p.amax(-1, keepdim=True)).all())
    assert float(p.min()) >= 2.0 * R.smallest_normal(dtype)          # no subnormal rounding anywhere on this family
    rel = R.probability_bound(q, k, SCALE, dtype)
    assert float(rel.max()) < (0.06 if dtype == torch.bfloat16 else 0.008), float(rel.max())      # a dropped or doubled key is 100 %


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("S", [200, 256])
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_steered_offsets_fall_on_the_intended_side_of_the_deferral(dtype, S, family):
    q, k, off = R.steered_inputs(family, B, H, 32, S, dtype, seed=3)
    assert R.steps_on_intended_side(family, off), off
    if family in ("all_negative", "falling"):
        assert float((R.scores_fp64(q, k, SCALE) * R.LOG2E).max()) < 0.0          # the first-tile reference is negative
    # the offsets are what the float64 scores show: tile means differ by the realised steps up to the flat part's noise
    s = (R.scores_fp64(q, k, SCALE) * R.LOG2E)[..., :(S // 64) * 64].reshape(B, H, 32, S // 64, 64).mean(-1).mean((0, 1, 2))
    assert float((s - off[:S // 64]).abs().max()) < 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("order", ["eager", "tiled"])
def test_emulation_of_the_contract_passes_the_bound_on_every_family(dtype, order):
    worst = 0.0
    for S in (65, 130, 256):
        q, k = R.flat_inputs(B, H, 48, S, dtype, seed=10 + S)
        rep = _report(q, k, dtype, order)
        assert rep.ok and rep.frac_relative == 1.0, f"flat S={S}: {rep}"
        worst = max(worst, rep.worst_ratio)
    for family in sorted(R.FAMILIES):
        for S in (200, 256):
            q, k, _ = R.steered_inputs(family, B, H, 48, S, dtype, seed=20 + S)
            rep = _report(q, k, dtype, order)
            assert rep.ok, f"{family} S={S}: {rep}"
            worst = max(worst, rep.worst_ratio)
    print(f"emulation {order} {dtype}: worst error / bound {worst:.3f}")
    for S, Tq in ((65, 100), (130, 200), (256, 256)):
        q, k, pi, _ = R.selector_inputs(B, H, Tq, S, dtype, seed=S)
        v = torch.randn(B, S, H * 64, generator=torch.Generator().manual_seed(S)).to(dtype)
        assert torch.equal(R.emulate(q, k, v, SCALE, dtype, order), v[:, pi])


def _mutation_case(mutation, dtype):
    """(q, k, key columns where the mistake must show) on the family that exposes it."""
    S = 130
    if mutation == "no_rescale":            # only a maximum that rises by more than 2^8 takes the rescale
        q, k, _ = R.steered_inputs("rising_over", B, H, 48, 256, dtype, seed=5)
        return q, k, range(0, 192)          # the tiles in front of the last raise keep a weight that is too large
    q, k = R.flat_inputs(B, H, 48, S, dtype, seed=6)
    where = {"drop_last_key": range(S - 1, S), "double_last_key": range(S - 1, S), "shift_keys_in_last_tile": range(128, S),
             "swap_value_tiles": range(0, 128)}[mutation]
    return q, k, where


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_each_mistake_fails_the_bound_where_it_was_made(dtype, mutation):
    q, k, where = _mutation_case(mutation, dtype)
    for order in (("tiled",) if mutation == "no_rescale" else ("eager", "tiled")):
        assert _report(q, k, dtype, order).ok                                   # the same inputs pass without the mistake
        rep = _report(q, k, dtype, order, mutation)
        assert rep.worst_ratio > 1.0 and not rep.ok, f"{mutation} {order}: {rep}"
        assert rep.worst_at[3] in where, f"{mutation} {order}: failed at key {rep.worst_at[3]}, expected one of {where}"
        # the mistakes renormalise: the rows still sum to 1, so only the per-key comparison sees them
        assert mutation == "no_rescale" or rep.row_sum_err <= rep.row_sum_limit and rep.small_violations == 0, rep


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_each_mistake_and_the_selector(dtype, mutation):
    """Four of the five return a wrong V row on selector inputs.  Counting the last key twice cannot: its query then holds the
    weights (1, 1) on two copies of the same row and (v + v) / 2 = v exactly -- which is why the probe test exists."""
    S, Tq = 130, 130
    q, k, pi, _ = R.selector_inputs(B, H, Tq, S, dtype, seed=7)
    v = torch.randn(B, S, H * 64, generator=torch.Generator().manual_seed(8)).to(dtype)
    for order in (("tiled",) if mutation == "no_rescale" else ("eager", "tiled")):
        wrong = (R.emulate(q, k, v, SCALE, dtype, order, mutation) != v[:, pi]).any(-1)          # [B, Tq]
        rows = set(torch.nonzero(wrong.any(0)).flatten().tolist())
        if mutation == "double_last_key":
            assert not rows
            continue
        expect = {"drop_last_key": {S - 1}, "shift_keys_in_last_tile": {128, 129}, "swap_value_tiles": set(range(128)),
                  "no_rescale": set(range(64, S))}[mutation]
        assert rows and rows <= expect, f"{mutation} {order}: wrong rows {sorted(rows)}"
        if mutation != "no_rescale":
            assert rows == expect, f"{mutation} {order}: wrong rows {sorted(rows)}"


def test_key_len_masks_exactly_and_the_bound_ignores_masked_keys():
    dtype = torch.float16
    q, k = R.flat_inputs(4, H, 8, 130, dtype, seed=9)
    kl = [1, 64, 65, 130]
    k_poison = k.clone()
    for b, n in enumerate(kl):
        k_poison[b, n:] = 240.0
    p = R.softmax_fp64(q, k_poison, SCALE, kl)
    for b, n in enumerate(kl):
        assert torch.equal(p[b, ..., n:], torch.zeros_like(p[b, ..., n:]))
        assert torch.equal(p[b:b + 1, ..., :n], R.softmax_fp64(q[b:b + 1], k[b:b + 1, :n], SCALE))
    assert torch.equal(R.probability_bound(q, k_poison, SCALE, dtype, kl)[1], R.probability_bound(q[1:2], k[1:2, :64], SCALE, dtype)[0])

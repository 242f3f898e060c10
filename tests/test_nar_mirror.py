"""The mirrors of tests/nar_mirror.py against the oracle (no GPU), and what the inputs of tests/test_gpu_nar_kernels.py must have for
that file's statements to mean something: the two-mirror AdaLN measurement that its caps rest on, the share of bf16 rows on which the
rounding of logit / T decides the greedy id, and the smallest Gumbel margin of the draw inputs."""
import math

import numpy as np
import pytest
import torch

import nar_mirror as NM
from oracle import nar_oracle as N

F32_TOL = 1e-4      # the fp32 criterion of tests/test_gpu_kernels.py: relative to the output scale


def test_embed_mirror_equals_the_oracle_in_fp32():
    """merged_sequence + sinusoid_pe on clean ids (the oracle takes no id outside the table); an utterance with fewer prompt levels
    is the oracle's codes[:, :k] and the mirror's -1 in the levels behind."""
    for d, n_given in ((128, 1), (512, 4)):
        inp = NM.embed_inputs(d, torch.float32, n_given)
        K = NM.EMBED_TOKENS
        for name in ("text", "prom", "resp"):                          # in-range ids where the kernel would clamp; -1 stays "absent"
            t = inp[name]
            t[(t >= K) & (t != 9999)] = K - 1
            if name != "prom":
                t[t < 0] = 0
        inp["prom"][1, 6, :] = 5                                        # the oracle has no row without any level
        inp["prom"][3, :2, :] = 7
        inp["prom"][3, :2, 3:] = -1                                     # three leading levels
        x, row_mask, key_len = NM.embed_mirror(**inp)
        sd = {"text_emb.weight": inp["w_text"], "proms_emb.weight": inp["w_prom"], "resps_emb.weight": inp["w_resp"], "sep": inp["sep"]}
        for b, (tt, tp, tr) in enumerate(NM.EMBED_LENS):
            levels = {2: 4, 3: 3}.get(b, NM.EMBED_LEVELS)
            ref = N.merged_sequence(sd, inp["text"][b, :tt].long(), inp["prom"][b, :tp, :levels].long(), inp["resp"][b, :tr, :n_given].long())
            total = tt + tp + tr + 2
            ref = ref + N.sinusoid_pe(total, d, torch.float32)
            assert int(key_len[b]) == total == len(ref) and row_mask[b].tolist() == [1] * total + [0] * (inp["t_max"] - total)
            assert (x[b, :total] - ref).abs().max().item() <= F32_TOL * ref.abs().max().item(), (d, b)
            assert not x[b, total:].any()


def test_embed_mirror_rounds_where_the_kernel_rounds():
    """bf16, one prompt row by hand: the level sum is rounded once, then the sum with the positional row once more."""
    inp = NM.embed_inputs(128, torch.bfloat16, 1)
    x, _, _ = NM.embed_mirror(**inp)
    b, row = 1, 2                                                       # utterance 1, prompt row 2: all eight levels present
    tt = NM.EMBED_LENS[b][0]
    acc = torch.zeros(128)
    for l in range(NM.EMBED_LEVELS):
        acc = acc + inp["w_prom"][l][int(inp["prom"][b, row, l])].float()
    want = (acc.bfloat16().float() + inp["pe"][tt + 1 + row].float()).bfloat16()
    assert torch.equal(x[b, tt + 1 + row], want)
    once = (acc + inp["pe"][tt + 1 + row].float()).bfloat16()
    assert not torch.equal(want, once), "the inner rounding is invisible on this row"


def test_adaln_mirror_equals_the_oracle_in_fp32():
    x, table, mask, _ = NM.adaln_inputs(512, torch.float32)
    emb = table[NM.ADALN_LEVEL]
    got = NM.adaln_mirror(x, emb, mask)
    ref = N.adaln(x.double(), emb.double()) * mask.double()[:, None]
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= F32_TOL * ref.abs().max().item()
    assert not got[mask == 0].any()


@pytest.mark.parametrize("d", [128, 512, 768, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_adaln_mirror_alone_stays_under_the_caps(dtype, d):
    """The measurement the caps of the GPU test rest on, on that test's own inputs: the mirror with float64 moments against the
    mirror with fp32 moments, and against the mirror with rstd moved by one fp32 step.  A kernel whose moments are fp32 sums in
    another order can differ from the mirror by about this much and no more; the GPU test allows 1e-3 differing and 64 ulp."""
    x, table, mask, kind = NM.adaln_inputs(d, dtype)
    emb = table[NM.ADALN_LEVEL]
    ref = NM.adaln_mirror(x, emb, mask)
    assert torch.isfinite(ref.float()).all()
    for what, other in (("fp32 moments", NM.adaln_mirror(x, emb, mask, stats=torch.float32)),
                        ("rstd + 1 ulp", NM.adaln_mirror(x, emb, mask, rstd_ulps=1)),
                        ("rstd - 1 ulp", NM.adaln_mirror(x, emb, mask, rstd_ulps=-1))):
        differ, worst = NM.lp_error(other, ref, dtype)
        print(f"adaln mirror alone {dtype} d={d} {what}: {differ:.2e} differing, worst {worst:.1f} ulp")
        assert differ < 3e-4 and worst < 64, (what, differ, worst)
    # what the special rows are for
    live = mask.bool()
    assert not ref[~live].any() and torch.equal(ref[live & (kind == 3)], emb[d:].expand(int((live & (kind == 3)).sum()), d))
    eps6 = NM.adaln_mirror(x, emb, mask, eps=1e-6)
    small = live & (kind == 1)
    assert (eps6[small] != ref[small]).float().mean().item() > 0.5, "the sigma = 1e-2 rows do not see eps"
    # a device expf one fp32 step away from torch's cannot flip a whole column of these inputs
    assert not NM.exp_near_boundary(emb[:d], dtype).any()


def test_adaln_small_launches_are_the_leading_rows():
    kind, mask = NM.adaln_row_kinds()
    assert kind[:4].tolist() == [0, 1, 2, 3] and mask[:5].tolist() == [1, 1, 1, 1, 0]
    assert 0.2 < 1.0 - mask.float().mean().item() < 0.3
    assert NM.ADALN_ROWS % 4 == 3 and mask[-1] == 1                      # a ragged last workgroup whose last row is live


@pytest.mark.parametrize("n_tokens", [1024, 1023, 6])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_draw_mirror_equals_the_oracle(dtype, n_tokens):
    """Rounding off and fp32 noise: id for id oracle.nar_oracle.sample_gumbel on the fp32 values of the draw inputs, where the
    oracle has nothing to round.  Rounding on: id for id the oracle on the 16-bit logits themselves, which rounds logit / T as the
    reference does."""
    T, seed, level = NM.DRAW_TEMPERATURE, NM.DRAW_SEEDS[0], 2
    grid = NM.draw_inputs(n_tokens, dtype, special=False)
    rows = [NM.draw_rows(grid, b, n_tokens) for b in range(3)]
    for greedy in (False, True):
        plain = N.sample_gumbel([r.float() for r in rows], T, seed, level, utt0=4, greedy=greedy)
        model = N.sample_gumbel(rows, T, seed, level, utt0=4, greedy=greedy)
        for b, r in enumerate(rows):
            ids, _ = NM.draw_mirror(r, T, greedy=greedy, seed=seed, level=level, utt=4 + b, rounded=False, fp32_noise=True)
            assert np.array_equal(ids, plain[b].numpy()), (greedy, b)
            ids, _ = NM.draw_mirror(r, T, greedy=greedy, seed=seed, level=level, utt=4 + b, rounded=True, fp32_noise=True)
            assert np.array_equal(ids, model[b].numpy()), (greedy, b)


def test_greedy_inputs_see_the_rounding_and_the_tie_rule():
    """bf16: on at least 50 rows the rounded rule and argmax(logit / T) name different classes; and the special rows are there."""
    n_tokens = 1024
    grid = NM.draw_inputs(n_tokens, torch.bfloat16)
    flips = 0
    for b in range(3):
        r = NM.draw_rows(grid, b, n_tokens)
        a, _ = NM.draw_mirror(r, NM.DRAW_TEMPERATURE, greedy=True)
        c, _ = NM.draw_mirror(r, NM.DRAW_TEMPERATURE, greedy=True, rounded=False)
        flips += int((a != c).sum())
    assert flips >= 50, flips
    for n in (1024, 1023, 6):
        r = NM.draw_rows(NM.draw_inputs(n, torch.float16), 0, n)
        ids, _ = NM.draw_mirror(r, NM.DRAW_TEMPERATURE, greedy=True)
        hi, lo = (700, 3) if n > 700 else (n - 1, 1)
        assert r[2, hi] == r[2, lo] == r[2].max() and ids[2] == lo and lo // 4 % 64 != hi // 4 % 64      # two lanes, the first index wins
        assert (r[5] == r[5, 0]).all() and ids[5] == 0                                                  # constant row
        assert math.isinf(float(r[6, 0])) and ids[6] % 3 != 0                                           # -inf classes
        assert (r[17] == -math.inf).all() and ids[17] == 0                                              # -inf throughout


@pytest.mark.parametrize("n_tokens", [1024, 1023, 6])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_gumbel_margins_of_the_draw_inputs_need_no_excuse(dtype, n_tokens):
    """No row of the draw inputs has its two best values within 64 fp32 steps of each other: the float64 mirror and an fp32 kernel
    (two logf and one add: 8 steps at the most) must name the same class on every row."""
    grid = NM.draw_inputs(n_tokens, dtype, special=False)
    for seed, level in NM.DRAW_RUNS:
        for b in range(3):
            ulps = NM.margin_ulps(NM.draw_rows(grid, b, n_tokens), NM.DRAW_TEMPERATURE, seed=seed, level=level, utt=b)
            assert ulps.min() > 64, (seed, level, b, ulps.min())

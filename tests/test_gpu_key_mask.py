"""Key-padding masks end to end (include/d3pm_hip.h: d3pm_keys; AR.generate_audio(mask_padding=True)).
  1. the feature exists: generate_audio(mask_padding=True) runs and returns [B, canvas];
  2. neutral: with every length full the masked call gives the ids of the unmasked one, bit for bit;
  3. reference: the live rows of a masked evaluation are what the unchanged oracle (fp32) / a HIP model (bf16, d = 512) computes at
     the truncated shape canvas = L_b, s_text = text[b], s_prompt = prompt[b];
  4. under D3PM_FLAG_FORCE_GENERIC in fp32 that equality is bit for bit (the walk over the keys is the same);
  5. independence: utterance b of a ragged masked batch = that utterance alone; stream chunks and the reveal loop reproduce the
     unsplit call; garbage ids behind text[b] / prompt[b] change no id."""
import dataclasses

import pytest
import torch

from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(cfg, dtype, sd=None):
    from vall_e.vall_e import AR, synth
    m = AR.from_config(cfg)
    m.load_state_dict(sd if sd is not None else synth.make_state_dict(cfg, 0))
    return m.to(dtype).to(DEV)


def _lengths(B, canvas):
    """1, the whole canvas, and values that are no multiples of 16, 32 or 128 (the pool of tests/test_gpu_canvas.py)."""
    pool = [1, canvas, 37, canvas - 1, 333, 129, 15, 250, 97, 401, 7, 211]
    return [min(pool[i % len(pool)] + 2 * (i // len(pool)), canvas) for i in range(B)]


@pytest.fixture(scope="module")
def native():
    from vall_e.vall_e import synth
    cfg = synth.D3PMConfig.native()
    sd = synth.make_state_dict(cfg, 0)
    texts, proms = synth.make_inputs(cfg, 8, 1)
    models = {}

    def get(dtype):
        if dtype not in models:
            models[dtype] = _model(cfg, dtype, sd)
        return models[dtype]
    return cfg, sd, texts, proms, get


@pytest.fixture(scope="module")
def libri():
    from vall_e.vall_e import synth
    cfg = synth.D3PMConfig.libritts()
    sd = synth.make_state_dict(cfg, 0)
    texts, proms = synth.make_inputs(cfg, 12, 1)
    return cfg, sd, texts, proms, _model(cfg, torch.bfloat16, sd)


def _full_inputs(cfg, B, seed=5):
    g = torch.Generator().manual_seed(seed)
    return ([torch.randint(1, 1024, (cfg.s_text,), generator=g) for _ in range(B)],
            [torch.randint(0, 1024, (cfg.s_prompt, cfg.n_levels), generator=g) for _ in range(B)])


def test_mask_padding_runs_and_full_lengths_are_neutral_native(native):
    """native fp16, B = 2, the whole reverse process (99 evaluations)"""
    cfg, _, texts, proms, get = native
    m = get(torch.float16)
    out = m.generate_audio(texts[:2], proms[:2], seed=3, steps=2, n_frames=[37, 300], mask_padding=True)
    assert out.shape == (2, cfg.canvas) and out.dtype == torch.int64
    ft, fp = _full_inputs(cfg, 2)
    a = m.generate_audio(ft, fp, seed=7, n_frames=cfg.canvas, mask_padding=True)
    b = m.generate_audio(ft, fp, seed=7, n_frames=cfg.canvas)
    assert torch.equal(a, b)


@pytest.mark.parametrize("B", [4, 12])
def test_full_lengths_are_neutral_libritts(libri, B):
    cfg, _, _, _, m = libri
    ft, fp = _full_inputs(cfg, B)
    a = m.generate_audio(ft, fp, seed=7, steps=4, n_frames=cfg.canvas, mask_padding=True)
    b = m.generate_audio(ft, fp, seed=7, steps=4, n_frames=cfg.canvas)
    assert a.shape == (B, cfg.canvas) and torch.equal(a, b)


def _half_masked(L, canvas, seed):
    from vall_e.vall_e.ar_discrete import MASK_ID
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(canvas, dtype=torch.int64)
    ids = torch.randint(0, 1024, (L,), generator=g)
    x[:L] = torch.where(torch.rand(L, generator=g) < 0.5, torch.full((L,), MASK_ID), ids)
    return x


def _masked_eval(m, cfg, texts, proms, lens, x, t, flags=0, tuning=None):
    """One masked evaluation of the padded batch through the Sampler -> (cond_text, cond_prompt, logits), the key counts"""
    from vall_e.vall_e import _hip
    B = len(texts)
    f, tl, pl = m.key_lengths(texts, proms, lens)
    keys = tuple(torch.tensor(v, dtype=torch.int32, device=DEV) for v in (f, tl, pl))
    smp = m.sampler()
    with _hip.tuning(**(tuning or {})):
        ct, cp = m.encode_conditions(texts, proms, keys[1], keys[2])
        kv_t, kv_p = smp.cond_kv(ct, cp)
        fm = torch.zeros(B, cfg.canvas, dtype=torch.uint8, device=DEV)
        for b, L in enumerate(f):
            fm[b, :L] = 1
        lg, _ = smp.denoise_canvas(x.to(torch.int32).to(DEV).contiguous(), fm, t, kv_t, kv_p, flags=flags, keys=keys)
    return ct, cp, lg, (f, tl, pl)


CASES = [(37, 20, 100), (349, 50, 398)]


def test_live_rows_match_the_oracle_at_the_truncated_shape_fp32(native):
    """fp32 native shape, one evaluation at t = 40 on a half-masked x_t: live-row logits within 1e-3 of the oracle built at
    Shape(canvas = L, n_frames = L, s_text = text, s_prompt = prompt) -- the bound tests/test_gpu_parity.py gives the same
    comparison at the full shape -- and the condition encoders' live rows within its ctol (1e-3 in fp32)."""
    from oracle import d3pm_oracle as O
    cfg, sd, _, _, get = native
    m = get(torch.float32)
    g = torch.Generator().manual_seed(9)
    texts = [torch.randint(1, 1024, (tl,), generator=g) for _, tl, _ in CASES]
    proms = [torch.randint(0, 1024, (pl, cfg.n_levels), generator=g) for _, _, pl in CASES]
    lens = [L for L, _, _ in CASES]
    x = torch.stack([_half_masked(L, cfg.canvas, 40 + L) for L in lens])
    ct, cp, lg, _ = _masked_eval(m, cfg, texts, proms, lens, x, 40)
    for b, (L, tl, pl) in enumerate(CASES):
        shape = dataclasses.replace(O.Shape.of(cfg), canvas=L, n_frames=L, s_text=tl, s_prompt=pl)
        orc = O.Oracle({k: v.to(torch.float32) for k, v in sd.items()}, shape)
        with torch.no_grad():
            rcp, rct = orc.conditions(texts[b], proms[b])
            ref = orc.logits(x[b, :L], 40, rcp, rct, torch.ones(L, dtype=torch.bool))
        et = (ct[b, :tl].cpu() - rct).abs().max().item()
        ep = (cp[b, :pl].cpu() - rcp).abs().max().item()
        err = (lg[b, :L].cpu() - ref).abs().max().item()
        print(f"[key_mask] fp32 case {CASES[b]}: cond_text {et:.2e} cond_prompt {ep:.2e} logits {err:.2e}")
        REPORT.setdefault("key_mask_fp32_vs_oracle", {})[str(CASES[b])] = {"cond_text": et, "cond_prompt": ep, "logits": err}
        assert et < 1e-3 and ep < 1e-3 and err < 1e-3


def test_generic_fp32_equals_the_truncated_model_bit_for_bit(native):
    from vall_e.vall_e import _hip, synth
    cfg, sd, _, _, get = native
    m = get(torch.float32)
    g = torch.Generator().manual_seed(9)
    texts = [torch.randint(1, 1024, (tl,), generator=g) for _, tl, _ in CASES]
    proms = [torch.randint(0, 1024, (pl, cfg.n_levels), generator=g) for _, _, pl in CASES]
    lens = [L for L, _, _ in CASES]
    x = torch.stack([_half_masked(L, cfg.canvas, 40 + L) for L in lens])
    _, _, lg, _ = _masked_eval(m, cfg, texts, proms, lens, x, 40, flags=_hip.FLAG_FORCE_GENERIC)
    for b, (L, tl, pl) in enumerate(CASES):
        small_cfg = dataclasses.replace(cfg, canvas=L, n_frames=L, s_text=tl, s_prompt=pl)
        small = _model(small_cfg, torch.float32, sd)
        smp = small.sampler()
        ct, cp = small.encode_conditions([texts[b]], [proms[b]])
        kv_t, kv_p = smp.cond_kv(ct, cp)
        ref, _ = smp.denoise(x[b:b + 1, :L].to(torch.int32).to(DEV).contiguous(), torch.ones(L, dtype=torch.uint8, device=DEV), 40, kv_t, kv_p,
                             flags=_hip.FLAG_FORCE_GENERIC)
        assert torch.equal(lg[b, :L], ref[0]), f"case {CASES[b]}: max diff {(lg[b, :L] - ref[0]).abs().max().item():.3e}"


def test_live_rows_match_a_truncated_hip_model_bf16_d512(libri):
    """d = 512 bf16, B = 12 (the 32 x 32 x 16 self-attention and the resident pair), lengths from _lengths: the live-row logits of the
    masked padded evaluation against a HIP model built at the truncated config.  The bound is not fixed in advance: it is twice
    what two unmasked schedules of the same evaluation (attn_query_groups 1 against 32) differ by at this shape -- accumulation
    order only; the factor covers the second instruction-shape change (the pair).  Both numbers are printed and reported.
    Every utterance of the batch is compared: one truncated model each."""
    from vall_e.vall_e import _hip
    cfg, sd, texts, proms, m = libri
    B = 12
    lens = _lengths(B, cfg.canvas)
    x = torch.stack([_half_masked(L, cfg.canvas, 40 + L) for L in lens])
    # the yardstick: the same unmasked evaluation on two schedules
    smp = m.sampler()
    fm = torch.zeros(cfg.canvas, dtype=torch.uint8, device=DEV)
    fm[:cfg.n_frames] = 1
    xf = torch.stack([_half_masked(cfg.n_frames, cfg.canvas, 7 + b) for b in range(B)]).to(torch.int32).to(DEV)
    ct, cp = m.encode_conditions(texts, proms)
    kv_t, kv_p = smp.cond_kv(ct, cp)
    sched = []
    for g in (1, 32):
        with _hip.tuning(attn_query_groups=g):
            sched.append(smp.denoise(xf, fm, 40, kv_t, kv_p)[0].float())
    yard = (sched[0][:, :cfg.n_frames] - sched[1][:, :cfg.n_frames]).abs().max().item()
    _, _, lg, (f, tl, pl) = _masked_eval(m, cfg, texts, proms, lens, x, 40)
    worst = 0.0
    for b in range(B):
        L = f[b]
        small_cfg = dataclasses.replace(cfg, canvas=L, n_frames=L, s_text=tl[b], s_prompt=pl[b])
        small = _model(small_cfg, torch.bfloat16, sd)
        ssm = small.sampler()
        sct, scp = small.encode_conditions([texts[b]], [proms[b]])
        skv_t, skv_p = ssm.cond_kv(sct, scp)
        ref, _ = ssm.denoise(x[b:b + 1, :L].to(torch.int32).to(DEV).contiguous(), torch.ones(L, dtype=torch.uint8, device=DEV), 40, skv_t, skv_p)
        worst = max(worst, (lg[b, :L].float() - ref[0].float()).abs().max().item())
        del small, ssm
    print(f"[key_mask] bf16 d512: masked vs truncated model {worst:.4e}; unmasked attn_query_groups 1 vs 32 {yard:.4e}; bound {2 * yard:.4e}")
    REPORT["key_mask_bf16_d512"] = {"masked_vs_truncated": worst, "schedules_1_vs_32": yard, "bound": 2 * yard}
    assert worst <= 2 * yard


def _ragged(cfg, texts, proms, B):
    return texts[:B], proms[:B], _lengths(B, cfg.canvas)


@pytest.mark.parametrize("B", [4, 12])
def test_an_utterance_of_a_ragged_batch_is_that_utterance_alone(libri, B):
    cfg, _, texts, proms, m = libri
    tx, pr, lens = _ragged(cfg, texts, proms, B)
    out = m.generate_audio(tx, pr, seed=11, steps=3, n_frames=lens, mask_padding=True, utt0=5)
    plain = m.generate_audio(tx, pr, seed=11, steps=3, n_frames=lens, utt0=5)
    assert not torch.equal(out, plain)          # the mask does something
    for b in range(B):
        alone = m.generate_audio([tx[b]], [pr[b]], seed=11, steps=3, n_frames=[lens[b]], mask_padding=True, utt0=5 + b, global_batch=B)
        assert torch.equal(out[b], alone), f"utterance {b} of {B}"


def test_stream_chunks_and_the_reveal_loop_reproduce_the_unsplit_call(libri):
    cfg, _, texts, proms, m = libri
    tx, pr, lens = _ragged(cfg, texts, proms, 4)
    one = m.generate_audio(tx, pr, seed=13, steps=3, n_frames=lens, mask_padding=True)
    two = m.generate_audio(tx, pr, seed=13, steps=3, n_frames=lens, mask_padding=True, streams=2)
    assert torch.equal(one, two)
    r1 = m.generate_audio(tx, pr, seed=13, reveal_steps=4, n_frames=lens, mask_padding=True)
    r2 = m.generate_audio(tx, pr, seed=13, reveal_steps=4, n_frames=lens, mask_padding=True, streams=2)
    assert torch.equal(r1, r2)
    for b in (0, 2):
        alone = m.generate_audio([tx[b]], [pr[b]], seed=13, reveal_steps=4, n_frames=[lens[b]], mask_padding=True, utt0=b, global_batch=4)
        assert torch.equal(r1[b], alone)


def test_garbage_ids_behind_the_lengths_change_no_id(libri):
    """Sampler level: the padded text / prompt tensors carry other ids behind text[b] / prompt[b], and the tensors reach
    d3pm_encode_conditions_keys as they are (the library does not read an id behind a length; the wrapper changes none).  The
    encoders' outputs are equal bit for bit in every row, and so is every id of the loop."""
    cfg, _, texts, proms, m = libri
    B = 4
    tx, pr, lens = _ragged(cfg, texts, proms, B)
    f, tl, pl = m.key_lengths(tx, pr, lens)
    assert any(v < cfg.s_text for v in tl) and any(v < cfg.s_prompt for v in pl)      # there are rows behind the lengths
    keys = tuple(torch.tensor(v, dtype=torch.int32, device=DEV) for v in (f, tl, pl))
    smp = m.sampler()
    text, prom = m._padded_inputs(tx, pr)
    outs, conds = [], []
    for garbage in (None, (777, 555), (-1, -1), (3, 1023)):
        t2, p2 = text.clone(), prom.clone()
        if garbage:
            for b in range(B):
                t2[b, tl[b]:] = garbage[0]
                p2[b, pl[b]:] = garbage[1]
            assert not (torch.equal(t2, text) and torch.equal(p2, prom))
        ct, cp = smp.encode_conditions(t2, p2, keys[1], keys[2])
        conds.append((ct.clone(), cp.clone()))
        kv_t, kv_p = smp.cond_kv(ct, cp)
        x, fm, _ = m.canvas_init_known(B, lens)
        smp.sample_loop(x, fm, 3, 0, kv_t, kv_p, 17, keys=keys)
        outs.append(x.clone())
    for (ct, cp), x in zip(conds[1:], outs[1:]):
        assert torch.equal(ct, conds[0][0]) and torch.equal(cp, conds[0][1])
        assert torch.equal(x, outs[0])
    # without the lengths the same garbage does reach the encoders: the comparison above is not vacuous
    t2, p2 = text.clone(), prom.clone()
    for b in range(B):
        t2[b, tl[b]:] = 777
        p2[b, pl[b]:] = 555
    ct_u, cp_u = smp.encode_conditions(text, prom)
    ct_g, cp_g = smp.encode_conditions(t2, p2)
    assert not torch.equal(ct_u, ct_g) and not torch.equal(cp_u, cp_g)

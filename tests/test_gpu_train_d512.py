"""The whole training step at the product's LibriTTS shape (synth.D3PMConfig.libritts(): d = 512, 8 denoiser heads of width 64,
16 encoder heads of width 32, 6 blocks, a 768-row canvas, 50 text and 225 prompt keys), fp32, against torch.autograd over the
CPU oracle (oracle/d3pm_oracle.py:training_forward) in float64.  Two utterances: one with 750 response frames, one with 500, so a
third of its canvas is padding and the frame mask does work.  tests/test_gpu_train.py and tests/test_gpu_train_dropout.py check
the same step at the upstream-native shape (heads of width 2); tests/test_gpu_train_kernels.py checks its kernels one by one."""
import time

import pytest
import torch

from dropout_mirror import mirror_encoder
from oracle import d3pm_oracle as O
from oracle import philox
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, T = 20261016, 3            # t = 1, 2
N_FRAMES = (750, 500)


def _setup():
    from vall_e.vall_e import synth
    cfg = synth.D3PMConfig.libritts()
    sd32 = synth.make_state_dict(cfg, 0)
    texts, proms = synth.make_inputs(cfg, 2, 1)
    gen = torch.Generator().manual_seed(5)
    resps = [torch.randint(1, cfg.n_classes - 1, (n,), generator=gen) for n in N_FRAMES]
    return cfg, sd32, texts, proms, resps


def _fp32_pe(orig):
    """O.sinusoid_pe follows the state-dict dtype; the fp32 model evaluates its angles and sines in fp32 (ar_discrete.py
    _sinusoid_table).  The float64 tables differ from those by ~1e-5 at 225 positions, so the reference takes the fp32 tables,
    widened: both sides then compute the same function and the comparison checks the kernels, not two definitions."""
    return lambda n, d, dtype: orig(n, d, torch.float32).to(dtype)


def _oracle(monkeypatch, cfg, sd32, texts, proms, resps, dropout):
    """(loss, grads): autograd over the mean of the two utterances' training_forward in float64.  Utterance b draws its
    q_sample noise with utterance index b (the trainer keys it utt0 + b, utt0 = 0) and, with dropout, its masks likewise."""
    from vall_e.vall_e.train import DROPOUT_TRAIN
    monkeypatch.setattr(O, "sinusoid_pe", _fp32_pe(O.sinusoid_pe))
    shape = O.Shape.of(cfg)
    sd = {k: v.double().requires_grad_(True) for k, v in sd32.items()}
    total = 0.0
    for b in range(2):
        if dropout:
            monkeypatch.setattr(O, "cond_encoder", mirror_encoder(SEED, b, *DROPOUT_TRAIN))

        def q_noise(t, b=b):
            return torch.from_numpy(philox.uniform_batch(SEED, t, b, 1, cfg.canvas, stream=philox.STREAM_Q_SAMPLE))[0]

        loss, _ = O.training_forward(sd, shape, texts[b], proms[b], resps[b], q_noise, timesteps=T)
        total = total + loss / 2
    total.backward()
    return float(total.detach()), {k: v.grad for k, v in sd.items() if v.grad is not None}


def _check(tag, cfg, sd32, texts, proms, resps, ref_loss, ref, dropout):
    from vall_e.vall_e import AR
    from vall_e.vall_e.train import D3PMTrainer
    m = AR.from_config(cfg)
    m.load_state_dict(sd32)
    m = m.float().to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, dconds = D3PMTrainer(m).forward_backward(texts, proms, resps, seed=SEED, timesteps=T, dropout=dropout)
    torch.cuda.synchronize()
    step_s = time.perf_counter() - t0
    assert abs(float(loss) - ref_loss) <= 1e-4 * abs(ref_loss), (float(loss), ref_loss)
    worst, checked = {}, 0
    for name, p in m.named_parameters():
        if ".cross_attn2." in name or name.startswith("token_emb"):
            assert p.grad is None, name                         # dead upstream parameters stay gradient-free
            continue
        want = ref.get(name)
        if want is None:                                        # a parameter the forward never reads (none expected here)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, f"no gradient for {name}"
        if name in ("text_emb.weight", "resps_emb.weight"):     # nn.Embedding(padding_idx=0) upstream: row 0 gets no gradient
            want = want.clone()
            want[0] = 0
        err = (p.grad.cpu().double() - want).abs().max().item()
        scale = want.abs().max().item()
        worst[name] = err / max(scale, 1e-8)
        checked += 1
        assert err <= 2e-4 * scale + 1e-7, f"{name}: max |grad error| {err:.3e} vs gradient scale {scale:.3e}"
    # every live parameter is checked: 194 at this shape (6 blocks; the >= 230 of the native-shape tests counts 8)
    live = [n for n, _ in m.named_parameters() if ".cross_attn2." not in n and not n.startswith("token_emb")]
    assert checked == len(live) >= 194, (checked, len(live))
    assert len(dconds) == 2 and dconds[1][1].shape == (cfg.s_prompt, cfg.d_model)
    REPORT[tag] = {"loss_hip": float(loss), "loss_autograd": ref_loss, "tensors_checked": checked,
                   "worst_relative_error": max(worst.values()), "worst_tensor": max(worst, key=worst.get),
                   "hip_step_seconds": step_s}


@pytest.mark.parametrize("dropout", [False, True], ids=["eval", "train"])
def test_d512_gradients_match_autograd_over_the_oracle(monkeypatch, dropout):
    cfg, sd32, texts, proms, resps = _setup()
    t0 = time.perf_counter()
    ref_loss, ref = _oracle(monkeypatch, cfg, sd32, texts, proms, resps, dropout)
    oracle_s = time.perf_counter() - t0
    tag = f"train_gradcheck_libritts_f32{'_dropout' if dropout else ''}"
    _check(tag, cfg, sd32, texts, proms, resps, ref_loss, ref, dropout)
    REPORT[tag]["oracle_seconds"] = oracle_s

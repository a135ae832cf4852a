"""The train step with a DecayLoss on the device: Trainer.step(..., wav_true=) is the step done by hand with the same kernels (forward with
the target, the wave-loss call with the fused spectrogram term and the waveform, the decay loss on that waveform, its
vector-Jacobian product added to dpred, backward from dpred) bit for bit; that dpred is the references' within the kernels' bounds;
and the step replayed as a HIP graph is the step issued launch by launch.  The smallest U-Net of tests/test_wave_loss_step_gpu.py:
32 x 48 planes, batch 2, n_fft 32 (17 bins), window 16, hop 8, 41 frames: T = 320."""
import numpy as np
import pytest
import torch

import decay_loss_ref as DR
import wave_loss_ref as WR
from test_wave_loss_step_gpu import B, DEV, GEO, H, T, W, _engine

pytestmark = pytest.mark.gpu
WEIGHT, FLOOR = 0.02, 40.0
GEO_REF = (GEO["des_shape"], GEO["n_fft"], GEO["win_length"], GEO["hop_length"])


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def _batches(n):
    """the batches of the wave-loss step test with decaying targets: noise under an exponential envelope, 60 dB down at 0.6 T"""
    gen = torch.Generator(); gen.manual_seed(5)
    envelope = torch.exp(-torch.arange(T, dtype=torch.float32) / (0.6 * T / (3.0 * np.log(10.0))))
    out = []
    for _ in range(n):
        out.append((torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
                    torch.rand((B, 2, H, W), generator=gen).to(DEV), (torch.randn((B, T), generator=gen) * 0.5 * envelope).to(DEV)))
    return out


def _decay(U, weight=WEIGHT):
    return U.DecayLoss(weight=weight, floor_db=FLOOR, **GEO)


def _wave(U):
    return U.WaveLoss(weight=0.25, norm="energy", time_weight=torch.linspace(1.0, 0.1, T), **GEO)


def _by_hand(U, eng, a, e, b, wav, wave):
    """forward(target), ops.wave_loss (the user's, or weight 0), ops.decay_loss, ops.istft_features_bwd(accumulate), backward(dpred) on
    `eng`; returns (dpred after the wave loss, dpred, wav_pred, dwav, decay_out, loss_out[0] before the decay term)"""
    eng.training = True
    eng.loss_diff = False
    eng.forward(a, e, target=b, global_batch=B, alpha=0.9)
    dp = torch.full_like(eng.pred, float("nan"))
    wv = torch.full((B, T), float("nan"), device=DEV)
    wo = torch.zeros(2, dtype=torch.float64, device=DEV)
    kw = dict(norm="energy", weight=0.25, time_weight=wave.time_weight) if wave is not None else dict(norm="mse", weight=0.0)
    U.ops.wave_loss(eng.pred, wav, wo, U.ops.Workspace(DEV), *GEO["des_shape"], GEO["n_fft"], GEO["win_length"], GEO["hop_length"],
                    global_batch=B, spec_target=b, alpha=0.9, inv_norm=1.0 / (2.0 * H * W * B), dpred=dp, wav_pred=wv,
                    loss_out=eng.loss_out, **kw)
    dp0, loss0 = dp.clone(), float(eng.loss_out[0])
    dw = torch.full((B, T), float("nan"), device=DEV)
    do = torch.zeros(2, dtype=torch.float64, device=DEV)
    U.ops.decay_loss(wv, wav, do, U.ops.Workspace(DEV), floor_db=FLOOR, weight=WEIGHT, global_batch=B, dwav=dw, loss_out=eng.loss_out)
    U.ops.istft_features_bwd(eng.pred, dw, dp, *GEO["des_shape"], GEO["n_fft"], GEO["win_length"], GEO["hop_length"], accumulate=True)
    eng.backward(dpred=dp)
    return dp0, dp, wv, dw, do, loss0


@pytest.mark.parametrize("user_wave", [False, True], ids=["decay-alone", "with-wave-loss"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_step_is_the_step_done_by_hand_and_the_references_dpred(U, dtype, user_wave):
    (a, e, b, wav), = _batches(1)
    eng = _engine(U, "unet", dtype)
    wl, dl = (_wave(U) if user_wave else None), _decay(U)
    tr = U.Trainer(eng, lr=1e-3, dropout=False, wave_loss=wl, decay_loss=dl)
    theta0 = eng.theta.clone()
    tr.step(a, e, b, wav_true=wav)
    hand = _engine(U, "unet", dtype)
    dp0, dp, wv, dw, do, loss0 = _by_hand(U, hand, a, e, b, wav, wl)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dp).all()) and bool(torch.isfinite(eng.grad).all())
    assert torch.equal(eng.grad.view(torch.int32), hand.grad.view(torch.int32))
    assert torch.equal(eng.loss_out, hand.loss_out) and torch.equal(dl.decay_out, do) and float(do[0]) > 0 and float(do[1]) == B
    assert not torch.equal(eng.theta, theta0)
    # the references' dpred: the decay term of the waveform the step reconstructed, carried to the prediction, on top of the wave
    # loss's dpred - each kernel within its own bound, the cotangent's one rounding to fp32 passed on by the linear map
    cf = DR.closed_form(wv.cpu().numpy(), wav.cpu().numpy(), FLOOR, weight=WEIGHT, global_batch=B)
    err_w, tol_w = np.abs(dw.cpu().numpy().astype(np.float64) - cf["dwav"]), DR.bound(cf["dwav"], cf["abs"], cf["n_terms"])
    assert (err_w <= tol_w).all() and np.abs(cf["dwav"]).max() > 0
    vj = DR.vjp_closed_form(hand.pred.cpu().numpy(), dw.cpu().numpy(), *GEO_REF)
    base = dp0.cpu().numpy()
    err = np.abs(dp.cpu().numpy().astype(np.float64) - (base.astype(np.float64) + vj["grad"]))
    assert (err <= DR.bound_accumulated(base, vj["grad"], vj["abs"], vj["n_terms"])).all() and np.abs(vj["grad"]).max() > 0
    # loss_out[0] has grown by the term: one fp32 addition of the rounded term
    assert abs(float(do[0]) - cf["decay_out"][0]) <= cf["decay_out_tol"][0]
    term = np.float32(WEIGHT / B * float(do[0]))
    assert float(hand.loss_out[0]) == float(np.float32(np.float32(loss0) + term)) and term > 0
    # the term is in the gradient: the step without it differs
    plain = _engine(U, "unet", dtype)
    ptr = U.Trainer(plain, lr=1e-3, dropout=False, wave_loss=_wave(U) if user_wave else None)
    ptr.step(a, e, b, wav_true=wav if user_wave else None)
    torch.cuda.synchronize()
    assert not torch.equal(plain.grad, eng.grad) and float(eng.loss_out[0]) > float(plain.loss_out[0])
    with pytest.raises(ValueError, match="wav_true"):
        tr.step(a, e, b)


@pytest.mark.parametrize("user_wave", [False, True], ids=["decay-alone", "with-wave-loss"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_weight_zero_leaves_the_steps_gradients_alone(U, dtype, user_wave):
    """weight = 0: dwav is an exact zero and the accumulating pass adds exact zeros, so the gradients, the loss and the updated
    parameters are those of the trainer without the option, bit for bit.  With a decay_loss alone that trainer is the one with the
    WaveLoss of weight 0 the option brings along, given by hand (that one against the plain trainer - the loss kernel's dL/dlogits
    against the wave-loss kernel's dL/dpred - is tests/test_wave_loss_sim.py's test_weight_zero_is_the_plain_trainer)."""
    (a, e, b, wav), = _batches(1)
    wave = (lambda: _wave(U)) if user_wave else (lambda: U.WaveLoss(weight=0.0, **GEO))
    with_eng, without_eng = _engine(U, "unet", dtype), _engine(U, "unet", dtype)
    tr = U.Trainer(with_eng, lr=1e-3, dropout=False, wave_loss=wave() if user_wave else None, decay_loss=_decay(U, 0.0))
    tr.step(a, e, b, wav_true=wav)
    U.Trainer(without_eng, lr=1e-3, dropout=False, wave_loss=wave()).step(a, e, b, wav_true=wav)
    torch.cuda.synchronize()
    assert torch.equal(with_eng.loss_out, without_eng.loss_out) and float(tr.decay_loss.decay_out[0]) > 0
    assert torch.equal(with_eng.grad.view(torch.int32), without_eng.grad.view(torch.int32))
    assert torch.equal(with_eng.theta.view(torch.int32), without_eng.theta.view(torch.int32))


@pytest.mark.parametrize("user_wave", [False, True], ids=["decay-alone", "with-wave-loss"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_three_graph_steps_equal_three_eager_steps(U, dtype, user_wave):
    data = _batches(3)
    res = []
    for graph in (True, False):
        eng = _engine(U, "unet", dtype)
        tr = U.Trainer(eng, lr=1e-3, graph=graph, wave_loss=_wave(U) if user_wave else None, decay_loss=_decay(U))
        if not graph:
            eng.use_device_counters(True)          # the same arithmetic by construction: the step's scalars in device memory for both
        losses = [tr.step(a, e, b, wav_true=wav, return_loss=True) for a, e, b, wav in data]
        torch.cuda.synchronize()
        if graph:
            assert tr.use_graph and set(tr._graphs) == {True} and len(tr._g_in) == 4
        res.append((losses, eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), tr.decay_loss.decay_out.clone(), eng.adam_t))
    g, h = res
    assert g[0] == h[0] and g[5] == h[5] == 3
    for i in (1, 2, 3, 4):
        assert torch.equal(g[i], h[i]), i
    assert float(g[4][0]) > 0


def test_train_script_with_the_decay_loss(U, tmp_path, monkeypatch):
    """scripts/train.py --decay-loss on the generated tree: the data set keeps the waveforms, fit records the term for the training and
    the validation pass; without a data set it refuses"""
    import json
    import os
    import dataset_tree as DT
    from test_dataset_gpu import run_script
    root = str(tmp_path / "rir")
    os.makedirs(root)
    DT.make_tree(root)
    out = str(tmp_path / "ckpt")
    common = ["--rooms", "HemiAnechoicRoom", "SmallMeetingRoom", "--no-debug", "--batch", 4, "--lr", 1e-4, "--out", out, "--epochs", 1,
              "--decay-loss", 0.01, "--decay-floor-db", 45]
    run_script(monkeypatch, "train", ["--dataset", root, DT.NAME, "--name", "unet", "--filters", 8] + common)
    hist = json.load(open(os.path.join(out, "history.json")))
    assert [h["epoch"] for h in hist] == [1]
    for h in hist:
        assert all(np.isfinite(h[k]) and h[k] > 0 for k in ("train_loss", "val_loss", "train_decay", "val_decay"))
        assert "train_wave" not in h
    with pytest.raises(SystemExit, match="--dataset"):
        run_script(monkeypatch, "train", ["--synthetic", 2, "--name", "unet", "--filters", 8] + common)

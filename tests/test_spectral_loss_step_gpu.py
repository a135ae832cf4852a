"""The train step with a SpectralLoss on the device: Trainer.step(..., wav_true=) is the step done by hand with the same kernels (forward
with the target, the wave-loss call with the fused spectrogram term and the waveform, the spectral loss on that waveform, its
vector-Jacobian product added to dpred, backward from dpred) bit for bit; that dpred is the references' within the kernels' bounds; with
a DecayLoss as well ONE vector-Jacobian product carries both cotangents; the step replayed as a HIP graph is the step issued launch by
launch; and a trainer without the term is the step it was.  The smallest U-Net of tests/test_wave_loss_step_gpu.py: 32 x 48 planes,
batch 2, n_fft 32 (17 bins), window 16, hop 8, 41 frames: T = 320, looked at through (64, 32, 16) and (128, 128, 32)."""
import numpy as np
import pytest
import torch

import decay_loss_ref as DR
import spectral_loss_ref as SR
from test_decay_loss_step_gpu import FLOOR as D_FLOOR, WEIGHT as D_WEIGHT, _batches, _by_hand as _decay_by_hand, _decay, _wave
from test_wave_loss_step_gpu import B, DEV, GEO, H, T, W, _engine

pytestmark = pytest.mark.gpu
WEIGHT, FLOOR, SCW, LW = 0.05, 40.0, 0.8, 1.3
RES = ((64, 32, 16), (128, 128, 32))
GEO_REF = (GEO["des_shape"], GEO["n_fft"], GEO["win_length"], GEO["hop_length"])
GEO_OP = (*GEO["des_shape"], GEO["n_fft"], GEO["win_length"], GEO["hop_length"])


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def _spectral(U, weight=WEIGHT):
    return U.SpectralLoss(weight=weight, resolutions=RES, sc_weight=SCW, log_weight=LW, floor_db=FLOOR, **GEO)


def _front(U, eng, a, e, b, wav, wave):
    """forward(target) and ops.wave_loss (the user's, or weight 0) on `eng` -> (dpred, wav_pred)"""
    eng.training = True
    eng.loss_diff = False
    eng.forward(a, e, target=b, global_batch=B, alpha=0.9)
    dp = torch.full_like(eng.pred, float("nan"))
    wv = torch.full((B, T), float("nan"), device=DEV)
    wo = torch.zeros(2, dtype=torch.float64, device=DEV)
    kw = dict(norm="energy", weight=0.25, time_weight=wave.time_weight) if wave is not None else dict(norm="mse", weight=0.0)
    U.ops.wave_loss(eng.pred, wav, wo, U.ops.Workspace(DEV), *GEO_OP, global_batch=B, spec_target=b, alpha=0.9,
                    inv_norm=1.0 / (2.0 * H * W * B), dpred=dp, wav_pred=wv, loss_out=eng.loss_out, **kw)
    return dp, wv


def _spectral_op(U, wv, wav, dw, accumulate, loss_out):
    so = torch.zeros(3, dtype=torch.float64, device=DEV)
    U.ops.spectral_loss(wv, wav, so, U.ops.Workspace(DEV), RES, floor_db=FLOOR, sc_weight=SCW, log_weight=LW, weight=WEIGHT, global_batch=B,
                        dwav=dw, accumulate=accumulate, loss_out=loss_out)
    return so


@pytest.mark.parametrize("user_wave", [False, True], ids=["spectral-alone", "with-wave-loss"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_step_is_the_step_done_by_hand_and_the_references_dpred(U, dtype, user_wave):
    (a, e, b, wav), = _batches(1)
    eng = _engine(U, "unet", dtype)
    wl, sl = (_wave(U) if user_wave else None), _spectral(U)
    tr = U.Trainer(eng, lr=1e-3, dropout=False, wave_loss=wl, spectral_loss=sl)
    theta0 = eng.theta.clone()
    tr.step(a, e, b, wav_true=wav)
    hand = _engine(U, "unet", dtype)
    dp, wv = _front(U, hand, a, e, b, wav, wl)
    dp0, loss0 = dp.clone(), float(hand.loss_out[0])
    dw = torch.full((B, T), float("nan"), device=DEV)
    so = _spectral_op(U, wv, wav, dw, False, hand.loss_out)
    U.ops.istft_features_bwd(hand.pred, dw, dp, *GEO_OP, accumulate=True)
    hand.backward(dpred=dp)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dp).all()) and bool(torch.isfinite(eng.grad).all())
    assert torch.equal(eng.grad.view(torch.int32), hand.grad.view(torch.int32))
    assert torch.equal(eng.loss_out, hand.loss_out) and torch.equal(sl.spectral_out, so) and float(so[0]) > 0 and float(so[2]) == B
    assert not torch.equal(eng.theta, theta0)
    # the references' dpred: the term of the waveform the step reconstructed, carried to the prediction, on top of the wave loss's
    # dpred - each kernel within its own bound
    cf = SR.closed_form(wv.cpu().numpy(), wav.cpu().numpy(), RES, FLOOR, SCW, LW, WEIGHT, B)
    err_w, tol_w = np.abs(dw.cpu().numpy().astype(np.float64) - cf["dwav"]), SR.bound(cf["dwav"], cf["abs"], cf["n_terms"])
    assert (err_w <= tol_w).all() and np.abs(cf["dwav"]).max() > 0
    vj = DR.vjp_closed_form(hand.pred.cpu().numpy(), dw.cpu().numpy(), *GEO_REF)
    base = dp0.cpu().numpy()
    err = np.abs(dp.cpu().numpy().astype(np.float64) - (base.astype(np.float64) + vj["grad"]))
    assert (err <= DR.bound_accumulated(base, vj["grad"], vj["abs"], vj["n_terms"])).all() and np.abs(vj["grad"]).max() > 0
    # loss_out[0] has grown by the term: one fp32 addition of the rounded term
    assert (np.abs(so.cpu().numpy()[:2] - cf["spectral_out"][:2]) <= cf["spectral_out_tol"][:2]).all()
    term = np.float32(WEIGHT / B * (SCW * float(so[0]) + LW * float(so[1])))
    assert float(hand.loss_out[0]) == float(np.float32(np.float32(loss0) + term)) and term > 0
    # the term is in the gradient: the step without it differs
    plain = _engine(U, "unet", dtype)
    ptr = U.Trainer(plain, lr=1e-3, dropout=False, wave_loss=_wave(U) if user_wave else None)
    ptr.step(a, e, b, wav_true=wav if user_wave else None)
    torch.cuda.synchronize()
    assert not torch.equal(plain.grad, eng.grad) and float(eng.loss_out[0]) > float(plain.loss_out[0])
    with pytest.raises(ValueError, match="wav_true"):
        tr.step(a, e, b)


@pytest.mark.parametrize("user_wave", [False, True], ids=["no-wave-loss", "with-wave-loss"])
def test_with_a_decay_loss_one_adjoint_carries_both(U, user_wave):
    """decay writes its dwav, the spectral term adds to it, one vector-Jacobian product: bit for bit the same launches by hand, and within
    the accumulate bounds of the step with two separate products.  With base the dpred of the wave-loss call: the shared form is
    fl(base + V(dw_sum)), dw_sum = fl32(dw_d + g_s); the separate one is fl(fl(base + V(dw_d)) + V(dw_s)), dw_s = fl32(g_s).  V is linear
    and |dw_sum - dw_d - dw_s| <= 2^-24 (|dw_sum| + |dw_s|) per element, which V passes on term by term: 2^-24 (abs of V at dw_sum + abs
    of V at dw_s), next to the three accumulating launches' own bounds."""
    (a, e, b, wav), = _batches(1)
    eng = _engine(U, "unet", "f32")
    wl, dl, sl = (_wave(U) if user_wave else None), _decay(U), _spectral(U)
    tr = U.Trainer(eng, lr=1e-3, dropout=False, wave_loss=wl, decay_loss=dl, spectral_loss=sl)
    tr.step(a, e, b, wav_true=wav)
    hand = _engine(U, "unet", "f32")
    dp, wv = _front(U, hand, a, e, b, wav, wl)
    dp0 = dp.clone()
    dw_d = torch.full((B, T), float("nan"), device=DEV)
    do = torch.zeros(2, dtype=torch.float64, device=DEV)
    U.ops.decay_loss(wv, wav, do, U.ops.Workspace(DEV), floor_db=D_FLOOR, weight=D_WEIGHT, global_batch=B, dwav=dw_d, loss_out=hand.loss_out)
    dw_sum = dw_d.clone()
    so = _spectral_op(U, wv, wav, dw_sum, True, hand.loss_out)
    U.ops.istft_features_bwd(hand.pred, dw_sum, dp, *GEO_OP, accumulate=True)
    hand.backward(dpred=dp)
    torch.cuda.synchronize()
    assert torch.equal(eng.grad.view(torch.int32), hand.grad.view(torch.int32)) and torch.equal(eng.loss_out, hand.loss_out)
    assert torch.equal(dl.decay_out, do) and torch.equal(sl.spectral_out, so) and torch.equal(dl._dwav, dw_sum)
    # the summed cotangent: the spectral kernel's accumulate bound on top of the decay term's dwav
    cf = SR.closed_form(wv.cpu().numpy(), wav.cpu().numpy(), RES, FLOOR, SCW, LW, WEIGHT, B)
    bd = dw_d.cpu().numpy()
    err = np.abs(dw_sum.cpu().numpy().astype(np.float64) - (bd.astype(np.float64) + cf["dwav"]))
    assert (err <= SR.bound_accumulated(bd, cf["dwav"], cf["abs"], cf["n_terms"])).all()
    # two separate products
    dw_s = torch.full((B, T), float("nan"), device=DEV)
    _spectral_op(U, wv, wav, dw_s, False, None)
    two = dp0.clone()
    U.ops.istft_features_bwd(hand.pred, dw_d, two, *GEO_OP, accumulate=True)
    mid = two.clone()
    U.ops.istft_features_bwd(hand.pred, dw_s, two, *GEO_OP, accumulate=True)
    torch.cuda.synchronize()
    pred = hand.pred.cpu().numpy()
    v_sum = DR.vjp_closed_form(pred, dw_sum.cpu().numpy(), *GEO_REF)
    v_d = DR.vjp_closed_form(pred, dw_d.cpu().numpy(), *GEO_REF)
    v_s = DR.vjp_closed_form(pred, dw_s.cpu().numpy(), *GEO_REF)
    base, mid_ = dp0.cpu().numpy(), mid.cpu().numpy()
    tol = (DR.bound_accumulated(base, v_sum["grad"], v_sum["abs"], v_sum["n_terms"]) +
           DR.bound_accumulated(base, v_d["grad"], v_d["abs"], v_d["n_terms"]) +
           DR.bound_accumulated(mid_, v_s["grad"], v_s["abs"], v_s["n_terms"]) + 2.0 ** -24 * (v_sum["abs"] + v_s["abs"]))
    err = np.abs(dp.cpu().numpy().astype(np.float64) - two.cpu().numpy().astype(np.float64))
    print(f"shared against separate: largest err / allowance {float((err / tol).max()):.3f}")
    assert (err <= tol).all() and np.abs(v_s["grad"]).max() > 0 and np.abs(v_d["grad"]).max() > 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_trainer_without_the_term_is_the_step_it_was(U, dtype):
    """no spectral_loss: the decay path's own launches (forward, wave loss, decay loss, its vector-Jacobian product, backward), bit for
    bit; and weight = 0 adds exact zeros: the gradients, the loss and the updated parameters of the trainer without the option"""
    (a, e, b, wav), = _batches(1)
    eng = _engine(U, "unet", dtype)
    wl = _wave(U)
    tr = U.Trainer(eng, lr=1e-3, dropout=False, wave_loss=wl, decay_loss=_decay(U))
    assert tr.spectral_loss is None
    tr.step(a, e, b, wav_true=wav)
    hand = _engine(U, "unet", dtype)
    _decay_by_hand(U, hand, a, e, b, wav, wl)
    torch.cuda.synchronize()
    assert torch.equal(eng.grad.view(torch.int32), hand.grad.view(torch.int32)) and torch.equal(eng.loss_out, hand.loss_out)
    with_eng, without_eng = _engine(U, "unet", dtype), _engine(U, "unet", dtype)
    t0 = U.Trainer(with_eng, lr=1e-3, dropout=False, wave_loss=_wave(U), spectral_loss=_spectral(U, 0.0))
    t0.step(a, e, b, wav_true=wav)
    U.Trainer(without_eng, lr=1e-3, dropout=False, wave_loss=_wave(U)).step(a, e, b, wav_true=wav)
    torch.cuda.synchronize()
    assert torch.equal(with_eng.loss_out, without_eng.loss_out) and float(t0.spectral_loss.spectral_out[0]) > 0
    assert torch.equal(with_eng.grad.view(torch.int32), without_eng.grad.view(torch.int32))
    assert torch.equal(with_eng.theta.view(torch.int32), without_eng.theta.view(torch.int32))


@pytest.mark.parametrize("others", [False, True], ids=["spectral-alone", "with-wave-and-decay"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_three_graph_steps_equal_three_eager_steps(U, dtype, others):
    data = _batches(3)
    res = []
    for graph in (True, False):
        eng = _engine(U, "unet", dtype)
        tr = U.Trainer(eng, lr=1e-3, graph=graph, wave_loss=_wave(U) if others else None, decay_loss=_decay(U) if others else None,
                       spectral_loss=_spectral(U))
        if not graph:
            eng.use_device_counters(True)          # the same arithmetic by construction: the step's scalars in device memory for both
        losses = [tr.step(a, e, b, wav_true=wav, return_loss=True) for a, e, b, wav in data]
        torch.cuda.synchronize()
        if graph:
            assert tr.use_graph and set(tr._graphs) == {True} and len(tr._g_in) == 4
        res.append((losses, eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), tr.spectral_loss.spectral_out.clone(), eng.adam_t))
    g, h = res
    assert g[0] == h[0] and g[5] == h[5] == 3
    for i in (1, 2, 3, 4):
        assert torch.equal(g[i], h[i]), i
    assert float(g[4][0]) > 0


def test_train_script_with_the_spectral_loss(U, tmp_path, monkeypatch):
    """scripts/train.py --spectral-loss on the generated tree: the data set keeps the waveforms, fit records the two terms for the
    training and the validation pass; without a data set, or with a resolution the kernels do not take, it refuses"""
    import json
    import os
    import dataset_tree as DT
    from test_dataset_gpu import run_script
    root = str(tmp_path / "rir")
    os.makedirs(root)
    DT.make_tree(root)
    out = str(tmp_path / "ckpt")
    common = ["--rooms", "HemiAnechoicRoom", "SmallMeetingRoom", "--no-debug", "--batch", 4, "--lr", 1e-4, "--out", out, "--epochs", 1,
              "--spectral-loss", 0.01, "--spectral-floor-db", 45]
    run_script(monkeypatch, "train", ["--dataset", root, DT.NAME, "--name", "unet", "--filters", 8, "--spectral-resolutions",
                                      "128:64:32,512:256:128"] + common)
    hist = json.load(open(os.path.join(out, "history.json")))
    assert [h["epoch"] for h in hist] == [1]
    for h in hist:
        assert all(np.isfinite(h[k]) and h[k] > 0 for k in ("train_loss", "val_loss", "train_sc", "val_sc", "train_logmag", "val_logmag"))
        assert "train_wave" not in h and "train_decay" not in h
    with pytest.raises(SystemExit, match="--dataset"):
        run_script(monkeypatch, "train", ["--synthetic", 2, "--name", "unet", "--filters", 8] + common)
    with pytest.raises(SystemExit, match="--spectral-resolutions"):
        run_script(monkeypatch, "train", ["--dataset", root, DT.NAME, "--name", "unet", "--filters", 8, "--spectral-resolutions", "100:64"] + common)

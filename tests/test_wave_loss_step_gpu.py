"""The train step with a WaveLoss on the device: Trainer.step(..., wav_true=) is the step done by hand (forward with the target, the
wave-loss call with the fused spectrogram term, backward from its dpred) bit for bit, and the step replayed as a HIP graph is the step
issued launch by launch.  32 x 48 planes, batch 2, n_fft 32 (17 bins), window 16, hop 8, 41 frames: T = 320."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, B = 32, 48, 2
GEO = dict(des_shape=(17, 41), n_fft=32, win_length=16, hop_length=8)
T = 320
CONV = ((8, 16, 16, 32), (3, 3, 3, 3), (2, 2, 2, 2), 8, 16)


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def _engine(U, kind, dtype):
    if kind == "unet":
        eng = U.UNetEngine(H, W, B, F0=8, k=3, device=DEV, dtype=dtype)
    elif kind == "ae":
        eng = U.AutoencoderEngine(H, W, B, *CONV, device=DEV, dtype=dtype)
    else:
        eng = U.DiffUNetEngine(H, W, B, F0=4 if dtype == "f32" else 16, device=DEV, dtype=dtype)
    g = torch.Generator(); g.manual_seed(3)
    eng.reset_parameters(g)
    eng.dropout_seed = 77
    return eng


def _batches(n):
    gen = torch.Generator(); gen.manual_seed(5)
    out = []
    for _ in range(n):
        out.append((torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
                    torch.rand((B, 2, H, W), generator=gen).to(DEV), (torch.randn((B, T), generator=gen) * 0.5).to(DEV)))
    return out


def _wave(U, **kw):
    return U.WaveLoss(weight=0.25, norm="energy", time_weight=torch.linspace(1.0, 0.1, T), **GEO, **kw)


def _by_hand(U, eng, wl_args, a, e, b, wav, diff):
    """forward(target), ops.wave_loss, backward(dpred) on `eng`; returns (dpred, wave_out)"""
    eng.training = True
    eng.loss_diff = diff
    eng.forward(a, e, target=b, global_batch=B, alpha=0.9)
    dp = torch.full_like(eng.pred, float("nan"))
    wo = torch.zeros(2, dtype=torch.float64, device=DEV)
    U.ops.wave_loss(eng.pred, wav, wo, U.ops.Workspace(DEV), *GEO["des_shape"], GEO["n_fft"], GEO["win_length"], GEO["hop_length"],
                    norm="energy", weight=0.25, global_batch=B, time_weight=wl_args.time_weight, phase_ref=a if diff else None,
                    spec_target=b, alpha=0.9, inv_norm=1.0 / (2.0 * H * W * B), dpred=dp, loss_out=eng.loss_out)
    eng.backward(dpred=dp)
    return dp, wo


@pytest.mark.parametrize("kind,dtype", [("unet", "f32"), ("unet", "bf16"), ("ae", "f32"), ("ae", "bf16"), ("diffunet", "f32"), ("diffunet", "bf16")])
def test_trainer_step_is_the_step_done_by_hand(U, kind, dtype):
    (a, e, b, wav), = _batches(1)
    diff = kind == "diffunet"
    eng = _engine(U, kind, dtype)
    wl = _wave(U)
    tr = U.Trainer(eng, lr=1e-3, dropout=False, wave_loss=wl, diff_loss=diff)
    theta0 = eng.theta.clone()
    tr.step(a, e, b, wav_true=wav)
    hand = _engine(U, kind, dtype)
    dp, wo = _by_hand(U, hand, wl, a, e, b, wav, diff)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dp).all()) and bool(torch.isfinite(eng.grad).all())
    assert torch.equal(eng.grad.view(torch.int32), hand.grad.view(torch.int32))
    assert torch.equal(eng.loss_out, hand.loss_out) and torch.equal(wl.wave_out, wo) and float(wo[0]) > 0
    assert not torch.equal(eng.theta, theta0)
    # the term is in the gradient: the plain step's differs
    plain = _engine(U, kind, dtype)
    U.Trainer(plain, lr=1e-3, dropout=False, diff_loss=diff).step(a, e, b)
    torch.cuda.synchronize()
    assert not torch.equal(plain.grad, eng.grad) and float(eng.loss_out[0]) > float(plain.loss_out[0])
    with pytest.raises(ValueError, match="wav_true"):
        tr.step(a, e, b)


def test_train_script_with_the_wave_loss(U, tmp_path, monkeypatch):
    """scripts/train.py --wave-loss on the generated tree: the data set keeps the waveforms, the generators hand them out, fit
    records the term for the training and the validation pass; without a data set, or for a model with a loss term of its own, it
    refuses."""
    import json
    import os
    import numpy as np
    import dataset_tree as DT
    from test_dataset_gpu import run_script
    root = str(tmp_path / "rir")
    os.makedirs(root)
    DT.make_tree(root)
    out = str(tmp_path / "ckpt")
    common = ["--rooms", "HemiAnechoicRoom", "SmallMeetingRoom", "--no-debug", "--batch", 4, "--lr", 1e-4, "--out", out, "--epochs", 2,
              "--wave-loss", 0.1, "--wave-loss-norm", "energy"]
    run_script(monkeypatch, "train", ["--dataset", root, DT.NAME, "--name", "unet", "--filters", 8] + common)
    hist = json.load(open(os.path.join(out, "history.json")))
    assert [h["epoch"] for h in hist] == [1, 2]
    for h in hist:
        assert all(np.isfinite(h[k]) and h[k] > 0 for k in ("train_loss", "val_loss", "train_wave", "val_wave"))
    with pytest.raises(SystemExit, match="--dataset"):
        run_script(monkeypatch, "train", ["--synthetic", 2, "--name", "unet", "--filters", 8] + common)
    with pytest.raises(ValueError, match="wave_loss"):
        run_script(monkeypatch, "train", ["--dataset", root, DT.NAME, "--name", "vae"] + common)


@pytest.mark.parametrize("kind,dtype", [("unet", "f32"), ("unet", "bf16"), ("ae", "f32"), ("ae", "bf16")])
def test_three_graph_steps_equal_three_eager_steps(U, kind, dtype):
    data = _batches(3)
    res = []
    for graph in (True, False):
        eng = _engine(U, kind, dtype)
        tr = U.Trainer(eng, lr=1e-3, graph=graph, wave_loss=_wave(U))
        if not graph:
            eng.use_device_counters(True)          # the same arithmetic by construction: the step's scalars in device memory for both
        losses = [tr.step(a, e, b, wav_true=wav, return_loss=True) for a, e, b, wav in data]
        torch.cuda.synchronize()
        if graph:
            assert tr.use_graph and set(tr._graphs) == {True} and len(tr._g_in) == 4
        res.append((losses, eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), tr.wave_loss.wave_out.clone(), eng.adam_t))
    g, h = res
    assert g[0] == h[0] and g[5] == h[5] == 3
    for i in (1, 2, 3, 4):
        assert torch.equal(g[i], h[i]), i

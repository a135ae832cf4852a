"""The PRODUCT's Trainer with a SpectralLoss(method="fft") on CPU tensors: only the kernels (the stand-ins of tests/, with
tests/spectral_loss_fft_cpu_ops.py on top) and the stream runtime (tests/sim_runtime.py: vector clocks + race check) are stand-ins.
The planes of tests/test_wave_loss_sim.py (16 x 16) with a geometry long enough for the FFT form's smallest transform: n_fft 16 (9
bins), window 16, hop 8, 13 frames, T = 96; the loss looks at it through (128, 64, 32) and (128, 128, 16).  The trainer has no branch
of its own for the method: the object dispatches, and everything else of the step is what it was."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_schedule_sim as SS  # noqa: E402  (its engine builders and oracle configurations)
import test_wave_loss_sim as WS  # noqa: E402  (its planes and batch)
from test_decay_loss_sim import _logged  # noqa: E402

B = WS.B
GEO = dict(des_shape=(9, 13), n_fft=16, win_length=16, hop_length=8)
T = 96
RES = ((128, 64, 32), (128, 128, 16))
OPS = ("wave_loss", "decay_loss", "spectral_loss", "spectral_loss_fft", "istft_features_bwd")


def _install(monkeypatch):
    import spectral_loss_fft_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    return rt, spectral_loss_fft_cpu_ops.install(monkeypatch, rt)


def _batch():
    spec_in, emb, spec_out, _ = WS._batch(B)
    wav = (np.random.RandomState(77).standard_normal((B, T)) * 0.5).astype(np.float32)
    return spec_in, emb, spec_out, (torch.tensor(wav) * torch.exp(-torch.arange(T, dtype=torch.float32) / 12.0)).contiguous()


def _build(rt, kind, overlap, wave, decay, spectral, lr=WS.LR, **kw):
    import unet_rir_amd as U
    cfg, eng, _ = SS._build(rt, B, overlap, world=1, bucket_bytes=8192, kind=kind)
    return eng, U.Trainer(eng, lr=lr, dropout=False, bucket_bytes=8192, wave_loss=wave, decay_loss=decay, spectral_loss=spectral, **kw)


def _spectral(method, weight=0.05):
    import unet_rir_amd as U
    return U.SpectralLoss(weight=weight, resolutions=RES, sc_weight=0.8, log_weight=1.3, floor_db=30.0, method=method, **GEO)


def _wave():
    import unet_rir_amd as U
    return U.WaveLoss(weight=0.3, norm="energy", **GEO)


def _decay():
    import unet_rir_amd as U
    return U.DecayLoss(weight=0.05, floor_db=30.0, **GEO)


@pytest.mark.parametrize("user_wave", [False, True])
@pytest.mark.parametrize("kind,overlap", [("unet", False), ("unet", True), ("ae", True)])
def test_a_step_launches_the_fft_op_where_the_dft_op_stood(monkeypatch, kind, overlap, user_wave):
    rt, impl = _install(monkeypatch)
    logs = {}
    for method in ("dft", "fft"):
        eng, tr = _build(rt, kind, overlap, _wave() if user_wave else None, None, _spectral(method))
        log = _logged(monkeypatch, rt)
        spec_in, emb, spec_out, wav = _batch()
        before = eng.theta.clone()
        for _ in range(2):
            tr.step(spec_in, emb, spec_out, wav_true=wav)          # a RaceError here: an unordered cross-stream access
        assert bool(torch.isfinite(eng.theta).all()) and not torch.equal(eng.theta, before)
        so = tr.spectral_loss.spectral_out
        assert float(so[0]) > 0 and float(so[1]) > 0 and float(so[2]) == B
        logs[method] = list(log)                                   # a later `_logged` wraps this one: keep what it held here
    assert impl.spectral.calls == [("spectral", B, True, False)] * 2 and impl.spectral_fft.calls == [("spectral_fft", B, True, False)] * 2
    assert "spectral_loss_fft" not in logs["dft"] and "spectral_loss" not in logs["fft"]
    # the same launches in the same order, one name exchanged
    assert [w.replace("spectral_loss_fft", "spectral_loss") for w in logs["fft"]] == logs["dft"]
    i = logs["fft"].index("wave_loss")
    assert logs["fft"][i + 1:i + 4] == ["spectral_loss_fft", "istft_features_bwd", "sigmoid_bwd"]


@pytest.mark.parametrize("overlap", [False, True])
def test_with_a_decay_loss_there_is_still_one_adjoint_launch(monkeypatch, overlap):
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", overlap, None, _decay(), _spectral("fft"), lr=0.0)
    log = _logged(monkeypatch, rt)
    spec_in, emb, spec_out, wav = _batch()
    tr.step(spec_in, emb, spec_out, wav_true=wav)
    assert impl.decay.calls == [("decay", B, True), ("vjp", True, False)] and impl.spectral_fft.calls == [("spectral_fft", B, True, True)]
    assert impl.spectral.calls == []
    i = log.index("wave_loss")
    assert log[i + 1:i + 5] == ["decay_loss", "spectral_loss_fft", "istft_features_bwd", "sigmoid_bwd"]
    assert log.count("istft_features_bwd") == 1 and log.count("spectral_loss_fft") == 1


@pytest.mark.parametrize("with_decay", [False, True])
def test_under_graph_the_captured_body_has_the_order_and_allocates_nothing(monkeypatch, with_decay):
    """what a capture depends on (the replayed step is held to the eager one bit for bit in tests/test_spectral_loss_fft_gpu.py): the
    body's launch order, and that its second pass - the one that would be recorded - allocates nothing: every buffer of the loss objects
    keeps its address, the spectral loss's from `prepare` at construction on, with the FFT form's (smaller) workspace"""
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", False, None, _decay() if with_decay else None, _spectral("fft"), graph=True)
    assert tr.use_graph
    sl, wl = tr.spectral_loss, tr._wave
    import unet_rir_amd as U
    assert sl._ws.buf.numel() * sl._ws.buf.element_size() >= U.ops.spectral_loss_fft_ws_bytes(B, T, RES) > 0
    prepared = (sl._ws.buf.data_ptr(), sl._dwav.data_ptr(), sl.spectral_out.data_ptr())
    spec_in, emb, spec_out, wav = _batch()
    tr._step_body(spec_in, emb, spec_out, None, True, wav)              # the ordinary pass
    held = lambda: (sl._ws.buf.data_ptr(), sl._dwav.data_ptr(), sl.spectral_out.data_ptr(), wl._ws.buf.data_ptr(), wl._dpred.data_ptr(),
                    wl.wav_pred.data_ptr(), wl.wave_out.data_ptr())
    first = held()
    assert first[:3] == prepared
    log = _logged(monkeypatch, rt)
    tr._step_body(spec_in, emb, spec_out, None, True, wav)              # the pass a capture records
    assert held() == first
    i = log.index("wave_loss")
    want = (["decay_loss"] if with_decay else []) + ["spectral_loss_fft", "istft_features_bwd", "sigmoid_bwd"]
    assert log[i + 1:i + 1 + len(want)] == want and log.count("spectral_loss_fft") == 1 and log.count("istft_features_bwd") == 1
    assert "spectral_loss" not in log


def test_a_trainer_with_the_dft_form_or_without_the_term_launches_no_new_op(monkeypatch):
    rt, impl = _install(monkeypatch)
    spec_in, emb, spec_out, wav = _batch()
    for wave, decay, spectral, want in ((None, None, None, []), (_wave(), None, None, ["wave_loss"]),
                                        (None, _decay(), None, ["wave_loss", "decay_loss", "istft_features_bwd"]),
                                        (None, None, _spectral("dft"), ["wave_loss", "spectral_loss", "istft_features_bwd"]),
                                        (_wave(), _decay(), _spectral("dft"), ["wave_loss", "decay_loss", "spectral_loss", "istft_features_bwd"])):
        eng, tr = _build(rt, "unet", False, wave, decay, spectral)
        log = _logged(monkeypatch, rt)
        tr.step(spec_in, emb, spec_out, wav_true=None if not want else wav)
        assert [w for w in log if w in OPS] == want
    assert impl.spectral_fft.calls == [] and len(impl.spectral.calls) == 2


def test_the_validation_pass_and_a_resolution_the_form_refuses(monkeypatch):
    import unet_rir_amd as U
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", False, None, None, _spectral("fft"), lr=0.0)
    spec_in, emb, spec_out, wav = _batch()
    rec = U.fit(tr, lambda ep: [(spec_in, emb, spec_out, wav)], 1, val_batches=lambda ep: [(spec_in, emb, spec_out, wav)], log=None)[0]
    assert impl.spectral_fft.calls == [("spectral_fft", B, True, False), ("spectral_fft", B, False, False)] and impl.spectral.calls == []
    assert rec["train_sc"] > 0 and rec["val_sc"] == rec["train_sc"] and rec["val_logmag"] == rec["train_logmag"]
    with pytest.raises(ValueError, match=r'\(64, 64, 16\).*method="dft"'):
        U.SpectralLoss(resolutions=((64, 64, 16),), method="fft", **GEO)
    with pytest.raises(ValueError, match=r'\(256, 128, 64\).*method="dft"'):               # T = 96 < 129
        U.SpectralLoss(resolutions=((256, 128, 64),), method="fft", **GEO)

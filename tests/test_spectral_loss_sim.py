"""The PRODUCT's Trainer / fit with a SpectralLoss on CPU tensors: only the kernels (tests/cpu_ops.py, tests/wave_loss_cpu_ops.py,
tests/decay_loss_cpu_ops.py and tests/spectral_loss_cpu_ops.py: fp64 arithmetic from the references) and the stream runtime
(tests/sim_runtime.py: vector clocks + race check) are stand-ins.  The geometry of tests/test_wave_loss_sim.py: 16 x 16 planes, n_fft
16 (9 bins), window 8, hop 4, 13 frames, T = 48; the loss looks at it through (16, 16, 4) and (32, 16, 8).  A missing happens-before
edge would raise RaceError."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_schedule_sim as SS  # noqa: E402  (its engine builders and oracle configurations)
import test_wave_loss_sim as WS  # noqa: E402  (its geometry, batches and wave-loss builder)
import test_decay_loss_sim as DS  # noqa: E402  (its decaying batch and decay-loss builder)

B, T, GEO = WS.B, WS.T, WS.GEO
RES = ((16, 16, 4), (32, 16, 8))
SPEC = ("spectral", B, True, False)
_batch, _decay, _logged = DS._batch, DS._decay, DS._logged


def _install(monkeypatch):
    import spectral_loss_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    return rt, spectral_loss_cpu_ops.install(monkeypatch, rt)


def _build(rt, kind, overlap, wave, decay, spectral, world=1, lr=WS.LR, **kw):
    import unet_rir_amd as U
    cfg, eng, _ = SS._build(rt, B, overlap, world=world, bucket_bytes=8192, kind=kind)
    extra = {} if spectral is None else {"spectral_loss": spectral}
    return eng, U.Trainer(eng, lr=lr, dropout=False, world_size=world, bucket_bytes=8192, wave_loss=wave, decay_loss=decay, **extra, **kw)


def _spectral(weight=0.05, floor_db=30.0):
    import unet_rir_amd as U
    return U.SpectralLoss(weight=weight, resolutions=RES, sc_weight=0.8, log_weight=1.3, floor_db=floor_db, **GEO)


@pytest.mark.parametrize("user_wave", [False, True])
@pytest.mark.parametrize("kind,overlap", [("unet", False), ("unet", True), ("ae", False), ("ae", True)])
def test_step_is_race_free_and_the_launch_order_holds(monkeypatch, kind, overlap, user_wave):
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, kind, overlap, WS._wave() if user_wave else None, None, _spectral())
    assert (tr.wave_loss is not None) == user_wave and tr._wave is not None and (user_wave or tr._wave.weight == 0.0)
    log = _logged(monkeypatch, rt)
    spec_in, emb, spec_out, wav = _batch()
    before = eng.theta.clone()
    for _ in range(2):
        tr.step(spec_in, emb, spec_out, wav_true=wav)          # a RaceError here: an unordered cross-stream access
    assert impl.wave.calls == [(B, True, True)] * 2
    assert impl.spectral.calls == [SPEC] * 2 and impl.decay.calls == [("vjp", True, False)] * 2
    assert bool(torch.isfinite(eng.theta).all()) and not torch.equal(eng.theta, before)
    i = log.index("wave_loss")
    assert log[i + 1:i + 4] == ["spectral_loss", "istft_features_bwd", "sigmoid_bwd"] and "sigmoid_loss" in log[:i]
    assert not [w for w in log[:i + 3] if "wgrad" in w or "dgrad" in w or w.endswith("_bwd") and w != "istft_features_bwd"]
    if overlap:
        assert rt.n_cross_stream > 50
    else:
        assert rt.n_cross_stream == 0
    so = tr.spectral_loss.spectral_out
    assert float(so[0]) > 0 and float(so[1]) > 0 and float(so[2]) == B


@pytest.mark.parametrize("overlap", [False, True])
def test_with_a_decay_loss_one_adjoint_launch_carries_both_cotangents(monkeypatch, overlap):
    import decay_loss_ref as DR
    import spectral_loss_ref as SR
    import wave_loss_ref as WR
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", overlap, None, _decay(), _spectral(), lr=0.0)
    log = _logged(monkeypatch, rt)
    spec_in, emb, spec_out, wav = _batch()
    tr.step(spec_in, emb, spec_out, wav_true=wav)
    assert impl.decay.calls == [("decay", B, True), ("vjp", True, False)] and impl.spectral.calls == [("spectral", B, True, True)]
    i = log.index("wave_loss")
    assert log[i + 1:i + 5] == ["decay_loss", "spectral_loss", "istft_features_bwd", "sigmoid_bwd"] and log.count("istft_features_bwd") == 1
    # dpred = the spectrogram term's, rounded to fp32, plus the product of the summed cotangent
    geo = (GEO["des_shape"], 16, 8, 4)
    wl = WR.closed_form(eng.pred.numpy(), wav.numpy(), *geo, norm="mse", weight=0.0, global_batch=B, spec_target=spec_out.numpy(),
                        alpha=0.9, inv_norm=1.0 / (2.0 * WS.H * WS.W * B))
    wav_pred = wl["wav"].astype(np.float32)
    d = DR.closed_form(wav_pred, wav.numpy(), 30.0, weight=0.05, global_batch=B)
    s = SR.closed_form(wav_pred, wav.numpy(), RES, 30.0, 0.8, 1.3, 0.05, B)
    dwav = (d["dwav"].astype(np.float32).astype(np.float64) + s["dwav"]).astype(np.float32)
    assert np.array_equal(tr.decay_loss._dwav.numpy(), dwav)
    vj = DR.vjp_closed_form(eng.pred.numpy(), dwav, *geo)["grad"]
    want = (wl["grad"].astype(np.float32).astype(np.float64) + vj).astype(np.float32)
    assert np.array_equal(tr._wave._dpred.numpy(), want) and np.abs(vj).max() > 0


def test_a_trainer_without_the_term_launches_what_it_launched_before(monkeypatch):
    """plain, wave_loss alone, decay_loss alone, both: no spectral launch, and the decay path's own sequence"""
    rt, impl = _install(monkeypatch)
    spec_in, emb, spec_out, wav = _batch()
    for wave, decay, want in ((None, None, []), (WS._wave(), None, ["wave_loss"]), (None, _decay(), ["wave_loss", "decay_loss", "istft_features_bwd"]),
                              (WS._wave(), _decay(), ["wave_loss", "decay_loss", "istft_features_bwd"])):
        eng, tr = _build(rt, "unet", False, wave, decay, None)
        assert tr.spectral_loss is None
        log = _logged(monkeypatch, rt)
        tr.step(spec_in, emb, spec_out, wav_true=None if not want else wav)
        assert [w for w in log if w in ("wave_loss", "decay_loss", "spectral_loss", "istft_features_bwd")] == want
        assert "spectral_loss" not in log
    assert impl.spectral.calls == []


@pytest.mark.parametrize("with_decay", [False, True])
def test_under_graph_the_captured_body_has_the_order_and_allocates_nothing(monkeypatch, with_decay):
    """graph=True captures `_step_body` after one ordinary pass through it.  A capture needs a device (the replayed step is held to the
    eager one bit for bit in tests/test_spectral_loss_step_gpu.py); what can be held here is what a capture depends on: the body's launch
    order, and that its second pass - the one that would be recorded - allocates nothing: every buffer of the loss objects keeps its
    address, the spectral loss's from `prepare` at construction on."""
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", False, None, _decay() if with_decay else None, _spectral(), graph=True)
    assert tr.use_graph
    sl, wl = tr.spectral_loss, tr._wave
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
    want = (["decay_loss"] if with_decay else []) + ["spectral_loss", "istft_features_bwd", "sigmoid_bwd"]
    assert log[i + 1:i + 1 + len(want)] == want and log.count("spectral_loss") == 1 and log.count("istft_features_bwd") == 1


def test_loss_out_grows_by_exactly_the_term_and_dpred_is_the_sum(monkeypatch):
    import decay_loss_ref as DR
    import spectral_loss_ref as SR
    import wave_loss_ref as WR
    rt, impl = _install(monkeypatch)
    plain_eng, plain = _build(rt, "unet", False, None, None, None, lr=0.0)
    sp_eng, sp = _build(rt, "unet", False, None, None, _spectral(), lr=0.0)
    spec_in, emb, spec_out, wav = _batch()
    plain.step(spec_in, emb, spec_out)
    sp.step(spec_in, emb, spec_out, wav_true=wav)
    assert torch.equal(plain_eng.pred, sp_eng.pred)
    geo = (GEO["des_shape"], 16, 8, 4)
    wl = WR.closed_form(sp_eng.pred.numpy(), wav.numpy(), *geo, norm="mse", weight=0.0, global_batch=B, spec_target=spec_out.numpy(),
                        alpha=0.9, inv_norm=1.0 / (2.0 * WS.H * WS.W * B))
    cf = SR.closed_form(wl["wav"].astype(np.float32), wav.numpy(), RES, 30.0, 0.8, 1.3, 0.05, B)
    assert cf["loss"] > 0 and wl["loss"] == 0.0
    assert float(sp_eng.loss_out[0]) == float(np.float32(np.float32(plain_eng.loss_out[0]) + np.float32(cf["loss"])))
    assert torch.equal(sp_eng.loss_out[1:3], plain_eng.loss_out[1:3])
    assert np.allclose(sp.spectral_loss.spectral_out.numpy(), cf["spectral_out"], rtol=1e-12)
    vj = DR.vjp_closed_form(sp_eng.pred.numpy(), cf["dwav"].astype(np.float32), *geo)["grad"]
    want = (wl["grad"].astype(np.float32).astype(np.float64) + vj).astype(np.float32)
    assert np.array_equal(sp._wave._dpred.numpy(), want) and np.abs(vj).max() > 0


@pytest.mark.parametrize("kind", ["unet", "ae"])
def test_weight_zero_is_the_trainer_without_the_option(monkeypatch, kind):
    """weight = 0 makes dwav an exact zero, so the accumulate pass adds zeros: the gradients of the step are those of the trainer with
    the same wave_loss and no spectral_loss, bit for bit"""
    rt, impl = _install(monkeypatch)
    a_eng, a = _build(rt, kind, False, WS._wave(), None, None)
    b_eng, b = _build(rt, kind, False, WS._wave(), None, _spectral(weight=0.0))
    spec_in, emb, spec_out, wav = _batch()
    la = a.step(spec_in, emb, spec_out, wav_true=wav, return_loss=True)
    lb = b.step(spec_in, emb, spec_out, wav_true=wav, return_loss=True)
    assert la == lb and torch.equal(a_eng.grad, b_eng.grad) and torch.equal(a_eng.theta, b_eng.theta)
    assert float(b.spectral_loss.spectral_out[0]) > 0


def test_fit_records_the_two_terms(monkeypatch):
    import unet_rir_amd as U
    import spectral_loss_ref as SR
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", False, None, None, _spectral(), lr=0.0)
    spec_in, emb, spec_out, wav = _batch()
    four = (spec_in, emb, spec_out, wav)
    generator_style = (spec_in, emb, spec_out, (torch.zeros(B, dtype=torch.int64), wav))
    rec = U.fit(tr, lambda ep: [four, generator_style], 1, val_batches=lambda ep: [generator_style], log=None)[0]
    cf = SR.closed_form(tr._wave.wav_pred.numpy(), wav.numpy(), RES, 30.0, 0.8, 1.3, 0.05, B)
    for key, want in (("sc", cf["spectral_out"][0] / B), ("logmag", cf["spectral_out"][1] / B)):     # lr = 0, no dropout: the same prediction
        assert abs(rec["train_" + key] - want) <= 1e-9 * want and abs(rec["val_" + key] - want) <= 1e-9 * want
    assert np.isfinite(rec["train_loss"]) and np.isfinite(rec["val_loss"])
    # the validation pass: the loss alone - no gradient, no vector-Jacobian product
    assert impl.spectral.calls == [SPEC] * 2 + [("spectral", B, False, False)] and impl.decay.calls == [("vjp", True, False)] * 2
    assert impl.wave.calls == [(B, True, True)] * 2 + [(B, False, False)]
    assert not {"train_wave", "val_wave", "train_decay", "val_decay"} & set(rec)
    with pytest.raises(ValueError, match="spectral_loss"):
        U.fit(tr, lambda ep: [(spec_in, emb, spec_out)], 1, log=None)
    # with a wave_loss and a decay_loss all pairs are recorded; a silent target is not counted in the means
    eng2, tr2 = _build(rt, "unet", False, WS._wave(), _decay(), _spectral(), lr=0.0)
    quiet = wav.clone()
    quiet[1] = 0.0
    rec2 = U.fit(tr2, lambda ep: [(spec_in, emb, spec_out, quiet)], 1, log=None)[0]
    cf2 = SR.closed_form(tr2._wave.wav_pred.numpy(), quiet.numpy(), RES, 30.0, 0.8, 1.3, 0.05, B)
    assert {"train_wave", "train_decay", "train_sc", "train_logmag"} <= set(rec2) and cf2["spectral_out"][2] == B - 1
    assert abs(rec2["train_sc"] - cf2["spectral_out"][0] / (B - 1)) <= 1e-9 * rec2["train_sc"]
    assert abs(rec2["train_logmag"] - cf2["spectral_out"][1] / (B - 1)) <= 1e-9 * rec2["train_logmag"]


def test_refusals(monkeypatch):
    import unet_rir_amd as U
    import cnn_clas_cpu_ops
    import vae_cpu_ops
    from sim_runtime import SimRuntime
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", False, None, None, _spectral())
    spec_in, emb, spec_out, wav = _batch()
    with pytest.raises(ValueError, match="wav_true"):
        tr.step(spec_in, emb, spec_out)
    other = dict(des_shape=(9, 13), n_fft=16, win_length=16, hop_length=4)
    with pytest.raises(ValueError, match="spectral_loss: its geometry"):
        _build(rt, "unet", False, WS._wave(), None, U.SpectralLoss(resolutions=RES, **other))
    with pytest.raises(ValueError, match="spectral_loss: its geometry"):
        _build(rt, "unet", False, None, _decay(), U.SpectralLoss(resolutions=RES, **other))
    with pytest.raises(ValueError, match="do not take"):                                    # T = 48 < 1024 / 2 + 1
        _build(rt, "unet", False, None, None, U.SpectralLoss(**GEO))
    conv = ((4, 8, 8, 8), (3, 3, 3, 3), (2, 2, 2, 2))
    rt2 = SimRuntime()
    vae_cpu_ops.install(monkeypatch, rt2)
    for make in (lambda: U.VAEEngine(WS.H, WS.W, B, *conv, 8, 16, device="cpu", runtime=rt2),
                 lambda: U.VQVAEEngine(16, 32, B, *conv, 4, 8, device="cpu", runtime=rt2)):
        with pytest.raises(ValueError, match="spectral_loss: .* has a loss term or target of its own"):
            U.Trainer(make(), spectral_loss=_spectral())
    rt3 = SimRuntime()
    cnn_clas_cpu_ops.install(monkeypatch, rt3)
    with pytest.raises(ValueError, match="spectral_loss: .* has a loss term or target of its own"):
        U.Trainer(U.DeepCNNEngine(21, 24, 3, classes=5, device="cpu", runtime=rt3), spectral_loss=_spectral())


def _dp_worker(rank, world, port, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mpatch = pytest.MonkeyPatch()
        rt, impl = _install(mpatch)
        eng, tr = _build(rt, "unet", True, None, None, _spectral(), world=world)
        tr.broadcast_parameters(0)
        spec_in, emb, spec_out, wav = _batch(B * world)
        sl = slice(rank * B, (rank + 1) * B)
        for _ in range(2):
            tr.step(spec_in[sl].contiguous(), emb[sl].contiguous(), spec_out[sl].contiguous(), wav_true=wav[sl].contiguous())
        torch.save({"calls": impl.spectral.calls, "theta": eng.theta.clone(), "out": tr.spectral_loss.spectral_out.clone()}, f"{out_path}.{rank}")
        mpatch.undo()
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_see_the_global_batch(tmp_path):
    world = 2
    out = str(tmp_path / "dp")
    mp.spawn(_dp_worker, args=(world, 36300 + (os.getpid() % 1500), out), nprocs=world, join=True)
    res = [torch.load(f"{out}.{r}") for r in range(world)]
    for r in range(world):
        assert res[r]["calls"] == [("spectral", 2 * B, True, False)] * 2
    assert torch.equal(res[0]["theta"], res[1]["theta"]) and not torch.equal(res[0]["out"], res[1]["out"])

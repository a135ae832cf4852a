"""The PRODUCT's Trainer / fit with a DecayLoss on CPU tensors: only the kernels (tests/cpu_ops.py, tests/wave_loss_cpu_ops.py and
tests/decay_loss_cpu_ops.py: fp64 arithmetic from the references) and the stream runtime (tests/sim_runtime.py: vector clocks + race
check) are stand-ins.  The geometry of tests/test_wave_loss_sim.py: 16 x 16 planes, n_fft 16 (9 bins), window 8, hop 4, 13 frames,
T = 48.  A missing happens-before edge would raise RaceError."""
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

B, T, GEO = WS.B, WS.T, WS.GEO


def _install(monkeypatch):
    import decay_loss_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    return rt, decay_loss_cpu_ops.install(monkeypatch, rt)


def _batch(n=B, rank=0):
    """the batch of the wave-loss tests with decaying targets: noise under an exponential envelope"""
    spec_in, emb, spec_out, wav = WS._batch(n, rank)
    return spec_in, emb, spec_out, (wav * torch.exp(-torch.arange(T, dtype=torch.float32) / 6.0)).contiguous()


def _build(rt, kind, overlap, wave, decay, world=1, lr=WS.LR, **kw):
    import unet_rir_amd as U
    cfg, eng, _ = SS._build(rt, B, overlap, world=world, bucket_bytes=8192, kind=kind)
    return eng, U.Trainer(eng, lr=lr, dropout=False, world_size=world, bucket_bytes=8192, wave_loss=wave, decay_loss=decay, **kw)


def _decay(weight=0.05, floor_db=30.0):
    import unet_rir_amd as U
    return U.DecayLoss(weight=weight, floor_db=floor_db, **GEO)


def _logged(monkeypatch, rt):
    log, touch = [], rt.touch

    def logged(reads=(), writes=(), what="", stream=None):
        log.append(what)
        return touch(reads, writes, what, stream)
    monkeypatch.setattr(rt, "touch", logged)
    return log


@pytest.mark.parametrize("user_wave", [False, True])
@pytest.mark.parametrize("kind,overlap", [("unet", False), ("unet", True), ("ae", False), ("ae", True)])
def test_step_is_race_free_and_the_launch_order_holds(monkeypatch, kind, overlap, user_wave):
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, kind, overlap, WS._wave() if user_wave else None, _decay())
    assert (tr.wave_loss is not None) == user_wave and tr._wave is not None and (user_wave or tr._wave.weight == 0.0)
    log = _logged(monkeypatch, rt)
    spec_in, emb, spec_out, wav = _batch()
    before = eng.theta.clone()
    for _ in range(2):
        tr.step(spec_in, emb, spec_out, wav_true=wav)          # a RaceError here: an unordered cross-stream access
    assert impl.wave.calls == [(B, True, True)] * 2
    assert impl.decay.calls == [("decay", B, True), ("vjp", True, False)] * 2
    assert bool(torch.isfinite(eng.theta).all()) and not torch.equal(eng.theta, before)
    i = log.index("wave_loss")
    assert log[i + 1:i + 4] == ["decay_loss", "istft_features_bwd", "sigmoid_bwd"] and "sigmoid_loss" in log[:i]
    assert not [w for w in log[:i + 3] if "wgrad" in w or "dgrad" in w or w.endswith("_bwd") and w != "istft_features_bwd"]
    if overlap:
        assert rt.n_cross_stream > 50
    else:
        assert rt.n_cross_stream == 0
    assert float(tr.decay_loss.decay_out[0]) > 0 and float(tr.decay_loss.decay_out[1]) == B


@pytest.mark.parametrize("user_wave", [False, True])
def test_under_graph_the_captured_body_has_the_order_and_allocates_nothing(monkeypatch, user_wave):
    """graph=True captures `_step_body` after one ordinary pass through it.  A capture needs a device (the replayed step is held to the
    eager one bit for bit in tests/test_decay_loss_step_gpu.py); what can be held here is what a capture depends on: the body's launch
    order, and that its second pass - the one that would be recorded - allocates nothing: every buffer of the two loss objects keeps
    its address, the decay loss's from `prepare` at construction on."""
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", False, WS._wave() if user_wave else None, _decay(), graph=True)
    assert tr.use_graph
    dl, wl = tr.decay_loss, tr._wave
    prepared = (dl._ws.buf.data_ptr(), dl._dwav.data_ptr(), dl.decay_out.data_ptr())
    spec_in, emb, spec_out, wav = _batch()
    tr._step_body(spec_in, emb, spec_out, None, True, wav)              # the ordinary pass
    held = lambda: (dl._ws.buf.data_ptr(), dl._dwav.data_ptr(), dl.decay_out.data_ptr(), wl._ws.buf.data_ptr(), wl._dpred.data_ptr(),
                    wl.wav_pred.data_ptr(), wl.wave_out.data_ptr())
    first = held()
    assert first[:3] == prepared
    log = _logged(monkeypatch, rt)
    tr._step_body(spec_in, emb, spec_out, None, True, wav)              # the pass a capture records
    assert held() == first
    i = log.index("wave_loss")
    assert log[i + 1:i + 4] == ["decay_loss", "istft_features_bwd", "sigmoid_bwd"] and log.count("decay_loss") == 1


def test_loss_out_grows_by_exactly_the_decay_term_and_dpred_is_the_sum(monkeypatch):
    import decay_loss_ref as DR
    import wave_loss_ref as WR
    rt, impl = _install(monkeypatch)
    plain_eng, plain = _build(rt, "unet", False, None, None, lr=0.0)
    dec_eng, dec = _build(rt, "unet", False, None, _decay(weight=0.05), lr=0.0)
    spec_in, emb, spec_out, wav = _batch()
    plain.step(spec_in, emb, spec_out)
    dec.step(spec_in, emb, spec_out, wav_true=wav)
    assert torch.equal(plain_eng.pred, dec_eng.pred)
    geo = (GEO["des_shape"], 16, 8, 4)
    wl = WR.closed_form(dec_eng.pred.numpy(), wav.numpy(), *geo, norm="mse", weight=0.0, global_batch=B, spec_target=spec_out.numpy(),
                        alpha=0.9, inv_norm=1.0 / (2.0 * WS.H * WS.W * B))
    wav_pred = wl["wav"].astype(np.float32)
    cf = DR.closed_form(wav_pred, wav.numpy(), 30.0, weight=0.05, global_batch=B)
    assert cf["loss"] > 0 and wl["loss"] == 0.0
    assert float(dec_eng.loss_out[0]) == float(np.float32(np.float32(plain_eng.loss_out[0]) + np.float32(cf["loss"])))
    assert torch.equal(dec_eng.loss_out[1:3], plain_eng.loss_out[1:3])
    assert abs(float(dec.decay_loss.decay_out[0]) - cf["decay_out"][0]) <= 1e-12 * cf["decay_out"][0]
    # the dpred the backward pass started from: the spectrogram term's, rounded to fp32, plus the decay term's
    vj = DR.vjp_closed_form(dec_eng.pred.numpy(), cf["dwav"].astype(np.float32), *geo)["grad"]
    want = (wl["grad"].astype(np.float32).astype(np.float64) + vj).astype(np.float32)
    assert np.array_equal(dec._wave._dpred.numpy(), want) and np.abs(vj).max() > 0


@pytest.mark.parametrize("kind", ["unet", "ae"])
def test_weight_zero_is_the_trainer_without_the_option(monkeypatch, kind):
    """weight = 0 makes dwav an exact zero, so the accumulate pass adds zeros: the gradients of the step are those of the trainer with
    the same wave_loss and no decay_loss, bit for bit"""
    rt, impl = _install(monkeypatch)
    a_eng, a = _build(rt, kind, False, WS._wave(), None)
    b_eng, b = _build(rt, kind, False, WS._wave(), _decay(weight=0.0))
    spec_in, emb, spec_out, wav = _batch()
    la = a.step(spec_in, emb, spec_out, wav_true=wav, return_loss=True)
    lb = b.step(spec_in, emb, spec_out, wav_true=wav, return_loss=True)
    assert la == lb and torch.equal(a_eng.grad, b_eng.grad) and torch.equal(a_eng.theta, b_eng.theta)
    assert float(b.decay_loss.decay_out[0]) > 0


def test_fit_records_the_decay_term(monkeypatch):
    import unet_rir_amd as U
    import decay_loss_ref as DR
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", False, None, _decay(), lr=0.0)
    spec_in, emb, spec_out, wav = _batch()
    four = (spec_in, emb, spec_out, wav)
    generator_style = (spec_in, emb, spec_out, (torch.zeros(B, dtype=torch.int64), wav))
    rec = U.fit(tr, lambda ep: [four, generator_style], 1, val_batches=lambda ep: [generator_style], log=None)[0]
    cf = DR.closed_form(tr._wave.wav_pred.numpy(), wav.numpy(), 30.0, weight=0.05, global_batch=B)
    want = cf["decay_out"][0] / B                                 # lr = 0, no dropout: every step sees the same prediction
    assert abs(rec["train_decay"] - want) <= 1e-9 * want and abs(rec["val_decay"] - want) <= 1e-9 * want
    assert np.isfinite(rec["train_loss"]) and np.isfinite(rec["val_loss"])
    # the validation pass: the loss alone - no gradient, no vector-Jacobian product
    assert impl.decay.calls == [("decay", B, True), ("vjp", True, False)] * 2 + [("decay", B, False)]
    assert impl.wave.calls == [(B, True, True)] * 2 + [(B, False, False)]
    assert "train_wave" not in rec and "val_wave" not in rec            # the internal WaveLoss of weight 0 is not the user's
    with pytest.raises(ValueError, match="decay_loss"):
        U.fit(tr, lambda ep: [(spec_in, emb, spec_out)], 1, log=None)
    # with a user's wave_loss both pairs are recorded; a silent target is not counted in the mean
    eng2, tr2 = _build(rt, "unet", False, WS._wave(), _decay(), lr=0.0)
    quiet = wav.clone()
    quiet[1] = 0.0
    rec2 = U.fit(tr2, lambda ep: [(spec_in, emb, spec_out, quiet)], 1, log=None)[0]
    cf2 = DR.closed_form(tr2._wave.wav_pred.numpy(), quiet.numpy(), 30.0, weight=0.05, global_batch=B)
    assert {"train_wave", "train_decay"} <= set(rec2) and cf2["decay_out"][1] == 1
    assert abs(rec2["train_decay"] - cf2["decay_out"][0]) <= 1e-9 * cf2["decay_out"][0]


def test_refusals(monkeypatch):
    import unet_rir_amd as U
    import cnn_clas_cpu_ops
    import vae_cpu_ops
    from sim_runtime import SimRuntime
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", False, None, _decay())
    spec_in, emb, spec_out, wav = _batch()
    with pytest.raises(ValueError, match="wav_true"):
        tr.step(spec_in, emb, spec_out)
    with pytest.raises(ValueError, match="geometry"):
        _build(rt, "unet", False, WS._wave(), U.DecayLoss(des_shape=(9, 13), n_fft=16, win_length=16, hop_length=4))
    conv = ((4, 8, 8, 8), (3, 3, 3, 3), (2, 2, 2, 2))
    rt2 = SimRuntime()
    vae_cpu_ops.install(monkeypatch, rt2)
    for make in (lambda: U.VAEEngine(WS.H, WS.W, B, *conv, 8, 16, device="cpu", runtime=rt2),
                 lambda: U.VQVAEEngine(16, 32, B, *conv, 4, 8, device="cpu", runtime=rt2)):
        with pytest.raises(ValueError, match="decay_loss: .* has a loss term or target of its own"):
            U.Trainer(make(), decay_loss=_decay())
    rt3 = SimRuntime()
    cnn_clas_cpu_ops.install(monkeypatch, rt3)
    with pytest.raises(ValueError, match="decay_loss: .* has a loss term or target of its own"):
        U.Trainer(U.DeepCNNEngine(21, 24, 3, classes=5, device="cpu", runtime=rt3), decay_loss=_decay())


def _dp_worker(rank, world, port, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mpatch = pytest.MonkeyPatch()
        rt, impl = _install(mpatch)
        eng, tr = _build(rt, "unet", True, None, _decay(), world=world)
        tr.broadcast_parameters(0)
        spec_in, emb, spec_out, wav = _batch(B * world)
        sl = slice(rank * B, (rank + 1) * B)
        for _ in range(2):
            tr.step(spec_in[sl].contiguous(), emb[sl].contiguous(), spec_out[sl].contiguous(), wav_true=wav[sl].contiguous())
        torch.save({"calls": impl.decay.calls, "theta": eng.theta.clone(), "decay": tr.decay_loss.decay_out.clone()}, f"{out_path}.{rank}")
        mpatch.undo()
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_see_the_global_batch(tmp_path):
    world = 2
    out = str(tmp_path / "dp")
    mp.spawn(_dp_worker, args=(world, 34300 + (os.getpid() % 1500), out), nprocs=world, join=True)
    res = [torch.load(f"{out}.{r}") for r in range(world)]
    for r in range(world):
        assert res[r]["calls"] == [("decay", 2 * B, True), ("vjp", True, False)] * 2
    assert torch.equal(res[0]["theta"], res[1]["theta"]) and not torch.equal(res[0]["decay"], res[1]["decay"])

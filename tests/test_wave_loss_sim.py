"""The PRODUCT's Trainer / fit with a WaveLoss on CPU tensors: only the kernels (tests/cpu_ops.py and tests/wave_loss_cpu_ops.py: fp64
arithmetic from tests/wave_loss_ref.py) and the stream runtime (tests/sim_runtime.py: vector clocks + race check) are stand-ins.
16 x 16 planes, n_fft 16 (9 bins), window 8, hop 4, 13 frames: T = 48.  A missing happens-before edge would raise RaceError."""
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

H = W = SS.H
B = 2
GEO = dict(des_shape=(9, 13), n_fft=16, win_length=8, hop_length=4)
T = 48
LR, N_STEPS = 1e-3, 2
P_ATOL = 0.02 * LR * N_STEPS          # the bound of tests/test_schedule_sim.py: Adam turns the rounding of a near-zero entry into a share of lr


def _install(monkeypatch):
    import wave_loss_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    return rt, wave_loss_cpu_ops.install(monkeypatch, rt)


def _batch(n=B, rank=0):
    from oracle import torch_ref as R
    spec_in, emb, spec_out = R.synthetic_batch(R.Config(H, W), n)
    wav = (np.random.RandomState(40 + rank).standard_normal((n, T)) * 0.5).astype(np.float32)
    return tuple(torch.tensor(a) for a in (spec_in, emb, spec_out, wav))


def _build(rt, kind, overlap, wave, world=1, lr=LR, **kw):
    import unet_rir_amd as U
    cfg, eng, _ = SS._build(rt, B, overlap, world=world, bucket_bytes=8192, kind=kind)
    return eng, U.Trainer(eng, lr=lr, dropout=False, world_size=world, bucket_bytes=8192, wave_loss=wave, **kw)


def _wave(weight=0.3, norm="energy", **kw):
    import unet_rir_amd as U
    return U.WaveLoss(weight=weight, norm=norm, **GEO, **kw)


@pytest.mark.parametrize("kind,overlap", [("unet", False), ("unet", True), ("ae", False), ("ae", True)])
def test_step_is_race_free_and_the_call_sits_between_loss_and_backward(monkeypatch, kind, overlap):
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, kind, overlap, _wave(time_weight=np.linspace(1.0, 0.0, T)))
    log, touch = [], rt.touch

    def logged(reads=(), writes=(), what="", stream=None):
        log.append(what)
        return touch(reads, writes, what, stream)
    monkeypatch.setattr(rt, "touch", logged)
    spec_in, emb, spec_out, wav = _batch()
    before = eng.theta.clone()
    for _ in range(2):
        tr.step(spec_in, emb, spec_out, wav_true=wav)          # a RaceError here: an unordered cross-stream access
    assert impl.wave.calls == [(B, True, True)] * 2 and bool(torch.isfinite(eng.theta).all()) and not torch.equal(eng.theta, before)
    i = log.index("wave_loss")
    assert log[i + 1] == "sigmoid_bwd" and "sigmoid_loss" in log[:i]
    assert not [w for w in log[:i] if "wgrad" in w or "dgrad" in w or w.endswith("_bwd")]       # no backward launch before it
    if overlap:
        assert rt.n_cross_stream > 50
    else:
        assert rt.n_cross_stream == 0


@pytest.mark.parametrize("kind", ["unet", "ae"])
def test_weight_zero_is_the_plain_trainer(monkeypatch, kind):
    """With weight = 0 the backward pass starts from dpred = the spectrogram loss's dL/dpred, rounded to fp32, times p (1 - p) -
    against the loss kernel's dL/dlogits formed in one piece: one extra fp32 rounding per element of dlogits (2^-24 relative), which
    the weight gradients pass on linearly.  Gradients are held to 1e-6 (2^-24 with a cancellation factor of 16 in the sums) of their
    tensor's largest entry plus the largest entry of all - the floor of tests/test_schedule_sim.py for tensors whose exact gradient
    is ~0 behind a 2-sample BatchNorm - and parameters to P_ATOL.  Measured on the CPU with these stand-ins, after
    the bounds were written: the largest gradient gap is 7.3e-8 of that scale ("unet") and 1.5e-7 ("ae"), the largest parameter gap
    1.2e-7 and 4.7e-7 (P_ATOL = 4e-5)."""
    rt, impl = _install(monkeypatch)
    plain_eng, plain = _build(rt, kind, False, None)
    wave_eng, wave = _build(rt, kind, False, _wave(weight=0.0))
    spec_in, emb, spec_out, wav = _batch()
    worst_g = worst_p = 0.0
    for t in range(N_STEPS):
        lp = plain.step(spec_in, emb, spec_out, return_loss=True)
        lw = wave.step(spec_in, emb, spec_out, wav_true=wav, return_loss=True)
        if t == 0:
            assert lp == lw                                      # the same forward pass, and a term of exactly 0
            gp, gw = plain_eng.export_keras_grads(), wave_eng.export_keras_grads()
            largest = max(float(g.abs().max()) for g in gp.values())
            for n, g in gp.items():
                top = float(g.abs().max())
                gap = float((gw[n] - g).abs().max())
                worst_g = max(worst_g, gap / (top + largest))
                assert gap <= 1e-6 * (top + largest), (n, gap, top)
    pp, pw = plain_eng.export_keras_params(), wave_eng.export_keras_params()
    for n, p in pp.items():
        worst_p = max(worst_p, float((pw[n] - p).abs().max()))
        assert float((pw[n] - p).abs().max()) <= P_ATOL, n
    print(f"{kind}: largest gradient gap {worst_g:.2e} of its scale, largest parameter gap {worst_p:.2e}")


def test_loss_out_grows_by_exactly_the_wave_term(monkeypatch):
    import wave_loss_ref as WR
    rt, impl = _install(monkeypatch)
    plain_eng, plain = _build(rt, "unet", False, None, lr=0.0)
    wave_eng, wave = _build(rt, "unet", False, _wave(weight=0.3, norm="mse"), lr=0.0)
    spec_in, emb, spec_out, wav = _batch()
    plain.step(spec_in, emb, spec_out)
    wave.step(spec_in, emb, spec_out, wav_true=wav)
    assert torch.equal(plain_eng.pred, wave_eng.pred)
    cf = WR.closed_form(wave_eng.pred.numpy(), wav.numpy(), GEO["des_shape"], 16, 8, 4, norm="mse", weight=0.3, global_batch=B)
    assert cf["loss"] > 0
    assert float(wave_eng.loss_out[0]) == float(np.float32(np.float32(plain_eng.loss_out[0]) + np.float32(cf["loss"])))
    assert torch.equal(wave_eng.loss_out[1:3], plain_eng.loss_out[1:3])
    assert abs(float(wave.wave_loss.wave_out[0]) - cf["wave_out"][0]) <= 1e-12 * cf["wave_out"][0]


def test_fit_records_the_wave_term_and_takes_both_tuple_shapes(monkeypatch):
    import unet_rir_amd as U
    import wave_loss_ref as WR
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", False, _wave(weight=0.3), lr=0.0)
    spec_in, emb, spec_out, wav = _batch()
    four = (spec_in, emb, spec_out, wav)
    generator_style = (spec_in, emb, spec_out, (torch.zeros(B, dtype=torch.int64), wav))
    rec = U.fit(tr, lambda ep: [four, generator_style], 1, val_batches=lambda ep: [generator_style], log=None)[0]
    cf = WR.closed_form(eng.pred.numpy(), wav.numpy(), GEO["des_shape"], 16, 8, 4, norm="energy", weight=0.3, global_batch=B)
    want = cf["wave_out"][0] / B                                  # lr = 0, no dropout: every step sees the same prediction
    assert abs(rec["train_wave"] - want) <= 1e-9 * want and abs(rec["val_wave"] - want) <= 1e-9 * want
    assert np.isfinite(rec["train_loss"]) and np.isfinite(rec["val_loss"])
    assert impl.wave.calls == [(B, True, True), (B, True, True), (B, False, False)]      # the validation pass: the loss alone
    with pytest.raises(ValueError):
        U.fit(tr, lambda ep: [(spec_in, emb, spec_out)], 1, log=None)
    # three-tuples without a wave_loss: the record as it was
    eng0, tr0 = _build(rt, "unet", False, None, lr=0.0)
    rec0 = U.fit(tr0, lambda ep: [(spec_in, emb, spec_out)], 1, val_batches=lambda ep: [(spec_in, emb, spec_out)], log=None)[0]
    assert set(rec0) == {"epoch", "lr", "train_loss", "train_amp", "train_phase", "val_loss", "val_amp", "val_phase"}
    assert set(rec) == set(rec0) | {"train_wave", "val_wave"}


def test_refusals(monkeypatch):
    import unet_rir_amd as U
    import cnn_clas_cpu_ops
    import vae_cpu_ops
    from sim_runtime import SimRuntime
    rt, impl = _install(monkeypatch)
    eng, tr = _build(rt, "unet", False, _wave())
    spec_in, emb, spec_out, wav = _batch()
    with pytest.raises(ValueError, match="wav_true"):
        tr.step(spec_in, emb, spec_out)
    conv = ((4, 8, 8, 8), (3, 3, 3, 3), (2, 2, 2, 2))
    rt2 = SimRuntime()
    vae_cpu_ops.install(monkeypatch, rt2)
    for make in (lambda: U.VAEEngine(H, W, B, *conv, 8, 16, device="cpu", runtime=rt2),
                 lambda: U.VQVAEEngine(16, 32, B, *conv, 4, 8, device="cpu", runtime=rt2)):
        with pytest.raises(ValueError, match="wave_loss"):
            U.Trainer(make(), wave_loss=_wave())
    rt3 = SimRuntime()
    cnn_clas_cpu_ops.install(monkeypatch, rt3)
    with pytest.raises(ValueError, match="wave_loss"):
        U.Trainer(U.DeepCNNEngine(21, 24, 3, classes=5, device="cpu", runtime=rt3), wave_loss=_wave())


def _dp_worker(rank, world, port, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mpatch = pytest.MonkeyPatch()
        rt, impl = _install(mpatch)
        eng, tr = _build(rt, "unet", True, _wave(), world=world)
        tr.broadcast_parameters(0)
        spec_in, emb, spec_out, wav = _batch(B * world)
        sl = slice(rank * B, (rank + 1) * B)
        for _ in range(2):
            tr.step(spec_in[sl].contiguous(), emb[sl].contiguous(), spec_out[sl].contiguous(), wav_true=wav[sl].contiguous())
        torch.save({"calls": impl.wave.calls, "theta": eng.theta.clone(), "wave": tr.wave_loss.wave_out.clone()}, f"{out_path}.{rank}")
        mpatch.undo()
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_see_the_global_batch(tmp_path):
    world = 2
    out = str(tmp_path / "dp")
    mp.spawn(_dp_worker, args=(world, 32700 + (os.getpid() % 1500), out), nprocs=world, join=True)
    res = [torch.load(f"{out}.{r}") for r in range(world)]
    for r in range(world):
        assert res[r]["calls"] == [(2 * B, True, True)] * 2
    assert torch.equal(res[0]["theta"], res[1]["theta"]) and not torch.equal(res[0]["wave"], res[1]["wave"])

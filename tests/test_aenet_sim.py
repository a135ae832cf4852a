"""The PRODUCT's AENetEngine + Trainer + fit on CPU tensors: only the kernels (tests/aenet_cpu_ops.py: fp64 arithmetic) and the stream
runtime (tests/sim_runtime.py: vector clocks + race check) are stand-ins.  32 x 48, number_filters_0 = 4, batch 2, against
tests/aenet_ref.py at the tolerances of tests/test_vqvae_sim.py (fp32 buffers, fp64 arithmetic); a missing happens-before edge
would raise RaceError."""
import numpy as np
import pytest
import torch

H, W, B, F0 = 32, 48, 2, 4
LR, N_STEPS = 1e-3, 2
P_ATOL = 0.02 * LR * N_STEPS


def _install(monkeypatch, passes=7):
    import aenet_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    return rt, aenet_cpu_ops.install(monkeypatch, rt, passes)


def _masks(rank=0):
    rs = np.random.RandomState(100 + rank)
    return tuple(((rs.uniform(size=(B, n)) >= 0.5) / 0.5).astype(np.float32) for n in (2048, (H // 16) * (W // 16) * 2))


def _setup(mode, batchnorm, world=1, f0=F0):
    import aenet_ref as A
    from oracle import torch_ref as R
    cfg = A.config(H, W, f0, mode, batchnorm)
    return cfg, A.init_params(cfg, f"sim{mode}{batchnorm}"), R.synthetic_batch(cfg, B * world, "sim/d")


def _build(rt, cfg, params, overlap, world=1, dtype="f32", dropout=False, lr=LR, share=None, batch=B):
    import unet_rir_amd as U
    eng = U.AENetEngine(H, W, batch, F0=cfg.F0, mode=cfg.mode, batchnorm=cfg.batchnorm, device="cpu", runtime=rt, n_replicas=world,
                        overlap_wgrad=overlap, dtype=dtype, share=share)
    if share is None:
        eng.load_keras_params(params)
    return eng, U.Trainer(eng, lr=lr, dropout=dropout, world_size=world, bucket_bytes=8192)


@pytest.mark.parametrize("mode,batchnorm,overlap", [(0, True, False), (0, True, True), (3, True, True), (0, False, False), (3, False, False)])
def test_step_on_the_product_schedule_matches_aenet_ref(monkeypatch, mode, batchnorm, overlap):
    import aenet_ref as A
    from oracle import torch_ref as R
    rt, impl = _install(monkeypatch)
    cfg, params, batch = _setup(mode, batchnorm)
    eng, tr = _build(rt, cfg, params, overlap)
    assert {n: tuple(s.keras_shape) for n, s in eng.specs.items()} == A.param_shapes(cfg)
    assert set(eng.l2_names) == set(A.l2_regularized(cfg)) and eng.n_dropout_draws == 2 and eng.dropout_p == 0.5
    masks = _masks()
    tb = tuple(torch.tensor(a) for a in batch)
    tm = tuple(torch.tensor(m).view(B, 1, 1, -1) for m in masks)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    m = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}
    v_ = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}
    for t in range(1, N_STEPS + 1):
        loss, data, pred, z, grads = A.loss_and_grads(p64, *batch, cfg, masks)
        got = tr.step(*tb, dropout_mask=tm, return_loss=True)
        assert abs(got - loss) <= 1e-5 * abs(loss), (t, got, loss)
        # fp32 buffers: every stored tensor is rounded to 2^-24 relative; about 40 of them lie between the input and the logits, whose
        # magnitude reaches ~10 here, and the clipped ReLU passes a logit's error on unscaled (a sigmoid would quarter it):
        # 40 * 2^-24 * 10 = 2.4e-5
        assert float((eng.pred.double() - pred).abs().max()) <= 2.4e-5
        if t == 1:
            got_g = eng.export_keras_grads()
            floor = 1e-6 * max(float(g.abs().max()) for g in grads.values())
            for n, g in grads.items():
                e = float((got_g[n].double() - g).abs().max())
                assert e <= 1e-4 * float(g.abs().max()) + floor, (n, e)
            for n in () if not batchnorm else ("enc3.down.kernel",          # (without BatchNorm this random net lets little through)
                                                "dec2.up.kernel", "vec.embedding", "vec.dense.kernel", "rec.dense.kernel", "rec.conv.kernel", "head.kernel"):
                assert float(grads[n].abs().max()) > 0, n
        for k in p64:
            new, m[k], v_[k] = R.adam_update(torch.tensor(p64[k]), grads[k], m[k], v_[k], t, LR)
            p64[k] = new.numpy()
    got = eng.export_keras_params()
    for n, w in p64.items():
        assert float(np.abs(got[n].double().numpy() - w).max()) <= P_ATOL, n
    assert impl.aenet.calls == {} and (rt.n_cross_stream > 50 if overlap else rt.n_cross_stream == 0)


def test_bf16_trunk_takes_the_conv2x2_branches_the_predicate_offers(monkeypatch):
    """With a bf16 trunk the `_conv2x2` nodes run the passes conv2x2s2_supported offers on the new entry points and the others on the
    generic ones; the stand-ins compute the same numbers either way, so the three runs (all passes, the weight gradient alone,
    none) end in the same loss and the same gradients."""
    results = []
    for passes in (7, 4, 0):
        with pytest.MonkeyPatch.context() as mp:
            rt, impl = _install(mp, passes)
            cfg, params, batch = _setup(0, True, f0=8)                 # a bf16 trunk stores 8 channels at least
            eng, tr = _build(rt, cfg, params, True, dtype="bf16", lr=0.0)
            assert set(eng.c22_passes) == {f"enc{l}.down" for l in range(2, 6)} | {f"dec{l}.up" for l in range(1, 5)}
            assert set(eng.c22_passes.values()) == {passes}
            loss = tr.step(*(torch.tensor(a) for a in batch), dropout_mask=tuple(torch.tensor(m).view(B, 1, 1, -1) for m in _masks()),
                           return_loss=True)
            want = {}
            if passes & 1:
                want.update(fwd=4, tfwd=4)
            if passes & 2:
                want.update(dgrad=4, tdgrad=4)
            if passes & 4:
                want.update(wgrad=4, twgrad=4)
            assert impl.aenet.calls == want and np.isfinite(loss)
            results.append((loss, {k: v.clone() for k, v in eng.export_keras_grads().items()}))
    for loss, grads in results[1:]:
        assert loss == results[0][0]
        for n, g in grads.items():
            assert torch.equal(g, results[0][1][n]), n


def test_module_class_round_trips_save_and_load(monkeypatch, tmp_path):
    """unet_rir_amd.AENet on the simulated runtime: the reference's constructor, parameters.pkl as ae_net.py:176-183 writes it (then
    this build's dtype), and a loaded model that predicts what the saved one did."""
    import pickle
    import unet_rir_amd as U
    rt, impl = _install(monkeypatch)
    cfg, params, batch = _setup(3, True)
    model = U.AENet((H, W, 2), (2, 16), mode=3, number_filters_0=F0, batch_size=B, device="cpu", runtime=rt, dropout=False)
    assert isinstance(model.engine, U.AENetEngine) and model.name == "AENet" and model.learning_rate == 1e-5
    model.engine.load_keras_params(params)
    x = [torch.tensor(batch[0]).permute(0, 2, 3, 1).contiguous(), torch.tensor(batch[1])]
    a = model.predict_stft(x).clone()
    assert tuple(a.shape) == (B, H, W, 2) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    model.save(str(tmp_path))
    with open(tmp_path / "parameters.pkl", "rb") as f:
        assert pickle.load(f) == [(H, W, 2), (2, 16), 1e-5, 3, F0, True, "f32"]
    again = U.AENet.load(str(tmp_path), batch_size=B, device="cpu", runtime=rt)
    assert again.mode == 3 and again.number_filters_0 == F0 and torch.equal(again.engine.theta, model.engine.theta)
    assert torch.equal(again.predict_stft(x), a)
    assert len(model.model.losses) == 9 and len(list(model.model.trainable_variables)) == len(model.engine.specs)


@pytest.mark.parametrize("dropout", [False, True])
def test_two_dropout_draws_per_step(monkeypatch, dropout):
    rt, impl = _install(monkeypatch)
    cfg, params, batch = _setup(0, True)
    eng, tr = _build(rt, cfg, params, False, dropout=dropout, lr=0.0)
    tb = tuple(torch.tensor(a) for a in batch)
    for _ in range(3):
        tr.step(*tb)
    assert eng._shared["dropout_step"] == (6 if dropout else 0)
    assert (eng.masks["vec"] is not None) == dropout and (eng.masks["rec"] is not None) == dropout
    if dropout:
        assert eng.mask_width == {"vec": 2048, "rec": 12}
        assert set(torch.unique(eng.masks["vec"]).tolist()) == {0.0, 2.0}            # Dropout(.5): keep scaled by 1 / (1 - 0.5)


def test_existing_engines_keep_their_dropout_masks(monkeypatch):
    """The rate became an engine attribute.  What could regress is the rate an existing engine's launch carries: it is still the
    literal 0.3, and the mask the stand-in generator makes from it is (u >= 0.3) / 0.7 on its stream, computed here with the literal
    (not a recording made on the device before the change: the HIP generator itself is held by the existing GPU dropout tests,
    which pass unchanged)."""
    import unet_rir_amd as U
    rt, impl = _install(monkeypatch)
    seen = []
    real = U.ops.dropout_mask
    monkeypatch.setattr(U.ops, "dropout_mask", lambda mask, p, seed, step: (seen.append(p), real(mask, p, seed, step))[1])
    eng = U.UNetGraphEngine(32, 32, 2, F0=4, k=3, mode=1, device="cpu", runtime=rt)
    eng.dropout_seed = 9
    m = eng.make_dropout_mask().clone()
    gen = torch.Generator().manual_seed(9 * 1000003 + 0)
    assert torch.equal(m, (torch.rand(m.shape, generator=gen) >= 0.3).float() / (1.0 - 0.3)) and seen == [0.3]
    assert U.UNetEngine.dropout_p == 0.3 and U.VQVAEEngine.dropout_p == 0.3 and U.AENetEngine.dropout_p == 0.5


def test_two_replicas_share_and_fit(monkeypatch):
    import unet_rir_amd as U
    import aenet_ref as A
    rt, impl = _install(monkeypatch)
    cfg, params, batch = _setup(0, True)
    eng, tr = _build(rt, cfg, params, True, world=2, lr=0.0)
    tb = tuple(torch.tensor(a[:B]) for a in batch)
    masks = _masks()
    loss = tr.step(*tb, dropout_mask=tuple(torch.tensor(m).view(B, 1, 1, -1) for m in masks), return_loss=True)
    # replica 0 of 2: data loss over the global batch 2 B, l2 terms / 2 (main_training.py:232-233)
    P = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in params.items()}
    pred = A.forward(P, torch.tensor(batch[0][:B], dtype=torch.float64), torch.tensor(batch[1][:B]), cfg,
                     masks=tuple(torch.tensor(m, dtype=torch.float64) for m in masks))
    from oracle import torch_ref as R
    want = float(R.data_loss(torch.tensor(batch[2][:B], dtype=torch.float64), pred, 0.9, 2 * B) + A.reg_loss(P, cfg, 2))
    assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)
    other, _ = _build(rt, cfg, params, True, share=eng, batch=3)
    assert other.theta.data_ptr() == eng.theta.data_ptr() and other.p["rec.dense.kernel"].data_ptr() == eng.p["rec.dense.kernel"].data_ptr()
    eng1, tr1 = _build(rt, cfg, params, False, lr=0.0)
    hist = U.fit(tr1, lambda ep: [tb, tb], 1, val_batches=lambda ep: [tb], log=None)
    assert np.isfinite(hist[0]["train_loss"]) and np.isfinite(hist[0]["val_loss"])

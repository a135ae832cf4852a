"""The PRODUCT's DiffUNetEngine / DiffVAEEngine + Trainer + fit on CPU tensors: only the kernels (tests/diff_cpu_ops.py over
aenet_cpu_ops / vae_cpu_ops: fp64 arithmetic) and the stream runtime (tests/sim_runtime.py: vector clocks + race check) are stand-ins.
Against tests/diffunet_ref.py / tests/diffvae_ref.py at the tolerances of tests/test_aenet_sim.py / tests/test_vae_sim.py (fp32
buffers, fp64 arithmetic): loss 1e-5 relative, gradients 1e-4 of the tensor's largest entry, parameters 2 % of the distance Adam can
have moved them; a missing happens-before edge would raise RaceError.  Both models are driven with diff_loss=True, the loss they
exist for (main_training.py:214-217)."""
import hashlib
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

H, W, B, F0 = 32, 48, 2, 4
LR, N_STEPS = 1e-3, 2
P_ATOL = 0.02 * LR * N_STEPS


def _install(monkeypatch, family="unet", head_passes=3, c22_passes=7):
    import diff_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    return rt, diff_cpu_ops.install(monkeypatch, rt, family, head_passes, c22_passes)


# ------------------------------------------------------------------------------------------------ DiffUNet
def _mask(cfg, rank=0):
    import diffunet_ref as DU
    return ((np.random.RandomState(100 + rank).uniform(size=(B, DU.vec_units(cfg))) >= 0.5) / 0.5).astype(np.float32)


def _setup(mode, batchnorm, world=1, f0=F0):
    import diffunet_ref as DU
    from oracle import torch_ref as R
    cfg = DU.config(H, W, f0, mode, batchnorm)
    return cfg, DU.init_params(cfg, f"sim{mode}{batchnorm}"), R.synthetic_batch(cfg, B * world, "sim/d")


def _build(rt, cfg, params, overlap, world=1, dtype="f32", dropout=False, lr=LR, share=None, batch=B, **kw):
    import unet_rir_amd as U
    eng = U.DiffUNetEngine(H, W, batch, F0=cfg.F0, mode=cfg.mode, batchnorm=cfg.batchnorm, device="cpu", runtime=rt, n_replicas=world,
                           overlap_wgrad=overlap, dtype=dtype, share=share, **kw)
    if share is None:
        eng.load_keras_params(params)
    return eng, U.Trainer(eng, lr=lr, dropout=dropout, world_size=world, bucket_bytes=8192, diff_loss=True)


@pytest.mark.parametrize("mode,batchnorm,overlap", [(0, True, False), (0, True, True), (3, True, True), (0, False, False), (3, False, True)])
def test_diffunet_step_on_the_product_schedule_matches_the_restatement(monkeypatch, mode, batchnorm, overlap):
    import diffunet_ref as DU
    from oracle import torch_ref as R
    rt, impl = _install(monkeypatch)
    cfg, params, batch = _setup(mode, batchnorm)
    eng, tr = _build(rt, cfg, params, overlap)
    assert {n: tuple(s.keras_shape) for n, s in eng.specs.items()} == DU.param_shapes(cfg)
    assert eng.specs["head.kernel"].kind == "conv_padout" and eng.output_act == "linear" and eng.head_passes == 0      # fp32 trunk: generic
    assert set(eng.l2_names) == set(DU.l2_regularized(cfg)) and eng.n_dropout_draws == 1 and eng.dropout_p == 0.5 and eng.MASKS == ("vec",)
    mask = _mask(cfg)
    tb = tuple(torch.tensor(a) for a in batch)
    tm = torch.tensor(mask).view(B, 1, 1, -1)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    m = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}
    v_ = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}
    for t in range(1, N_STEPS + 1):
        loss, data, pred, z, grads = DU.loss_and_grads(p64, *batch, cfg, (mask,), diff_loss=True)
        got = tr.step(*tb, dropout_mask=tm, return_loss=True)
        assert abs(got - loss) <= 1e-5 * abs(loss), (t, got, loss)
        # fp32 buffers: every stored tensor is rounded to 2^-24 relative; about 40 of them lie between the input and the logits, whose
        # magnitude reaches ~10 here, and the linear output passes a logit's error on unscaled: 40 * 2^-24 * 10 = 2.4e-5
        assert float((eng.pred.double() - pred).abs().max()) <= 2.4e-5
        if t == 1:
            assert float(((pred < 0) | (pred > 1)).double().mean()) > 0.05          # the linear output is exercised
            got_g = eng.export_keras_grads()
            floor = 1e-6 * max(float(g.abs().max()) for g in grads.values())
            for n, g in grads.items():
                e = float((got_g[n].double() - g).abs().max())
                assert e <= 1e-4 * float(g.abs().max()) + floor, (n, e)
            for n in () if not batchnorm else ("enc3.down.kernel", "dec2.up.kernel", "vec.embedding", "encoder_inf_dense.kernel", "head.kernel",
                                                "head.bias"):
                assert float(grads[n].abs().max()) > 0, n
        for k in p64:
            new, m[k], v_[k] = R.adam_update(torch.tensor(p64[k]), grads[k], m[k], v_[k], t, LR)
            p64[k] = new.numpy()
    got = eng.export_keras_params()
    for n, w in p64.items():
        assert float(np.abs(got[n].double().numpy() - w).max()) <= P_ATOL, n
    assert impl.aenet.calls == {} and impl.diff.calls == {} and (rt.n_cross_stream > 50 if overlap else rt.n_cross_stream == 0)


def test_bf16_trunk_takes_the_head1x1_branches_the_predicate_offers(monkeypatch):
    """With a bf16 trunk the `_head1x1` node runs the passes head1x1_supported offers on the new entry points and the others on the
    generic ones.  The stand-ins compute the same numbers either way - up to the forward pass's storage: the generic kernels store bf16
    logits - so the runs with one forward path end in the same loss and gradients."""
    results = {}
    for passes in (3, 2, 1, 0, "generic"):
        with pytest.MonkeyPatch.context() as mpatch:
            rt, impl = _install(mpatch, head_passes=3 if passes == "generic" else passes)
            cfg, params, batch = _setup(0, True, f0=8)                 # a bf16 trunk stores 8 channels at least
            eng, tr = _build(rt, cfg, params, True, dtype="bf16", lr=0.0, generic_head=(passes == "generic"))
            want_mask = 0 if passes == "generic" else passes
            assert eng.head_passes == want_mask and eng.logits.a.sfx == ("f32" if want_mask & 1 else "bf16") and eng.logits.g.sfx == "bf16"
            assert tuple(eng.specs["head.kernel"].shape) == (8, 1, 1, 8) and set(eng.c22_passes.values()) == {7}
            loss = tr.step(*(torch.tensor(a) for a in batch), dropout_mask=torch.tensor(_mask(cfg)).view(B, 1, 1, -1), return_loss=True)
            want = {}
            if want_mask & 1:
                want["fwd"] = 1
            if want_mask & 2:
                want["bwd"] = 1
            assert impl.diff.calls == want and np.isfinite(loss)
            results[passes] = (loss, {k: v.clone() for k, v in eng.export_keras_grads().items()})
    for a, b in ((3, 1), (2, 0), (0, "generic")):
        assert results[a][0] == results[b][0]
        for n, g in results[a][1].items():
            assert torch.equal(g, results[b][1][n]), (a, b, n)
    assert abs(results[3][0] - results[0][0]) <= 1e-2 * abs(results[3][0])


def test_diffunet_module_surface(monkeypatch, tmp_path):
    """unet_rir_amd.DiffUNet on the simulated runtime: the reference's constructor (dl_models/diff_u_net.py:40-45), parameters.pkl as
    :179-186 writes it (then this build's dtype), a loaded model that predicts what the saved one did, compile_and_fit (:82-83)."""
    import inspect
    import pickle
    import unet_rir_amd as U
    sig = inspect.signature(U.DiffUNet.__init__)
    assert list(sig.parameters)[1:10] == ["input_shape", "inf_vector_shape", "learning_rate", "mode", "number_filters_0", "BatchNorm",
                                          "resize_factor_0", "res_factor", "name"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["learning_rate"], d["mode"], d["number_filters_0"], d["BatchNorm"], d["resize_factor_0"], d["res_factor"], d["name"]) == \
        (1e-5, 0, 32, True, None, None, "U-Net")
    assert list(inspect.signature(U.DiffUNet.compile_and_fit).parameters)[1:] == ["x_train1", "x_train2", "y_train", "x_val1", "x_val2", "y_val",
                                                                                  "batch_size", "num_epochs", "steps_per_epoch"]
    rt, impl = _install(monkeypatch)
    cfg, params, batch = _setup(3, True)
    model = U.DiffUNet((H, W, 2), (2, 16), mode=3, number_filters_0=F0, batch_size=B, device="cpu", runtime=rt, dropout=False)
    assert isinstance(model.engine, U.DiffUNetEngine) and model.name == "U-Net" and model.learning_rate == 1e-5
    with pytest.raises(ValueError, match="multiples of 16"):
        U.DiffUNetEngine(40, 48, B, F0=4, device="cpu", runtime=rt)
    model.engine.load_keras_params(params)
    x = [torch.tensor(batch[0]).permute(0, 2, 3, 1).contiguous(), torch.tensor(batch[1])]
    a = model.predict_stft(x).clone()
    assert tuple(a.shape) == (B, H, W, 2) and (float(a.min()) < 0.0 or float(a.max()) > 1.0)
    model.save(str(tmp_path))
    with open(tmp_path / "parameters.pkl", "rb") as f:
        assert pickle.load(f) == [(H, W, 2), (2, 16), 1e-5, 3, F0, True, "f32"]
    again = U.DiffUNet.load(str(tmp_path), batch_size=B, device="cpu", runtime=rt)
    assert isinstance(again, U.DiffUNet) and again.mode == 3 and again.number_filters_0 == F0 and torch.equal(again.engine.theta, model.engine.theta)
    assert torch.equal(again.predict_stft(x), a)
    assert len(model.model.losses) == 9 and len(list(model.model.trainable_variables)) == len(model.engine.specs)
    monkeypatch.chdir(tmp_path)                                   # get_callbacks writes `U-Net.log`
    nhwc = lambda t: np.asarray(t).transpose(0, 2, 3, 1)
    hist = model.compile_and_fit(nhwc(batch[0]), batch[1], nhwc(batch[2]), nhwc(batch[0]), batch[1], nhwc(batch[2]), B, 2, 1)
    assert len(hist["loss"]) == 2 and len(hist["val_loss"]) == 2 and all(np.isfinite(v) for v in hist["loss"] + hist["val_loss"])
    assert not torch.equal(again.engine.theta, model.engine.theta)             # MSE through the autograd bridge (linear_bwd) trained it


def test_one_dropout_draw_per_step_and_fit(monkeypatch):
    import unet_rir_amd as U
    rt, impl = _install(monkeypatch)
    cfg, params, batch = _setup(0, True)
    eng, tr = _build(rt, cfg, params, False, dropout=True, lr=0.0)
    tb = tuple(torch.tensor(a) for a in batch)
    for _ in range(3):
        tr.step(*tb)
    assert eng._shared["dropout_step"] == 3 and eng.mask_width == {"vec": 2 * 3 * 64}
    assert set(torch.unique(eng.masks["vec"]).tolist()) == {0.0, 2.0}            # Dropout(.5): keep scaled by 1 / (1 - 0.5)
    other, _ = _build(rt, cfg, params, True, share=eng, batch=3)
    assert other.theta.data_ptr() == eng.theta.data_ptr()
    eng1, tr1 = _build(rt, cfg, params, False, lr=0.0)
    hist = U.fit(tr1, lambda ep: [tb, tb], 1, val_batches=lambda ep: [tb], log=None)
    assert np.isfinite(hist[0]["train_loss"]) and np.isfinite(hist[0]["val_loss"]) and "train_kl" not in hist[0]


def _unet_dp_worker(rank, world, port, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mpatch = pytest.MonkeyPatch()
        rt, impl = _install(mpatch)
        cfg, params, batch = _setup(0, True, world)
        eng, tr = _build(rt, cfg, params, True, world=world)
        if rank != 0:
            eng.theta.mul_(0.5)
        tr.broadcast_parameters(0)
        sl = slice(rank * B, (rank + 1) * B)
        t = torch.tensor
        losses = [tr.step(t(batch[0][sl]), t(batch[1][sl]), t(batch[2][sl]), dropout_mask=t(_mask(cfg, rank)).view(B, 1, 1, -1), return_loss=True)
                  for _ in range(N_STEPS)]
        lt = torch.tensor(losses, dtype=torch.float64)
        dist.all_reduce(lt)
        torch.save({"params": {k: v.double() for k, v in eng.export_keras_params().items()}, "losses": lt}, f"{out_path}.{rank}")
        mpatch.undo()
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_diffunet_two_gloo_ranks(tmp_path):
    import diffunet_ref as DU
    from oracle import torch_ref as R
    world = 2
    out = str(tmp_path / "udp")
    mp.spawn(_unet_dp_worker, args=(world, 34300 + (os.getpid() % 1500), out), nprocs=world, join=True)
    cfg, params, batch = _setup(0, True, world)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    m = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}
    v_ = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}
    want_l = []
    for t in range(1, N_STEPS + 1):
        total, tl = None, 0.0
        for r in range(world):
            sl = slice(r * B, (r + 1) * B)
            P = R.to_torch(p64, torch.float64, True)
            x = torch.tensor(batch[0][sl], dtype=torch.float64)
            z = DU.logits(P, x, torch.tensor(batch[1][sl]), cfg, masks=(torch.tensor(_mask(cfg, r), dtype=torch.float64),))
            # per replica: data loss over the GLOBAL batch, l2 terms / replicas (main_training.py:232-233)
            loss = R.data_loss(torch.tensor(batch[2][sl], dtype=torch.float64), z, 0.9, B * world, x_in=x) + DU.reg_loss(P, cfg, world)
            loss.backward()
            g = {n: p.grad.detach() for n, p in P.items()}
            total = g if total is None else {k: total[k] + g[k] for k in g}
            tl += float(loss.detach())
        want_l.append(tl)
        for k in p64:
            new, m[k], v_[k] = R.adam_update(torch.tensor(p64[k]), total[k], m[k], v_[k], t, LR)
            p64[k] = new.numpy()
    res = [torch.load(f"{out}.{r}") for r in range(world)]
    for r in range(world):
        np.testing.assert_allclose(res[r]["losses"].numpy(), np.array(want_l), rtol=1e-5)
        for n, wp in p64.items():
            assert float(np.abs(res[r]["params"][n].numpy() - wp).max()) <= P_ATOL, (r, n)
    for n in p64:
        assert torch.equal(res[0]["params"][n], res[1]["params"][n]), n


# ------------------------------------------------------------------------------------------------ DiffVAE
VH, VW = 16, 32


def _vcfg():
    import diffvae_ref as DV
    return DV.config(VH, VW, (4, 8, 8, 8), (3, 3, 3, 3), (2, 2, 2, 2), 8, 16)


def _vinputs(rank=0):
    cfg = _vcfg()
    rng = np.random.RandomState(100 + rank)
    eps = rng.standard_normal((B, cfg.latent_space_dim)).astype(np.float32)
    h, w, c = cfg.bottleneck_shape()
    return eps, ((rng.uniform(size=(B, h * w * c)) >= 0.3) / 0.7).astype(np.float32)


def _vbatch(world=1):
    import diffvae_ref as DV
    from oracle import torch_ref as R
    spec_in, emb, spec_out = R.synthetic_batch(R.Config(VH, VW), B * world)
    return spec_in, emb % DV.VOCAB, spec_out


def _vbuild(rt, overlap, world=1, dropout=False, lr=LR, dtype="f32"):
    import unet_rir_amd as U
    import diffvae_ref as DV
    cfg = _vcfg()
    params = DV.init_params(cfg, randomize_all=True, dtype=np.float64)
    eng = U.DiffVAEEngine(VH, VW, B, cfg.conv_filters, cfg.conv_kernels, cfg.conv_strides, cfg.latent_space_dim, cfg.n_neurons,
                          device="cpu", runtime=rt, n_replicas=world, overlap_wgrad=overlap, dtype=dtype)
    eng.load_keras_params(params)
    return cfg, params, eng, U.Trainer(eng, lr=lr, dropout=dropout, world_size=world, bucket_bytes=8192, diff_loss=True)


def _vref_steps(world, n_steps, lr, use_mask):
    import diffvae_ref as DV
    from oracle import torch_ref as R
    cfg = _vcfg()
    params = {k: np.asarray(v, np.float64) for k, v in DV.init_params(cfg, randomize_all=True, dtype=np.float64).items()}
    m = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in params.items()}
    v_ = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in params.items()}
    spec_in, emb, spec_out = _vbatch(world)
    out = []
    for t in range(1, n_steps + 1):
        total, per_rank = None, []
        for r in range(world):
            sl = slice(r * B, (r + 1) * B)
            eps, mask = _vinputs(r)
            inter = {}
            loss, dl, kl, pred, g = DV.loss_and_grads(params, spec_in[sl], emb[sl], spec_out[sl], cfg, eps, 0.9, B * world,
                                                      mask if use_mask else None, inter=inter, diff_loss=True)
            per_rank.append(dict(loss=loss, dl=dl, kl=kl, pred=pred, inter=inter))
            total = g if total is None else {k: total[k] + g[k] for k in g}
        out.append(dict(ranks=per_rank, grads=total))
        for k in params:
            new, m[k], v_[k] = R.adam_update(torch.tensor(params[k]), total[k], m[k], v_[k], t, lr)
            params[k] = new.numpy()
    return params, out


@pytest.mark.parametrize("overlap", [False, True])
def test_diffvae_step_on_the_product_schedule_matches_the_restatement(monkeypatch, overlap):
    import diffvae_ref as DV
    import unet_rir_amd as U
    rt, impl = _install(monkeypatch, "vae")
    cfg, params, eng, tr = _vbuild(rt, overlap)
    assert eng.l2_names == [] and {n: tuple(s.keras_shape) for n, s in eng.specs.items()} == DV.param_shapes(cfg)
    assert eng.specs["encoder_inf_dense.kernel"].kind == "dense" and eng.output_act == "linear" and eng.n_dropout_draws == 1
    assert U.DiffVAEEngine.DEFAULTS == ((32, 64, 128, 256), 16, 1280) and eng.n_noise_draws == 1 and eng.MASKS == (None, "dec")
    spec_in, emb, spec_out = (torch.tensor(a) for a in _vbatch())
    eps, mask = (torch.tensor(a) for a in _vinputs())
    mask = mask.view(B, 1, 1, -1)
    eng.masks["eps"] = eps
    want_p, steps = _vref_steps(1, N_STEPS, LR, True)
    w0 = steps[0]["ranks"][0]
    loss = tr.step(spec_in, emb, spec_out, dropout_mask=mask, return_loss=True)
    assert float(eng.reg_out[0]) == 0.0
    assert abs(loss - w0["loss"]) <= 1e-5 * abs(w0["loss"]), (loss, w0["loss"])
    assert abs(float(eng.kl_out[0]) - w0["kl"]) <= 1e-6 * w0["kl"] and abs(float(eng.kl_out[1]) - w0["kl"] * B) <= 1e-6 * w0["kl"] * B
    assert abs(float(eng.loss_out[0]) - float(eng.kl_out[0]) - w0["dl"]) <= 1e-5 * w0["dl"]
    # the linear output passes the logits' error on unscaled (the sigmoid of tests/test_vae_sim.py quarters it): 4e-6
    assert float((eng.pred.double() - w0["pred"]).abs().max()) <= 4e-6
    assert float((w0["pred"] < 0).double().mean()) > 0.02
    L = cfg.latent_space_dim
    for node, key in ((eng._latent, "z"), (eng._mu, "mu"), (eng._lv, "log_var")):
        ref = w0["inter"][key]
        assert float((node.a.base.view(B, L).double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-7, key
    got_g = eng.export_keras_grads()
    floor = 1e-6 * max(float(g.abs().max()) for g in steps[0]["grads"].values())
    for n, g in steps[0]["grads"].items():
        e = float((got_g[n].double() - g).abs().max())
        assert e <= 1e-4 * float(g.abs().max()) + floor, (n, e)
    for n in ("mu.kernel", "log_variance.kernel", "encoder_conv_layer_1.kernel", "embedding", "encoder_inf_dense.kernel"):
        assert float(steps[0]["grads"][n].abs().max()) > 0
    loss2 = tr.step(spec_in, emb, spec_out, dropout_mask=mask, return_loss=True)
    assert abs(loss2 - steps[1]["ranks"][0]["loss"]) <= 1e-5 * abs(loss2)
    got = eng.export_keras_params()
    for n, w in want_p.items():
        assert float(np.abs(got[n].double().numpy() - w).max()) <= P_ATOL, n
    assert rt.n_cross_stream > 50 if overlap else rt.n_cross_stream == 0
    z, mean, log_var = eng.encode(spec_in, emb)
    assert z.shape == mean.shape == log_var.shape == (B, L)


def test_diffvae_fit_records_the_kl_metric_and_module_surface(monkeypatch, tmp_path):
    import inspect
    import pickle
    import unet_rir_amd as U
    rt, impl = _install(monkeypatch, "vae")
    cfg, params, eng, tr = _vbuild(rt, False, lr=0.0)
    batch = tuple(torch.tensor(a) for a in _vbatch())
    eng.masks["eps"] = torch.tensor(_vinputs()[0])
    _, steps = _vref_steps(1, 1, 0.0, False)
    w0 = steps[0]["ranks"][0]
    rec = U.fit(tr, lambda ep: [batch, batch], 1, val_batches=lambda ep: [batch], log=None)[0]
    mean_kl = w0["kl"] * B / (B * cfg.latent_space_dim)
    assert abs(rec["train_kl"] - mean_kl) <= 1e-6 * mean_kl and abs(rec["val_kl"] - mean_kl) <= 1e-6 * mean_kl
    assert abs(rec["train_loss"] - w0["loss"]) <= 1e-5 * w0["loss"]
    sig = inspect.signature(U.DiffVAE.__init__)
    assert list(sig.parameters)[1:9] == ["input_shape", "inf_vector_shape", "conv_filters", "conv_kernels", "conv_strides", "latent_space_dim",
                                         "n_neurons", "name"] and sig.parameters["name"].default == "Diff_VAE"
    model = U.DiffVAE((VH, VW, 2), (2, 16), cfg.conv_filters, cfg.conv_kernels, cfg.conv_strides, cfg.latent_space_dim, cfg.n_neurons,
                      batch_size=B, device="cpu", runtime=rt, dropout=False)
    assert isinstance(model.engine, U.DiffVAEEngine) and model.name == "Diff_VAE" and model.reconstruction_loss_weight == 100000
    model.engine.load_keras_params(params)
    with pytest.raises(NotImplementedError):
        model.compile_and_fit(None, None, None, None, None, None, 2, 1, 1)
    with pytest.raises(NotImplementedError):
        model(batch[0], batch[1])                                # autograd through the module
    x = [batch[0].permute(0, 2, 3, 1).contiguous(), batch[1]]
    z, mean, log_var = model.encoder(x, training=False)
    assert z.shape == mean.shape == log_var.shape == (B, cfg.latent_space_dim)
    out = model.decoder(z)
    assert tuple(out.shape) == (B, VH, VW, 2) and float(out.min()) < 0.0
    model.save(str(tmp_path))
    with open(tmp_path / "parameters.pkl", "rb") as f:
        assert pickle.load(f) == [(VH, VW, 2), (2, 16), cfg.conv_filters, cfg.conv_kernels, cfg.conv_strides, cfg.latent_space_dim, cfg.n_neurons]
    again = U.DiffVAE.load(str(tmp_path), batch_size=B, device="cpu", runtime=rt)
    assert isinstance(again.engine, U.DiffVAEEngine) and torch.equal(again.engine.theta, model.engine.theta)
    assert torch.equal(again.decoder(z), out)


def _vae_dp_worker(rank, world, port, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mpatch = pytest.MonkeyPatch()
        rt, impl = _install(mpatch, "vae")
        cfg, params, eng, tr = _vbuild(rt, True, world=world)
        if rank != 0:
            eng.theta.mul_(0.5)
        tr.broadcast_parameters(0)
        spec_in, emb, spec_out = _vbatch(world)
        sl = slice(rank * B, (rank + 1) * B)
        eng.masks["eps"] = torch.tensor(_vinputs(rank)[0])
        t = torch.tensor
        losses, kls = [], []
        for _ in range(N_STEPS):
            losses.append(tr.step(t(spec_in[sl]), t(emb[sl]), t(spec_out[sl]), return_loss=True))
            kls.append([float(eng.kl_out[0]), float(eng.kl_out[1])])
        lt = torch.tensor(losses, dtype=torch.float64)
        dist.all_reduce(lt)
        torch.save({"params": {k: v.double() for k, v in eng.export_keras_params().items()}, "losses": lt, "kl": kls}, f"{out_path}.{rank}")
        mpatch.undo()
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_diffvae_two_gloo_ranks(tmp_path):
    world = 2
    out = str(tmp_path / "vdp")
    mp.spawn(_vae_dp_worker, args=(world, 35900 + (os.getpid() % 1500), out), nprocs=world, join=True)
    want_p, steps = _vref_steps(world, N_STEPS, LR, False)
    res = [torch.load(f"{out}.{r}") for r in range(world)]
    for r in range(world):
        w = steps[0]["ranks"][r]
        kl0, kl1 = res[r]["kl"][0]
        assert abs(kl0 - w["kl"]) <= 1e-6 * w["kl"] and abs(kl0 * B * world - kl1) <= 1e-6 * kl1
        for n, wp in want_p.items():
            assert float(np.abs(res[r]["params"][n].numpy() - wp).max()) <= P_ATOL, (r, n)
        np.testing.assert_allclose(res[r]["losses"].numpy(), np.array([sum(x["loss"] for x in s["ranks"]) for s in steps]), rtol=1e-5)
    for n in want_p:
        assert torch.equal(res[0]["params"][n], res[1]["params"][n]), n


# ------------------------------------------------------------------------------------------------ the shared helper
def test_vqvae_specs_and_op_count_are_what_the_parent_commit_built(monkeypatch):
    """AEFamilyEngine._join_vector_per_position took over VQVAEEngine's own lines.  The values below were computed from the parent
    commit's tree (VQVAEEngine(16, 32, 2, (8, 8, 8, 8), kernels 3, strides 2, latent 4, n_neurons 8) on the simulated runtime): the number of
    ops, the number of parameters and a digest of every (name, shape, offset, kind, keras_shape) in flat-buffer order."""
    import unet_rir_amd as U
    import vqvae_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    vqvae_cpu_ops.install(monkeypatch, rt)
    parent = {"f32": (27, 42, "9341c3aa71bd211b", 4864), "bf16": (28, 42, "46ab44fdb6358f1d", 5120)}
    for dtype, (n_ops, n_specs, digest, off) in parent.items():
        eng = U.VQVAEEngine(16, 32, 2, (8, 8, 8, 8), (3, 3, 3, 3), (2, 2, 2, 2), 4, 8, device="cpu", runtime=rt, dtype=dtype)
        spec = [(n, s.shape, s.offset, s.kind, s.keras_shape) for n, s in eng.specs.items()]
        assert (len(eng.ops), len(spec), hashlib.sha256(repr(spec).encode()).hexdigest()[:16]) == (n_ops, n_specs, digest), dtype
        assert eng.specs["encoder_inf_dense.kernel"].offset == off and eng.n_params() == 198694
        assert eng.specs["encoder_inf_dense.kernel"].kind == "dense" and tuple(eng.specs["encoder_inf_dense.kernel"].keras_shape) == (128, 8)

"""The PRODUCT's VAEEngine + Trainer + fit on CPU tensors: only the kernels (tests/vae_cpu_ops.py: fp64 arithmetic) and the stream
runtime (tests/sim_runtime.py: vector clocks + race check) are stand-ins.  Against the fp64 restatement tests/vae_ref.py:

  * one step with eps and the decoder mask supplied, plain and side-stream schedule: prediction, loss = data term + KL, the KL
    term alone (both normalisations), every gradient - the bottleneck's included, which is the SUM of the two heads' data
    gradients - and the parameters after two Adam steps; a missing happens-before edge would raise RaceError;
  * `fit` records carry train_kl / val_kl = the mean of kl_loss_object over every (b, l) element, other engines' records keep
    their keys;
  * the noise draw is counted in the dropout masks' counter whatever the trainer's `dropout` flag, and changes z every step;
  * two gloo ranks: the KL term is divided by the GLOBAL batch and the replicas end bit-identical.

The engine's buffers are fp32 (storage as on the device) while the arithmetic is fp64, so agreement is to fp32 storage rounding:
the tolerances of tests/test_schedule_sim.py (loss 1e-5 relative, gradients 1e-4 of the tensor's largest entry, parameters 2 % of
the distance Adam can have moved them).
"""
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

H = W = 16
LR, N_STEPS = 1e-3, 2
P_ATOL = 0.02 * LR * N_STEPS


def _cfg():
    import vae_ref as V
    return V.VAEConfig(H, W, (4, 8, 8, 8), (3, 3, 3, 3), (2, 2, 2, 2), 8, 16)


def _inputs(B, rank=0):
    cfg = _cfg()
    rng = np.random.RandomState(100 + rank)
    eps = rng.standard_normal((B, cfg.latent_space_dim)).astype(np.float32)
    h, w, c = cfg.bottleneck_shape()
    mask = ((rng.uniform(size=(B, h * w * c)) >= 0.3) / 0.7).astype(np.float32)
    return eps, mask


def _build(rt, B, overlap, world=1, bucket_bytes=8192, dropout=False, lr=LR):
    import unet_rir_amd as U
    import vae_ref as V
    cfg = _cfg()
    params = V.init_params(cfg, randomize_all=True, dtype=np.float64)
    eng = U.VAEEngine(H, W, B, cfg.conv_filters, cfg.conv_kernels, cfg.conv_strides, cfg.latent_space_dim, cfg.n_neurons,
                      device="cpu", runtime=rt, n_replicas=world, overlap_wgrad=overlap)
    eng.load_keras_params(params)
    tr = U.Trainer(eng, lr=lr, dropout=dropout, world_size=world, bucket_bytes=bucket_bytes)
    return cfg, params, eng, tr


def _ref_steps(world, B, n_steps, lr, use_mask):
    """The reference semantics on one process: per-replica loss over the global batch, gradients summed, one Adam per step."""
    import vae_ref as V
    from oracle import torch_ref as R
    cfg = _cfg()
    params = {k: np.asarray(v, np.float64) for k, v in V.init_params(cfg, randomize_all=True, dtype=np.float64).items()}
    m = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in params.items()}
    v_ = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in params.items()}
    spec_in, emb, spec_out = R.synthetic_batch(R.Config(H, W), B * world)
    out = []
    for t in range(1, n_steps + 1):
        total, per_rank = None, []
        for r in range(world):
            sl = slice(r * B, (r + 1) * B)
            eps, mask = _inputs(B, r)
            inter = {}
            loss, dl, kl, pred, g = V.loss_and_grads(params, spec_in[sl], emb[sl], spec_out[sl], cfg, eps, 0.9, B * world,
                                                     mask if use_mask else None, inter=inter)
            per_rank.append(dict(loss=loss, dl=dl, kl=kl, pred=pred, inter=inter))
            total = g if total is None else {k: total[k] + g[k] for k in g}
        out.append(dict(ranks=per_rank, grads=total))
        for k in params:
            new, m[k], v_[k] = R.adam_update(torch.tensor(params[k]), total[k], m[k], v_[k], t, lr)
            params[k] = new.numpy()
    return params, out


@pytest.mark.parametrize("overlap", [False, True])
def test_vae_step_on_the_product_schedule_matches_vae_ref(monkeypatch, overlap):
    import vae_cpu_ops
    from sim_runtime import SimRuntime
    from oracle import torch_ref as R
    rt = SimRuntime()
    vae_cpu_ops.install(monkeypatch, rt)
    B = 2
    cfg, params, eng, tr = _build(rt, B, overlap)
    assert eng.l2_names == [] and set(eng.specs) == set(params)
    spec_in, emb, spec_out = (torch.tensor(a) for a in R.synthetic_batch(R.Config(H, W), B))
    eps, mask = (torch.tensor(a) for a in _inputs(B))
    mask = mask.view(B, 1, 1, -1)                 # the stand-in of ops.mul multiplies tensors of one shape (the kernel is flat)
    eng.masks["eps"] = eps
    want_p, steps = _ref_steps(1, B, N_STEPS, LR, True)
    w0 = steps[0]["ranks"][0]
    loss = tr.step(spec_in, emb, spec_out, dropout_mask=mask, return_loss=True)
    assert float(eng.reg_out[0]) == 0.0
    assert abs(loss - w0["loss"]) <= 1e-5 * abs(w0["loss"]), (loss, w0["loss"])
    assert abs(float(eng.kl_out[0]) - w0["kl"]) <= 1e-6 * w0["kl"]
    assert abs(float(eng.kl_out[1]) - w0["kl"] * B) <= 1e-6 * w0["kl"] * B          # the raw sum: global batch = B here
    assert abs(float(eng.loss_out[0]) - float(eng.kl_out[0]) - w0["dl"]) <= 1e-5 * w0["dl"]
    assert float((eng.pred.double() - w0["pred"]).abs().max()) <= 1e-6
    L = cfg.latent_space_dim
    for node, key in ((eng._latent, "z"), (eng._mu, "mu"), (eng._lv, "log_var")):
        ref = w0["inter"][key]
        assert float((node.a.base.view(B, L).double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-7, key
    got_g = eng.export_keras_grads()
    assert set(got_g) == set(steps[0]["grads"])
    floor = 1e-6 * max(float(g.abs().max()) for g in steps[0]["grads"].values())
    for n, g in steps[0]["grads"].items():
        e = float((got_g[n].double() - g).abs().max())
        assert e <= 1e-4 * float(g.abs().max()) + floor, (n, e)
    for n in ("mu.kernel", "log_variance.kernel", "encoder_conv_layer_1.kernel", "embedding"):      # the KL term reaches all of these
        assert float(steps[0]["grads"][n].abs().max()) > 0
    loss2 = tr.step(spec_in, emb, spec_out, dropout_mask=mask, return_loss=True)
    assert abs(loss2 - steps[1]["ranks"][0]["loss"]) <= 1e-5 * abs(loss2)
    got = eng.export_keras_params()
    for n, w in want_p.items():
        assert float(np.abs(got[n].double().numpy() - w).max()) <= P_ATOL, n
    if overlap:
        assert len(tr.bucketer.bounds) > 3 and rt.n_cross_stream > 50
    else:
        assert rt.n_cross_stream == 0


def test_encode_and_decode_are_the_two_halves_of_forward(monkeypatch):
    import vae_cpu_ops
    from sim_runtime import SimRuntime
    from oracle import torch_ref as R
    rt = SimRuntime()
    vae_cpu_ops.install(monkeypatch, rt)
    B = 2
    cfg, params, eng, tr = _build(rt, B, False)
    spec_in, emb, _ = (torch.tensor(a) for a in R.synthetic_batch(R.Config(H, W), B))
    eps, mask = (torch.tensor(a) for a in _inputs(B))
    mask = mask.view(B, 1, 1, -1)                 # the stand-in of ops.mul multiplies tensors of one shape (the kernel is flat)
    eng.masks["eps"] = eps
    pred = eng.forward(spec_in, emb, dropout_mask=mask).clone()
    z, mean, log_var = eng.encode(spec_in, emb)
    assert z.shape == mean.shape == log_var.shape == (B, cfg.latent_space_dim)
    assert float((z - mean - torch.exp(0.5 * log_var) * eps).abs().max()) <= 1e-6
    assert torch.equal(eng.decode(z, mask), pred)


def test_fit_records_carry_the_kl_metric(monkeypatch):
    """lr = 0 keeps the parameters (Adam's update is lr_t * m / (sqrt(v) + eps)), the batch statistics are the batch's: every
    step sees the same KL sum, so train_kl = val_kl = mean over (b, l) of kl_loss_object."""
    import unet_rir_amd as U
    import vae_cpu_ops
    from sim_runtime import SimRuntime
    from oracle import torch_ref as R
    rt = SimRuntime()
    vae_cpu_ops.install(monkeypatch, rt)
    B = 2
    cfg, params, eng, tr = _build(rt, B, False, lr=0.0)
    batch = tuple(torch.tensor(a) for a in R.synthetic_batch(R.Config(H, W), B))
    eps, _ = _inputs(B)
    eng.masks["eps"] = torch.tensor(eps)
    _, steps = _ref_steps(1, B, 1, 0.0, False)
    w0 = steps[0]["ranks"][0]
    hist = U.fit(tr, lambda ep: [batch, batch, batch], 1, val_batches=lambda ep: [batch, batch], log=None)
    rec = hist[0]
    mean_kl = w0["kl"] * B / (B * cfg.latent_space_dim)
    assert abs(rec["train_kl"] - mean_kl) <= 1e-6 * mean_kl and abs(rec["val_kl"] - mean_kl) <= 1e-6 * mean_kl
    assert abs(rec["train_loss"] - w0["loss"]) <= 1e-5 * w0["loss"] and abs(rec["val_loss"] - w0["loss"]) <= 1e-5 * w0["loss"]
    # other engines: the records keep their keys
    ae = U.AutoencoderEngine(H, W, B, cfg.conv_filters, cfg.conv_kernels, cfg.conv_strides, 8, 16, device="cpu", runtime=rt)
    ae.reset_parameters(torch.Generator().manual_seed(1))
    rec_ae = U.fit(U.Trainer(ae, lr=1e-3, dropout=False), lambda ep: [batch], 1, val_batches=lambda ep: [batch], log=None)[0]
    assert set(rec_ae) == {"epoch", "lr", "train_loss", "train_amp", "train_phase", "val_loss", "val_amp", "val_phase"}
    assert set(rec) == set(rec_ae) | {"train_kl", "val_kl"}


@pytest.mark.parametrize("dropout", [False, True])
def test_noise_is_drawn_every_step_and_counted_with_the_masks(monkeypatch, dropout):
    import vae_cpu_ops
    from sim_runtime import SimRuntime
    from oracle import torch_ref as R
    rt = SimRuntime()
    vae_cpu_ops.install(monkeypatch, rt)
    B = 2
    cfg, params, eng, tr = _build(rt, B, False, dropout=dropout, lr=0.0)
    batch = tuple(torch.tensor(a) for a in R.synthetic_batch(R.Config(H, W), B))
    zs = []
    for _ in range(3):
        tr.step(*batch)
        zs.append(eng._latent.a.base.clone())
    assert not torch.equal(zs[0], zs[1]) and not torch.equal(zs[1], zs[2])
    assert eng._shared["dropout_step"] == 3 * (2 if dropout else 1)
    # a supplied eps consumes its draw number too: the host counter keeps pace with what the trainer announces per step
    eng.masks["eps"] = torch.zeros((B, cfg.latent_space_dim))
    tr.step(*batch)
    assert eng._shared["dropout_step"] == 4 * (2 if dropout else 1)
    assert torch.equal(eng._latent.a.base, eng._mu.a.base)                 # eps = 0: z is the mean


def _dp_worker(rank, world, port, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import vae_cpu_ops
        from sim_runtime import SimRuntime
        from oracle import torch_ref as R
        mpatch = pytest.MonkeyPatch()
        rt = SimRuntime()
        vae_cpu_ops.install(mpatch, rt)
        B = 2
        cfg, params, eng, tr = _build(rt, B, True, world=world)
        if rank != 0:
            eng.theta.mul_(0.5)                       # replicas must end up with rank 0's variables
        tr.broadcast_parameters(0)
        spec_in, emb, spec_out = R.synthetic_batch(R.Config(H, W), B * world)
        sl = slice(rank * B, (rank + 1) * B)
        eng.masks["eps"] = torch.tensor(_inputs(B, rank)[0])
        t = torch.tensor
        losses, kls = [], []
        for _ in range(N_STEPS):
            losses.append(tr.step(t(spec_in[sl]), t(emb[sl]), t(spec_out[sl]), return_loss=True))
            kls.append([float(eng.kl_out[0]), float(eng.kl_out[1])])
        lt = torch.tensor(losses, dtype=torch.float64)
        dist.all_reduce(lt)                           # strategy.reduce(SUM, per_replica_losses) (main_training.py:326)
        torch.save({"params": {k: v.double() for k, v in eng.export_keras_params().items()}, "losses": lt, "kl": kls,
                    "n_buckets": len(tr.bucketer.bounds)}, f"{out_path}.{rank}")
        mpatch.undo()
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_divide_the_kl_term_by_the_global_batch(tmp_path):
    world, B = 2, 2
    out = str(tmp_path / "vdp")
    mp.spawn(_dp_worker, args=(world, 32800 + (os.getpid() % 1500), out), nprocs=world, join=True)
    want_p, steps = _ref_steps(world, B, N_STEPS, LR, False)
    res = [torch.load(f"{out}.{r}") for r in range(world)]
    for r in range(world):
        assert res[r]["n_buckets"] > 3
        w = steps[0]["ranks"][r]
        kl0, kl1 = res[r]["kl"][0]
        assert abs(kl0 - w["kl"]) <= 1e-6 * w["kl"], (r, kl0, w["kl"])            # w["kl"]: this replica's sum / (B * world)
        assert abs(kl0 * B * world - kl1) <= 1e-6 * kl1
        for n, wp in want_p.items():
            assert float(np.abs(res[r]["params"][n].numpy() - wp).max()) <= P_ATOL, (r, n)
        want_l = np.array([sum(x["loss"] for x in s["ranks"]) for s in steps])
        np.testing.assert_allclose(res[r]["losses"].numpy(), want_l, rtol=1e-5)
    for n in want_p:                                  # replicas stay bit-identical
        assert torch.equal(res[0]["params"][n], res[1]["params"][n]), n

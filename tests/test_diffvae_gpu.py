"""unet_rir_amd.DiffVAEEngine / DiffVAE (dl_models/diff_vae.py) on the GPU against tests/diffvae_ref.py with a supplied eps, at the
bounds of tests/test_vae_gpu.py; bf16 by the storage-model criterion; the step machinery.  Driven with diff_loss=True."""
import math

import numpy as np
import pytest
import torch

import diffvae_ref as DV
from oracle import detrand, torch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, B = 32, 48, 2


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def _net_case(filters, latent, nn, dropout):
    cfg = DV.config(H, W, filters, (3,) * len(filters), (2,) * len(filters), latent, nn)
    Pn = DV.init_params(cfg, randomize_all=True, dtype=np.float64)
    spec_in, emb, spec_out = R.synthetic_batch(R.Config(H, W), B)
    h, w, c = cfg.bottleneck_shape()
    eps = np.random.RandomState(7).standard_normal((B, latent))
    md = (detrand.uniform("dvae-md", (B, h * w * c)) >= 0.3).astype(np.float64) / 0.7 if dropout else None
    return cfg, Pn, (spec_in, emb % DV.VOCAB, spec_out), eps, md


@pytest.mark.parametrize("filters,latent,nn,do", [((8, 16), 8, 16, False), ((8, 16, 32, 64), 32, 64, True)])
def test_fp32_engine_against_the_restatement(U, filters, latent, nn, do):
    """The fp32 criteria of tests/test_vae_gpu.py: prediction 1e-4 absolute, loss and KL term 1e-5 relative, every gradient 1e-3 of
    its own largest entry plus the floor."""
    cfg, Pn, (spec_in, emb, spec_out), eps, md = _net_case(filters, latent, nn, do)
    inter = {}
    loss, dl, kl, pred, grads = DV.loss_and_grads(Pn, spec_in, emb, spec_out, cfg, eps, 0.9, B, md, inter=inter, diff_loss=True)
    assert float((pred < 0).double().mean()) > 0.05           # the linear output is exercised
    eng = U.DiffVAEEngine(H, W, B, filters, cfg.conv_kernels, cfg.conv_strides, latent, nn, device=DEV)
    eng.load_keras_params(Pn)
    eng.loss_diff = True
    t = lambda a, dt=None: None if a is None else torch.tensor(a, dtype=dt).to(DEV)
    eng.masks["eps"] = t(eps, torch.float32)
    eng.forward(t(spec_in), t(emb), dropout_mask=None if md is None else t(md, torch.float32).view(B, 1, 1, -1), target=t(spec_out),
                global_batch=B)
    eng.backward()
    eng.reg_loss()
    torch.cuda.synchronize()
    assert eng.l2_names == [] and float(eng.reg_out[0]) == 0.0 and eng.output_act == "linear"
    assert float((eng.pred.double().cpu() - pred).abs().max()) <= 1e-4
    got = float(eng.loss_out[0]) + float(eng.reg_out[0])
    print(f"diffvae {filters}: loss {got:.8g} ref {loss:.8g}; kl {float(eng.kl_out[0]):.8g} ref {kl:.8g}; data ref {dl:.8g}")
    assert abs(got - loss) <= 1e-5 * abs(loss), (got, loss)
    assert abs(float(eng.kl_out[0]) - kl) <= 1e-5 * abs(kl) and abs(float(eng.kl_out[1]) - kl * B) <= 1e-5 * abs(kl * B)
    for node, key in ((eng._latent, "z"), (eng._mu, "mu"), (eng._lv, "log_var")):
        ref = inter[key]
        assert float((node.a.base.view(B, latent).double().cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), key
    kg = eng.export_keras_grads()
    assert set(kg) == set(grads) == set(DV.param_shapes(cfg))
    floor = 1e-6 * max(float(g.abs().max()) for g in grads.values())
    for n, g_ref in grads.items():
        e = float((kg[n].double() - g_ref).abs().max())
        assert e <= 1e-3 * float(g_ref.abs().max()) + floor, (n, e, float(g_ref.abs().max()))
    z, mean, log_var = eng.encode(t(spec_in), t(emb))
    assert z.shape == mean.shape == log_var.shape == (B, latent)
    assert float((mean.double().cpu() - inter["mu"]).abs().max()) <= 1e-4 * float(inter["mu"].abs().max())


def test_bf16_engine_is_as_close_as_the_storage_model(U):
    """tests/diffvae_ref.py with bf16 roundings where the product stores bf16 IS the storage model; the HIP path is as close to the exact
    fp64 result as it is (the bounds of tests/test_vae_gpu.py's bf16 test)."""
    Hq = Wq = 64
    Bq = 4
    cfg = DV.config(Hq, Wq, (8, 16, 16, 32), (3, 3, 3, 3), (2, 2, 2, 2), 8, 16)
    params = DV.init_params(cfg, randomize_all=True, dtype=np.float64)
    spec_in, emb, spec_out = R.synthetic_batch(R.Config(Hq, Wq), Bq)
    emb = emb % DV.VOCAB
    eps = np.random.RandomState(9).standard_normal((Bq, 8)).astype(np.float32)
    eng = U.DiffVAEEngine(Hq, Wq, Bq, cfg.conv_filters, cfg.conv_kernels, cfg.conv_strides, cfg.latent_space_dim, cfg.n_neurons,
                          dtype="bf16", device=DEV)
    eng.load_keras_params(params)
    eng.loss_diff = True
    t = lambda a: torch.tensor(a).to(DEV)
    eng.masks["eps"] = t(eps)
    eng.forward(t(spec_in), t(emb), target=t(spec_out), global_batch=Bq)
    eng.backward()
    torch.cuda.synchronize()
    pred_h, loss_h, kl_h = eng.pred.double().cpu(), float(eng.loss_out[0]), float(eng.kl_out[0])
    g_h = {k: v.double().cpu() for k, v in eng.export_keras_grads().items()}
    loss_x, _, kl_x, pred_x, g_x = DV.loss_and_grads(params, spec_in, emb, spec_out, cfg, eps, 0.9, Bq, diff_loss=True)
    loss_q, _, kl_q, pred_q, g_q = DV.loss_and_grads(params, spec_in, emb, spec_out, cfg, eps, 0.9, Bq, diff_loss=True, storage="bf16")
    nx = float(pred_x.norm())
    e_h, e_q = float((pred_h - pred_x).norm()) / nx, float((pred_q - pred_x).norm()) / nx
    print(f"diffvae bf16: pred rel L2 error hip {e_h:.2e} model {e_q:.2e}; loss hip {loss_h:.6f} model {loss_q:.6f} exact {loss_x:.6f}; "
          f"kl hip {kl_h:.6f} model {kl_q:.6f} exact {kl_x:.6f}")
    assert e_h <= 2.0 * e_q + 0.01, (e_h, e_q)
    assert abs(loss_h - loss_x) <= 2.0 * abs(loss_q - loss_x) + 1e-2 * abs(loss_x), (loss_h, loss_q, loss_x)
    assert abs(kl_h - kl_x) <= 2.0 * abs(kl_q - kl_x) + 1e-2 * abs(kl_x), (kl_h, kl_q, kl_x)
    checked = 0
    gmax = max(float(g.abs().max()) for g in g_x.values())
    for n, gx in g_x.items():
        if float(gx.abs().max()) < 1e-6 * gmax:
            continue                               # analytically zero (biases in front of a BatchNorm)
        nrm = float(gx.norm()) + 1e-30
        assert float((g_h[n] - gx).norm()) / nrm <= 2.0 * float((g_q[n] - gx).norm()) / nrm + 0.03, n
        checked += 1
    assert checked > 20


def _engine(U, dtype="f32", overlap=False):
    eng = U.DiffVAEEngine(H, W, B, (8, 16, 32), (3, 3, 3), (2, 2, 2), 16, 32, device=DEV, dtype=dtype, overlap_wgrad=overlap)
    eng.reset_parameters(torch.Generator().manual_seed(3))
    eng.dropout_seed = 77
    return eng


def _batches(n):
    gen = torch.Generator(); gen.manual_seed(5)
    return [(torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
             torch.rand((B, 2, H, W), generator=gen).to(DEV)) for _ in range(n)]


def _state(eng):
    return (eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), {k: v.clone() for k, v in eng.moving.items()}, eng.adam_t,
            eng._shared["dropout_step"])


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    assert a[4] == b[4] and a[5] == b[5]


@pytest.mark.parametrize("dtype,overlap", [("f32", False), ("bf16", True)])
def test_three_steps_twice_and_a_captured_step(U, dtype, overlap):
    """Three steps twice from one seed are bit-identical, and so is the captured step against the same launches issued one by one."""
    data = _batches(3)
    res = {}
    for mode in ("eager", "eager2", "graph", "eager_dev"):
        eng = _engine(U, dtype, overlap)
        tr = U.Trainer(eng, lr=1e-3, bucket_bytes=16 << 10, graph=(mode == "graph"), diff_loss=True)
        if mode == "eager_dev":
            eng.use_device_counters(True)
        losses = [tr.step(a, e, b, return_loss=True) for a, e, b in data]
        torch.cuda.synchronize()
        res[mode] = (losses, _state(eng), eng._latent.a.base.clone(), eng.pred.clone())
    for a, b in (("eager", "eager2"), ("graph", "eager_dev")):
        assert res[a][0] == res[b][0] and torch.equal(res[a][2], res[b][2]) and torch.equal(res[a][3], res[b][3])
        _same(res[a][1], res[b][1])
    assert res["eager"][1][5] == 3 * 2 and all(math.isfinite(x) for x in res["eager"][0])       # a mask and an eps per step
    assert float(res["eager"][3].min()) < 0.0


def test_checkpoint_after_step_2_resumes_to_a_bit_identical_step_3(U, tmp_path):
    data = _batches(3)
    e0 = _engine(U)
    t0 = U.Trainer(e0, lr=1e-3, diff_loss=True)
    for a, e, b in data:
        t0.step(a, e, b)
    torch.cuda.synchronize()
    e1 = _engine(U)
    t1 = U.Trainer(e1, lr=1e-3, diff_loss=True)
    for a, e, b in data[:2]:
        t1.step(a, e, b)
    path = U.CheckpointManager(t1, str(tmp_path)).save(epoch=0)
    e2 = _engine(U)
    e2.dropout_seed = 5
    t2 = U.Trainer(e2, lr=1e-3, diff_loss=True)
    U.CheckpointManager(t2, str(tmp_path)).restore(path)
    assert e2._shared["dropout_step"] == 4 and e2.dropout_seed == 77
    t2.step(*data[2])
    torch.cuda.synchronize()
    _same(_state(e0), _state(e2))
    assert torch.equal(e0._latent.a.base, e2._latent.a.base) and torch.equal(e0.pred, e2.pred)


def test_fit_reports_the_kl_metric_and_the_module_encodes(U):
    (a, e, b), = _batches(1)
    eng = _engine(U)
    tr = U.Trainer(eng, lr=0.0, dropout=False, diff_loss=True)
    eng.masks["eps"] = torch.zeros((B, 16), device=DEV)
    rec = U.fit(tr, lambda ep: [(a, e, b)] * 2, 1, val_batches=lambda ep: [(a, e, b)], log=None)[0]
    torch.cuda.synchronize()
    import vae_ref as V
    mu, lv = eng._mu.a.base.view(B, 16).double().cpu(), eng._lv.a.base.view(B, 16).double().cpu()
    want = float(V.kl_elements(mu, lv).mean())
    assert abs(rec["train_kl"] - want) <= 1e-5 * want and abs(rec["val_kl"] - want) <= 1e-5 * want
    model = U.DiffVAE((H, W, 2), (2, 16), (8, 16), (3, 3), (2, 2), 8, 16, batch_size=B, device=DEV)
    z, mean, log_var = model.encoder([a.permute(0, 2, 3, 1), e], training=False)
    assert z.shape == mean.shape == log_var.shape == (B, 8) and model.reconstruction_loss_weight == 100000
    with pytest.raises(NotImplementedError):
        model.compile_and_fit(None, None, None, None, None, None, 2, 1, 1)
    with pytest.raises(NotImplementedError):
        model.model([a.permute(0, 2, 3, 1), e], training=True)
    ev = U.Evaluator(model, diff_gen=True)
    with torch.no_grad():
        out = model.model([a.permute(0, 2, 3, 1), e], training=False)
    ev.update_scored(out.permute(0, 3, 1, 2).contiguous(), a, b, None, None, [ev.rooms[0]] * B)
    assert np.isfinite(ev.result()["phase"][0])

"""The PRODUCT's VQVAEEngine + Trainer + fit on CPU tensors: only the kernels (tests/vqvae_cpu_ops.py: fp64 arithmetic) and the
stream runtime (tests/sim_runtime.py: vector clocks + race check) are stand-ins.  Against the fp64 restatement tests/vqvae_ref.py:

  * the op list is the graph of dl_models/vqvae.py: one quantiser, one Dropout, a decoder without Dense / Dropout / Reshape;
  * one step with the bottleneck mask supplied, plain and side-stream schedule: prediction, loss = data term + vq term / replicas,
    the term alone, the indices, every gradient (the codebook's included) and the parameters after two Adam steps; a missing
    happens-before edge would raise RaceError;
  * one Dropout draw per step; the codebook lives in the parameter store, in a gradient bucket, and `share=` aliases it;
  * encode / decode are the two halves of forward and carry the quantised feature map; `fit` records train_vq / val_vq.

The engine's buffers are fp32 (storage as on the device) while the arithmetic is fp64, so agreement is to fp32 storage rounding:
the tolerances of tests/test_vae_sim.py.  The reference takes the engine's indices after they have been checked against its own
search (equal here: fp64 on both sides, margins far above fp32 storage rounding)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 16, 32
LR, N_STEPS = 1e-3, 2
P_ATOL = 0.02 * LR * N_STEPS


def _cfg():
    import vqvae_ref as Q
    return Q.VQVAEConfig(H, W, (4, 8, 8, 8), (3, 3, 3, 3), (2, 2, 2, 2), 4, 8)


def _mask(B, rank=0):
    h, w, c = _cfg().bottleneck_shape()
    return ((np.random.RandomState(100 + rank).uniform(size=(B, h * w * 2)) >= 0.3) / 0.7).astype(np.float32)


def _batch(B):
    import vqvae_ref as Q
    from oracle import torch_ref as R
    spec_in, emb, spec_out = R.synthetic_batch(R.Config(H, W), B)
    return spec_in, emb % Q.VOCAB, spec_out


def _build(rt, B, overlap, world=1, bucket_bytes=8192, dropout=False, lr=LR, share=None):
    import unet_rir_amd as U
    import vqvae_ref as Q
    cfg = _cfg()
    params = Q.init_params(cfg, randomize_all=True, dtype=np.float64, codebook_scale=8.0)
    eng = U.VQVAEEngine(H, W, B, cfg.conv_filters, cfg.conv_kernels, cfg.conv_strides, cfg.latent_space_dim, cfg.n_neurons,
                        device="cpu", runtime=rt, n_replicas=world, overlap_wgrad=overlap, share=share)
    if share is None:
        eng.load_keras_params(params)
    tr = U.Trainer(eng, lr=lr, dropout=dropout, world_size=world, bucket_bytes=bucket_bytes)
    return cfg, params, eng, tr


def _ref_steps(B, n_steps, lr):
    import vqvae_ref as Q
    from oracle import torch_ref as R
    cfg = _cfg()
    params = {k: np.asarray(v, np.float64) for k, v in Q.init_params(cfg, randomize_all=True, dtype=np.float64, codebook_scale=8.0).items()}
    m = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in params.items()}
    v_ = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in params.items()}
    batch = _batch(B)
    out = []
    for t in range(1, n_steps + 1):
        inter = {}
        loss, dl, term, pred, g = Q.loss_and_grads(params, *batch, cfg, 0.9, B, _mask(B), inter=inter)
        out.append(dict(loss=loss, dl=dl, term=term, pred=pred, inter=inter, grads=g))
        for k in params:
            new, m[k], v_[k] = R.adam_update(torch.tensor(params[k]), g[k], m[k], v_[k], t, lr)
            params[k] = new.numpy()
    return params, out


def _install(monkeypatch):
    import vqvae_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    return rt, vqvae_cpu_ops.install(monkeypatch, rt)


@pytest.mark.parametrize("overlap", [False, True])
def test_vqvae_step_on_the_product_schedule_matches_vqvae_ref(monkeypatch, overlap):
    import vqvae_ref as Q
    rt, impl = _install(monkeypatch)
    B = 2
    cfg, params, eng, tr = _build(rt, B, overlap)
    assert eng.l2_names == [] and set(eng.specs) == set(params)
    assert {n: s.keras_shape for n, s in eng.specs.items()} == Q.param_shapes(cfg)
    batch = tuple(torch.tensor(a) for a in _batch(B))
    mask = torch.tensor(_mask(B)).view(B, 1, 1, -1)          # the stand-in of ops.mul multiplies tensors of one shape
    want_p, steps = _ref_steps(B, N_STEPS, LR)
    w0 = steps[0]
    loss = tr.step(*batch, dropout_mask=mask, return_loss=True)
    assert float(eng.reg_out[0]) == 0.0
    assert torch.equal(eng.vq_indices.long(), w0["inter"]["idx"]) and len(set(eng.vq_indices.tolist())) > 1
    assert abs(loss - w0["loss"]) <= 1e-5 * abs(w0["loss"]), (loss, w0["loss"])
    assert abs(float(eng.vq_out[0]) - w0["term"]) <= 1e-6 * w0["term"]
    N = eng.vq_elems
    assert abs(float(eng.vq_out[1]) * (1 + Q.BETA) / N - w0["term"]) <= 1e-6 * w0["term"]
    assert abs(float(eng.loss_out[0]) - float(eng.vq_out[0]) - w0["dl"]) <= 1e-5 * w0["dl"]
    assert float((eng.pred.double() - w0["pred"]).abs().max()) <= 1e-6
    ref_y = w0["inter"]["y"]
    assert float((eng._latent.a.base.double() - ref_y).abs().max()) <= 1e-6 * float(ref_y.abs().max()) + 1e-7
    got_g = eng.export_keras_grads()
    assert set(got_g) == set(w0["grads"])
    floor = 1e-6 * max(float(g.abs().max()) for g in w0["grads"].values())
    for n, g in w0["grads"].items():
        e = float((got_g[n].double() - g).abs().max())
        assert e <= 1e-4 * float(g.abs().max()) + floor, (n, e)
    for n in (Q.CODEBOOK, "conv2d.kernel", "dense.kernel", "encoder_inf_dense.kernel", "encoder_conv_layer_1.kernel", "embedding"):
        assert float(w0["grads"][n].abs().max()) > 0, n
    loss2 = tr.step(*batch, dropout_mask=mask, return_loss=True)
    assert abs(loss2 - steps[1]["loss"]) <= 1e-5 * abs(loss2)
    got = eng.export_keras_params()
    for n, w in want_p.items():
        assert float(np.abs(got[n].double().numpy() - w).max()) <= P_ATOL, n
    assert impl.vq.n_fwd == 2 and impl.vq.n_bwd == 2
    if overlap:
        assert len(tr.bucketer.bounds) > 3 and rt.n_cross_stream > 50
    else:
        assert rt.n_cross_stream == 0


def test_op_list_is_the_graph_of_vqvae_py(monkeypatch):
    """Encoder: 4 x (conv, bn) | embedding, reshape, per-position dense, reshape | concat, dense, dropout, pad, conv 1x1, vq;
    decoder: 4 x (convT, bn), output layer - no Dense, Dropout or Reshape at its entry."""
    import unet_rir_amd as U
    rt, impl = _install(monkeypatch)
    B = 2
    cfg, params, eng, tr = _build(rt, B, False)
    n = len(cfg.conv_filters)
    assert eng._n_enc_ops == 2 * n + 4 + 6 and len(eng.ops) == eng._n_enc_ops + 2 * n + 1
    assert eng.MASKS == ("bottleneck", None) and list(eng.masks) == ["bottleneck"] and eng.n_dropout_draws == 1
    h, w, c = cfg.bottleneck_shape()
    assert eng.mask_width == {"bottleneck": h * w * 2}
    assert eng._latent_shape() == (B, h, w, c) and eng.vq_indices.numel() == B * h * w * c // cfg.latent_space_dim
    names = list(eng.specs)                                   # backward-completion order: decoder first, the codebook before conv2d
    assert names.index("decoder_conv_transpose_layer_0.kernel") < names.index("vector_quantizer.embeddings") < names.index("conv2d.kernel")
    assert eng.specs["encoder_inf_dense.kernel"].kind == "dense" and eng.specs["conv2d.kernel"].kind == "conv_padin"
    assert eng.specs["embedding"].shape == (1500, 128)
    # the reference's own size (dl_models/vqvae.py:522-531) is what an engine built without arguments has
    assert U.VQVAEEngine.DEFAULTS == ((32, 64, 128, 256), 16, 320)
    # operators of one step, in the stand-ins' log: one quantiser forward, one backward
    batch = tuple(torch.tensor(a) for a in _batch(B))
    tr.step(*batch)
    assert impl.vq.n_fwd == 1 and impl.vq.n_bwd == 1


@pytest.mark.parametrize("dropout", [False, True])
def test_one_dropout_draw_per_step(monkeypatch, dropout):
    rt, impl = _install(monkeypatch)
    B = 2
    cfg, params, eng, tr = _build(rt, B, False, dropout=dropout, lr=0.0)
    batch = tuple(torch.tensor(a) for a in _batch(B))
    for _ in range(3):
        tr.step(*batch)
    assert eng._shared["dropout_step"] == (3 if dropout else 0)
    assert (eng.masks["bottleneck"] is not None) == dropout


def test_codebook_is_a_parameter_in_a_bucket_and_shared(monkeypatch):
    rt, impl = _install(monkeypatch)
    B = 2
    cfg, params, eng, tr = _build(rt, B, True, bucket_bytes=8192)
    s = eng.specs["vector_quantizer.embeddings"]
    assert s.shape == (cfg.latent_space_dim, cfg.conv_filters[-1]) and s.kind == "codebook"
    assert eng.p[s.name].data_ptr() == eng.theta[s.offset:].data_ptr()
    bounds = [0] + list(tr.bucketer.bounds)
    assert any(lo <= s.offset and s.end <= hi for lo, hi in zip(bounds[:-1], bounds[1:])), (bounds, s.offset, s.end)
    before = eng.p[s.name].clone()
    tr.step(*(torch.tensor(a) for a in _batch(B)))
    assert not torch.equal(before, eng.p[s.name])                       # Adam moved it
    assert float(eng.adam_m[s.offset:s.offset + s.numel].abs().max()) > 0
    _, _, other, _ = _build(rt, 3, True, share=eng)
    assert other.p[s.name].data_ptr() == eng.p[s.name].data_ptr() and other.vq_indices.numel() * 2 == eng.vq_indices.numel() * 3
    # the initialiser: U(-0.05, 0.05) (tf.random_uniform_initializer, dl_models/vqvae.py:52)
    eng.reset_parameters(torch.Generator().manual_seed(2))
    cb = eng.p[s.name]
    assert float(cb.min()) >= -0.05 and float(cb.max()) <= 0.05 and float(cb.abs().max()) > 0.04 and float(cb.mean().abs()) < 0.02


def test_encode_and_decode_are_the_two_halves_of_forward(monkeypatch):
    rt, impl = _install(monkeypatch)
    B = 2
    cfg, params, eng, tr = _build(rt, B, False)
    spec_in, emb, _ = (torch.tensor(a) for a in _batch(B))
    mask = torch.tensor(_mask(B)).view(B, 1, 1, -1)
    pred = eng.forward(spec_in, emb, dropout_mask=mask).clone()
    y = eng.encode(spec_in, emb, mask)
    h, w, c = cfg.bottleneck_shape()
    assert tuple(y.shape) == (B, h, w, c)
    E = eng.p["vector_quantizer.embeddings"]
    q = E.t()[eng.vq_indices.long()].reshape(y.shape)
    assert float((y - q).abs().max()) <= 1e-6                           # x + (q - x): the code, to rounding
    assert torch.equal(eng.decode(y), pred)
    with pytest.raises(ValueError):
        eng.decode(torch.zeros((B, c)))
    eng.training = False                                               # inference quantises too (no `training` switch)
    n0 = impl.vq.n_fwd
    eng.forward(spec_in, emb)
    assert impl.vq.n_fwd == n0 + 1
    with pytest.raises(NotImplementedError):
        eng.loss_from_logits(spec_in)


def test_fit_records_carry_the_vq_metric(monkeypatch):
    """lr = 0 keeps the parameters, the batch statistics are the batch's: every step sees the same S."""
    import unet_rir_amd as U
    rt, impl = _install(monkeypatch)
    B = 2
    cfg, params, eng, tr = _build(rt, B, False, lr=0.0)
    batch = tuple(torch.tensor(a) for a in _batch(B))
    hist = U.fit(tr, lambda ep: [batch, batch, batch], 1, val_batches=lambda ep: [batch, batch], log=None)
    rec = hist[0]
    mean_sq = float(eng.vq_out[1]) / eng.vq_elems
    assert mean_sq > 0 and abs(rec["train_vq"] - mean_sq) <= 1e-6 * mean_sq and abs(rec["val_vq"] - mean_sq) <= 1e-6 * mean_sq
    assert {"train_vq", "val_vq"} <= set(rec) and "train_kl" not in rec
    assert abs(rec["train_loss"] - rec["val_loss"]) <= 1e-5 * rec["val_loss"]

"""tests/diffunet_ref.py and tests/diffvae_ref.py held to finite differences and to their siblings: diffunet_ref with the vector block
and the head swapped for AENet's must reproduce tests/aenet_ref.py; diffvae_ref with the flattened vector branch and a sigmoid must
reproduce tests/vae_ref.py."""
import numpy as np
import torch

import aenet_ref as A
import diffunet_ref as DU
import diffvae_ref as DV
import vae_ref as V
from oracle import torch_ref as R

D = torch.float64


def _fd(f, params, names, eps=1e-6, n_probe=3, seed=0):
    """Central differences of the scalar f(params) in a few entries of each named parameter."""
    rs = np.random.RandomState(seed)
    out = {}
    for n in names:
        a = params[n]
        res = []
        for _ in range(n_probe):
            idx = tuple(int(rs.randint(s)) for s in a.shape)
            keep = a[idx]
            a[idx] = keep + eps; up = f(params)
            a[idx] = keep - eps; dn = f(params)
            a[idx] = keep
            res.append((idx, (up - dn) / (2 * eps)))
        out[n] = res
    return out


def test_diffunet_ref_shapes_and_finite_differences():
    cfg = DU.config(32, 48, 4, 3, True)
    shapes = DU.param_shapes(cfg)
    assert shapes["vec.embedding"] == (1500, 128) and shapes["encoder_inf_dense.kernel"] == (32 * 128, 2 * 3 * 64)
    assert shapes["head.kernel"] == (1, 1, 4, 2) and not any(n.startswith(("rec.", "vec.dense")) for n in shapes)
    assert shapes["enc1.down.kernel"] == (2, 2, 2, 4) and shapes["dec1.up.kernel"] == (2, 2, 4, 8)
    assert len(DU.l2_regularized(cfg)) == 9
    params = DU.init_params(cfg, "fd")
    batch = R.synthetic_batch(cfg, 2, "fd/d")
    rs = np.random.RandomState(3)
    masks = (((rs.uniform(size=(2, DU.vec_units(cfg))) >= 0.5) / 0.5),)
    loss, data, pred, z, grads = DU.loss_and_grads(params, *batch, cfg, masks, diff_loss=True)
    assert torch.equal(pred, z)                                    # activation='linear'
    assert float((pred < 0).double().mean()) > 0.02 or float((pred > 1).double().mean()) > 0.02
    f = lambda p: DU.loss_and_grads(p, *batch, cfg, masks, diff_loss=True)[0]
    names = ["enc1.down.kernel", "enc3.fb.c3.kernel", "vec.embedding", "encoder_inf_dense.kernel", "encoder_inf_dense.bias", "dec2.up.kernel",
             "dec1.fb.c2.gamma", "head.kernel", "head.bias"]
    gmax = max(float(g.abs().max()) for g in grads.values())
    hit = 0
    for n, res in _fd(f, params, names).items():
        for idx, num in res:
            an = float(grads[n][idx])
            assert abs(num - an) <= 1e-5 * abs(an) + 1e-7 * gmax, (n, idx, num, an)
            hit += an != 0.0
    assert hit >= len(names)


def _aenet_join(P, x, emb, masks, q):
    """AENet's bottleneck (dl_models/ae_net.py:224-228, :253-268), as tests/aenet_ref.py states it."""
    B, cL, h5, w5 = x.shape
    v = P["vec.embedding"][emb.long()].reshape(B, -1) @ P["vec.dense.kernel"] + P["vec.dense.bias"]
    if masks is not None:
        v = v * masks[0].reshape(B, -1)
    lat = torch.cat([x.permute(0, 2, 3, 1).reshape(B, -1), v], dim=1)
    r = lat @ P["rec.dense.kernel"] + P["rec.dense.bias"]
    if masks is not None:
        r = r * masks[1].reshape(B, -1)
    r = r.view(B, h5, w5, 2).permute(0, 3, 1, 2)
    return q(R.conv2d_same(r, P["rec.conv.kernel"], P["rec.conv.bias"], 1))


def _aenet_head(P, x, storage, qw, head_storage=None):
    z = R.conv2d_same(x, qw(P["head.kernel"]), P["head.bias"], 1)
    return R._QuantBwd.apply(z) if storage == "bf16" else z


def test_diffunet_ref_with_aenets_vector_block_and_head_is_aenet_ref():
    for mode, bn, storage in ((0, True, None), (3, False, None), (0, True, "bf16")):
        cfg = A.config(32, 48, 8, mode, bn)
        params = A.init_params(cfg, "sib")
        batch = R.synthetic_batch(cfg, 2, "sib/d")
        rs = np.random.RandomState(1)
        masks = tuple(((rs.uniform(size=(2, n)) >= 0.5) / 0.5) for n in (A.VEC_UNITS, 2 * 3 * 2))
        want = A.loss_and_grads(params, *batch, cfg, masks, storage=storage)
        got = DU.loss_and_grads(params, *batch, cfg, masks, storage=storage, join=_aenet_join, head=_aenet_head,
                                out_act=lambda z: torch.clamp(z, 0.0, 1.0))
        assert got[0] == want[0] and got[1] == want[1] and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
        for n, g in want[4].items():
            assert torch.equal(got[4][n], g), n


def _vae_case(per_position):
    cfg = DV.config(32, 48, (8, 16), (3, 3), (2, 2), 8, 12)
    params = DV.init_params(cfg, "dv", randomize_all=True, dtype=np.float64, per_position=per_position)
    base = R.Config(32, 48)
    spec_in, emb, spec_out = R.synthetic_batch(base, 2, "dv/d")
    rs = np.random.RandomState(5)
    eps = rs.standard_normal((2, 8))
    h, w, c = cfg.bottleneck_shape()
    mask = (rs.uniform(size=(2, h * w * c)) >= 0.3) / 0.7
    return cfg, params, (spec_in, emb % (1500 if per_position else 2000), spec_out), eps, mask


def test_diffvae_ref_shapes_and_finite_differences():
    cfg, params, batch, eps, mask = _vae_case(True)
    shapes = DV.param_shapes(cfg)
    h, w, c = cfg.bottleneck_shape()
    assert shapes["embedding"] == (1500, 128) and shapes["encoder_inf_dense.kernel"] == (128, 12)
    assert shapes["mu.kernel"] == (h * w * c + 32 * 12, 8) and shapes["log_variance.kernel"] == shapes["mu.kernel"]
    full = DV.config(144, 128)
    assert (full.conv_filters, full.latent_space_dim, full.n_neurons) == ((32, 64, 128, 256), 16, 1280)
    inter = {}
    loss, dl, kl, pred, grads = DV.loss_and_grads(params, *batch, cfg, eps, mask_dec=mask, inter=inter, diff_loss=True)
    assert torch.equal(pred, inter["logits"]) and abs(loss - (dl + kl)) <= 1e-12 * abs(loss) and kl > 0
    assert float((pred < 0).double().mean()) > 0.02
    f = lambda p: DV.loss_and_grads(p, *batch, cfg, eps, mask_dec=mask, diff_loss=True)[0]
    names = ["encoder_conv_layer_1.kernel", "encoder_bn_2.gamma", "embedding", "encoder_inf_dense.kernel", "encoder_inf_dense.bias", "mu.kernel",
             "log_variance.bias", "decoder_dense.kernel", "decoder_conv_transpose_layer_1.kernel", "decoder_out_2.kernel", "decoder_out_2.bias"]
    gmax = max(float(g.abs().max()) for g in grads.values())
    for n, res in _fd(f, params, names).items():
        for idx, num in res:
            an = float(grads[n][idx])
            assert abs(num - an) <= 1e-5 * abs(an) + 1e-7 * gmax, (n, idx, num, an)


def test_diffvae_ref_with_the_flattened_vector_branch_and_a_sigmoid_is_vae_ref():
    cfg, params, batch, eps, mask = _vae_case(False)
    assert DV.param_shapes(cfg, per_position=False) == V.param_shapes(cfg)
    want = V.loss_and_grads(params, *batch, cfg, eps, mask_dec=mask)
    got = DV.loss_and_grads(params, *batch, cfg, eps, mask_dec=mask, per_position=False, out_act=torch.sigmoid)
    assert got[:3] == want[:3] and torch.equal(got[3], want[3])
    for n, g in want[4].items():
        assert torch.equal(got[4][n], g), n


def test_bf16_storage_mode_rounds_and_stays_close():
    cfg = DU.config(32, 48, 8, 0, True)
    params = DU.init_params(cfg, "q")
    batch = R.synthetic_batch(cfg, 2, "q/d")
    exact = DU.loss_and_grads(params, *batch, cfg)
    for hs in ("f32", "bf16"):
        q = DU.loss_and_grads(params, *batch, cfg, storage="bf16", head_storage=hs)
        rel = float((q[2] - exact[2]).norm() / exact[2].norm())
        assert 0.0 < rel < 0.05, (hs, rel)
    cfgv, pv, bv, eps, mask = _vae_case(True)
    ex = DV.loss_and_grads(pv, *bv, cfgv, eps, mask_dec=mask)
    qv = DV.loss_and_grads(pv, *bv, cfgv, eps, mask_dec=mask, storage="bf16")
    rel = float((qv[3] - ex[3]).norm() / ex[3].norm())
    assert 0.0 < rel < 0.05, rel
    assert torch.equal(qv[3], qv[3].to(torch.bfloat16).double())             # the output layer stores bf16

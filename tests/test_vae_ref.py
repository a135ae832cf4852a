"""Checks of the fp64 restatement of the VAE (tests/vae_ref.py) itself: the analytic gradients of the sampling + KL stage that the
HIP backward kernel implements, a finite-difference check of the whole loss, and the size of the reference's configuration."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_ref as V  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

D = torch.float64


def test_analytic_sample_kl_gradients_equal_autograd():
    """dmu = dz + mu / gb and dlv = dz 0.5 exp(0.5 lv) eps + 0.5 (exp(lv) - 1) / gb are the gradients of
    <dz, z> + KL / gb with z = mu + exp(0.5 lv) eps - for any upstream dz."""
    g = torch.Generator().manual_seed(11)
    B, L, gb = 3, 8, 6
    mu = torch.randn((B, L), generator=g, dtype=D).requires_grad_(True)
    lv = (torch.rand((B, L), generator=g, dtype=D) * 6 - 4).requires_grad_(True)
    eps = torch.randn((B, L), generator=g, dtype=D)
    dz = torch.randn((B, L), generator=g, dtype=D)
    obj = (V.sample(mu, lv, eps) * dz).sum() + V.kl_loss(mu, lv, gb)
    gmu, glv = torch.autograd.grad(obj, (mu, lv))
    dmu, dlv = V.sample_kl_grads(mu.detach(), lv.detach(), eps, dz, 1.0 / gb)
    assert float((gmu - dmu).abs().max()) <= 1e-14 * float(gmu.abs().max())
    assert float((glv - dlv).abs().max()) <= 1e-14 * float(glv.abs().max())
    # the metric's mean and the loss term are two normalisations of one sum
    assert abs(float(V.kl_elements(mu, lv).sum()) / gb - float(V.kl_loss(mu, lv, gb))) <= 1e-12


def _tiny():
    cfg = V.VAEConfig(16, 16, (4, 8), (3, 3), (2, 2), 4, 8)
    params = V.init_params(cfg, randomize_all=True, dtype=np.float64)
    B = 3
    spec_in, emb, spec_out = R.synthetic_batch(R.Config(16, 16), B)
    g = torch.Generator().manual_seed(5)
    eps = torch.randn((B, cfg.latent_space_dim), generator=g, dtype=D).numpy()
    h, w, c = cfg.bottleneck_shape()
    mask = ((torch.rand((B, h * w * c), generator=g) >= V.DROPOUT_P).double() / (1 - V.DROPOUT_P)).numpy()
    return cfg, params, (spec_in, emb, spec_out), eps, mask


def test_whole_loss_by_finite_differences():
    """Central differences of loss = compute_loss + compute_kl_loss along random directions of several tensors (the heads, a
    convolution on either side of the bottleneck, a BatchNorm scale, the embedding): the autograd gradient's projection agrees to
    the second-order error of the difference quotient."""
    cfg, params, batch, eps, mask = _tiny()
    gb = 6                                               # a global batch that is not this replica's batch
    loss, dl, kl, pred, grads = V.loss_and_grads(params, *batch, cfg, eps, 0.9, gb, mask)
    assert abs(loss - (dl + kl)) <= 1e-15 * abs(loss) and kl > 0
    rng = np.random.RandomState(3)
    for name in ("mu.kernel", "log_variance.kernel", "log_variance.bias", "encoder_conv_layer_2.kernel", "decoder_bn_0.gamma",
                 "decoder_conv_transpose_layer_1.kernel", "decoder_dense.kernel", "embedding"):
        d = rng.standard_normal(params[name].shape)
        d /= np.linalg.norm(d)
        h = 1e-5
        lp = V.loss_and_grads({**params, name: params[name] + h * d}, *batch, cfg, eps, 0.9, gb, mask)[0]
        lm = V.loss_and_grads({**params, name: params[name] - h * d}, *batch, cfg, eps, 0.9, gb, mask)[0]
        fd = (lp - lm) / (2 * h)
        an = float((grads[name] * torch.tensor(d)).sum())
        scale = float(grads[name].norm())
        assert abs(fd - an) <= 1e-6 * scale + 1e-9, (name, fd, an)


def test_kl_term_is_divided_by_the_global_batch():
    cfg, params, batch, eps, mask = _tiny()
    _, dl1, kl1, _, _ = V.loss_and_grads(params, *batch, cfg, eps, 0.9, 3, mask)
    _, dl2, kl2, _, _ = V.loss_and_grads(params, *batch, cfg, eps, 0.9, 6, mask)
    assert abs(kl1 - 2 * kl2) <= 1e-13 * kl1 and abs(dl1 - 2 * dl2) <= 1e-13 * dl1


def test_param_count_of_the_reference_configuration():
    """main_training.py:143-152 at 144 x 160 (bottleneck 9 x 10 x 512 = 46080 features), trainable variables:
      encoder convolutions + BatchNorm   (3*3*2*64 + 64 + 128) + (9*64*128 + 128 + 256) + (9*128*256 + 256 + 512)
                                         + (9*256*512 + 512 + 1024)        = 1344 + 74112 + 295680 + 1181184 =  1 552 320
      embedding 2000 * 256                                                                                  =    512 000
      encoder_inf_dense (2*16*256) * 2048 + 2048                                                            = 16 779 264
      mu, log_variance   2 * ((46080 + 2048) * 64 + 64)                                                     =  6 160 512
      decoder_dense 64 * 46080 + 46080                                                                      =  2 995 200
      decoder_conv_transpose_layer_0..3 + BatchNorm   (9*512*512 + 512 + 1024) + (9*256*512 + 256 + 512)
                                         + (9*128*256 + 128 + 256) + (9*64*128 + 64 + 128)
                                         = 2360832 + 1180416 + 295296 + 73920                               =  3 910 464
      decoder_out_4  9*2*64 + 2                                                                             =      1 154
                                                                                                      total = 31 910 914"""
    shapes = V.param_shapes(V.VAEConfig(144, 160))
    assert sum(int(np.prod(s)) for s in shapes.values()) == 31_910_914
    assert list(shapes)[:4] == ["encoder_conv_layer_1.kernel", "encoder_conv_layer_1.bias", "encoder_bn_1.gamma", "encoder_bn_1.beta"]
    assert list(shapes).index("mu.kernel") < list(shapes).index("log_variance.kernel") < list(shapes).index("decoder_dense.kernel")

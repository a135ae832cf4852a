"""Checks of the fp64 restatement of the VQ-VAE (tests/vqvae_ref.py) itself - the pin of this model, since TensorFlow does not run
here: the hand-written gradients of the quantiser that the HIP backward kernels implement equal torch autograd of the literal
expressions of dl_models/vqvae.py:61-98; finite differences agree where the best-to-second margin is large (away from index flips);
ties pick the lowest index; the size of the reference's configuration."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vqvae_ref as Q  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

D = torch.float64


def _layer(seed=7, shape=(2, 3, 2, 8), Dv=4, K=6):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g, dtype=D) * 0.4 - 0.2)
    E = (torch.rand((Dv, K), generator=g, dtype=D) * 0.1 - 0.05)
    dy = torch.randn(shape, generator=g, dtype=D)
    return x, E, dy


def test_handwritten_quantiser_gradients_equal_autograd_of_the_literal_expressions():
    for r in (1.0, 0.5):
        x, E, dy = _layer()
        E[:, 4] = 1.0                                                    # a code far from every input: nobody chooses it
        x.requires_grad_(True); E.requires_grad_(True)
        y, vq, idx = Q.quantize_literal(x, E)
        gx, gE = torch.autograd.grad((y * dy).sum() + r * vq, (x, E))
        y2, term, S, idx2 = Q.quantize(x.detach(), E.detach(), Q.BETA, r)
        assert torch.equal(idx, idx2) and len(set(idx.tolist())) < E.shape[1] and len(set(idx.tolist())) > 1
        assert float((y.detach() - y2).abs().max()) <= 1e-16
        assert abs(float(term) - r * float(vq.detach())) <= 1e-15 * float(vq.detach())
        assert abs(float(S) / x.numel() * (1 + Q.BETA) - float(vq.detach())) <= 1e-15 * float(vq.detach())
        dx, dE = Q.quantize_grads(x.detach(), E.detach(), idx, dy, Q.BETA, r)
        assert float((gx - dx).abs().max()) <= 1e-14 * float(gx.abs().max())
        assert float((gE - dE).abs().max()) <= 1e-14 * float(gE.abs().max())
        unused = [k for k in range(E.shape[1]) if k not in set(idx.tolist())]
        assert unused and all(bool((dE[:, k] == 0).all()) for k in unused)            # exactly 0, not small


def test_given_indices_are_taken_as_given():
    x, E, dy = _layer()
    idx = torch.arange(x.numel() // E.shape[0]) % E.shape[1]
    y, term, S, got = Q.quantize(x, E, indices=idx)
    assert torch.equal(got, idx)
    assert float((y - (x + (E.t()[idx].reshape(x.shape) - x))).abs().max()) == 0.0
    yl, vq, gl = Q.quantize_literal(x, E, indices=idx)
    assert torch.equal(gl, idx) and abs(float(vq) - float(term)) <= 1e-15 * float(vq)


def test_ties_pick_the_lowest_index():
    g = torch.Generator().manual_seed(3)
    E = torch.randint(-3, 4, (4, 8), generator=g).to(D)
    E[:, 5] = E[:, 2]; E[:, 7] = E[:, 2]; E[:, 6] = E[:, 1]            # duplicated columns: exact ties
    x = E.t()[[5, 7, 2, 6, 1, 5]].clone()                                # each vector IS a code (distance exactly 0)
    assert Q.code_indices(x, E).tolist() == [2, 2, 2, 1, 1, 2]
    mid = (E[:, 0] + E[:, 3]) / 2                                       # halfway between two codes: equal distances (exact in fp64)
    d = Q.distances(mid[None], E)[0]
    if float(d[0]) == float(d[3]) == float(d.min()):
        assert int(Q.code_indices(mid[None], E)[0]) == 0


def _tiny(n_replicas=1):
    cfg = Q.VQVAEConfig(16, 32, (4, 8), (3, 3), (2, 2), 4, 8)
    params = Q.init_params(cfg, randomize_all=True, dtype=np.float64, codebook_scale=8.0)
    B = 3
    spec_in, emb, spec_out = R.synthetic_batch(R.Config(16, 32), B)
    g = torch.Generator().manual_seed(5)
    h, w, c = cfg.bottleneck_shape()
    mask = ((torch.rand((B, h * w * 2), generator=g) >= Q.DROPOUT_P).double() / (1 - Q.DROPOUT_P)).numpy()
    return cfg, params, (spec_in, emb % Q.VOCAB, spec_out), mask


def test_whole_loss_by_finite_differences_away_from_index_flips():
    """Central differences of loss = compute_loss + vq term / replicas along random directions of several tensors on both sides of
    the quantiser and of the codebook itself.  What backpropagation through the stop_gradients yields is the true gradient of the
    function in which they hold constants (vqvae_ref.quantize_literal(frozen=)): differences are taken of that one, at a point
    whose best-to-second margin is so large that no vector changes its code within +-h (asserted, also on the searched indices
    of both displaced points)."""
    cfg, params, batch, mask = _tiny()
    gb, nrep = 6, 2
    inter = {}
    loss, dl, term, pred, grads = Q.loss_and_grads(params, *batch, cfg, 0.9, gb, mask, nrep, inter=inter)
    assert abs(loss - (dl + term)) <= 1e-15 * abs(loss) and term > 0
    E = torch.tensor(params[Q.CODEBOOK])
    dist = Q.distances(inter["x"].reshape(-1, cfg.latent_space_dim), E)
    two = torch.topk(dist, 2, dim=1, largest=False).values
    margin = float((two[:, 1] - two[:, 0]).min())
    assert margin > 1e-4, margin                                         # h = 1e-6 moves a distance by ~1e-6: no flip
    assert len(set(inter["idx"].tolist())) > 1
    x0 = inter["x"]
    frozen = {"x": x0, "q": E.t()[inter["idx"]].reshape(x0.shape)}
    rng = np.random.RandomState(3)
    h = 1e-6
    for name in (Q.CODEBOOK, "conv2d.kernel", "dense.kernel", "encoder_inf_dense.kernel", "encoder_conv_layer_2.kernel", "embedding",
                 "decoder_bn_0.gamma", "decoder_conv_transpose_layer_0.kernel"):
        d = rng.standard_normal(params[name].shape)
        d /= np.linalg.norm(d)
        ip, im = {}, {}
        lp = Q.loss_and_grads({**params, name: params[name] + h * d}, *batch, cfg, 0.9, gb, mask, nrep, inter=ip, frozen=frozen)[0]
        lm = Q.loss_and_grads({**params, name: params[name] - h * d}, *batch, cfg, 0.9, gb, mask, nrep, inter=im, frozen=frozen)[0]
        assert torch.equal(ip["idx"], inter["idx"]) and torch.equal(im["idx"], inter["idx"]), name      # searched, not given
        fd = (lp - lm) / (2 * h)
        an = float((grads[name] * torch.tensor(d)).sum())
        scale = float(grads[name].norm())
        assert scale > 0, name
        assert abs(fd - an) <= 1e-5 * scale + 1e-9, (name, fd, an)


def test_vq_term_is_divided_by_the_replicas_not_by_the_batch():
    cfg, params, batch, mask = _tiny()
    _, dl1, t1, _, _ = Q.loss_and_grads(params, *batch, cfg, 0.9, 3, mask, 1)
    _, dl2, t2, _, _ = Q.loss_and_grads(params, *batch, cfg, 0.9, 6, mask, 2)
    assert abs(t1 - 2 * t2) <= 1e-13 * t1 and abs(dl1 - 2 * dl2) <= 1e-13 * dl1
    _, _, t3, _, _ = Q.loss_and_grads(params, *batch, cfg, 0.9, 6, mask, 1)
    assert t3 == t1


def test_param_count_of_the_reference_configuration():
    """dl_models/vqvae.py:522-531 at 160 x 144 (bottleneck 10 x 9 x 256), trainable variables:
      encoder convolutions + BatchNorm   (9*2*32 + 32 + 64) + (9*32*64 + 64 + 128) + (9*64*128 + 128 + 256) + (9*128*256 + 256 + 512)
                                         = 672 + 18624 + 74112 + 295680                                     =    389 088
      embedding 1500 * 128                                                                                  =    192 000
      encoder_inf_dense 128 * 320 + 320                                                                     =     41 280
      dense (23040 + 32 * 320) * 180 + 180                                                                  =  5 990 580
      conv2d 2 * 256 + 256                                                                                  =        768
      vector_quantizer.embeddings 16 * 256                                                                  =      4 096
      decoder_conv_transpose_layer_0..3 + BatchNorm   (9*256*256 + 256 + 512) + (9*128*256 + 128 + 256) + (9*64*128 + 64 + 128)
                                         + (9*32*64 + 32 + 64) = 590592 + 295296 + 73920 + 18528            =    978 336
      decoder_out_4  9*2*32 + 2                                                                             =        578
                                                                                                      total =  7 596 726"""
    shapes = Q.param_shapes(Q.VQVAEConfig(160, 144))
    assert sum(int(np.prod(s)) for s in shapes.values()) == 7_596_726
    names = list(shapes)
    assert names.index("conv2d.kernel") < names.index(Q.CODEBOOK) < names.index("decoder_conv_transpose_layer_0.kernel")
    assert "decoder_dense.kernel" not in shapes

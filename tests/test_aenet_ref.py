"""tests/aenet_ref.py held to three properties (no GPU): finite differences on a handful of parameters per layer kind, the 2x2
stride-2 convolution equal to space-to-depth + matmul with the transposed layer as its adjoint, and the default model's shapes."""
import numpy as np
import torch

import aenet_ref as A
from oracle import detrand, torch_ref as R

D64 = torch.float64


def test_conv2x2_is_space_to_depth_matmul_and_the_transpose_is_its_adjoint():
    B, Ci, Co, Hh, Ww = 2, 3, 5, 6, 10
    x = torch.tensor(detrand.uniform("a/x", (B, Ci, Hh, Ww), -1, 1, np.float64))
    w = torch.tensor(detrand.uniform("a/w", (2, 2, Ci, Co), -1, 1, np.float64))          # HWIO
    y = torch.tensor(detrand.uniform("a/y", (B, Co, Hh // 2, Ww // 2), -1, 1, np.float64))
    zero_o, zero_i = torch.zeros(Co, dtype=D64), torch.zeros(Ci, dtype=D64)
    conv = R.conv2d_same(x, w, zero_o, 2)
    # space to depth: [B, H/2, W/2, (kh, kw, c)] @ [(kh, kw, c), Co]
    s2d = x.view(B, Ci, Hh // 2, 2, Ww // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(B, Hh // 2, Ww // 2, 4 * Ci)
    assert torch.allclose(conv, (s2d @ w.reshape(4 * Ci, Co)).permute(0, 3, 1, 2), rtol=0, atol=1e-13)
    # Conv2DTranspose with the kernel read as HWOI (O = Ci here) is the adjoint: <conv(x), y> == <x, convT(y)>
    back = R.conv2d_transpose_same(y, w, zero_i, 2)
    assert abs(float((conv * y).sum()) - float((x * back).sum())) <= 1e-12 * float(conv.abs().sum())


def test_default_model_shapes():
    for (H, W) in ((144, 160), (144, 304)):
        cfg = A.config(H, W)
        sh = A.param_shapes(cfg)
        h5, w5 = H // 16, W // 16
        assert sh["enc1.down.kernel"] == (2, 2, 2, 32) and sh["enc5.down.kernel"] == (2, 2, 256, 512)
        assert sh["vec.embedding"] == (2500, 256) and sh["vec.dense.kernel"] == (32 * 256, 2048)
        assert sh["rec.dense.kernel"] == (h5 * w5 * 512 + 2048, h5 * w5 * 2) and sh["rec.conv.kernel"] == (1, 1, 2, 512)
        assert sh["dec4.up.kernel"] == (2, 2, 256, 512) and sh["dec1.cb1a.kernel"] == (3, 3, 64, 32) and sh["head.kernel"] == (6, 6, 32, 2)
    assert (144 // 16) * (160 // 16) * 512 + 2048 == 48128 and 9 * 10 * 2 == 180
    cfg = A.config(32, 48, 4)
    P = R.to_torch(A.init_params(cfg), D64)
    spec, emb, _ = R.synthetic_batch(cfg, 2, "a/d")
    out = A.forward(P, torch.tensor(spec, dtype=D64), torch.tensor(emb), cfg)
    assert tuple(out.shape) == (2, 2, 32, 48) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0


def test_gradients_against_finite_differences():
    """Central differences in fp64 on three entries of one parameter per layer kind, modes 0 and 3.  The loss is piecewise smooth
    (ReLUs, the output clip): the logits are checked to stay away from 0 and 1, and the probe is 1e-8 so that none of the ~3e5 ReLU
    inputs of this fixed batch crosses zero inside it (at 1e-6 one does, and the difference quotient is off by 1e-3); rounding then
    costs 0.2 * 2^-52 / 2e-8 = 2e-9 of absolute error, which the bound allows for."""
    for mode in (0, 3):
        cfg = A.config(32, 48, 4, mode)
        params = A.init_params(cfg, f"fd{mode}")
        spec_in, emb, spec_out = R.synthetic_batch(cfg, 2, "fd/d")
        g = torch.Generator().manual_seed(1)
        masks = tuple(((torch.rand((2, n), generator=g) >= 0.5).double() / 0.5).numpy() for n in (A.VEC_UNITS, 2 * 3 * 2))
        loss, _, _, z, grads = A.loss_and_grads(params, spec_in, emb, spec_out, cfg, masks)
        assert float(torch.minimum(z.abs(), (z - 1).abs()).min()) > 1e-6
        names = ["enc1.down.kernel", "enc3.down.kernel", "enc2.down.bias", "vec.dense.kernel", "rec.dense.kernel", "rec.conv.kernel",
                 "dec2.up.kernel", "dec3.up.bias", "dec1.cb1a.kernel", "dec1.cb1a.gamma", "head.kernel", "head.bias",
                 "enc4.cb1.beta" if mode == 0 else "enc4.fb.c3.beta"]
        eps = 1e-8
        for n in names:
            flat = grads[n].reshape(-1)
            for i in torch.topk(flat.abs(), min(3, flat.numel())).indices.tolist():
                vals = []
                for sgn in (1, -1):
                    p2 = {k: v.copy() for k, v in params.items()}
                    p2[n].reshape(-1)[i] += sgn * eps
                    vals.append(A.loss_and_grads(p2, spec_in, emb, spec_out, cfg, masks)[0])
                fd = (vals[0] - vals[1]) / (2 * eps)
                assert abs(fd - float(flat[i])) <= 1e-5 * abs(float(flat[i])) + 5e-9, (mode, n, i, fd, float(flat[i]))

"""AENet (dl_models/ae_net.py:197-268) restated in torch, fp64 by default, from the source text: configuration, parameters in Keras
shapes, forward, the loss with the clipped-ReLU output, gradients by autograd of the literal expressions.  Test infrastructure only.
The convolutions are oracle.torch_ref.conv2d_same / conv2d_transpose_same (generic in k); convolutional_block_1 and the feature
blocks are the U-Net's (ae_net.py:327-399 repeats u_net.py:324-386 word for word).  Parameter names are the engine's.

  encoder   level 1 Conv2D(F0, 2, strides=1, 'same') (resize_factor_0 = [1, 1]: TF pads bottom / right by 1), levels 2-5
            Conv2D(2, strides=2); each followed by the feature block of `mode`; l2(0.001) on these kernels (:273-279)
  vector    Embedding(2500, 256) -> Flatten -> Dense(64 * 32) -> Dropout(.5) (:263-268)
  join      concatenate([Flatten(enc5) (NHWC order), vector]) -> Dense(h5 w5 2) -> Dropout(.5) -> Reshape((h5, w5, 2)) ->
            Conv2D(16 F0, 1x1) (:224-228, :253-261)
  decoder   Conv2DTranspose(2, strides=2, l2) -> concatenate([skip, x]) -> convolutional_block_1 -> feature block (:295-325)
  output    UpSampling2D((1, 1)) = identity, Conv2D(2, (6, 6), 'same'), relu(out, alpha=0, max_value=1) (:247-249)
"""
import math

import numpy as np
import torch

from oracle import detrand, torch_ref as R

VOCAB, EMB_DIM, VEC_UNITS = 2500, 256, 64 * 32
DROPOUT_P = 0.5
L2_COEF = 0.001


def config(H, W, F0=32, mode=0, batchnorm=True):
    if H % 16 or W % 16:
        raise ValueError("H and W must be multiples of 16")
    return R.Config(H, W, F0=F0, k=2, depth=4, batchnorm=batchnorm, mode=mode)


def param_shapes(cfg):
    shapes, ch, cin = {}, cfg.enc_channels(), 2

    def unit(name, c, c_in=None):
        shapes[name + ".kernel"] = (3, 3, c if c_in is None else c_in, c)
        shapes[name + ".bias"] = (c,)
        if cfg.batchnorm:
            shapes[name + ".gamma"] = (c,)
            shapes[name + ".beta"] = (c,)
    for l, c in enumerate(ch, start=1):
        shapes[f"enc{l}.down.kernel"] = (2, 2, cin, c)
        shapes[f"enc{l}.down.bias"] = (c,)
        for u in R._feature_block_names(cfg, f"enc{l}"):
            unit(u, c)
        cin = c
    h5, w5 = cfg.H // 16, cfg.W // 16
    n_idx = int(np.prod(cfg.inf_vector_shape))
    shapes["vec.embedding"] = (VOCAB, EMB_DIM)
    shapes["vec.dense.kernel"] = (n_idx * EMB_DIM, VEC_UNITS)
    shapes["vec.dense.bias"] = (VEC_UNITS,)
    shapes["rec.dense.kernel"] = (h5 * w5 * ch[-1] + VEC_UNITS, h5 * w5 * 2)
    shapes["rec.dense.bias"] = (h5 * w5 * 2,)
    shapes["rec.conv.kernel"] = (1, 1, 2, ch[-1])
    shapes["rec.conv.bias"] = (ch[-1],)
    for l in range(4, 0, -1):
        c = ch[l - 1]
        shapes[f"dec{l}.up.kernel"] = (2, 2, c, ch[l])          # HWOI
        shapes[f"dec{l}.up.bias"] = (c,)
        unit(f"dec{l}.cb1a", c, 2 * c)
        for u in R._feature_block_names(cfg, f"dec{l}"):
            unit(u, c)
    shapes["head.kernel"] = (6, 6, ch[0], 2)
    shapes["head.bias"] = (2,)
    return shapes


def l2_regularized(cfg):
    return [f"enc{l}.down.kernel" for l in range(1, 6)] + [f"dec{l}.up.kernel" for l in range(4, 0, -1)]


def init_params(cfg, seed_name="aenet", dtype=np.float64):
    """Keras defaults (glorot_uniform kernels, Embedding U(-0.05, 0.05)) with biases, gamma and beta perturbed so that tests see them."""
    out = {}
    for name, shp in param_shapes(cfg).items():
        key = f"{seed_name}/{name}"
        if name == "vec.embedding":
            a = detrand.uniform(key, shp, -0.05, 0.05)
        elif name.endswith(".kernel"):
            rf = shp[0] * shp[1] if len(shp) == 4 else 1
            fan_in, fan_out = (shp[2] * rf, shp[3] * rf) if len(shp) == 4 else shp
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            a = detrand.uniform(key, shp, -lim, lim)
        elif name.endswith(".gamma"):
            a = detrand.uniform(key, shp, 0.5, 1.5)
        else:
            a = detrand.uniform(key, shp, -0.2, 0.2)
        out[name] = a.astype(dtype)
    return out


def logits(P, spec, emb, cfg, training=True, masks=None, bn_state=None, storage=None):
    """AENet._build up to the 6x6 convolution.  masks: (vector mask [B, 2048], join mask [B, h5 w5 2]), already scaled by 1 / (1 - p).
    storage="bf16": trunk activations, their gradients and trunk kernels rounded where the product stores them in bf16."""
    q = R._QuantSTE.apply if storage == "bf16" else R._ident
    qw = R._QuantFwd.apply if storage == "bf16" else R._ident
    x, skips = q(spec), []
    for l in range(1, 6):
        x = q(R.conv2d_same(x, qw(P[f"enc{l}.down.kernel"]), P[f"enc{l}.down.bias"], 1 if l == 1 else 2))
        x = R.feature_block(x, P, f"enc{l}", cfg, bn_state, training, None, q, qw)
        skips.append(x)
    B, cL, h5, w5 = x.shape
    v = P["vec.embedding"][emb.long()].reshape(B, -1) @ P["vec.dense.kernel"] + P["vec.dense.bias"]
    if masks is not None:
        v = v * masks[0].reshape(B, -1)
    lat = torch.cat([x.permute(0, 2, 3, 1).reshape(B, -1), v], dim=1)          # Flatten of the NHWC tensor
    r = lat @ P["rec.dense.kernel"] + P["rec.dense.bias"]
    if masks is not None:
        r = r * masks[1].reshape(B, -1)
    r = r.view(B, h5, w5, 2).permute(0, 3, 1, 2)                               # Reshape((h5, w5, 2)) is NHWC
    x = q(R.conv2d_same(r, P["rec.conv.kernel"], P["rec.conv.bias"], 1))       # the Dense branch stays fp32
    for l in range(4, 0, -1):
        x = q(R.conv2d_transpose_same(x, qw(P[f"dec{l}.up.kernel"]), P[f"dec{l}.up.bias"], 2))
        x = q(torch.cat([skips[l - 1], x], dim=1))
        x = R.conv_block_1(x, P, f"dec{l}.cb1a", cfg, bn_state, training, None, q, qw)
        x = R.feature_block(x, P, f"dec{l}", cfg, bn_state, training, None, q, qw)
    z = R.conv2d_same(x, qw(P["head.kernel"]), P["head.bias"], 1)
    return R._QuantBwd.apply(z) if storage == "bf16" else z


def forward(P, spec, emb, cfg, **kw):
    """relu(out, alpha=0.0, max_value=1) (ae_net.py:249)."""
    return torch.clamp(logits(P, spec, emb, cfg, **kw), 0.0, 1.0)


def reg_loss(P, cfg, n_replicas=1):
    return sum(L2_COEF * (P[n] ** 2).sum() for n in l2_regularized(cfg)) / n_replicas


def loss_and_grads(params, spec_in, emb, spec_out, cfg, masks=None, alpha=0.9, dtype=torch.float64, storage=None, training=True):
    """(loss = compute_loss + sum(model.losses), data loss, prediction, logits, gradients by name) of one train step."""
    P = R.to_torch(params, dtype, True)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    z = logits(P, t(spec_in), torch.as_tensor(np.asarray(emb)), cfg, training=training, storage=storage,
               masks=None if masks is None else tuple(t(m) for m in masks))
    pred = torch.clamp(z, 0.0, 1.0)
    data = R.data_loss(t(spec_out), pred, alpha)
    loss = data + reg_loss(P, cfg)
    loss.backward()
    return float(loss), float(data), pred.detach(), z.detach(), {n: p.grad.detach() for n, p in P.items()}

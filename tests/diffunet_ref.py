"""DiffUNet (dl_models/diff_u_net.py:200-272) restated in torch, fp64 by default, from the source text: configuration, parameters in
Keras shapes, forward, the loss with the linear output, gradients by autograd of the literal expressions.  Test infrastructure only.
The encoder, the decoder and the feature blocks are AENet's word for word (diff_u_net.py:262-392 repeats ae_net.py:270-399), so they are
taken from the same helpers as tests/aenet_ref.py (oracle.torch_ref); what differs is restated here.  Parameter names are the engine's.

  encoder   level 1 Conv2D(F0, 2, strides=1, 'same'), levels 2-5 Conv2D(2, strides=2), each followed by the feature block of `mode`;
            l2(0.001) on these kernels (:266-272)
  vector    Embedding(1500, 128) -> Flatten -> Dense(h5 w5 16 F0, name="encoder_inf_dense") -> Dropout(.5) -> Reshape((h5, w5, 16 F0))
            (:251-260): no 1x1 convolution behind it
  join      Add()([encoding_5_out, vector_out]) (:228)
  decoder   Conv2DTranspose(2, strides=2, l2) -> concatenate([skip, x]) -> convolutional_block_1 -> feature block (:288-318)
  output    UpSampling2D((1, 1)) = identity, Conv2D(2, (1, 1), activation='linear') (:246-247)
"""
import math

import numpy as np
import torch

import aenet_ref as A
from oracle import detrand, torch_ref as R

VOCAB, EMB_DIM = 1500, 128
DROPOUT_P = 0.5
L2_COEF = 0.001

config = A.config                    # the same hyper-parameters: H, W multiples of 16, F0, mode, BatchNorm; k = 2, depth 4
l2_regularized = A.l2_regularized    # the five encoder kernels and the four transposed ones (:266-272, :294-300)


def vec_units(cfg):
    return (cfg.H // 16) * (cfg.W // 16) * cfg.enc_channels()[-1]


def param_shapes(cfg):
    shapes = {}
    for n, s in A.param_shapes(cfg).items():
        if n.startswith(("vec.", "rec.", "head.")):
            if n == "vec.embedding":          # the vector block sits where AENet's does in creation order
                n_idx = int(np.prod(cfg.inf_vector_shape))
                shapes["vec.embedding"] = (VOCAB, EMB_DIM)
                shapes["encoder_inf_dense.kernel"] = (n_idx * EMB_DIM, vec_units(cfg))
                shapes["encoder_inf_dense.bias"] = (vec_units(cfg),)
            continue
        shapes[n] = s
    shapes["head.kernel"] = (1, 1, cfg.enc_channels()[0], 2)
    shapes["head.bias"] = (2,)
    return shapes


def init_params(cfg, seed_name="diffunet", dtype=np.float64):
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


def join_add(P, x, emb, masks, q):
    """vector_block (:251-260) and Add()([encoding_5_out, vector_out]) (:228).  masks: (vector mask [B, h5 w5 16 F0],) or None."""
    B, cL, h5, w5 = x.shape
    v = P["vec.embedding"][emb.long()].reshape(B, -1) @ P["encoder_inf_dense.kernel"] + P["encoder_inf_dense.bias"]
    if masks is not None:
        v = v * masks[0].reshape(B, -1)
    v = v.view(B, h5, w5, cL).permute(0, 3, 1, 2)               # Reshape((h5, w5, 16 F0)) is NHWC
    return q(x + v)                                             # bf16 trunk + fp32 branch -> bf16


def head_1x1(P, x, storage, qw, head_storage="f32"):
    """Conv2D(2, (1, 1), activation='linear') (:247).  bf16 storage: fp32 logits whose gradient is stored in bf16 (csrc/head1x1.hip);
    head_storage="bf16": the generic kernels, which store the logits in bf16 as well."""
    z = R.conv2d_same(x, qw(P["head.kernel"]), P["head.bias"], 1)
    if storage != "bf16":
        return z
    return R._QuantSTE.apply(z) if head_storage == "bf16" else R._QuantBwd.apply(z)


def logits(P, spec, emb, cfg, training=True, masks=None, bn_state=None, storage=None, join=join_add, head=head_1x1, head_storage="f32"):
    """DiffUNet._build up to its output (which is linear: the logits ARE the prediction).  storage="bf16": trunk activations, their
    gradients and trunk kernels rounded where the product stores them in bf16.  join / head: the two places a sibling model differs in
    (tests/test_diff_ref.py puts AENet's there and must get tests/aenet_ref.py back)."""
    q = R._QuantSTE.apply if storage == "bf16" else R._ident
    qw = R._QuantFwd.apply if storage == "bf16" else R._ident
    x, skips = q(spec), []
    for l in range(1, 6):
        x = q(R.conv2d_same(x, qw(P[f"enc{l}.down.kernel"]), P[f"enc{l}.down.bias"], 1 if l == 1 else 2))
        x = R.feature_block(x, P, f"enc{l}", cfg, bn_state, training, None, q, qw)
        skips.append(x)
    x = join(P, x, emb, masks, q)
    for l in range(4, 0, -1):
        x = q(R.conv2d_transpose_same(x, qw(P[f"dec{l}.up.kernel"]), P[f"dec{l}.up.bias"], 2))
        x = q(torch.cat([skips[l - 1], x], dim=1))
        x = R.conv_block_1(x, P, f"dec{l}.cb1a", cfg, bn_state, training, None, q, qw)
        x = R.feature_block(x, P, f"dec{l}", cfg, bn_state, training, None, q, qw)
    return head(P, x, storage, qw, head_storage)


forward = logits                     # activation='linear'


def reg_loss(P, cfg, n_replicas=1):
    return sum(L2_COEF * (P[n] ** 2).sum() for n in l2_regularized(cfg)) / n_replicas


def loss_and_grads(params, spec_in, emb, spec_out, cfg, masks=None, alpha=0.9, dtype=torch.float64, storage=None, training=True,
                   diff_loss=False, head_storage="f32", out_act=None, **kw):
    """(loss = compute_loss + sum(model.losses), data loss, prediction, logits, gradients by name) of one train step.  diff_loss: the
    phase target is phase_true - phase_x (main_training.py:214-217), what this model is trained with."""
    P = R.to_torch(params, dtype, True)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    x_in = t(spec_in)
    z = logits(P, x_in, torch.as_tensor(np.asarray(emb)), cfg, training=training, storage=storage, head_storage=head_storage,
               masks=None if masks is None else tuple(t(m) for m in masks), **kw)
    pred = z if out_act is None else out_act(z)
    data = R.data_loss(t(spec_out), pred, alpha, x_in=x_in if diff_loss else None)
    loss = data + reg_loss(P, cfg)
    loss.backward()
    return float(loss.detach()), float(data.detach()), pred.detach(), z.detach(), {n: p.grad.detach() for n, p in P.items()}

"""fp64 restatement of the reference DiffVAE (dl_models/diff_vae.py:258-472) and of its share of the train step (main_training.py:192-201,
:257-265): torch CPU autograd.  Test infrastructure only.  What is word for word dl_models/vae.py comes from tests/vae_ref.py
(configuration, the sampling layer, the KL term); the encoder / decoder stacks are restated here with the storage hooks vae_ref.py
lacks (storage="bf16": trunk activations, their gradients and trunk kernels rounded where the product stores bf16; the Dense branches,
the heads and the sampling layer stay fp32).

The three differences from the VAE:
  information vector   Embedding(1500, 128) -> Dense(n_neurons) on the UNFLATTENED [B, 2, 16, 128] tensor, i.e. per position
                       (:416-417); Flatten at the join (:463-465)
  output               Activation("linear") (:385)
  model of __main__    filters (32, 64, 128, 256), latent_space_dim 16, n_neurons 20 * 64 (:476-485)
"""
import numpy as np
import torch
import torch.nn.functional as F

import vae_ref as V
from oracle import torch_ref as R
from oracle.torch_ref import conv2d_same, conv2d_transpose_same, data_loss
from oracle.torch_resae import init_from_shapes

VOCAB, EMB_DIM = 1500, 128
DROPOUT_P = V.DROPOUT_P
LEAKY_ALPHA = V.LEAKY_ALPHA


def config(H, W, conv_filters=(32, 64, 128, 256), conv_kernels=(3, 3, 3, 3), conv_strides=(2, 2, 2, 2), latent_space_dim=16, n_neurons=1280,
           inf_vector_shape=(2, 16)):
    """DiffVAE.__init__ arguments (:48-57); the defaults are the model of its __main__ block."""
    return V.VAEConfig(H, W, tuple(conv_filters), tuple(conv_kernels), tuple(conv_strides), latent_space_dim, n_neurons, tuple(inf_vector_shape))


def param_shapes(cfg, per_position=True):
    """vae_ref's with the information-vector branch of this model.  per_position=False: the VAE's flattened branch (its Embedding
    included), for the sibling check."""
    shapes = {}
    h, w, c = cfg.bottleneck_shape()
    n_idx = int(np.prod(cfg.inf_vector_shape))
    for n, s in V.param_shapes(cfg).items():
        if per_position:
            if n == "embedding":
                s = (VOCAB, EMB_DIM)
            elif n == "encoder_inf_dense.kernel":
                s = (EMB_DIM, cfg.n_neurons)
            elif n in ("mu.kernel", "log_variance.kernel"):
                s = (h * w * c + n_idx * cfg.n_neurons, cfg.latent_space_dim)
        shapes[n] = s
    return shapes


def init_params(cfg, seed_name="dvp", randomize_all=False, dtype=np.float32, per_position=True):
    return init_from_shapes(param_shapes(cfg, per_position), seed_name, randomize_all, dtype)


def _bn(x, P, base, bn_state, training):
    if training or bn_state is None:
        return F.batch_norm(x, None, None, P[base + ".gamma"], P[base + ".beta"], training=True, momentum=1 - R.BN_MOMENTUM, eps=R.BN_EPS)
    return F.batch_norm(x, bn_state[base + ".moving_mean"].to(x.dtype), bn_state[base + ".moving_variance"].to(x.dtype),
                        P[base + ".gamma"], P[base + ".beta"], training=False, eps=R.BN_EPS)


def vector(P, emb, cfg, per_position=True):
    """_add_dense_to_inf (:407-418) flattened for the join (:464).  per_position=False: the VAE's Flatten -> Dense."""
    B = emb.shape[0]
    e = P["embedding"][emb.long()]                                             # [B, 2, 16, dim]
    if per_position:
        return (e @ P["encoder_inf_dense.kernel"] + P["encoder_inf_dense.bias"]).reshape(B, -1)
    return e.reshape(B, -1) @ P["encoder_inf_dense.kernel"] + P["encoder_inf_dense.bias"]


def encode(P, spec, emb, cfg, eps, storage=None, per_position=True, bn_state=None, training=True):
    """model.encoder([spec, emb]) -> (z, mu, log_var) (this class returns z alone, :472; the engine hands out all three)."""
    q = R._QuantSTE.apply if storage == "bf16" else R._ident
    qw = R._QuantFwd.apply if storage == "bf16" else R._ident
    B = spec.shape[0]
    x = q(spec)
    for i in range(len(cfg.conv_filters)):
        x = q(conv2d_same(x, qw(P[f"encoder_conv_layer_{i + 1}.kernel"]), P[f"encoder_conv_layer_{i + 1}.bias"], cfg.conv_strides[i]))
        x = q(F.relu(_bn(x, P, f"encoder_bn_{i + 1}", bn_state, training)))
    flat = x.permute(0, 2, 3, 1).reshape(B, -1)                               # Flatten of the NHWC tensor (:463)
    cat = torch.cat([flat, vector(P, emb, cfg, per_position)], dim=1)
    mu = cat @ P["mu.kernel"] + P["mu.bias"]
    log_var = cat @ P["log_variance.kernel"] + P["log_variance.bias"]
    return V.sample(mu, log_var, eps), mu, log_var


def decode_logits(P, z, cfg, mask_dec=None, storage=None, bn_state=None, training=True):
    """model.decoder(z) up to the output layer; mask_dec [B, h*w*c]: keep mask already scaled by 1/(1-p) (None = no dropout)."""
    q = R._QuantSTE.apply if storage == "bf16" else R._ident
    qw = R._QuantFwd.apply if storage == "bf16" else R._ident
    n = len(cfg.conv_filters)
    B = z.shape[0]
    h, w, c = cfg.bottleneck_shape()
    d = z @ P["decoder_dense.kernel"] + P["decoder_dense.bias"]
    if mask_dec is not None:
        d = d * mask_dec.reshape(B, -1)
    x = q(d.view(B, h, w, c).permute(0, 3, 1, 2))
    x = q(conv2d_transpose_same(x, qw(P["decoder_conv_transpose_layer_0.kernel"]), P["decoder_conv_transpose_layer_0.bias"], 1))
    x = q(F.leaky_relu(_bn(x, P, "decoder_bn_0", bn_state, training), LEAKY_ALPHA))
    for layer_index in reversed(range(1, n)):
        num = n - layer_index
        x = q(conv2d_transpose_same(x, qw(P[f"decoder_conv_transpose_layer_{num}.kernel"]), P[f"decoder_conv_transpose_layer_{num}.bias"],
                                    cfg.conv_strides[layer_index - 1]))
        x = q(F.leaky_relu(_bn(x, P, f"decoder_bn_{num}", bn_state, training), LEAKY_ALPHA))
    return q(conv2d_transpose_same(x, qw(P[f"decoder_out_{n}.kernel"]), P[f"decoder_out_{n}.bias"], cfg.conv_strides[0]))


def forward(P, spec, emb, cfg, eps, mask_dec=None, inter=None, storage=None, per_position=True, out_act=None, bn_state=None, training=True):
    """DiffVAE.model([spec, emb]) with the noise `eps` [B, latent] given; Activation("linear") (:385) unless out_act is given."""
    z, mu, log_var = encode(P, spec, emb, cfg, eps, storage, per_position, bn_state, training)
    if inter is not None:
        inter.update(z=z, mu=mu, log_var=log_var)
    lg = decode_logits(P, z, cfg, mask_dec, storage, bn_state, training)
    if inter is not None:
        inter["logits"] = lg
    return lg if out_act is None else out_act(lg)


def loss_and_grads(params, spec_in, emb, spec_out, cfg, eps, alpha=0.9, global_batch=None, mask_dec=None, dtype=torch.float64, inter=None,
                   storage=None, per_position=True, out_act=None, diff_loss=False):
    """compute_loss (no model losses: diff_vae.py has no regulariser) + compute_kl_loss (main_training.py:263-265) and its gradients.
    Returns (loss, data term, KL term, prediction, grads)."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for k, v in params.items()}
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
    inter = {} if inter is None else inter
    spec = t(spec_in)
    gb = spec.shape[0] if global_batch is None else global_batch
    pred = forward(P, spec, torch.as_tensor(np.asarray(emb)), cfg, t(eps), t(mask_dec), inter, storage, per_position, out_act)
    dl = data_loss(t(spec_out), pred, alpha, gb, x_in=spec if diff_loss else None)
    kl = V.kl_loss(inter["mu"], inter["log_var"], gb)
    loss = dl + kl
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in P.items()}
    for k in ("z", "mu", "log_var", "logits"):
        inter[k] = inter[k].detach()
    return float(loss.detach()), float(dl.detach()), float(kl.detach()), pred.detach(), grads

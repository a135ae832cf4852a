"""fp64 restatement of the reference VAE (dl_models/vae.py) and of its share of the train step (main_training.py:192-201,
:257-265): torch CPU autograd, built from the helpers of oracle/torch_ref.py and oracle/torch_ae.py.  Test infrastructure only.

Parameters are held in Keras layouts (Conv2D [kh,kw,Cin,Cout], Conv2DTranspose [kh,kw,Cout,Cin], Dense [in,out]); activations
NCHW inside this file, Flatten / Reshape follow the Keras NHWC order.  What differs from oracle/torch_ae.py: no l2 terms, no Dropout
on the information-vector branch, two Dense heads and the sampling layer at the bottleneck, LeakyReLU(0.3) in the decoder, the KL term.
"""
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle.torch_ref import conv2d_same, conv2d_transpose_same, data_loss, BN_EPS, BN_MOMENTUM, VOCAB, EMB_DIM
from oracle.torch_resae import init_from_shapes

DROPOUT_P = 0.3        # Dropout(.3) behind decoder_dense (dl_models/vae.py:303)
LEAKY_ALPHA = 0.3      # keras LeakyReLU() default (dl_models/vae.py:331, :366)


@dataclass
class VAEConfig:
    """VAE.__init__ arguments (dl_models/vae.py:48-57); the defaults are the call of main_training.py:143-152."""
    H: int
    W: int
    conv_filters: tuple = (64, 128, 256, 512)
    conv_kernels: tuple = (3, 3, 3, 3)
    conv_strides: tuple = (2, 2, 2, 2)
    latent_space_dim: int = 64
    n_neurons: int = 2048
    inf_vector_shape: tuple = (2, 16)

    def bottleneck_shape(self):
        h, w = self.H, self.W
        for s in self.conv_strides:
            h, w = -(-h // s), -(-w // s)
        return h, w, self.conv_filters[-1]


def param_shapes(cfg: VAEConfig) -> Dict[str, tuple]:
    """Trainable variables in creation order: encoder (dl_models/vae.py:387-472), decoder (:274-385)."""
    shapes = {}
    n = len(cfg.conv_filters)
    cin = 2
    for i in range(n):                                                         # _add_conv_layer (:432-451)
        f, k = cfg.conv_filters[i], cfg.conv_kernels[i]
        shapes[f"encoder_conv_layer_{i + 1}.kernel"] = (k, k, cin, f)
        shapes[f"encoder_conv_layer_{i + 1}.bias"] = (f,)
        shapes[f"encoder_bn_{i + 1}.gamma"] = (f,)
        shapes[f"encoder_bn_{i + 1}.beta"] = (f,)
        cin = f
    h, w, c = cfg.bottleneck_shape()
    n_in = int(np.prod(cfg.inf_vector_shape)) * EMB_DIM
    shapes["embedding"] = (VOCAB, EMB_DIM)                                     # _add_dense_to_inf (:407-418)
    shapes["encoder_inf_dense.kernel"] = (n_in, cfg.n_neurons)
    shapes["encoder_inf_dense.bias"] = (cfg.n_neurons,)
    for head in ("mu", "log_variance"):                                        # _add_bottleneck (:462-472)
        shapes[head + ".kernel"] = (h * w * c + cfg.n_neurons, cfg.latent_space_dim)
        shapes[head + ".bias"] = (cfg.latent_space_dim,)
    shapes["decoder_dense.kernel"] = (cfg.latent_space_dim, h * w * c)         # _add_dense_layer (:294-304)
    shapes["decoder_dense.bias"] = (h * w * c,)
    f, k = cfg.conv_filters[-1], cfg.conv_kernels[-1]                          # _add_first_conv (:315-333): stride 1
    shapes["decoder_conv_transpose_layer_0.kernel"] = (k, k, f, c)
    shapes["decoder_conv_transpose_layer_0.bias"] = (f,)
    shapes["decoder_bn_0.gamma"] = (f,)
    shapes["decoder_bn_0.beta"] = (f,)
    cin = f
    for layer_index in reversed(range(1, n)):                                  # _add_conv_transpose_layer (:348-367)
        num = n - layer_index
        f, k = cfg.conv_filters[layer_index - 1], cfg.conv_kernels[layer_index - 1]
        shapes[f"decoder_conv_transpose_layer_{num}.kernel"] = (k, k, f, cin)
        shapes[f"decoder_conv_transpose_layer_{num}.bias"] = (f,)
        shapes[f"decoder_bn_{num}.gamma"] = (f,)
        shapes[f"decoder_bn_{num}.beta"] = (f,)
        cin = f
    k0 = cfg.conv_kernels[0]
    shapes[f"decoder_out_{n}.kernel"] = (k0, k0, 2, cin)                       # _add_decoder_output (:369-385)
    shapes[f"decoder_out_{n}.bias"] = (2,)
    return shapes


def init_params(cfg: VAEConfig, seed_name="vp", randomize_all=False, dtype=np.float32):
    """Keras default initialisers; values from detrand (platform independent)."""
    return init_from_shapes(param_shapes(cfg), seed_name, randomize_all, dtype)


def _bn(x, P, base):
    return F.batch_norm(x, None, None, P[base + ".gamma"], P[base + ".beta"], training=True, momentum=1 - BN_MOMENTUM, eps=BN_EPS)


def sample(mu, log_var, eps):
    """SamplingLayer.call (dl_models/vae.py:34-39) with the noise given."""
    return mu + torch.exp(0.5 * log_var) * eps


def kl_elements(mu, log_var):
    """kl_loss_object (main_training.py:192-194): one value per (b, l)."""
    return -0.5 * (1 + log_var - mu ** 2 - torch.exp(log_var))


def kl_loss(mu, log_var, global_batch):
    """compute_kl_loss (main_training.py:196-201): per-example sums / global batch."""
    return kl_elements(mu, log_var).sum(dim=1).sum() / global_batch


def sample_kl_grads(mu, log_var, eps, dz, inv_gb):
    """The analytic backward pass of sampling + KL (what unetrir_vae_sample_kl_bwd_f32 computes): dmu, dlv."""
    dmu = dz + inv_gb * mu
    dlv = dz * 0.5 * torch.exp(0.5 * log_var) * eps + inv_gb * 0.5 * (torch.exp(log_var) - 1.0)
    return dmu, dlv


def encode(P, spec, emb, cfg: VAEConfig, eps):
    """model.encoder([spec, emb], training=True) -> (z, mu, log_var)."""
    B = spec.shape[0]
    x = spec
    for i in range(len(cfg.conv_filters)):
        x = conv2d_same(x, P[f"encoder_conv_layer_{i + 1}.kernel"], P[f"encoder_conv_layer_{i + 1}.bias"], cfg.conv_strides[i])
        x = F.relu(_bn(x, P, f"encoder_bn_{i + 1}"))
    flat = x.permute(0, 2, 3, 1).reshape(B, -1)                               # Flatten of the NHWC tensor (:463)
    vec = P["embedding"][emb.long()].reshape(B, -1) @ P["encoder_inf_dense.kernel"] + P["encoder_inf_dense.bias"]
    cat = torch.cat([flat, vec], dim=1)
    mu = cat @ P["mu.kernel"] + P["mu.bias"]
    log_var = cat @ P["log_variance.kernel"] + P["log_variance.bias"]
    return sample(mu, log_var, eps), mu, log_var


def decode(P, z, cfg: VAEConfig, mask_dec: Optional[torch.Tensor] = None, inter=None):
    """model.decoder(z, training=True); mask_dec [B, h*w*c]: dropout keep mask already scaled by 1/(1-p) (None = no dropout)."""
    n = len(cfg.conv_filters)
    B = z.shape[0]
    h, w, c = cfg.bottleneck_shape()
    d = z @ P["decoder_dense.kernel"] + P["decoder_dense.bias"]
    if mask_dec is not None:
        d = d * mask_dec
    x = d.view(B, h, w, c).permute(0, 3, 1, 2)
    x = conv2d_transpose_same(x, P["decoder_conv_transpose_layer_0.kernel"], P["decoder_conv_transpose_layer_0.bias"], 1)
    x = F.leaky_relu(_bn(x, P, "decoder_bn_0"), LEAKY_ALPHA)
    for layer_index in reversed(range(1, n)):
        num = n - layer_index
        x = conv2d_transpose_same(x, P[f"decoder_conv_transpose_layer_{num}.kernel"], P[f"decoder_conv_transpose_layer_{num}.bias"],
                                  cfg.conv_strides[layer_index - 1])
        x = F.leaky_relu(_bn(x, P, f"decoder_bn_{num}"), LEAKY_ALPHA)
    x = conv2d_transpose_same(x, P[f"decoder_out_{n}.kernel"], P[f"decoder_out_{n}.bias"], cfg.conv_strides[0])
    if inter is not None:
        inter["logits"] = x
    return torch.sigmoid(x)


def forward(P, spec, emb, cfg: VAEConfig, eps, mask_dec: Optional[torch.Tensor] = None, inter=None):
    """VAE.model([spec, emb]) with the noise `eps` [B, latent] given.  spec [B,2,H,W] NCHW, emb int [B,2,16]."""
    z, mu, log_var = encode(P, spec, emb, cfg, eps)
    if inter is not None:
        inter.update(z=z, mu=mu, log_var=log_var)
    return decode(P, z, cfg, mask_dec, inter)


def loss_and_grads(params, spec_in, emb, spec_out, cfg: VAEConfig, eps, alpha=0.9, global_batch=None, mask_dec=None,
                   dtype=torch.float64, inter=None):
    """The loss of train_step (main_training.py:263-265): compute_loss (no model losses: vae.py has no regulariser) +
    compute_kl_loss, and its gradients.  Returns (loss, data term, KL term, prediction, grads)."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for k, v in params.items()}
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
    inter = {} if inter is None else inter
    spec = t(spec_in)
    gb = spec.shape[0] if global_batch is None else global_batch
    pred = forward(P, spec, torch.as_tensor(np.asarray(emb)), cfg, t(eps), t(mask_dec), inter)
    dl = data_loss(t(spec_out), pred, alpha, gb)
    kl = kl_loss(inter["mu"], inter["log_var"], gb)
    loss = dl + kl
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in P.items()}
    for k in ("z", "mu", "log_var", "logits"):
        inter[k] = inter[k].detach()
    return float(loss.detach()), float(dl.detach()), float(kl.detach()), pred.detach(), grads

"""fp64 restatement of the reference VQ-VAE (dl_models/vqvae.py) and of its share of the train step (main_training.py:232-233:
`loss += sum(model.losses) / replicas`): torch CPU, built from the helpers of oracle/torch_ref.py.  Test infrastructure only.
PARITY UNPINNED: TensorFlow does not run here, so this is a restatement of the source text, checked against torch autograd of the
literal expressions and against finite differences (tests/test_vqvae_ref.py).

Parameters are held in Keras layouts (Conv2D [kh,kw,Cin,Cout], Conv2DTranspose [kh,kw,Cout,Cin], Dense [in,out], the codebook
[embedding_dim, num_embeddings]); activations NCHW inside this file except around the quantiser, which - like Flatten / Reshape -
works on the Keras NHWC order.  What differs from oracle/torch_ae.py: no l2 terms; Embedding(1500, 128) and a PER-POSITION Dense on
the information vector, no Dropout there; Dense -> Dropout -> Reshape(h, w, 2) -> Conv2D(1x1) -> VectorQuantizer at the bottleneck;
a decoder that starts at the first transposed convolution.
"""
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import detrand
from oracle.torch_ref import conv2d_same, conv2d_transpose_same, data_loss, BN_EPS, BN_MOMENTUM
from oracle.torch_resae import init_from_shapes

DROPOUT_P = 0.3        # Dropout(.3) behind the bottleneck Dense (dl_models/vqvae.py:511)
BETA = 0.25            # VectorQuantizer(beta=0.25) (:43)
VOCAB, EMB_DIM = 1500, 128          # Embedding(1500, 128) (:453)
CODEBOOK = "vector_quantizer.embeddings"


# ---------------------------------------------------------------------------------------------------------------- the quantiser
def distances(flat, E):
    """get_code_indices (:87-94): ||x||^2 + ||E_k||^2 - 2 x . E_k, [vectors, K]."""
    return (flat ** 2).sum(dim=1, keepdim=True) + (E ** 2).sum(dim=0) - 2 * (flat @ E)


def code_indices(flat, E):
    """tf.argmin(distances, axis=1) (:97): the lowest index among equal minima (torch.argmin returns the first one too)."""
    return torch.argmin(distances(flat, E), dim=1)


def quantize_literal(x, E, beta=BETA, indices=None, frozen=None):
    """VectorQuantizer.call (:61-85) as written, `detach` for stop_gradient: x [..., C] in NHWC order, E [D, K].  Returns
    (straight-through output, the add_loss term, the indices).  indices: take these instead of searching.
    frozen = {"q": ..., "x": ...}: the values stop_gradient holds, given as constants of a base point - the function whose TRUE
    gradient at that point is what backpropagation through the stop_gradients yields (finite differences are taken of this one:
    the literal function's own derivative is another thing, its output being E[:, idx] whatever x is)."""
    D, K = E.shape
    flat = x.reshape(-1, D)
    idx = code_indices(flat, E) if indices is None else indices.long()
    quantized = (F.one_hot(idx, K).to(x.dtype) @ E.t()).reshape(x.shape)
    sg_q, sg_x = (quantized.detach(), x.detach()) if frozen is None else (frozen["q"], frozen["x"])
    commitment_loss = ((sg_q - x) ** 2).mean()
    codebook_loss = ((quantized - sg_x) ** 2).mean()
    return x + (sg_q - sg_x), beta * commitment_loss + codebook_loss, idx


def quantize(x, E, beta=BETA, r=1.0, indices=None):
    """The same values without the one-hot matrix, as the kernel states them: y = x + (q - x), S = sum (q - x)^2, the term as it
    enters the loss r (1 + beta) S / N.  Returns (y, term, S, idx)."""
    D = E.shape[0]
    flat = x.reshape(-1, D)
    idx = code_indices(flat, E) if indices is None else indices.long()
    q = E.t()[idx].reshape(x.shape)
    S = ((q - x) ** 2).sum()
    return x + (q - x), r * (1 + beta) * S / x.numel(), S, idx


def quantize_grads(x, E, idx, dy, beta=BETA, r=1.0):
    """The hand-written backward pass (what unetrir_vq_bwd_f32 computes) of <dy, y> + r * term:
    dx = dy + r beta 2 (x - q) / N;  dE[:, k] = r sum_{i: idx_i = k} 2 (q_i - x_i) / N, codes nobody chose get exactly 0."""
    D = E.shape[0]
    N = x.numel()
    q = E.t()[idx.long()].reshape(x.shape)
    dx = dy + r * beta * 2 * (x - q) / N
    dE = torch.zeros_like(E)
    dE.index_add_(1, idx.long(), (r * 2 * (q - x) / N).reshape(-1, D).t())
    return dx, dE


# ---------------------------------------------------------------------------------------------------------------- the model
@dataclass
class VQVAEConfig:
    """VQVAE.__init__ arguments (dl_models/vqvae.py:107-116); the defaults are the __main__ block's (:522-531)."""
    H: int
    W: int
    conv_filters: tuple = (32, 64, 128, 256)
    conv_kernels: tuple = (3, 3, 3, 3)
    conv_strides: tuple = (2, 2, 2, 2)
    latent_space_dim: int = 16
    n_neurons: int = 320
    inf_vector_shape: tuple = (2, 16)

    def bottleneck_shape(self):
        h, w = self.H, self.W
        for s in self.conv_strides:
            h, w = -(-h // s), -(-w // s)
        return h, w, self.conv_filters[-1]


def param_shapes(cfg: VQVAEConfig) -> Dict[str, tuple]:
    """Trainable variables in creation order: encoder (:425-520), decoder (:333-423)."""
    shapes = {}
    n = len(cfg.conv_filters)
    cin = 2
    for i in range(n):                                                         # _add_conv_layer (:469-488)
        f, k = cfg.conv_filters[i], cfg.conv_kernels[i]
        shapes[f"encoder_conv_layer_{i + 1}.kernel"] = (k, k, cin, f)
        shapes[f"encoder_conv_layer_{i + 1}.bias"] = (f,)
        shapes[f"encoder_bn_{i + 1}.gamma"] = (f,)
        shapes[f"encoder_bn_{i + 1}.beta"] = (f,)
        cin = f
    h, w, c = cfg.bottleneck_shape()
    n_pos = int(np.prod(cfg.inf_vector_shape))
    shapes["embedding"] = (VOCAB, EMB_DIM)                                     # _add_dense_to_inf (:445-455)
    shapes["encoder_inf_dense.kernel"] = (EMB_DIM, cfg.n_neurons)              # Dense on the last axis: per position
    shapes["encoder_inf_dense.bias"] = (cfg.n_neurons,)
    shapes["dense.kernel"] = (h * w * c + n_pos * cfg.n_neurons, h * w * 2)    # _add_bottleneck (:490-520)
    shapes["dense.bias"] = (h * w * 2,)
    shapes["conv2d.kernel"] = (1, 1, 2, c)
    shapes["conv2d.bias"] = (c,)
    shapes[CODEBOOK] = (cfg.latent_space_dim, c)                               # VectorQuantizer(conv_filters[-1], latent_space_dim)
    f, k = cfg.conv_filters[-1], cfg.conv_kernels[-1]                          # _add_first_conv (:353-371): stride 1
    shapes["decoder_conv_transpose_layer_0.kernel"] = (k, k, f, c)
    shapes["decoder_conv_transpose_layer_0.bias"] = (f,)
    shapes["decoder_bn_0.gamma"] = (f,)
    shapes["decoder_bn_0.beta"] = (f,)
    cin = f
    for layer_index in reversed(range(1, n)):                                  # _add_conv_transpose_layer (:386-405)
        num = n - layer_index
        f, k = cfg.conv_filters[layer_index - 1], cfg.conv_kernels[layer_index - 1]
        shapes[f"decoder_conv_transpose_layer_{num}.kernel"] = (k, k, f, cin)
        shapes[f"decoder_conv_transpose_layer_{num}.bias"] = (f,)
        shapes[f"decoder_bn_{num}.gamma"] = (f,)
        shapes[f"decoder_bn_{num}.beta"] = (f,)
        cin = f
    k0 = cfg.conv_kernels[0]
    shapes[f"decoder_out_{n}.kernel"] = (k0, k0, 2, cin)                       # _add_decoder_output (:407-423)
    shapes[f"decoder_out_{n}.bias"] = (2,)
    return shapes


def init_params(cfg: VQVAEConfig, seed_name="qp", randomize_all=False, dtype=np.float32, codebook_scale=1.0):
    """Keras default initialisers, the codebook tf.random_uniform_initializer() = U(-0.05, 0.05) (:52); values from detrand.
    codebook_scale widens the codebook (tests: codes that are actually used after a random 1x1 convolution)."""
    shapes = param_shapes(cfg)
    out = init_from_shapes(shapes, seed_name, randomize_all, dtype)
    out[CODEBOOK] = (detrand.uniform(f"{seed_name}/{CODEBOOK}", shapes[CODEBOOK], -0.05, 0.05) * codebook_scale).astype(dtype)
    return out


def _bn(x, P, base, moving=None):
    if moving is not None:          # training=False: the moving statistics
        return F.batch_norm(x, moving[base + ".moving_mean"], moving[base + ".moving_variance"], P[base + ".gamma"], P[base + ".beta"],
                            training=False, eps=BN_EPS)
    return F.batch_norm(x, None, None, P[base + ".gamma"], P[base + ".beta"], training=True, momentum=1 - BN_MOMENTUM, eps=BN_EPS)


def pre_quantizer(P, spec, emb, cfg: VQVAEConfig, mask=None, moving=None):
    """The encoder up to the quantiser's input, NHWC [B, h, w, C].  mask [B, h*w*2]: keep mask scaled by 1/(1-p), or None."""
    B = spec.shape[0]
    x = spec
    for i in range(len(cfg.conv_filters)):
        x = conv2d_same(x, P[f"encoder_conv_layer_{i + 1}.kernel"], P[f"encoder_conv_layer_{i + 1}.bias"], cfg.conv_strides[i])
        x = F.relu(_bn(x, P, f"encoder_bn_{i + 1}", moving))
    h, w, c = cfg.bottleneck_shape()
    flat = x.permute(0, 2, 3, 1).reshape(B, -1)                               # Flatten of the NHWC tensor (:504)
    vec = P["embedding"][emb.long()] @ P["encoder_inf_dense.kernel"] + P["encoder_inf_dense.bias"]      # [B, 2, 16, n_neurons]
    d = torch.cat([flat, vec.reshape(B, -1)], dim=1) @ P["dense.kernel"] + P["dense.bias"]
    if mask is not None:
        d = d * mask
    return d.view(B, h, w, 2) @ P["conv2d.kernel"][0, 0] + P["conv2d.bias"]    # Conv2D(C, (1, 1)) on NHWC


def decode(P, y, cfg: VQVAEConfig, inter=None, moving=None):
    """model.decoder(y): y NHWC [B, h, w, C], the quantiser's output."""
    n = len(cfg.conv_filters)
    x = y.permute(0, 3, 1, 2)
    x = conv2d_transpose_same(x, P["decoder_conv_transpose_layer_0.kernel"], P["decoder_conv_transpose_layer_0.bias"], 1)
    x = F.relu(_bn(x, P, "decoder_bn_0", moving))
    for layer_index in reversed(range(1, n)):
        num = n - layer_index
        x = conv2d_transpose_same(x, P[f"decoder_conv_transpose_layer_{num}.kernel"], P[f"decoder_conv_transpose_layer_{num}.bias"],
                                  cfg.conv_strides[layer_index - 1])
        x = F.relu(_bn(x, P, f"decoder_bn_{num}", moving))
    x = conv2d_transpose_same(x, P[f"decoder_out_{n}.kernel"], P[f"decoder_out_{n}.bias"], cfg.conv_strides[0])
    if inter is not None:
        inter["logits"] = x
    return torch.sigmoid(x)


def forward(P, spec, emb, cfg: VQVAEConfig, mask=None, indices=None, inter=None, moving=None, frozen=None):
    """VQVAE.model([spec, emb]).  Returns (prediction NCHW, the quantiser's add_loss term)."""
    x = pre_quantizer(P, spec, emb, cfg, mask, moving)
    y, vq, idx = quantize_literal(x, P[CODEBOOK], BETA, indices, frozen)
    if inter is not None:
        inter.update(x=x, y=y, idx=idx, vq=vq)
    return decode(P, y, cfg, inter, moving), vq


def loss_and_grads(params, spec_in, emb, spec_out, cfg: VQVAEConfig, alpha=0.9, global_batch=None, mask=None, n_replicas=1,
                   indices=None, dtype=torch.float64, inter=None, frozen=None):
    """The loss of train_step (main_training.py:203-235): compute_loss's data term + sum(model.losses) / replicas, the only model
    loss being the quantiser's, and its gradients.  Returns (loss, data term, vq term / replicas, prediction, grads)."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for k, v in params.items()}
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
    inter = {} if inter is None else inter
    spec = t(spec_in)
    gb = spec.shape[0] if global_batch is None else global_batch
    idx = None if indices is None else torch.as_tensor(np.asarray(indices)).long()
    pred, vq = forward(P, spec, torch.as_tensor(np.asarray(emb)), cfg, t(mask), idx, inter, frozen=frozen)
    dl = data_loss(t(spec_out), pred, alpha, gb)
    term = vq / n_replicas
    loss = dl + term
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in P.items()}
    for k in ("x", "y", "vq", "logits"):
        inter[k] = inter[k].detach()
    return float(loss.detach()), float(dl.detach()), float(term.detach()), pred.detach(), grads

"""deep_CNN (dl_models/cnn_clas.py:19-53) and its loss restated in torch, fp64 by default, from the source text: configuration,
parameters in Keras shapes, forward, categorical cross-entropy on the softmax output, gradients by autograd of these expressions.
Test infrastructure only.  Written with explicit sums (shifted slices, strided slices, means) rather than the library calls
tests/test_cnn_clas_ref.py holds it to.  Parameter names are the engine's.

  block i   Conv2D(F_i, 3x3, strides 1, 'valid', activation='relu') [Conv0_A, Conv1_A, Conv0_C; F = 16, 32, 64]
            -> BatchNormalization (if batchNorm; eps 1e-3, statistics over the ReLU output) [bn0, bn1, bn2]
            -> AveragePooling2D(2x2, strides 2, 'valid') (blocks 0, 1: floor(h/2) x floor(w/2)) | GlobalAveragePooling2D (block 2)
  head      Dense(256, relu) [dense] -> BatchNormalization over the batch [bn3] -> Dropout(.5) -> Dense(classes, softmax) [dense_1]
  loss      categorical_crossentropy(y, p) per sample = -sum_c y_c log p_c, taken as the log-softmax of the max-subtracted logits
            (PARITY UNPINNED: Keras goes through the logits when the softmax op is in sight and through clipped probabilities
            otherwise), summed over the rows and divided by the global batch
  accuracy  argmax(logits) == argmax(y), the lowest index on ties on both sides
"""
import collections
import math

import numpy as np
import torch

from oracle import detrand

FILTERS = (16, 32, 64)
CONV_NAMES = ("Conv0_A", "Conv1_A", "Conv0_C")
DENSE_UNITS = 256
BN_EPS, BN_MOMENTUM = 1e-3, 0.99
DROPOUT_P = 0.5

Config = collections.namedtuple("Config", "H W depth classes batchnorm")


def config(H, W, depth=2, classes=5, batchnorm=True):
    return Config(H, W, depth, classes, bool(batchnorm))


def param_shapes(cfg):
    shapes, cin = {}, cfg.depth
    for i, (name, c) in enumerate(zip(CONV_NAMES, FILTERS)):
        shapes[name + ".kernel"] = (3, 3, cin, c)
        shapes[name + ".bias"] = (c,)
        if cfg.batchnorm:
            shapes[f"bn{i}.gamma"] = (c,)
            shapes[f"bn{i}.beta"] = (c,)
        cin = c
    shapes["dense.kernel"] = (cin, DENSE_UNITS)
    shapes["dense.bias"] = (DENSE_UNITS,)
    if cfg.batchnorm:
        shapes["bn3.gamma"] = (DENSE_UNITS,)
        shapes["bn3.beta"] = (DENSE_UNITS,)
    shapes["dense_1.kernel"] = (DENSE_UNITS, cfg.classes)
    shapes["dense_1.bias"] = (cfg.classes,)
    return shapes


def moving_shapes(cfg):
    if not cfg.batchnorm:
        return {}
    out = {}
    for i, c in enumerate(FILTERS + (DENSE_UNITS,)):
        out[f"bn{i}.moving_mean"] = (c,)
        out[f"bn{i}.moving_variance"] = (c,)
    return out


def n_params(cfg):
    return sum(int(np.prod(s)) for s in param_shapes(cfg).values())


def init_params(cfg, seed_name="cnn_clas", dtype=np.float64):
    """Keras defaults (glorot_uniform kernels) with biases, gamma and beta perturbed so that tests see them."""
    out = {}
    for name, shp in param_shapes(cfg).items():
        key = f"{seed_name}/{name}"
        if name.endswith(".kernel"):
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


def synthetic_batch(cfg, B, seed_name="cnn_clas/data"):
    """(x NCHW [B, depth, H, W] in [0, 1), one-hot target [B, classes], labels [B])."""
    x = detrand.uniform(seed_name + "/x", (B, cfg.depth, cfg.H, cfg.W)).astype(np.float32)
    lab = detrand.randint(seed_name + "/y", (B,), 0, cfg.classes)
    y = np.zeros((B, cfg.classes), np.float32)
    y[np.arange(B), lab] = 1.0
    return x, y, lab


def keep_clear_of_flat_biases(cfg, params, x, margin=0.05):
    """A copy of `params` whose Conv2D / Dense(256) biases are lowered where a unit's pre-activation is positive on every sample
    (and pixel) of the batch `x`, until its smallest one is -margin.

    Why a test of several Adam steps needs it: with BatchNormalization behind the ReLU, the bias of a unit that is active everywhere
    has an analytically ZERO gradient (the normalisation removes a shift, so the gradients of the ReLU output sum to zero over the
    batch), and a unit at 3 samples is active on all of them one time in eight.  In fp32 that zero is rounding noise of ~1e-8, which
    Adam's m / (sqrt(v) + 1e-7) turns into an update of up to the full rate, where fp64 gives none: no fp32 implementation can
    then stay within 0.02 * lr of the fp64 trajectory.  A unit with a sample on either side of zero has a generic gradient; the
    margin (the pre-activations move by ~1e-2 per step at lr 1e-3) keeps it so over the steps a test takes."""
    out = {k: np.array(v, np.float64) for k, v in params.items()}
    if not cfg.batchnorm:            # no normalisation, no flat direction: nothing to keep clear of
        return out
    h = torch.tensor(np.asarray(x), dtype=torch.float64)
    for i, name in enumerate(CONV_NAMES):
        P = to_torch(out)
        pre = conv_valid(h, P[name + ".kernel"], P[name + ".bias"])
        lo = pre.amin((0, 2, 3)).numpy()
        out[name + ".bias"] -= np.where(lo > -margin, lo + margin, 0.0)
        h = torch.relu(conv_valid(h, P[name + ".kernel"], torch.tensor(out[name + ".bias"])))
        h = batch_norm(h, P[f"bn{i}.gamma"], P[f"bn{i}.beta"], (0, 2, 3))
        h = avg_pool2(h) if i < 2 else h.sum((2, 3)) / (h.shape[2] * h.shape[3])
    P = to_torch(out)
    lo = (h @ P["dense.kernel"] + P["dense.bias"]).amin(0).numpy()
    out["dense.bias"] -= np.where(lo > -margin, lo + margin, 0.0)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in out.items()}      # fp32-representable, as init_params gives them


def conv_valid(x, k_hwio, bias):
    """x NCHW, kernel HWIO: y[b, o, i, j] = bias[o] + sum_{ky, kx, c} x[b, c, i + ky, j + kx] k[ky, kx, c, o]."""
    H, W = x.shape[2] - 2, x.shape[3] - 2
    y = bias.view(1, -1, 1, 1).expand(x.shape[0], -1, H, W)
    for ky in range(3):
        for kx in range(3):
            y = y + torch.einsum("bcij,co->boij", x[:, :, ky:ky + H, kx:kx + W], k_hwio[ky, kx])
    return y


def avg_pool2(x):
    PH, PW = x.shape[2] // 2, x.shape[3] // 2
    return 0.25 * (x[:, :, 0:2 * PH:2, 0:2 * PW:2] + x[:, :, 0:2 * PH:2, 1:2 * PW:2] + x[:, :, 1:2 * PH:2, 0:2 * PW:2] + x[:, :, 1:2 * PH:2, 1:2 * PW:2])


def batch_norm(x, gamma, beta, dims, name=None, bn_state=None, training=True):
    """Training: batch statistics (biased variance) over `dims`; bn_state (name -> tensor) gets the Keras moving-statistics update
    (unbiased variance).  Inference: the moving statistics."""
    shape = [1] * x.dim()
    shape[1] = -1
    if training:
        mean = x.mean(dims)
        var = ((x - mean.view(shape)) ** 2).mean(dims)
        if bn_state is not None:
            n = x.numel() // x.shape[1]
            with torch.no_grad():
                bn_state[name + ".moving_mean"] = BN_MOMENTUM * bn_state[name + ".moving_mean"] + (1 - BN_MOMENTUM) * mean
                bn_state[name + ".moving_variance"] = BN_MOMENTUM * bn_state[name + ".moving_variance"] + (1 - BN_MOMENTUM) * var * n / max(n - 1, 1)
    else:
        mean, var = bn_state[name + ".moving_mean"], bn_state[name + ".moving_variance"]
    return (x - mean.view(shape)) / torch.sqrt(var.view(shape) + BN_EPS) * gamma.view(shape) + beta.view(shape)


def logits(P, x, cfg, training=True, mask=None, bn_state=None):
    """mask: the Dropout keep mask [B, 256], already scaled by 1 / (1 - p); None: no Dropout."""
    for i, name in enumerate(CONV_NAMES):
        x = torch.relu(conv_valid(x, P[name + ".kernel"], P[name + ".bias"]))
        if cfg.batchnorm:
            x = batch_norm(x, P[f"bn{i}.gamma"], P[f"bn{i}.beta"], (0, 2, 3), f"bn{i}", bn_state, training)
        x = avg_pool2(x) if i < 2 else x.sum((2, 3)) / (x.shape[2] * x.shape[3])
    x = torch.relu(x @ P["dense.kernel"] + P["dense.bias"])
    if cfg.batchnorm:
        x = batch_norm(x, P["bn3.gamma"], P["bn3.beta"], (0,), "bn3", bn_state, training)
    if mask is not None:
        x = x * mask
    return x @ P["dense_1.kernel"] + P["dense_1.bias"]


def log_softmax(z):
    zs = z - z.max(1, keepdim=True).values
    return zs - torch.log(torch.exp(zs).sum(1, keepdim=True))


def forward(P, x, cfg, **kw):
    return torch.exp(log_softmax(logits(P, x, cfg, **kw)))


def cross_entropy_rows(z, y):
    return -(y * log_softmax(z)).sum(1)


def n_correct(z, y):
    return int((torch.argmax(z, 1) == torch.argmax(y, 1)).sum())


def to_torch(params, dtype=torch.float64, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in params.items()}


def loss_and_grads(params, x, target, cfg, mask=None, global_batch=None, dtype=torch.float64, training=True, bn_state=None):
    """(loss = sum CE / global batch, sum CE, probabilities, logits, correct rows, gradients by name) of one train step."""
    P = to_torch(params, dtype, True)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    z = logits(P, t(x), cfg, training=training, mask=None if mask is None else t(mask), bn_state=bn_state)
    y = t(target)
    ce = cross_entropy_rows(z, y).sum()
    loss = ce / (z.shape[0] if global_batch is None else global_batch)
    loss.backward()
    return (float(loss.detach()), float(ce.detach()), torch.exp(log_softmax(z)).detach(), z.detach(), n_correct(z.detach(), y),
            {n: p.grad.detach() for n, p in P.items()})

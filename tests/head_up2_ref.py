"""Test infrastructure: fp64 restatement of the output head of a U-Net with resize_factor_0 = [2, 2] (dl_models/u_net.py:247-248),
UpSampling2D((2, 2)) -> Conv2D(2, (6, 6), padding='same'), and of the folded form csrc/head_up2.hip computes.

LITERAL form (the reference of every test): `repeat_interleave(2)` on both spatial axes, then the oracle's conv2d_same(., K, bias, 1);
autograd of that expression gives dx, dK and dbias.

FOLDED form.  x[i, j, c] is the coarse activation, a fine pixel is (2i + a, 2j + b), a, b in {0, 1}, K[o, dh, dw, c] the 6x6 kernel:
    u_a(dh) = (a + dh) >> 1          a = 0: dh 0,1 -> 0  2,3 -> 1  4,5 -> 2 (3 taps)     a = 1: dh 0 -> 0  1,2 -> 1  3,4 -> 2  5 -> 3 (4 taps)
    fold     K'[(o,a,b), u, v, c] = sum_{dh: u_a(dh) = u} sum_{dw: u_b(dw) = v} K[o, dh, dw, c]        dh outer, dw inner, both ascending
    forward  logit[o, 2i+a, 2j+b] = bias[o] + sum_{u,v,c} K'[(o,a,b), u, v, c] x[i+u-1, j+v-1, c]     a 4x4 'same' convolution (pad 1, 2)
    unfold   dK[o, dh, dw, c] = sum_{a,b} dK'[(o,a,b), u_a(dh), u_b(dw), c]                            a outer, b inner
ROUNDING RULE of bf16 storage (one rule): K' is summed in fp32 from the fp32 master kernel in the order above and rounded to bf16
ONCE - it is the trunk's bf16 work copy of this layer, not a sum of bf16-rounded taps (`fold_bf16`; the sums of at most four fp32
values are formed with fp32 additions in exactly that order, so the restatement and the kernel agree bit for bit).

Kernels here are in the layout of the master parameter, [o][dh][dw][c]; `hwio` turns one into what oracle.torch_ref takes.
`unet_forward` / `unet_loss_and_grads` assemble the whole half-resolution U-Net from oracle/torch_ref.py's own blocks with the literal
up-sampling in front of the head (oracle.torch_ref.forward applies none)."""
import numpy as np
import torch

from oracle import torch_ref as R

D = torch.float64


def hwio(k_odwc):
    return k_odwc.permute(1, 2, 3, 0)


def upsample2(x_nchw):
    return x_nchw.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def literal(x_nchw, k_odwc, bias):
    """[B,C,h,w] -> logits [B,2,2h,2w]."""
    return R.conv2d_same(upsample2(x_nchw), hwio(k_odwc), bias, 1)


def literal_grads(x_nchw, k_odwc, bias, dlogits):
    """(logits, dx, dK [2][6][6][C], dbias) of the literal form by autograd."""
    x = x_nchw.detach().clone().requires_grad_(True)
    k = k_odwc.detach().clone().requires_grad_(True)
    b = bias.detach().clone().requires_grad_(True)
    y = literal(x, k, b)
    (y * dlogits).sum().backward()
    return y.detach(), x.grad, k.grad, b.grad


def tap(a, d):
    return (a + d) >> 1


def fold(k_odwc, dtype=D):
    """K [2][6][6][C] -> K' [8][4][4][C], summed in `dtype` with dh outer, dw inner, both ascending."""
    k = k_odwc.to(dtype)
    out = torch.zeros((8, 4, 4, k.shape[-1]), dtype=dtype)
    for o in range(2):
        for a in range(2):
            for b in range(2):
                j = o * 4 + a * 2 + b
                for dh in range(6):
                    for dw in range(6):
                        u, v = tap(a, dh), tap(b, dw)
                        out[j, u, v] = out[j, u, v] + k[o, dh, dw]
    return out


def fold_bf16(k_odwc):
    """The bf16 work copy: fp32 sums in the order of `fold`, one rounding to bf16; returned as fp64."""
    return fold(k_odwc.float(), torch.float32).to(torch.bfloat16).to(D)


def unfold(g_fold):
    """dK' [8][4][4][C] -> dK [2][6][6][C]: the transpose of fold, a outer, b inner."""
    out = torch.zeros((2, 6, 6, g_fold.shape[-1]), dtype=g_fold.dtype)
    for o in range(2):
        for dh in range(6):
            for dw in range(6):
                for a in range(2):
                    for b in range(2):
                        out[o, dh, dw] = out[o, dh, dw] + g_fold[o * 4 + a * 2 + b, tap(a, dh), tap(b, dw)]
    return out


def depth_to_space(y8):
    """[B,8,h,w] with channel (o,a,b) -> [B,2,2h,2w]."""
    B, _, h, w = y8.shape
    return y8.reshape(B, 2, 2, 2, h, w).permute(0, 1, 4, 2, 5, 3).reshape(B, 2, 2 * h, 2 * w)


def space_to_depth(y2):
    """[B,2,2h,2w] -> [B,8,h,w]: the inverse of depth_to_space."""
    B, _, H, W = y2.shape
    return y2.reshape(B, 2, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, 8, H // 2, W // 2)


def folded(x_nchw, k_fold, bias):
    """The forward pass as the kernels compute it: 4x4 'same' convolution with the folded kernel, depth-to-space, bias."""
    y8 = R.conv2d_same(x_nchw, k_fold.permute(1, 2, 3, 0), None, 1)
    y = depth_to_space(y8)
    return y if bias is None else y + bias.view(1, 2, 1, 1)


def folded_grads(x_nchw, k_fold, dlogits):
    """(dx, dK') of the folded form by autograd."""
    x = x_nchw.detach().clone().requires_grad_(True)
    k = k_fold.detach().clone().requires_grad_(True)
    (folded(x, k, None) * dlogits).sum().backward()
    return x.grad, k.grad


# ---- the whole U-Net with resize_factor_0 = [2, 2]: oracle.torch_ref.forward with the literal up-sampling in front of the head
def unet_forward(P, spec, emb, cfg, training=True, dropout_mask=None, bn_state=None):
    x = spec
    skips = []
    for l in range(1, cfg.depth + 2):
        x = R.conv2d_same(x, P[f"enc{l}.down.kernel"], P[f"enc{l}.down.bias"], cfg.s0 if l == 1 else cfg.s)
        x = R.feature_block(x, P, f"enc{l}", cfg, bn_state, training, None, R._ident, R._ident)
        skips.append(x)
    B, h5, w5 = spec.shape[0], x.shape[2], x.shape[3]
    v = P["vec.embedding"][emb.long()].reshape(B, -1) @ P["vec.dense.kernel"] + P["vec.dense.bias"]
    if dropout_mask is not None:
        v = v * dropout_mask
    v = v.view(B, h5, w5, R.VEC_CH).permute(0, 3, 1, 2)
    x = x + R.conv2d_same(v, P["vec.conv.kernel"], P["vec.conv.bias"], 1)
    for l in range(cfg.depth, 0, -1):
        x = R.conv2d_transpose_same(x, P[f"dec{l}.up.kernel"], P[f"dec{l}.up.bias"], cfg.s)
        x = torch.cat([skips[l - 1], x], dim=1)
        x = R.conv_block_1(x, P, f"dec{l}.cb1a", cfg, bn_state, training, None)
        x = R.feature_block(x, P, f"dec{l}", cfg, bn_state, training, None, R._ident, R._ident)
    if cfg.s0 == 2:
        x = upsample2(x)                                           # UpSampling2D((2, 2)) (dl_models/u_net.py:247)
    return torch.sigmoid(R.conv2d_same(x, P["head.kernel"], P["head.bias"], 1))


def unet_loss_and_grads(params, spec_in, emb, spec_out, cfg, dropout_mask=None, bn_state=None, n_replicas=1):
    """oracle.torch_ref.loss_and_grads on `unet_forward`, in fp64: (loss, pred, grads)."""
    P = R.to_torch(params, D, True)
    t = lambda a: torch.as_tensor(np.asarray(a))
    mask = None if dropout_mask is None else t(dropout_mask).to(D)
    pred = unet_forward(P, t(spec_in).to(D), t(emb), cfg, True, mask, bn_state)
    loss = R.data_loss(t(spec_out).to(D), pred) + R.reg_loss(P, cfg, n_replicas)
    loss.backward()
    return float(loss.detach()), pred.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in P.items()}

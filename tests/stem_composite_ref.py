"""Test infrastructure: the stem's gradients through the next 3x3 layer, in numpy fp64, term by term as csrc/stem_composite.hip
states them - the 5x5 correlation S, the pixel sums T and the border terms E, F written with the predicate itself (a pixel p counts
for tap t1 when p + t1 - 1 lies outside the image), not with the kernel's row + column - corner decomposition.

Layouts: x [B,H,W,Ci], g [B,H,W,C1], w1 [C1,3,3,C0] (Conv2D kernel, [Cout][k][k][Cin]); dw0 [C0,3,3,Ci], db0 [C0].
"""
import numpy as np


def terms(x, g):
    """S [5,5,Ci,C1], T [C1], E [3,3,3,3,Ci,C1] (t0y,t0x,t1y,t1x), F [3,3,C1]."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    B, H, W, Ci = x.shape
    xp = np.zeros((B, H + 4, W + 4, Ci))
    xp[:, 2:H + 2, 2:W + 2] = x

    def corr(gm, dy, dx):        # sum_p x[p + (dy, dx)] * gm[p]
        return np.einsum("bhwi,bhwo->io", xp[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W], gm)

    S = np.zeros((5, 5, Ci, g.shape[3]))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            S[dy + 2, dx + 2] = corr(g, dy, dx)
    T = g.sum((0, 1, 2))
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    E = np.zeros((3, 3, 3, 3, Ci, g.shape[3]))
    F = np.zeros((3, 3, g.shape[3]))
    for t1y in range(3):
        for t1x in range(3):
            qy, qx = py + t1y - 1, px + t1x - 1
            outside = (qy < 0) | (qy >= H) | (qx < 0) | (qx >= W)
            gm = g * outside[None, :, :, None]
            F[t1y, t1x] = gm.sum((0, 1, 2))
            for t0y in range(3):
                for t0x in range(3):
                    E[t0y, t0x, t1y, t1x] = corr(gm, t0y + t1y - 2, t0x + t1x - 2)
    return S, T, E, F


def contract(S, T, E, F, w1, reg=0.0, w0=None):
    w1 = np.asarray(w1, np.float64)
    C1, _, _, C0 = w1.shape
    Ci = S.shape[2]
    dw0 = np.zeros((C0, 3, 3, Ci))
    db0 = np.zeros(C0)
    for t1y in range(3):
        for t1x in range(3):
            wt = w1[:, t1y, t1x, :]                       # [C1, C0]
            db0 += (T - F[t1y, t1x]) @ wt
            for t0y in range(3):
                for t0x in range(3):
                    a = S[t0y + t1y, t0x + t1x] - E[t0y, t0x, t1y, t1x]      # offset t0 + t1 - 2, index + 2
                    dw0[:, t0y, t0x, :] += (a @ wt).T
    if reg:
        dw0 = dw0 + reg * np.asarray(w0, np.float64)
    return dw0, db0


def stem_composite(x, g, w1, reg=0.0, w0=None):
    return contract(*terms(x, g), w1, reg, w0)

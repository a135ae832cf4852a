"""Test infrastructure: the stem's gradients through the next 3x3 layer, in numpy fp64, term by term as csrc/stem_composite.hip
states them - the 5x5 correlation S, the pixel sums T and the border terms E, F written with the predicate itself (a pixel p counts
for tap t1 when p + t1 - 1 lies outside the image), not with the kernel's row + column - corner decomposition.
chain() is the same result without any of these terms: one layer's data gradient, then the other's weight gradient.  The exact device
tests (tests/test_stem_composite_exact_gpu.py) compare with it on the integer data of exact_case().

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


def chain(x, g, w1, reg=0.0, w0=None):
    """The same two gradients from the two layers one after the other, with none of S, T, E, F: D = the data gradient of the
    zero-padded 'same' 3x3 convolution C0 -> C1 at G (the transposed convolution with the same kernel), then the stem's own weight
    gradient - the correlation of the zero-padded x with D - and bias gradient, the sum of D.  fp64 throughout; on integer data
    every sum is exact in any order."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    x, g, w1 = t(x), t(g), t(w1)
    B, H, W, Ci = x.shape
    C0 = w1.shape[3]
    d = F.conv_transpose2d(g.permute(0, 3, 1, 2), w1.permute(0, 3, 1, 2), padding=1)        # weight [C1][C0][3][3] -> D [B,C0,H,W]
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))
    dw0 = torch.zeros((C0, 3, 3, Ci), dtype=torch.float64)
    for ty in range(3):
        for tx in range(3):
            dw0[:, ty, tx, :] = torch.einsum("bohw,bihw->oi", d, xp[:, :, ty:ty + H, tx:tx + W])
    dw0, db0 = dw0.numpy(), d.sum((0, 2, 3)).numpy()
    if reg:
        dw0 = dw0 + reg * np.asarray(w0, np.float64)
    return dw0, db0


# The shapes (B, H, W) of the exact comparisons on integer data, each the smallest that reaches what stands beside it.  nblk =
# min(512, B * ceil(H / 16) * ceil(W / 256)) correlation partials, B frame partials per frame sum.
EXACT_SHAPES = [
    (1, 1, 1),        # B = 1; all four frame lines and all four corners are one pixel.  nblk 1
    (2, 1, 7),        # top line = bottom line.  nblk 2
    (2, 7, 1),        # left line = right line.  nblk 2
    (2, 2, 2),        # every pixel a corner.  nblk 2
    (1, 16, 256),     # exactly one correlation tile; a row line of exactly one chunk.  nblk 1
    (3, 17, 257),     # second tiles of one row and of one column; the right halo column 256 is the image edge.  nblk 12
    (2, 33, 515),     # three row blocks (dy ring at y0 = 0, 16, 32), three column blocks with both halos inside.  nblk 18
    (1, 1, 4096),     # the widest admitted image: 16 column blocks, a row line of 16 chunks.  nblk 16
    (2, 257, 3),      # a column line with a second chunk of one pixel.  nblk 34
    (32, 256, 1),     # exactly the grid cap, one block per workgroup; a column line of one full chunk.  nblk 512
    (33, 272, 2),     # 561 blocks on 512 workgroups: 49 walk a second block; column lines past a chunk; 33 frame partials.  nblk 512
]
REG_SHAPES = [(3, 17, 257), (33, 272, 2)]       # the shapes also run with the weight-decay term
_CASES = {}


def exact_case(B, H, W):
    """The integer data of one shape from the project's one data set (tests/exact_data.py), fp64 numpy: x [B,H,W,2], g [B,H,W,64],
    w1 [64,3,3,64] ([co1][k][k][co0]), w0 [64,3,3,8] (the stem kernel; channels >= 2, the padding of the 2-channel end, hold
    non-zero integers so that a weight-decay term shows there), and the chain's dw0 [64,3,3,2], db0 [64] without that term.
    Computed once per process and shared: callers do not modify what they get."""
    key = (B, H, W)
    if key not in _CASES:
        import exact_data as X
        n = f"sc{B}x{H}x{W}"
        x, g = X.acts(n + ".x", (B, H, W, 2)).numpy(), X.acts(n + ".g", (B, H, W, 64)).numpy()
        w1 = X.kernels(n + ".w1", (64, 3, 3, 64)).numpy()
        w0 = np.concatenate([X.kernels(n + ".w0", (64, 3, 3, 2)).numpy(), X.ints(n + ".w0pad", (64, 3, 3, 6), 1, 3).numpy()], axis=3)
        dw0, db0 = chain(x, g, w1)
        c = dict(x=x, g=g, w1=w1, w0=w0, dw0=dw0, db0=db0)
        for a in c.values():
            a.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]

"""The FFT form of `auralize` (csrc/auralize_fft.hip) restated with torch's CPU FFTs in fp32 / complex64, and its error bound.

Uniform partitioned overlap-save with block P, transforms of 2P samples, Q = ceil(K / P) partitions of h, J = ceil(L / P) blocks
anchored at n = 0:

    H_q = rfft(h[qP ... (q+1)P) | 0_P)          X_i = rfft(x[(i-1)P ... (i+1)P)), zeros outside 0 <= m < N
    Y_j = sum_{q <= min(j, Q-1)} H_q X_{j-q}    ascending q, complex64
    out[jP ... (j+1)P) = the LAST P samples of irfft(Y_j)

`bound` is the bound of include/unetrir.h, per element n of block j, with u = 2^-24 and Q_j = min(j, Q-1) + 1:

    |out[n] - y[n]| <= u (19 log2(2P) + 8 + Q_j) sum_{q < Q_j} |h_q|_1 |x[(j-q-1)P ... (j-q+1)P)|_2

The constants are derived in the header of csrc/auralize_fft.hip, not fitted; the bound is loose by orders of magnitude on random data,
which is why the tests also demand round(result) == y on integer data and that three deliberate mutations of this restatement break
the bound."""
import math

import numpy as np
import torch

C1, C2 = 19.0, 8.0
MUTATIONS = ("drop_last_partition", "shift_block", "first_half")


def _geometry(h, x, P, L):
    h = np.asarray(h)
    x = np.asarray(x)
    h2 = h[None] if h.ndim == 1 else h
    B, K = h2.shape
    x2 = x[None] if x.ndim == 1 else x
    assert x2.shape[0] in (1, B)
    N = x2.shape[1]
    L = N + K - 1 if L is None else L
    assert 1 <= L <= N + K - 1
    return h2, x2, B, K, N, L, -(-K // P), -(-L // P)


def _partitions(h2, P, Q, dtype):
    B, K = h2.shape
    hp = np.zeros((B, Q * P), dtype=dtype)
    hp[:, :K] = h2
    return hp.reshape(B, Q, P)


def _windows(x2, P, J, dtype):
    """[rows, J, 2P]: window i = x[(i-1)P ... (i+1)P) with zeros outside 0 <= m < N"""
    rows, N = x2.shape
    xe = np.zeros((rows, (J + 1) * P), dtype=dtype)
    n = min(N, J * P)
    xe[:, P:P + n] = x2[:, :n]
    return np.stack([xe[:, i * P:(i + 2) * P] for i in range(J)], axis=1)


def ols_ref(h, x, P, L=None, mutate=None):
    """h fp32 [B, K] or [K], x fp32 [N] (shared) or [B, N] -> fp32 [B, L] by the formulation above.  mutate: one of MUTATIONS, a
    deliberately wrong variant (the last partition of h dropped; block J // 2 shifted by one sample; the first instead of the last P
    samples of every inverse)."""
    assert mutate is None or mutate in MUTATIONS
    h2, x2, B, K, N, L, Q, J = _geometry(h, x, P, L)
    hp = np.zeros((B, Q, 2 * P), dtype=np.float32)
    hp[:, :, :P] = _partitions(h2, P, Q, np.float32)
    H = torch.fft.rfft(torch.from_numpy(hp))                                   # complex64 [B, Q, P + 1]
    X = torch.fft.rfft(torch.from_numpy(_windows(x2.astype(np.float32), P, J, np.float32)))        # [rows, J, P + 1]
    assert H.dtype == torch.complex64 and X.dtype == torch.complex64
    Y = torch.zeros((B, J, P + 1), dtype=torch.complex64)
    for q in range(Q - 1 if mutate == "drop_last_partition" else Q):           # ascending q; block j takes X_{j-q} for j >= q
        if q < J:
            Y[:, q:] += H[:, q:q + 1] * X[:, :J - q]
    y = torch.fft.irfft(Y, n=2 * P)                                            # fp32 [B, J, 2P]
    y = y[..., :P] if mutate == "first_half" else y[..., P:]
    y = y.numpy().copy()
    if mutate == "shift_block":
        y[:, J // 2] = np.roll(y[:, J // 2], 1, axis=-1)
    assert y.dtype == np.float32
    return y.reshape(B, J * P)[:, :L]


def bound(h, x, P, L=None):
    """fp64 [B, L]: the bound above for every element."""
    h2, x2, B, K, N, L, Q, J = _geometry(h, x, P, L)
    h1 = np.abs(_partitions(h2.astype(np.float64), P, Q, np.float64)).sum(axis=2)                  # [B, Q]
    xn = np.sqrt((_windows(x2.astype(np.float64), P, J, np.float64) ** 2).sum(axis=2))             # [rows, J]
    xn = np.broadcast_to(xn, (B, J))
    out = np.zeros((B, J))
    for j in range(J):
        qj = min(j, Q - 1) + 1
        s = sum(h1[:, q] * xn[:, j - q] for q in range(qj))
        out[:, j] = 2.0 ** -24 * (C1 * math.log2(2 * P) + C2 + qj) * s
    return np.repeat(out, P, axis=1)[:, :L]

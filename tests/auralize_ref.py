"""The definition `auralize` is held to, restated in fp64 as the literal double sum (no numpy.convolve, no FFT):

    y_b[n] = sum_{k=0}^{K-1} h_b[k] x_b[n - k],   x_b[m] = 0 outside 0 <= m < N,   0 <= n < L <= N + K - 1

with, per element, S[n] = sum_k |h[k] x[n - k]| and the number of non-zero terms: the two figures of the error bound of an fp32 sum
with one rounding per accumulated term, |y_fp32 - y| <= (terms + 2) 2^-24 S.  The loop over k is python's; the loop over n is one numpy
statement per tap (each y[n] still receives its terms one at a time, in ascending k)."""
import functools

import numpy as np


def convolve_ref(h, x, L=None):
    """h [B, K] or [K], x [N] (shared by every row) or [B, N] -> (y, S, terms), each [B, L] (or [L] for two vectors): fp64, fp64, int64."""
    h = np.asarray(h, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    single = h.ndim == 1 and x.ndim == 1
    h2 = h[None] if h.ndim == 1 else h
    B, K = h2.shape
    x2 = np.broadcast_to(x[None], (B, x.shape[0])) if x.ndim == 1 else x
    assert x2.shape[0] == B
    N = x2.shape[1]
    full = N + K - 1
    y = np.zeros((B, full))
    S = np.zeros((B, full))
    terms = np.zeros((B, full), dtype=np.int64)
    for k in range(K):
        p = h2[:, k, None] * x2                 # the terms h[k] x[n - k] for n = k ... k + N - 1
        y[:, k:k + N] += p
        S[:, k:k + N] += np.abs(p)
        terms[:, k:k + N] += p != 0.0
    L = full if L is None else L
    assert 1 <= L <= full
    out = (y[:, :L], S[:, :L], terms[:, :L])
    return tuple(a[0] for a in out) if single else out


def make_data(K, N, kind, B=3, seed=0):
    """fp32 h [B, K] and x [B, N]: kind "int" - integers with |h| <= 3, |x| <= 7 (every partial sum below 21 K <= 201 600 < 2^24: exact in
    fp32); kind "uniform" - uniform in [-1, 1] with magnitudes below 2^-10 lifted to it (no subnormal value, product or sum's term)."""
    rng = np.random.default_rng([seed, K, N, int(kind == "int")])
    if kind == "int":
        h = rng.integers(-3, 4, size=(B, K)).astype(np.float32)
        x = rng.integers(-7, 8, size=(B, N)).astype(np.float32)
    else:
        h = rng.uniform(-1.0, 1.0, size=(B, K)).astype(np.float32)
        x = rng.uniform(-1.0, 1.0, size=(B, N)).astype(np.float32)
        for a in (h, x):
            small = np.abs(a) < 2.0 ** -10
            a[small] = np.where(a[small] < 0, -2.0 ** -10, 2.0 ** -10)
    return h, x


@functools.lru_cache(maxsize=None)
def case(K, N, kind):
    """The data of one geometry and its references, computed once: h [3, K], x [3, N], `rows` = (y, S, terms) with x per row, `shared` =
    the same with x[0] for every row.  Read-only."""
    h, x = make_data(K, N, kind)
    rows = convolve_ref(h, x)
    shared = convolve_ref(h, x[0])
    for a in (h, x) + rows + shared:
        a.setflags(write=False)
    return h, x, rows, shared

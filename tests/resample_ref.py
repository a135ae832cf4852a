"""The definition the resampler is held to, restated in fp64 with NumPy alone.

Rates reduced to L / M (output / input, gcd 1), Z zero crossings (`zeros`) to each side, a rolloff and a Kaiser beta.  With
C = Z max(L, M), s = rolloff min(1, L / M) and W = C / L:

    h(tau) = s sinc(s tau) I0(beta sqrt(1 - (tau / W)^2)) / I0(beta)     for |tau| < W, else 0          sinc(u) = sin(pi u) / (pi u)
    y[m] = sum_n h(m M / L - n) x[n]        0 <= m < ceil(N L / M),   x[n] = 0 outside 0 <= n < N

The table [L][T], D = ceil(C / L), T = 2 D:  table[p][i] = h((p - (i - D + 1) L) / L), support by the integer test |p - (i - D + 1) L| < C,
and y[m] = sum_i table[p][i] x[q - D + 1 + i] with (q, p) = divmod(m M, L).  `resample_ref` walks that sum for ANY table with an even T
(window of output m starting at q - T/2 + 1) and returns, per output, the sum, S = sum |h x| and the number of non-zero products: the two
figures of the error bound of an fp32 sum with one rounding per accumulated term, |y_fp32 - y| <= (terms + 2) 2^-24 S.

`MUTATIONS` are one-line changes of the restatement; tests/test_resample_ref.py shows that each fails a named check."""
import functools
import math

import numpy as np

PRESETS = {"kaiser_best": (64, 0.9475937167399596, 14.769656459379492), "kaiser_fast": (16, 0.85, 8.555504641634386)}
MUTATIONS = ("phase_from_mL", "window_a_tap_late", "no_downsampling_gain", "support_closed_a_tap_wide")


def taps(L, M, zeros):
    return 2 * -(-zeros * max(L, M) // L)


def out_length(N, L, M):
    return -(-N * L // M)


def h_ref(k, L, M, zeros, rolloff, beta, mutation=None):
    """h at tau = k / L for an integer array k"""
    k = np.asarray(k, dtype=np.int64)
    C = zeros * max(L, M)
    s = rolloff * (1.0 if mutation == "no_downsampling_gain" else min(1.0, L / M))
    W = C / L
    tau = k / L
    inside = np.abs(tau) <= W + 1 if mutation == "support_closed_a_tap_wide" else np.abs(k) < C
    u = tau / W
    a = np.pi * (rolloff * min(1.0, L / M)) * tau
    sinc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    root = np.sqrt(np.clip(1.0 - u * u, 0.0, None))                 # the clip acts outside the support only (a mutation reaches there)
    return np.where(inside, s * sinc * np.i0(beta * root) / np.i0(beta), 0.0)


def table_ref(L, M, zeros, rolloff, beta, mutation=None):
    """fp64 [L, T]"""
    T = taps(L, M, zeros)
    D = T // 2
    p = np.arange(L, dtype=np.int64)[:, None]
    i = np.arange(T, dtype=np.int64)[None, :]
    return h_ref(p - (i - D + 1) * L, L, M, zeros, rolloff, beta, mutation)


def resample_ref(x, table, L, M, mutation=None):
    """x [B, N] or [N], table [L, T] (any; T even) -> (y, S, terms), each [B, Nout] (or [Nout]): fp64, fp64, int64.  One numpy statement
    per tap; every y[m] receives its terms one at a time, in ascending i."""
    x = np.asarray(x, dtype=np.float64)
    table = np.asarray(table, dtype=np.float64)
    single = x.ndim == 1
    x2 = x[None] if single else x
    B, N = x2.shape
    T = table.shape[1]
    assert table.shape[0] == L and T % 2 == 0 and math.gcd(L, M) == 1
    Nout = out_length(N, L, M)
    m = np.arange(Nout, dtype=np.int64)
    q, p = np.divmod(m * (L if mutation == "phase_from_mL" else M), L)
    start = q - T // 2 + (2 if mutation == "window_a_tap_late" else 1)
    y = np.zeros((B, Nout))
    S = np.zeros((B, Nout))
    terms = np.zeros((B, Nout), dtype=np.int64)
    for i in range(T):
        n = start + i
        ok = (n >= 0) & (n < N)
        prod = table[p, i][None, :] * np.where(ok[None, :], x2[:, np.clip(n, 0, N - 1)], 0.0)
        y += prod
        S += np.abs(prod)
        terms += prod != 0.0
    out = (y, S, terms)
    return tuple(a[0] for a in out) if single else out


def resample_def(x, L, M, zeros, rolloff, beta, mutation=None):
    """y of the definition for x [N]: the table of the definition through `resample_ref`"""
    return resample_ref(x, table_ref(L, M, zeros, rolloff, beta, mutation), L, M, mutation)[0]


def tone(rate, freq, n):
    return np.sin(2.0 * np.pi * freq * np.arange(n) / rate)


def int_table(L, T, seed=0):
    """An integer-valued table |h| <= 3, fp32 [L, T]: nothing like a filter, which is the point - the kernel does not interpret it."""
    rng = np.random.default_rng([seed, L, T, 7])
    return rng.integers(-3, 4, size=(L, T)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(L, M, zeros, N, kind, B=3):
    """The data of one geometry and its reference, computed once and read-only: (table fp32 [L, T], x fp32 [B, N], (y, S, terms)).
    kind "int": an integer table |h| <= 3 and |x| <= 7 (every partial sum below 21 T < 2^24: exact in fp32); kind "uniform": the
    kaiser_fast-shaped table of this geometry (rolloff 0.85, beta 8.555504641634386) rounded to fp32, and x uniform in [-1, 1] with
    magnitudes below 2^-10 lifted to it."""
    T = taps(L, M, zeros)
    rng = np.random.default_rng([L, M, zeros, N, int(kind == "int")])
    if kind == "int":
        table = int_table(L, T)
        x = rng.integers(-7, 8, size=(B, N)).astype(np.float32)
    else:
        table = table_ref(L, M, zeros, 0.85, 8.555504641634386).astype(np.float32)
        x = rng.uniform(-1.0, 1.0, size=(B, N)).astype(np.float32)
        small = np.abs(x) < 2.0 ** -10
        x[small] = np.where(x[small] < 0, -2.0 ** -10, 2.0 ** -10)
    ref = resample_ref(x, table, L, M)
    for a in (table, x) + ref:
        a.setflags(write=False)
    return table, x, ref

"""`auralize_path` (csrc/auralize_fft.hip) restated twice, and its error bound.

    n <= tau_0: y_0[n]     n >= tau_{R-1}: y_{R-1}[n]     tau_r <= n < tau_{r+1}: (1 - a) y_r[n] + a y_{r+1}[n],  a = (n - tau_r) / (tau_{r+1} - tau_r)

`path_ref64` is that definition with the fp64 double sums of tests/auralize_ref.py and gains from integer differences divided in fp64.
`path_ols_ref` is the kernel's algorithm in fp32 on tests/auralize_fft_ref.ols_ref (imported, not edited): per output block of P samples
the nodes r_lo ... r_hi found as the kernel finds them, every y_r from the complex64 overlap-save, gains by the kernel's fp32 arithmetic
(IEEE division, 1 - a, a zero gain skipped), the first term a product and the second a fused multiply-add, in ascending r.  `mutate`
selects one of MUTATIONS, deliberately wrong variants of one line each.

`bound` is the bound of include/unetrir.h, per element, with u = 2^-24, g_r the exact gains and E_r the bound of the stationary form
(tests/auralize_fft_ref.bound) for h_r:

    |out[n] - sum_r g_r[n] y_r[n]| <= sum_r g_r[n] E_r[n] + C u sum_r g_r[n] |y_r[n]|,    C = 4

(the division, the subtraction, the product and the fma: derived in the header of csrc/auralize_fft.hip)."""
import functools

import numpy as np

from auralize_fft_ref import bound as stationary_bound
from auralize_fft_ref import ols_ref
from auralize_ref import convolve_ref

P = 2048
C = 4.0
MUTATIONS = ("late_gain", "drop_r_hi", "block_gain", "block_anchor", "tail_from_r_minus_2")

# name: (R, K, N, times) - the smallest shapes that span the block and partition edges of the fixed P = 2048
CASES = {
    "a": (1, 33, 5000, (0,)),
    "b": (40, 33, 5000, tuple(100 + 64 * r for r in range(40))),          # 32 nodes in one block, a tail after the last node
    "c": (5, 2049, 9000, tuple(300 + 2048 * r for r in range(5))),
    "d": (4, 4097, 12000, tuple(777 + 4096 * r for r in range(4))),
    "e": (3, 9600, 20000, tuple(1000 + 8192 * r for r in range(3))),
    "f": (3, 100, 10000, (2048, 4096, 8192)),                             # nodes on block edges
    "g": (6, 2047, 7000, (-500, 37, 2047, 2079, 6000, 50000)),
}
# integer data for round(D out) == D y: the cases whose spacings are the power of two D, with amplitudes at which the restatement's own
# error times D stays at or below 1 / 8 (asserted in tests/test_auralize_path_ref.py): name: (amplitude, D)
INT_CASES = {"b": (8, 64), "c": (1, 2048)}         # case d with -1, 0, 1 gives 0.15 and case e more: not asked


def gains64(times, L):
    """fp64 [R, L]: the hat-function gains of the definition, from integer differences"""
    tau = np.asarray(times, dtype=np.int64)
    R = tau.shape[0]
    n = np.arange(L, dtype=np.int64)
    g = np.zeros((R, L))
    g[0, n <= tau[0]] = 1.0
    g[R - 1, n >= tau[R - 1]] = 1.0
    for r in range(R - 1):
        m = (n >= tau[r]) & (n < tau[r + 1])
        a = (n[m] - tau[r]) / float(tau[r + 1] - tau[r])
        g[r, m] = 1.0 - a
        g[r + 1, m] = a
    return g


def gain32(n, r, tau):
    """fp32 [len(n)]: the gain of node r at the samples n (int64) by the kernel's arithmetic"""
    R = tau.shape[0]
    tp, tc, tn = tau[max(r - 1, 0)], tau[r], tau[min(r + 1, R - 1)]
    g = np.zeros(n.shape, dtype=np.float32)
    before = n < tc
    if r == 0:
        g[before] = 1.0
    else:
        m = before & (n >= tp)
        g[m] = (n[m] - tp).astype(np.float32) / np.float32(tc - tp)
    if r == R - 1:
        g[~before] = 1.0
    else:
        m = ~before & (n < tn)
        g[m] = np.float32(1.0) - (n[m] - tc).astype(np.float32) / np.float32(tn - tc)
    assert g.dtype == np.float32
    return g


def _rows(h, x):
    """h [B, R, K], x [N] or [B, N] -> h as [B R, K] and x as one row per response"""
    B, R, K = h.shape
    x = np.asarray(x)
    return h.reshape(B * R, K), (x if x.ndim == 1 else np.repeat(x, R, axis=0))


def nodes64(h, x, L=None):
    """fp64 [B, R, L]: y_{b,r} = h_{b,r} * x_b, the literal double sums"""
    B, R, K = h.shape
    hr, xr = _rows(h, x)
    return convolve_ref(hr, xr, L)[0].reshape(B, R, -1)


def path_ref64(h, x, times, L=None, nodes=None):
    """h [B, R, K], x [N] or [B, N], times [R] -> fp64 [B, L]: the definition.  nodes: nodes64(h, x, L), if the caller has it."""
    y = nodes64(h, x, L) if nodes is None else nodes
    return np.einsum("rl,brl->bl", gains64(times, y.shape[-1]), y)


def block_nodes(times, j):
    """(r_lo, r_hi) of output block j: the last node with tau <= jP (else 0), the first with tau >= (j+1)P - 1 (else R - 1)"""
    tau = np.asarray(times, dtype=np.int64)
    R = tau.shape[0]
    lo = int(np.searchsorted(tau, j * P, side="right"))
    hi = int(np.searchsorted(tau, (j + 1) * P - 1, side="left"))
    r_lo = max(lo - 1, 0)
    return r_lo, max(min(hi, R - 1), r_lo)


def nodes_ols(h, x, L=None):
    """fp32 [B, R, L]: every y_{b,r} by the complex64 overlap-save, in the one batch of B R rows path_ols_ref makes"""
    B, R, K = h.shape
    hr, xr = _rows(h, x)
    y = ols_ref(hr, xr, P, L)
    return y.reshape(B, R, y.shape[1])


def path_ols_ref(h, x, times, L=None, mutate=None):
    """fp32 [B, L]: the kernel's algorithm on ols_ref.  mutate: one of MUTATIONS - the gains taken one sample late; r_hi dropped from
    every block that has more than one node; one gain per block (that of its first sample) instead of one per sample; the nodes
    re-anchored to the block edge at or before them; the tail after tau_{R-1} taken from node R - 2."""
    assert mutate is None or mutate in MUTATIONS
    B, R, K = h.shape
    y = nodes_ols(h, x, L)
    L = y.shape[-1]
    tau = np.asarray(times, dtype=np.int64)
    anchors = tau // P * P if mutate == "block_anchor" else tau
    out = np.zeros((B, L), dtype=np.float32)
    for j in range(-(-L // P)):
        n = np.arange(j * P, min((j + 1) * P, L), dtype=np.int64)
        r_lo, r_hi = block_nodes(anchors, j)
        if mutate == "drop_r_hi" and r_hi > r_lo:
            r_hi -= 1
        acc = np.zeros((B, n.shape[0]), dtype=np.float32)
        have = np.zeros(n.shape[0], dtype=bool)
        for r in range(r_lo, r_hi + 1):
            at = n - 1 if mutate == "late_gain" else np.full_like(n, n[0]) if mutate == "block_gain" else n
            g = gain32(at, r, anchors)
            yr = y[:, r, n[0]:n[0] + n.shape[0]]
            if mutate == "tail_from_r_minus_2" and r == R - 1 and R >= 2:
                yr = np.where((n >= tau[R - 1])[None], y[:, R - 2, n[0]:n[0] + n.shape[0]], yr)
            first = g[None] * yr                                  # fp32 product
            fused = (g[None].astype(np.float64) * yr.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            use = g != 0
            acc = np.where(use[None], np.where(have[None], fused, first), acc)
            have |= use
        out[:, n[0]:n[0] + n.shape[0]] = acc
    assert out.dtype == np.float32
    return out


def bound(h, x, times, nodes, L=None):
    """fp64 [B, L]: the bound above; nodes = nodes64(h, x, L)"""
    B, R, K = h.shape
    L = nodes.shape[-1] if L is None else L
    g = gains64(times, L)
    hr, xr = _rows(h, x)
    E = stationary_bound(hr, xr, P, L=L).reshape(B, R, L)
    return np.einsum("rl,brl->bl", g, E) + C * 2.0 ** -24 * np.einsum("rl,brl->bl", g, np.abs(nodes[..., :L]))


def peak_error(got, ref):
    """[B]: the largest error of every row over the row's peak"""
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max(axis=1) / np.abs(ref).max(axis=1)


def single_node(times, L):
    """[(r, samples)]: where one node has gain 1 - n <= tau_0, n >= tau_{R-1}, every n = tau_r - within 0 <= n < L"""
    tau = np.asarray(times, dtype=np.int64)
    R = tau.shape[0]
    n = np.arange(L, dtype=np.int64)
    res = [(0, n[n <= tau[0]]), (R - 1, n[n >= tau[R - 1]])] + [(r, n[n == tau[r]]) for r in range(R)]
    return [(r, idx) for r, idx in res if idx.size]


# The checks of tests/test_auralize_path_gpu.py as figures: each must be <= 1 for a result to pass.
def bound_figure(got, ref, lim):
    """check 1: the largest error over the bound"""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref) / lim))


def sharp_figure(got, ref, restated):
    """check 2: per row e = largest error over the row's peak; the largest e(got) / (4 e(restated) + 2^-22)"""
    return float(np.max(peak_error(got, ref) / (4.0 * peak_error(restated, ref) + 2.0 ** -22)))


def int_figure(got, ref, D):
    """check 3: the largest |D got - D ref| over 1/2: below 1, round(D got) == D ref (D ref is whole: power-of-two spacings)"""
    want = D * ref
    assert np.array_equal(want, np.rint(want))
    return float(np.max(np.abs(D * np.asarray(got, dtype=np.float64) - want)) / 0.5)


def make_data(name, kind):
    """fp32 h [3, R, K], x [3, N]: kind "uniform" - uniform in [-1, 1] with magnitudes below 2^-10 lifted to it; "int" - integers of
    magnitude up to INT_CASES[name][0]"""
    R, K, N, _ = CASES[name]
    rng = np.random.default_rng([7, sorted(CASES).index(name), int(kind == "int")])
    if kind == "int":
        amp = INT_CASES[name][0]
        return (rng.integers(-amp, amp + 1, size=(3, R, K)).astype(np.float32), rng.integers(-amp, amp + 1, size=(3, N)).astype(np.float32))
    h = rng.uniform(-1.0, 1.0, size=(3, R, K)).astype(np.float32)
    x = rng.uniform(-1.0, 1.0, size=(3, N)).astype(np.float32)
    for a in (h, x):
        small = np.abs(a) < 2.0 ** -10
        a[small] = np.where(a[small] < 0, -2.0 ** -10, 2.0 ** -10)
    return h, x


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """The data of one case and its references, computed once and read-only: h [3, R, K], x [3, N], times, and for x per row (`rows`) and
    x[0] for every row (`shared`) the pair (nodes64, path_ref64)."""
    h, x = make_data(name, kind)
    times = CASES[name][3]
    res = []
    for xs in (x, x[0]):
        nodes = nodes64(h, xs)
        res.append((nodes, path_ref64(h, xs, times, nodes=nodes)))
    for a in (h, x) + res[0] + res[1]:
        a.setflags(write=False)
    return h, x, times, res[0], res[1]

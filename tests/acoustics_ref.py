"""The yardstick of the room-acoustics tests: a NumPy fp64 restatement of the definitions behind `unet_rir_amd.acoustics` and
`Evaluator(acoustics=True)` (include/unetrir.h, "room-acoustic figures of impulse responses").

For one waveform h[0..T) (fp32 samples, all arithmetic fp64), sample rate fs and integer windows n_pre, n_dir, n_early:

    e = h*h
    n0 = argmax |h|                       lowest index on ties; |h| compared as fp32
    s = max(0, n0 - n_pre)
    S[n] = sum_{k >= n} e[k]              Schroeder backward integral
    E_tot = S[s]
    E_dir = sum_{s <= n <= min(T-1, n0+n_dir)} e[n]
    E_early = sum_{s <= n < min(T, s+n_early)} e[n]
    M1 = sum_{n >= s} (n - s) e[n]
    N_fit = #{ n >= s : 10*S[n] >= E_tot }
    drr = 10 log10(E_dir / (E_tot - E_dir))         dB
    c50 = 10 log10(E_early / (E_tot - E_early))     dB
    ts = M1 / E_tot / fs * 1e3                      ms
    L[k] = 10 log10(S[s+k] / E_tot), k = 0..N_fit-1
    slope = (N SkL - Sk SL) / (N Sk2 - Sk^2) * fs   dB/s; Sk and Sk2 from their closed forms
    edt = -60 / slope                               s; NaN when N_fit < 2

Degenerate input follows IEEE arithmetic (all-zero row: NaN; no late energy: +inf dB; flat decay curve: edt = -inf).
`tests/test_acoustics.py` holds this file to closed forms it was not written from.
"""
import numpy as np

FIGURES = ("n0", "e_tot", "e_dir", "e_early", "m1", "n_fit", "drr", "c50", "ts", "edt")
ERRORS = ("toa_ms", "drr_db", "c50_db", "ts_ms", "edt_pct")
RAW = 6                                 # the first six columns are sums and counts, the last four derived


def figures(h, n_pre=120, n_dir=120, n_early=2400, fs=48000.0, detail=False):
    """One waveform -> fig[10] in the order of FIGURES (detail=True: also (s, S, L), the curve the regression ran over)."""
    h = np.asarray(h, dtype=np.float32)
    T = len(h)
    e = h.astype(np.float64) ** 2
    n0 = int(np.argmax(np.abs(h)))                                    # first occurrence of the maximum
    s = max(0, n0 - n_pre)
    S = np.cumsum(e[::-1])[::-1]
    e_tot = S[s]
    e_dir = e[s:min(T - 1, n0 + n_dir) + 1].sum()
    e_early = e[s:min(T, s + n_early)].sum()
    m1 = (np.arange(T - s, dtype=np.float64) * e[s:]).sum()
    n_fit = int(np.count_nonzero(10.0 * S[s:] >= e_tot))
    with np.errstate(divide="ignore", invalid="ignore"):
        drr = 10.0 * np.log10(np.float64(e_dir) / (e_tot - e_dir))
        c50 = 10.0 * np.log10(np.float64(e_early) / (e_tot - e_early))
        ts = np.float64(m1) / e_tot / fs * 1e3
        L = 10.0 * np.log10(S[s:s + n_fit] / e_tot)
        N = float(n_fit)
        k = np.arange(n_fit, dtype=np.float64)
        sk, sk2 = N * (N - 1.0) / 2.0, (N - 1.0) * N * (2.0 * N - 1.0) / 6.0
        slope = (N * (k * L).sum() - sk * L.sum()) / np.float64(N * sk2 - sk * sk) * fs
        edt = np.float64(-60.0) / slope if n_fit >= 2 else np.nan
    fig = np.array([n0, e_tot, e_dir, e_early, m1, n_fit, drr, c50, ts, edt], dtype=np.float64)
    return (fig, s, S, L) if detail else fig


def batch_figures(wav, **kw):
    return np.stack([figures(h, **kw) for h in wav])


def condition(L):
    """The regression's condition number (N S|kL| + Sk S|L|) / |N SkL - Sk SL|."""
    N = float(len(L))
    k = np.arange(len(L), dtype=np.float64)
    return (N * np.abs(k * L).sum() + k.sum() * np.abs(L).sum()) / abs(N * (k * L).sum() - k.sum() * L.sum())


def errors(fig_p, fig_t, fs=48000.0):
    """(err[5], pred[5], true[5], counts[5] bool) of one (pred, true) pair of figure rows.  err holds the IEEE value whether the
    figure counts or not; it counts when both sides are finite, edt additionally when both are > 0."""
    fp, ft = np.asarray(fig_p, dtype=np.float64), np.asarray(fig_t, dtype=np.float64)
    p = np.array([fp[0] / fs * 1e3, fp[6], fp[7], fp[8], fp[9]])
    t = np.array([ft[0] / fs * 1e3, ft[6], ft[7], ft[8], ft[9]])
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(p - t)
        err[0] = abs(fp[0] - ft[0]) / fs * 1e3
        err[4] = 100.0 * abs(p[4] - t[4]) / t[4]
    ok = np.isfinite(p) & np.isfinite(t)
    ok[4] = ok[4] and p[4] > 0 and t[4] > 0
    return err, p, t, ok


def fold(fig, group, n_groups, fs=48000.0):
    """fig [N, 2, 10], group [N] ints -> (err [N, 5], acc [n_groups + 1, 20]): per figure the columns sum of errors, sum of pred
    values, sum of true values, count; row 0 every pair, row 1 + g the pairs of room g (any other group value: row 0 only)."""
    fig = np.asarray(fig, dtype=np.float64)
    acc = np.zeros((n_groups + 1, 4 * len(ERRORS)))
    errs = np.zeros((len(fig), len(ERRORS)))
    for b in range(len(fig)):
        err, p, t, ok = errors(fig[b, 0], fig[b, 1], fs)
        errs[b] = err
        rows = [0] + ([1 + int(group[b])] if 0 <= int(group[b]) < n_groups else [])
        for f in range(len(ERRORS)):
            if ok[f]:
                for r in rows:
                    acc[r, 4 * f:4 * f + 4] += (err[f], p[f], t[f], 1.0)
    return errs, acc


def result_block(acc):
    """acc [G + 1, 20] -> the "acoustics" block of Evaluator.result()."""
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for f, name in enumerate(ERRORS):
            n = acc[:, 4 * f + 3]
            out[name] = {"err": (acc[:, 4 * f] / n).tolist(), "pred": (acc[:, 4 * f + 1] / n).tolist(),
                         "true": (acc[:, 4 * f + 2] / n).tolist(), "n": [int(v) for v in n]}
    return out


# ---- the waveforms of the device tests ----------------------------------------------------------------------------------

SHAPES = ((5, 9600, 120, 120, 2400), (3, 1000, 20, 16, 100), (2, 257, 5, 8, 40))            # (B, T, n_pre, n_dir, n_early)
PEAKS = {9600: ((300, 1500.0), (5000, 3000.0), (0, 4000.0), (1200, 2200.0), (2500, 1800.0)),      # (peak, tau) per row
         1000: ((37, 150.0), (599, 120.0), (250, 200.0)),
         257: ((3, 60.0), (20, 45.0))}


def normal(name, shape):
    """Standard normal numbers by Box-Muller from two `oracle.detrand` uniform streams."""
    from oracle import detrand
    u1 = detrand.uniform(name + "/u1", shape, dtype=np.float64)
    u2 = detrand.uniform(name + "/u2", shape, dtype=np.float64)
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


def decay_rows(name, T, cases, integer=True):
    """One impulse response per (peak, tau): silence, a spike of 2000 at `peak`, behind it 600 g[n] exp(-(n - peak) / tau) with g
    standard normal - rounded to integers when `integer` - and the whole row times 2^-15.  The integer rows are exact in fp32
    and every energy sum of theirs is exact in fp64 in any order (|value| < 2^12, so e 2^30 < 2^24 and the largest sum, M1,
    stays below T^2 2^24 < 2^53)."""
    g = normal(f"acoustics/{name}/{T}", (len(cases), T))
    rows = np.zeros((len(cases), T))
    n = np.arange(T, dtype=np.float64)
    for b, (peak, tau) in enumerate(cases):
        tail = 600.0 * g[b] * np.exp(-(n - peak) / tau)
        rows[b] = np.where(n > peak, np.rint(tail) if integer else tail, 0.0)
        rows[b, peak] = 2000.0
    return (rows * 2.0 ** -15).astype(np.float32)

"""The room-acoustic figures without a GPU: the NumPy restatement (tests/acoustics_ref.py) against closed forms it was not
written from, its IEEE results on degenerate rows, the entry points' argument checks, and the fourth report file.

Closed forms.  For h[n] = r^n, r = exp(-1/tau), n_pre = 0 (so n0 = s = 0), q = r^2 and eps = q^T:
    S[n] = (q^n - eps) / (1 - q)      E_dir = (1 - q^(n_dir+1)) / (1 - q)      E_early = (1 - q^n_early) / (1 - q)
    M1 = (q - T q^T + (T - 1) q^(T+1)) / (1 - q)^2
    N_fit = 1 + floor(-tau/2 ln((1 + 9 eps) / 10))        from 10 (q^n - eps) >= 1 - eps
    L[k] = k 20 log10(r) + d[k],   d[k] = 10 log10((1 - eps / q^k) / (1 - eps)),   and edt -> 3 ln(10) tau / fs as eps -> 0.
The restatement squares the fp32 samples, each within 2^-24 relative of r^n, so every e[n] - and every sum of them, all terms
being non-negative - is within u = 2^-23 (1 + 2^-25) relative of the closed form; fp64 summation adds T 2^-53, which the bounds
below absorb in their rounding up:
    raw sums            1.3e-7 relative (u = 1.19e-7)
    drr, c50            numerator and denominator each within u: 10 / ln(10) * 2u = 1.04e-6 -> 1.1e-6 dB
    ts                  a ratio of two sums: 2u -> 2.5e-7 relative
    edt                 the slope is linear in L with weights w[k] = (N k - Sk) / (N Sk2 - Sk^2) fs.  L[k] is off the straight line
                        by the rounding term (1.1e-6 dB, as for drr) plus the truncation term |d[k]| <= 10 / ln(10) * 10 eps / (1 -
                        10 eps) (q^k >= 1/10 inside the fit), so |slope - 20 log10(r) fs| <= sum|w| (1.1e-6 + max|d|); relative to
                        the slope that is the bound on edt, computed in the test from N, tau and eps.
"""
import csv
import math
import os

import numpy as np
import pytest

import acoustics_ref as A

FS = 48000.0


@pytest.mark.parametrize("tau,T,n_dir,n_early", [(400.0, 9600, 120, 2400),        # T / tau = 24: eps = 1.4e-21, the limit itself
                                                  (250.0, 2000, 30, 300),          # T / tau = 8: eps = 1.1e-7, the truncation term shows
                                                  (33.3, 257, 8, 40)])
def test_restatement_against_the_exponential_decay(tau, T, n_dir, n_early):
    r = math.exp(-1.0 / tau)
    q = r * r
    eps = q ** T
    h = (r ** np.arange(T, dtype=np.float64)).astype(np.float32)
    fig, s, S, L = A.figures(h, 0, n_dir, n_early, FS, detail=True)
    e_tot, e_dir, e_early = (1 - eps) / (1 - q), (1 - q ** (n_dir + 1)) / (1 - q), (1 - q ** n_early) / (1 - q)
    m1 = (q - T * q ** T + (T - 1) * q ** (T + 1)) / (1 - q) ** 2
    x = -tau / 2 * math.log((1 + 9 * eps) / 10)
    assert min(x - math.floor(x), math.ceil(x) - x) > 1e-3, "the end of the fit must not hang on the samples' rounding"
    n_fit = 1 + math.floor(x)
    want = [0, e_tot, e_dir, e_early, m1, n_fit, 10 * math.log10(e_dir / (e_tot - e_dir)), 10 * math.log10(e_early / (e_tot - e_early)),
            m1 / e_tot / FS * 1e3, 3 * math.log(10) * tau / FS]
    assert s == 0 and fig[0] == 0 and fig[5] == n_fit
    n = np.arange(T)
    assert np.all(np.abs(S - (q ** n - eps) / (1 - q)) <= 1.3e-7 * (q ** n - eps) / (1 - q))
    k = np.arange(n_fit, dtype=np.float64)
    w = (n_fit * k - k.sum()) / (n_fit * (k * k).sum() - k.sum() ** 2) * FS
    d_max = 10 / math.log(10) * 10 * eps / (1 - 10 * eps)
    edt_rel = np.abs(w).sum() * (1.1e-6 + d_max) / abs(20 * math.log10(r) * FS)
    edt_rel = edt_rel / (1 - edt_rel)                                   # 1 / (1 + x) - 1 for |x| <= edt_rel
    bounds = [0, 1.3e-7, 1.3e-7, 1.3e-7, 1.3e-7, 0, None, None, 2.5e-7, edt_rel]
    for c, name in enumerate(A.FIGURES):
        err = abs(fig[c] - want[c])
        print(f"tau {tau} T {T} {name}: got {fig[c]!r} want {want[c]!r} abs err {err:.3e} bound {bounds[c]}")
        if bounds[c] is None:
            assert err <= 1.1e-6, name
        else:
            assert err <= bounds[c] * abs(want[c]), name
    assert edt_rel < (1e-6 if eps < 1e-12 else 1e-4)                    # the bounds themselves are tight enough to mean something


def test_halving_decay_is_exact():
    """h[n] = 2^-n is exact in fp32 and all its sums are exact in fp64: the raw columns EQUAL the closed form."""
    T = 40
    h = (0.5 ** np.arange(T)).astype(np.float32)
    fig = A.figures(h, 0, 3, 10, FS)
    q, S0 = 0.25, (1 - 0.25 ** T) / 0.75
    assert fig[0] == 0 and fig[1] == S0 and fig[2] == (1 - q ** 4) / 0.75 and fig[3] == (1 - q ** 10) / 0.75
    assert fig[4] == sum(n * q ** n for n in range(T))
    assert fig[5] == 2                                                  # 0 dB and -6.02 dB; the third point is at -12.04 dB
    assert abs(fig[9] - 3 / (math.log10(2) * FS)) <= 1e-12 * fig[9]     # two points: the slope is L[1] - L[0] = 20 log10(1/2)


def test_degenerate_rows():
    nan, inf = float("nan"), float("inf")
    # all zero: n0 = 0, every n passes 10 * 0 >= 0, every derived figure 0/0
    f = A.figures(np.zeros(50, np.float32), 5, 5, 20, FS)
    assert f[0] == 0 and f[1] == 0 and f[5] == 50 and np.isnan(f[6:]).all()
    # the peak at index 0, nothing else: s = 0, all the energy is direct and early -> +inf dB, ts = 0; S drops to 0 behind the
    # peak, so the fit holds one point -> edt NaN
    h = np.zeros(50, np.float32)
    h[0] = 1.0
    f = A.figures(h, 5, 5, 20, FS)
    assert f[0] == 0 and list(f[1:6]) == [1, 1, 1, 0, 1] and f[6] == inf and f[7] == inf and f[8] == 0 and np.isnan(f[9])
    # the peak at T - 1 behind silence: s = T - 1 - n_pre, the decay curve is flat over the n_pre + 1 samples of the fit -> edt = -inf
    h = np.zeros(50, np.float32)
    h[49] = -2.0
    f = A.figures(h, 5, 5, 20, FS)
    assert f[0] == 49 and list(f[1:6]) == [4, 4, 4, 20, 6] and f[6] == inf and f[7] == inf and f[8] == 5 / FS * 1e3 and f[9] == -inf
    # the same without a pre-window: one point
    f = A.figures(h, 0, 5, 20, FS)
    assert f[5] == 1 and np.isnan(f[9]) and f[8] == 0
    # T = 1
    f = A.figures(np.array([3.0], np.float32), 120, 120, 2400, FS)
    assert f[0] == 0 and list(f[1:6]) == [9, 9, 9, 0, 1] and f[6] == inf and f[7] == inf and f[8] == 0 and np.isnan(f[9])
    f = A.figures(np.array([0.0], np.float32), 120, 120, 2400, FS)
    assert f[0] == 0 and f[5] == 1 and np.isnan(f[6:]).all()
    # two equal peaks of opposite sign: the lower index wins
    h = np.zeros(60, np.float32)
    h[[20, 40]] = (-0.75, 0.75)
    h[41:] = 0.01
    f = A.figures(h, 2, 2, 30, FS)
    assert f[0] == 20 and np.isfinite(f).all()
    assert A.figures(-h, 2, 2, 30, FS)[0] == 20


def test_counting_rule_is_per_figure():
    """A figure's error counts only when both sides are finite (edt: and positive); the other figures of the pair still count."""
    true = A.decay_rows("count", 257, A.PEAKS[257], integer=True)
    ft = A.batch_figures(true, n_pre=5, n_dir=8, n_early=40)
    assert np.isfinite(ft).all() and (ft[:, 9] > 0).all()
    last = np.zeros(257, np.float32)
    last[256] = 1.0                                                     # peak at the last sample: drr = c50 = +inf, edt = -inf
    fp = np.stack([A.figures(np.zeros(257, np.float32), 5, 8, 40), A.figures(last, 5, 8, 40)])
    fig = np.stack([fp, ft], axis=1)
    err, acc = A.fold(fig, [0, 7], 2)
    counts = acc[:, 3::4]
    assert counts[0].tolist() == [2, 0, 0, 1, 0]                        # toa from both, ts from the second, nothing else
    assert counts[1].tolist() == [1, 0, 0, 0, 0] and counts[2].tolist() == [0, 0, 0, 0, 0]          # group 7 is global only
    assert err[0, 0] == ft[0, 0] / FS * 1e3 and err[1, 0] == (256 - ft[1, 0]) / FS * 1e3
    assert np.isnan(err[0, 1:]).all() and err[1, 1] == np.inf and err[1, 2] == np.inf and np.isfinite(err[1, 3]) and err[1, 4] == np.inf
    assert acc[0, 0] == err[0, 0] + err[1, 0] and acc[0, 12] == err[1, 3]
    block = A.result_block(acc)
    assert block["toa_ms"]["n"] == [2, 1, 0] and np.isnan(block["drr_db"]["err"]).all() and np.isnan(block["toa_ms"]["err"][2])
    # a negative edt on one side does not count although it is finite
    e, p, t, ok = A.errors([0, 1, 1, 1, 1, 3, 1.0, 2.0, 3.0, -0.5], ft[0])
    assert ok.tolist() == [True, True, True, True, False] and np.isfinite(e).all()


def test_entry_points_reject_invalid_arguments_without_gpu():
    """UNETRIR_EINVAL = 10001 before the device is touched (the pointers are never followed)."""
    import ctypes as C
    import unet_rir_amd
    L = unet_rir_amd._lib.lib()
    p = C.c_void_p(4096)
    fig = L.unetrir_acoustic_figures_f32
    assert fig(None, p, 2, 100, 1, 1, 10, FS, p, None) == 10001              # wav_a
    assert fig(p, p, 2, 100, 1, 1, 10, FS, None, None) == 10001              # fig
    assert fig(p, None, 0, 100, 1, 1, 10, FS, p, None) == 10001              # B
    assert fig(p, None, 2, 0, 1, 1, 10, FS, p, None) == 10001                # T
    assert fig(p, None, 2, 100, -1, 1, 10, FS, p, None) == 10001             # n_pre
    assert fig(p, None, 2, 100, 1, -1, 10, FS, p, None) == 10001             # n_dir
    assert fig(p, None, 2, 100, 1, 1, -1, FS, p, None) == 10001              # n_early
    assert fig(p, None, 2, 100, 1, 1, 10, 0.0, p, None) == 10001             # fs
    assert fig(p, None, 2, 100, 1, 1, 10, -FS, p, None) == 10001
    assert fig(p, None, 2, 100, 1, 1, 10, float("nan"), p, None) == 10001
    acc = L.unetrir_acoustic_accumulate
    assert acc(None, p, 2, 5, FS, None, p, None) == 10001                    # fig
    assert acc(p, None, 2, 5, FS, None, p, None) == 10001                    # group
    assert acc(p, p, 2, 5, FS, None, None, None) == 10001                    # acc
    assert acc(p, p, 0, 5, FS, None, p, None) == 10001                       # B
    assert acc(p, p, 2, -1, FS, None, p, None) == 10001                      # G
    assert acc(p, p, 2, 5, 0.0, None, p, None) == 10001                      # fs


def test_host_wrappers_refuse_cpu_tensors():
    import torch
    import unet_rir_amd as U
    w = torch.zeros((2, 100))
    with pytest.raises(ValueError):
        U.acoustics(w)
    with pytest.raises(ValueError):
        U.ops.acoustic_figures(w, None, torch.zeros((2, 1, 10), dtype=torch.float64))
    with pytest.raises(ValueError):
        U.ops.acoustic_accumulate(torch.zeros((2, 2, 10), dtype=torch.float64), torch.zeros(2, dtype=torch.int32),
                                  torch.zeros((6, 20), dtype=torch.float64))
    with pytest.raises(ValueError):
        U.Evaluator(None, acoustics=True, fs=0)
    assert U.evaluate.ACOUSTIC_FIGURES == A.FIGURES and U.evaluate.ACOUSTIC_ERRORS == A.ERRORS


def _hand_made_result():
    import unet_rir_amd as U
    rooms = list(U.evaluate.ROOMS) + ["Cellar"]
    rows = len(rooms) + 1
    res = {"rooms": rooms, "n": [9, 2, 3, 0, 1, 2, 1]}
    for k, m in enumerate(U.evaluate.METRICS):
        res[m] = [float("nan") if r == 3 else 0.001 * (k + 1) * (r + 1.5) - (30 if m.startswith("mis") else 0) for r in range(rows)]
    res["timing"] = {"n_batches": 3, "batch_size": 3, "inference_s": 0.0123, "postprocess_s": 0.00045, "loss_s": 0.00012, "total_s": 1.5}
    block = {}
    for k, name in enumerate(U.evaluate.ACOUSTIC_ERRORS):
        n = [9 - k, 2, 3 - (k > 2), 0, 1, 2, 1 - (k == 4)]
        block[name] = {"err": [float("nan") if c == 0 else 0.1 / 3 * (k + 1) + r for r, c in enumerate(n)],
                       "pred": [float("nan") if c == 0 else -1.25e-7 * (k + 2) * (r + 1) for r, c in enumerate(n)],
                       "true": [float("nan") if c == 0 else 1e9 / 7 * (k + 1) + r for r, c in enumerate(n)], "n": n}
    res["acoustics"] = block
    return res


def test_report_files(tmp_path):
    import unet_rir_amd as U
    from unet_rir_amd.rooms import UTS_ROOMS
    res = _hand_made_result()
    bare = {k: v for k, v in res.items() if k != "acoustics"}
    with_dir, bare_dir = str(tmp_path / "with"), str(tmp_path / "bare")
    paths = U.write_report(res, with_dir, "net")
    assert [os.path.basename(p) for p in paths] == ["net_losses.csv", "net_infer_time.csv", "net_results_inference.txt",
                                                    "net_acoustics.csv"]
    assert sorted(os.listdir(with_dir)) == sorted(os.path.basename(p) for p in paths)
    bare_paths = U.write_report(bare, bare_dir, "net")
    assert len(bare_paths) == 3 and sorted(os.listdir(bare_dir)) == sorted(os.path.basename(p) for p in bare_paths)
    for a, b in zip(paths, bare_paths):
        assert open(a, "rb").read() == open(b, "rb").read(), os.path.basename(a)
    # the fourth file, parsed back
    with open(paths[3], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["room", "figure", "mean error", "mean pred", "mean true", "n samples", "rt60 ms"]
    labels = ["Global", "HemiAnechoic", "Large", "Medium", "Shoe", "Small", "Cellar"]
    body = rows[1:]
    assert len(body) == len(labels) * len(U.evaluate.ACOUSTIC_ERRORS)
    same = lambda a, b: (math.isnan(a) and math.isnan(b)) or a == b
    for i, label in enumerate(labels):
        for k, name in enumerate(U.evaluate.ACOUSTIC_ERRORS):
            row = body[i * len(U.evaluate.ACOUSTIC_ERRORS) + k]
            v = res["acoustics"][name]
            assert row[0] == label and row[1] == name and int(row[5]) == v["n"][i]
            assert same(float(row[2]), v["err"][i]) and same(float(row[3]), v["pred"][i]) and same(float(row[4]), v["true"][i])
            room = res["rooms"][i - 1] if i else None
            assert row[6] == (str(UTS_ROOMS[room][-1]) if room in UTS_ROOMS else "")
    assert body[len(U.evaluate.ACOUSTIC_ERRORS)][6] == "52" and body[2 * len(U.evaluate.ACOUSTIC_ERRORS)][6] == "1281"

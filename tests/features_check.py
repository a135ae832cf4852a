"""Per-element bounds for the waveform <-> feature kernels (csrc/features.hip), the plain NumPy twins of the kernels' arithmetic
from which the bounds' constants are measured, and the two checking functions the CPU and GPU tests share.

Both sides of every comparison start from the same fp32 inputs, compute in fp64 and round each output to fp32 once.  The fp64
disagreement of analysis frame f is modelled as delta_f = EPS_ANALYSIS * sum_n |xw_f[n]| (xw: the windowed frame), that of a
synthesis sample t as EPS_SYNTHESIS * A_t with A_t = sum_f w_f(t) (1/n_fft) sum_k c_k |X_kf| / envelope(t), the absolute-value
twin of the sum the kernel forms (c_k = 1 for DC and Nyquist, 2 otherwise).

  raw analysis           |S_dev - S| <= 2^-24 (1 + pi) |S| + delta_f                      (S_dev = amp exp(i ph) of the fp32 planes)
  normalised amplitude   |a_dev - a| <= 2^-24 |a| + 20/(100 ln 10) delta_f / (|S| + 128e-5)        (d normalize / d|S|)
  normalised phase       decided bins (pi - |angle S| > 4 delta_f/|S|): |p_dev - p| <= 2^-24 |p| + delta_f / (2 pi |S|), NOT
                         wrapped; undecided bins: the same bound on the circle; |S| <= 4 delta_f: no phase, complex value only
  DC / Nyquist rows      imaginary part exactly +0 on both sides: the phase plane EQUALS the oracle's fp32 value (0.5 / 1.0
                         normalised, 0 / fp32(pi) raw); these two rows are held by that equality and are not counted as decided
                         or undecided (a negative real bin sits exactly on the cut)
  silent frames          every sample under the window's taps exactly zero: phase EQUALS 0.5 (0 raw)
  mirror frames          a frame that 'reflect' padding makes symmetric about its centre (frame 0 always, and the frame centred
                         on the last sample) has a real spectrum in exact arithmetic: every bin with a negative real part sits on
                         the cut and the sign of its imaginary part is a rounding residue on both sides, in librosa as well.  These
                         bins are undecided by the rule above, half of each such frame, and no choice of waveform avoids them; they
                         are compared on the circle with the same bound and are not counted against the cap of 0.1 % undecided
                         bins, which holds for all other bins (no case of the table has any)
  synthesis              |y_dev - y| <= 2^-24 |y| + EPS_SYNTHESIS A_t where the envelope exceeds tiny, y_dev == y elsewhere

Where the constants come from.  `twin_stft` is the kernel's direct DFT over the non-zero taps (sequential sum over n, twiddles
indexed (k n) mod n_fft, the tree-summed mean); `twin_istft` is the kernel's gather (per frame four partial sums over
k = kg, kg + 4, ..., accumulated over the frames in ascending order and added as ((r0 + r1) + r2) + r3, then divided by the
envelope).  `measure_gaps()` runs both over the whole case table (tests/features_cases.py, every pad mode / mean removal /
synthesis input kind) against the FFT oracle (oracle/features.py):

    analysis   max |S_twin - S_fft| / sum|xw|      = 1.88e-15   (MEASURED_GAP_ANALYSIS; at "n1024", 400 taps summed in sequence;
                                                                 2.5e-16 at "n4" ... 8.7e-16 at "oddwin" for the others)
    synthesis  max |y_twin - y_fft| / A_t          = 3.43e-15   (MEASURED_GAP_SYNTHESIS; at "hop_eq_win", 1.6e-15 at "gaps", beside
                                                                 the zeros of the envelope, where one ulp of a Hann tap of 0.0096
                                                                 shows; 1.4e-16 ... 5.6e-16 for the other seven)

EPS_ANALYSIS and EPS_SYNTHESIS are 64 times these: the margin covers the device's sincospi, sincos, atan2, log10 and pow
differing from libm by a few ulp, and FMA contraction.  tests/test_features.py re-measures the gaps and holds them to the
recorded figures with a x4 margin.  Nothing here was measured on, or adjusted to, a kernel's output.
"""
import math

import numpy as np

from oracle import features as FO

MEASURED_GAP_ANALYSIS = 1.88e-15
MEASURED_GAP_SYNTHESIS = 3.43e-15
EPS_ANALYSIS = 64.0 * MEASURED_GAP_ANALYSIS
EPS_SYNTHESIS = 64.0 * MEASURED_GAP_SYNTHESIS
U32 = 2.0 ** -24                                  # one rounding to fp32, relative
C_AMP = 20.0 / (100.0 * math.log(10.0))           # d normalize(amp) / d amp * (amp + 128 ep)
UNDECIDED_CAP = 1e-3
PI = math.pi


# ---------------------------------------------------------------------------------------------------------------- twins
def twin_mean(x):
    """The kernel's mean: 256 strided partial sums, each sequential, then a halving tree; fp64."""
    x = np.asarray(x, dtype=np.float64)
    rows = -(-len(x) // 256)
    xp = np.zeros(rows * 256, dtype=np.float64)
    xp[:len(x)] = x
    red = np.zeros(256, dtype=np.float64)
    for r in xp.reshape(rows, 256):
        red = red + r
    st = 128
    while st > 0:
        red[:st] = red[:st] + red[st:2 * st]
        st >>= 1
    return red[0] / float(len(x))


def sincospi(a):
    """(sin(pi a), cos(pi a)) for a in [0, 2] as the device's sincospi forms them: the argument is reduced exactly to
    [-1/4, 1/4] turns of pi before pi is multiplied in, so multiples of 1/2 give exact zeros and ones."""
    a = np.asarray(a, dtype=np.float64)
    q = np.rint(2.0 * a)
    r = a - 0.5 * q
    s, c = np.sin(PI * r), np.cos(PI * r)
    q = q.astype(np.int64) & 3
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def twin_hann(n_fft, win):
    """(taps [win] of the periodic Hann, n_lo): the window sits at n_lo = (n_fft - win) // 2 of the frame."""
    m = np.arange(win, dtype=np.float64)
    return 0.5 - 0.5 * sincospi(2.0 * m / float(win))[1], (n_fft - win) // 2


def _twiddles(n_fft):
    s, c = sincospi(2.0 * np.arange(n_fft, dtype=np.float64) / float(n_fft))
    return c, s


def twin_stft(x32, n_fft, win, hop, pad_mode, remove_mean):
    """stft_feature_kernel's arithmetic for one fp32 waveform [T] -> complex128 [n_bins, n_frames]."""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    T = len(x)
    mean = twin_mean(x) if remove_mean else 0.0
    nf, nb, mask = 1 + T // hop, n_fft // 2 + 1, n_fft - 1
    w, n_lo = twin_hann(n_fft, win)
    i = np.arange(nf)[:, None] * hop + np.arange(n_lo, n_lo + win)[None, :] - n_fft // 2
    inside = (i >= 0) & (i < T)
    j = np.where(i < 0, -i, np.where(i >= T, 2 * (T - 1) - i, i))
    v = x[j] - mean
    if pad_mode == "constant":
        v = np.where(inside, v, 0.0)
    xw = v * w[None, :]                                            # [n_frames, win]
    tc, ts = _twiddles(n_fft)
    k = np.arange(nb)
    re, im = np.zeros((nb, nf)), np.zeros((nb, nf))
    for m in range(win):
        idx = (k * (n_lo + m)) & mask
        re = re + xw[None, :, m] * tc[idx][:, None]
        im = im - xw[None, :, m] * ts[idx][:, None]
    return re + 1j * im


def twin_denormalize(a, p):
    amp = (np.power(10.0, (a * FO.MD - FO.MD) / 20.0) - FO.EP) * FO.AMP_REF
    ph = p * 2.0 * PI - PI
    v = ph + PI
    return amp, v - np.floor(v / (2.0 * PI)) * (2.0 * PI) - PI      # the kernel's floor form of python's %


def twin_istft(amp32, ph32, n_fft, win, hop, denormalize):
    """istft_feature_kernel's arithmetic for one pair of fp32 planes [n_bins, n_frames] -> fp64 [hop (n_frames - 1)]."""
    amp, ph = np.asarray(amp32, dtype=np.float64), np.asarray(ph32, dtype=np.float64)
    nb, nf = amp.shape
    mask = n_fft - 1
    if denormalize:
        amp, ph = twin_denormalize(amp, ph)
    xr, xi = amp * np.cos(ph), amp * np.sin(ph)
    w, n_lo = twin_hann(n_fft, win)
    n = np.arange(n_lo, n_lo + win)
    tc, ts = _twiddles(n_fft)
    part = np.zeros((4, win, nf))
    for k in range(nb):
        idx = (k * n) & mask
        if k == 0 or k == nb - 1:
            part[k % 4] = part[k % 4] + xr[k][None, :] * tc[idx][:, None]
        else:
            part[k % 4] = part[k % 4] + 2.0 * (xr[k][None, :] * tc[idx][:, None] - xi[k][None, :] * ts[idx][:, None])
    total = n_fft + hop * (nf - 1)
    acc, wss = np.zeros((4, total)), np.zeros(total)
    for f in range(nf):
        lo = f * hop + n_lo
        acc[:, lo:lo + win] = acc[:, lo:lo + win] + w[None, :] * part[:, :, f] / float(n_fft)
        wss[lo:lo + win] = wss[lo:lo + win] + w * w
    y = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    nz = wss > FO.TINY32
    y[nz] = y[nz] / wss[nz]
    return y[n_fft // 2:n_fft // 2 + hop * (nf - 1)]


# --------------------------------------------------------------------------------------------- the pieces of the bounds
def envelope(n_frames, n_fft, win, hop):
    """The overlap-added squared window on the output samples, fp64 [hop (n_frames - 1)], as the oracle forms it."""
    w = FO.hann_padded(n_fft, win)
    wss = np.zeros(n_fft + hop * (n_frames - 1))
    for f in range(n_frames):
        wss[f * hop:f * hop + n_fft] += w * w
    return wss[n_fft // 2:n_fft // 2 + hop * (n_frames - 1)]


def abs_synthesis(mag, n_fft, win, hop):
    """A_t for magnitudes mag >= 0 [n_bins, n_frames]: sum_f w_f(t) (1/n_fft) sum_k c_k mag[k, f], over the envelope where the
    envelope exceeds tiny.  Every term of the kernel's sum for sample t is bounded by its term here."""
    mag = np.abs(np.asarray(mag, dtype=np.float64))
    nb, nf = mag.shape
    c = np.full(nb, 2.0)
    c[0] = c[-1] = 1.0
    s = (c[:, None] * mag).sum(axis=0) / float(n_fft)
    w = FO.hann_padded(n_fft, win)
    a = np.zeros(n_fft + hop * (nf - 1))
    for f in range(nf):
        a[f * hop:f * hop + n_fft] += w * s[f]
    a = a[n_fft // 2:n_fft // 2 + hop * (nf - 1)]
    env = envelope(nf, n_fft, win, hop)
    nz = env > FO.TINY32
    a[nz] /= env[nz]
    return a


def frame_stats(x32, n_fft, win, hop, pad_mode, remove_mean):
    """Per frame [n_frames]: sum_n |xw_f[n]|; silent - every sample under the window's taps, the zero tap included, is exactly
    0; mirror - the frame's samples are symmetric about its centre, and so is the window (it is unless n_fft - win is odd)."""
    y = np.asarray(x32, dtype=np.float32).astype(np.float64)
    if remove_mean:
        y = y - y.mean()
    yp = np.pad(y, n_fft // 2, mode=pad_mode)
    w = FO.hann_padded(n_fft, win)
    nf, n_lo = 1 + len(y) // hop, (n_fft - win) // 2
    fr = np.stack([yp[f * hop:f * hop + n_fft] for f in range(nf)])
    xw = fr * w[None, :]
    silent = ~fr[:, n_lo:n_lo + win].any(axis=1)
    assert float(np.abs(w[1:] - w[:0:-1]).max()) <= 1e-15 or (n_fft - win) % 2          # an odd margin shifts the window off centre
    mirror = (fr[:, 1:] == fr[:, :0:-1]).all(axis=1) & ~silent & ((n_fft - win) % 2 == 0)
    return np.abs(xw).sum(axis=1), silent, mirror


def classify(S, l1, mirror=None):
    """(delta [B, 1, F], decided, undecided, mirrored, nophase): masks [B, K, F] of the phase rules.  DC and Nyquist rows are in
    none; mirrored holds the undecided bins of the mirror frames [B, F], which undecided then leaves out."""
    delta = EPS_ANALYSIS * np.asarray(l1)[:, None, :]
    mag = np.abs(S)
    inner = np.zeros(S.shape, dtype=bool)
    inner[:, 1:-1, :] = True
    nophase = mag <= 4.0 * delta
    with np.errstate(divide="ignore", invalid="ignore"):
        dec = (PI - np.abs(np.angle(S))) > 4.0 * delta / mag
    und = inner & ~nophase & ~dec
    mir = und & (np.broadcast_to(np.asarray(mirror)[:, None, :], S.shape) if mirror is not None else False)
    return delta, inner & ~nophase & dec, und & ~mir, mir, inner & nophase


def plane_error_as_complex(S, l1):
    """The normalised-plane bounds carried back to the complex value: what one fp32 rounding of each plane plus delta_f can move
    S by (delta_f once through each plane).  a -> a (1 +- 2^-24) multiplies amp/128 + ep by 10^(+-5 2^-24 |a|); p by 2^-24 |p| turns is 2 pi 2^-24 |p| radians."""
    delta = EPS_ANALYSIS * np.asarray(l1)[:, None, :]
    mag = np.abs(S)
    a, p = FO.normalize(mag, np.angle(S))
    return 2.0 * delta + (mag + FO.AMP_REF * FO.EP) * (np.power(10.0, 5.0 * U32 * np.abs(a)) - 1.0) + mag * 2.0 * PI * U32 * np.abs(p)


def _worst(label, what, err, bound, mask=None):
    """print the element with the largest err - bound (among mask), return whether all of them hold"""
    if mask is not None and not mask.any():
        print(f"{label} {what}: no such element")
        return True
    ex = np.where(mask, err - bound, -np.inf) if mask is not None else err - bound
    at = np.unravel_index(int(np.argmax(ex)), ex.shape)
    n = int(mask.sum()) if mask is not None else ex.size
    print(f"{label} {what}: {n} elements, worst at {tuple(int(i) for i in at)}: err {float(err[at]):.3e} bound {float(bound[at]):.3e}")
    return bool((ex <= 0).all())


def circ(a, b):
    d = np.abs(a - b) % 1.0
    return np.minimum(d, 1.0 - d)


# ------------------------------------------------------------------------------------------------------------ the checks
def check_planes(label, amp, ph, S, l1, normalize, silent=None, mirror=None):
    """amp, ph: the kernel's fp32 planes [B, n_bins, n_frames]; S: the oracle's complex128 values; l1: sum|xw| [B, n_frames];
    silent, mirror: bool [B, n_frames] or None.  Prints the worst element of every rule, then asserts all of them."""
    assert amp.dtype == np.float32 and ph.dtype == np.float32 and amp.shape == ph.shape == S.shape
    assert np.isfinite(amp).all() and np.isfinite(ph).all(), label
    a64, p64 = amp.astype(np.float64), ph.astype(np.float64)
    mag, ang = np.abs(S), np.angle(S)
    delta, dec, und, mir, nop = classify(S, l1, mirror)
    ok = []
    edge = np.zeros(S.shape, dtype=bool)
    edge[:, 0, :] = edge[:, -1, :] = True
    assert not S.imag[edge].any() and not np.signbit(S.imag[edge]).any(), label        # the oracle's DC / Nyquist rows: exactly +0
    pinned = edge & (mag > 4.0 * delta)
    if silent is not None:
        pinned = pinned | np.broadcast_to(silent[:, None, :], S.shape)
    if normalize:
        a_ref, p_ref = FO.normalize(mag, ang)
        ok.append(_worst(label, "amplitude plane", np.abs(a64 - a_ref), U32 * np.abs(a_ref) + C_AMP * delta / (mag + FO.AMP_REF * FO.EP)))
        with np.errstate(divide="ignore", invalid="ignore"):
            pb = U32 * np.abs(p_ref) + delta / (2.0 * PI * mag)
        ok.append(_worst(label, "phase plane, decided bins, not wrapped", np.abs(p64 - p_ref), pb, dec))
        ok.append(_worst(label, "phase plane, undecided bins, circular", circ(p64, p_ref), pb, und))
        ok.append(_worst(label, "phase plane, cut bins of mirror frames, circular", circ(p64, p_ref), pb, mir))
        assert und.sum() <= UNDECIDED_CAP * und.size, (label, int(und.sum()))
        ad, pd = FO.denormalize(a64, p64)
        # one rounding of each plane carried back through denormalize, plus 8 ulp of fp64 for this line's own denormalize
        cb = delta + (mag + FO.AMP_REF * FO.EP) * (np.power(10.0, 5.0 * U32 * np.abs(a_ref)) - 1.0 + 2.0 ** -49) + mag * 2.0 * PI * U32
        ok.append(_worst(label, "complex value of bins without phase", np.abs(ad * np.exp(1j * pd) - S), cb, nop))
        want = p_ref.astype(np.float32)
    else:
        ok.append(_worst(label, "complex value", np.abs(a64 * np.exp(1j * p64) - S), U32 * (1.0 + PI) * mag + delta))
        want = ang.astype(np.float32)
    bad = pinned & (ph != want)
    print(f"{label} pinned phases (DC / Nyquist rows, silent frames): {int(pinned.sum())} elements, {int(bad.sum())} differ"
          + (f", first at {tuple(int(i) for i in np.argwhere(bad)[0])}: {ph[bad][0]!r} for {want[bad][0]!r}" if bad.any() else ""))
    ok.append(not bad.any())
    assert all(ok), label


def check_wave(label, wav, y, A, env, eps_extra=None):
    """wav: the kernel's fp32 waveforms [B, T_out]; y: the oracle's fp64; A: A_t [B, T_out]; env: the envelope [T_out];
    eps_extra: an additional per-sample allowance [B, T_out] (the round trip's analysis share) or None."""
    assert wav.dtype == np.float32 and wav.shape == y.shape == A.shape and np.isfinite(wav).all(), label
    live = np.broadcast_to((env > FO.TINY32)[None, :], y.shape)
    bound = U32 * np.abs(y) + EPS_SYNTHESIS * A + (0.0 if eps_extra is None else eps_extra)
    ok = _worst(label, "samples with an envelope", np.abs(wav.astype(np.float64) - y), bound, live)
    bad = ~live & (wav != y.astype(np.float32))
    print(f"{label} samples without an envelope: {int((~live).sum())} elements, {int(bad.sum())} differ from the oracle")
    assert ok and not bad.any(), label


# ------------------------------------------------------------------------------------------------------ the measurement
def measure_gaps(names=None):
    """(analysis gap, synthesis gap) of the twins against the FFT oracle over the case table, in the bounds' units."""
    import features_cases as FC
    ga = gs = 0.0
    for name in (names or FC.GEOMETRIES):
        B, T, n_fft, win, hop = FC.GEOMETRIES[name]
        for kind in FC.WAVE_KINDS:
            for pad_mode in FC.PAD_MODES:
                for remove_mean in ((False,) if kind == "zeros" else (True, False)):
                    S, l1 = FC.analysis(name, kind, pad_mode, remove_mean)[:2]
                    x = FC.waves(name, kind)
                    for b in range(x.shape[0]):
                        d = np.abs(twin_stft(x[b], n_fft, win, hop, pad_mode, remove_mean) - S[b])
                        live = l1[b] > 0
                        assert not d[:, ~live].any()
                        if live.any():
                            ga = max(ga, float((d[:, live] / l1[b][None, live]).max()))
        nb, nf = FC.dims(name)
        for kind in FC.PLANE_KINDS:
            feat = FC.planes(name, kind, True, False)
            y, A, env = FC.synthesis(name, kind)
            for b in range(feat.shape[0]):
                d = np.abs(twin_istft(feat[b, 0], feat[b, 1], n_fft, win, hop, kind != "raw") - y[b])
                live = (env > FO.TINY32) & (A[b] > 0)
                assert not d[env <= FO.TINY32].any()
                gs = max(gs, float((d[live] / A[b][live]).max()))
    return ga, gs

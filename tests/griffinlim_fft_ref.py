"""What the FFT form of Griffin-Lim (csrc/griffinlim_fft.hip) is held to, shared by the CPU and GPU tests.

`griffinlim32` is a complex64 restatement of the loop of tests/griffinlim_ref.py as the kernels form it: S rounded to fp32 once,
angles0 the fp32 rounding of cos / sin taken in fp64, the window in fp32, every transform an fp32 FFT (`rfft32` / `irfft32` below: radix 2 on half the
length plus the real split, not the kernels' factorisation; written out in single fp32 NumPy operations on separate real and imaginary
parts, so that the restatement gives the same bits on every machine, which a library FFT does not), the overlap-add of a sample in ascending frame order in fp32, the envelope rule `wss > tiny32`, the
angle update a / (|a| + 1e-16) in fp32 with alpha rounded to fp32.  The yardstick is the fp64 waveform of griffinlim_ref on the same
fp32 inputs, and with e(y) = max_t |y - y64| / max_t |y64| per row the kernels are held to

    e(kernel) <= C e(restatement on the same data) + 2^-22

No bound per element can be derived - the iteration amplifies rounding, fastest with momentum - so C is measured, and not on a kernel:
it is twice the largest factor by which two equally good fp32 realisations of the loop differ in e.  The realisations compared with the
restatement (VARIANTS) are the restatement with the overlap-add in descending frame order, and the restatement run on 3 S and on 0.7 S with
the waveform scaled back (other roundings of every product, the same loop).  tests/test_griffinlim_fft_ref.py measures all of them over
the whole case table of tests/griffinlim_fft_cases.py and asserts that C covers twice the spread; the figures are in its docstring.

`variant=` also takes one-line MUTATIONS - the mistakes a kernel of this kind makes:
    "nyquist"  bin N/2 dropped from the inverse transform                               (raw magnitudes: bin N/2 is not silent)
    "nofold"   the reflected edge not folded: the analysis sees zeros there            (pad_mode "reflect", n_iter >= 1)
    "shift"    the window a tap late
    "notprev"  tprev not subtracted                                                     (n_iter >= 2, momentum 0.99)
    "noenv"    the envelope division left out over the first and the last hop of a row
    "nohalo"   frame 1 left out of the overlap-add of the second half of its taps - a halo frame a workgroup forgot
                                                                                        (geometries whose frames overlap: hop < win)

The per-sample check alone is loose where it matters most.  After 32 iterations with momentum a few rows are chaotic: the restatement's
own e reaches 3.4e-3 of the peak (rir, raw magnitudes, row 0), C e is then 5 % of the peak, and a mistake passes it by a factor of 4 only.
In such a row two correct waveforms differ sample by sample, but they are equally good reconstructions, and that does not amplify: the
spectral convergence sc(y) = || |stft(y)| - S || / || S ||, in fp64 on the host, of the restatement and of its three variants stays
within 2.64e-5 (relative) of the fp64 yardstick's in every row of every case.  So a row is also held to

    |sc(kernel) - sc(y64)| <= SC_TOL sc(y64),     SC_TOL = 5.3e-5 = twice that largest spread

(the issue's 1 % at two geometries is asserted as well; this is the same quantity at every row, at the tolerance the fp32 realisations
themselves keep).  Each mutation must fail one of the two checks by a factor of ten at the least in every row of every case it applies
to, or the checks would say nothing; tests/test_griffinlim_fft_ref.py asserts it."""
import numpy as np

from oracle import features as FO

C = 16.5
SC_TOL = 5.3e-5
VARIANTS = ("descending", "scale3", "scale0.7")
MUTATIONS = ("nyquist", "nofold", "shift", "notprev", "noenv", "nohalo")
TINY32 = np.float32(np.finfo(np.float32).tiny)
F32 = np.float32


def applies(mutation, n_iter, momentum, pad_mode, denormalize, overlap=True):
    if mutation == "nohalo":
        return overlap                          # without overlap there is no halo: every frame's taps are a workgroup's own
    if mutation == "nyquist":
        return not denormalize                  # the cases' denormalised features have the last five magnitude rows zeroed
    if mutation == "nofold":
        return pad_mode == "reflect" and n_iter >= 1
    if mutation == "notprev":
        return n_iter >= 2 and momentum > 0
    return True


def _twiddle(n, sign, count):
    """exp(sign 2 pi i k / n), k < count, fp32 of fp64 -> (re, im) as columns"""
    a = 2.0 * np.pi * np.arange(count, dtype=np.float64) / n
    return np.cos(a).astype(F32)[:, None], (sign * np.sin(a)).astype(F32)[:, None]


def _fft32(xr, xi, sign):
    """the unnormalised complex DFT along axis 0 (a power of two) of fp32 [M, C] pairs: Stockham radix 2, every operation one fp32
    rounding"""
    M, cols = xr.shape
    ns = 1
    while ns < M:
        ar, ai, br, bi = (v.reshape(M // (2 * ns), ns, cols) for v in (xr[:M // 2], xi[:M // 2], xr[M // 2:], xi[M // 2:]))
        if ns > 1:
            wr, wi = _twiddle(2 * ns, sign, ns)
            br, bi = wr * br - wi * bi, wr * bi + wi * br
        outr = np.empty((M // (2 * ns), 2, ns, cols), dtype=F32)
        outi = np.empty_like(outr)
        outr[:, 0], outr[:, 1], outi[:, 0], outi[:, 1] = ar + br, ar - br, ai + bi, ai - bi
        xr, xi = outr.reshape(M, cols), outi.reshape(M, cols)
        ns *= 2
    return xr, xi


def rfft32(a):
    """fp32 [N, C] -> (re, im) fp32 [N / 2 + 1, C]: z[n] = a[2n] + i a[2n+1], Z = FFT(z), A[k] = E + W^k O"""
    N = a.shape[0]
    M = N // 2
    zr, zi = _fft32(np.ascontiguousarray(a[0::2]), np.ascontiguousarray(a[1::2]), -1.0)
    zr, zi = np.concatenate((zr, zr[:1])), np.concatenate((zi, zi[:1]))            # Z[M] = Z[0]
    cr, ci = zr[::-1], -zi[::-1]                                                    # conj Z[M - k]
    half = F32(0.5)
    er, ei = half * (zr + cr), half * (zi + ci)
    o_r, o_i = half * (zi - ci), -(half * (zr - cr))                                # -i (Z[k] - conj Z[M - k]) / 2
    wr, wi = _twiddle(N, -1.0, M + 1)
    return er + (wr * o_r - wi * o_i), ei + (wr * o_i + wi * o_r)


def irfft32(ar, ai):
    """(re, im) fp32 [N / 2 + 1, C] -> fp32 [N, C], numpy.fft.irfft: the imaginary parts of bins 0 and N / 2 are ignored"""
    M = ar.shape[0] - 1
    ai = ai.copy()
    ai[0] = 0
    ai[M] = 0
    cr, ci = ar[::-1], -ai[::-1]                                                    # conj A[M - k]
    half = F32(0.5)
    er, ei = half * (ar + cr), half * (ai + ci)
    dr, di = half * (ar - cr), half * (ai - ci)
    wr, wi = _twiddle(2 * M, 1.0, M + 1)
    o_r, o_i = wr * dr - wi * di, wr * di + wi * dr
    zr, zi = _fft32((er - o_i)[:M], (ei + o_r)[:M], 1.0)                            # Z = E + i O
    out = np.empty((2 * M, ar.shape[1]), dtype=F32)
    out[0::2], out[1::2] = zr * F32(1.0 / M), zi * F32(1.0 / M)
    return out


def _istft32(sr, si, w, n_fft, hop, variant):
    """spectra fp32 [n_bins, B, n_frames] -> fp32 [B, hop (n_frames - 1)]"""
    nb, B, n_frames = sr.shape
    if variant == "nyquist":
        sr, si = sr.copy(), si.copy()
        sr[n_fft // 2] = 0
        si[n_fft // 2] = 0
    frames = irfft32(sr.reshape(nb, -1), si.reshape(nb, -1)).reshape(n_fft, B, n_frames)
    ws = np.roll(w, 1) if variant == "shift" else w
    terms = ws[:, None, None] * frames
    if variant == "nohalo":
        terms[n_fft // 2:, :, 1] = 0
    total = n_fft + hop * (n_frames - 1)
    y = np.zeros((B, total), dtype=F32)
    wss = np.zeros(total, dtype=F32)
    w2 = w * w
    for f in (range(n_frames - 1, -1, -1) if variant == "descending" else range(n_frames)):
        y[:, f * hop:f * hop + n_fft] += terms[:, :, f].T
        wss[f * hop:f * hop + n_fft] += w2
    nz = wss > TINY32
    if variant == "noenv":
        nz[n_fft // 2:n_fft // 2 + hop] = False
        nz[total - n_fft // 2 - hop:total - n_fft // 2] = False
    y[:, nz] /= wss[nz]
    return y[:, n_fft // 2:total - n_fft // 2]


def _stft32(y, w, n_fft, hop, pad_mode, variant):
    """fp32 [B, T] -> spectra fp32 [n_bins, B, 1 + T // hop]"""
    B = y.shape[0]
    yp = np.pad(y, ((0, 0), (n_fft // 2, n_fft // 2)), mode="constant" if variant == "nofold" else pad_mode)
    ws = np.roll(w, 1) if variant == "shift" else w
    frames = np.lib.stride_tricks.sliding_window_view(yp, n_fft, axis=1)[:, ::hop, :]           # [B, n_frames, n_fft]
    n_frames = frames.shape[1]
    frames = np.ascontiguousarray((frames * ws).transpose(2, 0, 1)).reshape(n_fft, B * n_frames)
    rr, ri = rfft32(frames)
    return rr.reshape(-1, B, n_frames), ri.reshape(-1, B, n_frames)


def griffinlim32(S, init_phase, n_fft=256, win_length=128, hop_length=64, n_iter=32, momentum=0.99, pad_mode="reflect", variant=None):
    """S fp64 [B, n_bins, n_frames] (rounded to fp32 here, once), init_phase fp32 like it, in turns -> fp32 [B, hop_length (n_frames - 1)]"""
    scale = {"scale3": 3.0, "scale0.7": 0.7}.get(variant, 1.0)
    S32 = (np.asarray(S, dtype=np.float64).astype(F32) * F32(scale)).transpose(1, 0, 2)
    u = np.asarray(init_phase, dtype=np.float64).transpose(1, 0, 2)
    ang_r, ang_i = np.cos(2.0 * np.pi * u).astype(F32), np.sin(2.0 * np.pi * u).astype(F32)
    w = FO.hann_padded(n_fft, win_length).astype(F32)
    alpha = F32(0.0 if variant == "notprev" else momentum / (1.0 + momentum))
    reb_r = reb_i = None
    for _ in range(n_iter):
        prev_r, prev_i = reb_r, reb_i
        inverse = _istft32(S32 * ang_r, S32 * ang_i, w, n_fft, hop_length, variant)
        reb_r, reb_i = _stft32(inverse, w, n_fft, hop_length, pad_mode, variant)
        a_r, a_i = (reb_r, reb_i) if prev_r is None else (reb_r - alpha * prev_r, reb_i - alpha * prev_i)
        d = np.sqrt(a_r * a_r + a_i * a_i) + F32(1e-16)
        ang_r, ang_i = a_r / d, a_i / d
        assert ang_r.dtype == F32 and ang_i.dtype == F32
    y = _istft32(S32 * ang_r, S32 * ang_i, w, n_fft, hop_length, variant)
    assert y.dtype == F32
    return y if scale == 1.0 else y / F32(scale)

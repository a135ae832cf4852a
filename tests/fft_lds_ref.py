"""References and criteria for the in-LDS FFT of csrc/fft_lds.h (tests/test_fft_lds.py on the host walk, tests/test_fft_lds_gpu.py on
the device).  Importable without the product.

An image is M float2 in natural order, here a complex array [n_img, M].  The four modes of the probe (tests/probe/fft_walk.h):

    0  complex forward                     FFT_M(z)
    1  complex inverse, unnormalised       M ifft(z)
    2  real forward of the 2M samples a[2n] = Re z[n], a[2n+1] = Im z[n]      -> packed spectrum, slot 0 = (A[0], A[M]), slot k = A[k]
    3  real inverse of a packed spectrum   -> z[n] = a[2n] + i a[2n+1] of the signal times 2M

Truth: numpy.fft in fp64 / complex128 on the fp32 inputs; for impulses the closed form exp(-+2 pi i (kn mod M) / M) evaluated in fp64
from the reduced integer.  Restatement: torch's CPU FFTs in complex64 (pocketfft's factorisation, not the header's): a second fp32 FFT
on the same data.

Error measure e(v): the relative L2 error of one image against the truth; in a packed real spectrum the interior bins count twice (they
stand for k and 2M - k), as in Parseval.  u = 2^-24 and `levels(M, mode)` = log2 of the transform's length: M for modes 0 and 1, 2M for
modes 2 and 3.

    C1  random data, every image:  e(got) <= 2 e(restatement of the same image)  and  e(got) <= 6.66 u levels
        (the ceiling is Higham's Theorem 24.2 per radix-2 level as the header of csrc/auralize_fft.hip derives it; the factor 2 is a
        margin over another fp32 FFT with correctly rounded twiddles, not a fit)
    C2  impulses at every position, every output element within 4.83 u levels of the closed form (modes 0 - 2: the modulus of the
        complex difference; mode 3: every real sample, twice the allowance as each sample is the sum of two paths): the componentwise
        per-level factor (1 + u)(1 + 2 sqrt2 u)(1 + u) of the same header, one path per element
    C3  round trip mode 3(mode 2(a)) / 2M against a:  e <= 2 e(irfft(rfft(a)) in complex64), ceiling 2 x 6.66 u log2(2M)

A twiddle index one step of the 4096-step table off is an error of 1.5e-3 = 2.5e4 u in one element; MUTATIONS holds that and three more
deliberate errors, applied to the restatement's output: each must fail C1 or C2 for every M."""
import functools
import math

import numpy as np
import torch

SIZES = (64, 128, 256, 512, 1024, 2048)
MODES = (0, 1, 2, 3)
U = 2.0 ** -24
L2_LEVEL, EL_LEVEL, MARGIN = 6.66, 4.83, 2.0
MUTATIONS = ("rotate_bin", "swap_bins", "swap_dc_nyquist", "unsplit_pair")
MUTATION_MODES = {"rotate_bin": MODES, "swap_bins": MODES, "swap_dc_nyquist": (2,), "unsplit_pair": (2,)}


def levels(M, mode):
    return int(math.log2(M)) + (1 if mode >= 2 else 0)


def n_images(M):
    """2 (2048 / M) + 1: two full workgroups of the many-images form and a ragged third"""
    return 2 * (2048 // M) + 1


def _ro(a):
    a.setflags(write=False)
    return a


# ---- layouts ----

def samples(z):
    """complex [n, M] -> real [n, 2M]: a[2n] = Re z[n], a[2n+1] = Im z[n]"""
    return np.stack([z.real, z.imag], axis=-1).reshape(z.shape[0], -1)


def from_samples(a):
    return a[:, 0::2] + 1j * a[:, 1::2]


def pack(A):
    """half spectrum [n, M+1] -> packed [n, M]: slot 0 = (Re A[0], Re A[M])"""
    out = np.array(A[:, :-1])
    out[:, 0] = A[:, 0].real + 1j * A[:, -1].real
    return out


def unpack(p):
    """packed [n, M] -> half spectrum [n, M+1] with real A[0] and A[M]"""
    A = np.concatenate([p, np.zeros_like(p[:, :1])], axis=1)
    A[:, 0] = p[:, 0].real
    A[:, -1] = p[:, 0].imag
    return A


# ---- truth and restatement ----

def truth(mode, x):
    """fp64 / complex128 on the fp32 input x (complex64 [n, M]) -> complex128 [n, M]"""
    x = np.asarray(x).astype(np.complex128)
    M = x.shape[1]
    if mode == 0:
        return np.fft.fft(x, axis=1)
    if mode == 1:
        return np.fft.ifft(x, axis=1) * M
    if mode == 2:
        return pack(np.fft.rfft(samples(x), axis=1))
    return from_samples(np.fft.irfft(unpack(x), n=2 * M, axis=1) * (2 * M))


def restate(mode, x):
    """the same in torch's complex64 on the CPU -> complex64 [n, M]"""
    x = np.ascontiguousarray(np.asarray(x).astype(np.complex64))
    M = x.shape[1]
    t = torch.from_numpy(x)
    if mode == 0:
        r = torch.fft.fft(t, dim=1)
    elif mode == 1:
        r = torch.fft.ifft(t, dim=1, norm="forward")
    elif mode == 2:
        A = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(samples(x).astype(np.float32))), dim=1)
        assert A.dtype == torch.complex64
        return pack(A.numpy()).astype(np.complex64)
    else:
        a = torch.fft.irfft(torch.from_numpy(unpack(x)), n=2 * M, dim=1, norm="forward")
        assert a.dtype == torch.float32
        return from_samples(a.numpy()).astype(np.complex64)
    assert r.dtype == torch.complex64
    return r.numpy()


def restate_roundtrip(z):
    """irfft(rfft(a)) in complex64 / fp32, normalised -> complex64 [n, M]"""
    a = torch.from_numpy(np.ascontiguousarray(samples(np.asarray(z)).astype(np.float32)))
    b = torch.fft.irfft(torch.fft.rfft(a, dim=1), n=a.shape[1], dim=1)
    assert b.dtype == torch.float32
    return from_samples(b.numpy()).astype(np.complex64)


# ---- inputs ----

@functools.lru_cache(maxsize=None)
def random_images(M):
    """complex64 [n_images(M), M], uniform in (-1, 1) per component, read-only"""
    v = np.random.default_rng(5000 + M).uniform(-1.0, 1.0, size=(n_images(M), M, 2)).astype(np.float32)
    return _ro(np.ascontiguousarray(v).view(np.complex64)[..., 0])


@functools.lru_cache(maxsize=None)
def random_input(M, mode):
    """the input of a mode on the random set: the images themselves, for mode 3 their fp64-true packed spectrum rounded to fp32"""
    z = random_images(M)
    return z if mode < 3 else _ro(truth(2, z).astype(np.complex64))


@functools.lru_cache(maxsize=None)
def random_reference(M, mode):
    """(truth, restatement) of random_input(M, mode), computed once, read-only"""
    x = random_input(M, mode)
    return _ro(truth(mode, x)), _ro(restate(mode, x))


def impulse_input(M, mode):
    """mode 0: a real unit at each n; mode 1: an imaginary unit at each n; mode 2: a unit at each of the 2M samples (image s: sample s);
    mode 3: (1, 0) in slot k (image 2k) and (0, 1) in slot k (image 2k + 1).  complex64 [M or 2M, M]"""
    eye = np.eye(M, dtype=np.complex64)
    if mode == 0:
        return eye
    if mode == 1:
        return eye * np.complex64(1j)
    out = np.zeros((2 * M, M), dtype=np.complex64)
    out[0::2] = eye
    out[1::2] = eye * np.complex64(1j)
    return out


def impulse_closed_form(M, mode, lo=0, hi=None):
    """images lo ... hi of the exact response to impulse_input(M, mode): complex128, every angle from the reduced integer"""
    n_all = M if mode < 2 else 2 * M
    hi = n_all if hi is None else hi
    idx = np.arange(lo, hi, dtype=np.int64)[:, None]
    if mode < 2:
        k = np.arange(M, dtype=np.int64)[None, :]
        w = np.exp((-2j if mode == 0 else 2j) * np.pi * ((k * idx) % M) / M)
        return w if mode == 0 else 1j * w
    if mode == 2:
        k = np.arange(M + 1, dtype=np.int64)[None, :]
        A = np.exp(-2j * np.pi * ((k * idx) % (2 * M)) / (2 * M))
        A[:, 0] = 1.0
        A[:, M] = np.where(idx[:, 0] % 2 == 0, 1.0, -1.0)
        return pack(A)
    k, imag = idx // 2, idx % 2                          # slot and which component holds the unit
    n = np.arange(2 * M, dtype=np.int64)[None, :]
    ang = np.pi * ((k * n) % (2 * M)) / M
    a = np.where(imag == 0, 2.0 * np.cos(ang), -2.0 * np.sin(ang))
    sign = np.where(n % 2 == 0, 1.0, -1.0)
    a = np.where(k == 0, np.where(imag == 0, 1.0, sign), a)
    return from_samples(a)


# ---- the error measure and the criteria ----

def rel_l2(v, ref, packed=False):
    """e(v) per image: |v - ref|_2 / |ref|_2 in fp64; packed: interior bins twice, slot 0 as the two real bins it holds"""
    d = np.asarray(v).astype(np.complex128) - ref
    w = np.ones(ref.shape[1])
    if packed:
        w[1:] = 2.0
    num = (w * (d.real ** 2 + d.imag ** 2)).sum(axis=1)
    den = (w * (ref.real ** 2 + ref.imag ** 2)).sum(axis=1)
    return np.sqrt(num / den)


def check_c1(M, mode, got, x=None, quiet=False):
    """C1 for `got` = the transform of x (default: the random set).  Returns (worst e(got) / e(restatement), worst e(got) / ceiling)."""
    if x is None:
        ref, rs = random_reference(M, mode)
    else:
        ref, rs = truth(mode, x), restate(mode, x)
    got = np.asarray(got)
    assert got.shape == ref.shape and np.all(np.isfinite(got.view(np.float32))), (M, mode, "shape or non-finite")
    e, er = rel_l2(got, ref, packed=mode == 2), rel_l2(rs, ref, packed=mode == 2)
    ceil = L2_LEVEL * U * levels(M, mode)
    assert np.all(er > 0) and np.all(er <= ceil), (M, mode, "the restatement itself", er.max(), ceil)
    ratio, top = float(np.max(e / er)), float(np.max(e / ceil))
    if not quiet:
        print(f"C1 M={M} mode={mode}: e = {e.min():.3g} ... {e.max():.3g}, worst e / e(restatement) = {ratio:.3g}, worst e / ceiling = {top:.3g}")
    bad = np.flatnonzero((e > MARGIN * er) | (e > ceil))
    assert bad.size == 0, (f"C1 M={M} mode={mode}", bad[:8], e[bad[:8]], er[bad[:8]], ceil)
    return ratio, top


def check_c2(M, mode, got, quiet=False, chunk=256):
    """C2 for `got` = the transform of impulse_input(M, mode).  Returns the largest element error in u."""
    got = np.asarray(got)
    n_all = M if mode < 2 else 2 * M
    assert got.shape == (n_all, M) and np.all(np.isfinite(got.view(np.float32))), (M, mode, "shape or non-finite")
    tol = EL_LEVEL * U * levels(M, mode) * (2.0 if mode == 3 else 1.0)
    worst = 0.0
    for lo in range(0, n_all, chunk):
        hi = min(lo + chunk, n_all)
        d = got[lo:hi].astype(np.complex128) - impulse_closed_form(M, mode, lo, hi)
        err = np.maximum(np.abs(d.real), np.abs(d.imag)) if mode == 3 else np.abs(d)
        worst = max(worst, float(err.max()))
        bad = np.argwhere(err > tol)
        assert bad.size == 0, (f"C2 M={M} mode={mode}: (image - {lo}, element)", bad[:8], err[err > tol][:8] / U, tol / U)
    if not quiet:
        print(f"C2 M={M} mode={mode}: largest element error = {worst / U:.3g} u, allowance {tol / U:.3g} u")
    return worst / U


def check_c3(M, got, quiet=False):
    """C3 for `got` = mode 3(mode 2(random set)), unscaled.  Returns the worst e(got) / e(restatement)."""
    z = random_images(M)
    ref = z.astype(np.complex128)
    back = np.asarray(got).astype(np.complex128) / (2 * M)        # the exact 1 / 2M
    assert back.shape == ref.shape and np.all(np.isfinite(back.view(np.float64)))
    e, er = rel_l2(back, ref), rel_l2(restate_roundtrip(z), ref)
    ceil = 2.0 * L2_LEVEL * U * levels(M, 2)
    assert np.all(er > 0) and np.all(er <= ceil), (M, "the restatement itself", er.max(), ceil)
    ratio = float(np.max(e / er))
    if not quiet:
        print(f"C3 M={M}: e = {e.min():.3g} ... {e.max():.3g}, worst e / e(restatement) = {ratio:.3g}, worst e / ceiling = {np.max(e / ceil):.3g}")
    bad = np.flatnonzero((e > MARGIN * er) | (e > ceil))
    assert bad.size == 0, (f"C3 M={M}", bad[:8], e[bad[:8]], er[bad[:8]], ceil)
    return ratio


# ---- mutations ----

def mutate(name, M, mode, out, x, img=1):
    """A deliberately wrong copy of `out` = the restatement's output for input x (both complex64 [n, M]), wrong in image `img` alone:
    rotate_bin       element M/2 + 3 multiplied by exp(2 pi i / 4096): one twiddle index one table step off
    swap_bins        elements 5 and 6 exchanged
    swap_dc_nyquist  (mode 2) the two halves of slot 0 exchanged
    unsplit_pair     (mode 2) slots 3 and M - 3 left as the complex transform Z of z, without the split"""
    assert name in MUTATIONS and mode in MUTATION_MODES[name]
    out = np.array(out)
    if name == "rotate_bin":
        out[img, M // 2 + 3] *= np.complex64(np.exp(2j * np.pi / 4096))
    elif name == "swap_bins":
        out[img, [5, 6]] = out[img, [6, 5]]
    elif name == "swap_dc_nyquist":
        out[img, 0] = out[img, 0].imag + 1j * out[img, 0].real
    else:
        Z = restate(0, np.asarray(x)[img:img + 1])[0]
        out[img, 3], out[img, M - 3] = Z[3], Z[M - 3]
    return out

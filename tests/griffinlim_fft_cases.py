"""Inputs and references shared by the tests of the FFT form of Griffin-Lim (tests/test_griffinlim_fft_ref.py on the CPU,
tests/test_griffinlim_fft_gpu.py on the device), built the way tests/griffinlim_cases.py builds its own - decaying noise, another decay
per row, the last five magnitude rows zeroed under `denormalize` - over a geometry table of this form's own: the smallest at which each
of its mechanisms can go wrong.  Every array is computed once per key and handed out read-only."""
import functools

import numpy as np

import griffinlim_fft_ref as FR
import griffinlim_ref as GR
from oracle import features as FO

# (B, T, n_fft, win_length, hop_length)
GEOMETRIES = {
    "4frames": (2, 96, 128, 64, 32),            # every frame touches the reflected edge
    "18frames": (3, 544, 128, 64, 32),          # not a multiple of any frames-per-workgroup, three rows
    "fullwin": (2, 416, 128, 128, 32),          # win == n_fft, fourfold overlap: the widest halo
    "odd": (2, 400, 128, 100, 40),              # a window and a hop that are no powers of two
    "n128": (2, 1000, 128, 128, 32),
    "n512": (2, 2048, 512, 256, 128),           # 17 frames, M = 256
    "n1024": (2, 4096, 1024, 512, 256),         # 17 frames, M = 512
    "rir": (2, 9600, 256, 128, 64),             # the reference's own 129 x 151 (dataset.py:62-70)
    # more frames reach a workgroup's samples than one batch of 4096 / n_fft images holds: the overlap-add carries a sample's sum from
    # one batch of inverse transforms to the next, in the iterations and in the last synthesis
    "n1024x4": (2, 2048, 1024, 1024, 256),      # 9 frames, 4 images: fourfold overlap at M = 512
    "n512x4": (2, 2560, 512, 512, 128),         # 21 frames, 8 images: fourfold overlap at M = 256
    "gaps": (2, 9000, 256, 128, 3000),          # a hop beyond the window: samples no frame reaches (zero envelope), fewer frames per
                                                # workgroup than images because the run of samples would outgrow LDS
}
N_ITERS = (0, 1, 2, 32)
MOMENTA = (0.99, 0.0)
PAD_MODES = ("reflect", "constant")
CASES = [(name, n_iter, momentum, pad_mode, denormalize) for name in GEOMETRIES for n_iter in N_ITERS for momentum in MOMENTA
         for pad_mode in PAD_MODES for denormalize in (True, False)]
IDS = ["-".join((c[0], f"it{c[1]}", f"m{c[2]}", c[3], "denorm" if c[4] else "raw")) for c in CASES]


def dims(name):
    B, T, n_fft, win, hop = GEOMETRIES[name]
    return n_fft // 2 + 1, 1 + T // hop


@functools.lru_cache(maxsize=None)
def waveforms(name):
    """fp64 [B, T]: decaying noise, another draw and another decay per row (a batch-stride error shows)."""
    B, T, *_ = GEOMETRIES[name]
    rng = np.random.default_rng(4000 + sum(map(ord, name)))
    t = np.arange(T, dtype=np.float64)
    w = np.stack([rng.standard_normal(T) * np.exp(-t / (T / (5.0 + 2.0 * b))) * (0.5 + 0.25 * b) for b in range(B)])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def init_phase(name):
    """fp32 [B, n_bins, n_frames], turns in [0, 1)."""
    B = GEOMETRIES[name][0]
    rng = np.random.default_rng(5000 + sum(map(ord, name)))
    u = rng.random((B,) + dims(name), dtype=np.float32)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def features(name, denormalize):
    """fp32 [B, 2, H, W], planes padded to multiples of 16.  denormalize on: the PreProcess chain with the last five magnitude rows
    zeroed (they denormalise to a rounding residue of either sign that is not clamped).  Off: the raw |stft| in the magnitude plane.  The
    phase plane holds the analysed phase; Griffin-Lim must not read it."""
    B, T, n_fft, win, hop = GEOMETRIES[name]
    nb, nf = dims(name)
    H, W = ((nb + 15) // 16) * 16, ((nf + 15) // 16) * 16
    out = np.zeros((B, 2, H, W), dtype=np.float32)
    for b in range(B):
        if denormalize:
            f = FO.wav_to_feature(waveforms(name)[b], (H, W), n_fft, win, hop)
            f[0, nb - 5:nb, :] = 0.0
            out[b] = f.astype(np.float32)
        else:
            S = FO.stft(waveforms(name)[b], n_fft, win, hop)
            out[b, 0, :nb, :nf] = np.abs(S).astype(np.float32)
            out[b, 1, :nb, :nf] = ((np.angle(S) + np.pi) / (2 * np.pi)).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def magnitude(name, denormalize):
    """fp64 [B, n_bins, n_frames]: S as both forms of the loop define it, from the fp32 feature values"""
    nb, nf = dims(name)
    a = features(name, denormalize)[:, 0, :nb, :nf].astype(np.float64)
    if denormalize:
        a, _ = FO.denormalize(a, np.zeros_like(a))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(name, n_iter, momentum, pad_mode, denormalize):
    """The yardstick, fp64 [B, hop (n_frames - 1)]: griffinlim_ref on the fp32 feature values and the fp32 initial phases."""
    B, T, n_fft, win, hop = GEOMETRIES[name]
    y = np.stack([GR.griffinlim(magnitude(name, denormalize)[b], init_phase(name)[b], n_fft, win, hop, n_iter=n_iter, momentum=momentum,
                                pad_mode=pad_mode) for b in range(B)])
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def restated(name, n_iter, momentum, pad_mode, denormalize, variant=None):
    """fp32 [B, hop (n_frames - 1)]: the complex64 restatement (or a variant or a mutation of it) on the same data."""
    B, T, n_fft, win, hop = GEOMETRIES[name]
    y = np.array(FR.griffinlim32(magnitude(name, denormalize), init_phase(name), n_fft, win, hop, n_iter=n_iter, momentum=momentum,
                                 pad_mode=pad_mode, variant=variant))
    y.setflags(write=False)
    return y


def rel_err(y, ref):
    """e per row: max |y - y_ref| / max |y_ref|"""
    return np.abs(np.asarray(y, dtype=np.float64) - ref).max(axis=1) / np.abs(ref).max(axis=1)


def allowed(case):
    """what a device row may be off by: C e(restatement on the same data) + 2^-22, per row"""
    return FR.C * rel_err(restated(*case), reference(*case)) + 2.0 ** -22


def overlaps(name):
    B, T, n_fft, win, hop = GEOMETRIES[name]
    return hop < win


def convergence(y, case):
    """sc per row, in fp64: || |stft(y)| - S || / || S || with the case's S and pad mode"""
    name, n_iter, momentum, pad_mode, denormalize = case
    B, T, n_fft, win, hop = GEOMETRIES[name]
    S = magnitude(name, denormalize)
    return np.array([GR.spectral_convergence(np.asarray(y[b], dtype=np.float64), S[b], n_fft, win, hop, pad_mode) for b in range(B)])


@functools.lru_cache(maxsize=None)
def reference_convergence(case):
    c = convergence(reference(*case), case)
    c.setflags(write=False)
    return c


def excess(y, case):
    """per row, how far a result is from passing the two checks of the kernels, as multiples of what they allow (<= 1 passes both):
    (e / (C e(restatement) + 2^-22), |sc - sc64| / (SC_TOL sc64))"""
    c64 = reference_convergence(case)
    return rel_err(y, reference(*case)) / allowed(case), np.abs(convergence(y, case) - c64) / (FR.SC_TOL * c64)

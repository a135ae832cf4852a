"""Inputs and fp64 references shared by the Griffin-Lim tests (tests/test_griffinlim.py on the CPU, tests/test_griffinlim_gpu.py on
the device): every reference is computed once per (geometry, arguments) and handed out read-only."""
import functools

import numpy as np

import griffinlim_ref as GR
from oracle import features as FO

# (B, T, n_fft, win_length, hop_length)
GEOMETRIES = {
    "3frames": (2, 40, 64, 32, 16),             # every frame touches the reflected edge
    "11frames": (3, 160, 64, 32, 16),           # not a multiple of a 16-row tile
    "fullwin": (2, 176, 64, 64, 16),            # win == n_fft, 4x overlap
    "n128": (2, 1000, 128, 128, 32),
    "rir": (2, 9600, 256, 128, 64),             # the reference's own 129 x 151 (dataset.py:62-70)
}


def dims(name):
    B, T, n_fft, win, hop = GEOMETRIES[name]
    return n_fft // 2 + 1, 1 + T // hop


@functools.lru_cache(maxsize=None)
def waveforms(name):
    """fp64 [B, T]: decaying noise, another draw and another decay per sample (a batch-stride error shows)."""
    B, T, *_ = GEOMETRIES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    t = np.arange(T, dtype=np.float64)
    w = np.stack([rng.standard_normal(T) * np.exp(-t / (T / (5.0 + 2.0 * b))) * (0.5 + 0.25 * b) for b in range(B)])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def init_phase(name):
    """fp32 [B, n_bins, n_frames], turns in [0, 1)."""
    B = GEOMETRIES[name][0]
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    u = rng.random((B,) + dims(name), dtype=np.float32)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def features(name, denormalize, tight):
    """fp32 [B, 2, H, W].  denormalize on: the PreProcess chain (mean removal, extract, normalize, pad) with the last five
    magnitude rows zeroed - those denormalise to (10^-5 - 1e-5) 128, a rounding residue of either sign that is not clamped.
    Off: the raw |stft| in the magnitude plane.  The phase plane holds the analysed phase; Griffin-Lim must not read it."""
    B, T, n_fft, win, hop = GEOMETRIES[name]
    nb, nf = dims(name)
    H, W = (nb, nf) if tight else (((nb + 15) // 16) * 16, ((nf + 15) // 16) * 16)
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
def reference(name, denormalize, n_iter, momentum, pad_mode):
    """fp64 [B, hop (n_frames - 1)]: griffinlim_ref on the fp32 feature values and the fp32 initial phases."""
    B, T, n_fft, win, hop = GEOMETRIES[name]
    feat = features(name, denormalize, True)
    y = np.stack([GR.feature_to_wav(feat[b], init_phase(name)[b], dims(name), n_fft, win, hop, denormalize=denormalize,
                                    n_iter=n_iter, momentum=momentum, pad_mode=pad_mode) for b in range(B)])
    y.setflags(write=False)
    return y

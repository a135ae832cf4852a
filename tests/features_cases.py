"""Geometries, inputs and fp64 references shared by the per-element tests of the waveform <-> feature kernels
(tests/test_features.py on the CPU, tests/test_features_cases_gpu.py on the device).  Every input and every reference is computed
once and handed out read-only; the references are the FFT oracle (oracle/features.py) on the same fp32 values the kernels get."""
import functools

import numpy as np

import features_check as FK
from oracle import features as FO

# (B, T, n_fft, win_length, hop_length)
GEOMETRIES = {
    "rir": (2, 9600, 256, 128, 64),             # the reference's constants (dataset.py:62-70)
    "edge": (2, 17, 32, 16, 8),                 # T = n_fft/2 + 1: every frame reflects at both ends; T_out = 16 < one segment
    "oddwin": (2, 203, 32, 25, 7),              # odd window, truncated n_lo, hop not 2^k; T_out % 64 = 11; odd T: rows off 16 bytes
    "hop96": (2, 700, 256, 128, 96),            # hop > a 64-sample segment: segments reached by one frame; lowest envelope 0.043
    "hop_eq_win": (2, 300, 64, 32, 32),         # Hann tap 0 alone at 9 samples: envelope exactly 0 there, 9.2e-5 beside them
    "gaps": (2, 300, 64, 16, 40),               # hop > win: 175 of 280 output samples have no frame at all
    "n512": (2, 1100, 512, 512, 128),           # win == n_fft, 257 bins: the k loops go round twice
    "n1024": (1, 1300, 1024, 400, 100),         # the largest n_fft, 513 bins, hop not 2^k
    "n4": (2, 50, 4, 4, 1),                     # the smallest n_fft accepted, hop 1
}
PAD_MODES = ("reflect", "constant")
WAVE_KINDS = ("noise", "zeros")                 # "zeros" goes with remove_mean=False only
PLANE_KINDS = ("feature", "range", "raw")       # "raw" goes with denormalize=False
TIGHT = ("rir", "oddwin")
LAYOUTS = [(n, False) for n in GEOMETRIES] + [(n, True) for n in TIGHT]
LAYOUT_IDS = [n + ("-tight" if t else "") for n, t in LAYOUTS]
ZERO_ENVELOPE = {"gaps": 175, "hop_eq_win": 9}  # output samples whose envelope is at or below tiny
PLANTED = (-1.0, 0.0, 0.5, 1.0, 2.0, 2.5)       # phases planted in the "range" planes: the wrap's fixed points


def dims(name):
    B, T, n_fft, win, hop = GEOMETRIES[name]
    return n_fft // 2 + 1, 1 + T // hop


def t_out(name):
    B, T, n_fft, win, hop = GEOMETRIES[name]
    return hop * (T // hop)


def shape(name, tight):
    nb, nf = dims(name)
    return (nb, nf) if tight else (((nb + 15) // 16) * 16, ((nf + 15) // 16) * 16)


def _seed(name):
    return sum(map(ord, name))


def lead(name):
    """Length of the leading stretch of exact zeros of zero-waveform row 0: longer than n_fft + hop, so that at least two
    whole frames are silent - or all but the last eighth (at least 8 samples) of a waveform too short for that ("edge": T = 17
    is shorter than n_fft + hop = 40, and one frame is silent)."""
    B, T, n_fft, win, hop = GEOMETRIES[name]
    return min(n_fft + hop + 1, T - max(8, T // 8))


@functools.lru_cache(maxsize=None)
def waves(name, kind="noise"):
    """fp32.  "noise" [B, T]: decaying noise plus a small offset, another draw, decay and offset per row (a batch-stride error
    shows).  "zeros" [2, T]: row 0 begins with lead(name) exact zeros, as an impulse response does before the direct sound;
    row 1 is all zero."""
    B, T, *_ = GEOMETRIES[name]
    rng = np.random.default_rng(_seed(name) + (0 if kind == "noise" else 500))
    t = np.arange(T, dtype=np.float64)
    if kind == "noise":
        w = np.stack([rng.standard_normal(T) * np.exp(-t / (T / (3.0 + 2.0 * b))) * (0.5 + 0.25 * b) + 0.02 * (b + 1) for b in range(B)])
    else:
        w = np.zeros((2, T))
        n0 = lead(name)
        w[0, n0:] = rng.standard_normal(T - n0) * np.exp(-t[:T - n0] / (T / 3.0)) * 0.5 + 0.02
    w = w.astype(np.float32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def analysis(name, kind, pad_mode, remove_mean):
    """(S complex128 [B, n_bins, n_frames], sum|xw| fp64 [B, n_frames], silent bool [B, n_frames], mirror bool [B, n_frames]):
    see features_check.frame_stats"""
    B, T, n_fft, win, hop = GEOMETRIES[name]
    x = waves(name, kind)
    S, l1, silent, mirror = [], [], [], []
    for b in range(x.shape[0]):
        y = x[b].astype(np.float64)
        S.append(FO.stft(y - y.mean() if remove_mean else y, n_fft, win, hop, pad_mode))
        a, s, m = FK.frame_stats(x[b], n_fft, win, hop, pad_mode, remove_mean)
        l1.append(a)
        silent.append(s)
        mirror.append(m)
    out = (np.stack(S), np.stack(l1), np.stack(silent), np.stack(mirror))
    for o in out:
        o.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def planes(name, kind, tight, dirty):
    """fp32 [B, 2, H, W] synthesis inputs.  "feature": the oracle's own feature of the noise waveforms (mean removed, reflect).
    "range": what a phase-difference model hands over - amplitude uniform in [-0.2, 1.3], phase uniform in [-1.5, 2.5] with
    PLANTED at fixed places.  "raw": (|S|, angle S) for denormalize=False.  dirty: the appended rows and columns hold non-zero
    rubbish, otherwise zeros; the n_bins x n_frames block is the same either way."""
    B, T, n_fft, win, hop = GEOMETRIES[name]
    nb, nf = dims(name)
    H, W = shape(name, tight)
    rng = np.random.default_rng(_seed(name) + 1000 + PLANE_KINDS.index(kind))
    out = np.random.default_rng(_seed(name) + 2000).uniform(0.3, 3.0, (B, 2, H, W)) if dirty else np.zeros((B, 2, H, W))
    if kind == "range":
        out[:, 0, :nb, :nf] = rng.uniform(-0.2, 1.3, (B, nb, nf))
        ph = rng.uniform(-1.5, 2.5, (B, nb * nf))
        for j, v in enumerate(PLANTED):
            ph[:, 1 + 7 * j] = v
        out[:, 1, :nb, :nf] = ph.reshape(B, nb, nf)
    else:
        S = analysis(name, "noise", "reflect", True)[0]
        a, p = (np.abs(S), np.angle(S)) if kind == "raw" else FO.normalize(np.abs(S), np.angle(S))
        out[:, 0, :nb, :nf], out[:, 1, :nb, :nf] = a, p
    out = out.astype(np.float32)
    out.setflags(write=False)
    return out


def planted(name):
    """(row, column) of each PLANTED phase in the n_bins x n_frames block"""
    nb, nf = dims(name)
    return [divmod(1 + 7 * j, nf) for j in range(len(PLANTED))]


@functools.lru_cache(maxsize=None)
def synthesis(name, kind):
    """(y fp64 [B, T_out], A_t fp64 [B, T_out], envelope fp64 [T_out]) of planes(name, kind): the oracle on the fp32 values."""
    B, T, n_fft, win, hop = GEOMETRIES[name]
    nb, nf = dims(name)
    feat = planes(name, kind, True, False).astype(np.float64)
    y, A = [], []
    for b in range(B):
        if kind == "raw":
            amp, ph = feat[b, 0], feat[b, 1]
            y.append(FO.istft(amp * (np.cos(ph) + 1j * np.sin(ph)), n_fft, win, hop))
        else:
            amp = FO.denormalize(feat[b, 0], feat[b, 1])[0]
            y.append(FO.feature_to_wav(feat[b], (nb, nf), n_fft, win, hop))
        A.append(FK.abs_synthesis(amp, n_fft, win, hop))
    out = (np.stack(y), np.stack(A), FK.envelope(nf, n_fft, win, hop))
    for o in out:
        o.setflags(write=False)
    return out

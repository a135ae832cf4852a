"""The yardstick of the Griffin-Lim tests: a NumPy fp64 restatement of `librosa.griffinlim` as the reference calls it
(postprocess.py:130-131: `librosa.griffinlim(denorm_f, n_fft=n_fft, win_length=win_length, hop_length=hop_length)`), built on
`oracle.features.stft` / `istft`.

PARITY UNPINNED like the rest of the features path (oracle/features.py): librosa is absent here and is not pinned by the
reference; what is restated is librosa 0.9.x's published loop at its defaults (n_iter=32, momentum=0.99, init='random',
pad_mode='reflect', window='hann', center=True, length=None):

    angles  = exp(2 pi i u)                                   u = rng.rand(*S.shape)
    rebuilt = 0
    n_iter times:
        tprev   = rebuilt
        rebuilt = stft(istft(S * angles))
        angles  = rebuilt - momentum / (1 + momentum) * tprev
        angles /= |angles| + 1e-16
    return istft(S * angles)

librosa keeps `angles` in complex64; this restatement (and the device) keeps everything in fp64, which is what makes a comparison per
element possible: two fp64 forms with different summation orders agree to ~1e-11 of the peak after 32 iterations, a complex64
form drifts to ~1e-5.  The random draw is an argument, `init_phase`, in turns: u in [0, 1), one per bin.
"""
import numpy as np

from oracle import features as FO


def griffinlim(S, init_phase, n_fft=256, win_length=128, hop_length=64, n_iter=32, momentum=0.99, pad_mode="reflect"):
    """S fp64 [n_bins, n_frames] (not clamped, as librosa does not), init_phase [n_bins, n_frames] in turns -> fp64
    [hop_length * (n_frames - 1)]."""
    S = np.asarray(S, dtype=np.float64)
    u = np.asarray(init_phase, dtype=np.float64)
    assert S.shape == u.shape and S.shape[0] == n_fft // 2 + 1
    angles = np.cos(2.0 * np.pi * u) + 1j * np.sin(2.0 * np.pi * u)
    rebuilt = 0.0
    alpha = momentum / (1.0 + momentum)
    for _ in range(n_iter):
        tprev = rebuilt
        inverse = FO.istft(S * angles, n_fft, win_length, hop_length)
        rebuilt = FO.stft(inverse, n_fft, win_length, hop_length, pad_mode)
        angles = rebuilt - alpha * tprev
        angles = angles / (np.abs(angles) + 1e-16)
    return FO.istft(S * angles, n_fft, win_length, hop_length)


def feature_to_wav(feat, init_phase, des_shape, n_fft=256, win_length=128, hop_length=64, denormalize=True, **kw):
    """PostProcess.post_process with algorithm='gl' without the file writes (postprocess.py:69-72): un_pad -> denormalize ->
    griffinlim of the magnitude, for one feature [2, H, W] (the phase plane is ignored)."""
    a = np.asarray(feat, dtype=np.float64)[0, :des_shape[0], :des_shape[1]]
    if denormalize:
        a, _ = FO.denormalize(a, np.zeros_like(a))
    return griffinlim(a, init_phase, n_fft, win_length, hop_length, **kw)


def spectral_convergence(y, S, n_fft=256, win_length=128, hop_length=64, pad_mode="reflect"):
    """|| |stft(y)| - S ||_F / || S ||_F"""
    R = np.abs(FO.stft(y, n_fft, win_length, hop_length, pad_mode))
    return float(np.linalg.norm(R - S) / np.linalg.norm(S))

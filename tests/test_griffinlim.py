"""CPU checks of the Griffin-Lim yardstick (tests/griffinlim_ref.py) and argument validation of its C entry points (no GPU).

The restatement is held to an independent implementation of the same published loop: torch.stft / torch.istft in fp64 on the
CPU (another FFT, another overlap-add).  Bound: max|dy| <= 1e-9 max|y|.  Two NumPy forms with different summation orders
(np.fft and a direct DFT matrix product) agree to 8.1e-12 max|y| after 32 iterations over these geometries - the iteration does
not amplify rounding - and the bound is that with two orders of margin.  PARITY UNPINNED w.r.t. librosa itself (absent here)."""
import numpy as np
import pytest
import torch

import griffinlim_cases as GC
import griffinlim_ref as GR
from oracle import features as FO


def torch_griffinlim(S, u, n_fft, win, hop, n_iter, momentum, pad_mode):
    """The loop of griffinlim_ref on torch's transform pair.  The analysis pads by hand (numpy.pad) and runs uncentred:
    torch.stft refuses a reflect padding as long as the signal, which the 3-frame geometry needs."""
    w = torch.hann_window(win, periodic=True, dtype=torch.float64)
    S = torch.tensor(np.asarray(S, dtype=np.float64))
    u = torch.tensor(np.asarray(u, dtype=np.float64))
    angles = torch.complex(torch.cos(2 * np.pi * u), torch.sin(2 * np.pi * u))
    rebuilt = torch.zeros_like(angles)
    alpha = momentum / (1 + momentum)
    for _ in range(n_iter):
        tprev = rebuilt
        inverse = torch.istft(S * angles, n_fft, hop, win, w, center=True)
        padded = torch.tensor(np.pad(inverse.numpy(), n_fft // 2, mode=pad_mode))
        rebuilt = torch.stft(padded, n_fft, hop, win, w, center=False, return_complex=True)
        angles = rebuilt - alpha * tprev
        angles = angles / (angles.abs() + 1e-16)
    return torch.istft(S * angles, n_fft, hop, win, w, center=True).numpy()


@pytest.mark.parametrize("n_iter", [0, 1, 2, 32])
@pytest.mark.parametrize("name", list(GC.GEOMETRIES))
def test_restatement_matches_the_torch_loop(name, n_iter):
    B, T, n_fft, win, hop = GC.GEOMETRIES[name]
    for pad_mode, momentum in (("reflect", 0.99), ("reflect", 0.0), ("constant", 0.99), ("constant", 0.0)):
        for b in range(B):
            S = np.abs(FO.stft(GC.waveforms(name)[b], n_fft, win, hop))
            u = GC.init_phase(name)[b]
            y = GR.griffinlim(S, u, n_fft, win, hop, n_iter, momentum, pad_mode)
            yt = torch_griffinlim(S, u, n_fft, win, hop, n_iter, momentum, pad_mode)
            assert y.shape == yt.shape == (hop * (T // hop),)
            err, peak = float(np.abs(y - yt).max()), float(np.abs(y).max())
            print(f"{name} n_iter={n_iter} {pad_mode} momentum={momentum} b={b}: max|dy| = {err:.3e} = {err / peak:.3e} max|y|")
            assert peak > 0 and err <= 1e-9 * peak


@pytest.mark.parametrize("name", list(GC.GEOMETRIES))
def test_zero_iterations_is_one_inverse_transform(name):
    B, T, n_fft, win, hop = GC.GEOMETRIES[name]
    S = np.abs(FO.stft(GC.waveforms(name)[0], n_fft, win, hop))
    u = GC.init_phase(name)[0].astype(np.float64)
    y = GR.griffinlim(S, u, n_fft, win, hop, n_iter=0)
    assert np.array_equal(y, FO.istft(S * (np.cos(2 * np.pi * u) + 1j * np.sin(2 * np.pi * u)), n_fft, win, hop))
    # the feature form un-pads, denormalises and ignores the phase plane
    feat = GC.features(name, True, False).astype(np.float64)
    other = feat[0].copy()
    other[1] = 0.25
    a, _ = FO.denormalize(feat[0, 0, :GC.dims(name)[0], :GC.dims(name)[1]], 0.0)
    assert float(a.min()) < 1e-12                     # the zeroed rows: a residue around zero, not clamped
    assert np.array_equal(GR.feature_to_wav(other, u, GC.dims(name), n_fft, win, hop, n_iter=2),
                          GR.griffinlim(a, u, n_fft, win, hop, n_iter=2))


def test_spectral_convergence_falls():
    """|| |stft(y)| - S || / || S || from the random-phase start to 32 iterations, decaying noise at the reference's size."""
    B, T, n_fft, win, hop = GC.GEOMETRIES["rir"]
    for b in range(B):
        S = np.abs(FO.stft(GC.waveforms("rir")[b], n_fft, win, hop))
        u = GC.init_phase("rir")[b]
        sc = [GR.spectral_convergence(GR.griffinlim(S, u, n_fft, win, hop, n_iter=n), S, n_fft, win, hop) for n in (0, 32)]
        print(f"sample {b}: spectral convergence {sc[0]:.3f} -> {sc[1]:.3f}")
        assert sc[1] < sc[0]


def test_entry_points_validate_without_gpu():
    """UNETRIR_EINVAL (10001) before the device is touched; the pointers are never dereferenced on the host."""
    import ctypes as C
    import unet_rir_amd
    L = unet_rir_amd._lib.lib()
    need = L.unetrir_griffinlim_ws_bytes(2, 129, 151, 256)
    assert need > 0
    assert need >= 2 * 151 * (7 * 129 + 128) * 8        # S, S angles, rebuilt, tprev (complex) and the waveform, all fp64
    assert L.unetrir_griffinlim_ws_bytes(2, 128, 151, 256) == 0 and L.unetrir_griffinlim_ws_bytes(2, 129, 1, 256) == 0

    def call(B=2, H=144, W=160, n_bins=129, n_frames=151, n_fft=256, win=128, hop=64, pad_mode=0, denorm=1, n_iter=32, momentum=0.99,
             feat=4096, wav=4096, ws=4096, ws_bytes=need):
        return L.unetrir_griffinlim_f32(feat, B, H, W, n_bins, n_frames, n_fft, win, hop, pad_mode, denorm, n_iter, C.c_float(momentum),
                                        None, 0, 0, wav, ws, ws_bytes, None)

    assert call(n_bins=128) == 10001                   # n_bins != n_fft/2 + 1
    assert call(n_bins=130) == 10001
    assert call(n_frames=1) == 10001                   # n_frames < 2
    assert call(n_iter=-1) == 10001
    assert call(ws_bytes=need - 1) == 10001            # a short workspace
    assert call(feat=None) == 10001 and call(wav=None) == 10001 and call(ws=None) == 10001
    assert call(momentum=-0.5) == 10001 and call(pad_mode=2) == 10001
    assert call(momentum=float("inf")) == 10001 and call(momentum=float("nan")) == 10001
    assert call(n_fft=192, n_bins=97) == 10001 and call(win=257) == 10001 and call(hop=0) == 10001
    assert call(H=128) == 10001 and call(W=150) == 10001 and call(B=0) == 10001
    assert L.unetrir_uniform_f32(None, 16, 0, 0, None) == 10001 and L.unetrir_uniform_f32(4096, 0, 0, 0, None) == 10001

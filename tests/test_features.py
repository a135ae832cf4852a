"""CPU checks of the waveform <-> feature oracle (oracle/features.py): against torch.stft / torch.istft (an independent
implementation of the same published algorithm), the analysis -> synthesis round trip, the committed golden vectors, and
argument validation of the C entry points (no GPU needed); and, second half, the case table of the per-element device tests
(tests/features_cases.py): its oracle against torch, the twins behind the bounds' constants (tests/features_check.py), and the
preconditions tests/test_features_cases_gpu.py relies on.  PARITY UNPINNED w.r.t. librosa itself (absent here)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_features_golden as MFG  # noqa: E402
from oracle import features as FO  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", list(MFG.CASES))
def test_oracle_matches_torch_stft_and_istft(name):
    B, T, n_fft, win, hop, shape, pad_mode = MFG.CASES[name]
    wav = MFG.waveforms(name).astype(np.float64)
    w = torch.hann_window(win, periodic=True, dtype=torch.float64)
    for b in range(B):
        S = FO.stft(wav[b], n_fft, win, hop, pad_mode)
        St = torch.stft(torch.tensor(wav[b]), n_fft, hop, win, w, center=True, pad_mode=pad_mode, return_complex=True)
        assert S.shape == (n_fft // 2 + 1, 1 + T // hop)
        assert float(np.abs(S - St.numpy()).max()) <= 1e-12 * max(1.0, float(np.abs(S).max()))
        y = FO.istft(S, n_fft, win, hop)
        yt = torch.istft(St, n_fft, hop, win, w, center=True).numpy()
        assert y.shape == (hop * (T // hop),)
        assert float(np.abs(y - yt).max()) <= 1e-12
        assert float(np.abs(y - wav[b][:len(y)]).max()) <= 1e-12     # Hann at 50 % / 25 % hop reconstructs exactly


def test_reference_constants_give_the_reference_shapes():
    """0.2 s at 48 kHz with n_fft 256 / hop 64 is 129 x 151, padded to (144, 160) (dataset.py:62-70, postprocess.py:51)."""
    wav = MFG.waveforms("features_rir_9600")[0]
    f = FO.wav_to_feature(wav)
    assert f.shape == (2, 144, 160)
    assert float(f.min()) >= 0.0 and float(f.max()) <= 1.0
    assert not f[:, 129:, :].any() and not f[:, :, 151:].any()
    back = FO.feature_to_wav(f)
    assert back.shape == (9600,)
    assert float(np.abs(back - (wav.astype(np.float64) - wav.astype(np.float64).mean())).max()) <= 1e-6


def test_normalizer_round_trip_and_ranges():
    amp = np.array([0.0, 1e-6, 1e-3, 1.0, 128.0 * (1 - FO.EP)])
    ph = np.array([-np.pi, -1.0, 0.0, 1.0, np.pi - 1e-9])
    a, p = FO.normalize(amp, ph)
    assert abs(a[0]) <= 1e-12 and abs(a[-1] - 1.0) <= 1e-12 and abs(p[0]) <= 1e-15 and p[-1] < 1.0
    amp2, ph2 = FO.denormalize(a, p)
    assert np.allclose(amp2, amp, rtol=1e-9, atol=1e-12) and np.allclose(ph2, ph, atol=1e-12)


@pytest.mark.parametrize("name", list(MFG.CASES))
def test_golden_vectors_are_reproduced(name):
    gold = dict(np.load(os.path.join(GOLD, name + ".npz")))
    got = MFG.compute(name)
    for k, v in gold.items():
        assert got[k].shape == v.shape, k
        assert float(np.abs(got[k].astype(np.float64) - v.astype(np.float64)).max()) <= 1e-6 * max(1.0, float(np.abs(v).max())), k


def test_entry_points_reject_bad_arguments_without_gpu():
    import unet_rir_amd
    L = unet_rir_amd._lib.lib()
    assert L.unetrir_stft_frames(9600, 64) == 151 and L.unetrir_stft_frames(1000, 32) == 32
    one = 16                                        # a non-null, never dereferenced pointer: validation happens before launch
    E = 10001
    assert L.unetrir_stft_features_f32(None, 1, 9600, 256, 128, 64, 0, 1, 1, one, 144, 160, None) == E
    assert L.unetrir_stft_features_f32(one, 1, 9600, 250, 128, 64, 0, 1, 1, one, 144, 160, None) == E     # n_fft not 2^k
    assert L.unetrir_stft_features_f32(one, 1, 9600, 256, 300, 64, 0, 1, 1, one, 144, 160, None) == E     # win > n_fft
    assert L.unetrir_stft_features_f32(one, 1, 9600, 256, 128, 64, 0, 1, 1, one, 128, 160, None) == E     # H < 129
    assert L.unetrir_stft_features_f32(one, 1, 9600, 256, 128, 64, 0, 1, 1, one, 144, 150, None) == E     # W < 151
    assert L.unetrir_stft_features_f32(one, 1, 100, 256, 128, 64, 0, 1, 1, one, 144, 160, None) == E      # reflect needs T > n_fft/2
    assert L.unetrir_stft_features_f32(one, 1, 9600, 256, 128, 64, 2, 1, 1, one, 144, 160, None) == E     # pad mode
    assert L.unetrir_istft_features_f32(one, 1, 144, 160, 128, 151, 256, 128, 64, 1, one, None) == E      # bins != n_fft/2+1
    assert L.unetrir_istft_features_f32(one, 1, 144, 160, 129, 161, 256, 128, 64, 1, one, None) == E      # frames > W
    assert L.unetrir_istft_features_f32(one, 1, 144, 160, 129, 1, 256, 128, 64, 1, one, None) == E        # no output samples


# ------------------------------------------------------------------------------------------------------------------------------
# The case table of the per-element tests (tests/features_cases.py), the twins and bounds (tests/features_check.py), and the
# preconditions tests/test_features_cases_gpu.py relies on.
import features_cases as FC  # noqa: E402
import features_check as FK  # noqa: E402


@pytest.mark.parametrize("pad_mode", FC.PAD_MODES)
@pytest.mark.parametrize("name", list(FC.GEOMETRIES))
def test_case_oracle_matches_torch_stft(name, pad_mode):
    B, T, n_fft, win, hop = FC.GEOMETRIES[name]
    w = torch.hann_window(win, periodic=True, dtype=torch.float64)
    for kind in FC.WAVE_KINDS:
        x = FC.waves(name, kind).astype(np.float64)
        S = FC.analysis(name, kind, pad_mode, False)[0]
        assert S.shape == (x.shape[0],) + FC.dims(name)
        for b in range(x.shape[0]):
            St = torch.stft(torch.tensor(x[b]), n_fft, hop, win, w, center=True, pad_mode=pad_mode, return_complex=True).numpy()
            assert float(np.abs(S[b] - St).max()) <= 1e-12 * max(1.0, float(np.abs(St).max())), (kind, b)


@pytest.mark.parametrize("name", list(FC.GEOMETRIES))
def test_case_oracle_matches_torch_istft_or_the_identity(name):
    """torch.istft where it accepts the overlap; it refuses the two geometries whose envelope has zeros, and there the oracle is
    held to istft(stft(x)) == x on the samples whose envelope exceeds 1e-3 and to exact zeros where no frame reaches."""
    B, T, n_fft, win, hop = FC.GEOMETRIES[name]
    w = torch.hann_window(win, periodic=True, dtype=torch.float64)
    x = FC.waves(name).astype(np.float64)
    S = FC.analysis(name, "noise", "reflect", False)[0]
    env = FK.envelope(FC.dims(name)[1], n_fft, win, hop)
    for b in range(B):
        y = FO.istft(S[b], n_fft, win, hop)
        assert y.shape == (FC.t_out(name),)
        if name in FC.ZERO_ENVELOPE:
            with pytest.raises(RuntimeError):
                torch.istft(torch.tensor(S[b]), n_fft, hop, win, w, center=True)
        else:
            yt = torch.istft(torch.tensor(S[b]), n_fft, hop, win, w, center=True).numpy()
            assert float(np.abs(y - yt).max()) <= 1e-12 * max(1.0, float(np.abs(yt).max()))
        live = env > 1e-3
        assert float(np.abs(y - x[b][:len(y)])[live].max()) <= 1e-12 * max(1.0, float(np.abs(x[b]).max()))
        assert not y[env == 0.0].any()
    assert int((env <= FO.TINY32).sum()) == FC.ZERO_ENVELOPE.get(name, 0)
    assert int((env == 0.0).sum()) == FC.ZERO_ENVELOPE.get(name, 0)         # nothing between 0 and tiny: a Hann tap is 0 or > 1e-3


def test_twins_agree_with_the_oracle_within_the_recorded_gaps():
    """The constants of the bounds stay reproducible: the measured twin-versus-oracle gaps are within x4 of the recorded ones
    (and the recorded ones are not padded: within x4 the other way), and the epsilons are 64 times the recorded gaps."""
    ga, gs = FK.measure_gaps()
    print(f"analysis gap {ga:.3e} (recorded {FK.MEASURED_GAP_ANALYSIS:.3e}), synthesis gap {gs:.3e} (recorded {FK.MEASURED_GAP_SYNTHESIS:.3e})")
    assert FK.MEASURED_GAP_ANALYSIS / 4.0 <= ga <= 4.0 * FK.MEASURED_GAP_ANALYSIS
    assert FK.MEASURED_GAP_SYNTHESIS / 4.0 <= gs <= 4.0 * FK.MEASURED_GAP_SYNTHESIS
    assert FK.EPS_ANALYSIS == 64.0 * FK.MEASURED_GAP_ANALYSIS and FK.EPS_SYNTHESIS == 64.0 * FK.MEASURED_GAP_SYNTHESIS


@pytest.mark.parametrize("name", list(FC.GEOMETRIES))
def test_case_preconditions(name):
    B, T, n_fft, win, hop = FC.GEOMETRIES[name]
    nb, nf = FC.dims(name)
    x = FC.waves(name)
    assert x.dtype == np.float32 and x.shape == (B, T)
    if B > 1:
        assert float(np.abs(x[0] - x[1]).max()) > 0.1                               # a batch-stride error shows
    for pad_mode in FC.PAD_MODES:
        for remove_mean in (True, False):
            S, l1, silent, mirror = FC.analysis(name, "noise", pad_mode, remove_mean)
            delta, dec, und, mir, nop = FK.classify(S, l1, mirror)
            assert und.sum() <= FK.UNDECIDED_CAP * und.size and not nop.any() and not silent.any()
            assert not mirror.any() if pad_mode == "constant" else (mirror.sum(axis=1) <= 2).all()    # frame 0, the one on sample T - 1
            for row in (0, nb - 1):                                                 # imaginary part exactly +0 on DC and Nyquist
                assert not S[:, row].imag.any() and not np.signbit(S[:, row].imag).any()
                assert (np.abs(S[:, row]) > 4.0 * delta[:, 0]).all()
                if remove_mean:                                                     # both signs: 0.5 and 1.0 on the phase plane
                    assert (S[:, row].real > 0).any() and (S[:, row].real < 0).any(), (pad_mode, row)
        # exact zeros: silent frames are exactly silent in the oracle, with phase exactly 0.5
        S, l1, silent, mirror = FC.analysis(name, "zeros", pad_mode, False)
        assert int(silent[0].sum()) >= (1 if name == "edge" else 2) and not silent[0].all() and silent[1].all()
        sb = np.broadcast_to(silent[:, None, :], S.shape)
        assert not S[sb].any() and not l1[silent].any() and (l1[~silent] > 0).all()
        a, p = FO.normalize(np.abs(S), np.angle(S))
        assert (p[sb] == 0.5).all() and (np.angle(S)[sb] == 0.0).all() and float(np.abs(a[sb]).max()) <= 1e-15
        delta, dec, und, mir, nop = FK.classify(S, l1, mirror)
        assert und.sum() <= FK.UNDECIDED_CAP * und.size and not (nop & ~sb).any()
    assert FC.lead(name) > n_fft + hop or name == "edge"
    assert not FC.waves(name, "zeros")[0, :FC.lead(name)].any() and FC.waves(name, "zeros")[0, FC.lead(name):].all()
    # synthesis inputs
    y, A, env = FC.synthesis(name, "range")
    assert int((env <= FO.TINY32).sum()) == FC.ZERO_ENVELOPE.get(name, 0)
    for kind in FC.PLANE_KINDS:
        for tight in ((False, True) if name in FC.TIGHT else (False,)):
            clean, dirty = FC.planes(name, kind, tight, False), FC.planes(name, kind, tight, True)
            assert clean.dtype == np.float32 and clean.shape == dirty.shape == (B, 2) + FC.shape(name, tight)
            assert np.array_equal(clean[:, :, :nb, :nf], dirty[:, :, :nb, :nf])
            assert np.array_equal(clean[:, :, :nb, :nf], FC.planes(name, kind, True, False))
            assert not clean[:, :, nb:, :].any() and not clean[:, :, :, nf:].any()
            assert dirty[:, :, nb:, :].all() and dirty[:, :, :, nf:].all()
    r = FC.planes(name, "range", True, False)
    assert r[:, 0].min() < -0.1 and r[:, 0].max() > 1.2 and r[:, 1].min() < -1.0 and r[:, 1].max() > 2.0
    for (k, f), v in zip(FC.planted(name), FC.PLANTED):
        assert (r[:, 1, k, f] == np.float32(v)).all()
        ph = FO.denormalize(r[:, 0, k, f].astype(np.float64), r[:, 1, k, f].astype(np.float64))[1]
        assert (ph == (0.0 if v in (0.5, 2.5) else -np.pi)).all(), (v, ph)          # -1, 0, 1, 2 -> -pi; 0.5, 2.5 -> 0
        assert (FK.twin_denormalize(r[:, 0, k, f].astype(np.float64), r[:, 1, k, f].astype(np.float64))[1] == ph).all()


@pytest.mark.parametrize("name", list(FC.GEOMETRIES))
def test_twins_pass_the_checks_the_kernels_are_held_to(name):
    """A dry run of the device tests with the twins in the kernels' place: the bounds can be met by the kernels' arithmetic."""
    B, T, n_fft, win, hop = FC.GEOMETRIES[name]
    for pad_mode in FC.PAD_MODES:
        for kind, remove_mean in (("noise", True), ("noise", False), ("zeros", False)):
            S, l1, silent, mirror = FC.analysis(name, kind, pad_mode, remove_mean)
            x = FC.waves(name, kind)
            St = np.stack([FK.twin_stft(x[b], n_fft, win, hop, pad_mode, remove_mean) for b in range(x.shape[0])])
            amp, ph = np.abs(St), np.arctan2(St.imag, St.real)
            FK.check_planes(f"{name} {pad_mode} {kind} mean={remove_mean} raw", amp.astype(np.float32), ph.astype(np.float32), S, l1,
                            False, silent, mirror)
            a, p = FO.normalize(amp, ph)
            FK.check_planes(f"{name} {pad_mode} {kind} mean={remove_mean} normalised", a.astype(np.float32), p.astype(np.float32), S, l1,
                            True, silent, mirror)
    for kind in FC.PLANE_KINDS:
        feat = FC.planes(name, kind, True, False)
        y, A, env = FC.synthesis(name, kind)
        yt = np.stack([FK.twin_istft(feat[b, 0], feat[b, 1], n_fft, win, hop, kind != "raw") for b in range(B)])
        FK.check_wave(f"{name} {kind}", yt.astype(np.float32), y, A, env)


def test_the_checks_catch_what_the_max_norm_and_the_circle_let_through():
    name = "rir"
    B, T, n_fft, win, hop = FC.GEOMETRIES[name]
    S, l1, silent, mirror = FC.analysis(name, "noise", "constant", True)
    a, p = FO.normalize(np.abs(S), np.angle(S))
    a32, p32 = a.astype(np.float32), p.astype(np.float32)
    FK.check_planes("oracle", a32, p32, S, l1, True, silent, mirror)
    # a DC bin flipped from 1.0 to 0.0: the same point of the circle, the opposite end of the network's input range
    f = int(np.argmax(S[0, 0].real < 0))
    assert p32[0, 0, f] == 1.0
    flipped = p32.copy()
    flipped[0, 0, f] = 0.0
    assert float(FK.circ(flipped.astype(np.float64), p).max()) <= 2.0 ** -24
    with pytest.raises(AssertionError):
        FK.check_planes("flipped", a32, flipped, S, l1, True, silent, mirror)
    # a wrong value in the quietest bin: far inside 2e-6 max|S|, far outside its own bound
    raw_a, raw_p = np.abs(S).astype(np.float32), np.angle(S).astype(np.float32)
    FK.check_planes("oracle raw", raw_a, raw_p, S, l1, False, silent, mirror)
    q = np.unravel_index(int(np.argmin(np.abs(S))), S.shape)
    quiet = raw_a.copy()
    quiet[q] += np.float32(1e-6 * np.abs(S).max())
    assert abs(float(quiet[q]) - float(np.abs(S[q]))) <= 2e-6 * float(np.abs(S).max())
    with pytest.raises(AssertionError):
        FK.check_planes("quiet", quiet, raw_p, S, l1, False, silent, mirror)
    # a sample beside a zero of the envelope that is off by 1e-6 of the waveform's peak
    y, A, env = FC.synthesis("hop_eq_win", "feature")
    FK.check_wave("oracle", y.astype(np.float32), y, A, env)
    t = int(np.argmin(np.where(env > FO.TINY32, env, np.inf)))
    off = y.astype(np.float32)
    off[0, t] += np.float32(1e-6 * np.abs(y).max())
    with pytest.raises(AssertionError):
        FK.check_wave("off", off, y, A, env)
    dead = y.astype(np.float32)
    dead[1, int(np.argmax(env <= FO.TINY32))] = np.float32(1e-30)
    with pytest.raises(AssertionError):
        FK.check_wave("dead", dead, y, A, env)

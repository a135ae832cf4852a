"""The fp64 restatement of tests/auralize_ref.py against numpy.convolve, and write_wav against read_wav (CPU)."""
import numpy as np
import pytest

from auralize_ref import convolve_ref, make_data

GEOMS = [(1, 1), (1, 40), (40, 1), (7, 7), (33, 100), (100, 33), (257, 64)]          # K = 1, N = 1, N < K, N > K


@pytest.mark.parametrize("K,N", GEOMS)
def test_restatement_equals_numpy_convolve_on_integer_data(K, N):
    h, x = make_data(K, N, "int")
    y, S, terms = convolve_ref(h, x)
    assert y.shape == (3, N + K - 1) and y.dtype == np.float64
    for b in range(3):
        hb, xb = h[b].astype(np.float64), x[b].astype(np.float64)
        assert np.array_equal(y[b], np.convolve(hb, xb))
        assert np.array_equal(S[b], np.convolve(np.abs(hb), np.abs(xb)))
        assert np.array_equal(terms[b], np.convolve((hb != 0).astype(np.int64), (xb != 0).astype(np.int64)))
    ys, Ss, ts = convolve_ref(h, x[0])                       # one x for every row
    for b in range(3):
        assert np.array_equal(ys[b], np.convolve(h[b].astype(np.float64), x[0].astype(np.float64)))
    assert np.array_equal(ys[0], y[0]) and np.array_equal(Ss[0], S[0]) and np.array_equal(ts[0], terms[0])


@pytest.mark.parametrize("K,N", GEOMS)
def test_restatement_equals_numpy_convolve_on_random_data(K, N):
    """Both are fp64 sums of the same terms in orders of their own: they agree within the terms' roundings."""
    h, x = make_data(K, N, "uniform")
    assert np.abs(h).min() >= 2.0 ** -10 and np.abs(x).min() >= 2.0 ** -10 and np.abs(h).max() <= 1.0 and np.abs(x).max() <= 1.0
    y, S, terms = convolve_ref(h, x)
    for b in range(3):
        ref = np.convolve(h[b].astype(np.float64), x[b].astype(np.float64))
        assert np.all(np.abs(y[b] - ref) <= 2.0 * (terms[b] + 1) * 2.0 ** -53 * S[b])
        n = np.arange(N + K - 1)
        assert np.array_equal(terms[b], np.minimum(np.minimum(n + 1, N + K - 1 - n), min(K, N)))      # no term is zero here


def test_vectors_truncation_and_the_literal_sum():
    h, x = make_data(5, 9, "int")
    y, S, terms = convolve_ref(h[0], x[0])
    assert y.shape == (13,)
    for n in range(13):                                      # the definition, term by term
        t = [float(h[0][k]) * float(x[0][n - k]) for k in range(5) if 0 <= n - k < 9]
        assert y[n] == sum(t) and S[n] == sum(abs(v) for v in t) and terms[n] == sum(v != 0 for v in t)
    for L in (1, 9, 13):
        yl, Sl, tl = convolve_ref(h[0], x[0], L)
        assert np.array_equal(yl, y[:L]) and np.array_equal(Sl, S[:L]) and np.array_equal(tl, terms[:L])


@pytest.mark.parametrize("shape", [(4801,), (1200, 2)])
def test_write_wav_then_read_wav_returns_the_data(tmp_path, shape):
    """write_wav stores the fp32 values as they are; read_wav averages the channels and subtracts the mean in fp32."""
    from unet_rir_amd import read_wav
    from unet_rir_amd.auralize import write_wav
    rng = np.random.default_rng(3)
    data = (rng.uniform(-0.9, 0.9, size=shape) + 0.05).astype(np.float32)
    p = str(tmp_path / "a.wav")
    write_wav(p, data, 48000)
    raw = open(p, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and int.from_bytes(raw[4:8], "little") == len(raw) - 8
    assert int.from_bytes(raw[20:22], "little") == 3 and int.from_bytes(raw[34:36], "little") == 32          # IEEE float, 32 bit
    assert raw[-data.nbytes:] == data.tobytes()
    T = shape[0]
    got = read_wav(p, 48000, (T + 0.5) / 48000)            # int(duration * rate) == T
    mono = data if data.ndim == 1 else data.mean(axis=1, dtype=np.float32)
    want = mono - np.mean(mono)
    assert got.dtype == np.float32 and got.shape == (T,) and np.array_equal(got, want)
    if data.ndim == 2:
        both = read_wav(p, 48000, (T + 0.5) / 48000, mono=False)
        assert np.array_equal(both, data.T - np.mean(data.T))
    with pytest.raises(ValueError):
        read_wav(p, 44100, T / 44100)                         # no resampler
    import torch
    write_wav(p, torch.from_numpy(data), 48000)               # a tensor is taken too
    assert open(p, "rb").read() == raw
    with pytest.raises(ValueError):
        write_wav(p, np.zeros((2, 3, 4), np.float32), 48000)
    with pytest.raises(ValueError):
        write_wav(p, data, 0)

"""The file ends of scripts/auralize.py --stream, without a GPU: the dry signal read in chunks is `read_wav`'s signal bit for bit - the
mean included, which numpy sums in runs of np.getbufsize() elements - and `WavWriter` writes the bytes of `write_wav`."""
import importlib.util
import os
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("auralize_script", os.path.join(ROOT, "scripts", "auralize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _chunked(script, path, per_chunk):
    frames, rate, chunks = script.dry_chunks(path, per_chunk)
    mean, n = script.dry_mean(chunks)
    assert n == frames
    parts = []
    for x in chunks():
        mono = x.mean(axis=1, dtype=np.float32)
        mono -= mean
        parts.append(mono)
    return rate, np.concatenate(parts)


# lengths around the runs of numpy's summation (8192) and its pairwise blocks (128), and one of many runs
@pytest.mark.parametrize("frames", (1, 7, 129, 8191, 8192, 8193, 40000, 100003, 250001))
def test_a_float_file_in_chunks_is_read_wav(script, tmp_path, frames):
    import unet_rir_amd as U
    from unet_rir_amd.auralize import write_wav
    rng = np.random.default_rng(frames)
    path = str(tmp_path / "dry.wav")
    write_wav(path, (rng.uniform(-0.5, 0.5, frames) + 0.25).astype(np.float32), 8000)
    want = U.read_wav(path, 8000, (frames + 0.5) / 8000)
    for per_chunk in (8192, 3 * 8192):
        rate, got = _chunked(script, path, per_chunk)
        assert rate == 8000 and got.dtype == np.float32 and np.array_equal(got, want), per_chunk


@pytest.mark.parametrize("width, channels", ((2, 1), (2, 2), (3, 2), (4, 1)))
def test_a_pcm_file_in_chunks_is_read_wav(script, tmp_path, width, channels):
    import unet_rir_amd as U
    frames = 50001
    rng = np.random.default_rng([width, channels])
    path = str(tmp_path / "dry.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(8000)
        f.writeframes(rng.integers(0, 256, size=frames * channels * width, dtype=np.uint8).tobytes())
    want = U.read_wav(path, 8000, (frames + 0.5) / 8000)
    rate, got = _chunked(script, path, 2 * 8192)
    assert rate == 8000 and np.array_equal(got, want)


@pytest.mark.parametrize("shape", ((5000,), (5000, 1), (777, 3)))
def test_the_incremental_writer_writes_the_bytes_of_write_wav(tmp_path, shape):
    from unet_rir_amd.auralize import WavWriter, write_wav
    x = np.random.default_rng(3).uniform(-1, 1, shape).astype(np.float32)
    write_wav(str(tmp_path / "whole.wav"), x, 48000)
    with WavWriter(str(tmp_path / "pieces.wav"), 48000, channels=1 if len(shape) == 1 else shape[1]) as w:
        for lo, hi in ((0, 1), (1, 1), (1, 300), (300, shape[0])):
            w.write(x[lo:hi])
    assert w.frames == shape[0]
    assert (tmp_path / "pieces.wav").read_bytes() == (tmp_path / "whole.wav").read_bytes()
    with pytest.raises(ValueError, match="channels"):
        WavWriter(str(tmp_path / "bad.wav"), 48000).write(np.zeros((4, 2), dtype=np.float32))


@pytest.mark.parametrize("bad", (["--resample", "kaiser_fast"], ["--peak", "0.5"], ["--walk", "100"]), ids=lambda b: b[0])
def test_stream_refuses_what_needs_the_whole_signal_and_names_the_option(script, tmp_path, monkeypatch, bad):
    monkeypatch.setattr("sys.argv", ["auralize.py", "--rirs", str(tmp_path), "--dry", str(tmp_path / "dry.wav"), "--out", str(tmp_path / "out"),
                                     "--stream"] + bad)
    with pytest.raises(SystemExit) as e:
        script.main()
    assert "--stream" in str(e.value) and bad[0] in str(e.value)
    assert not (tmp_path / "out").exists()

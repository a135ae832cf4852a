"""The entry points of csrc/resample.hip without a GPU: exported, declared in include/unetrir.h, bound in _lib and wrapped in ops; the
supported range; the host table builder (csrc/resample_table.h) against the fp64 restatement of tests/resample_ref.py, entry by entry,
and as a stand-alone program under the host sanitizers; every bad argument of the kernel's entry point refused with UNETRIR_EINVAL
(10001) before the device is touched (the pointers are the non-null dummy 16, or null); the Python gates on CPU tensors; and
`read_wav(resample=)` as far as it goes without a device."""
import math
import os
import subprocess

import numpy as np
import pytest

import resample_ref as RR
from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
NEW = ["unetrir_resample_supported", "unetrir_resample_taps", "unetrir_resample_out_length", "unetrir_resample_table_f32",
       "unetrir_resample_f32"]
P = 16          # a dummy device pointer
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)
RATIOS = [(2, 1), (1, 2), (3, 2), (2, 3), (7, 3), (3, 7), (160, 147), (147, 160), (441, 1280)]
ZEROS = (1, 2, 16, 64)
SHAPES = [RR.PRESETS["kaiser_best"][1:], RR.PRESETS["kaiser_fast"][1:]]


@pytest.fixture(scope="module")
def lib():
    import unet_rir_amd
    return unet_rir_amd._lib.lib()


def test_new_symbols_are_exported_declared_bound_and_wrapped(lib):
    import unet_rir_amd as U
    declared = declared_symbols()
    for n in NEW:
        assert n in declared and n in U._lib.EXPORTS and hasattr(lib, n), n
    for n in ("resample_supported", "resample_taps", "resample_out_length", "resample_table", "resample_f32"):
        assert callable(getattr(U.ops, n)), n
    assert "resample.hip" in U.build.SOURCES
    assert lib.unetrir_abi_version() == 1
    assert "Resampler" in U.__all__ and "resample" in U.__all__ and callable(U.resample) and callable(U.Resampler)
    import ctypes as C
    assert U._lib._EXCEPTIONS[("unetrir_resample_table_f32", "table")] is C.POINTER(C.c_float)          # a host array


def test_supported_range(lib):
    import unet_rir_amd as U
    largest = 0
    for res_type, (zeros, _, _) in RR.PRESETS.items():
        for a in RATES:
            for b in RATES:
                if a == b:
                    continue
                g = math.gcd(a, b)
                L, M = b // g, a // g
                assert lib.unetrir_resample_supported(L, M, zeros) == 1, (a, b, res_type)
                T = lib.unetrir_resample_taps(L, M, zeros)
                assert T == RR.taps(L, M, zeros) and T % 2 == 0 and U.ops.resample_taps(L, M, zeros) == T
                largest = max(largest, L * T)
    assert largest == 164052                                                # 32000 -> 11025, kaiser_best
    assert lib.unetrir_resample_supported(1, 1, 64) == 1 and lib.unetrir_resample_taps(1, 1, 64) == 128
    for L, M, zeros in ((4, 2, 16), (6, 3, 16), (0, 1, 16), (1, 0, 16), (-3, 2, 16), (3, -2, 16), (3, 2, 0), (3, 2, -1), (2049, 1, 16),
                        (1, 2049, 16), (3, 2, 65), (1, 2048, 3), (1, 2048, 64), (3, 2047, 7)):
        assert lib.unetrir_resample_supported(L, M, zeros) == 0, (L, M, zeros)          # the last three: T = 12288, 262144 and 9554
        assert lib.unetrir_resample_taps(L, M, zeros) == 0 and U.ops.resample_supported(L, M, zeros) is False
    # with L, M <= 2048 and zeros <= 64 the table stays below L T = 2 (64 x 2048 + 2048) < 2^20: that limit is reached through the T of
    # unetrir_resample_f32 alone (BAD below), and the largest tables there are are taken
    assert lib.unetrir_resample_supported(2048, 2047, 64) == 1 and lib.unetrir_resample_taps(2048, 2047, 64) == 128
    assert lib.unetrir_resample_supported(2047, 2048, 64) == 1 and lib.unetrir_resample_taps(2047, 2048, 64) == 130


def test_out_length(lib):
    import unet_rir_amd as U
    for N in (1, 2, 146, 147, 148, 1000, 480000, 1 << 40):
        for L, M in RATIOS:
            assert lib.unetrir_resample_out_length(N, L, M) == RR.out_length(N, L, M) == U.ops.resample_out_length(N, L, M)
    for N, L, M in ((0, 1, 1), (-1, 1, 1), (5, 0, 1), (5, 1, 0), ((1 << 63) - 1, 2048, 1)):
        assert lib.unetrir_resample_out_length(N, L, M) == 0


CASES = [(L, M, z) for L, M in RATIOS for z in ZEROS]


@pytest.mark.parametrize("L,M,zeros", CASES, ids=[f"{L}-{M}-z{z}" for L, M, z in CASES])
def test_table_builder_against_the_restatement(L, M, zeros):
    """Every entry within one fp32 rounding (2^-24 |ref|) plus what two fp64 evaluations of the formula can differ by (1e-13), and
    exactly 0 where the reference is 0"""
    import unet_rir_amd as U
    for rolloff, beta in SHAPES:
        got = U.ops.resample_table(L, M, zeros, rolloff, beta)
        assert got.dtype.is_floating_point and got.element_size() == 4 and not got.is_cuda
        ref = RR.table_ref(L, M, zeros, rolloff, beta)
        assert tuple(got.shape) == ref.shape == (L, RR.taps(L, M, zeros))
        g = got.numpy().astype(np.float64)
        bad = np.argwhere(np.abs(g - ref) > 2.0 ** -24 * np.abs(ref) + 1e-13)
        assert bad.size == 0, (bad[:4], g[tuple(bad[:4].T)], ref[tuple(bad[:4].T)])
        assert np.all(g[ref == 0.0] == 0.0) and np.all(g[ref != 0.0] != 0.0)


def test_table_builder_refuses_bad_arguments(lib):
    import ctypes as C
    import unet_rir_amd as U
    buf = (C.c_float * 64)(*([7.0] * 64))
    for L, M, zeros, rolloff, beta in ((4, 2, 1, 0.85, 8.0), (3, 2, 65, 0.85, 8.0), (3, 2, 1, 0.0, 8.0), (3, 2, 1, 1.0001, 8.0),
                                       (3, 2, 1, 0.85, -0.5), (3, 2, 1, 0.85, 32.5), (3, 2, 1, float("nan"), 8.0)):
        assert lib.unetrir_resample_table_f32(buf, L, M, zeros, rolloff, beta) == EINVAL
    assert lib.unetrir_resample_table_f32(None, 3, 2, 1, 0.85, 8.0) == EINVAL
    assert all(v == 7.0 for v in buf)
    assert lib.unetrir_resample_table_f32(buf, 3, 2, 1, 1.0, 0.0) == 0 and buf[6] == 7.0 and buf[0] != 7.0      # [3][2] and no more
    with pytest.raises(ValueError, match="L = 4, M = 2"):
        U.ops.resample_table(4, 2, 16, 0.85, 8.0)
    with pytest.raises(ValueError, match="rolloff"):
        U.ops.resample_table(3, 2, 16, 1.5, 8.0)


def _checksum(t):
    bits = np.ascontiguousarray(t).view(np.uint32).ravel().astype(np.uint64)
    with np.errstate(over="ignore"):
        return int((bits * np.arange(1, bits.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_table_builder_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/probe/resample_table_main.cpp: the header compiled host-only (no device code, no HIP call) with the sanitizers, run as a
    child process of its own, tables in heap blocks of exactly L T floats.  Exit status 0, and every table it printed a checksum of has
    the library's bits."""
    import unet_rir_amd as U
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "resample_table_main")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-O1", "-g", "-std=c++17", "-I", U.build.CSRC, os.path.join(ROOT, "tests", "probe", "resample_table_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["ok", ""] and len(lines) - 2 == len(RATIOS) * len(ZEROS) * len(SHAPES)
    seen = set()
    for line in lines[:-2]:
        L, M, zeros, T, rolloff, beta, want = line.split()
        L, M, zeros = int(L), int(M), int(zeros)
        table = U.ops.resample_table(L, M, zeros, float(rolloff), float(beta))
        assert table.shape[1] == int(T) and _checksum(table.numpy()) == int(want), line
        seen.add((L, M, zeros, (float(rolloff), float(beta))))
    assert seen == {(L, M, z, s) for L, M in RATIOS for z in ZEROS for s in SHAPES}


def _call(lib, **kw):
    a = dict(x=P, table=P, out=P, B=3, N=1000, L=160, M=147, T=128, Nout=1089)
    a.update(kw)
    return lib.unetrir_resample_f32(a["x"], a["table"], a["out"], a["B"], a["N"], a["L"], a["M"], a["T"], a["Nout"], None)


BAD = [dict(x=None), dict(table=None), dict(out=None), dict(x=None, table=None, out=None),
       dict(B=0), dict(B=-1), dict(N=0), dict(N=-1), dict(Nout=0), dict(Nout=-1), dict(Nout=1090), dict(N=1, Nout=3),
       dict(T=127), dict(T=1), dict(T=0), dict(T=-2), dict(T=8194), dict(L=2048, M=2047, T=514),
       dict(L=320, M=294), dict(L=0), dict(M=0), dict(L=-160), dict(M=-147), dict(L=2049, M=1), dict(L=1, M=2049, Nout=1),
       dict(N=(1 << 62), Nout=1), dict(N=(1 << 50), Nout=1), dict(B=(1 << 31) - 1, N=(1 << 40), Nout=1)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_every_bad_argument_is_refused_before_the_device(lib, bad):
    assert _call(lib, **bad) == EINVAL
    null = dict(x=None, table=None, out=None)
    null.update(bad)
    assert _call(lib, **null) == EINVAL                 # and with null device pointers


def test_the_python_gates_check_their_arguments_before_the_launch():
    import torch
    import unet_rir_amd as U
    x, table, out = torch.zeros(3, 1000), torch.zeros(160, 128), torch.zeros(3, 1089)
    f = U.ops.resample_f32
    for args, word in (((x, table, 160, 147, out), "CUDA"),
                       ((x.double(), table, 160, 147, out), "float32"), ((x, table.half(), 160, 147, out), "float32"),
                       ((x, table, 160, 147, out.int()), "float32"),
                       ((torch.zeros(1000, 3).t(), table, 160, 147, out), "contiguous"),
                       ((x, torch.zeros(160, 256)[:, ::2], 160, 147, out), "contiguous"),
                       ((x, table, 160, 147, torch.zeros(1089, 3).t()), "contiguous"),
                       ((x, table, 160, 147, torch.zeros(2, 1089)), "batch"),
                       ((x[0], table, 160, 147, out), r"x \[B, N\]"), ((x, table[0], 160, 147, out), r"table \[L, T\]"),
                       ((x, table, 159, 147, out), "table"), ((x, torch.zeros(160, 127), 160, 147, out), "even"),
                       ((x, table, 160, 147, torch.zeros(3, 1090)), "outside"), ((x, table, 160, 147, torch.zeros(3, 0)), "outside"),
                       ((torch.zeros(3, 0), table, 160, 147, out), "empty"), ((None, table, 160, 147, out), "tensors")):
        with pytest.raises(ValueError, match=word):
            f(*args)
    # Resampler: the constructor's checks come before any device is looked at
    for args, kw, word in (((44100, 48000, "sinc_best"), {}, "res_type"), ((0, 48000), {}, "rate_in"), ((44100, -1), {}, "rate_out"),
                           ((44100.5, 48000), {}, "rate_in"), ((44100, 48000), dict(zeros=65), "zeros = 65"),
                           ((44100, 48000), dict(rolloff=1.5), "rolloff"), ((44100, 48000), dict(beta=40.0), "beta"),
                           ((48000, 48001), {}, r"L = 48001, M = 48000: L = 48001 is beyond the limit of 2048"),
                           ((2048, 1), {}, r"L = 1, M = 2048: T = 262144 is beyond the limit of 8192"),
                           ((44100, 48000), dict(device="cpu"), "CUDA")):
        with pytest.raises(ValueError, match=word):
            U.Resampler(*args, **kw)
    with pytest.raises(ValueError, match="CUDA"):
        U.resample(torch.zeros(100), 44100, 48000)
    r = U.Resampler(48000, 48000, device="cuda")                     # equal rates: no table, no launch, a copy
    assert (r.L, r.M, r.table) == (1, 1, None) and r.out_length(77) == 77
    src = torch.arange(12, dtype=torch.float32).reshape(2, 6)
    got = r(src)
    assert torch.equal(got, src) and got.data_ptr() != src.data_ptr() and torch.equal(r(src, length=4), src[:, :4])
    assert U.Resampler.out_length(type("R", (), dict(L=160, M=147))(), 1000) == 1089


def _write_pcm16(path, rate, samples):
    import wave
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(np.asarray(samples, dtype="<i2").tobytes())


def test_read_wav_with_and_without_resample(tmp_path):
    import torch
    import unet_rir_amd as U
    from unet_rir_amd.auralize import write_wav
    rng = np.random.default_rng(5)
    pcm = rng.integers(-20000, 20000, size=9600)
    p48, pf = tmp_path / "a48.wav", tmp_path / "f48.wav"
    _write_pcm16(p48, 48000, pcm)
    write_wav(str(pf), rng.uniform(-1, 1, size=(9600, 2)).astype(np.float32), 48000)
    for p in (p48, pf):
        with pytest.raises(ValueError, match="48000 Hz, expected 44100 Hz"):
            U.read_wav(str(p), 44100, 0.1)                                          # resample=None: today's behaviour, the error included
        with pytest.raises(ValueError, match="resample"):
            U.read_wav(str(p), 44100, 0.1, resample="sinc")
        if not torch.cuda.is_available():
            with pytest.raises(ValueError, match="CUDA device"):
                U.read_wav(str(p), 44100, 0.1, resample="kaiser_best")
        base = U.read_wav(str(p), 48000, 0.2)                                       # a file at the asked rate: the old path, bit for bit
        for mode in ("kaiser_best", "kaiser_fast"):
            assert np.array_equal(U.read_wav(str(p), 48000, 0.2, resample=mode), base)
            assert np.array_equal(U.read_wav(str(p), 48000, 0.1, True, mode), U.read_wav(str(p), 48000, 0.1))
        with pytest.raises(ValueError, match="shorter"):
            U.read_wav(str(p), 48000, 0.3, resample="kaiser_best")
    x = pcm.astype(np.float32) * np.float32(2.0 ** -15)
    want = x - np.mean(x)
    assert np.array_equal(U.read_wav(str(p48), 48000, 0.2), want)
    both = U.read_wav(str(pf), 48000, 0.2, mono=False, resample="kaiser_fast")
    assert both.shape == (2, 9600) and np.array_equal(both, U.read_wav(str(pf), 48000, 0.2, mono=False))
    with pytest.raises(ValueError, match="resample"):
        U.Dataset(str(tmp_path), "none", resample="sinc")

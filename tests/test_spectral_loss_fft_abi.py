"""The entry points of csrc/spectralloss_fft.hip are exported, declared in include/unetrir.h, bound in _lib and wrapped in ops, and refuse
every bad argument with UNETRIR_EINVAL (10001) before the device is touched - checked here without a GPU: the pointers are the
non-null, 16-byte aligned dummy 16, so only the argument checks stand between the call and a launch."""
import ctypes as C
import math

import pytest

from test_abi import declared_symbols

EINVAL = 10001
NEW = ["unetrir_spectral_loss_fft_supported", "unetrir_spectral_loss_fft_ws_bytes", "unetrir_spectral_loss_fft_f32"]
P = 16          # a dummy device pointer
DEFAULT = ((128, 64, 32), (512, 256, 128), (1024, 512, 256))


@pytest.fixture(scope="module")
def L():
    import unet_rir_amd
    return unet_rir_amd._lib.lib()


def arr(res):
    return None if res is None else (C.c_int * (3 * len(res)))(*[v for r in res for v in r])


def test_new_symbols_are_exported_declared_bound_and_wrapped(L):
    import unet_rir_amd as U
    declared = declared_symbols()
    for n in NEW:
        assert n in declared and n in U._lib.EXPORTS and hasattr(L, n), n
    for n in ("spectral_loss_fft_ws_bytes", "spectral_loss_fft_supported", "spectral_loss_fft"):
        assert callable(getattr(U.ops, n)), n
    assert "spectralloss_fft.hip" in U.build.SOURCES and "spectralloss.hip" in U.build.SOURCES
    assert len(U._lib.Config._fields_) == 18 and L.unetrir_abi_version() == 1


def test_the_supported_predicate_at_each_edge(L):
    s = L.unetrir_spectral_loss_fft_supported
    assert [s(9600, n, 8, 4) for n in (64, 96, 128, 256, 512, 1024, 2048, 130, 127, 0, -128)] == [0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert [s(9600, 256, w, 64) for w in (1, 2, 256, 257, 0, -4)] == [0, 1, 1, 0, 0, 0]
    assert [s(9600, 256, 128, h) for h in (0, 1, -1, 9600, 1 << 20)] == [0, 1, 0, 1, 1]
    assert [s(T, 256, 128, 64) for T in (128, 129, 16384, 16385, 0, -1)] == [0, 1, 1, 0, 0, 0]
    assert [s(T, 128, 128, 32) for T in (64, 65)] == [0, 1]
    assert [s(T, 1024, 512, 256) for T in (512, 513)] == [0, 1]
    # everything this form takes, the DFT form takes
    d = L.unetrir_spectral_loss_supported
    assert all(d(T, n, w, h) for T, n, w, h in ((65, 128, 128, 32), (16384, 1024, 2, 1), (129, 256, 256, 1 << 20)) if s(T, n, w, h))


def ws_bytes(B, T, res):
    """fp64: a slab of three sums per workgroup of 2048 / n_fft frames, SC / LM and the two gradient scalars per (row, resolution), three
    figures per row; fp32: the windowed frames F win; to a multiple of 8 bytes"""
    doubles, floats = 3, 0
    for n, w, h in res:
        F = 1 + T // h
        doubles += 3 * (-(-F // (2048 // n))) + 4
        floats += F * w
    return 8 * B * doubles + 8 * (-(-(4 * B * floats) // 8))


def test_workspace_size(L):
    for B, T, res in ((1, 65, ((128, 128, 32),)), (3, 1000, ((128, 64, 16), (256, 100, 37))), (32, 9600, DEFAULT), (2, 16384, ((512, 256, 128),)),
                      (1, 100, ((128, 7, 3),))):
        assert L.unetrir_spectral_loss_fft_ws_bytes(B, T, len(res), arr(res)) == ws_bytes(B, T, res)
    # no spectra in memory: a tenth of the DFT form's at the flagship shape
    assert 10 * ws_bytes(32, 9600, DEFAULT) <= L.unetrir_spectral_loss_ws_bytes(32, 9600, 3, arr(DEFAULT))
    ok = ((256, 128, 64),)
    assert L.unetrir_spectral_loss_fft_ws_bytes(2, 9600, 1, arr(ok)) > 0
    for B, T, R, res in ((0, 9600, 1, ok), (-1, 9600, 1, ok), (2, 128, 1, ok), (2, 16385, 1, ok), (2, 9600, 0, ok), (2, 9600, 9, ok * 9),
                         (2, 9600, 1, None), (2, 9600, 1, ((64, 8, 4),)), (2, 9600, 1, ((2048, 8, 4),)), (2, 9600, 1, ((96, 8, 4),)),
                         (2, 9600, 1, ((256, 1, 4),)), (2, 9600, 1, ((256, 257, 4),)), (2, 9600, 1, ((256, 128, 0),)),
                         (2, 9600, 2, ok + ((256, 257, 4),)), (2, 500, 2, ok + ((1024, 512, 256),)), (2, 9600, 2, ok + ((64, 64, 16),))):
        assert L.unetrir_spectral_loss_fft_ws_bytes(B, T, R, arr(res)) == 0, (B, T, R, res)


def _call(L, **kw):
    a = dict(wav_pred=P, wav_true=P, B=2, T=9600, R=3, res=DEFAULT, floor_db=60.0, scw=1.0, lw=1.0, weight=1.0, inv_gb=0.5, accumulate=0,
             dwav=P, out=P, loss_out=None, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(L.unetrir_spectral_loss_fft_ws_bytes(2, 9600, 3, arr(DEFAULT)), 1)
    return L.unetrir_spectral_loss_fft_f32(a["wav_pred"], a["wav_true"], a["B"], a["T"], a["R"], arr(a["res"]), a["floor_db"], a["scw"],
                                           a["lw"], a["weight"], a["inv_gb"], a["accumulate"], a["dwav"], a["out"], a["loss_out"], a["ws"],
                                           a["ws_bytes"], None)


BAD = [dict(wav_pred=None), dict(wav_true=None), dict(out=None), dict(ws=None), dict(res=None), dict(B=0), dict(B=-3), dict(R=0), dict(R=-1),
       dict(R=9, res=DEFAULT * 3), dict(T=0), dict(T=512), dict(T=16385), dict(R=1, res=((64, 8, 4),)), dict(R=1, res=((2048, 512, 256),)),
       dict(R=1, res=((96, 64, 32),)), dict(R=1, res=((16, 16, 4),)), dict(R=1, res=((256, 1, 64),)), dict(R=1, res=((256, 257, 64),)),
       dict(R=1, res=((256, 128, 0),)), dict(R=2, res=((256, 128, 64), (256, 128, -1))), dict(R=2, res=((256, 128, 64), (64, 64, 16))),
       dict(floor_db=0.0), dict(floor_db=-60.0), dict(floor_db=200.5), dict(floor_db=math.inf), dict(floor_db=math.nan), dict(scw=-1.0),
       dict(scw=math.inf), dict(scw=math.nan), dict(lw=-1.0), dict(lw=math.inf), dict(lw=math.nan), dict(weight=-1.0), dict(weight=math.inf),
       dict(weight=math.nan), dict(inv_gb=0.0), dict(inv_gb=-0.5), dict(inv_gb=math.inf), dict(inv_gb=math.nan),
       dict(accumulate=1, dwav=None), dict(ws_bytes=0), dict(ws_bytes=-1), dict(ws=20)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_spectral_loss_fft_refuses_every_bad_argument_before_the_device(L, bad):
    if bad.get("ws_bytes") == -1:
        bad = dict(ws_bytes=L.unetrir_spectral_loss_fft_ws_bytes(2, 9600, 3, arr(DEFAULT)) - 1)
    assert _call(L, **bad) == EINVAL


def test_the_wrappers_and_the_method_argument():
    """the op raises on CPU tensors before the library is asked; method is a keyword, "dft" by default, and "fft" refuses in the
    constructor what the predicate refuses, naming the resolution and the form that takes it"""
    import inspect
    import torch
    import unet_rir_amd as U
    with pytest.raises(ValueError):
        U.ops.spectral_loss_fft(torch.zeros(2, 320), torch.zeros(2, 320), torch.zeros(3, dtype=torch.float64), None, ((128, 64, 32),))
    with pytest.raises(ValueError):
        U.ops.spectral_loss_fft_ws_bytes(2, 320, ())
    with pytest.raises(ValueError):
        U.ops.spectral_loss_fft_ws_bytes(2, 320, ((128, 64),))
    assert U.ops.spectral_loss_fft_supported(320, 128, 64, 32) and not U.ops.spectral_loss_fft_supported(320, 64, 64, 16)
    assert U.ops.spectral_loss_fft_ws_bytes(2, 320, ((128, 64, 32),)) == ws_bytes(2, 320, ((128, 64, 32),))
    params = list(inspect.signature(U.SpectralLoss.__init__).parameters.values())
    assert params[-1].name == "method" and params[-1].kind is inspect.Parameter.KEYWORD_ONLY and params[-1].default == "dft"
    assert U.SpectralLoss().method == "dft" and U.SpectralLoss(method="fft").method == "fft"
    for bad in ("FFT", "", None, "rfft"):
        with pytest.raises(ValueError, match="method"):
            U.SpectralLoss(method=bad)
    small = dict(des_shape=(17, 41), n_fft=32, win_length=16, hop_length=8)                  # T = 320
    assert U.SpectralLoss(resolutions=((64, 32, 16), (128, 128, 32)), **small).method == "dft"
    with pytest.raises(ValueError, match=r'\(64, 32, 16\).*method="dft"'):
        U.SpectralLoss(resolutions=((128, 128, 32), (64, 32, 16)), method="fft", **small)
    with pytest.raises(ValueError, match=r'\(1024, 512, 256\).*method="dft"'):                # T = 320 < 513
        U.SpectralLoss(method="fft", **small)
    with pytest.raises(ValueError, match=r'\(96, 64, 32\).*method="dft"'):
        U.SpectralLoss(resolutions=((96, 64, 32),), method="fft")
    assert U.SpectralLoss(resolutions=((128, 128, 32), (256, 100, 37)), method="fft", **small).T == 320

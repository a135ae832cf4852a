"""The entry points of csrc/spectralloss.hip are exported, declared in include/unetrir.h, bound in _lib and wrapped in ops, and refuse
every bad argument with UNETRIR_EINVAL (10001) before the device is touched - checked here without a GPU: the pointers are the
non-null, 16-byte aligned dummy 16, so only the argument checks stand between the call and a launch."""
import ctypes as C
import math

import pytest

from test_abi import declared_symbols

EINVAL = 10001
NEW = ["unetrir_spectral_loss_supported", "unetrir_spectral_loss_ws_bytes", "unetrir_spectral_loss_f32"]
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
    for n in ("spectral_loss_ws_bytes", "spectral_loss_supported", "spectral_loss"):
        assert callable(getattr(U.ops, n)), n
    assert "spectralloss.hip" in U.build.SOURCES
    assert len(U._lib.Config._fields_) == 18 and L.unetrir_abi_version() == 1
    assert "SpectralLoss" in U.__all__ and U.SpectralLoss is not None


def test_the_supported_predicate_at_each_edge(L):
    s = L.unetrir_spectral_loss_supported
    assert [s(9600, n, 8, 4) for n in (14, 16, 1024, 1026, 17, 255)] == [0, 1, 1, 0, 0, 0]
    assert [s(9600, 256, w, 64) for w in (1, 2, 256, 257, 0, -4)] == [0, 1, 1, 0, 0, 0]
    assert [s(9600, 256, 128, h) for h in (0, 1, -1, 9600, 1 << 20)] == [0, 1, 0, 1, 1]
    assert [s(T, 256, 128, 64) for T in (128, 129, 16384, 16385, 0, -1)] == [0, 1, 1, 0, 0, 0]
    assert [s(T, 16, 16, 4) for T in (8, 9)] == [0, 1]
    assert [s(T, 1024, 512, 256) for T in (512, 513)] == [0, 1]


def ws_doubles(B, T, res):
    """slabs (3 per tile of 16 frames x 64 of the n_fft / 2 bin columns), SC / LM and the two gradient scalars per (row, resolution),
    three figures per row, four planes of F K per resolution, the windowed frames F win"""
    per_row = 3
    for n, w, h in res:
        F, K = 1 + T // h, n // 2 + 1
        per_row += 3 * (-(-F // 16)) * (-(-(n // 2) // 64)) + 4 + 4 * F * K + F * w
    return B * per_row


def test_workspace_size(L):
    for B, T, res in ((1, 9, ((16, 16, 4),)), (3, 1000, ((64, 64, 16), (256, 100, 37))), (32, 9600, DEFAULT), (2, 16384, ((512, 256, 128),))):
        assert L.unetrir_spectral_loss_ws_bytes(B, T, len(res), arr(res)) == 8 * ws_doubles(B, T, res)
    ok = ((256, 128, 64),)
    assert L.unetrir_spectral_loss_ws_bytes(2, 9600, 1, arr(ok)) > 0
    for B, T, R, res in ((0, 9600, 1, ok), (-1, 9600, 1, ok), (2, 128, 1, ok), (2, 16385, 1, ok), (2, 9600, 0, ok), (2, 9600, 9, ok * 9),
                         (2, 9600, 1, None), (2, 9600, 1, ((14, 8, 4),)), (2, 9600, 1, ((1026, 8, 4),)), (2, 9600, 1, ((255, 8, 4),)),
                         (2, 9600, 1, ((256, 1, 4),)), (2, 9600, 1, ((256, 257, 4),)), (2, 9600, 1, ((256, 128, 0),)),
                         (2, 9600, 2, ok + ((256, 257, 4),)), (2, 500, 2, ok + ((1024, 512, 256),))):
        assert L.unetrir_spectral_loss_ws_bytes(B, T, R, arr(res)) == 0, (B, T, R, res)


def _call(L, **kw):
    a = dict(wav_pred=P, wav_true=P, B=2, T=9600, R=3, res=DEFAULT, floor_db=60.0, scw=1.0, lw=1.0, weight=1.0, inv_gb=0.5, accumulate=0,
             dwav=P, out=P, loss_out=None, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(L.unetrir_spectral_loss_ws_bytes(2, 9600, 3, arr(DEFAULT)), 1)
    return L.unetrir_spectral_loss_f32(a["wav_pred"], a["wav_true"], a["B"], a["T"], a["R"], arr(a["res"]), a["floor_db"], a["scw"], a["lw"],
                                       a["weight"], a["inv_gb"], a["accumulate"], a["dwav"], a["out"], a["loss_out"], a["ws"],
                                       a["ws_bytes"], None)


BAD = [dict(wav_pred=None), dict(wav_true=None), dict(out=None), dict(ws=None), dict(res=None), dict(B=0), dict(B=-3), dict(R=0), dict(R=-1),
       dict(R=9, res=DEFAULT * 3), dict(T=0), dict(T=512), dict(T=16385), dict(R=1, res=((14, 8, 4),)), dict(R=1, res=((1026, 512, 256),)),
       dict(R=1, res=((255, 128, 64),)), dict(R=1, res=((256, 1, 64),)), dict(R=1, res=((256, 257, 64),)), dict(R=1, res=((256, 128, 0),)),
       dict(R=2, res=((256, 128, 64), (256, 128, -1))), dict(floor_db=0.0), dict(floor_db=-60.0), dict(floor_db=200.5),
       dict(floor_db=math.inf), dict(floor_db=math.nan), dict(scw=-1.0), dict(scw=math.inf), dict(scw=math.nan), dict(lw=-1.0),
       dict(lw=math.inf), dict(lw=math.nan), dict(weight=-1.0), dict(weight=math.inf), dict(weight=math.nan), dict(inv_gb=0.0),
       dict(inv_gb=-0.5), dict(inv_gb=math.inf), dict(inv_gb=math.nan), dict(accumulate=1, dwav=None), dict(ws_bytes=0), dict(ws_bytes=-1),
       dict(ws=20)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_spectral_loss_refuses_every_bad_argument_before_the_device(L, bad):
    if bad.get("ws_bytes") == -1:
        bad = dict(ws_bytes=L.unetrir_spectral_loss_ws_bytes(2, 9600, 3, arr(DEFAULT)) - 1)
    assert _call(L, **bad) == EINVAL


def test_the_wrappers_check_their_arguments_first():
    """the op raises on CPU tensors and wrong shapes before the library is asked; the constructor mirrors DecayLoss's checks"""
    import torch
    import unet_rir_amd as U
    with pytest.raises(ValueError):
        U.ops.spectral_loss(torch.zeros(2, 320), torch.zeros(2, 320), torch.zeros(3, dtype=torch.float64), None, ((32, 16, 8),))
    with pytest.raises(ValueError):
        U.ops.spectral_loss_ws_bytes(2, 320, ())
    with pytest.raises(ValueError):
        U.ops.spectral_loss_ws_bytes(2, 320, ((32, 16),))
    assert U.ops.spectral_loss_supported(320, 32, 16, 8) and not U.ops.spectral_loss_supported(16, 32, 16, 8)
    for kw in (dict(weight=-1.0), dict(weight=math.inf), dict(weight=math.nan), dict(sc_weight=-1.0), dict(log_weight=math.nan),
               dict(floor_db=0.0), dict(floor_db=250.0), dict(floor_db=math.nan), dict(resolutions=()), dict(resolutions=((32, 16),)),
               dict(resolutions=((31, 16, 8),)), dict(resolutions=((2048, 16, 8),)), dict(resolutions=((32, 33, 8),)),
               dict(resolutions=((32, 16, 0),)), dict(resolutions=((32, 16, 8),) * 9)):
        with pytest.raises(ValueError):
            U.SpectralLoss(**kw)
    sl = U.SpectralLoss(weight=0.5, floor_db=45.0, des_shape=(17, 41), n_fft=32, win_length=16, hop_length=8, resolutions=((16, 16, 4),))
    assert (sl.T, sl.weight, sl.sc_weight, sl.log_weight, sl.floor_db, sl.spectral_out) == (320, 0.5, 1.0, 1.0, 45.0, None)
    assert U.SpectralLoss().resolutions == DEFAULT and (256, 128, 64) not in U.SpectralLoss().resolutions

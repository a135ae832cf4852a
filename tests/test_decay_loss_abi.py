"""The entry points of csrc/decayloss.hip and csrc/istft_bwd.hip are exported, declared in include/unetrir.h, bound in _lib and wrapped
in ops, and refuse every bad argument with UNETRIR_EINVAL (10001) before the device is touched - checked here without a GPU: the
pointers are the non-null, 16-byte aligned dummy 16, so only the argument checks stand between the call and a launch."""
import math

import pytest

from test_abi import declared_symbols

EINVAL = 10001
NEW = ["unetrir_istft_features_bwd_f32", "unetrir_decay_loss_ws_bytes", "unetrir_decay_loss_supported", "unetrir_decay_loss_f32"]
P = 16          # a dummy device pointer


@pytest.fixture(scope="module")
def L():
    import unet_rir_amd
    return unet_rir_amd._lib.lib()


def test_new_symbols_are_exported_declared_bound_and_wrapped(L):
    import unet_rir_amd as U
    declared = declared_symbols()
    for n in NEW:
        assert n in declared and n in U._lib.EXPORTS and hasattr(L, n), n
    for n in ("istft_features_bwd", "decay_loss_ws_bytes", "decay_loss_supported", "decay_loss"):
        assert callable(getattr(U.ops, n)), n
    assert "decayloss.hip" in U.build.SOURCES and "istft_bwd.hip" in U.build.SOURCES
    assert len(U._lib.Config._fields_) == 18 and L.unetrir_abi_version() == 1
    assert "DecayLoss" in U.__all__ and U.DecayLoss is not None
    assert callable(U.features.PostProcess.differentiable)


def test_supported_lengths_and_workspace_size(L):
    """one (Q_b, counted) pair of fp64 per row"""
    for T in (1, 2, 64, 9600, 16384):
        assert L.unetrir_decay_loss_supported(T) == 1
    for T in (0, -1, -2 ** 31):
        assert L.unetrir_decay_loss_supported(T) == 0
    for B, T in ((1, 1), (3, 9600), (32, 9600), (65536, 16384)):
        assert L.unetrir_decay_loss_ws_bytes(B, T) == 16 * B
    for B, T in ((0, 9600), (-1, 9600), (2, 0), (2, -5)):
        assert L.unetrir_decay_loss_ws_bytes(B, T) == 0
    for T in (16385, 1 << 20, 2 ** 31 - 1):          # whatever a build supports, the two functions agree
        assert (L.unetrir_decay_loss_ws_bytes(2, T) == 32) == bool(L.unetrir_decay_loss_supported(T))


def _decay(L, **kw):
    a = dict(wav_pred=P, wav_true=P, B=2, T=9600, floor_db=60.0, weight=1.0, inv_gb=0.5, dwav=P, decay_out=P, loss_out=None, ws=P,
             ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(L.unetrir_decay_loss_ws_bytes(2, 9600), 1)
    return L.unetrir_decay_loss_f32(a["wav_pred"], a["wav_true"], a["B"], a["T"], a["floor_db"], a["weight"], a["inv_gb"], a["dwav"],
                                    a["decay_out"], a["loss_out"], a["ws"], a["ws_bytes"], None)


def _unsupported_T(L):
    T = 16385
    while L.unetrir_decay_loss_supported(T) and T < 2 ** 30:
        T *= 2
    return T


BAD_DECAY = [dict(wav_pred=None), dict(wav_true=None), dict(decay_out=None), dict(ws=None), dict(B=0), dict(B=-3), dict(T=0), dict(T=-1),
             dict(T="unsupported"), dict(floor_db=0.0), dict(floor_db=-60.0), dict(floor_db=200.5), dict(floor_db=math.inf),
             dict(floor_db=math.nan), dict(weight=-1.0), dict(weight=math.inf), dict(weight=math.nan), dict(inv_gb=0.0), dict(inv_gb=-0.5),
             dict(inv_gb=math.inf), dict(inv_gb=math.nan), dict(ws_bytes=0), dict(ws_bytes=-1), dict(ws=20)]


@pytest.mark.parametrize("bad", BAD_DECAY, ids=[str(b) for b in BAD_DECAY])
def test_decay_loss_refuses_every_bad_argument_before_the_device(L, bad):
    if bad.get("ws_bytes") == -1:
        bad = dict(ws_bytes=L.unetrir_decay_loss_ws_bytes(2, 9600) - 1)
    if bad.get("T") == "unsupported":
        bad = dict(T=_unsupported_T(L))
        assert not L.unetrir_decay_loss_supported(bad["T"])
    assert _decay(L, **bad) == EINVAL


def _vjp(L, **kw):
    a = dict(pred=P, phase_ref=None, dwav=P, B=2, H=144, W=160, n_bins=129, n_frames=151, n_fft=256, win=128, hop=64, accumulate=0, dpred=P)
    a.update(kw)
    return L.unetrir_istft_features_bwd_f32(a["pred"], a["phase_ref"], a["dwav"], a["B"], a["H"], a["W"], a["n_bins"], a["n_frames"],
                                            a["n_fft"], a["win"], a["hop"], a["accumulate"], a["dpred"], None)


# the geometry rules of unetrir_wave_loss_f32 (tests/test_wave_loss_abi.py) and the three pointers
BAD_VJP = [dict(pred=None), dict(dwav=None), dict(dpred=None), dict(B=0), dict(B=65536), dict(n_fft=96, n_bins=49),
           dict(n_fft=2048, n_bins=1025, H=1040), dict(n_fft=2, n_bins=2), dict(win=0), dict(win=257), dict(hop=0), dict(n_bins=128),
           dict(n_bins=130), dict(H=128), dict(n_frames=1), dict(n_frames=161), dict(hop=1 << 24, n_frames=160)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("bad", BAD_VJP, ids=[str(b) for b in BAD_VJP])
def test_the_vjp_refuses_every_bad_argument_before_the_device(L, bad, accumulate):
    assert _vjp(L, accumulate=accumulate, **bad) == EINVAL


def test_the_wrappers_check_their_arguments_first():
    """the ops raise on CPU tensors and wrong shapes before the library is asked; the constructor mirrors WaveLoss's checks"""
    import torch
    import unet_rir_amd as U
    with pytest.raises(ValueError):
        U.ops.decay_loss(torch.zeros(2, 320), torch.zeros(2, 320), torch.zeros(2, dtype=torch.float64), None)
    with pytest.raises(ValueError):
        U.ops.istft_features_bwd(torch.zeros(2, 2, 32, 48), torch.zeros(2, 320), torch.zeros(2, 2, 32, 48), 17, 41, 32, 16, 8)
    for kw in (dict(weight=-1.0), dict(weight=math.inf), dict(weight=math.nan), dict(floor_db=0.0), dict(floor_db=250.0),
               dict(floor_db=math.nan)):
        with pytest.raises(ValueError):
            U.DecayLoss(**kw)
    dl = U.DecayLoss(weight=0.5, floor_db=45.0, des_shape=(17, 41), n_fft=32, win_length=16, hop_length=8)
    assert (dl.T, dl.weight, dl.floor_db, dl.decay_out) == (320, 0.5, 45.0, None)

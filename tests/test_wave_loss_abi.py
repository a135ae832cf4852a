"""The entry points of csrc/waveloss.hip are exported, declared in include/unetrir.h, bound in _lib and wrapped in ops, and refuse every
bad argument with UNETRIR_EINVAL (10001) before the device is touched - checked here without a GPU: the pointers are the non-null,
16-byte aligned dummy 16, so only the argument checks stand between the call and a launch."""
import math

import pytest

from test_abi import declared_symbols

EINVAL = 10001
NEW = ["unetrir_wave_loss_ws_bytes", "unetrir_wave_loss_f32"]
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
    for n in ("wave_loss_ws_bytes", "wave_loss"):
        assert callable(getattr(U.ops, n)), n
    assert "waveloss.hip" in U.build.SOURCES
    assert len(U._lib.Config._fields_) == 18 and L.unetrir_abi_version() == 1
    assert "WaveLoss" in U.__all__ and U.WaveLoss is not None


def _call(L, **kw):
    a = dict(pred=P, phase_ref=None, wav_true=P, time_weight=None, B=2, H=144, W=160, n_bins=129, n_frames=151, n_fft=256, win=128, hop=64,
             norm=0, weight=1.0, inv_gb=0.5, spec_target=None, phase_weight=None, alpha=0.9, inv_norm=1e-5, dpred=P, wav_pred=None,
             wave_out=P, loss_out=None, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(L.unetrir_wave_loss_ws_bytes(2, 151, 64), 1)
    return L.unetrir_wave_loss_f32(a["pred"], a["phase_ref"], a["wav_true"], a["time_weight"], a["B"], a["H"], a["W"], a["n_bins"],
                                   a["n_frames"], a["n_fft"], a["win"], a["hop"], a["norm"], a["weight"], a["inv_gb"], a["spec_target"],
                                   a["phase_weight"], a["alpha"], a["inv_norm"], a["dpred"], a["wav_pred"], a["wave_out"], a["loss_out"],
                                   a["ws"], a["ws_bytes"], None)


def test_workspace_size_is_the_advertised_layout(L):
    """u fp64 [B][T] + two partials per 64-sample segment + one factor per sample"""
    for B, nf, hop in ((2, 151, 64), (32, 151, 64), (1, 30, 7), (3, 3, 8), (65535, 2, 1)):
        T = hop * (nf - 1)
        assert L.unetrir_wave_loss_ws_bytes(B, nf, hop) == 8 * (B * T + 2 * B * -(-T // 64) + B)
    for B, nf, hop in ((0, 151, 64), (65536, 151, 64), (2, 1, 64), (2, 151, 0), (2, 1 << 30, 64)):
        assert L.unetrir_wave_loss_ws_bytes(B, nf, hop) == 0


BAD = [dict(pred=None), dict(wav_true=None), dict(wave_out=None), dict(ws=None),
       dict(B=0), dict(B=65536), dict(n_fft=96, n_bins=49), dict(n_fft=2048, n_bins=1025, H=1040), dict(n_fft=2, n_bins=2), dict(win=0),
       dict(win=257), dict(hop=0), dict(n_bins=128), dict(n_bins=130), dict(H=128), dict(n_frames=1), dict(n_frames=161),
       dict(norm=2), dict(norm=-1), dict(weight=-1.0), dict(weight=math.inf), dict(weight=math.nan), dict(inv_gb=0.0), dict(inv_gb=math.nan),
       dict(ws_bytes=0), dict(ws_bytes=-1), dict(ws=20)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_every_bad_argument_is_refused_before_the_device(L, bad):
    if bad.get("ws_bytes") == -1:
        bad = dict(ws_bytes=L.unetrir_wave_loss_ws_bytes(2, 151, 64) - 1)
    assert _call(L, **bad) == EINVAL


def test_the_wrapper_checks_its_arguments_first():
    """ops.wave_loss raises on a CPU tensor, a wrong norm and a wrong shape before the library is asked."""
    import torch
    import unet_rir_amd as U
    pred = torch.zeros(2, 2, 32, 48)
    with pytest.raises(ValueError):
        U.ops.wave_loss(pred, torch.zeros(2, 320), torch.zeros(2, dtype=torch.float64), None, 17, 41, 32, 16, 8)
    with pytest.raises(ValueError):
        U.WaveLoss(norm="l1")
    with pytest.raises(ValueError):
        U.WaveLoss(weight=-1.0)

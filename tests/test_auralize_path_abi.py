"""The entry points of `auralize_path` (csrc/auralize_fft.hip) are exported, declared in include/unetrir.h, bound in _lib and wrapped in
ops, and refuse every bad argument with UNETRIR_EINVAL (10001) before the device is touched - checked here without a GPU: the pointers
are the non-null dummy 16 (or null where that is the fault), so only the argument checks stand between the call and a launch.  The
python gates - `auralize_path` and `ops.auralize_path_f32` - are checked with CPU tensors."""
import numpy as np
import pytest

from test_abi import declared_symbols

EINVAL = 10001
NEW = ["unetrir_auralize_path_supported", "unetrir_auralize_path_ws_bytes", "unetrir_auralize_path_f32"]
P = 16          # a dummy device pointer, 16-byte aligned
SPEC = 16384    # bytes of one packed spectrum


@pytest.fixture(scope="module")
def lib():
    import unet_rir_amd
    return unet_rir_amd._lib.lib()


def test_new_symbols_are_exported_declared_bound_and_wrapped(lib):
    import unet_rir_amd as U
    declared = declared_symbols()
    for n in NEW:
        assert n in declared and n in U._lib.EXPORTS and hasattr(lib, n), n
    for n in ("auralize_path_supported", "auralize_path_ws_bytes", "auralize_path_f32"):
        assert callable(getattr(U.ops, n)), n
    assert callable(U.auralize_path) and "auralize_path" in U.__all__
    assert lib.unetrir_abi_version() == 1


def test_supported_range(lib):
    import unet_rir_amd as U
    for K, want in ((1, 1), (2048, 1), (9600, 1), (16384, 1), (0, 0), (16385, 0), (-1, 0)):
        assert lib.unetrir_auralize_path_supported(K) == want == lib.unetrir_auralize_fft_supported(K), K
        assert U.ops.auralize_path_supported(K) is bool(want)


def test_workspace_bytes(lib):
    import unet_rir_amd as U
    ws = lib.unetrir_auralize_path_ws_bytes
    # B R Q spectra of h and J (x shared) or B J (x per row) of x
    assert ws(3, 4, 9600, 1000, 0, 10599) == SPEC * (3 * 4 * 5 + 6)
    assert ws(3, 4, 9600, 1000, 1000, 10599) == SPEC * (3 * 4 * 5 + 3 * 6) == U.ops.auralize_path_ws_bytes(3, 4, 9600, 1000, 1000, 10599)
    assert ws(3, 7, 9600, 1000, 1024, 1) == SPEC * (3 * 7 * 5 + 3 * 1)
    assert ws(1, 1, 1, 1, 0, 1) == SPEC * 2
    assert ws(32, 32, 2048, 2049, 0, 2048) == SPEC * (1024 + 1) and ws(32, 2, 2049, 2049, 0, 2049) == SPEC * (128 + 2)
    for B, K, N, stride, L in ((3, 9600, 1000, 0, 10599), (2, 33, 5000, 5000, 5032), (1, 16384, 1, 0, 16384)):      # R = 1: the FFT form's
        assert ws(B, 1, K, N, stride, L) == lib.unetrir_auralize_fft_ws_bytes(B, K, N, stride, L) > 0
    for bad in ((0, 4, 9600, 1000, 0, 10599), (-1, 4, 9600, 1000, 0, 10599), (3, 0, 9600, 1000, 0, 10599), (3, -1, 9600, 1000, 0, 10599),
                (3, 4, 0, 1000, 0, 1), (3, 4, 16385, 1000, 0, 1), (3, 4, 9600, 0, 0, 1), (3, 4, 9600, 1000, 0, 0),
                (3, 4, 9600, 1000, 0, 10600), (3, 4, 9600, 1000, 999, 10599), (3, 4, 9600, 1000, -1, 10599),
                (2147483647, 4, 9600, 1000, 0, 10599), (3, 2147483647, 9600, 1000, 0, 10599), (65536, 65536, 33, 1000, 0, 1000),
                (1 << 20, 1, 9600, 2147483647, 0, 2147483647), (1 << 15, 1 << 14, 16384, 1000, 0, 1000)):
        assert ws(*bad) == 0, bad


def _call(lib, **kw):
    a = dict(rir=P, times=P, dry=P, out=P, B=3, R=4, K=9600, N=1000, dry_stride=0, L=10599, ws=P, ws_bytes=SPEC * 66)
    a.update(kw)
    return lib.unetrir_auralize_path_f32(a["rir"], a["times"], a["dry"], a["out"], a["B"], a["R"], a["K"], a["N"], a["dry_stride"], a["L"],
                                         a["ws"], a["ws_bytes"], None)


BAD = [dict(rir=None), dict(times=None), dict(dry=None), dict(out=None), dict(ws=None),
       dict(rir=None, times=None, dry=None, out=None, ws=None),
       dict(B=0), dict(B=-1), dict(R=0), dict(R=-1), dict(K=0), dict(K=-5), dict(N=0), dict(N=-1),
       dict(K=16385, L=1), dict(K=1 << 20, L=1),
       dict(L=0), dict(L=-1), dict(L=10600), dict(N=2147483647, K=16384, L=-2147483648),
       dict(dry_stride=1), dict(dry_stride=999), dict(dry_stride=-1000), dict(dry_stride=-1),
       dict(ws_bytes=SPEC * 66 - 1), dict(ws_bytes=0), dict(ws_bytes=SPEC * 21), dict(dry_stride=1000, ws_bytes=SPEC * 78 - 1),
       dict(ws=24), dict(ws=17), dict(ws=20),
       dict(B=2147483647, ws_bytes=1 << 62), dict(R=2147483647, ws_bytes=1 << 62), dict(B=65536, R=65536, ws_bytes=1 << 62),
       dict(B=1 << 15, R=1 << 14, K=16384, ws_bytes=1 << 62),                       # B R Q = 2^32 spectra: beyond a launch
       dict(B=1 << 20, R=1, N=2147483647, L=2147483647, ws_bytes=1 << 62)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_every_bad_argument_is_refused_before_the_device(lib, bad):
    assert _call(lib, **bad) == EINVAL
    null = dict(rir=None, times=None, dry=None, out=None)
    null.update(bad)
    assert _call(lib, **null) == EINVAL                 # and with null device pointers


def test_good_arguments_with_null_device_pointers_are_refused_too(lib):
    assert _call(lib, rir=None, dry=None, out=None) == EINVAL
    assert _call(lib, times=None) == EINVAL


def test_the_python_gate_refuses_a_bad_schedule_before_the_launch():
    import torch
    import unet_rir_amd as U
    h, x = torch.zeros(4, 50), torch.zeros(200)
    for times, word in (([0, 100, 100, 300], "increasing"), ([0, 100, 90, 300], "increasing"), ([300, 200, 100, 0], "increasing"),
                        ([0, 31, 100, 200], "32 samples"), ([0, 100, 200, 231], "32 samples"),
                        ([0, 100, 200], "times for 4 nodes"), ([0, 100, 200, 300, 400], "times for 4 nodes"), ([[0, 100, 200, 300]], "times for"),
                        ([0, 100, 200, (1 << 30) + 1], "range"), ([-(1 << 30) - 1, 100, 200, 300], "range"),
                        ([0.5, 100, 200, 300], "whole"), ([0, 100, float("nan"), 300], "whole"),
                        (np.array([0, 100, 100, 300]), "increasing"), (torch.tensor([0, 100, 100, 300]), "increasing")):
        with pytest.raises(ValueError, match=word):
            U.auralize_path(h, x, times)
    for kw, word in ((dict(spacing=31), "32 samples"), (dict(spacing=0), "increasing"), (dict(spacing=-64), "increasing"),
                     (dict(spacing=2.5), "whole"), (dict(spacing=64, start=0.5), "whole"), (dict(spacing=1 << 29), "range"),
                     (dict(), "either"), (dict(times=[0, 100, 200, 300], spacing=64), "either")):
        with pytest.raises(ValueError, match=word):
            U.auralize_path(h, x, **kw)
    # a good schedule passes the host checks and stops at the device gate: there is no CPU path
    for kw in (dict(times=[0, 32, 64, 96]), dict(times=[-500, 37, 2047, 1 << 30]), dict(times=np.array([0, 100, 200, 300], dtype=np.int16)),
               dict(times=torch.tensor([0.0, 100.0, 200.0, 300.0])), dict(spacing=32), dict(spacing=32, start=-1000)):
        with pytest.raises(ValueError, match="CUDA"):
            U.auralize_path(h, x, **kw)
    with pytest.raises(ValueError, match="CUDA"):
        U.auralize_path(torch.zeros(1, 50), x, [7])     # R = 1: nothing to compare


def test_the_python_gate_checks_shapes_dtypes_and_devices():
    import torch
    import unet_rir_amd as U
    x = torch.zeros(200)
    t4 = [0, 100, 200, 300]
    bad = [((torch.zeros(3, 4, 50), x), "CUDA"), ((torch.zeros(4, 50), x), "CUDA"),
           ((torch.zeros(3, 4, 50).double(), x), "float32"), ((torch.zeros(3, 4, 50), x.to(torch.float16)), "float32"),
           ((torch.zeros(3, 50, 4).transpose(1, 2), x), "contiguous"), ((torch.zeros(3, 4, 50), torch.zeros(400)[::2]), "contiguous"),
           ((torch.zeros(3, 4, 50), torch.zeros(2, 200)), "batch"), ((torch.zeros(4, 50), torch.zeros(2, 200)), "batch"),
           ((torch.zeros(50), x), "rir"), ((torch.zeros(2, 3, 4, 50), x), "rir"), ((torch.zeros(3, 4, 50), torch.zeros(1, 3, 200)), "dry"),
           ((torch.zeros(3, 4, 50), torch.zeros(0)), "empty"), ((torch.zeros(3, 0, 50), x), "empty"), ((torch.zeros(3, 4, 0), x), "empty"),
           (("rir", x), "tensors")]
    for args, word in bad:
        with pytest.raises(ValueError, match=word):
            U.auralize_path(*args, times=t4)
    h = torch.zeros(3, 4, 50)
    for length in (0, 250, -1, "valid", 2.5, True, None):
        with pytest.raises(ValueError, match="length"):
            U.auralize_path(h, x, t4, length=length)
    for out, word in ((torch.zeros(3, 248), "out"), (torch.zeros(2, 249), "out"), (torch.zeros(3, 249, dtype=torch.float64), "float32"),
                      (torch.zeros(249, 3).t(), "contiguous")):
        with pytest.raises(ValueError, match=word):
            U.auralize_path(h, x, t4, out=out)


def test_the_wrapper_checks_its_tensors_and_not_the_schedule():
    import torch
    import unet_rir_amd as U
    h, x, out = torch.zeros(3, 4, 50), torch.zeros(200), torch.zeros(3, 249)
    t = torch.tensor([0, 100, 200, 300], dtype=torch.int32)
    f = U.ops.auralize_path_f32
    for args, word in (((h, t, x, out), "CUDA"), ((h.double(), t, x, out), "float32"), ((h, t, x.int(), out), "float32"),
                       ((h, t, x, out.double()), "float32"), ((torch.zeros(3, 50, 4).transpose(1, 2), t, x, out), "contiguous"),
                       ((h, t, torch.zeros(2, 200), out), "batch"), ((h, t, x, torch.zeros(2, 249)), "batch"),
                       ((torch.zeros(4, 50), t, x, out), "rir"), ((h, t, x, torch.zeros(3, 250)), "outside"),
                       ((torch.zeros(3, 0, 50), t, x, out), "empty"), ((h, t, torch.zeros(0), out), "empty"), ((h, t, x, "out"), "tensors")):
        with pytest.raises(ValueError, match=word):
            f(*args)
    # a schedule that is no strictly increasing one passes: the contents of times are the device's business
    with pytest.raises(ValueError, match="CUDA"):
        f(h, torch.tensor([5, 5, 1, 0], dtype=torch.int32), x, out)

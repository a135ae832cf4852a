"""The entry points of csrc/auralize_fft.hip are exported, declared in include/unetrir.h, bound in _lib and wrapped in ops, and refuse
every bad argument with UNETRIR_EINVAL (10001) before the device is touched - checked here without a GPU: the pointers are the non-null
dummy 16 (or null where that is the fault), so only the argument checks stand between the call and a launch.  The python gate is checked
with CPU tensors."""
import pytest

from test_abi import declared_symbols

EINVAL = 10001
NEW = ["unetrir_auralize_fft_supported", "unetrir_auralize_fft_block", "unetrir_auralize_fft_ws_bytes", "unetrir_auralize_fft_f32"]
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
    for n in ("auralize_fft_supported", "auralize_fft_block", "auralize_fft_ws_bytes", "auralize_fft_f32"):
        assert callable(getattr(U.ops, n)), n
    assert "auralize_fft.hip" in U.build.SOURCES
    assert lib.unetrir_abi_version() == 1


def test_supported_range_and_block(lib):
    import unet_rir_amd as U
    for K, want in ((1, 1), (2048, 1), (9600, 1), (16384, 1), (0, 0), (16385, 0), (-1, 0)):
        assert lib.unetrir_auralize_fft_supported(K) == want, K
        assert U.ops.auralize_fft_supported(K) is bool(want)
        assert lib.unetrir_auralize_fft_block(K) == (2048 if want else 0), K
        assert U.ops.auralize_fft_block(K) == (2048 if want else 0)


def test_workspace_bytes(lib):
    import unet_rir_amd as U
    ws = lib.unetrir_auralize_fft_ws_bytes
    # B Q spectra of h and J (x shared) or B J (x per row) of x
    assert ws(3, 9600, 1000, 0, 10599) == SPEC * (3 * 5 + 6)
    assert ws(3, 9600, 1000, 1000, 10599) == SPEC * (3 * 5 + 3 * 6) == U.ops.auralize_fft_ws_bytes(3, 9600, 1000, 1000, 10599)
    assert ws(3, 9600, 1000, 1024, 1) == SPEC * (3 * 5 + 3 * 1)
    assert ws(1, 1, 1, 0, 1) == SPEC * 2
    assert ws(32, 2048, 2049, 0, 2048) == SPEC * (32 + 1) and ws(32, 2049, 2049, 0, 2049) == SPEC * (64 + 2)
    for bad in ((0, 9600, 1000, 0, 10599), (-1, 9600, 1000, 0, 10599), (3, 0, 1000, 0, 1), (3, 16385, 1000, 0, 1), (3, 9600, 0, 0, 1),
                (3, 9600, 1000, 0, 0), (3, 9600, 1000, 0, 10600), (3, 9600, 1000, 999, 10599), (3, 9600, 1000, -1, 10599),
                (2147483647, 9600, 1000, 0, 10599), (1 << 20, 9600, 2147483647, 0, 2147483647)):
        assert ws(*bad) == 0, bad


def _call(lib, **kw):
    a = dict(rir=P, dry=P, out=P, B=3, K=9600, N=1000, dry_stride=0, L=10599, ws=P, ws_bytes=SPEC * 21)
    a.update(kw)
    return lib.unetrir_auralize_fft_f32(a["rir"], a["dry"], a["out"], a["B"], a["K"], a["N"], a["dry_stride"], a["L"], a["ws"],
                                        a["ws_bytes"], None)


BAD = [dict(rir=None), dict(dry=None), dict(out=None), dict(ws=None), dict(rir=None, dry=None, out=None, ws=None),
       dict(B=0), dict(B=-1), dict(K=0), dict(K=-5), dict(N=0), dict(N=-1),
       dict(K=16385, L=1), dict(K=1 << 20, L=1),
       dict(L=0), dict(L=-1), dict(L=10600), dict(N=2147483647, K=16384, L=-2147483648),
       dict(dry_stride=1), dict(dry_stride=999), dict(dry_stride=-1000), dict(dry_stride=-1),
       dict(ws_bytes=SPEC * 21 - 1), dict(ws_bytes=0), dict(dry_stride=1000, ws_bytes=SPEC * 33 - 1),
       dict(ws=24), dict(ws=17), dict(ws=20),
       dict(B=2147483647, ws_bytes=1 << 62), dict(B=1 << 20, N=2147483647, L=2147483647, ws_bytes=1 << 62)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_every_bad_argument_is_refused_before_the_device(lib, bad):
    assert _call(lib, **bad) == EINVAL
    null = dict(rir=None, dry=None, out=None)
    null.update(bad)
    assert _call(lib, **null) == EINVAL                 # and with null device pointers


def test_good_arguments_with_null_device_pointers_are_refused_too(lib):
    assert _call(lib, rir=None, dry=None, out=None) == EINVAL


def test_the_python_gate_checks_its_arguments_before_the_launch():
    import torch
    import unet_rir_amd as U
    from test_auralize_abi import _gate
    h, x = torch.zeros(3, 50), torch.zeros(200)
    for method in ("bogus", "auto", "FFT", None, 1):
        with pytest.raises(ValueError, match="method"):
            U.auralize(h, x, method=method)
    _gate(lambda rir, dry: U.auralize(rir, dry, method="fft"))
    for length in (0, 250, -1, "valid", 2.5, True, None):
        with pytest.raises(ValueError, match="length"):
            U.auralize(h, x, length=length, method="fft")
    _gate(lambda rir, dry: U.ops.auralize_fft_f32(rir, dry, torch.zeros(rir.shape[0], 249)))
    with pytest.raises(ValueError, match="batch"):
        U.ops.auralize_fft_f32(h, x, torch.zeros(2, 249))
    with pytest.raises(ValueError, match="outside"):
        U.ops.auralize_fft_f32(h, x, torch.zeros(3, 250))

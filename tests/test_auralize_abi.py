"""The entry points of csrc/auralize.hip are exported, declared in include/unetrir.h, bound in _lib and wrapped in ops, and refuse every
bad argument with UNETRIR_EINVAL (10001) before the device is touched - checked here without a GPU: the pointers are the non-null
dummy 16 (or null where that is the fault), so only the argument checks stand between the call and a launch.  The python gate is
checked with CPU tensors: shape, dtype and contiguity are looked at before the device is."""
import pytest

from test_abi import declared_symbols

EINVAL = 10001
NEW = ["unetrir_auralize_supported", "unetrir_auralize_f32"]
P = 16          # a dummy device pointer


@pytest.fixture(scope="module")
def lib():
    import unet_rir_amd
    return unet_rir_amd._lib.lib()


def test_new_symbols_are_exported_declared_bound_and_wrapped(lib):
    L = lib
    import unet_rir_amd as U
    declared = declared_symbols()
    for n in NEW:
        assert n in declared and n in U._lib.EXPORTS and hasattr(L, n), n
    for n in ("auralize_supported", "auralize_f32"):
        assert callable(getattr(U.ops, n)), n
    assert "auralize.hip" in U.build.SOURCES
    assert L.unetrir_abi_version() == 1
    assert "auralize" in U.__all__ and callable(U.auralize) and callable(U.auralize.__globals__["write_wav"])
    assert "auralize" not in U.evaluate.__all__


def test_supported_range(lib):
    L = lib
    import unet_rir_amd as U
    for K, want in ((1, 1), (9600, 1), (16384, 1), (0, 0), (16385, 0), (-1, 0)):
        assert L.unetrir_auralize_supported(K) == want, K
        assert U.ops.auralize_supported(K) is bool(want)


def _call(lib, **kw):
    a = dict(rir=P, dry=P, out=P, B=3, K=9600, N=1000, dry_stride=0, L=10599)
    a.update(kw)
    return lib.unetrir_auralize_f32(a["rir"], a["dry"], a["out"], a["B"], a["K"], a["N"], a["dry_stride"], a["L"], None)


BAD = [dict(rir=None), dict(dry=None), dict(out=None), dict(rir=None, dry=None, out=None),
       dict(B=0), dict(B=-1), dict(K=0), dict(K=-5), dict(N=0), dict(N=-1),
       dict(K=16385, L=1), dict(K=1 << 20, L=1),
       dict(L=0), dict(L=-1), dict(L=10600), dict(N=2147483647, K=16384, L=-2147483648),
       dict(dry_stride=1), dict(dry_stride=999), dict(dry_stride=-1000), dict(dry_stride=-1)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_every_bad_argument_is_refused_before_the_device(lib, bad):
    assert _call(lib, **bad) == EINVAL
    null = dict(rir=None, dry=None, out=None)
    null.update(bad)
    assert _call(lib, **null) == EINVAL                 # and with null device pointers


def _gate(fn):
    """fn(rir, dry, **kw) must raise ValueError with these words, on CPU tensors."""
    import torch
    h, x = torch.zeros(3, 50), torch.zeros(200)
    bad = [
        ((h, x), {}, "CUDA"),                                                      # a CPU tensor
        ((h.double(), x), {}, "float32"), ((h, x.to(torch.float16)), {}, "float32"), ((h, x.int()), {}, "float32"),
        ((torch.zeros(50, 3).t(), x), {}, "contiguous"), ((h, torch.zeros(400)[::2]), {}, "contiguous"),
        ((h, torch.zeros(2, 200)), {}, "batch"), ((h, torch.zeros(4, 200)), {}, "batch"),
        ((torch.zeros(2, 3, 50), x), {}, "rir"), ((h, torch.zeros(1, 3, 200)), {}, "dry"), ((h, torch.zeros(0)), {}, "empty"),
    ]
    for args, kw, word in bad:
        with pytest.raises(ValueError, match=word):
            fn(*args, **kw)


def test_the_python_gate_checks_its_arguments_before_the_launch():
    import torch
    import unet_rir_amd as U
    _gate(U.auralize)
    h, x = torch.zeros(3, 50), torch.zeros(200)
    for length in (0, 250, -1, "valid", 2.5, True, None):
        with pytest.raises(ValueError, match="length"):
            U.auralize(h, x, length=length)
    for out, word in ((torch.zeros(3, 248), "out"), (torch.zeros(2, 249), "out"), (torch.zeros(3, 249, dtype=torch.float64), "float32"),
                      (torch.zeros(249, 3).t(), "contiguous")):
        with pytest.raises(ValueError, match=word):
            U.auralize(h, x, out=out)
    with pytest.raises(ValueError, match="CUDA"):
        U.auralize(torch.zeros(50), x, length="same", out=torch.zeros(1, 200))      # [K] is taken as one row; still no CPU path
    # the wrapper has the same gate
    _gate(lambda rir, dry: U.ops.auralize_f32(rir, dry, torch.zeros(rir.shape[0], 249)))
    with pytest.raises(ValueError, match="batch"):
        U.ops.auralize_f32(h, x, torch.zeros(2, 249))
    with pytest.raises(ValueError, match="outside"):
        U.ops.auralize_f32(h, x, torch.zeros(3, 250))

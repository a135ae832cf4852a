"""The entry points of `AuralizeStream` (csrc/auralize_fft.hip) are exported, declared in include/unetrir.h, bound in _lib and wrapped in
ops, and refuse every bad argument with UNETRIR_EINVAL (10001) before the device is touched - checked here without a GPU: the pointers
are the non-null dummy 16 (or null where that is the fault), so only the argument checks stand between the call and a launch.  The
python gates - `AuralizeStream` and the `ops.auralize_stream_*` wrappers - are checked with CPU tensors."""
import pytest

from test_abi import declared_symbols

EINVAL = 10001
NEW = ["unetrir_auralize_stream_supported", "unetrir_auralize_stream_state_bytes", "unetrir_auralize_stream_init",
       "unetrir_auralize_stream_update", "unetrir_auralize_stream_push"]
PTR = 16        # a dummy device pointer, 16-byte aligned
SPEC = 16384    # bytes of one packed spectrum
P = 2048


def state_bytes(B, K, rows, mb):
    """the formula of include/unetrir.h: control, 2 B Q spectra of h, the ring of rows S spectra, the carry of rows P floats"""
    Q = -(-K // P)
    return 64 + SPEC * (2 * B * Q + rows * (Q + mb - 1)) + 4 * P * rows


@pytest.fixture(scope="module")
def lib():
    import unet_rir_amd
    return unet_rir_amd._lib.lib()


def test_new_symbols_are_exported_declared_bound_and_wrapped(lib):
    import unet_rir_amd as U
    declared = declared_symbols()
    for n in NEW:
        assert n in declared and n in U._lib.EXPORTS and hasattr(lib, n), n
    for n in ("auralize_stream_supported", "auralize_stream_state_bytes", "auralize_stream_init", "auralize_stream_update",
              "auralize_stream_push_f32", "AuralizeStreamState"):
        assert callable(getattr(U.ops, n)), n
    assert callable(U.AuralizeStream) and "AuralizeStream" in U.__all__
    for n in ("push", "update", "flush", "reset", "state_bytes"):
        assert hasattr(U.AuralizeStream, n), n
    assert lib.unetrir_abi_version() == 1


def test_supported_range(lib):
    import unet_rir_amd as U
    for K, want in ((1, 1), (2048, 1), (9600, 1), (16384, 1), (0, 0), (16385, 0), (-1, 0)):
        assert lib.unetrir_auralize_stream_supported(K) == want == lib.unetrir_auralize_fft_supported(K), K
        assert U.ops.auralize_stream_supported(K) is bool(want)


def test_state_bytes(lib):
    import unet_rir_amd as U
    f = lib.unetrir_auralize_stream_state_bytes
    assert f(3, 9600, 1, 8) == 64 + SPEC * (2 * 3 * 5 + 12) + 8192 == 696384
    for B, K, rows, mb in ((1, 1, 1, 1), (3, 9600, 3, 8), (3, 2048, 1, 64), (3, 2049, 3, 1), (32, 16384, 1, 2), (32, 16384, 32, 64),
                           (1, 4097, 1, 3)):
        assert f(B, K, rows, mb) == state_bytes(B, K, rows, mb) == U.ops.auralize_stream_state_bytes(B, K, rows, mb), (B, K, rows, mb)
    for bad in ((0, 9600, 1, 8), (-1, 9600, 1, 8), (3, 0, 1, 8), (3, 16385, 1, 8), (3, -5, 1, 8), (3, 9600, 0, 8), (3, 9600, 2, 8),
                (3, 9600, 4, 8), (3, 9600, -1, 8), (3, 9600, 1, 0), (3, 9600, 1, 65), (3, 9600, 1, -1), (2147483647, 9600, 1, 8),
                (1 << 28, 16384, 1, 1), (1 << 26, 1, 1, 64)):
        assert f(*bad) == 0, bad


GOOD = dict(state=PTR, state_bytes=state_bytes(3, 9600, 1, 8), rir=PTR, B=3, K=9600, dry_rows=1, max_blocks=8, dry=PTR, dry_stride=0,
            out=PTR, out_stride=4 * P, blocks=4)


def _init(lib, entry="init", **kw):
    a = dict(GOOD)
    a.update(kw)
    f = lib.unetrir_auralize_stream_init if entry == "init" else lib.unetrir_auralize_stream_update
    return f(a["state"], a["state_bytes"], a["rir"], a["B"], a["K"], a["dry_rows"], a["max_blocks"], None)


def _push(lib, **kw):
    a = dict(GOOD)
    a.update(kw)
    return lib.unetrir_auralize_stream_push(a["state"], a["state_bytes"], a["B"], a["K"], a["dry_rows"], a["max_blocks"], a["dry"],
                                            a["dry_stride"], a["out"], a["out_stride"], a["blocks"], None)


BAD_STATE = [dict(state=None), dict(state=24), dict(state=17), dict(state=20), dict(state_bytes=0), dict(state_bytes=GOOD["state_bytes"] - 1),
             dict(B=4), dict(K=16384), dict(max_blocks=9), dict(dry_rows=3),                 # the state is too small for these
             dict(B=0), dict(B=-1), dict(K=0), dict(K=-5), dict(K=16385, state_bytes=1 << 40), dict(dry_rows=0), dict(dry_rows=2),
             dict(dry_rows=-1), dict(max_blocks=0), dict(max_blocks=65, state_bytes=1 << 40), dict(max_blocks=-1),
             dict(B=2147483647, state_bytes=1 << 62), dict(B=1 << 28, K=16384, state_bytes=1 << 62)]
BAD_RIR = [dict(rir=None), dict(rir=None, state=None)]
BAD_PUSH = [dict(out=None), dict(out=None, dry=None), dict(blocks=0), dict(blocks=-1), dict(blocks=9), dict(blocks=2147483647),
            dict(max_blocks=2, blocks=3), dict(out_stride=4 * P - 1), dict(out_stride=0), dict(out_stride=-4 * P),
            dict(dry_stride=1), dict(dry_stride=4 * P - 1), dict(dry_stride=-1), dict(dry_stride=-4 * P),
            dict(dry_rows=3, state_bytes=1 << 40, dry_stride=0), dict(dry_rows=3, state_bytes=1 << 40, dry_stride=4 * P - 1)]


@pytest.mark.parametrize("entry", ("init", "update"))
@pytest.mark.parametrize("bad", BAD_STATE + BAD_RIR, ids=[str(b) for b in BAD_STATE + BAD_RIR])
def test_init_and_update_refuse_every_bad_argument_before_the_device(lib, entry, bad):
    assert _init(lib, entry, **bad) == EINVAL
    null = dict(rir=None)
    null.update(bad)
    assert _init(lib, entry, **null) == EINVAL           # and with a null device pointer


@pytest.mark.parametrize("bad", BAD_STATE + BAD_PUSH, ids=[str(b) for b in BAD_STATE + BAD_PUSH])
def test_push_refuses_every_bad_argument_before_the_device(lib, bad):
    assert _push(lib, **bad) == EINVAL
    null = dict(dry=None, out=None)
    null.update(bad)
    assert _push(lib, **null) == EINVAL                  # and with null device pointers


def test_good_arguments_with_null_device_pointers_are_refused_too(lib):
    assert _init(lib, "init", rir=None) == EINVAL and _init(lib, "update", rir=None) == EINVAL
    assert _push(lib, out=None) == EINVAL and _push(lib, state=None) == EINVAL
    assert _push(lib, dry=None, out=None) == EINVAL      # a null dry alone is no fault: it stands for zeros


def test_the_class_checks_its_arguments_before_the_device():
    import torch
    import unet_rir_amd as U
    h = torch.zeros(3, 50)
    for args, kw, word in (((h,), {}, "CUDA"), ((h,), dict(dry_rows="rows"), "CUDA"), ((torch.zeros(50),), {}, "CUDA"),
                           ((h.double(),), {}, "float32"), ((h.int(),), {}, "float32"),
                           ((h,), dict(dry_rows="both"), "dry_rows"), ((h,), dict(dry_rows=1), "dry_rows"), ((h,), dict(dry_rows=None), "dry_rows"),
                           ((h,), dict(max_blocks=0), "max_blocks"), ((h,), dict(max_blocks=65), "max_blocks"),
                           ((h,), dict(max_blocks=2.0), "max_blocks"), ((h,), dict(max_blocks=True), "max_blocks"),
                           ((torch.zeros(3, 16385),), {}, "supported"), ((torch.zeros(3, 0),), {}, "empty"),
                           ((torch.zeros(0, 50),), {}, "empty"), ((torch.zeros(2, 3, 50),), {}, "rir"), (("rir",), {}, "tensor")):
        with pytest.raises(ValueError, match=word):
            U.AuralizeStream(*args, **kw)


def test_the_wrappers_check_their_tensors():
    """A state on the CPU can be made (it is memory and four numbers); every call on it stops at its gate."""
    import torch
    import unet_rir_amd as U
    st = U.ops.AuralizeStreamState("cpu", 3, 50, 1, 2)
    assert st.nbytes == st.need == state_bytes(3, 50, 1, 2) and st.block == P
    for args, word in (((3, 50, 2, 2), "dry_rows"), ((3, 50, 1, 0), "max_blocks"), ((3, 50, 1, 65), "max_blocks"), ((0, 50, 1, 2), "B ="),
                       ((3, 16385, 1, 2), "supported"), ((3, 0, 1, 2), "supported")):
        with pytest.raises(ValueError, match=word):
            U.ops.AuralizeStreamState("cpu", *args)
    for buf, word in ((torch.zeros(st.need - 1, dtype=torch.uint8), "at least"), (torch.zeros(st.need, dtype=torch.int8), "uint8"),
                      (torch.zeros(st.need + 16, dtype=torch.uint8)[1:], "aligned")):
        with pytest.raises(ValueError, match=word):
            U.ops.AuralizeStreamState("cpu", 3, 50, 1, 2, buf=buf)
    h = torch.zeros(3, 50)
    for f in (U.ops.auralize_stream_init, U.ops.auralize_stream_update):
        for rir, word in ((h, "CUDA"), (torch.zeros(3, 60), "shape"), (torch.zeros(2, 50), "shape"), (torch.zeros(50), "shape"),
                          (h.double(), "float32"), (torch.zeros(50, 3).t(), "contiguous"), ("rir", "tensor")):
            with pytest.raises(ValueError, match=word):
                f(st, rir)
        with pytest.raises(ValueError, match="state"):
            f("state", h)
    push = U.ops.auralize_stream_push_f32
    x, out = torch.zeros(2 * P), torch.zeros(3, 2 * P)
    for args, word in (((st, x, out), "CUDA"), ((st, None, out), "CUDA"), ((st, x.view(1, -1), out), "CUDA"),
                       ((st, x, torch.zeros(3, 3 * P)), "blocks"), ((st, x, torch.zeros(3, P + 1)), "blocks"), ((st, x, torch.zeros(3, 0)), "blocks"),
                       ((st, x, torch.zeros(2, 2 * P)), "blocks"), ((st, x, torch.zeros(2 * P)), "blocks"),
                       ((st, torch.zeros(P), out), "dry must be"), ((st, torch.zeros(3, 2 * P), out), "dry must be"),
                       ((st, x.double(), out), "float32"), ((st, x, out.double()), "float32"),
                       ((st, torch.zeros(4 * P)[::2], out), "contiguous"), ((st, x, torch.zeros(2 * P, 3).t()), "contiguous"),
                       ((st, "x", out), "tensors"), (("st", x, out), "state")):
        with pytest.raises(ValueError, match=word):
            push(*args)
    rows = U.ops.AuralizeStreamState("cpu", 3, 50, 3, 2)
    for dry, word in ((x, "dry must be"), (torch.zeros(1, 2 * P), "dry must be"), (torch.zeros(3, 2 * P), "CUDA"),
                      (torch.zeros(3, 4 * P)[:, :2 * P], "CUDA")):                          # a column slice of dense rows passes the gate
        with pytest.raises(ValueError, match=word):
            push(rows, dry, out)

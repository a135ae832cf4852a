"""The entry points of csrc/griffinlim_fft.hip are exported, declared in include/unetrir.h, bound in _lib and wrapped in ops, answer the
supported rule and the workspace by their closed forms, and refuse every bad argument with UNETRIR_EINVAL (10001) before the device is
touched - checked here without a GPU: the pointers are the non-null dummy 16 (or null where that is the fault), so only the argument checks
stand between the call and a launch.  The python gate is checked with CPU tensors."""
import pytest

from test_abi import declared_symbols

EINVAL = 10001
NEW = ["unetrir_griffinlim_fft_supported", "unetrir_griffinlim_fft_ws_bytes", "unetrir_griffinlim_fft_f32"]
P = 16          # a dummy device pointer, 16-byte aligned


@pytest.fixture(scope="module")
def lib():
    import unet_rir_amd
    return unet_rir_amd._lib.lib()


def test_new_symbols_are_exported_declared_bound_and_wrapped(lib):
    import unet_rir_amd as U
    declared = declared_symbols()
    for n in NEW:
        assert n in declared and n in U._lib.EXPORTS and hasattr(lib, n), n
    for n in ("griffinlim_fft_supported", "griffinlim_fft_ws_bytes", "griffinlim_fft"):
        assert callable(getattr(U.ops, n)), n
    assert "griffinlim_fft.hip" in U.build.SOURCES
    assert lib.unetrir_abi_version() == 1


# (n_bins, n_frames, n_fft, win, hop) -> supported
RULE = [((129, 151, 256, 128, 64), 1), ((65, 4, 128, 64, 32), 1), ((65, 14, 128, 128, 32), 1), ((65, 11, 128, 100, 40), 1),
        ((257, 17, 512, 256, 128), 1), ((513, 17, 1024, 512, 256), 1), ((513, 4, 1024, 1024, 256), 1),
        ((65, 3, 128, 2, 33), 1), ((65, 66, 128, 2, 1), 1), ((65, 66, 128, 4, 1), 1), ((65, 2, 128, 64, 65), 1),
        ((129, 151, 256, 3, 64), 1), ((129, 151, 256, 256, 64), 1), ((129, 3, 256, 128, 100000), 1),
        # n_fft outside 128 ... 1024 or no power of two
        ((33, 151, 64, 32, 16), 0), ((1025, 151, 2048, 1024, 512), 0), ((97, 151, 192, 96, 48), 0), ((1, 151, 0, 0, 1), 0),
        # n_bins is not n_fft / 2 + 1
        ((128, 151, 256, 128, 64), 0), ((130, 151, 256, 128, 64), 0), ((256, 151, 256, 128, 64), 0),
        # frames, window
        ((129, 1, 256, 128, 64), 0), ((129, 0, 256, 128, 64), 0), ((129, -3, 256, 128, 64), 0),
        ((129, 151, 256, 1, 64), 0), ((129, 151, 256, 0, 64), 0), ((129, 151, 256, 257, 65), 0), ((129, 151, 256, -128, 64), 0),
        # the hop: at least win / 4
        ((129, 151, 256, 128, 31), 0), ((129, 151, 256, 128, 32), 1), ((129, 151, 256, 129, 32), 0), ((129, 151, 256, 129, 33), 1),
        ((129, 151, 256, 128, 0), 0), ((129, 151, 256, 128, -64), 0), ((65, 66, 128, 5, 1), 0),
        # the length: hop (n_frames - 1) > n_fft / 2
        ((65, 3, 128, 64, 32), 0), ((65, 2, 128, 64, 64), 0), ((65, 65, 128, 2, 1), 0), ((129, 3, 256, 128, 64), 0),
        ((129, 4, 256, 128, 64), 1),
        # hop n_frames + n_fft fits an int
        ((129, 21474, 256, 128, 100000), 1), ((129, 21475, 256, 128, 100000), 0), ((129, 2147483647, 256, 128, 64), 0)]


@pytest.mark.parametrize("geo,want", RULE, ids=[str(g) for g, _ in RULE])
def test_the_supported_rule_at_its_edges(lib, geo, want):
    import unet_rir_amd as U
    assert lib.unetrir_griffinlim_fft_supported(*geo) == want
    assert U.ops.griffinlim_fft_supported(*geo) is bool(want)
    # the workspace: 7 fp32 planes of B n_frames n_bins, rounded up to 8 bytes; 0 for everything the rule refuses
    for B in (1, 3, 32):
        nb, nf = geo[0], geo[1]
        closed = (7 * B * nf * nb * 4 + 7) // 8 * 8 if want else 0
        assert lib.unetrir_griffinlim_fft_ws_bytes(B, *geo) == closed == U.ops.griffinlim_fft_ws_bytes(B, *geo)
    for B in (0, -1, 65536, 2147483647):
        assert lib.unetrir_griffinlim_fft_ws_bytes(B, *geo) == 0


def test_workspace_is_well_under_half_of_the_dft_forms(lib):
    for B, geo in ((32, (129, 151, 256, 128, 64)), (3, (65, 18, 128, 64, 32)), (2, (513, 17, 1024, 512, 256))):
        fft, dft = lib.unetrir_griffinlim_fft_ws_bytes(B, *geo), lib.unetrir_griffinlim_ws_bytes(B, *geo[:3])
        assert 0 < fft < 0.4 * dft, (geo, fft, dft)
    assert lib.unetrir_griffinlim_fft_ws_bytes(32, 129, 151, 256, 128, 64) == 7 * 32 * 151 * 129 * 4


GOOD = dict(feat=P, B=3, H=144, W=160, n_bins=129, n_frames=151, n_fft=256, win=128, hop=64, pad_mode=0, denormalize=1, n_iter=32,
            momentum=0.99, init_phase=P, seed=0, draw=0, wav=P, ws=P, ws_bytes=7 * 3 * 151 * 129 * 4)


def _call(lib, **kw):
    a = dict(GOOD)
    a.update(kw)
    return lib.unetrir_griffinlim_fft_f32(a["feat"], a["B"], a["H"], a["W"], a["n_bins"], a["n_frames"], a["n_fft"], a["win"], a["hop"],
                                          a["pad_mode"], a["denormalize"], a["n_iter"], a["momentum"], a["init_phase"], a["seed"],
                                          a["draw"], a["wav"], a["ws"], a["ws_bytes"], None)


BIG = 1 << 62
BAD = [dict(feat=None), dict(wav=None), dict(ws=None), dict(feat=None, wav=None, ws=None, init_phase=None),
       dict(ws=20), dict(ws=17), dict(ws=12),
       dict(B=0), dict(B=-1), dict(B=65536, ws_bytes=BIG), dict(B=2147483647, ws_bytes=BIG),
       dict(H=128), dict(W=150), dict(H=0), dict(W=-1),
       dict(n_fft=64, n_bins=33, win=32, hop=16, ws_bytes=BIG), dict(n_fft=2048, n_bins=1025, H=1040, win=1024, hop=512, ws_bytes=BIG),
       dict(n_fft=192, n_bins=97, ws_bytes=BIG), dict(n_fft=0, ws_bytes=BIG), dict(n_fft=-256, ws_bytes=BIG),
       dict(n_bins=128, ws_bytes=BIG), dict(n_bins=130, ws_bytes=BIG), dict(n_bins=0, ws_bytes=BIG),
       dict(n_frames=1, ws_bytes=BIG), dict(n_frames=0, ws_bytes=BIG), dict(n_frames=-151, ws_bytes=BIG), dict(n_frames=3, ws_bytes=BIG),
       dict(win=1, ws_bytes=BIG), dict(win=0, ws_bytes=BIG), dict(win=257, hop=128, ws_bytes=BIG), dict(win=-1, ws_bytes=BIG),
       dict(hop=31, ws_bytes=BIG), dict(hop=0, ws_bytes=BIG), dict(hop=-64, ws_bytes=BIG),
       dict(hop=100000, n_frames=21475, W=21488, ws_bytes=BIG),
       dict(pad_mode=2), dict(pad_mode=-1), dict(n_iter=-1),
       dict(momentum=-0.5), dict(momentum=float("nan")), dict(momentum=float("inf")),
       dict(ws_bytes=7 * 3 * 151 * 129 * 4 - 1), dict(ws_bytes=0), dict(B=4)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_every_bad_argument_is_refused_before_the_device(lib, bad):
    assert _call(lib, **bad) == EINVAL
    null = dict(feat=None, wav=None, init_phase=None)
    null.update(bad)
    assert _call(lib, **null) == EINVAL                 # and with null device pointers


def test_good_arguments_with_null_device_pointers_are_refused_too(lib):
    assert _call(lib, feat=None, wav=None) == EINVAL
    assert _call(lib, feat=None) == EINVAL and _call(lib, wav=None) == EINVAL


def test_the_python_gate_checks_its_arguments_before_the_launch():
    import torch
    import unet_rir_amd as U
    from unet_rir_amd import features as F
    for method in ("bogus", "auto", "FFT", None, 1):
        with pytest.raises(ValueError, match="method"):
            F.GriffinLim(method=method)
        with pytest.raises(ValueError, match="method"):
            U.Evaluator(object(), algorithm="gl", gl_method=method)
        with pytest.raises(ValueError, match="gl_method"):
            U.Evaluator(object(), algorithm="ph", gl_method=method)      # whatever the algorithm
    assert F.GriffinLim().method == "dft" and F.GriffinLim(method="fft").method == "fft" and F.GriffinLim(method="fft").algorithm == "gl"
    assert U.Evaluator(object(), algorithm="gl", gl_method="fft")._post.method == "fft"
    assert U.Evaluator(object(), algorithm="gl")._post.method == "dft"
    feat = torch.zeros(2, 2, 144, 160)
    for method in ("dft", "fft"):                                                      # host tensors: there is no CPU path
        with pytest.raises(ValueError):
            F.GriffinLim(method=method).post_process(feat)
    ws = None                                                                          # the gate raises before the workspace is touched
    geo = (129, 151, 256, 128, 64)
    with pytest.raises(ValueError, match="contiguous fp32"):
        U.ops.griffinlim_fft(feat.double(), torch.zeros(2, 9600), *geo, ws)
    with pytest.raises(ValueError, match="contiguous fp32"):
        U.ops.griffinlim_fft(feat.permute(0, 1, 3, 2), torch.zeros(2, 9600), *geo, ws)
    with pytest.raises(ValueError, match=r"feat \[B, 2, H, W\]"):
        U.ops.griffinlim_fft(feat, torch.zeros(2, 9599), *geo, ws)
    with pytest.raises(ValueError, match=r"feat \[B, 2, H, W\]"):
        U.ops.griffinlim_fft(feat, torch.zeros(3, 9600), *geo, ws)
    with pytest.raises(ValueError, match="pad_mode"):
        U.ops.griffinlim_fft(feat, torch.zeros(2, 9600), *geo, ws, pad_mode="edge")
    with pytest.raises(ValueError, match="init_phase"):
        U.ops.griffinlim_fft(feat, torch.zeros(2, 9600), *geo, ws, init_phase=torch.zeros(2, 129, 150))

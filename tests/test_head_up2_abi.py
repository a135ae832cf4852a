"""The entry points of the folded up-sampling head (csrc/head_up2.hip, dl_models/u_net.py:247-248) checked without a GPU: exported,
declared in the header with their source lines, bound, wrapped, and every argument-validation case returns UNETRIR_EINVAL (10001)
before the device is touched."""
import os

NAMES = ("unetrir_head_up2_supported_f32", "unetrir_head_up2_supported_bf16", "unetrir_head_up2_fold", "unetrir_head_up2_fwd_f32",
         "unetrir_head_up2_fwd_bf16", "unetrir_head_up2_dgrad_f32", "unetrir_head_up2_dgrad_bf16", "unetrir_head_up2_wgrad_ws_bytes",
         "unetrir_head_up2_wgrad_f32", "unetrir_head_up2_wgrad_bf16")
EINVAL = 10001
P = 0x7F0000001000          # a non-null, 16-byte aligned address: validation must return before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import unet_rir_amd
    return unet_rir_amd, unet_rir_amd._lib.lib()


def test_new_symbols_are_exported_declared_bound_and_wrapped():
    import re
    U, L = _lib()
    header = open(os.path.join(ROOT, "include", "unetrir.h")).read()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in U._lib.EXPORTS, n
        assert n + "(" in header, n
    assert "u_net.py:247-248" in header                              # the entry points cite their call site
    for n in ("head_up2_supported", "head_up2_fold", "head_up2_fwd", "head_up2_dgrad", "head_up2_wgrad", "head_up2_wgrad_ws_bytes",
              "head_up2_folded_elems"):
        assert callable(getattr(U.ops, n)), n
    assert "head_up2.hip" in U.build.SOURCES
    assert L.unetrir_abi_version() == 1
    assert len(U._lib.Config._fields_) == 18                         # no new kernel-selection switch
    declared = set(re.findall(r"\b(unetrir_[a-z0-9_]+)\s*\(", header))
    assert set(U._lib.EXPORTS) == declared, (set(U._lib.EXPORTS) ^ declared)


def test_predicate_and_workspace_query():
    U, L = _lib()
    for sfx in ("f32", "bf16"):
        fn = getattr(L, "unetrir_head_up2_supported_" + sfx)
        for c in (8, 16, 32, 40, 64, 128, 256):
            m = fn(c)
            assert 0 <= m <= 7 and U.ops.head_up2_supported(c, sfx) == m, (sfx, c)
        for c in (0, -8, 4, 12, 36):
            assert fn(c) == 0, (sfx, c)
    assert (U.ops.UP2_FWD, U.ops.UP2_DGRAD, U.ops.UP2_WGRAD) == (1, 2, 4)
    ws = L.unetrir_head_up2_wgrad_ws_bytes
    # a function of (B, h, w, C) alone: one slab of 8 * 16 * C floats per 16 x 16 coarse tile, 256 at most, and the folded gradient
    assert ws(1, 1, 3, 8) == 2 * 128 * 8 * 4
    assert ws(2, 5, 7, 16) == 3 * 128 * 16 * 4
    assert ws(3, 16, 24, 64) == 7 * 128 * 64 * 4
    assert ws(32, 128, 128, 64) == 257 * 128 * 64 * 4
    assert U.ops.head_up2_wgrad_ws_bytes(3, 16, 24, 64) == ws(3, 16, 24, 64) and U.ops.head_up2_folded_elems(64) == 8192
    for a in ((0, 8, 8, 16), (2, 0, 8, 16), (2, 8, -1, 16), (2, 8, 8, 12), (2, 8, 8, 0)):
        assert ws(*a) == 0, a


def test_entry_points_validate_their_arguments():
    _, L = _lib()
    assert L.unetrir_head_up2_fold(None, 16, P, 0, None) == EINVAL and L.unetrir_head_up2_fold(P, 16, None, 1, None) == EINVAL
    assert L.unetrir_head_up2_fold(P, 12, P, 0, None) == EINVAL and L.unetrir_head_up2_fold(P, 0, P, 0, None) == EINVAL
    assert L.unetrir_head_up2_fold(P, 16, P + 4, 0, None) == EINVAL
    for sfx, g in (("f32", 4), ("bf16", 8)):
        fwd = lambda x=P, ldx=32, B=2, h=8, w=8, Cc=32, wf=P, bias=P, y=P, ldy=4: \
            getattr(L, "unetrir_head_up2_fwd_" + sfx)(x, ldx, B, h, w, Cc, wf, bias, y, ldy, None)
        for kw in (dict(x=None), dict(wf=None), dict(y=None), dict(B=0), dict(h=0), dict(w=-1), dict(Cc=12), dict(Cc=4), dict(Cc=0),
                   dict(ldx=24), dict(ldx=32 + g // 2), dict(ldy=1), dict(ldy=6), dict(x=P + 8), dict(wf=P + 4), dict(y=P + 4), dict(bias=P + 2)):
            assert fwd(**kw) == EINVAL, (sfx, kw)
        dgrad = lambda dy=P, lddy=8, B=2, h=8, w=8, wf=P, Cc=32, dx=P, lddx=32: \
            getattr(L, "unetrir_head_up2_dgrad_" + sfx)(dy, lddy, B, h, w, wf, Cc, dx, lddx, None)
        for kw in (dict(dy=None), dict(wf=None), dict(dx=None), dict(B=0), dict(h=-2), dict(w=0), dict(Cc=12), dict(Cc=0), dict(lddy=1),
                   dict(lddy=7), dict(lddx=24), dict(lddx=32 + g // 2), dict(dy=P + 2), dict(wf=P + 8), dict(dx=P + 8)):
            assert dgrad(**kw) == EINVAL, (sfx, kw)
        need = L.unetrir_head_up2_wgrad_ws_bytes(2, 8, 8, 32)
        assert need > 0
        wgrad = lambda x=P, ldx=32, B=2, h=8, w=8, Cc=32, dy=P, lddy=8, dw=P, ws=P, ws_bytes=need: \
            getattr(L, "unetrir_head_up2_wgrad_" + sfx)(x, ldx, B, h, w, Cc, dy, lddy, dw, ws, ws_bytes, None)
        for kw in (dict(x=None), dict(dy=None), dict(dw=None), dict(ws=None), dict(B=0), dict(h=0), dict(w=-3), dict(Cc=12), dict(Cc=0),
                   dict(ldx=24), dict(ldx=32 + g // 2), dict(lddy=1), dict(lddy=7), dict(x=P + 8), dict(dy=P + 2), dict(dw=P + 4),
                   dict(ws=P + 8), dict(ws_bytes=need - 4), dict(ws_bytes=0)):
            assert wgrad(**kw) == EINVAL, (sfx, kw)

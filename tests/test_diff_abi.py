"""The entry points DiffUNet / DiffVAE add to the C ABI - the five `linear` output kernels (csrc/elementwise.hip) and the 1x1 head
(csrc/head1x1.hip) - checked without a GPU: exported, declared in the header with their source lines, bound, wrapped, and every
argument-validation case returns UNETRIR_EINVAL (10001) before the device is touched."""
import ctypes as C
import os

LINEAR = ("unetrir_linear_loss_ex_f32", "unetrir_linear_loss_ex_bf16", "unetrir_linear_nchw_f32", "unetrir_linear_bwd_f32",
          "unetrir_linear_bwd_bf16")
HEAD = ("unetrir_head1x1_supported", "unetrir_head1x1_fwd_bf16", "unetrir_head1x1_bwd_ws_bytes", "unetrir_head1x1_bwd_bf16")
EINVAL = 10001
P = 0x7F0000001000          # a non-null, 16-byte aligned address: validation must return before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import unet_rir_amd
    return unet_rir_amd, unet_rir_amd._lib.lib()


def test_new_symbols_are_exported_declared_bound_and_wrapped():
    U, L = _lib()
    header = open(os.path.join(ROOT, "include", "unetrir.h")).read()
    for n in LINEAR + HEAD:
        assert hasattr(L, n), n
        assert n in U._lib.EXPORTS, n
        assert n + "(" in header, n
    assert "diff_u_net.py:247" in header and "diff_vae.py:385" in header          # the entry points cite their source lines
    for n in ("linear_loss", "linear_nchw", "linear_bwd", "head1x1_supported", "head1x1_fwd", "head1x1_bwd", "head1x1_bwd_ws_bytes"):
        assert callable(getattr(U.ops, n)), n
    assert "head1x1.hip" in U.build.SOURCES
    assert L.unetrir_abi_version() == 1
    assert len(U._lib.Config._fields_) == 18                # no new kernel-selection switch
    for n in ("DiffUNet", "DiffUNetEngine", "DiffVAE", "DiffVAEEngine"):
        assert n in U.__all__ and getattr(U, n) is not None
    assert U.DiffUNetEngine.output_act == "linear" and U.DiffVAEEngine.output_act == "linear"
    assert U.AENetEngine.output_act == "relu1" and U.UNetGraphEngine.output_act == "sigmoid" and U.VAEEngine.output_act == "sigmoid"


def test_linear_entry_points_validate_as_their_relu1_counterparts():
    _, L = _lib()
    need = L.unetrir_loss_ws_bytes(64)
    for fn in (L.unetrir_linear_loss_ex_f32, L.unetrir_linear_loss_ex_bf16):
        assert fn(None, 4, P, None, None, 1, 8, 8, 0.9, 1.0, P, P, P, P, need, None) == EINVAL
        assert fn(P, 1, P, None, None, 1, 8, 8, 0.9, 1.0, P, P, P, P, need, None) == EINVAL
        assert fn(P, 4, P, None, None, 1, 8, 8, 0.9, 1.0, P, P, P, P, need - 8, None) == EINVAL
        assert fn(P, 4, P, None, None, 1, 0, 8, 0.9, 1.0, P, P, P, P, need, None) == EINVAL
    assert L.unetrir_linear_nchw_f32(None, 4, 1, 8, 8, P, None) == EINVAL and L.unetrir_linear_nchw_f32(P, 4, 1, 8, 0, P, None) == EINVAL
    assert L.unetrir_linear_nchw_f32(P, 1, 1, 8, 8, P, None) == EINVAL
    for fn in (L.unetrir_linear_bwd_f32, L.unetrir_linear_bwd_bf16):
        assert fn(P, None, 1, 8, 8, P, None) == EINVAL and fn(P, P, 0, 8, 8, P, None) == EINVAL and fn(None, P, 1, 8, 8, P, None) == EINVAL


def test_head1x1_predicate_and_workspace_query():
    U, L = _lib()
    for c in (8, 16, 32, 40, 64, 248, 256):
        m = L.unetrir_head1x1_supported(c)
        assert 0 <= m <= 3 and U.ops.head1x1_supported(c) == m, c
        assert L.unetrir_head1x1_bwd_ws_bytes(2, 8, 8, c) > 0, c
    for c in (0, -8, 4, 12, 36, 264, 512):                     # not a multiple of 8, or outside 8 .. 256
        assert L.unetrir_head1x1_supported(c) == 0, c
        assert L.unetrir_head1x1_bwd_ws_bytes(2, 8, 8, c) == 0, c
    for bhw in ((0, 8, 8), (2, 0, 8), (2, 8, -1)):
        assert L.unetrir_head1x1_bwd_ws_bytes(*bhw, 32) == 0, bhw
    # a function of (B, H, W, C) alone: one slab of 2 C + 8 floats per block of pixels, 1024 blocks at most
    assert L.unetrir_head1x1_bwd_ws_bytes(1, 1, 1, 8) == 24 * 4
    assert L.unetrir_head1x1_bwd_ws_bytes(32, 144, 160, 32) == 1024 * 72 * 4


def test_head1x1_entry_points_validate_their_arguments():
    _, L = _lib()
    fwd = lambda x=P, ldx=32, B=2, H=8, W=8, Cc=32, w=P, bias=P, y=P, ldy=4: L.unetrir_head1x1_fwd_bf16(x, ldx, B, H, W, Cc, w, bias, y, ldy, None)
    for kw in (dict(x=None), dict(w=None), dict(bias=None), dict(y=None), dict(B=0), dict(H=0), dict(W=-1), dict(Cc=12), dict(Cc=4), dict(Cc=0),
               dict(Cc=264, ldx=264), dict(ldx=24), dict(ldx=36), dict(ldy=3), dict(ldy=2), dict(x=P + 8), dict(w=P + 4), dict(bias=P + 8),
               dict(y=P + 4)):
        assert fwd(**kw) == EINVAL, kw
    need = L.unetrir_head1x1_bwd_ws_bytes(2, 8, 8, 32)
    bwd = lambda x=P, ldx=32, dy=P, lddy=8, B=2, H=8, W=8, Cc=32, w=P, dx=P, lddx=32, dw=P, db=P, ws=P, ws_bytes=need: \
        L.unetrir_head1x1_bwd_bf16(x, ldx, dy, lddy, B, H, W, Cc, w, dx, lddx, dw, db, ws, ws_bytes, None)
    for kw in (dict(x=None), dict(dy=None), dict(w=None), dict(dx=None), dict(dw=None), dict(db=None), dict(ws=None), dict(B=0), dict(H=-2),
               dict(W=0), dict(Cc=12), dict(Cc=264, ldx=264, lddx=264), dict(ldx=24), dict(ldx=36), dict(lddx=24), dict(lddx=44),
               dict(lddy=7), dict(lddy=2), dict(x=P + 8), dict(dy=P + 2), dict(w=P + 4), dict(dx=P + 8), dict(dw=P + 4), dict(db=P + 8),
               dict(ws=P + 4), dict(ws_bytes=need - 4), dict(ws_bytes=0)):
        assert bwd(**kw) == EINVAL, kw


def test_exports_equal_the_header():
    import re
    U, _ = _lib()
    header = open(os.path.join(ROOT, "include", "unetrir.h")).read()
    declared = set(re.findall(r"\b(unetrir_[a-z0-9_]+)\s*\(", header))
    assert set(U._lib.EXPORTS) == declared, (set(U._lib.EXPORTS) ^ declared)

"""The 2x2 stride-2 entry points of the C ABI (csrc/conv2x2.hip), checked without a GPU: exported, declared in the header with their
Keras call sites, bound, wrapped, and every argument-validation case returns UNETRIR_EINVAL (10001) before the device is touched."""
import ctypes as C
import os

NEW = ("unetrir_conv2x2s2_supported_bf16", "unetrir_conv2x2s2_fwd_bf16", "unetrir_conv2x2s2_dgrad_bf16", "unetrir_conv2x2s2_wgrad_ws_bytes",
       "unetrir_conv2x2s2_wgrad_bf16", "unetrir_conv2x2s2_wgrad_partials_bf16", "unetrir_conv2x2s2_transpose_supported_bf16",
       "unetrir_conv2x2s2_transpose_fwd_bf16", "unetrir_conv2x2s2_transpose_dgrad_bf16", "unetrir_conv2x2s2_transpose_wgrad_ws_bytes",
       "unetrir_conv2x2s2_transpose_wgrad_bf16", "unetrir_conv2x2s2_transpose_wgrad_partials_bf16")
EINVAL = 10001
P = 0x7F0000001000          # a non-null, 16-byte aligned address: validation must return before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import unet_rir_amd
    return unet_rir_amd, unet_rir_amd._lib.lib()


def test_new_symbols_are_exported_declared_bound_and_wrapped():
    U, L = _lib()
    header = open(os.path.join(ROOT, "include", "unetrir.h")).read()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in U._lib.EXPORTS, n
        assert n + "(" in header, n
    assert "ae_net.py:273-279" in header and "ae_net.py:301-307" in header          # the entry points cite their source lines
    for n in ("conv2x2s2_supported", "conv2x2s2_fwd", "conv2x2s2_dgrad", "conv2x2s2_wgrad", "conv2x2s2_wgrad_ws_bytes",
              "conv2x2s2_transpose_fwd", "conv2x2s2_transpose_dgrad", "conv2x2s2_transpose_wgrad", "conv2x2s2_transpose_wgrad_ws_bytes"):
        assert callable(getattr(U.ops, n)), n
    assert "conv2x2.hip" in U.build.SOURCES
    assert L.unetrir_abi_version() == 1
    assert len(U._lib.Config._fields_) == 18                # the kernels are reached through their entry points, not through a switch


def G(B=2, H=8, W=8, Cin=32, Cout=64, k=2, stride=2):
    from unet_rir_amd._lib import ConvGeom
    return ConvGeom(B, H, W, Cin, Cout, k, stride)


# geometries no pass of a Conv2D(2, strides=2) layer is served for (ld_in = Cin, ld_out = Cout)
BAD_GEOM = (dict(H=7), dict(W=9), dict(k=3), dict(k=1), dict(stride=1), dict(Cin=8), dict(Cout=8), dict(Cin=48), dict(Cout=96),
            dict(Cin=1024), dict(Cout=2048), dict(B=0), dict(H=0))


def test_supported_predicate_and_workspace_query():
    _, L = _lib()
    g = G()
    assert L.unetrir_conv2x2s2_supported_bf16(C.byref(g), 32, 64) == 7                  # forward | data gradient | weight gradient
    assert L.unetrir_conv2x2s2_supported_bf16(C.byref(g), 64, 64) == 7                  # a concat half
    assert L.unetrir_conv2x2s2_transpose_supported_bf16(C.byref(G(H=7, W=5, Cin=64, Cout=32)), 64, 64) == 7      # coarse sizes may be odd
    # the measured rule (profiles/aenet.json): the GEMM forms up to K = 256, the weight gradient always
    assert L.unetrir_conv2x2s2_supported_bf16(C.byref(G(Cin=64, Cout=128)), 64, 128) == 7           # gather K = 256, scatter K = 128
    assert L.unetrir_conv2x2s2_supported_bf16(C.byref(G(Cin=128, Cout=256)), 128, 256) == 2 | 4     # gather K = 512
    assert L.unetrir_conv2x2s2_supported_bf16(C.byref(G(Cin=256, Cout=512)), 256, 512) == 4         # ... and scatter K = 512
    assert L.unetrir_conv2x2s2_transpose_supported_bf16(C.byref(G(Cin=512, Cout=256)), 512, 512) == 4
    assert L.unetrir_conv2x2s2_transpose_supported_bf16(C.byref(G(Cin=256, Cout=128)), 256, 256) == 1 | 4
    assert L.unetrir_conv2x2s2_supported_bf16(C.byref(G(Cin=512, Cout=1024)), 512, 1024) == 4
    assert L.unetrir_conv2x2s2_supported_bf16(None, 32, 64) == 0
    for kw in BAD_GEOM:
        gb = G(**kw)
        assert L.unetrir_conv2x2s2_supported_bf16(C.byref(gb), gb.Cin, gb.Cout) == 0, kw
        assert L.unetrir_conv2x2s2_wgrad_ws_bytes(C.byref(gb)) == 0, kw
    for ld_in, ld_out in ((24, 64), (36, 64), (32, 56), (32, 68)):                      # ld < C, ld % 8 != 0
        assert L.unetrir_conv2x2s2_supported_bf16(C.byref(g), ld_in, ld_out) == 0, (ld_in, ld_out)
    # one slab per 4 blocks of 32 coarse pixels at most: B 4 x 4 = 32 pixels -> one slab of [Cout][2][2][Cin] floats
    assert L.unetrir_conv2x2s2_wgrad_ws_bytes(C.byref(g)) == 64 * 4 * 32 * 4
    assert L.unetrir_conv2x2s2_transpose_wgrad_ws_bytes(C.byref(G(H=4, W=4, Cin=64, Cout=32))) == 64 * 4 * 32 * 4
    # the default AENet's deepest layer at batch 32 (18 x 20 -> 9 x 10, 256 -> 512): slabs of 2 MB, a few tens of them
    big = L.unetrir_conv2x2s2_wgrad_ws_bytes(C.byref(G(B=32, H=18, W=20, Cin=256, Cout=512)))
    assert big % (512 * 4 * 256 * 4) == 0 and 1 <= big // (512 * 4 * 256 * 4) <= 64


def test_gemm_entry_points_validate_their_arguments():
    _, L = _lib()
    fwd = lambda g=None, x=P, ldx=32, w=P, y=P, ldy=64, add=None, ldadd=0: L.unetrir_conv2x2s2_fwd_bf16(
        C.byref(g or G()), x, ldx, w, None, add, ldadd, y, ldy, None)
    dgrad = lambda g=None, dy=P, lddy=64, wt=P, dx=P, lddx=32, add=None, ldadd=0: L.unetrir_conv2x2s2_dgrad_bf16(
        C.byref(g or G()), dy, lddy, wt, add, ldadd, dx, lddx, None)
    tfwd = lambda g=None, x=P, ldx=64, wt=P, y=P, ldy=32: L.unetrir_conv2x2s2_transpose_fwd_bf16(
        C.byref(g or G(H=4, W=4, Cin=64, Cout=32)), x, ldx, wt, None, y, ldy, None)
    tdgrad = lambda g=None, dy=P, lddy=32, w=P, dx=P, lddx=64, add=None, ldadd=0: L.unetrir_conv2x2s2_transpose_dgrad_bf16(
        C.byref(g or G(H=4, W=4, Cin=64, Cout=32)), dy, lddy, w, add, ldadd, dx, lddx, None)
    for kw in BAD_GEOM:
        assert fwd(g=G(**kw)) == EINVAL, kw
        assert dgrad(g=G(**kw)) == EINVAL, kw
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(ldx=24), dict(ldx=36), dict(ldy=56), dict(ldy=68), dict(x=P + 8), dict(w=P + 2),
               dict(y=P + 4), dict(add=P, ldadd=32), dict(add=P, ldadd=68), dict(add=P + 8, ldadd=64)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(dy=None), dict(wt=None), dict(dx=None), dict(lddy=56), dict(lddx=24), dict(lddx=36), dict(dx=P + 8),
               dict(add=P, ldadd=24)):
        assert dgrad(**kw) == EINVAL, kw
    for kw in (dict(x=None), dict(wt=None), dict(y=None), dict(ldx=56), dict(ldy=24), dict(ldy=36), dict(g=G(H=4, W=4, Cin=8, Cout=32)),
               dict(g=G(H=4, W=4, Cin=64, Cout=32, k=3)), dict(g=G(H=4, W=4, Cin=64, Cout=1024))):
        assert tfwd(**kw) == EINVAL, kw
    for kw in (dict(dy=None), dict(w=None), dict(dx=None), dict(lddy=24), dict(lddx=56), dict(add=P, ldadd=32), dict(dy=P + 8)):
        assert tdgrad(**kw) == EINVAL, kw


def test_weight_gradient_entry_points_validate_their_arguments():
    U, L = _lib()
    from unet_rir_amd._lib import ReduceDesc
    need = L.unetrir_conv2x2s2_wgrad_ws_bytes(C.byref(G()))
    wg = lambda g=None, x=P, ldx=32, dy=P, lddy=64, dw=P, reg=0.5, w=P, ws=P, ws_bytes=need: L.unetrir_conv2x2s2_wgrad_bf16(
        C.byref(g or G()), x, ldx, dy, lddy, dw, reg, w, ws, ws_bytes, None)
    for kw in BAD_GEOM:
        assert wg(g=G(**kw)) == EINVAL, kw
    for kw in (dict(x=None), dict(dy=None), dict(dw=None), dict(w=None), dict(ws=None), dict(ws_bytes=need - 4), dict(ws_bytes=0),
               dict(ldx=24), dict(ldx=36), dict(lddy=56), dict(x=P + 8), dict(dy=P + 4)):
        assert wg(**kw) == EINVAL, kw
    gt = G(H=4, W=4, Cin=64, Cout=32)
    need_t = L.unetrir_conv2x2s2_transpose_wgrad_ws_bytes(C.byref(gt))
    twg = lambda x=P, ldx=64, dy=P, lddy=32, dw=P, reg=0.5, w=P, ws=P, ws_bytes=need_t: L.unetrir_conv2x2s2_transpose_wgrad_bf16(
        C.byref(gt), x, ldx, dy, lddy, dw, reg, w, ws, ws_bytes, None)
    for kw in (dict(x=None), dict(dy=None), dict(dw=None), dict(w=None), dict(ws=None), dict(ws_bytes=need_t - 4), dict(ldx=56),
               dict(lddy=24)):
        assert twg(**kw) == EINVAL, kw
    # the deferred forms need a descriptor to fill; with one, a refused call leaves it empty (nsplit == 0: nothing to reduce)
    assert L.unetrir_conv2x2s2_wgrad_partials_bf16(C.byref(G()), P, 32, P, 64, P, 0.5, P, P, need, None, None) == EINVAL
    assert L.unetrir_conv2x2s2_transpose_wgrad_partials_bf16(C.byref(gt), P, 64, P, 32, P, 0.5, P, P, need_t, None, None) == EINVAL
    d = ReduceDesc()
    d.nsplit = 7
    assert L.unetrir_conv2x2s2_wgrad_partials_bf16(C.byref(G()), P, 32, P, 64, P, 0.5, P, P, need - 4, C.byref(d), None) == EINVAL
    assert d.nsplit == 0


def test_no_generic_fallback_exists_for_a_pixel_stride_that_is_no_multiple_of_8():
    """`supported` is 0 for ld % 8 != 0, and the fallback a caller would take refuses the same buffers (bf16 rows are 16-byte units
    everywhere: ops.Act cannot even describe such a buffer), so this case ends in UNETRIR_EINVAL on either path."""
    _, L = _lib()
    g = G()
    assert L.unetrir_conv2x2s2_supported_bf16(C.byref(g), 36, 64) == 0
    assert L.unetrir_conv2x2s2_fwd_bf16(C.byref(g), P, 36, P, None, None, 0, P, 64, None) == EINVAL
    assert L.unetrir_conv2d_fwd_bf16(C.byref(g), P, 36, P, None, None, 0, P, 64, None) == EINVAL


def test_relu1_entry_points_are_declared_bound_and_validate():
    U, L = _lib()
    header = open(os.path.join(ROOT, "include", "unetrir.h")).read()
    for n in ("unetrir_relu1_loss_ex_f32", "unetrir_relu1_loss_ex_bf16", "unetrir_relu1_nchw_f32", "unetrir_relu1_bwd_f32", "unetrir_relu1_bwd_bf16"):
        assert hasattr(L, n) and n in U._lib.EXPORTS and n + "(" in header, n
    assert "ae_net.py:249" in header and U.AENet is not None and U.AENetEngine.output_act == "relu1" and U.UNetGraphEngine.output_act == "sigmoid"
    need = L.unetrir_loss_ws_bytes(64)
    for fn in (L.unetrir_relu1_loss_ex_f32, L.unetrir_relu1_loss_ex_bf16):
        assert fn(None, 4, P, None, None, 1, 8, 8, 0.9, 1.0, P, P, P, P, need, None) == EINVAL
        assert fn(P, 1, P, None, None, 1, 8, 8, 0.9, 1.0, P, P, P, P, need, None) == EINVAL
        assert fn(P, 4, P, None, None, 1, 8, 8, 0.9, 1.0, P, P, P, P, need - 8, None) == EINVAL
        assert fn(P, 4, P, None, None, 1, 0, 8, 0.9, 1.0, P, P, P, P, need, None) == EINVAL
    assert L.unetrir_relu1_nchw_f32(None, 4, 1, 8, 8, P, None) == EINVAL and L.unetrir_relu1_nchw_f32(P, 4, 1, 8, 0, P, None) == EINVAL
    for fn in (L.unetrir_relu1_bwd_f32, L.unetrir_relu1_bwd_bf16):
        assert fn(P, None, 1, 8, 8, P, None) == EINVAL and fn(P, P, 0, 8, 8, P, None) == EINVAL

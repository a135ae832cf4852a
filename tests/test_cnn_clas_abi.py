"""The entry points of csrc/cnn_clas.hip are exported, declared in include/unetrir.h, bound in _lib and wrapped in ops, and refuse
every bad argument with UNETRIR_EINVAL (10001) before the device is touched - checked here without a GPU: the pointers are the
non-null, 16-byte aligned dummy 16, so only the argument checks stand between the call and a launch."""
import ctypes as C

import pytest

from test_abi import declared_symbols

EINVAL = 10001
NEW = ["unetrir_conv3x3_valid_fwd_f32", "unetrir_conv3x3_valid_dgrad_f32", "unetrir_conv3x3_valid_wgrad_ws_bytes",
       "unetrir_conv3x3_valid_wgrad_f32", "unetrir_avgpool2_fwd_f32", "unetrir_avgpool2_bwd_f32", "unetrir_gap_fwd_f32",
       "unetrir_gap_bwd_f32", "unetrir_softmax_ce_f32", "unetrir_softmax_fwd_f32", "unetrir_softmax_bwd_f32"]
WRAPPED = ["conv3x3_valid_fwd", "conv3x3_valid_dgrad", "conv3x3_valid_wgrad_ws_bytes", "conv3x3_valid_wgrad", "avgpool2_fwd",
           "avgpool2_bwd", "gap_fwd", "gap_bwd", "softmax_ce", "softmax_fwd", "softmax_bwd"]
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
    for n in WRAPPED:
        assert callable(getattr(U.ops, n)), n
    assert len(U._lib.Config._fields_) == 18 and L.unetrir_abi_version() == 1
    for n in ("deep_CNN", "DeepCNNEngine"):
        assert n in U.__all__ and getattr(U, n) is not None


def _g(B=2, H=9, W=11, Cin=16, Cout=32, k=3, stride=1):
    from unet_rir_amd._lib import ConvGeom
    return ConvGeom(B, H, W, Cin, Cout, k, stride)


BAD_GEOMS = [dict(H=2), dict(W=2), dict(Cin=8), dict(Cin=64), dict(Cout=24), dict(Cout=128), dict(k=5), dict(stride=2), dict(B=0)]


@pytest.mark.parametrize("bad", BAD_GEOMS, ids=[str(b) for b in BAD_GEOMS])
def test_convolution_refuses_bad_geometry(L, bad):
    g = _g(**bad)
    ws = max(L.unetrir_conv3x3_valid_wgrad_ws_bytes(C.byref(_g())), 1)
    assert L.unetrir_conv3x3_valid_fwd_f32(C.byref(g), P, g.Cin, P, P, 1, P, g.Cout, None) == EINVAL
    assert L.unetrir_conv3x3_valid_dgrad_f32(C.byref(g), P, g.Cout, P, g.Cout, 1, P, P, g.Cin, None) == EINVAL
    assert L.unetrir_conv3x3_valid_wgrad_f32(C.byref(g), P, g.Cin, P, g.Cout, P, g.Cout, 1, P, P, P, ws, None) == EINVAL
    assert L.unetrir_conv3x3_valid_wgrad_ws_bytes(C.byref(g)) == 0


def test_convolution_refuses_bad_pointers_strides_and_workspace(L):
    g = _g()
    need = L.unetrir_conv3x3_valid_wgrad_ws_bytes(C.byref(g))
    assert need > 0 and need % ((g.Cout * 9 * g.Cin + g.Cout) * 4) == 0
    fwd = lambda x=P, ldx=16, w=P, b=P, y=P, ldy=32: L.unetrir_conv3x3_valid_fwd_f32(C.byref(g), x, ldx, w, b, 1, y, ldy, None)
    for kw in (dict(x=None), dict(w=None), dict(b=None), dict(y=None), dict(ldx=12), dict(ldx=18), dict(ldy=28), dict(ldy=34), dict(x=20), dict(y=24)):
        assert fwd(**kw) == EINVAL, kw
    dg = lambda dy=P, lddy=32, y=P, ldy=32, relu=1, wt=P, dx=P, lddx=16: L.unetrir_conv3x3_valid_dgrad_f32(
        C.byref(g), dy, lddy, y, ldy, relu, wt, dx, lddx, None)
    for kw in (dict(dy=None), dict(y=None), dict(wt=None), dict(dx=None), dict(lddy=16), dict(ldy=30), dict(lddx=12), dict(dx=8)):
        assert dg(**kw) == EINVAL, kw
    wg = lambda x=P, ldx=16, dy=P, lddy=32, y=P, ldy=32, relu=1, dw=P, db=P, ws=P, n=need: L.unetrir_conv3x3_valid_wgrad_f32(
        C.byref(g), x, ldx, dy, lddy, y, ldy, relu, dw, db, ws, n, None)
    for kw in (dict(x=None), dict(dy=None), dict(y=None), dict(dw=None), dict(db=None), dict(ws=None), dict(n=need - 1), dict(n=0),
               dict(ldx=8), dict(lddy=31), dict(ws=8)):
        assert wg(**kw) == EINVAL, kw


def test_workspace_depends_on_the_geometry_alone(L):
    """The split is a function of (B, H, W, Cin, Cout) as include/unetrir.h states it: slabs of r = ceil(R / min(R, 524288 / (Cin Cout)))
    whole output rows, R = B (H - 2) of them - about eight waves per SIMD in flight, one (co, ci) pair per lane."""
    for B, H, W, ci, co in ((32, 144, 160, 4, 16), (32, 71, 79, 16, 32), (32, 34, 38, 32, 64), (2, 3, 3, 16, 32), (3, 21, 24, 4, 16)):
        g = _g(B, H, W, ci, co)
        R = B * (H - 2)
        r = -(-R // min(R, max(1, 524288 // (ci * co))))
        a, b = L.unetrir_conv3x3_valid_wgrad_ws_bytes(C.byref(g)), L.unetrir_conv3x3_valid_wgrad_ws_bytes(C.byref(g))
        assert a == b == -(-R // r) * (co * 9 * ci + co) * 4, (B, H, W, ci, co)


def test_pooling_refuses_bad_arguments(L):
    pool_f = lambda x=P, ldx=16, B=2, H=7, W=9, C_=16, aff=P, y=P, ldy=16: L.unetrir_avgpool2_fwd_f32(x, ldx, B, H, W, C_, aff, y, ldy, None)
    pool_b = lambda dy=P, lddy=16, B=2, H=7, W=9, C_=16, dx=P, lddx=16: L.unetrir_avgpool2_bwd_f32(dy, lddy, B, H, W, C_, dx, lddx, None)
    for kw in (dict(H=1), dict(W=1), dict(H=1, W=2), dict(B=0), dict(C_=6), dict(C_=0), dict(ldx=12), dict(ldy=18), dict(x=None), dict(y=None),
               dict(aff=8)):
        assert pool_f(**kw) == EINVAL, kw
    for kw in (dict(H=1), dict(W=1), dict(B=0), dict(C_=6), dict(lddy=12), dict(lddx=18), dict(dy=None), dict(dx=None), dict(dx=4)):
        assert pool_b(**kw) == EINVAL, kw
    gap_f = lambda x=P, ldx=64, B=2, H=1, W=2, C_=64, aff=None, y=P, ldy=64: L.unetrir_gap_fwd_f32(x, ldx, B, H, W, C_, aff, y, ldy, None)
    gap_b = lambda dy=P, lddy=64, B=2, H=1, W=2, C_=64, dx=P, lddx=64: L.unetrir_gap_bwd_f32(dy, lddy, B, H, W, C_, dx, lddx, None)
    for kw in (dict(H=0), dict(W=0), dict(B=0), dict(C_=62), dict(C_=1028, ldx=1028, ldy=1028), dict(ldx=60), dict(ldy=66), dict(x=None), dict(y=None)):
        assert gap_f(**kw) == EINVAL, kw
    for kw in (dict(H=0), dict(W=0), dict(B=0), dict(C_=62), dict(lddy=60), dict(lddx=66), dict(dy=None), dict(dx=None)):
        assert gap_b(**kw) == EINVAL, kw


def test_softmax_refuses_bad_arguments(L):
    ce = lambda z=P, ldl=8, t=P, B=3, K=5, p=P, d=P, ldd=8, lo=P, ac=P: L.unetrir_softmax_ce_f32(z, ldl, t, B, K, 0.5, p, d, ldd, lo, ac, None)
    for kw in (dict(K=0), dict(K=1025, ldl=1028, ldd=1028), dict(K=-1), dict(B=0), dict(ldl=4), dict(ldd=4), dict(z=None), dict(t=None), dict(p=None),
               dict(d=None), dict(lo=None), dict(ac=None)):
        assert ce(**kw) == EINVAL, kw
    for K, ld in ((0, 8), (1025, 1028), (5, 4)):
        assert L.unetrir_softmax_fwd_f32(P, ld, 3, K, P, None) == EINVAL
        assert L.unetrir_softmax_bwd_f32(P, P, 3, K, P, ld, None) == EINVAL
    assert L.unetrir_softmax_fwd_f32(None, 8, 3, 5, P, None) == EINVAL and L.unetrir_softmax_fwd_f32(P, 8, 0, 5, P, None) == EINVAL
    assert L.unetrir_softmax_bwd_f32(P, None, 3, 5, P, 8, None) == EINVAL and L.unetrir_softmax_bwd_f32(P, P, 0, 5, P, 8, None) == EINVAL

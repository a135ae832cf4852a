"""The vector-quantiser entry points of the C ABI (csrc/vq.hip), checked without a GPU: exported, declared in the header, bound,
wrapped, and every argument-validation case of include/unetrir.h returns UNETRIR_EINVAL (10001) before the device is touched."""
import os

NEW = ("unetrir_vq_ws_bytes", "unetrir_vq_fwd_f32", "unetrir_vq_bwd_f32")
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
    assert "vqvae.py:61-98" in header and "vqvae.py:89" in header          # the entry points cite their source lines
    for n in ("vq_fwd", "vq_bwd", "vq_workspace"):
        assert callable(getattr(U.ops, n)), n
    assert L.unetrir_abi_version() == 1
    assert U.VQVAE.ENGINE is U.VQVAEEngine
    assert "vq.hip" in U.build.SOURCES
    assert L.unetrir_vq_ws_bytes() >= 16 + 8 * 1024


def _fwd(L, x=P, rows=6, ld=8, C=8, D=4, E=P, K=8, idx=P, y=P, ld_y=8, out=P, ws=P, ws_bytes=None):
    return L.unetrir_vq_fwd_f32(x, rows, ld, C, D, E, K, 0.25, 1.0, idx, y, ld_y, out, ws,
                                L.unetrir_vq_ws_bytes() if ws_bytes is None else ws_bytes, None)


def _bwd(L, x=P, rows=6, ld=8, C=8, D=4, idx=P, E=P, K=8, dy=P, ld_dy=8, dx=P, ld_dx=8, dE=P):
    return L.unetrir_vq_bwd_f32(x, rows, ld, C, D, idx, E, K, dy, ld_dy, 0.25, 1.0, dx, ld_dx, dE, None)


GEOMETRY = (dict(D=0), dict(D=2), dict(D=6), dict(D=68, C=68, ld=68), dict(D=128, C=128, ld=128),        # D % 4, 4 <= D <= 64
            dict(K=0), dict(K=2), dict(K=6), dict(K=516), dict(K=1024), dict(K=-8),                      # K % 4, 4 <= K <= 512
            dict(C=12, ld=12, D=8), dict(C=4, D=8), dict(C=0),                                           # C % D == 0
            dict(ld=4), dict(ld=10), dict(ld=9),                                                         # ld >= C, ld % 4 == 0
            dict(rows=0), dict(rows=-3), dict(rows=1 << 40))                                             # rows > 0 (and countable)


def test_fwd_argument_validation():
    _, L = _lib()
    for kw in (dict(x=None), dict(E=None), dict(idx=None), dict(y=None), dict(out=None), dict(ws=None)) + GEOMETRY + (
            dict(ld_y=4), dict(ld_y=10), dict(ws_bytes=64), dict(x=P + 4), dict(y=P + 8), dict(ws=P + 4)):
        assert _fwd(L, **kw) == EINVAL, kw


def test_bwd_argument_validation():
    _, L = _lib()
    for kw in (dict(x=None), dict(idx=None), dict(E=None), dict(dy=None), dict(dx=None), dict(dE=None)) + GEOMETRY + (
            dict(ld_dy=4), dict(ld_dy=10), dict(ld_dx=4), dict(ld_dx=10), dict(x=P + 4), dict(dy=P + 8), dict(dx=P + 4)):
        assert _bwd(L, **kw) == EINVAL, kw

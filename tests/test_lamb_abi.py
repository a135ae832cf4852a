"""The LAMB entry points of the C ABI (csrc/lamb.hip; tfa.optimizers.LAMB of trainer.py:37-38), checked without a GPU: exported,
declared in the header with their source lines, bound and wrapped; the host-side table builder; and every argument-validation case
returns UNETRIR_EINVAL (10001) before anything is launched."""
import ctypes as C
import os

NEW = ("unetrir_lamb_chunk_elems", "unetrir_lamb_table_init", "unetrir_lamb_ws_bytes", "unetrir_lamb_f32", "unetrir_lamb_dev_f32")
EINVAL = 10001
P = 0x7F0000001000          # a non-null, 16-byte aligned address: validation must return before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import unet_rir_amd
    return unet_rir_amd, unet_rir_amd._lib.lib()


def _table(L, rows):
    from unet_rir_amd._lib import LambSeg
    segs = (LambSeg * len(rows))()
    for s_, (off, cnt, slot, flags) in zip(segs, rows):
        s_.offset, s_.count, s_.slot, s_.flags = off, cnt, slot, flags
    return segs


def test_new_symbols_are_exported_declared_bound_and_wrapped():
    U, L = _lib()
    header = open(os.path.join(ROOT, "include", "unetrir.h")).read()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in U._lib.EXPORTS, n
        assert n + "(" in header, n
    assert "trainer.py:37-38" in header and "PARITY UNPINNED" in header
    for n in ("lamb", "lamb_dev", "lamb_ws_bytes", "lamb_chunk_elems", "make_lamb_table", "LambTable"):
        assert callable(getattr(U.ops, n)), n
    assert "lamb.hip" in U.build.SOURCES and U.LAMB is not None
    assert L.unetrir_abi_version() == 1
    assert C.sizeof(U._lib.LambSeg) == 32


def test_table_builder_numbers_chunks_from_each_variable_start():
    U, L = _lib()
    Cn = L.unetrir_lamb_chunk_elems()
    assert Cn > 0 and Cn % 4 == 0
    rows = [(0, 2, 64, 3), (64, Cn, Cn, 3), (64 + Cn, Cn + 4, Cn + 64, 1), (128 + 2 * Cn, 3 * Cn + 100, 3 * Cn + 128, 0)]
    segs = _table(L, rows)
    n = L.unetrir_lamb_table_init(segs, len(rows), None, 0)
    assert n == 1 + 1 + 2 + 4
    assert [s_.chunk0 for s_ in segs] == [0, 1, 2, 4]
    cmap = (C.c_int32 * n)()
    assert L.unetrir_lamb_table_init(segs, len(rows), C.cast(cmap, C.c_void_p), n) == n
    assert list(cmap) == [0, 1, 2, 2, 3, 3, 3, 3]
    assert L.unetrir_lamb_table_init(segs, len(rows), C.cast(cmap, C.c_void_p), n - 1) == -1          # the map would not fit
    assert L.unetrir_lamb_ws_bytes(len(rows), n) == 16 * n + 4 * len(rows)
    assert L.unetrir_lamb_ws_bytes(0, n) == 0 and L.unetrir_lamb_ws_bytes(4, 0) == 0
    for bad in ([(0, 0, 64, 3)], [(0, 65, 64, 3)], [(2, 2, 64, 3)], [(0, 2, 62, 3)], [(0, 2, 64, 4)], [(0, 2, 64, 3), (128, 2, 64, 3)],
                [(0, 2, 64, 3), (32, 2, 64, 3)], [(-64, 2, 64, 3)]):
        assert L.unetrir_lamb_table_init(_table(L, bad), len(bad), None, 0) == -1, bad
    assert L.unetrir_lamb_table_init(None, 1, None, 0) == -1 and L.unetrir_lamb_table_init(segs, 0, None, 0) == -1


def test_step_entry_points_validate_their_arguments():
    U, L = _lib()
    rows = [(0, 2, 64, 3), (64, 46, 64, 3), (128, 300, 320, 3)]
    segs = _table(L, rows)
    n = L.unetrir_lamb_table_init(segs, 3, None, 0)
    need = L.unetrir_lamb_ws_bytes(3, n)

    def host(theta=P, g=P, m=P, v=P, sh=segs, sd=P, cs=P, n_seg=3, lo=0, hi=448, ws=P, ws_bytes=need):
        return L.unetrir_lamb_f32(theta, g, m, v, sh, sd, cs, n_seg, lo, hi, 1e-3, 0.9, 0.999, 1e-6, 0.0, 0.1, 0.001, 1.0, ws, ws_bytes, None)

    def dev(theta=P, g=P, m=P, v=P, sh=segs, sd=P, cs=P, n_seg=3, lo=0, hi=448, ws=P, ws_bytes=need, state=P, cfg=P):
        return L.unetrir_lamb_dev_f32(theta, g, m, v, sh, sd, cs, n_seg, lo, hi, 0.0, state, cfg, ws, ws_bytes, None)

    cases = (dict(theta=None), dict(g=None), dict(m=None), dict(v=None), dict(sh=None), dict(sd=None), dict(cs=None), dict(ws=None),
             dict(n_seg=0), dict(n_seg=-1), dict(theta=P + 4), dict(g=P + 8), dict(m=P + 4), dict(v=P + 12), dict(ws=P + 4),
             dict(ws_bytes=need - 1), dict(ws_bytes=0),
             # a range that does not begin and end on a variable boundary
             dict(lo=32), dict(lo=4), dict(hi=447), dict(hi=384), dict(hi=512), dict(lo=64, hi=64), dict(lo=128, hi=64), dict(lo=-64),
             dict(lo=448, hi=448))
    for kw in cases:
        assert host(**kw) == EINVAL, kw
        assert dev(**kw) == EINVAL, kw
    assert dev(state=None) == EINVAL and dev(cfg=None) == EINVAL


def test_python_side_table_and_hyperparameters():
    """ops.LambTable refuses a table the library refuses; unet_rir_amd.LAMB mirrors tfa's constructor and resolves its exclusion lists
    by re.search on the parameter names."""
    import pytest
    U, L = _lib()
    o = U.LAMB()
    assert (o.learning_rate, o.beta_1, o.beta_2, o.epsilon, o.weight_decay) == (0.001, 0.9, 0.999, 1e-6, 0.0)
    assert o.exclude_from_weight_decay is None and o.exclude_from_layer_adaptation is None and o.decayed("x.bias") and o.adapted("x.bias")
    o = U.LAMB(weight_decay=0.01, exclude_from_weight_decay=["bias", "^bn"], exclude_from_layer_adaptation=["kernel$"])
    assert not o.decayed("enc0.bias") and not o.decayed("bn3.gamma") and o.decayed("enc0.kernel") and o.decayed("x.bn")
    assert o.adapted("enc0.bias") and not o.adapted("enc0.kernel")
    with pytest.raises(ValueError):
        U.ops.LambTable([(0, 2, 64, True, True), (128, 2, 64, True, True)], "cpu")

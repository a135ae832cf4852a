"""Host-side operator wrappers: torch tensors (device memory, streams) -> the C ABI.

Each function mirrors one Keras call site of the reference graph and forwards to the HIP
library.  PyTorch is used for device memory and streams only; no arithmetic happens here.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ConvGeom, check


class Act:
    """An NHWC activation view (fp32 or bf16 storage): channels [c0, c0+C) of a [B,H,W,ld] device buffer.
    A channel-concat (dl_models/u_net.py:308) is two Acts over one buffer."""
    __slots__ = ("base", "B", "H", "W", "C", "ld", "c0", "ptr", "sfx")

    def __init__(self, base: torch.Tensor, c0: int = 0, C_: int = None):
        if base.dim() != 4 or not base.is_contiguous() or base.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("Act needs a contiguous fp32 or bf16 [B,H,W,ld] tensor")
        self.base = base
        self.B, self.H, self.W, self.ld = base.shape
        self.c0 = c0
        self.C = self.ld - c0 if C_ is None else C_
        self.sfx = "f32" if base.dtype == torch.float32 else "bf16"
        al = 16 // base.element_size()                    # rows and slices start on 16-byte boundaries
        if self.c0 % al or self.ld % al or self.c0 + self.C > self.ld:
            raise ValueError(f"channel offset and pixel stride must be multiples of {al}")
        self.ptr = base.data_ptr() + base.element_size() * c0

    @property
    def P(self):
        return self.B * self.H * self.W

    def slice(self, c0, C_):
        return Act(self.base, self.c0 + c0, C_)

    def dense(self):
        """A contiguous [B,H,W,C] copy (tests / debugging)."""
        return self.base[..., self.c0:self.c0 + self.C].contiguous()


def new_act(B, H, W, C_, device, ld=None, dtype=torch.float32):
    return Act(torch.empty((B, H, W, C_ if ld is None else ld), dtype=dtype, device=device), 0, C_)


def _fn(name, sfx):
    """C entry point `unetrir_<name>_<f32|bf16>`."""
    return getattr(_lib.lib(), f"unetrir_{name}_{sfx}")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if isinstance(t, Act):
        return C.c_void_p(t.ptr)
    return C.c_void_p(t.data_ptr())


def geom(B, H, W, Cin, Cout, k, stride):
    return ConvGeom(B, H, W, Cin, Cout, k, stride)


class Workspace:
    """A reusable scratch buffer (the C ABI never allocates)."""

    def __init__(self, device, nbytes=0):
        self.device = device
        self.buf = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)

    def reserve(self, nbytes):
        if nbytes > self.buf.numel():
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    @property
    def nbytes(self):
        return self.buf.numel()


# ---- Conv2D / Conv2DTranspose --------------------------------------------------------------

def conv3x3s2_packed_elems(N, C_):
    """Elements of the packed copy the stride-2 3x3 forward kernel reads (0: none defined for these channel counts)."""
    return int(_lib.lib().unetrir_conv3x3s2_packed_elems(int(N), int(C_)))


def conv2d_fwd(g, x: Act, w, bias, y: Act, addend: Act = None, w_packed=None):
    """Conv2D(padding='same') forward (dl_models/u_net.py:269-276, :366, :248, :262).  w_packed: the packed copy of a 3x3
    stride-2 kernel (bf16 storage; made by cast_weights_batched), passed beside the plain one."""
    if w_packed is not None:
        check(_lib.lib().unetrir_conv2d_fwd_packed_bf16(C.byref(g), _p(x), x.ld, _p(w), _p(w_packed), _p(bias), _p(addend),
                                                        addend.ld if addend is not None else 0, _p(y), y.ld, _stream()),
              "conv2d_fwd_packed")
        return
    check(_fn("conv2d_fwd", x.sfx)(C.byref(g), _p(x), x.ld, _p(w), _p(bias), _p(addend),
                                            addend.ld if addend is not None else 0, _p(y), y.ld, _stream()),
          "conv2d_fwd")


def conv2d_dgrad(g, dy: Act, wt, dx: Act, addend: Act = None):
    check(_fn("conv2d_dgrad", dy.sfx)(C.byref(g), _p(dy), dy.ld, _p(wt), _p(addend),
                                              addend.ld if addend is not None else 0, _p(dx), dx.ld, _stream()),
          "conv2d_dgrad")


def conv2d_colstat_rows(g, dgrad, x: Act):
    """Rows of fused column statistics the conv kernel serving this layer emits (0: none; bf16 storage only)."""
    if x.sfx != "bf16":
        return 0
    return int(_lib.lib().unetrir_conv2d_colstat_rows_bf16(C.byref(g), int(bool(dgrad)), x.ld))


K3_NAMES = ("tap-table", "conv3x3r", "conv3x3g", "conv3x3g pair", "conv3x3h", "conv3x3s", "conv3x3p", "stem", "patch")


def conv3x3_kernel(g, dgrad, x: Act):
    """Name of the kernel that serves this 3x3 stride-1 layer (bf16 storage) under the switches in effect."""
    return K3_NAMES[int(_lib.lib().unetrir_conv3x3_kernel_id_bf16(C.byref(g), int(bool(dgrad)), x.ld))]


def conv2d_fwd_colstat(g, x: Act, w, bias, y: Act, colstat, addend: Act = None):
    """conv2d_fwd that also writes per-tile (sum, sum of squares) of the stored output: colstat [rows][Cout][2] fp32."""
    check(_lib.lib().unetrir_conv2d_fwd_colstat_bf16(C.byref(g), _p(x), x.ld, _p(w), _p(bias), _p(addend),
                                                     addend.ld if addend is not None else 0, _p(y), y.ld, _p(colstat), _stream()),
          "conv2d_fwd_colstat")


def conv2d_dgrad_colstat(g, dy: Act, wt, dx: Act, colstat, addend: Act = None):
    check(_lib.lib().unetrir_conv2d_dgrad_colstat_bf16(C.byref(g), _p(dy), dy.ld, _p(wt), _p(addend),
                                                       addend.ld if addend is not None else 0, _p(dx), dx.ld, _p(colstat), _stream()),
          "conv2d_dgrad_colstat")


def conv2d_transpose_colstat_rows(g, x: Act):
    """Rows of fused column statistics of a Conv2DTranspose forward launch (0: none; bf16 storage only)."""
    if x.sfx != "bf16":
        return 0
    return int(_lib.lib().unetrir_conv2d_transpose_colstat_rows_bf16(C.byref(g), x.ld))


def conv2d_transpose_fwd_colstat(g, x: Act, wt, bias, y: Act, colstat):
    """conv2d_transpose_fwd that also writes per-tile (sum, sum of squares) of the stored output: colstat [rows][Cout][2] fp32."""
    check(_lib.lib().unetrir_conv2d_transpose_fwd_colstat_bf16(C.byref(g), _p(x), x.ld, _p(wt), _p(bias), _p(y), y.ld, _p(colstat),
                                                               _stream()), "conv2d_transpose_fwd_colstat")


def bn_stats_colstat(colstat, rows, P, C_, gamma, beta, affine, saved, moving_mean=None, moving_var=None, eps=1e-3, momentum=0.99):
    """BatchNormalization() batch statistics from fused conv-epilogue partials."""
    check(_lib.lib().unetrir_bn_stats_colstat(_p(colstat), rows, P, C_, _p(gamma), _p(beta), eps, momentum, _p(moving_mean),
                                              _p(moving_var), _p(affine), _p(saved), _stream()), "bn_stats_colstat")


def bn_colstat_act_add(colstat, rows, x: Act, gamma, beta, affine, saved, y: Act, act=2, addend: Act = None, moving_mean=None,
                       moving_var=None, eps=1e-3, momentum=0.99):
    """BatchNormalization (training) from fused conv-epilogue partials + Add + activation in one call (tensors <= 64 MB: one launch)."""
    check(_fn("bn_colstat_act_add", x.sfx)(_p(colstat), rows, _p(x), x.ld, x.P, x.C, _p(gamma), _p(beta), eps, momentum, _p(moving_mean),
                                            _p(moving_var), _p(affine), _p(saved), int(act), _p(addend),
                                            addend.ld if addend is not None else 0, _p(y), y.ld, _stream()), "bn_colstat_act_add")


def colsum_colstat(colstat, rows, ldc, c0, C_, out):
    """Bias gradient from fused conv-epilogue partials: out[c] = sum over rows of colstat[row][c0 + c][0]."""
    check(_lib.lib().unetrir_colsum_colstat(_p(colstat), rows, ldc, c0, C_, _p(out), _stream()), "colsum_colstat")


def conv2d_wgrad_ws_bytes(g):
    return _lib.lib().unetrir_conv2d_wgrad_ws_bytes(C.byref(g))


def wgrad_defer_supported(storage):
    """Whether the weight gradients of a trunk with this storage type ("f32" | "bf16") can leave their split-K reduction to a
    ReduceBatch (the *_partials_* entry points exist for bf16 storage)."""
    return storage == "bf16"


class ReduceBatch:
    """Deferred split-K reductions of weight gradients (bf16 storage): `conv2d_wgrad(..., defer=batch)` runs the weight-gradient kernel
    only, leaving its fp32 partial slabs in this object's arena; `flush()` reduces everything gathered so far in one launch per 16
    reductions (unetrir_splitk_reduce_batched) - same sums in the same order as the immediate form, bit-identical.  A step has 23
    (configs[1]) to 57 (configs[4]) such reductions of 5-20 us, most of it launch latency.  The owner flushes before anything reads
    the gradients (bucket hand-over, optimizer) and on the stream the weight gradients ran on."""

    def __init__(self, device, arena_bytes, capacity=64, park_max_bytes=None):
        """park_max_bytes: weight gradients whose slabs are larger reduce at once instead (None: park everything).  Measured on
        MI355X (scripts/ab_switch.py attr:park_reduces): the 37.7 MB slab sets of configs[1] are read back from the Infinity Cache when
        reduced at once and from HBM when parked - parking them costs 0.06-0.09 ms per step; the few-MB slab sets of configs[4] gain
        0.1 (side-stream schedule) to 0.57 ms (single stream) from sharing a launch."""
        self.arena = Workspace(device, int(arena_bytes))
        self.descs = (_lib.ReduceDesc * capacity)()
        self.n, self.used, self.capacity = 0, 0, capacity
        self.park_max_bytes = park_max_bytes

    def __len__(self):
        return self.n

    def take(self, nbytes):
        """(pointer, bytes) of a fresh 256-byte-aligned arena region, or None when the arena or the descriptor table is full (the
        caller flushes first, or reduces immediately)."""
        nbytes = -(-int(nbytes) // 256) * 256
        if self.n == 0 and nbytes > self.arena.nbytes:
            self.arena.reserve(4 * nbytes)          # empty: nothing parked points into the old buffer
        if self.n == self.capacity or self.used + nbytes > self.arena.nbytes:
            return None
        ptr = self.arena.buf.data_ptr() + self.used
        self.used += nbytes
        return C.c_void_p(ptr), nbytes

    def flush(self):
        if self.n:
            check(_lib.lib().unetrir_splitk_reduce_batched(self.descs, self.n, _stream()), "splitk_reduce_batched")
        self.n, self.used = 0, 0


def _wgrad(name, g, x: Act, dy: Act, dw, ws: Workspace, reg, w, defer, need):
    if defer is not None and x.sfx == "bf16" and (defer.park_max_bytes is None or need <= defer.park_max_bytes):
        got = defer.take(need)
        if got is None and len(defer):
            defer.flush()                  # arena or table full: reduce what is there (same stream), then defer this one
            got = defer.take(need)
        if got is not None:
            ptr, nbytes = got
            check(getattr(_lib.lib(), f"unetrir_{name}_partials_bf16")(C.byref(g), _p(x), x.ld, _p(dy), dy.ld, _p(dw), float(reg), _p(w), ptr, nbytes,
                                                                       C.byref(defer.descs[defer.n]), _stream()), name + "_partials")
            if defer.descs[defer.n].nsplit:
                defer.n += 1
            else:
                defer.used -= nbytes       # written straight into dw: the region is free again
            return
    ws.reserve(need)
    check(_fn(name, x.sfx)(C.byref(g), _p(x), x.ld, _p(dy), dy.ld, _p(dw), float(reg), _p(w), ws.ptr, ws.nbytes, _stream()), name)


def conv2d_wgrad(g, x: Act, dy: Act, dw, ws: Workspace, reg=0.0, w=None, defer: ReduceBatch = None):
    """Conv2DBackpropFilter.  defer: leave the split-K reduction to `defer.flush()` (bf16 storage; see ReduceBatch)."""
    _wgrad("conv2d_wgrad", g, x, dy, dw, ws, reg, w, defer, conv2d_wgrad_ws_bytes(g))


def conv2d_transpose_fwd(g, x: Act, wt, bias, y: Act):
    """Conv2DTranspose(strides=2, padding='same') forward (dl_models/u_net.py:297-304)."""
    check(_fn("conv2d_transpose_fwd", x.sfx)(C.byref(g), _p(x), x.ld, _p(wt), _p(bias), _p(y), y.ld,
                                                      _stream()), "conv2d_transpose_fwd")


def conv2d_transpose_dgrad(g, dy: Act, w, dx: Act, addend: Act = None, w_packed=None):
    if w_packed is not None:
        check(_lib.lib().unetrir_conv2d_transpose_dgrad_packed_bf16(C.byref(g), _p(dy), dy.ld, _p(w), _p(w_packed), _p(addend),
                                                                    addend.ld if addend is not None else 0, _p(dx), dx.ld,
                                                                    _stream()), "conv2d_transpose_dgrad_packed")
        return
    check(_fn("conv2d_transpose_dgrad", dy.sfx)(C.byref(g), _p(dy), dy.ld, _p(w), _p(addend),
                                                        addend.ld if addend is not None else 0, _p(dx), dx.ld,
                                                        _stream()), "conv2d_transpose_dgrad")


def conv2d_transpose_wgrad_ws_bytes(g):
    return _lib.lib().unetrir_conv2d_transpose_wgrad_ws_bytes(C.byref(g))


def conv2d_transpose_wgrad(g, x: Act, dy: Act, dw, ws: Workspace, reg=0.0, w=None, defer: ReduceBatch = None):
    _wgrad("conv2d_transpose_wgrad", g, x, dy, dw, ws, reg, w, defer, conv2d_transpose_wgrad_ws_bytes(g))


# ---- the 2x2 stride-2 layers (dl_models/ae_net.py:273-279, :301-307; csrc/conv2x2.hip): same arguments as the conv2d_* twins

C22_FWD, C22_DGRAD, C22_WGRAD = (_lib.CONSTS[n] for n in ("C22_FWD", "C22_DGRAD", "C22_WGRAD"))


def conv2x2s2_supported(g, x: Act, y: Act, transpose=False):
    """The passes of the layer with input x and output y that the 2x2 stride-2 kernels should run, as a mask of C22_FWD | C22_DGRAD |
    C22_WGRAD (bf16 storage, even sizes, power-of-two channel counts, and not slower than the generic kernels in the measured
    record; include/unetrir.h).  The caller runs the other passes - 0: the whole layer - on conv2d_* / conv2d_transpose_*."""
    if x.sfx != "bf16" or y.sfx != "bf16":
        return 0
    fn = _lib.lib().unetrir_conv2x2s2_transpose_supported_bf16 if transpose else _lib.lib().unetrir_conv2x2s2_supported_bf16
    return int(fn(C.byref(g), x.ld, y.ld))


def conv2x2s2_fwd(g, x: Act, w, bias, y: Act, addend: Act = None):
    """Conv2D(k=2, strides=2, 'same') forward on even sizes (dl_models/ae_net.py:273-279); w [Cout][2][2][Cin] bf16."""
    check(_lib.lib().unetrir_conv2x2s2_fwd_bf16(C.byref(g), _p(x), x.ld, _p(w), _p(bias), _p(addend),
                                                addend.ld if addend is not None else 0, _p(y), y.ld, _stream()), "conv2x2s2_fwd")


def conv2x2s2_dgrad(g, dy: Act, wt, dx: Act, addend: Act = None):
    """Its data gradient; wt [Cin][2][2][Cout] bf16.  Every dx pixel is written once."""
    check(_lib.lib().unetrir_conv2x2s2_dgrad_bf16(C.byref(g), _p(dy), dy.ld, _p(wt), _p(addend),
                                                  addend.ld if addend is not None else 0, _p(dx), dx.ld, _stream()), "conv2x2s2_dgrad")


def conv2x2s2_wgrad_ws_bytes(g):
    return _lib.lib().unetrir_conv2x2s2_wgrad_ws_bytes(C.byref(g))


def conv2x2s2_wgrad(g, x: Act, dy: Act, dw, ws: Workspace, reg=0.0, w=None, defer: ReduceBatch = None):
    """Its weight gradient dw [Cout][2][2][Cin] fp32 (+ reg * w); defer as conv2d_wgrad."""
    _wgrad("conv2x2s2_wgrad", g, x, dy, dw, ws, reg, w, defer, conv2x2s2_wgrad_ws_bytes(g))


def conv2x2s2_transpose_fwd(g, x: Act, wt, bias, y: Act):
    """Conv2DTranspose(k=2, strides=2, 'same') forward (dl_models/ae_net.py:301-307); wt [Cout][2][2][Cin] bf16."""
    check(_lib.lib().unetrir_conv2x2s2_transpose_fwd_bf16(C.byref(g), _p(x), x.ld, _p(wt), _p(bias), _p(y), y.ld, _stream()),
          "conv2x2s2_transpose_fwd")


def conv2x2s2_transpose_dgrad(g, dy: Act, w, dx: Act, addend: Act = None):
    """Its data gradient; w [Cin][2][2][Cout] bf16 (the primary layout)."""
    check(_lib.lib().unetrir_conv2x2s2_transpose_dgrad_bf16(C.byref(g), _p(dy), dy.ld, _p(w), _p(addend),
                                                            addend.ld if addend is not None else 0, _p(dx), dx.ld, _stream()),
          "conv2x2s2_transpose_dgrad")


def conv2x2s2_transpose_wgrad_ws_bytes(g):
    return _lib.lib().unetrir_conv2x2s2_transpose_wgrad_ws_bytes(C.byref(g))


def conv2x2s2_transpose_wgrad(g, x: Act, dy: Act, dw, ws: Workspace, reg=0.0, w=None, defer: ReduceBatch = None):
    """Its weight gradient dw [Cin][2][2][Cout] fp32 (+ reg * w)."""
    _wgrad("conv2x2s2_transpose_wgrad", g, x, dy, dw, ws, reg, w, defer, conv2x2s2_transpose_wgrad_ws_bytes(g))


def dense_fwd(x: Act, w, bias, y: Act, ws: Workspace):
    """Dense on a small batch (dl_models/u_net.py:259): x [B,1,1,K] . w[N][K]^T + bias -> y [B,1,1,N]."""
    B, K, N = x.B, x.C, y.C
    ws.reserve(_lib.lib().unetrir_dense_fwd_ws_bytes(B, K, N))
    check(_lib.lib().unetrir_dense_fwd_f32(_p(x), x.ld, _p(w), _p(bias), _p(y), y.ld, B, K, N, ws.ptr, ws.nbytes, _stream()),
          "dense_fwd")


def dense_dgrad_supported(B, K, N):
    return bool(_lib.lib().unetrir_dense_dgrad_supported(B, K, N))


def dense_dgrad(dy: Act, w, dx: Act, ws: Workspace):
    """dL/dx of Dense(N) (dl_models/u_net.py:259) from the [N][K] kernel as stored: dx[b][k] = sum_n dy[b][n] w[n][k]."""
    B, N, K = dy.P, dy.C, dx.C
    ws.reserve(_lib.lib().unetrir_dense_dgrad_ws_bytes(B, K, N))
    check(_lib.lib().unetrir_dense_dgrad_f32(_p(dy), dy.ld, _p(w), _p(dx), dx.ld, B, K, N, ws.ptr, ws.nbytes, _stream()),
          "dense_dgrad")


def transpose_weight(w, wt, N, T, C_):
    """[N][T][C] -> [C][T][N]."""
    check(_lib.lib().unetrir_transpose_weight_f32(_p(w), _p(wt), N, T, C_, _stream()), "transpose_weight")


def cast_weight_bf16(w, o, N, T, C_, Cp):
    """fp32 master [N][T][C] -> bf16 [N][T][Cp] (zero-padded channels)."""
    check(_lib.lib().unetrir_cast_weight_bf16(_p(w), _p(o), N, T, C_, Cp, _stream()), "cast_weight_bf16")


def transpose_cast_weight_bf16(w, wt, N, T, C_, Np):
    """fp32 master [N][T][C] -> bf16 [C][T][Np] (zero-padded rows)."""
    check(_lib.lib().unetrir_transpose_cast_weight_bf16(_p(w), _p(wt), N, T, C_, Np, _stream()),
          "transpose_cast_weight_bf16")


def make_cast_table(entries, device):
    """Device-resident unetrir_cast_desc array for cast_weights_batched: entries = [(w fp32 [N][T][C], same bf16 or None,
    transposed bf16 or None, N, T, C, Cp, Np[, packed bf16 or None])].  The returned tensor keeps the table alive; the weight
    tensors must too."""
    arr = (_lib.CastDesc * len(entries))()
    for i, ent in enumerate(entries):
        w, same, tr, N, T, C_, Cp, Np = ent[:8]
        pk = ent[8] if len(ent) > 8 else None
        arr[i] = _lib.CastDesc(w.data_ptr(), same.data_ptr() if same is not None else None,
                               tr.data_ptr() if tr is not None else None, N, T, C_, Cp, Np, 0,
                               pk.data_ptr() if pk is not None else None)
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return raw.to(device), len(entries)


def cast_weights_batched(table):
    """fp32 master kernels -> bf16 work copies (both orientations) for every layer of the table in two launches."""
    dev, n = table
    check(_lib.lib().unetrir_cast_weights_batched_bf16(dev.data_ptr(), n, _stream()), "cast_weights_batched")


def stage_h2d(src_ptrs, pinned, dev, stream):
    """Host arrays (addresses src_ptrs) -> pinned staging tensors -> device tensors on `stream`, in one foreign call (no interpreter
    lock while it copies).  src_ptrs[k] must stay alive until the call returns; pinned[k] until the copies have completed."""
    n = len(src_ptrs)
    vp, sz = C.c_void_p * n, C.c_size_t * n
    nbytes = [p.numel() * p.element_size() for p in pinned]
    check(_lib.lib().unetrir_stage_h2d(n, vp(*src_ptrs), vp(*[p.data_ptr() for p in pinned]), vp(*[d.data_ptr() for d in dev]),
                                       sz(*nbytes), C.c_void_p(stream.cuda_stream)), "stage_h2d")


def add_f32_to_bf16(a: Act, b: Act, y: Act):
    """y = a + b with a, y bf16 and b fp32, dense buffers (Add() of dl_models/u_net.py:229 in the bf16 trunk)."""
    check(_lib.lib().unetrir_add_f32_to_bf16(_p(a), _p(b), _p(y), a.base.numel(), _stream()), "add_f32_to_bf16")


def cast_f32_to_bf16(a: Act, y: Act):
    check(_lib.lib().unetrir_cast_f32_to_bf16(_p(a), _p(y), a.base.numel(), _stream()), "cast_f32_to_bf16")


def cast_bf16_to_f32(a: Act, y: Act):
    check(_lib.lib().unetrir_cast_bf16_to_f32(_p(a), _p(y), a.base.numel(), _stream()), "cast_bf16_to_f32")


# ---- BatchNormalization + ReLU ---------------------------------------------------------------

def bn_ws_bytes(P, C_):
    return _lib.lib().unetrir_bn_ws_bytes(P, C_)


def bn_stats(x: Act, gamma, beta, affine, saved, ws: Workspace, moving_mean=None, moving_var=None,
             eps=1e-3, momentum=0.99):
    """BatchNormalization() batch statistics (dl_models/u_net.py:368)."""
    ws.reserve(bn_ws_bytes(x.P, x.C))
    check(_fn("bn_stats", x.sfx)(_p(x), x.ld, x.P, x.C, _p(gamma), _p(beta), eps, momentum,
                                          _p(moving_mean), _p(moving_var), _p(affine), _p(saved), ws.ptr, ws.nbytes,
                                          _stream()), "bn_stats")


def bn_apply(x: Act, affine, y: Act, relu=True):
    check(_fn("bn_apply", x.sfx)(_p(x), x.ld, x.P, x.C, _p(affine), int(relu), _p(y), y.ld, _stream()),
          "bn_apply")


def bn_bwd(da: Act, x: Act, gamma, affine, saved, dx: Act, dgamma, dbeta, ws: Workspace, relu=True):
    ws.reserve(bn_ws_bytes(x.P, x.C))
    if x.sfx == "f32":
        check(_lib.lib().unetrir_bn_bwd_f32(_p(da), da.ld, _p(x), x.ld, x.P, x.C, _p(gamma), _p(affine), _p(saved),
                                            int(relu), _p(dx), dx.ld, _p(dgamma), _p(dbeta), ws.ptr, ws.nbytes,
                                            _stream()), "bn_bwd")
    else:
        check(_lib.lib().unetrir_bn_bwd_bf16(_p(da), da.ld, _p(x), x.ld, x.P, x.C, _p(affine), _p(saved), int(relu),
                                             _p(dx), dx.ld, _p(dgamma), _p(dbeta), ws.ptr, ws.nbytes, _stream()),
              "bn_bwd")


def bn_inference_affine(gamma, beta, moving_mean, moving_var, eps, affine):
    """training=False: the BatchNormalization affine from the moving statistics (rir_generation.py:165)."""
    check(_lib.lib().unetrir_bn_inference_affine_f32(_p(gamma), _p(beta), _p(moving_mean), _p(moving_var), eps, moving_mean.numel(),
                                                     _p(affine), _stream()), "bn_inference_affine")


def bn_act_add(x: Act, affine, y: Act, act=2, addend: Act = None):
    """BatchNormalization -> Add -> activation (dl_models/res_ae.py:331-336); act 0 none, 1 ReLU, 2 LeakyReLU(0.3)."""
    check(_fn("bn_act_add", x.sfx)(_p(x), x.ld, x.P, x.C, _p(affine), int(act), _p(addend),
                                   addend.ld if addend is not None else 0, _p(y), y.ld, _stream()), "bn_act_add")


def bn_bwd_junction(da: Act, x: Act, out: Act, affine, saved, dx: Act, dgamma, dbeta, ws: Workspace, act=2, gskip: Act = None,
                    gskip_add: Act = None):
    """Backward of out = act(BatchNormalization(x) + skip) (dl_models/res_ae.py:334-336, :478-480): dx, dgamma, dbeta and the
    gradient of `skip` (gskip = g (+ gskip_add)) from one reduce / finalize / apply sequence."""
    ws.reserve(bn_ws_bytes(x.P, x.C))
    check(_fn("bn_bwd_junction", x.sfx)(_p(da), da.ld, _p(x), x.ld, _p(out), out.ld, x.P, x.C, _p(affine), _p(saved), int(act), _p(dx), dx.ld,
                                        _p(gskip), gskip.ld if gskip is not None else 0, _p(gskip_add),
                                        gskip_add.ld if gskip_add is not None else 0, _p(dgamma), _p(dbeta), ws.ptr, ws.nbytes, _stream()),
          "bn_bwd_junction")


def act_bwd(da: Act, out: Act, g: Act, act=2):
    check(_fn("act_bwd", out.sfx)(_p(da), da.ld, _p(out), out.ld, out.P, out.C, int(act), _p(g), g.ld, _stream()), "act_bwd")


def add(a, b, y):
    check(_lib.lib().unetrir_add_f32(_p(a), _p(b), _p(y), a.numel(), _stream()), "add")


def colsum(x: Act, out, ws: Workspace):
    """Bias gradient: out[c] = sum over pixels."""
    ws.reserve(bn_ws_bytes(x.P, x.C))
    check(_fn("colsum", x.sfx)(_p(x), x.ld, x.P, x.C, _p(out), ws.ptr, ws.nbytes, _stream()), "colsum")


def relu_fwd(x: Act, y: Act):
    if x.sfx == "f32":
        check(_lib.lib().unetrir_relu_fwd_f32(_p(x), x.ld, x.P, x.C, _p(y), y.ld, _stream()), "relu_fwd")
    else:
        check(_lib.lib().unetrir_bn_apply_bf16(_p(x), x.ld, x.P, x.C, None, 1, _p(y), y.ld, _stream()), "relu_fwd")


def relu_bwd(da: Act, x: Act, dx: Act):
    check(_fn("relu_bwd", x.sfx)(_p(da), da.ld, _p(x), x.ld, x.P, x.C, _p(dx), dx.ld, _stream()),
          "relu_bwd")


# ---- boundary / head / loss ------------------------------------------------------------------

def nchw_to_nhwc_pad(x, y: Act):
    B, C_, H, W = x.shape
    check(_fn("nchw_to_nhwc_pad", y.sfx)(_p(x), B, C_, H, W, _p(y), y.ld, _stream()), "nchw_to_nhwc_pad")


def head6x6_supported(C_):
    return bool(_lib.lib().unetrir_head6x6_supported(C_))


def head6x6_fwd(x: Act, w, bias, y: Act):
    """Conv2D(2, (6,6), padding='same') (dl_models/u_net.py:248), direct kernel."""
    check(_fn("head6x6_fwd", x.sfx)(_p(x), x.ld, x.B, x.H, x.W, x.C, _p(w), _p(bias), _p(y), y.ld, _stream()),
          "head6x6_fwd")


def head6x6_wgrad(x: Act, dy: Act, dw, ws: Workspace):
    ws.reserve(_lib.lib().unetrir_head6x6_wgrad_ws_bytes(x.C))
    check(_fn("head6x6_wgrad", x.sfx)(_p(x), x.ld, x.B, x.H, x.W, x.C, _p(dy), dy.ld, _p(dw), ws.ptr, ws.nbytes,
                                               _stream()), "head6x6_wgrad")


def stem_composite_supported(B, H, W, C0, C1):
    """Whether stem_composite serves a stem of C0 filters in front of a 3x3 layer of C1 filters at this size (bf16 storage)."""
    return bool(_lib.lib().unetrir_stem_composite_supported(int(B), int(H), int(W), int(C0), int(C1)))


def stem_composite_ws_bytes(B):
    return int(_lib.lib().unetrir_stem_composite_ws_bytes(int(B)))


def stem_composite(g: Act, x: Act, w1t, dw0, db0, ws: Workspace, reg=0.0, w0=None):
    """Kernel and bias gradients of the stem Conv2D(64, 3x3) from g = dL/d(output of the 3x3 layer behind it), the network input x
    and that layer's transposed bf16 kernel copy w1t - the data gradient between the two layers is never formed.  dw0 is the
    stem's [64][3][3][pad] gradient tensor (+ reg * w0), db0 its [64] bias gradient."""
    ws.reserve(stem_composite_ws_bytes(g.B))
    check(_lib.lib().unetrir_stem_composite_bf16(_p(g), g.ld, _p(x), x.ld, g.B, g.H, g.W, _p(w1t), reg, _p(w0) if reg else None, _p(dw0),
                                                 int(dw0.shape[-1]), _p(db0), ws.ptr, ws.nbytes, _stream()), "stem_composite")


H1_FWD, H1_BWD = 1, 2       # passes in the mask head1x1_supported returns


def head1x1_supported(C_):
    """Passes of a Conv2D(2, (1, 1)) head with C_ input channels (bf16 trunk) that csrc/head1x1.hip serves: H1_FWD | H1_BWD."""
    return int(_lib.lib().unetrir_head1x1_supported(int(C_)))


def head1x1_fwd(x: Act, w, bias, y: Act):
    """Conv2D(2, (1, 1), activation='linear') (dl_models/diff_u_net.py:247): bf16 activations in, fp32 logits [.., >=4] out; w is
    the fp32 [>=2][C] kernel."""
    check(_lib.lib().unetrir_head1x1_fwd_bf16(_p(x), x.ld, x.B, x.H, x.W, x.C, _p(w), _p(bias), _p(y), y.ld, _stream()), "head1x1_fwd")


def head1x1_bwd_ws_bytes(B, H, W, C_):
    return int(_lib.lib().unetrir_head1x1_bwd_ws_bytes(int(B), int(H), int(W), int(C_)))


def head1x1_bwd(x: Act, dy: Act, w, dx: Act, dw, dbias, ws: Workspace):
    """The whole backward pass of head1x1_fwd in one sweep: dx (bf16, written, no addend), rows 0, 1 of dw and entries 0, 1 of
    dbias (fp32; the rest of the padded gradients is left as it is)."""
    ws.reserve(head1x1_bwd_ws_bytes(x.B, x.H, x.W, x.C))
    check(_lib.lib().unetrir_head1x1_bwd_bf16(_p(x), x.ld, _p(dy), dy.ld, x.B, x.H, x.W, x.C, _p(w), _p(dx), dx.ld, _p(dw), _p(dbias),
                                              ws.ptr, ws.nbytes, _stream()), "head1x1_bwd")


def head6x6_dgrad_supported(W_, C_):
    return bool(_lib.lib().unetrir_head6x6_dgrad_supported(W_, C_))


def head6x6_dgrad(dy: Act, w, dx: Act):
    """Adjoint of head6x6_fwd on bf16 activations (matrix-core kernel): dx = conv-transpose of dy[..., :2] with the fp32 kernel w."""
    if dy.sfx != "bf16" or dx.sfx != "bf16":
        raise ValueError("head6x6_dgrad is a bf16-storage kernel")
    check(_lib.lib().unetrir_head6x6_dgrad_bf16(_p(dy), dy.ld, dy.B, dy.H, dy.W, _p(w), dx.C, _p(dx), dx.ld, _stream()),
          "head6x6_dgrad")


# UpSampling2D((2, 2)) -> Conv2D(2, (6, 6), 'same') (dl_models/u_net.py:247-248) folded to a 4x4 convolution with 8 output channels on
# the coarse grid (csrc/head_up2.hip).  x / dx are the coarse [B,h,w,C] tensors, y / dy the fine [B,2h,2w,..] logits / dlogits.
UP2_FWD, UP2_DGRAD, UP2_WGRAD = 1, 2, 4       # passes in the mask head_up2_supported returns


def head_up2_supported(C_, storage="f32"):
    """Passes of the folded head with C_ input channels that csrc/head_up2.hip serves in this storage type."""
    return int(_fn("head_up2_supported", storage)(int(C_)))


def head_up2_folded_elems(C_):
    return 8 * 4 * 4 * int(C_)


def head_up2_fold(w, wf, C_, round_bf16=False):
    """Master head kernel [PAD][6][6][C] -> folded work copy [8][4][4][C] (fp32; round_bf16: every tap rounded to bf16 once)."""
    if wf.numel() < head_up2_folded_elems(C_) or w.numel() < 2 * 36 * C_:
        raise ValueError("head_up2_fold: buffer too small")
    check(_lib.lib().unetrir_head_up2_fold(_p(w), int(C_), _p(wf), int(bool(round_bf16)), _stream()), "head_up2_fold")


def head_up2_fwd(x: Act, wf, bias, y: Act):
    """Coarse activations in, fp32 logits of the fine grid out, in the layout head6x6_fwd writes."""
    if (y.H, y.W) != (2 * x.H, 2 * x.W) or y.B != x.B or y.sfx != "f32":
        raise ValueError("head_up2_fwd: y must be the fp32 [B,2h,2w,..] logits")
    check(_fn("head_up2_fwd", x.sfx)(_p(x), x.ld, x.B, x.H, x.W, x.C, _p(wf), _p(bias), _p(y), y.ld, _stream()), "head_up2_fwd")


def head_up2_dgrad(dy: Act, wf, dx: Act):
    """Adjoint of head_up2_fwd: fine dlogits (channels 0, 1) -> coarse dx, written (no addend)."""
    if (dy.H, dy.W) != (2 * dx.H, 2 * dx.W) or dy.B != dx.B or dy.sfx != dx.sfx:
        raise ValueError("head_up2_dgrad: dy must be the fine grid of dx, in its storage type")
    check(_fn("head_up2_dgrad", dx.sfx)(_p(dy), dy.ld, dx.B, dx.H, dx.W, _p(wf), dx.C, _p(dx), dx.ld, _stream()), "head_up2_dgrad")


def head_up2_wgrad_ws_bytes(B, h, w, C_):
    return int(_lib.lib().unetrir_head_up2_wgrad_ws_bytes(int(B), int(h), int(w), int(C_)))


def head_up2_wgrad(x: Act, dy: Act, dw, ws: Workspace):
    """Rows 0, 1 of the [PAD][6][6][C] master kernel's gradient (the rest is left as it is) from the coarse x and the fine dlogits."""
    if (dy.H, dy.W) != (2 * x.H, 2 * x.W) or dy.B != x.B or dy.sfx != x.sfx:
        raise ValueError("head_up2_wgrad: dy must be the fine grid of x, in its storage type")
    ws.reserve(head_up2_wgrad_ws_bytes(x.B, x.H, x.W, x.C))
    check(_fn("head_up2_wgrad", x.sfx)(_p(x), x.ld, x.B, x.H, x.W, x.C, _p(dy), dy.ld, _p(dw), ws.ptr, ws.nbytes, _stream()),
          "head_up2_wgrad")


# ---- waveform <-> feature transforms ----------------------------------------------------------------

PAD_MODES = {"reflect": 0, "constant": 1}


def stft_frames(T, hop_length):
    return _lib.lib().unetrir_stft_frames(int(T), int(hop_length))


def stft_features(wav, out, n_fft=256, win_length=128, hop_length=64, pad_mode="reflect", remove_mean=True, normalize=True):
    """wav fp32 [B, T] -> out fp32 [B, 2, H, W] (amplitude / phase planes, zero padded): Loader mean removal +
    FeatureExtractor.extract + Normalizer.normalize + TensorPadder.pad_amp_phase (preprocess.py:13-18, :26-32, :56, :65-70)."""
    if wav.dtype != torch.float32 or out.dtype != torch.float32 or not wav.is_contiguous() or not out.is_contiguous():
        raise ValueError("stft_features takes contiguous fp32 tensors")
    if wav.dim() != 2 or out.dim() != 4 or out.shape[0] != wav.shape[0] or out.shape[1] != 2:
        raise ValueError("stft_features: wav [B, T], out [B, 2, H, W]")
    if pad_mode not in PAD_MODES:
        raise ValueError(f"pad_mode must be one of {sorted(PAD_MODES)}")
    B, T = wav.shape
    check(_lib.lib().unetrir_stft_features_f32(_p(wav), B, T, n_fft, win_length, hop_length, PAD_MODES[pad_mode], int(remove_mean),
                                               int(normalize), _p(out), out.shape[2], out.shape[3], _stream()), "stft_features")


def istft_features(feat, wav, n_bins, n_frames, n_fft=256, win_length=128, hop_length=64, denormalize=True):
    """feat fp32 [B, 2, H, W] -> wav fp32 [B, hop (n_frames - 1)]: un_pad + Normalizer.denormalize + librosa.istft
    (postprocess.py:68-71, :127-134; preprocess.py:34-41, :107-113)."""
    if feat.dtype != torch.float32 or wav.dtype != torch.float32 or not feat.is_contiguous() or not wav.is_contiguous():
        raise ValueError("istft_features takes contiguous fp32 tensors")
    if feat.dim() != 4 or feat.shape[1] != 2 or wav.dim() != 2 or wav.shape[0] != feat.shape[0] or \
            wav.shape[1] != hop_length * (n_frames - 1):
        raise ValueError("istft_features: feat [B, 2, H, W], wav [B, hop_length * (n_frames - 1)]")
    B, _, H, W = feat.shape
    check(_lib.lib().unetrir_istft_features_f32(_p(feat), B, H, W, n_bins, n_frames, n_fft, win_length, hop_length,
                                                int(denormalize), _p(wav), _stream()), "istft_features")


WAVE_NORMS = {"mse": 0, "energy": 1}


def wave_loss_ws_bytes(B, n_frames, hop_length):
    """Bytes of fp64 state `wave_loss` keeps in its workspace (0: a geometry the kernels do not take)."""
    return int(_lib.lib().unetrir_wave_loss_ws_bytes(int(B), int(n_frames), int(hop_length)))


def wave_loss(pred, wav_true, wave_out, ws: Workspace, n_bins, n_frames, n_fft=256, win_length=128, hop_length=64, norm="mse",
              weight=1.0, global_batch=None, time_weight=None, phase_ref=None, spec_target=None, alpha=0.9, inv_norm=None,
              phase_weight=None, dpred=None, wav_pred=None, loss_out=None):
    """The loss on the waveform PostProcess makes of pred fp32 [B, 2, H, W] against wav_true fp32 [B, hop (n_frames - 1)], and (with
    dpred, fp32 like pred) its gradient on pred, plus (with spec_target) that of the spectrogram loss: wave_out fp64 [2] = (sum_b E_b /
    D_b, sum_b E_b); loss_out[0] += weight / global_batch * wave_out[0]; wav_pred receives the waveform (include/unetrir.h)."""
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda or pred.dim() != 4 or pred.shape[1] != 2:
        raise ValueError("wave_loss: pred must be a CUDA tensor [B, 2, H, W]")
    if norm not in WAVE_NORMS:
        raise ValueError(f"norm must be one of {sorted(WAVE_NORMS)}")
    B, _, H, W = pred.shape
    T = hop_length * (n_frames - 1)
    _f32c(pred, pred.shape, "pred", pred)
    _f32c(wav_true, (B, T), "wav_true", pred)
    for t, shape, what in ((time_weight, (T,), "time_weight"), (phase_ref, pred.shape, "phase_ref"), (spec_target, pred.shape, "spec_target"),
                           (phase_weight, (W,), "phase_weight"), (dpred, pred.shape, "dpred"), (wav_pred, (B, T), "wav_pred")):
        if t is not None:
            _f32c(t, shape, what, pred)
    if wave_out.dtype != torch.float64 or not wave_out.is_contiguous() or tuple(wave_out.shape) != (2,) or wave_out.device != pred.device:
        raise ValueError(f"wave_loss: wave_out must be a contiguous float64 [2] tensor on {pred.device}")
    if loss_out is not None and (loss_out.dtype != torch.float32 or loss_out.dim() != 1 or loss_out.numel() < 1 or
                                 not loss_out.is_contiguous() or loss_out.device != pred.device):
        raise ValueError(f"wave_loss: loss_out must be a contiguous float32 vector on {pred.device}")
    if spec_target is not None and inv_norm is None:
        raise ValueError("wave_loss: the spectrogram term needs inv_norm (the loss kernel's 1 / (2 H W global_batch))")
    gb = B if global_batch is None else global_batch
    need = wave_loss_ws_bytes(B, n_frames, hop_length)
    if need:
        ws.reserve(need)
    check(_lib.lib().unetrir_wave_loss_f32(_p(pred), _p(phase_ref), _p(wav_true), _p(time_weight), B, H, W, int(n_bins), int(n_frames),
                                           int(n_fft), int(win_length), int(hop_length), WAVE_NORMS[norm], float(weight), 1.0 / gb,
                                           _p(spec_target), _p(phase_weight), float(alpha), 0.0 if inv_norm is None else float(inv_norm),
                                           _p(dpred), _p(wav_pred), _p(wave_out), _p(loss_out), ws.ptr, ws.nbytes, _stream()),
          "wave_loss")


def istft_features_bwd(pred, dwav, dpred, n_bins, n_frames, n_fft=256, win_length=128, hop_length=64, phase_ref=None, accumulate=False):
    """The vector-Jacobian product of `istft_features(denormalize=True)`: pred fp32 [B, 2, H, W] and a cotangent dwav fp32
    [B, hop (n_frames - 1)] on the waveform -> dpred fp32 like pred, written (exact zeros in the padding) or, with accumulate, added
    to (padding untouched).  One launch (include/unetrir.h)."""
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda or pred.dim() != 4 or pred.shape[1] != 2:
        raise ValueError("istft_features_bwd: pred must be a CUDA tensor [B, 2, H, W]")
    B, _, H, W = pred.shape
    _f32c(pred, pred.shape, "pred", pred)
    _f32c(dwav, (B, hop_length * (n_frames - 1)), "dwav", pred)
    _f32c(dpred, pred.shape, "dpred", pred)
    if phase_ref is not None:
        _f32c(phase_ref, pred.shape, "phase_ref", pred)
    check(_lib.lib().unetrir_istft_features_bwd_f32(_p(pred), _p(phase_ref), _p(dwav), B, H, W, int(n_bins), int(n_frames), int(n_fft),
                                                    int(win_length), int(hop_length), int(bool(accumulate)), _p(dpred), _stream()),
          "istft_features_bwd")


def decay_loss_supported(T):
    """Whether `decay_loss` takes waveforms of T samples (1 <= T <= 16384)."""
    return bool(_lib.lib().unetrir_decay_loss_supported(int(T)))


def decay_loss_ws_bytes(B, T):
    """Bytes `decay_loss` keeps in its workspace (0: a shape the kernels do not take)."""
    return int(_lib.lib().unetrir_decay_loss_ws_bytes(int(B), int(T)))


def decay_loss(wav_pred, wav_true, decay_out, ws: Workspace, floor_db=60.0, weight=1.0, global_batch=None, dwav=None, loss_out=None):
    """The loss on the energy decay curves (dB, both normalised by the target's energy, floored at -floor_db) of wav_pred against
    wav_true, fp32 [B, T], and (with dwav, fp32 like them) its gradient on wav_pred: decay_out fp64 [2] = (sum_b Q_b, rows counted);
    loss_out[0] += weight / global_batch * decay_out[0].  Two launches (include/unetrir.h)."""
    if not isinstance(wav_pred, torch.Tensor) or not wav_pred.is_cuda or wav_pred.dim() != 2:
        raise ValueError("decay_loss: wav_pred must be a CUDA tensor [B, T]")
    B, T = wav_pred.shape
    _f32c(wav_pred, (B, T), "wav_pred", wav_pred)
    _f32c(wav_true, (B, T), "wav_true", wav_pred)
    if dwav is not None:
        _f32c(dwav, (B, T), "dwav", wav_pred)
    if decay_out.dtype != torch.float64 or not decay_out.is_contiguous() or tuple(decay_out.shape) != (2,) or decay_out.device != wav_pred.device:
        raise ValueError(f"decay_loss: decay_out must be a contiguous float64 [2] tensor on {wav_pred.device}")
    if loss_out is not None and (loss_out.dtype != torch.float32 or loss_out.dim() != 1 or loss_out.numel() < 1 or
                                 not loss_out.is_contiguous() or loss_out.device != wav_pred.device):
        raise ValueError(f"decay_loss: loss_out must be a contiguous float32 vector on {wav_pred.device}")
    gb = B if global_batch is None else global_batch
    need = decay_loss_ws_bytes(B, T)
    if need:
        ws.reserve(need)
    check(_lib.lib().unetrir_decay_loss_f32(_p(wav_pred), _p(wav_true), B, T, float(floor_db), float(weight), 1.0 / gb, _p(dwav),
                                            _p(decay_out), _p(loss_out), ws.ptr, ws.nbytes, _stream()), "decay_loss")


def _res_array(resolutions):
    """R triples (n_fft, win_length, hop_length) -> (a host int array of 3 R entries, R)"""
    res = [tuple(int(v) for v in r) for r in resolutions]
    if not 1 <= len(res) <= 8 or any(len(r) != 3 for r in res):
        raise ValueError("resolutions: 1 to 8 triples (n_fft, win_length, hop_length)")
    return (C.c_int * (3 * len(res)))(*[v for r in res for v in r]), len(res)


def spectral_loss_supported(T, n_fft, win_length, hop_length):
    """Whether `spectral_loss` takes waveforms of T samples at this resolution (n_fft even in 16 ... 1024, 2 <= win_length <= n_fft,
    hop_length >= 1, n_fft / 2 + 1 <= T <= 16384)."""
    return bool(_lib.lib().unetrir_spectral_loss_supported(int(T), int(n_fft), int(win_length), int(hop_length)))


def spectral_loss_ws_bytes(B, T, resolutions):
    """Bytes `spectral_loss` keeps in its workspace (0: a shape the kernels do not take)."""
    arr, R = _res_array(resolutions)
    return int(_lib.lib().unetrir_spectral_loss_ws_bytes(int(B), int(T), R, arr))


def spectral_loss(wav_pred, wav_true, spectral_out, ws: Workspace, resolutions, floor_db=60.0, sc_weight=1.0, log_weight=1.0, weight=1.0,
                  global_batch=None, dwav=None, accumulate=False, loss_out=None):
    """The multi-resolution STFT loss (squared spectral convergence + squared log-magnitude distance, magnitudes smoothed at -floor_db
    relative to the target's mean bin power) of wav_pred against wav_true, fp32 [B, T], and (with dwav, fp32 like them) its gradient
    on wav_pred, written or with accumulate added: spectral_out fp64 [3] = (sum_b mean_r SC, sum_b mean_r LM, rows counted);
    loss_out[0] += weight / global_batch * (sc_weight spectral_out[0] + log_weight spectral_out[1]).  Four launches with dwav, two
    without (include/unetrir.h)."""
    _spectral_loss_call("unetrir_spectral_loss", "spectral_loss", wav_pred, wav_true, spectral_out, ws, resolutions, floor_db, sc_weight,
                        log_weight, weight, global_batch, dwav, accumulate, loss_out)


def spectral_loss_fft_supported(T, n_fft, win_length, hop_length):
    """Whether `spectral_loss_fft` takes waveforms of T samples at this resolution (n_fft 128, 256, 512 or 1024, 2 <= win_length <=
    n_fft, hop_length >= 1, n_fft / 2 + 1 <= T <= 16384)."""
    return bool(_lib.lib().unetrir_spectral_loss_fft_supported(int(T), int(n_fft), int(win_length), int(hop_length)))


def spectral_loss_fft_ws_bytes(B, T, resolutions):
    """Bytes `spectral_loss_fft` keeps in its workspace (0: a shape the kernels do not take)."""
    arr, R = _res_array(resolutions)
    return int(_lib.lib().unetrir_spectral_loss_fft_ws_bytes(int(B), int(T), R, arr))


def spectral_loss_fft(wav_pred, wav_true, spectral_out, ws: Workspace, resolutions, floor_db=60.0, sc_weight=1.0, log_weight=1.0, weight=1.0,
                      global_batch=None, dwav=None, accumulate=False, loss_out=None):
    """`spectral_loss` with fp32 FFTs in LDS in place of the fp64 DFTs: the same arguments, outputs and launch counts, reductions in
    fp64 from fp32 terms, every element of dwav rounded once; an fp32 transform's error, not the DFT form's bound (include/unetrir.h)."""
    _spectral_loss_call("unetrir_spectral_loss_fft", "spectral_loss_fft", wav_pred, wav_true, spectral_out, ws, resolutions, floor_db,
                        sc_weight, log_weight, weight, global_batch, dwav, accumulate, loss_out)


def _spectral_loss_call(symbol, name, wav_pred, wav_true, spectral_out, ws, resolutions, floor_db, sc_weight, log_weight, weight,
                        global_batch, dwav, accumulate, loss_out):
    """The checks and the call of both forms of the spectral loss.  The messages carry the name `spectral_loss` for either."""
    if not isinstance(wav_pred, torch.Tensor) or not wav_pred.is_cuda or wav_pred.dim() != 2:
        raise ValueError("spectral_loss: wav_pred must be a CUDA tensor [B, T]")
    B, T = wav_pred.shape
    _f32c(wav_pred, (B, T), "wav_pred", wav_pred)
    _f32c(wav_true, (B, T), "wav_true", wav_pred)
    if dwav is not None:
        _f32c(dwav, (B, T), "dwav", wav_pred)
    elif accumulate:
        raise ValueError("spectral_loss: accumulate adds to a dwav the caller gives")
    if (spectral_out.dtype != torch.float64 or not spectral_out.is_contiguous() or tuple(spectral_out.shape) != (3,) or
            spectral_out.device != wav_pred.device):
        raise ValueError(f"spectral_loss: spectral_out must be a contiguous float64 [3] tensor on {wav_pred.device}")
    if loss_out is not None and (loss_out.dtype != torch.float32 or loss_out.dim() != 1 or loss_out.numel() < 1 or
                                 not loss_out.is_contiguous() or loss_out.device != wav_pred.device):
        raise ValueError(f"spectral_loss: loss_out must be a contiguous float32 vector on {wav_pred.device}")
    arr, R = _res_array(resolutions)
    gb = B if global_batch is None else global_batch
    ws_bytes, entry = getattr(_lib.lib(), symbol + "_ws_bytes"), getattr(_lib.lib(), symbol + "_f32")
    need = int(ws_bytes(B, T, R, arr))
    if need:
        ws.reserve(need)
    check(entry(_p(wav_pred), _p(wav_true), B, T, R, arr, float(floor_db), float(sc_weight), float(log_weight), float(weight), 1.0 / gb,
                int(bool(accumulate)), _p(dwav), _p(spectral_out), _p(loss_out), ws.ptr, ws.nbytes, _stream()), name)


def auralize_supported(K):
    """Whether `auralize_f32` takes impulse responses of K taps (1 <= K <= 16384)."""
    return bool(_lib.lib().unetrir_auralize_supported(int(K)))


def _auralize_args(rir, dry, out, path=False):
    """The tensor checks of every form of auralize -> (B, K, N, L); path: rir is [B, R, K], R >= 1"""
    named = ((rir, "rir"), (dry, "dry"), (out, "out"))
    if not all(isinstance(t, torch.Tensor) for t, _ in named):
        raise ValueError("auralize: rir, dry and out must be tensors")
    if rir.dim() != (3 if path else 2) or dry.dim() not in (1, 2) or out.dim() != 2:
        raise ValueError(f"auralize: rir {'[B, R, K]' if path else '[B, K]'}, dry [N] or [B, N], out [B, L]")
    B, K = rir.shape[0], rir.shape[-1]
    if path and rir.shape[1] < 1:
        raise ValueError("auralize: empty input: a path has at least one node")
    N, L = dry.shape[-1], out.shape[1]
    if (dry.dim() == 2 and dry.shape[0] != B) or out.shape[0] != B:
        raise ValueError(f"auralize: batch sizes differ: rir {tuple(rir.shape)}, dry {tuple(dry.shape)}, out {tuple(out.shape)}")
    if B < 1 or K < 1 or N < 1 or not 1 <= L <= N + K - 1:
        raise ValueError(f"auralize: empty input, or {L} output samples outside 1 ... N + K - 1 = {N + K - 1}")
    for t, what in named:
        if t.dtype != torch.float32:
            raise ValueError(f"auralize: {what} must be float32, not {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"auralize: {what} must be contiguous")
    for t, what in named:
        if not t.is_cuda or t.device != rir.device:
            raise ValueError(f"auralize: {what} must be a CUDA tensor on the device of rir (there is no CPU path)")
    return B, K, N, L


def auralize_f32(rir, dry, out):
    """out fp32 [B, L] = the first L samples of rir fp32 [B, K] convolved with dry fp32 [N] (one dry signal heard through every row) or
    [B, N] (one per row), 1 <= L <= N + K - 1: direct form on the fp32 matrix cores in one launch on the current stream, every element
    an fp32 fma chain in ascending tap order (include/unetrir.h)."""
    B, K, N, L = _auralize_args(rir, dry, out)
    if not auralize_supported(K):
        raise ValueError(f"auralize: impulse responses of {K} taps are not supported (1 ... 16384)")
    check(_lib.lib().unetrir_auralize_f32(_p(rir), _p(dry), _p(out), B, K, N, 0 if dry.dim() == 1 else N, L, _stream()), "auralize")


def auralize_fft_supported(K):
    """Whether `auralize_fft_f32` takes impulse responses of K taps (1 <= K <= 16384)."""
    return bool(_lib.lib().unetrir_auralize_fft_supported(int(K)))


def auralize_fft_block(K):
    """The block P of the overlap-save form for K taps (2048; 0: K is not supported)."""
    return int(_lib.lib().unetrir_auralize_fft_block(int(K)))


def auralize_fft_ws_bytes(B, K, N, dry_stride, L):
    """Bytes `auralize_fft_f32` keeps in its workspace: the spectra of h and x (0: arguments the call refuses)."""
    return int(_lib.lib().unetrir_auralize_fft_ws_bytes(int(B), int(K), int(N), int(dry_stride), int(L)))


def auralize_fft_f32(rir, dry, out, ws: Workspace = None):
    """`auralize_f32` by partitioned overlap-save with FFTs in LDS: two launches on the current stream, within the bound of
    include/unetrir.h of the convolution, not the direct form's bits.  ws: a Workspace that is grown to what the call needs (a
    temporary one when None)."""
    B, K, N, L = _auralize_args(rir, dry, out)
    if not auralize_fft_supported(K):
        raise ValueError(f"auralize: impulse responses of {K} taps are not supported (1 ... 16384)")
    stride = 0 if dry.dim() == 1 else N
    need = auralize_fft_ws_bytes(B, K, N, stride, L)
    if ws is None:
        ws = Workspace(rir.device, need)
    elif not isinstance(ws, Workspace) or ws.buf.device != rir.device:
        raise ValueError(f"auralize: ws must be a Workspace on {rir.device}")
    else:
        ws.reserve(need)
    check(_lib.lib().unetrir_auralize_fft_f32(_p(rir), _p(dry), _p(out), B, K, N, stride, L, ws.ptr, ws.nbytes, _stream()),
          "auralize_fft")


def auralize_path_supported(K):
    """Whether `auralize_path_f32` takes impulse responses of K taps (1 <= K <= 16384)."""
    return bool(_lib.lib().unetrir_auralize_path_supported(int(K)))


def auralize_path_ws_bytes(B, R, K, N, dry_stride, L):
    """Bytes `auralize_path_f32` keeps in its workspace: the spectra of the B R responses and of x (0: arguments the call refuses)."""
    return int(_lib.lib().unetrir_auralize_path_ws_bytes(int(B), int(R), int(K), int(N), int(dry_stride), int(L)))


def auralize_path_f32(rir, times_dev, dry, out, ws: Workspace = None):
    """out fp32 [B, L] = dry rendered along the path of responses rir fp32 [B, R, K]: node r is reached at output sample times_dev[r]
    (a contiguous int32 [R] tensor on the device, strictly increasing, |tau| <= 2^30 - its CONTENTS are not looked at here, so a captured
    graph replays with whatever schedule the tensor holds then), hat-function gains between the nodes (include/unetrir.h).  dry, out
    and ws as `auralize_fft_f32`: two launches on the current stream."""
    B, K, N, L = _auralize_args(rir, dry, out, path=True)
    R = rir.shape[1]
    if (not isinstance(times_dev, torch.Tensor) or times_dev.dtype != torch.int32 or tuple(times_dev.shape) != (R,) or
            not times_dev.is_contiguous() or times_dev.device != rir.device):
        raise ValueError(f"auralize_path: times must be a contiguous int32 [{R}] tensor on {rir.device}")
    if not auralize_path_supported(K):
        raise ValueError(f"auralize: impulse responses of {K} taps are not supported (1 ... 16384)")
    stride = 0 if dry.dim() == 1 else N
    need = auralize_path_ws_bytes(B, R, K, N, stride, L)
    if ws is None:
        ws = Workspace(rir.device, need)
    elif not isinstance(ws, Workspace) or ws.buf.device != rir.device:
        raise ValueError(f"auralize: ws must be a Workspace on {rir.device}")
    else:
        ws.reserve(need)
    check(_lib.lib().unetrir_auralize_path_f32(_p(rir), _p(times_dev), _p(dry), _p(out), B, R, K, N, stride, L, ws.ptr, ws.nbytes,
                                               _stream()), "auralize_path")


def auralize_stream_supported(K):
    """Whether a stream takes impulse responses of K taps (1 <= K <= 16384)."""
    return bool(_lib.lib().unetrir_auralize_stream_supported(int(K)))


def auralize_stream_state_bytes(B, K, dry_rows, max_blocks):
    """Bytes of a stream's device state: 64 + 16384 (2 B Q + dry_rows S) + 8192 dry_rows, Q = ceil(K / 2048), S = Q + max_blocks - 1
    (0: arguments the calls refuse: dry_rows is 1 or B, 1 <= max_blocks <= 64)."""
    return int(_lib.lib().unetrir_auralize_stream_state_bytes(int(B), int(K), int(dry_rows), int(max_blocks)))


class AuralizeStreamState:
    """The device state of one stream and the arguments it was sized for (include/unetrir.h).  buf: a uint8 tensor to use instead of a
    new one - at least `auralize_stream_state_bytes` bytes, 16-byte aligned."""

    def __init__(self, device, B, K, dry_rows, max_blocks, buf=None):
        self.B, self.K, self.dry_rows, self.max_blocks = int(B), int(K), int(dry_rows), int(max_blocks)
        if not auralize_stream_supported(self.K):
            raise ValueError(f"auralize: impulse responses of {K} taps are not supported (1 ... 16384)")
        self.need = auralize_stream_state_bytes(self.B, self.K, self.dry_rows, self.max_blocks)
        if not self.need:
            raise ValueError(f"auralize_stream: B = {B} >= 1, dry_rows = {dry_rows} in (1, B), max_blocks = {max_blocks} in 1 ... 64")
        if buf is None:
            buf = torch.empty(self.need, dtype=torch.uint8, device=device)
        elif (not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous() or
              buf.numel() < self.need or buf.data_ptr() % 16 or buf.device != torch.device(device)):
            raise ValueError(f"auralize_stream: buf must be a contiguous uint8 tensor of at least {self.need} bytes on {device}, 16-byte aligned")
        self.buf = buf
        self.block = auralize_fft_block(self.K)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    @property
    def nbytes(self):
        return self.buf.numel()


def _stream_rir(state, rir, what):
    if not isinstance(state, AuralizeStreamState):
        raise ValueError(f"{what}: state must be an AuralizeStreamState")
    if not isinstance(rir, torch.Tensor):
        raise ValueError(f"{what}: rir must be a tensor")
    if tuple(rir.shape) != (state.B, state.K):
        raise ValueError(f"{what}: rir must have the shape the stream was made for, {(state.B, state.K)}, not {tuple(rir.shape)}")
    if rir.dtype != torch.float32:
        raise ValueError(f"{what}: rir must be float32, not {rir.dtype}")
    if not rir.is_contiguous():
        raise ValueError(f"{what}: rir must be contiguous")
    if not rir.is_cuda or rir.device != state.buf.device:
        raise ValueError(f"{what}: rir must be a CUDA tensor on the device of the state (there is no CPU path)")


def auralize_stream_init(state, rir):
    """Clears the stream (block 0, silence before it) and makes rir fp32 [B, K] its response: a memset and one launch on the current
    stream."""
    _stream_rir(state, rir, "auralize_stream_init")
    check(_lib.lib().unetrir_auralize_stream_init(state.ptr, state.nbytes, _p(rir), state.B, state.K, state.dry_rows, state.max_blocks,
                                                  _stream()), "auralize_stream_init")


def auralize_stream_update(state, rir):
    """A new response rir fp32 [B, K], faded in across the first block of the next push: one launch on the current stream.  A second
    update before a push replaces the first."""
    _stream_rir(state, rir, "auralize_stream_update")
    check(_lib.lib().unetrir_auralize_stream_update(state.ptr, state.nbytes, _p(rir), state.B, state.K, state.dry_rows, state.max_blocks,
                                                    _stream()), "auralize_stream_update")


def auralize_stream_push_f32(state, dry, out):
    """The next blocks of the stream: out fp32 [B, blocks 2048], 1 <= blocks <= max_blocks, from as many new dry samples - dry fp32
    [blocks 2048] (dry_rows = 1) or [dry_rows, blocks 2048], or None for zeros (the tail after the last sample).  Three launches on the
    current stream, whose arguments do not change from call to call: a captured push renders the next blocks at every replay, from
    what dry holds then.  dry and out may be column slices of larger tensors: their rows must be dense (stride 1), not the tensors."""
    if not isinstance(state, AuralizeStreamState):
        raise ValueError("auralize_stream_push: state must be an AuralizeStreamState")
    if not isinstance(out, torch.Tensor) or (dry is not None and not isinstance(dry, torch.Tensor)):
        raise ValueError("auralize_stream_push: dry (or None) and out must be tensors")
    P = state.block
    if out.dim() != 2 or out.shape[0] != state.B or out.shape[1] < P or out.shape[1] % P or out.shape[1] // P > state.max_blocks:
        raise ValueError(f"auralize_stream_push: out must be [{state.B}, blocks {P}] with 1 <= blocks <= {state.max_blocks}, not "
                         f"{tuple(out.shape)}")
    n = out.shape[1]
    named = [(out, "out")]
    stride = 0
    if dry is not None:
        want = (n,) if state.dry_rows == 1 and dry.dim() == 1 else (state.dry_rows, n)
        if tuple(dry.shape) != want:
            raise ValueError(f"auralize_stream_push: dry must be {want} for out {tuple(out.shape)} and dry_rows = {state.dry_rows}, not "
                             f"{tuple(dry.shape)}")
        named.append((dry, "dry"))
        stride = dry.stride(0) if dry.dim() == 2 and state.dry_rows > 1 else 0
    for t, what in named:
        if t.dtype != torch.float32:
            raise ValueError(f"auralize_stream_push: {what} must be float32, not {t.dtype}")
        if t.stride(-1) != 1 or (t.dim() == 2 and t.shape[0] > 1 and t.stride(0) < n):
            raise ValueError(f"auralize_stream_push: {what} must be contiguous along its rows, and the rows must not overlap")
    for t, what in named:
        if not t.is_cuda or t.device != state.buf.device:
            raise ValueError(f"auralize_stream_push: {what} must be a CUDA tensor on the device of the state (there is no CPU path)")
    out_stride = out.stride(0) if state.B > 1 else n
    check(_lib.lib().unetrir_auralize_stream_push(state.ptr, state.nbytes, state.B, state.K, state.dry_rows, state.max_blocks, _p(dry),
                                                  stride, _p(out), out_stride, n // P, _stream()), "auralize_stream_push")


def resample_supported(L, M, zeros):
    """Whether the resampler takes the reduced ratio L / M with `zeros` zero crossings to each side (include/unetrir.h)."""
    return bool(_lib.lib().unetrir_resample_supported(int(L), int(M), int(zeros)))


def resample_taps(L, M, zeros):
    """T, the taps of every phase of the table (even; 0: not supported)."""
    return int(_lib.lib().unetrir_resample_taps(int(L), int(M), int(zeros)))


def resample_out_length(N, L, M):
    """ceil(N L / M): the samples N input samples become (0: an argument below 1)."""
    return int(_lib.lib().unetrir_resample_out_length(int(N), int(L), int(M)))


def resample_table(L, M, zeros, rolloff, beta):
    """The polyphase Kaiser-windowed sinc table of include/unetrir.h as a CPU fp32 tensor [L, T], built on the host in fp64."""
    T = resample_taps(L, M, zeros)
    if not T:
        raise ValueError(f"resample: the ratio L = {L}, M = {M} with zeros = {zeros} is not supported "
                         "(gcd 1, L and M <= 2048, zeros <= 64, T <= 8192, L T <= 2^20)")
    table = torch.empty((int(L), T), dtype=torch.float32)
    err = _lib.lib().unetrir_resample_table_f32(C.cast(table.data_ptr(), C.POINTER(C.c_float)), int(L), int(M), int(zeros),
                                                float(rolloff), float(beta))
    if err == _lib.EINVAL:
        raise ValueError(f"resample: rolloff {rolloff} outside (0, 1] or beta {beta} outside [0, 32]")
    check(err, "resample_table")
    return table


def resample_f32(x, table, L, M, out):
    """out fp32 [B, Nout] = the first Nout <= ceil(N L / M) samples of x fp32 [B, N] resampled by L / M through table fp32 [L, T] (T
    even; `resample_table`, or any other: the kernel does not interpret it): one launch on the current stream, every element one fp32
    fma chain in ascending tap order (include/unetrir.h)."""
    named = ((x, "x"), (table, "table"), (out, "out"))
    if not all(isinstance(t, torch.Tensor) for t, _ in named):
        raise ValueError("resample: x, table and out must be tensors")
    if x.dim() != 2 or table.dim() != 2 or out.dim() != 2:
        raise ValueError("resample: x [B, N], table [L, T], out [B, Nout]")
    L, M = int(L), int(M)
    B, N = x.shape
    T, Nout = table.shape[1], out.shape[1]
    if table.shape[0] != L or T < 2 or T % 2:
        raise ValueError(f"resample: table {tuple(table.shape)} is not [L = {L}, T] with T even")
    if out.shape[0] != B:
        raise ValueError(f"resample: batch sizes differ: x {tuple(x.shape)}, out {tuple(out.shape)}")
    if B < 1 or N < 1:
        raise ValueError("resample: empty input")
    full = resample_out_length(N, L, M)
    if not 1 <= Nout <= full:
        raise ValueError(f"resample: {Nout} output samples outside 1 ... ceil(N L / M) = {full}")
    for t, what in named:
        if t.dtype != torch.float32:
            raise ValueError(f"resample: {what} must be float32, not {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"resample: {what} must be contiguous")
    for t, what in named:
        if not t.is_cuda or t.device != x.device:
            raise ValueError(f"resample: {what} must be a CUDA tensor on the device of x (there is no CPU path)")
    err = _lib.lib().unetrir_resample_f32(_p(x), _p(table), _p(out), B, N, L, M, T, Nout, _stream())
    if err == _lib.EINVAL:
        raise ValueError(f"resample: the geometry L = {L}, M = {M}, T = {T} is not supported (gcd 1, L and M <= 2048, T <= 8192, "
                         "L T <= 2^20)")
    check(err, "resample")


def griffinlim_ws_bytes(B, n_bins, n_frames, n_fft):
    """Bytes of fp64 state `griffinlim` keeps in its workspace (0: a geometry the kernels do not take)."""
    return int(_lib.lib().unetrir_griffinlim_ws_bytes(int(B), int(n_bins), int(n_frames), int(n_fft)))


def griffinlim(feat, wav, n_bins, n_frames, n_fft, win_length, hop_length, ws: Workspace, pad_mode="reflect", denormalize=True,
               n_iter=32, momentum=0.99, init_phase=None, seed=0, draw=0):
    """feat fp32 [B, 2, H, W] (plane 0, the magnitude, alone is read) -> wav fp32 [B, hop (n_frames - 1)]: un_pad +
    Normalizer.denormalize + librosa.griffinlim (postprocess.py:47-50, :69-71, :130-131) for the whole batch, fp64 inside.
    init_phase fp32 [B, n_bins, n_frames] in turns, or None: draw (seed, draw) of `uniform` over that shape."""
    B, H, W = _griffinlim_gate(feat, wav, n_bins, n_frames, hop_length, pad_mode, init_phase)
    need = griffinlim_ws_bytes(B, n_bins, n_frames, n_fft)
    if need:
        ws.reserve(need)
    check(_lib.lib().unetrir_griffinlim_f32(_p(feat), B, H, W, n_bins, n_frames, n_fft, win_length, hop_length, PAD_MODES[pad_mode],
                                            int(denormalize), int(n_iter), float(momentum), _p(init_phase), int(seed), int(draw),
                                            _p(wav), ws.ptr, ws.nbytes, _stream()), "griffinlim")


def _griffinlim_gate(feat, wav, n_bins, n_frames, hop_length, pad_mode, init_phase):
    """The tensor checks of both forms of griffinlim -> (B, H, W)"""
    if feat.dtype != torch.float32 or wav.dtype != torch.float32 or not feat.is_contiguous() or not wav.is_contiguous():
        raise ValueError("griffinlim takes contiguous fp32 tensors")
    if feat.dim() != 4 or feat.shape[1] != 2 or wav.dim() != 2 or wav.shape[0] != feat.shape[0] or \
            wav.shape[1] != hop_length * (n_frames - 1):
        raise ValueError("griffinlim: feat [B, 2, H, W], wav [B, hop_length * (n_frames - 1)]")
    if pad_mode not in PAD_MODES:
        raise ValueError(f"pad_mode must be one of {sorted(PAD_MODES)}")
    B, _, H, W = feat.shape
    if init_phase is not None:
        _f32c(init_phase, (B, n_bins, n_frames), "init_phase", feat)
    return B, H, W


def griffinlim_fft_supported(n_bins, n_frames, n_fft, win_length, hop_length):
    """Whether `griffinlim_fft` takes this geometry: n_fft 128, 256, 512 or 1024, n_bins = n_fft / 2 + 1, n_frames >= 2, 2 <= win_length
    <= n_fft, hop_length >= win_length / 4, hop_length (n_frames - 1) > n_fft / 2 (include/unetrir.h)."""
    return bool(_lib.lib().unetrir_griffinlim_fft_supported(int(n_bins), int(n_frames), int(n_fft), int(win_length), int(hop_length)))


def griffinlim_fft_ws_bytes(B, n_bins, n_frames, n_fft, win_length, hop_length):
    """Bytes of fp32 state `griffinlim_fft` keeps in its workspace (0: a geometry the kernels do not take)."""
    return int(_lib.lib().unetrir_griffinlim_fft_ws_bytes(int(B), int(n_bins), int(n_frames), int(n_fft), int(win_length),
                                                          int(hop_length)))


def griffinlim_fft(feat, wav, n_bins, n_frames, n_fft, win_length, hop_length, ws: Workspace, pad_mode="reflect", denormalize=True,
                   n_iter=32, momentum=0.99, init_phase=None, seed=0, draw=0):
    """`griffinlim` with fp32 state and fp32 FFTs in LDS in place of fp64 state and fp64 DFTs: the same arguments and output, n_iter + 2
    launches; librosa's own complex64 precision, not a bound per element (include/unetrir.h)."""
    B, H, W = _griffinlim_gate(feat, wav, n_bins, n_frames, hop_length, pad_mode, init_phase)
    need = griffinlim_fft_ws_bytes(B, n_bins, n_frames, n_fft, win_length, hop_length)
    if need:
        ws.reserve(need)
    check(_lib.lib().unetrir_griffinlim_fft_f32(_p(feat), B, H, W, n_bins, n_frames, n_fft, win_length, hop_length, PAD_MODES[pad_mode],
                                                int(denormalize), int(n_iter), float(momentum), _p(init_phase), int(seed), int(draw),
                                                _p(wav), ws.ptr, ws.nbytes, _stream()), "griffinlim_fft")


def uniform(out, seed, step):
    """Uniform [0, 1) numbers (the random initial phases of librosa.griffinlim, in turns), draw number `step` of stream `seed`
    (a key of its own beside the dropout masks' and the normal draw's)."""
    check(_lib.lib().unetrir_uniform_f32(_p(out), out.numel(), int(seed), int(step), _stream()), "uniform")


def _f32c(t, shape, what, like):
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape) or t.device != like.device:
        raise ValueError(f"{what} must be a contiguous float32 tensor of shape {tuple(shape)} on {like.device}")


def eval_metrics(pred, target, out, wav_pred=None, wav_true=None, phase_ref=None, n50=2400):
    """pred / target fp32 [B, 2, H, W] (+ phase_ref, the network input, for diff_gen; + the waveform pair fp32 [B, T]) -> out fp64
    [B, 7]: the seven per-sample figures of rir_generation.py:185-225 in one launch (include/unetrir.h)."""
    if not pred.is_cuda or pred.dim() != 4 or pred.shape[1] != 2:
        raise ValueError("eval_metrics: pred must be a CUDA tensor [B, 2, H, W]")
    B, _, H, W = pred.shape
    _f32c(pred, pred.shape, "pred", pred)
    _f32c(target, pred.shape, "target", pred)
    if phase_ref is not None:
        _f32c(phase_ref, pred.shape, "phase_ref", pred)
    if (wav_pred is None) != (wav_true is None):
        raise ValueError("eval_metrics: wav_pred and wav_true come as a pair")
    T = 0
    if wav_pred is not None:
        if wav_pred.dim() != 2 or wav_pred.shape[0] != B:
            raise ValueError("eval_metrics: waveforms must be [B, T]")
        T = wav_pred.shape[1]
        _f32c(wav_pred, (B, T), "wav_pred", pred)
        _f32c(wav_true, (B, T), "wav_true", pred)
    if out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != (B, 7) or out.device != pred.device:
        raise ValueError(f"eval_metrics: out must be a contiguous float64 [{B}, 7] tensor on {pred.device}")
    check(_lib.lib().unetrir_eval_metrics_f32(_p(pred), _p(target), _p(phase_ref), B, H, W, _p(wav_pred), _p(wav_true), T, int(n50),
                                              _p(out), _stream()), "eval_metrics")


def eval_accumulate(out, group, acc):
    """Fold out fp64 [B, 7] into the running sums acc fp64 [G + 1, 8] (row 0 global, rows 1..G the groups; column 7 the count);
    group int32 [B], values outside 0..G-1 count in the global row only (rir_generation.py:227-290)."""
    if not out.is_cuda or out.dtype != torch.float64 or out.dim() != 2 or out.shape[1] != 7 or not out.is_contiguous():
        raise ValueError("eval_accumulate: out must be a contiguous float64 CUDA tensor [B, 7]")
    B = out.shape[0]
    if group.dtype != torch.int32 or tuple(group.shape) != (B,) or not group.is_contiguous() or group.device != out.device:
        raise ValueError(f"eval_accumulate: group must be a contiguous int32 [{B}] tensor on {out.device}")
    if acc.dtype != torch.float64 or acc.dim() != 2 or acc.shape[0] < 2 or acc.shape[1] != 8 or not acc.is_contiguous() or \
            acc.device != out.device:
        raise ValueError(f"eval_accumulate: acc must be a contiguous float64 [G + 1, 8] tensor on {out.device}")
    check(_lib.lib().unetrir_eval_accumulate(_p(out), _p(group), B, acc.shape[0] - 1, _p(acc), _stream()), "eval_accumulate")


def acoustic_figures(wav_a, wav_b, fig, n_pre=120, n_dir=120, n_early=2400, fs=48000.0):
    """wav_a fp32 [B, T] (+ wav_b, its partner, scored in the same launch) -> fig fp64 [B, 2, 10], or [B, 1, 10] without wav_b: the
    room-acoustic figures of each waveform (n0, E_tot, E_dir, E_early, M1, N_fit, drr, c50, ts, edt; include/unetrir.h)."""
    if not isinstance(wav_a, torch.Tensor) or not wav_a.is_cuda or wav_a.dim() != 2:
        raise ValueError("acoustic_figures: wav_a must be a CUDA tensor [B, T]")
    B, T = wav_a.shape
    _f32c(wav_a, (B, T), "wav_a", wav_a)
    if wav_b is not None:
        _f32c(wav_b, (B, T), "wav_b", wav_a)
    nw = 1 if wav_b is None else 2
    if fig.dtype != torch.float64 or not fig.is_contiguous() or tuple(fig.shape) != (B, nw, 10) or fig.device != wav_a.device:
        raise ValueError(f"acoustic_figures: fig must be a contiguous float64 [{B}, {nw}, 10] tensor on {wav_a.device}")
    check(_lib.lib().unetrir_acoustic_figures_f32(_p(wav_a), _p(wav_b), B, T, int(n_pre), int(n_dir), int(n_early), float(fs), _p(fig),
                                                  _stream()), "acoustic_figures")


def acoustic_accumulate(fig, group, acc, fs=48000.0, err=None):
    """Fold the errors of the (pred, true) pairs fig fp64 [B, 2, 10] into the running sums acc fp64 [G + 1, 20] (row 0 global, rows
    1..G the groups; per figure: sum of errors, of pred values, of true values, count); group int32 [B], values outside 0..G-1
    count in the global row only.  err fp64 [B, 5], optional, receives the errors of each pair (include/unetrir.h)."""
    if not isinstance(fig, torch.Tensor) or not fig.is_cuda or fig.dtype != torch.float64 or fig.dim() != 3 or \
            tuple(fig.shape[1:]) != (2, 10) or not fig.is_contiguous():
        raise ValueError("acoustic_accumulate: fig must be a contiguous float64 CUDA tensor [B, 2, 10]")
    B = fig.shape[0]
    if group.dtype != torch.int32 or tuple(group.shape) != (B,) or not group.is_contiguous() or group.device != fig.device:
        raise ValueError(f"acoustic_accumulate: group must be a contiguous int32 [{B}] tensor on {fig.device}")
    if acc.dtype != torch.float64 or acc.dim() != 2 or acc.shape[0] < 1 or acc.shape[1] != 20 or not acc.is_contiguous() or \
            acc.device != fig.device:
        raise ValueError(f"acoustic_accumulate: acc must be a contiguous float64 [G + 1, 20] tensor on {fig.device}")
    if err is not None and (err.dtype != torch.float64 or tuple(err.shape) != (B, 5) or not err.is_contiguous() or
                            err.device != fig.device):
        raise ValueError(f"acoustic_accumulate: err must be a contiguous float64 [{B}, 5] tensor on {fig.device}")
    check(_lib.lib().unetrir_acoustic_accumulate(_p(fig), _p(group), B, acc.shape[0] - 1, float(fs), _p(err), _p(acc), _stream()),
          "acoustic_accumulate")


# ---- batches out of the device-resident data set ------------------------------------------------------

def _bank(t, dtype, what, like=None, rows=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"gather_batch: {what} must be a contiguous {dtype} CUDA tensor")
    if like is not None and t.device != like.device:
        raise ValueError(f"gather_batch: {what} lives on {t.device}, the bank on {like.device}")
    if rows is not None and (t.dim() < 1 or t.shape[0] != rows):
        raise ValueError(f"gather_batch: {what} must have {rows} rows")


def gather_batch(bank, emb_bank, idx_in, idx_out, spec_in, spec_out, emb, wav_bank=None, room_bank=None, wav_true=None, room=None):
    """One launch of DataGenerator.__getitem__ (datageneratorv2.py:64-102): rows `idx_in` / `idx_out` (int32 [B], on the device)
    of bank fp32 [N, 2, H, W] -> spec_in / spec_out [B, 2, H, W]; of emb_bank int32 [N, L] -> emb [B, 2, L]; rows `idx_out` of
    wav_bank fp32 [N, T] / room_bank int32 [N] -> wav_true [B, T] / room [B] when asked for.  The indices are NOT range-checked
    here (include/unetrir.h): whoever builds them checks them against N on the host."""
    _bank(bank, torch.float32, "bank")
    if bank.dim() < 2:
        raise ValueError("gather_batch: bank must be [N, ...]")
    N, B = bank.shape[0], idx_in.numel()
    _bank(emb_bank, torch.int32, "emb_bank", bank, N)
    if emb_bank.dim() != 2:
        raise ValueError("gather_batch: emb_bank must be [N, L]")
    _bank(idx_in, torch.int32, "idx_in", bank)
    _bank(idx_out, torch.int32, "idx_out", bank, B)
    if idx_in.dim() != 1:
        raise ValueError("gather_batch: idx_in / idx_out must be [B]")
    for t, what in ((spec_in, "spec_in"), (spec_out, "spec_out")):
        _bank(t, torch.float32, what, bank)
        if tuple(t.shape) != (B,) + tuple(bank.shape[1:]):
            raise ValueError(f"gather_batch: {what} must be {(B,) + tuple(bank.shape[1:])}")
    _bank(emb, torch.int32, "emb", bank)
    if tuple(emb.shape) != (B, 2, emb_bank.shape[1]):
        raise ValueError(f"gather_batch: emb must be {(B, 2, emb_bank.shape[1])}")
    T = 0
    if (wav_true is None) != (wav_bank is None):
        raise ValueError("gather_batch: wav_true and wav_bank come as a pair")
    if wav_bank is not None:
        _bank(wav_bank, torch.float32, "wav_bank", bank, N)
        _bank(wav_true, torch.float32, "wav_true", bank, B)
        if wav_bank.dim() != 2 or tuple(wav_true.shape) != (B, wav_bank.shape[1]):
            raise ValueError("gather_batch: wav_bank [N, T], wav_true [B, T]")
        T = wav_bank.shape[1]
    if room is not None:
        if room_bank is None:
            raise ValueError("gather_batch: room needs room_bank")
        _bank(room_bank, torch.int32, "room_bank", bank, N)
        _bank(room, torch.int32, "room", bank, B)
        if room_bank.dim() != 1 or room.dim() != 1:
            raise ValueError("gather_batch: room_bank [N], room [B]")
    else:
        room_bank = None
    check(_lib.lib().unetrir_gather_batch_f32(_p(bank), N, bank[0].numel(), _p(emb_bank), emb_bank.shape[1], _p(wav_bank), T,
                                              _p(room_bank), _p(idx_in), _p(idx_out), B, _p(spec_in), _p(spec_out), _p(emb),
                                              _p(wav_true), _p(room), _stream()), "gather_batch")


def sigmoid_loss(logits: Act, target, alpha, inv_norm, pred, dlogits: Act, loss_out, ws: Workspace, phase_ref=None, phase_weight=None):
    """sigmoid head (dl_models/u_net.py:249) + compute_loss (main_training.py:203-231) + dL/dlogits.
    phase_ref: the network input [B,2,H,W] (the `diff_loss` switch, main_training.py:214-217); phase_weight: fp32 [W] column
    weights of the phase term (the `sigmoid_loss` switch, :221-222)."""
    B, _, H, W = target.shape
    ws.reserve(_lib.lib().unetrir_loss_ws_bytes(B * H * W))
    if phase_ref is None and phase_weight is None:
        check(_fn("sigmoid_loss", dlogits.sfx)(_p(logits), logits.ld, _p(target), B, H, W, alpha, inv_norm, _p(pred),
                                               _p(dlogits), _p(loss_out), ws.ptr, ws.nbytes, _stream()), "sigmoid_loss")
        return
    if phase_ref is not None and (tuple(phase_ref.shape) != tuple(target.shape) or phase_ref.dtype != torch.float32 or
                                  not phase_ref.is_contiguous() or phase_ref.device != target.device):
        raise ValueError("phase_ref must be a contiguous float32 tensor of the target's shape on the same device")
    if phase_weight is not None and (tuple(phase_weight.shape) != (W,) or phase_weight.dtype != torch.float32 or
                                     phase_weight.device != target.device):
        raise ValueError(f"phase_weight must be float32 [{W}] on the target's device")
    check(_fn("sigmoid_loss_ex", dlogits.sfx)(_p(logits), logits.ld, _p(target), _p(phase_ref), _p(phase_weight), B, H, W, alpha,
                                              inv_norm, _p(pred), _p(dlogits), _p(loss_out), ws.ptr, ws.nbytes, _stream()),
          "sigmoid_loss_ex")


def sigmoid_nchw(logits: Act, pred):
    B, _, H, W = pred.shape
    check(_lib.lib().unetrir_sigmoid_nchw_f32(_p(logits), logits.ld, B, H, W, _p(pred), _stream()), "sigmoid_nchw")


def sigmoid_bwd(pred, dpred, dlogits: Act):
    B, _, H, W = pred.shape
    check(_fn("sigmoid_bwd", dlogits.sfx)(_p(pred), _p(dpred), B, H, W, _p(dlogits), _stream()), "sigmoid_bwd")


def relu1_loss(logits: Act, target, alpha, inv_norm, pred, dlogits: Act, loss_out, ws: Workspace, phase_ref=None, phase_weight=None):
    """Clipped-ReLU head `relu(out, max_value=1)` (dl_models/ae_net.py:249) + compute_loss + dL/dlogits: sigmoid_loss with the other
    output activation (same arguments, same loss_out)."""
    B, _, H, W = target.shape
    ws.reserve(_lib.lib().unetrir_loss_ws_bytes(B * H * W))
    check(_fn("relu1_loss_ex", dlogits.sfx)(_p(logits), logits.ld, _p(target), _p(phase_ref), _p(phase_weight), B, H, W, alpha,
                                            inv_norm, _p(pred), _p(dlogits), _p(loss_out), ws.ptr, ws.nbytes, _stream()), "relu1_loss_ex")


def relu1_nchw(logits: Act, pred):
    B, _, H, W = pred.shape
    check(_lib.lib().unetrir_relu1_nchw_f32(_p(logits), logits.ld, B, H, W, _p(pred), _stream()), "relu1_nchw")


def relu1_bwd(pred, dpred, dlogits: Act):
    B, _, H, W = pred.shape
    check(_fn("relu1_bwd", dlogits.sfx)(_p(pred), _p(dpred), B, H, W, _p(dlogits), _stream()), "relu1_bwd")


def linear_loss(logits: Act, target, alpha, inv_norm, pred, dlogits: Act, loss_out, ws: Workspace, phase_ref=None, phase_weight=None):
    """Linear output (dl_models/diff_u_net.py:247, diff_vae.py:385) + compute_loss + dL/dlogits: sigmoid_loss with pred = logit
    (same arguments, same loss_out)."""
    B, _, H, W = target.shape
    ws.reserve(_lib.lib().unetrir_loss_ws_bytes(B * H * W))
    check(_fn("linear_loss_ex", dlogits.sfx)(_p(logits), logits.ld, _p(target), _p(phase_ref), _p(phase_weight), B, H, W, alpha,
                                             inv_norm, _p(pred), _p(dlogits), _p(loss_out), ws.ptr, ws.nbytes, _stream()), "linear_loss_ex")


def linear_nchw(logits: Act, pred):
    B, _, H, W = pred.shape
    check(_lib.lib().unetrir_linear_nchw_f32(_p(logits), logits.ld, B, H, W, _p(pred), _stream()), "linear_nchw")


def linear_bwd(pred, dpred, dlogits: Act):
    B, _, H, W = pred.shape
    check(_fn("linear_bwd", dlogits.sfx)(_p(pred), _p(dpred), B, H, W, _p(dlogits), _stream()), "linear_bwd")


# ---- information vector ----------------------------------------------------------------------

def embedding_fwd(idx, table, out):
    check(_lib.lib().unetrir_embedding_fwd_f32(_p(idx), idx.numel(), _p(table), table.shape[0], table.shape[1],
                                               _p(out), _stream()), "embedding_fwd")


def embedding_bwd(idx, dout, dtable):
    check(_lib.lib().unetrir_embedding_bwd_f32(_p(idx), idx.numel(), _p(dout), dtable.shape[0], dtable.shape[1],
                                               _p(dtable), _stream()), "embedding_bwd")


def dropout_mask(mask, p, seed, step):
    """Keep mask of Dropout(p) scaled by 1/(1-p) (dl_models/u_net.py:260), draw number `step` of stream `seed`."""
    check(_lib.lib().unetrir_dropout_mask_f32(_p(mask), mask.numel(), float(p), int(seed), int(step), _stream()), "dropout_mask")


def index_to_i32(idx, out):
    """int32 / int64 index tensor -> the int32 array the embedding kernels read."""
    if idx.dtype not in (torch.int32, torch.int64) or not idx.is_contiguous() or idx.numel() != out.numel():
        raise ValueError("indices must be a contiguous int32 or int64 tensor of the expected size")
    if idx.device != out.device:      # a host pointer handed to the kernel is a GPU memory fault, not an exception
        raise ValueError(f"indices live on {idx.device}, the engine on {out.device}")
    check(_lib.lib().unetrir_index_to_i32(_p(idx), idx.element_size(), idx.numel(), _p(out), _stream()), "index_to_i32")


def mul(x, m, y):
    check(_lib.lib().unetrir_mul_f32(_p(x), _p(m), _p(y), x.numel(), _stream()), "mul")


def sumsq(x, coef, out, accumulate, ws: Workspace):
    ws.reserve(512 * 8)
    check(_lib.lib().unetrir_sumsq_f32(_p(x), x.numel(), float(coef), _p(out), int(accumulate), ws.ptr, ws.nbytes,
                                       _stream()), "sumsq")


def adam(theta, g, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
    """tf.keras.optimizers.Adam step over a flat buffer (main_training.py:168-169, :268)."""
    check(_lib.lib().unetrir_adam_f32(_p(theta), _p(g), _p(m), _p(v), theta.numel(), float(lr_t), beta1, beta2, eps,
                                      float(grad_scale), _stream()), "adam")


def sgd(theta, g, lr, grad_scale=1.0):
    """tf.keras.optimizers.SGD(learning_rate) step (main_training.py:166-167)."""
    check(_lib.lib().unetrir_sgd_f32(_p(theta), _p(g), theta.numel(), float(lr), float(grad_scale), _stream()), "sgd")


def nadam(theta, g, m, v, lr, beta1, beta2, eps, c_g, c_m, c_v, grad_scale=1.0):
    """tf.keras.optimizers.Nadam step (main_training.py:164-165) with the step's schedule coefficients (engine_base.DeviceCounters)."""
    check(_lib.lib().unetrir_nadam_f32(_p(theta), _p(g), _p(m), _p(v), theta.numel(), float(lr), beta1, beta2, eps, float(c_g), float(c_m),
                                       float(c_v), float(grad_scale), _stream()), "nadam")


def adam_dev(theta, g, m, v, hyper):
    """adam() with its five scalars read from device memory (hyper: fp32 [>=5], written by step_advance): HIP-graph replay."""
    check(_lib.lib().unetrir_adam_dev_f32(_p(theta), _p(g), _p(m), _p(v), theta.numel(), _p(hyper), _stream()), "adam_dev")


# ---- tfa.optimizers.LAMB (trainer.py:37-38; csrc/lamb.hip) ---------------------------------------------

LAMB_DECAY, LAMB_ADAPT = _lib.CONSTS["LAMB_DECAY"], _lib.CONSTS["LAMB_ADAPT"]


def lamb_chunk_elems():
    """Elements of one chunk of the LAMB kernels (a chunk never crosses a variable)."""
    return int(_lib.lib().unetrir_lamb_chunk_elems())


def lamb_ws_bytes(n_seg, n_chunks):
    return int(_lib.lib().unetrir_lamb_ws_bytes(int(n_seg), int(n_chunks)))


class LambTable:
    """The segment table of the LAMB kernels, built once per parameter set: one entry (offset, real element count, slot length,
    flags) per variable, slots back to back, in host memory (argument checks) and in device memory (the kernels), the map
    chunk -> variable, and the workspace every range of the table shares (per-chunk partial sums, then one ratio per variable)."""

    def __init__(self, segments, device):
        """segments: (offset, count, slot, decayed, adapted) per variable, in buffer order."""
        L = _lib.lib()
        self.n_seg = len(segments)
        self.host = (_lib.LambSeg * max(self.n_seg, 1))()
        for s_, (off, cnt, slot, dec, ada) in zip(self.host, segments):
            s_.offset, s_.count, s_.slot = int(off), int(cnt), int(slot)
            s_.flags = (LAMB_DECAY if dec else 0) | (LAMB_ADAPT if ada else 0)
        self.n_chunks = int(L.unetrir_lamb_table_init(self.host, self.n_seg, None, 0))
        if self.n_chunks <= 0:
            raise ValueError("LAMB segment table: slots must be contiguous, 4-element aligned and hold 1 <= count <= slot elements")
        chunk_seg = torch.empty(self.n_chunks, dtype=torch.int32)
        L.unetrir_lamb_table_init(self.host, self.n_seg, C.c_void_p(chunk_seg.data_ptr()), self.n_chunks)
        self.device = torch.device(device)
        self.segs = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(self.device)
        self.chunk_seg = chunk_seg.to(self.device)
        self.starts = {int(s[0]): i for i, s in enumerate(segments)}
        self.ends = {int(s[0]) + int(s[2]): i + 1 for i, s in enumerate(segments)}
        self.begin, self.end = int(segments[0][0]), int(segments[-1][0]) + int(segments[-1][2])
        self.ws_bytes = lamb_ws_bytes(self.n_seg, self.n_chunks)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)

    def is_range(self, lo, hi):
        """[lo, hi) begins and ends on a variable boundary."""
        return lo in self.starts and hi in self.ends and self.starts[lo] < self.ends[hi]

    def ratios(self, ws=None):
        """The trust ratios the last call wrote, one per variable (fp32 view of the workspace)."""
        ws = self.ws if ws is None else ws
        return ws[16 * self.n_chunks:16 * self.n_chunks + 4 * self.n_seg].view(torch.float32)


def make_lamb_table(segments, device):
    return LambTable(segments, device)


def _lamb_buffers(table, theta, g, m, v, ws):
    for t in (theta, g, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != table.device or t.numel() < table.end:
            raise ValueError(f"lamb: theta, g, m and v must be contiguous float32 buffers of >= {table.end} elements on {table.device}")
    ws = table.ws if ws is None else ws
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.device != table.device:
        raise ValueError("lamb: the workspace is a contiguous uint8 tensor on the table's device")
    return ws


def lamb(table, theta, g, m, v, lo, hi, lr, beta1, beta2, eps, weight_decay, corr1, corr2, grad_scale=1.0, ws=None):
    """tfa.optimizers.LAMB step (trainer.py:37-38) on the variables whose slots are [lo, hi) of the WHOLE flat buffers theta / g /
    m / v; corr1 = 1 - beta1^t, corr2 = 1 - beta2^t (engine_base.DeviceCounters.adam_begin).  Three launches."""
    ws = _lamb_buffers(table, theta, g, m, v, ws)
    check(_lib.lib().unetrir_lamb_f32(_p(theta), _p(g), _p(m), _p(v), table.host, _p(table.segs), _p(table.chunk_seg), table.n_seg,
                                      int(lo), int(hi), float(lr), beta1, beta2, eps, float(weight_decay), float(corr1), float(corr2),
                                      float(grad_scale), _p(ws), ws.numel(), _stream()), "lamb")


def lamb_dev(table, theta, g, m, v, lo, hi, weight_decay, state, cfg, ws=None):
    """lamb() with the step count read from state[0] and lr, the betas, eps and grad_scale from cfg (the device memory
    step_advance works on): HIP-graph replay."""
    ws = _lamb_buffers(table, theta, g, m, v, ws)
    check(_lib.lib().unetrir_lamb_dev_f32(_p(theta), _p(g), _p(m), _p(v), table.host, _p(table.segs), _p(table.chunk_seg), table.n_seg,
                                          int(lo), int(hi), float(weight_decay), _p(state), _p(cfg), _p(ws), ws.numel(), _stream()),
          "lamb_dev")


def dropout_mask_dev(mask, p, seed, state, offset):
    """dropout_mask() with draw number state[2] + offset read from device memory (state: the uint64 [3] of step_advance)."""
    check(_lib.lib().unetrir_dropout_mask_dev_f32(_p(mask), mask.numel(), float(p), int(seed), C.c_void_p(state.data_ptr() + 16),
                                                  int(offset), _stream()), "dropout_mask_dev")


def step_advance(state, cfg, hyper, n_draws, advance_t=True):
    """Start of a step whose counters live in device memory: t += 1, hyper = (lr_t, beta1, beta2, eps, grad_scale), draw base.
    advance_t=False: a forward-only pass (the validation loop draws dropout masks, main_training.py:297-300)."""
    check(_lib.lib().unetrir_step_advance(_p(state), _p(cfg), _p(hyper), int(n_draws), int(bool(advance_t)), _stream()), "step_advance")


# ---- variational autoencoder (dl_models/vae.py) -------------------------------------------------------

def normal(out, seed, step):
    """Standard-normal noise of SamplingLayer.call (dl_models/vae.py:38), draw number `step` of stream `seed` (the dropout masks'
    draw counter; a key of its own)."""
    check(_lib.lib().unetrir_normal_f32(_p(out), out.numel(), int(seed), int(step), _stream()), "normal")


def normal_dev(out, seed, state, offset):
    """normal() with draw number state[2] + offset read from device memory (state: the uint64 [3] of step_advance)."""
    check(_lib.lib().unetrir_normal_dev_f32(_p(out), out.numel(), int(seed), C.c_void_p(state.data_ptr() + 16), int(offset), _stream()),
          "normal_dev")


def vae_sample_kl_fwd(mu: Act, log_var: Act, eps, inv_global_batch, z: Act, kl_out):
    """z = mu + exp(0.5 log_var) eps (dl_models/vae.py:34-39) and the KL term (main_training.py:192-201): kl_out[1] the raw sum of
    kl_loss_object over every element, kl_out[0] = kl_out[1] / global batch.  mu / log_var / z: [B,1,1,L] nodes; eps dense [B, L]."""
    if eps.dtype != torch.float32 or not eps.is_contiguous() or eps.numel() != mu.B * mu.C:
        raise ValueError(f"eps must be a contiguous float32 [{mu.B},{mu.C}] tensor")
    check(_lib.lib().unetrir_vae_sample_kl_fwd_f32(_p(mu), mu.ld, _p(log_var), log_var.ld, _p(eps), mu.P, mu.C, float(inv_global_batch),
                                                   _p(z), z.ld, _p(kl_out), _stream()), "vae_sample_kl_fwd")


def vae_sample_kl_bwd(mu: Act, log_var: Act, eps, dz: Act, inv_global_batch, dmu: Act, dlv: Act):
    """Backward of vae_sample_kl_fwd: dmu = dz + mu / gb, dlv = dz 0.5 exp(0.5 lv) eps + 0.5 (exp(lv) - 1) / gb (written, not added)."""
    check(_lib.lib().unetrir_vae_sample_kl_bwd_f32(_p(mu), mu.ld, _p(log_var), log_var.ld, _p(eps), _p(dz), dz.ld, mu.P, mu.C,
                                                   float(inv_global_batch), _p(dmu), dmu.ld, _p(dlv), dlv.ld, _stream()),
          "vae_sample_kl_bwd")


def vae_loss_add(kl_out, loss_out):
    """loss += compute_kl_loss(mean, log_var) (main_training.py:264-265): loss_out[0] += kl_out[0] on the device."""
    check(_lib.lib().unetrir_vae_loss_add_f32(_p(kl_out), _p(loss_out), _stream()), "vae_loss_add")


# ---- vector quantiser (dl_models/vqvae.py:42-98) -------------------------------------------------------

def vq_workspace(device):
    """The quantiser layer's own scratch (include/unetrir.h: zero before the first call, every call leaves its head zero)."""
    return torch.zeros(_lib.lib().unetrir_vq_ws_bytes(), dtype=torch.uint8, device=device)


def _vq_check(x: Act, D, E, idx):
    if x.sfx != "f32" or E.dtype != torch.float32 or E.dim() != 2 or E.shape[0] != D or not E.is_contiguous():
        raise ValueError("the quantiser is fp32: x an fp32 Act, E a contiguous float32 [D, K] tensor")
    if x.C % D or idx.dtype != torch.int32 or not idx.is_contiguous() or idx.numel() != x.P * (x.C // D):
        raise ValueError(f"indices must be a contiguous int32 tensor of {x.P} * {x.C} / {D} elements")


def vq_fwd(x: Act, D, E, beta, r, idx, y: Act, vq_out, ws):
    """VectorQuantizer.call (dl_models/vqvae.py:61-98) in one launch: idx int32 [pixels * C / D], y = x + (E[:, idx] - x),
    vq_out[1] = S = sum (E[:, idx] - x)^2, vq_out[0] = r (1 + beta) S / N.  ws: vq_workspace()."""
    _vq_check(x, D, E, idx)
    if y.sfx != "f32" or (y.P, y.C) != (x.P, x.C) or vq_out.dtype != torch.float32 or vq_out.numel() < 2:
        raise ValueError("y must be an fp32 Act of x's shape, vq_out float32 [>= 2]")
    check(_lib.lib().unetrir_vq_fwd_f32(_p(x), x.P, x.ld, x.C, int(D), _p(E), E.shape[1], float(beta), float(r), _p(idx), _p(y), y.ld,
                                        _p(vq_out), _p(ws), ws.numel(), _stream()), "vq_fwd")


def vq_bwd(x: Act, D, idx, E, dy: Act, beta, r, dx: Act, dE):
    """Backward of vq_fwd (two launches, both outputs written): dx = dy + 2 r beta (x - q) / N, dE[:, k] = 2 r sum_{idx == k} (q - x) / N."""
    _vq_check(x, D, E, idx)
    if any(a.sfx != "f32" or (a.P, a.C) != (x.P, x.C) for a in (dy, dx)) or dE.dtype != torch.float32 or dE.shape != E.shape or not dE.is_contiguous():
        raise ValueError("dy / dx must be fp32 Acts of x's shape, dE a contiguous float32 tensor of E's shape")
    check(_lib.lib().unetrir_vq_bwd_f32(_p(x), x.P, x.ld, x.C, int(D), _p(idx), _p(E), E.shape[1], _p(dy), dy.ld, float(beta), float(r),
                                        _p(dx), dx.ld, _p(dE), _stream()), "vq_bwd")


def reset_tile_tickets():
    check(_lib.lib().unetrir_reset_tile_tickets(), "reset_tile_tickets")


# ---- kernel-selection switches --------------------------------------------------------------------

def get_config():
    """The kernel-selection switches in effect (unetrir_config) as a dict."""
    c = _lib.Config()
    check(_lib.lib().unetrir_get_config(C.byref(c)), "get_config")
    return {n: getattr(c, n) for n, _ in _lib.Config._fields_}


_CONFIG_GEN = [0]


def config_generation():
    """Counts the set_config calls that changed a switch.  Anything derived from the dispatch (which kernel serves a layer, how many
    rows of column statistics it writes) is cached against this number by the engines and recomputed when it moves."""
    return _CONFIG_GEN[0]


def set_config(**switches):
    """Replace kernel-selection switches (tests, A/B scripts), e.g. set_config(conv3x3s=0); returns the previous values."""
    old = get_config()
    new = dict(old)
    for k, v in switches.items():
        if k not in new:
            raise KeyError(f"unknown switch {k}")
        new[k] = int(v)
    c = _lib.Config(*[new[n] for n, _ in _lib.Config._fields_])
    check(_lib.lib().unetrir_set_config(C.byref(c)), "set_config")
    if new != old:
        _CONFIG_GEN[0] += 1
    return old


# ---- profiling hooks -------------------------------------------------------------------------

def prof_enable(on):
    _lib.lib().unetrir_prof_enable(int(on))


def prof_collect():
    n = _lib.PROF_FAMILIES
    counts = (C.c_int * n)()
    ms = (C.c_double * n)()
    fl = (C.c_double * n)()
    _lib.lib().unetrir_prof_collect(counts, ms, fl)
    return list(counts), list(ms), list(fl)


# ---- the room classifier deep_CNN (dl_models/cnn_clas.py:19-53; csrc/cnn_clas.hip), fp32 storage -------------------------------

def conv3x3_valid_fwd(g, x: Act, w, bias, y: Act, relu=True):
    """Conv2D(3x3, strides 1, padding='valid', activation='relu') (cnn_clas.py:25, :31, :37): y [B,H-2,W-2,Cout]; w [Cout][3][3][Cin]."""
    check(_lib.lib().unetrir_conv3x3_valid_fwd_f32(C.byref(g), _p(x), x.ld, _p(w), _p(bias), int(bool(relu)), _p(y), y.ld, _stream()),
          "conv3x3_valid_fwd")


def conv3x3_valid_dgrad(g, dy: Act, y: Act, wt, dx: Act, relu=True):
    """Its data gradient from dy * [y > 0] (relu; y the stored forward output) - all of dx is written; wt [Cin][3][3][Cout]."""
    check(_lib.lib().unetrir_conv3x3_valid_dgrad_f32(C.byref(g), _p(dy), dy.ld, _p(y) if relu else None, y.ld if relu else 0,
                                                     int(bool(relu)), _p(wt), _p(dx), dx.ld, _stream()), "conv3x3_valid_dgrad")


def conv3x3_valid_wgrad_ws_bytes(g):
    return int(_lib.lib().unetrir_conv3x3_valid_wgrad_ws_bytes(C.byref(g)))


def conv3x3_valid_wgrad(g, x: Act, dy: Act, y: Act, dw, dbias, ws: Workspace, relu=True):
    """Its weight gradient dw [Cout][3][3][Cin] and bias gradient from the same masked dy."""
    ws.reserve(conv3x3_valid_wgrad_ws_bytes(g))
    check(_lib.lib().unetrir_conv3x3_valid_wgrad_f32(C.byref(g), _p(x), x.ld, _p(dy), dy.ld, _p(y) if relu else None, y.ld if relu else 0,
                                                     int(bool(relu)), _p(dw), _p(dbias), ws.ptr, ws.nbytes, _stream()),
          "conv3x3_valid_wgrad")


def avgpool2_fwd(x: Act, affine, y: Act):
    """AveragePooling2D(2x2, strides 2, 'valid') (cnn_clas.py:28, :34) of x * scale + shift (affine [2C] of bn_stats, or None)."""
    check(_lib.lib().unetrir_avgpool2_fwd_f32(_p(x), x.ld, x.B, x.H, x.W, x.C, _p(affine), _p(y), y.ld, _stream()), "avgpool2_fwd")


def avgpool2_bwd(dy: Act, dx: Act):
    """dx = dy / 4 per cell pixel, 0 in a dropped trailing row / column; dx has the un-pooled size."""
    check(_lib.lib().unetrir_avgpool2_bwd_f32(_p(dy), dy.ld, dx.B, dx.H, dx.W, dx.C, _p(dx), dx.ld, _stream()), "avgpool2_bwd")


def gap_fwd(x: Act, affine, y: Act):
    """GlobalAveragePooling2D (cnn_clas.py:40) of x * scale + shift: [B,h,w,C] -> [B,1,1,C]."""
    check(_lib.lib().unetrir_gap_fwd_f32(_p(x), x.ld, x.B, x.H, x.W, x.C, _p(affine), _p(y), y.ld, _stream()), "gap_fwd")


def gap_bwd(dy: Act, dx: Act):
    check(_lib.lib().unetrir_gap_bwd_f32(_p(dy), dy.ld, dx.B, dx.H, dx.W, dx.C, _p(dx), dx.ld, _stream()), "gap_bwd")


def softmax_ce(logits: Act, classes, target, inv_norm, probs, dlogits: Act, loss_out, acc_out):
    """Dense(classes, softmax) output + categorical_crossentropy (cnn_clas.py:49, :63) + accuracy count in one launch: probs
    [B, classes], dlogits, loss_out[0:3], acc_out[0] (include/unetrir.h)."""
    check(_lib.lib().unetrir_softmax_ce_f32(_p(logits), logits.ld, _p(target), logits.P, int(classes), float(inv_norm), _p(probs),
                                            _p(dlogits), dlogits.ld, _p(loss_out), _p(acc_out), _stream()), "softmax_ce")


def softmax_fwd(logits: Act, classes, probs):
    check(_lib.lib().unetrir_softmax_fwd_f32(_p(logits), logits.ld, logits.P, int(classes), _p(probs), _stream()), "softmax_fwd")


def softmax_bwd(probs, dprobs, classes, dlogits: Act):
    """dlogits from an upstream gradient on the probabilities."""
    check(_lib.lib().unetrir_softmax_bwd_f32(_p(probs), _p(dprobs), dlogits.P, int(classes), _p(dlogits), dlogits.ld, _stream()),
          "softmax_bwd")

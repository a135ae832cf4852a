"""A small static-graph executor over the HIP kernels: the graph is built once as a list of (forward, backward)
closures over preallocated NHWC buffers; forward runs the list, backward runs it in reverse.

Two storage modes, as engine.UNetEngine: "f32" (everything fp32) and "bf16" (trunk activations, their gradients and the
trunk kernels' work copies bf16; accumulation, BatchNorm statistics, biases, weight gradients, master weights, Adam and the
Dense / Embedding branches fp32).  A convolution runs in the storage type of its INPUT node; `_cast` nodes join the two.

Used for the operator graphs that are not hand-scheduled in engine.py: ResAE (dl_models/res_ae.py) and the U-Net feature
block modes 1-3 (dl_models/u_net.py:324-386).  A tensor with several consumers gets its gradient from several writers:
the first one writes, the others accumulate in place (conv data gradients through the kernels' `addend` epilogue).
Parameters, gradients and Adam moments live in flat buffers ordered by backward completion (engine_base.EngineBase).
"""
import torch

from . import ops
from .ops import Act
from .engine_base import BN_EPS, BN_MOMENTUM, L2_COEF, KERNEL_KINDS, EngineBase, ParamSpec

RELU, LEAKY = 1, 2       # activation codes of the C ABI (LeakyReLU: keras default alpha 0.3)


class Node:
    """An activation buffer (or a channel slice of one) and the buffer of its gradient."""
    __slots__ = ("a", "g", "g_set", "needs_grad", "children", "cst")

    def __init__(self, a: Act, needs_grad=True, g: Act = None):
        self.a = a
        self.g = g if g is not None else (Act(torch.empty_like(a.base)) if needs_grad else None)
        self.g_set = False
        self.needs_grad = needs_grad
        self.children = []           # channel-slice views: written whenever this node's gradient is written
        self.cst = None              # (rows, buffer): fused column statistics the producing convolution wrote (BatchNorm statistics)


class GraphEngine(EngineBase):
    mask_on_side_stream = False      # the dropout masks are consumed by nodes of the main stream (trainer.Trainer._make_mask)
    # the output activation fused into the loss kernel: "sigmoid" | "relu1" (dl_models/ae_net.py:249) | "linear" (diff_u_net.py:247)
    output_act = "sigmoid"

    def _out_op(self, what):
        """ops.<output_act>_<what>: the loss kernel, the inference form or the autograd bridge of this engine's output activation."""
        if self.output_act not in ("sigmoid", "relu1", "linear"):
            raise ValueError(f"unknown output activation {self.output_act!r}")
        return getattr(ops, f"{self.output_act}_{what}")

    def __init__(self, B, device="cuda:0", n_replicas=1, runtime=None, share=None, dtype="f32", overlap_wgrad=False):
        """dtype: storage type of the trunk ("f32" or "bf16").
        overlap_wgrad: the side-stream schedule of engine.UNetEngine for the backward pass - weight and bias gradients of every
        convolution / Dense / head / Embedding node on a second stream (they are leaves: nothing in the backward pass reads them),
        gradient buckets handed over from that stream, the optimizer bucket by bucket on a third (trainer.Trainer).  These
        graphs are chains of small launches (ResAE cfg 5: ~770 per step, 12 us on average), so the two chains run side by side.
        runtime, share: see EngineBase (share: an engine of the same class and configuration)."""
        super().__init__(device, n_replicas, dtype, runtime, share)
        self._h_kernels = []                           # kernels of the convolutions that run in bf16 (work copies needed)
        self.c22_passes = {}                           # layer name -> passes served by the 2x2 stride-2 kernels (_conv2x2)
        self.head_passes = 0                           # passes of a 1x1 head served by csrc/head1x1.hip (_head1x1)
        self._s2_kernels = []                          # 3x3 stride-2 kernels among them
        self._share = share
        self.include_reg = True       # backward adds d/dw of the l2 terms (False: the caller differentiates them itself)
        self.B = B
        self.nodes, self.specs_fwd, self.ops = [], [], []
        self._op_params, self._n_specs_seen = [], 0
        self.bn_names, self.l2_names = [], []
        self.moving = {}
        self.masks = {}              # dropout keep masks by name (None = no dropout)
        self.mask_width = {}         # ... and the width of the node each one multiplies
        self._logits32 = None        # fp32 copy of a bf16 output layer's logits, made on first use
        self.ws = ops.Workspace(self.device, 1 << 20)
        # the split-K reductions of the weight gradients are parked and run together (ops.ReduceBatch): one launch per bucket
        # hand-over / full arena instead of one per convolution (configs[4]: 57 per step).  Every slab set is parked here: measured on
        # configs[4] (scripts/sweep_park.py, engines alternating in one process) 6.78 ms per step with none parked, 6.69-6.79 with only
        # the sets <= 4 / 16 / 64 MB parked, 6.47 with all of them (single stream: 6.82 / 6.61-6.76 / 6.49)
        self._init_side_stream(share, overlap_wgrad, 512 << 20)

    # ------------------------------------------------------------------ construction helpers
    def _param(self, name, shape, kind, keras_shape, l2=False):
        self.specs_fwd.append(ParamSpec(name, shape, kind, keras_shape))
        if l2:
            self.l2_names.append(name)

    def _reg(self, node):
        self.nodes.append(node)
        return node

    def _push(self, fwd, bwd):
        """Append one op; the parameters declared since the previous op are the ones whose gradients its `bwd` finalises."""
        self.ops.append((fwd, bwd))
        self._op_params.append([s_.name for s_ in self.specs_fwd[self._n_specs_seen:]])
        self._n_specs_seen = len(self.specs_fwd)

    def _new(self, h, w, c, needs_grad=True, f32=False):
        """A trunk activation (storage type of the engine) or, f32=True, a node of the fp32 branches."""
        return self._reg(Node(ops.new_act(self.B, h, w, c, self.device, dtype=torch.float32 if f32 else self.adt), needs_grad))

    def _input(self):
        """The network input: the NCHW batch as NHWC with its 2 channels zero-padded to PAD (EngineBase.load_input writes it)."""
        self.x4 = self._reg(Node(ops.new_act(self.B, self.H, self.W, self.PAD, self.device, dtype=self.adt), needs_grad=False))
        self.x_in = self.x4.a
        return self.x4

    def _cast(self, x: Node):
        """The same tensor in the other storage type (fp32 <-> bf16 seam between a Dense branch and the trunk)."""
        to16 = x.a.sfx == "f32"
        y = self._reg(Node(ops.new_act(self.B, x.a.H, x.a.W, x.a.C, self.device, dtype=torch.bfloat16 if to16 else torch.float32)))

        def fwd():
            (ops.cast_f32_to_bf16 if to16 else ops.cast_bf16_to_f32)(x.a, y.a)

        def bwd():
            (ops.cast_bf16_to_f32 if to16 else ops.cast_f32_to_bf16)(y.g, x.g)
            x.g_set = True
        self._push(fwd, bwd)
        return y

    def _view(self, parent: Node, c0, c):
        """Channel slice [c0, c0+c) of a buffer (one half of a skip concat)."""
        v = self._reg(Node(parent.a.slice(c0, c), True, parent.g.slice(c0, c)))
        parent.children.append(v)
        return v

    def _emit(self, node, writer):
        """writer(dst, addend): dst = value (+ addend).  First writer of a gradient writes, later ones accumulate."""
        if not node.needs_grad:
            return
        writer(node.g, node.g if node.g_set else None)
        node.g_set = True
        for ch in node.children:
            ch.g_set = True

    def _conv(self, x: Node, name, cout, k, stride, transpose=False, followed_by_bn=True, pad_in=0, pad_out=0, l2=True,
              dense=False, out: Node = None, c22=False):
        """Conv2D / Conv2DTranspose (TF 'same'; 1x1 'valid' is the same geometry) + bias.  c22: a 2x2 stride-2 layer whose passes run
        on csrc/conv2x2.hip where ops.conv2x2s2_supported offers them (_conv2x2)."""
        B, cin = self.B, x.a.C
        if transpose:
            H, W = x.a.H * stride, x.a.W * stride
        else:
            H, W = -(-x.a.H // stride), -(-x.a.W // stride)
        co = pad_out if pad_out else cout
        h16 = x.a.sfx == "bf16"           # the convolution runs in the storage type of its input
        if dense and h16:
            raise ValueError("Dense layers run in fp32: cast the input first")
        y = out if out is not None else self._new(H, W, co, f32=not h16)
        kname, bname = name + ".kernel", name + ".bias"
        if h16:
            self._h_kernels.append(kname)
        real_in = 2 if pad_in else cin
        if transpose:      # primary layout [Cin][k][k][Cout]; keras (k,k,Cout,Cin)
            self._param(kname, (cin, k, k, co), "convT_padout" if pad_out else "convT", (k, k, cout, real_in), l2)
        else:              # [Cout][k][k][Cin]; keras (k,k,Cin,Cout) or Dense [in,out]
            kind = "dense" if dense else "conv_padin" if pad_in else ("conv_padout" if pad_out else "conv")
            self._param(kname, (co, k, k, cin), kind, (cin, cout) if dense else (k, k, real_in, cout), l2)
        self._param(bname, (co,), "bias_pad" if pad_out else "bias", (cout,))
        g = ops.geom(B, x.a.H, x.a.W, cin, co, k, stride)
        reg = lambda: (2.0 * L2_COEF / self.n_replicas) if (l2 and self.include_reg) else 0.0

        if h16 and k == 3 and stride == 2:
            self._s2_kernels.append(kname)             # gets a packed copy for the stride-2 forward kernel (csrc/conv3x3d.hip)
        wpk = lambda: self.ppk.get(kname)
        wf = (lambda: self.ph[kname]) if h16 else (lambda: self.p[kname])       # kernel as stored ([N][T][C])
        wb = (lambda: self.pth[kname]) if h16 else (lambda: self.pt[kname])     # channel roles swapped ([C][T][N])
        # BatchNormalization statistics from the convolution's own epilogue (bf16 trunk): the tensor is not read again for them
        want_cst = bool(h16 and followed_by_bn and not dense and out is None)
        cs = {"gen": None, "rows": 0, "buf": None}

        def colstat():
            """(rows, buffer) of this layer under the kernel-selection switches in effect (the row count depends on which kernel
            serves the layer: sized again when ops.set_config has changed a switch since)."""
            if cs["gen"] != ops.config_generation():
                rows = 0
                if want_cst:
                    rows = ops.conv2d_transpose_colstat_rows(g, x.a) if transpose else ops.conv2d_colstat_rows(g, 0, x.a)
                if rows != cs["rows"] or (rows and cs["buf"] is None):
                    cs["buf"] = torch.empty((rows, co, 2), dtype=torch.float32, device=self.device) if rows else None
                cs["rows"], cs["gen"] = rows, ops.config_generation()
            return cs["rows"], cs["buf"]

        colstat()
        # the passes of a 2x2 stride-2 layer that the conv2x2 kernels take (0: every other layer)
        m22 = ops.conv2x2s2_supported(g, x.a, y.a, transpose) if c22 else 0
        if c22:
            self.c22_passes[name] = m22

        def dense_dgrad(dst, add):
            if add is None:      # split-K path: the weight matrix streams from every CU
                ops.dense_fwd(y.g, self.pt[kname], None, dst, self.ws)
            else:
                ops.conv2d_dgrad(g, y.g, self.pt[kname], dst, addend=add)

        def fwd():
            y.cst = None
            rows, cst = colstat()
            if dense:
                ops.dense_fwd(x.a, self.p[kname], self.p[bname], y.a, self.ws)
            elif cst is not None and self.training:
                if transpose:
                    ops.conv2d_transpose_fwd_colstat(g, x.a, wb(), self.p[bname], y.a, cst)
                else:
                    ops.conv2d_fwd_colstat(g, x.a, wf(), self.p[bname], y.a, cst)
                y.cst = (rows, cst)
            elif m22 & ops.C22_FWD:
                (ops.conv2x2s2_transpose_fwd if transpose else ops.conv2x2s2_fwd)(g, x.a, wb() if transpose else wf(), self.p[bname], y.a)
            elif transpose:
                ops.conv2d_transpose_fwd(g, x.a, wb(), self.p[bname], y.a)
            else:
                ops.conv2d_fwd(g, x.a, wf(), self.p[bname], y.a, w_packed=wpk())

        def bwd():
            with self._wg() as ws_:       # leaves of the backward pass: side stream when there is one
                if m22 & ops.C22_WGRAD:
                    (ops.conv2x2s2_transpose_wgrad if transpose else ops.conv2x2s2_wgrad)(
                        g, x.a, y.g, self.g[kname], ws_, reg=reg(), w=self.p[kname], defer=self._rb if self.park_reduces else None)
                elif transpose:
                    ops.conv2d_transpose_wgrad(g, x.a, y.g, self.g[kname], ws_, reg=reg(), w=self.p[kname], defer=self._rb if self.park_reduces else None)
                else:
                    ops.conv2d_wgrad(g, x.a, y.g, self.g[kname], ws_, reg=reg(), w=self.p[kname], defer=self._rb if self.park_reduces else None)
                if not followed_by_bn:        # a bias in front of BatchNorm has an identically zero gradient
                    ops.colsum(y.g, self.g[bname], ws_)
            if dense:
                self._emit(x, dense_dgrad)
            elif m22 & ops.C22_DGRAD and transpose:
                self._emit(x, lambda dst, add: ops.conv2x2s2_transpose_dgrad(g, y.g, wf(), dst, addend=add))
            elif m22 & ops.C22_DGRAD:
                self._emit(x, lambda dst, add: ops.conv2x2s2_dgrad(g, y.g, wb(), dst, addend=add))
            elif transpose:
                self._emit(x, lambda dst, add: ops.conv2d_transpose_dgrad(g, y.g, wf(), dst, addend=add, w_packed=wpk()))
            else:
                self._emit(x, lambda dst, add: ops.conv2d_dgrad(g, y.g, wb(), dst, addend=add))
        self._push(fwd, bwd)
        return y

    def _conv2x2(self, x: Node, name, cout, transpose=False, out: Node = None, generic=False):
        """Conv2D / Conv2DTranspose(k=2, strides=2, 'same', l2(0.001)) (dl_models/ae_net.py:273-279, :301-307), no BatchNorm behind it.
        On a bf16 trunk the passes ops.conv2x2s2_supported offers run on the 2x2 kernels, the others - generic=True, fp32 storage,
        odd sizes: all of them - on the tap-table kernels of _conv."""
        y = self._conv(x, name, cout, 2, 2, transpose=transpose, followed_by_bn=False, l2=True, out=out,
                       c22=not generic and x.a.sfx == "bf16")
        self.c22_passes.setdefault(name, 0)
        return y

    def _pad2(self, x: Node, h, w):
        """Reshape((h, w, 2)) of a [B,1,1,h*w*2] fp32 node with the 2 channels zero-padded to 4, as the network input is: a strided copy."""
        B = self.B
        y = self._new(h, w, 4, f32=True)
        y.a.base.zero_()

        def fwd():
            y.a.base.view(B, h * w, 4)[:, :, :2].copy_(x.a.base.view(B, h * w, 2))

        def bwd():
            x.g.base.view(B, h * w, 2).copy_(y.g.base.view(B, h * w, 4)[:, :, :2])
            x.g_set = True
        self._push(fwd, bwd)
        return y

    def _head6x6(self, x: Node, name):
        """Conv2D(2, (6,6), 'same') in front of the sigmoid (dl_models/u_net.py:248).  fp32 trunk: an ordinary conv node with the
        2 output channels padded to 4.  bf16 trunk: the head kernels of engine.UNetEngine - bf16 activations in, fp32 logits
        [.., 4] out, bf16 dL/dlogits [.., 8] back."""
        if x.a.sfx == "f32":
            return self._conv(x, name, 2, 6, 1, followed_by_bn=False, pad_out=4, l2=False)
        B, H, W, c, PAD = self.B, x.a.H, x.a.W, x.a.C, self.PAD
        if not ops.head6x6_supported(c):
            raise ValueError("the bf16 head needs number_filters_0 % 8 == 0")
        kname, bname = name + ".kernel", name + ".bias"
        self._param(kname, (PAD, 6, 6, c), "conv_padout", (6, 6, c, 2))
        self._param(bname, (PAD,), "bias_pad", (2,))
        self._h_kernels.append(kname)
        y = self._reg(Node(ops.new_act(B, H, W, 4, self.device), True, ops.new_act(B, H, W, PAD, self.device, dtype=self.adt)))
        g = ops.geom(B, H, W, c, PAD, 6, 1)
        self.ws.reserve(512 * 2 * 36 * c * 4)
        self.ws_w.reserve(512 * 2 * 36 * c * 4)

        def fwd():
            ops.head6x6_fwd(x.a, self.p[kname], self.p[bname], y.a)

        def dgrad(dst, add):
            if add is None and ops.head6x6_dgrad_supported(W, c):
                ops.head6x6_dgrad(y.g, self.p[kname], dst)
            else:
                ops.conv2d_dgrad(g, y.g, self.pth[kname], dst, addend=add)

        def bwd():
            with self._wg() as ws_:
                ops.head6x6_wgrad(x.a, y.g, self.g[kname], ws_)          # rows 2.. of the padded kernel gradient stay 0
                ops.colsum(y.g, self.g[bname], ws_)
            self._emit(x, dgrad)
        self._push(fwd, bwd)
        return y

    def _head6x6_up2(self, x: Node, name):
        """UpSampling2D((2, 2)) -> Conv2D(2, (6,6), 'same') in front of the sigmoid (dl_models/u_net.py:247-248, resize_factor_0 =
        [2, 2]) on the folded kernels of csrc/head_up2.hip, both storage types: x is the coarse [B,h,w,c] node, the result the fine
        fp32 logits [B,2h,2w,4] with dL/dlogits [.., PAD] in the trunk's storage type.  The up-sampled tensor does not exist.  The
        parameter is the 6x6 kernel, as in _head6x6; its folded work copy (EngineBase._fold_copy) is what the kernels read."""
        B, h, w, c, PAD = self.B, x.a.H, x.a.W, x.a.C, self.PAD
        if ops.head_up2_supported(c, x.a.sfx) != (ops.UP2_FWD | ops.UP2_DGRAD | ops.UP2_WGRAD):
            raise ValueError("the head behind resize_factor_0=[2,2] needs number_filters_0 % 8 == 0")
        kname, bname = name + ".kernel", name + ".bias"
        self._param(kname, (PAD, 6, 6, c), "conv_padout", (6, 6, c, 2))
        self._param(bname, (PAD,), "bias_pad", (2,))
        wf = self._fold_copy(kname, c, self._share)
        y = self._reg(Node(ops.new_act(B, 2 * h, 2 * w, 4, self.device), True, ops.new_act(B, 2 * h, 2 * w, PAD, self.device, dtype=self.adt)))
        need = ops.head_up2_wgrad_ws_bytes(B, h, w, c)
        self.ws.reserve(need)
        self.ws_w.reserve(need)

        def fwd():
            ops.head_up2_fwd(x.a, wf, self.p[bname], y.a)

        def dgrad(dst, add):
            if add is not None:
                raise NotImplementedError("the folded head is the only consumer of its input")
            ops.head_up2_dgrad(y.g, wf, dst)

        def bwd():
            with self._wg() as ws_:
                ops.head_up2_wgrad(x.a, y.g, self.g[kname], ws_)         # rows 2.. of the padded kernel gradient stay 0
                ops.colsum(y.g, self.g[bname], ws_)
            self._emit(x, dgrad)
        self._push(fwd, bwd)
        return y

    def _head1x1(self, x: Node, name, generic=False):
        """Conv2D(2, (1, 1), activation='linear') (dl_models/diff_u_net.py:247).  fp32 trunk: an ordinary conv node with the 2 output
        channels padded to 4.  bf16 trunk: the passes ops.head1x1_supported offers run on csrc/head1x1.hip - bf16 activations in,
        fp32 logits [.., 4] out; bf16 dL/dlogits [.., 8] back, the whole backward pass in one sweep - and the others (generic=True:
        all of them) on the tap-table kernels with the padded kernel, whose forward pass stores bf16 logits [.., 8]."""
        if x.a.sfx == "f32":
            return self._conv(x, name, 2, 1, 1, followed_by_bn=False, pad_out=4, l2=False)
        B, H, W, c, PAD = self.B, x.a.H, x.a.W, x.a.C, self.PAD
        m = 0 if generic else ops.head1x1_supported(c)
        self.head_passes = m
        kname, bname = name + ".kernel", name + ".bias"
        self._param(kname, (PAD, 1, 1, c), "conv_padout", (1, 1, c, 2))
        self._param(bname, (PAD,), "bias_pad", (2,))
        self._h_kernels.append(kname)
        ya = ops.new_act(B, H, W, 4, self.device) if m & ops.H1_FWD else ops.new_act(B, H, W, PAD, self.device, dtype=self.adt)
        y = self._reg(Node(ya, True, ops.new_act(B, H, W, PAD, self.device, dtype=self.adt)))
        g = ops.geom(B, H, W, c, PAD, 1, 1)
        if m & ops.H1_BWD:
            # one sweep writes dx (no addend) together with dw and dbias: the head must be the first writer of a gradient that exists
            if not x.needs_grad or x.children:
                raise ValueError("the 1x1 head's backward kernel writes its input's whole gradient: the input must need one and have no views")
            self.ws.reserve(ops.head1x1_bwd_ws_bytes(B, H, W, c))

        def fwd():
            if m & ops.H1_FWD:
                ops.head1x1_fwd(x.a, self.p[kname], self.p[bname], y.a)
            else:
                ops.conv2d_fwd(g, x.a, self.ph[kname], self.p[bname], y.a)

        def bwd():
            if m & ops.H1_BWD:
                # one sweep writes dx, dw and dbias: on the main stream, which the data gradient is on anyway
                if x.g_set:
                    raise NotImplementedError("the 1x1 head is the only consumer of its input")
                ops.head1x1_bwd(x.a, y.g, self.p[kname], x.g, self.g[kname], self.g[bname], self.ws)
                x.g_set = True
                return
            with self._wg() as ws_:
                ops.conv2d_wgrad(g, x.a, y.g, self.g[kname], ws_, w=self.p[kname], defer=self._rb if self.park_reduces else None)
                ops.colsum(y.g, self.g[bname], ws_)
            self._emit(x, lambda dst, add: ops.conv2d_dgrad(g, y.g, self.pth[kname], dst, addend=add))
        self._push(fwd, bwd)
        return y

    def _bn_act(self, x: Node, name, act, addend: Node = None, out: Node = None, batchnorm=True):
        """BatchNormalization (+ Add) (+ activation).  x must have this op as its only consumer."""
        c = x.a.C
        y = out if out is not None else self._new(x.a.H, x.a.W, c, f32=x.a.sfx == "f32")
        if batchnorm:
            self._param(name + ".gamma", (c,), "gamma", (c,))
            self._param(name + ".beta", (c,), "beta", (c,))
            self.bn_names.append(name)
            aff = torch.empty(2 * c, dtype=torch.float32, device=self.device)
            saved = torch.empty(2 * c, dtype=torch.float32, device=self.device)
            if self._share is not None:
                mm, mv = self._share.moving[name + ".moving_mean"], self._share.moving[name + ".moving_variance"]
            else:
                mm = torch.zeros(c, dtype=torch.float32, device=self.device)
                mv = torch.ones(c, dtype=torch.float32, device=self.device)
            self.moving[name + ".moving_mean"], self.moving[name + ".moving_variance"] = mm, mv
        gj = Act(torch.empty_like(x.a.base)) if (addend is not None and not batchnorm) else None

        def fwd():
            if batchnorm and self.training and x.cst is not None:      # statistics rows -> affine -> apply (+ Add, activation): one call
                ops.bn_colstat_act_add(x.cst[1], x.cst[0], x.a, self.p[name + ".gamma"], self.p[name + ".beta"], aff, saved, y.a, act,
                                       addend.a if addend is not None else None, mm, mv, BN_EPS, BN_MOMENTUM)
                return
            elif batchnorm and self.training:
                ops.bn_stats(x.a, self.p[name + ".gamma"], self.p[name + ".beta"], aff, saved, self.ws, mm, mv, BN_EPS, BN_MOMENTUM)
            elif batchnorm:          # training=False: normalise with the moving statistics
                ops.bn_inference_affine(self.p[name + ".gamma"], self.p[name + ".beta"], mm, mv, BN_EPS, aff)
            ops.bn_act_add(x.a, aff if batchnorm else None, y.a, act, addend.a if addend is not None else None)

        def bwd():
            if addend is None and batchnorm:
                ops.bn_bwd(y.g, x.a, None, aff, saved, x.g, self.g[name + ".gamma"], self.g[name + ".beta"], self.ws, relu=act)
            elif addend is None:
                ops.act_bwd(y.g, y.a, x.g, act)
            elif batchnorm:
                # junction y = act(bn(x) + addend): g = dy * act'(y) feeds both branches; one reduce / finalize / apply sequence
                # writes dx, dgamma, dbeta AND the addend's gradient (written, or accumulated in place behind an earlier writer)
                def junction(dst, add):
                    ops.bn_bwd_junction(y.g, x.a, y.a, aff, saved, x.g, self.g[name + ".gamma"], self.g[name + ".beta"], self.ws, act,
                                        gskip=dst, gskip_add=add)
                if addend.needs_grad:
                    self._emit(addend, junction)
                else:
                    junction(None, None)
            else:      # y = act(x + addend) without BatchNorm
                if act:
                    ops.act_bwd(y.g, y.a, gj, act)
                    gsrc = gj
                else:
                    gsrc = y.g
                ops.bn_act_add(gsrc, None, x.g, 0, None)
                self._emit(addend, lambda dst, add: ops.bn_act_add(gsrc, None, dst, 0, add))
            x.g_set = True
        self._push(fwd, bwd)
        return y

    def _add(self, x: Node, y: Node, out: Node = None):
        """Add()([x, y]) without activation (dl_models/u_net.py:229, :337, :359)."""
        z = out if out is not None else self._new(x.a.H, x.a.W, x.a.C, f32=x.a.sfx == "f32")
        mixed = x.a.sfx != y.a.sfx                # bf16 trunk + fp32 information-vector branch (dl_models/u_net.py:229)
        if mixed and not (x.a.sfx == "bf16" and y.a.sfx == "f32"):
            raise ValueError("mixed Add: the first operand is the bf16 trunk, the second the fp32 branch")

        def fwd():
            if mixed:
                ops.add_f32_to_bf16(x.a, y.a, z.a)
            else:
                ops.bn_act_add(x.a, None, z.a, 0, y.a)

        def y_grad(dst, add):
            if not mixed:
                ops.bn_act_add(z.g, None, dst, 0, add)
            elif add is None:
                ops.cast_bf16_to_f32(z.g, dst)
            else:
                raise NotImplementedError("the fp32 operand of a mixed Add has one consumer")

        def bwd():
            self._emit(x, lambda dst, add: ops.bn_act_add(z.g, None, dst, 0, add))
            self._emit(y, y_grad)
        self._push(fwd, bwd)
        return z

    def _concat(self, x: Node, vec: Node):
        """concatenate([Flatten(x), vec]) as an fp32 [B,1,1,n] node: a copy of two row blocks (the copies convert a bf16 x)."""
        B, n_x = self.B, x.a.H * x.a.W * x.a.C
        cat = self._new(1, 1, n_x + vec.a.C, f32=True)

        def fwd():
            cat.a.base.view(B, -1)[:, :n_x].copy_(x.a.base.view(B, -1))
            cat.a.base.view(B, -1)[:, n_x:].copy_(vec.a.base.view(B, -1))

        def bwd():
            x.g.base.view(B, -1).copy_(cat.g.base.view(B, -1)[:, :n_x]); x.g_set = True
            vec.g.base.view(B, -1).copy_(cat.g.base.view(B, -1)[:, n_x:]); vec.g_set = True
        self._push(fwd, bwd)
        return cat

    def _dense(self, x: Node, name, n_out):
        return self._conv(x, name, n_out, 1, 1, False, followed_by_bn=False, l2=False, dense=True)

    def _dropout(self, x: Node, which):
        """Dropout(dropout_p) with an externally supplied keep mask self.masks[which] (already scaled by 1/(1-p))."""
        y = self._new(x.a.H, x.a.W, x.a.C, f32=x.a.sfx == "f32")
        if x.a.sfx != "f32":
            raise ValueError("Dropout sits on the fp32 Dense branches")
        self.masks.setdefault(which, None)
        self.mask_width[which] = x.a.C

        def fwd():
            m = self.masks[which]
            if m is None:
                y.a.base.copy_(x.a.base)
            else:
                ops.mul(x.a.base, m, y.a.base)

        def bwd():
            m = self.masks[which]
            if m is None:
                x.g.base.copy_(y.g.base)
            else:
                ops.mul(y.g.base, m, x.g.base)
            x.g_set = True
        self._push(fwd, bwd)
        return y

    def _embedding(self, n_idx, name="embedding", vocab=2000, dim=256):
        """Embedding(2000, 256) -> Flatten; returns a [B,1,1,n_idx*dim] node."""
        B, dev = self.B, self.device
        self._param(name, (vocab, dim), "embedding", (vocab, dim))
        self.emb_idx = torch.zeros(B * n_idx, dtype=torch.int32, device=dev)
        self.n_idx = n_idx
        emb_out = torch.empty((B * n_idx, dim), dtype=torch.float32, device=dev)
        g_emb_out = torch.empty_like(emb_out)
        node = self._reg(Node(Act(emb_out.view(B, 1, 1, n_idx * dim)), True, Act(g_emb_out.view(B, 1, 1, n_idx * dim))))

        def fwd():
            ops.embedding_fwd(self.emb_idx, self.p[name], emb_out)

        def bwd():
            with self._wg():
                ops.embedding_bwd(self.emb_idx, g_emb_out, self.g[name])
        self._push(fwd, bwd)
        return node

    def _reshape(self, x: Node, h, w, c):
        """Reshape of a [B,1,1,h*w*c] node to NHWC [B,h,w,c] (Keras Reshape is NHWC): a view, gradients alias."""
        v = self._reg(Node(Act(x.a.base.view(self.B, h, w, c)), True, Act(x.g.base.view(self.B, h, w, c))))

        def bwd():
            x.g_set = True
        self._push(lambda: None, bwd)
        return v

    # ------------------------------------------------------------------ parameters
    def _finalize_params(self):
        specs = list(reversed(self.specs_fwd))          # backward completion order
        self._layout_params(specs, [s_.name for s_ in specs if s_.kind in KERNEL_KINDS], self._h_kernels, self._s2_kernels, self._share)
        # per op: the end of the flat-buffer prefix that is final after its backward closure (0: the op has no parameters)
        self._op_ends = [max((self.specs[n].end for n in names), default=0) for names in self._op_params]

    # ------------------------------------------------------------------ step pieces
    def run_forward(self, lo=0, hi=None):
        if self.t_dirty or self.training:
            self.refresh_transposed()
        for fwd, _ in self.ops[lo:hi]:
            fwd()

    def backward(self, on_ready=None, dpred=None, include_reg=True):
        """Gradients of every trainable variable into the flat gradient buffer, seeded by the loss kernel's dL/dlogits (or by an
        upstream dL/dpred, NCHW).  The flat buffer is laid out in backward-completion order, so after an op's backward closure
        everything up to the end of that op's parameters is final: `on_ready(offset_end)` hands that prefix to the trainer
        (gradient bucket all-reduce, trainer.GradBucketer)."""
        self.include_reg = include_reg
        if dpred is not None:
            self._check_batch(dpred, "dpred")
            self._out_op("bwd")(self.pred, dpred, self.logits.g)
            self.logits.g_set = True
        for (_, bwd), end in zip(reversed(self.ops), reversed(self._op_ends)):
            bwd()
            if on_ready is not None and end:
                # the prefix is final once this op's leaves (side stream) and its last reader of these parameters (the data
                # gradient just queued) have run
                self._ready(on_ready, end)
        self._end_backward()
        for node in self.nodes:          # next step: the first writer of every gradient writes again
            node.g_set = False

    def loss_or_sigmoid(self, target, global_batch, alpha):
        """The end of a forward pass: sigmoid, and with a target compute_loss and dL/dlogits (which seeds backward())."""
        logits = self.logits
        la = logits.a
        if la.sfx == "bf16":          # a bf16 output layer (ResAE / Autoencoder): the sigmoid + loss kernel reads fp32 logits
            if self._logits32 is None:
                self._logits32 = ops.new_act(self.B, la.H, la.W, la.ld, self.device)
            ops.cast_bf16_to_f32(la, self._logits32)
            la = self._logits32
        if target is not None:
            gb = self.B if global_batch is None else global_batch
            self._out_op("loss")(
                la, target, alpha, 1.0 / (2.0 * self.H * self.W * gb), self.pred, logits.g, self.loss_out, self.ws, **self._loss_extras())
            logits.g_set = True
        else:
            self._out_op("nchw")(la, self.pred)
        return self.pred

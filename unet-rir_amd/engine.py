"""Execution plan of the U-Net train step on one MI355X: buffers, forward schedule, backward
schedule.  Mirrors the Keras graph UNet._build creates (dl_models/u_net.py:201-251, mode 0) and
the tape.gradient pass of main_training.py:256-267, as an explicit list of HIP kernel launches.

Memory layout in HBM (all fp32):
  * activations NHWC, one buffer per layer output, allocated once for a fixed batch size;
    the skip concat of level l is ONE buffer [B,Hl,Wl,2*Cl]: the encoder's BN+ReLU output is written
    into channels [0,Cl), the Conv2DTranspose output into [Cl,2Cl) (dl_models/u_net.py:308 costs no copy);
  * parameters, gradients and Adam moments are four flat buffers with identical layout, ordered by
    backward completion (head first, enc1 last) so gradient buckets for the all-reduce are contiguous
    slices that become final in order;
  * Conv2D kernels [Cout][k][k][Cin], Conv2DTranspose kernels [Cin][k][k][Cout], Dense [out][in];
    the first conv's Cin and the head's Cout are zero-padded 2 -> 4 (pad weights stay exactly zero:
    their gradient is identically zero).
"""
import math

import torch

from . import _lib, ops
from .engine_base import BN_EPS, BN_MOMENTUM, EMB_DIM, L2_COEF, VEC_CH, VOCAB, EngineBase, ParamSpec
from .ops import Act


def same_out(n, s):
    return -(-n // s)


def pick_concurrent_streams(device, n, candidates=12):
    """n HIP streams that really run beside the current stream and beside each other.  Streams are multiplexed onto a few
    hardware queues, and two streams that share a queue execute in order: the side-stream schedule then gains nothing (or
    loses: measured 14.1 vs 15.0-17.3 ms per step depending on which pool streams an engine happened to get).  So probe:
    queue ~2 ms of copies on stream A, then a tiny kernel on candidate B; B is concurrent with A if its kernel finishes
    while A is still busy."""
    dev = torch.device(device)
    main = torch.cuda.current_stream(dev)
    a = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    tiny = torch.zeros(64, device=dev)

    def runs_beside(busy, cand):
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(busy):
            for _ in range(24):
                b.copy_(a, non_blocking=True)
            end_busy = torch.cuda.Event()
            end_busy.record(busy)
        with torch.cuda.stream(cand):
            tiny.add_(1.0)
            end_cand = torch.cuda.Event()
            end_cand.record(cand)
        end_cand.synchronize()
        ok = not end_busy.query()
        torch.cuda.synchronize(dev)
        return ok

    chosen, pool = [], [torch.cuda.Stream(device=dev) for _ in range(candidates)]
    for c in pool:
        if len(chosen) == n:
            break
        if all(runs_beside(o, c) and runs_beside(c, o) for o in [main] + chosen):
            chosen.append(c)
    for c in pool:                      # fewer independent queues than asked for: fill up (correct, just less overlap)
        if len(chosen) == n:
            break
        if c not in chosen:
            chosen.append(c)
    return chosen


class UNetEngine(EngineBase):
    """One replica of the model for a fixed per-replica batch size B on one device."""
    mask_on_side_stream = True       # the dropout mask's only consumers (information-vector branch) run on the side stream

    def __init__(self, H, W, B, F0=32, k=3, depth=4, batchnorm=True, inf_vector_shape=(2, 16), s0=1, s=2,
                 device="cuda:0", n_replicas=1, dtype="f32", overlap_wgrad=False, runtime=None, share=None):
        """runtime, share: see EngineBase (share: a UNetEngine of the same configuration)."""
        super().__init__(device, n_replicas, dtype, runtime, share)
        # s0 = resize_factor_0 (dl_models/u_net.py:213, :272): 2 = the first encoder convolution has stride 2, every level runs on
        # (H/2, W/2) / 2^l and UpSampling2D((2, 2)) in front of the head (:247-248) is folded into it (csrc/head_up2.hip)
        if s0 not in (1, 2) or s != 2:
            raise NotImplementedError("HIP path implements resize_factor_0=[1,1] or [2,2] and res_factor=[2,2]")
        self.s0 = s0
        self._cst_rows, self._cst_buf, self._cst_gen = {}, None, ops.config_generation()
        if F0 % self.PAD:
            raise ValueError(f"number_filters_0 must be a multiple of {self.PAD} for dtype {dtype}")
        # kernels != 3 in bf16 storage (kernels=6 is the reference's constructor default, dl_models/u_net.py:40-45): forward and data
        # gradients on the tap-table kernels, weight gradients on the tap-table weight-gradient kernel with bf16 operand loads
        if k < 1 or k > 6:
            raise ValueError("kernels must be in 1..6")
        self.H, self.W, self.B, self.F0, self.k, self.depth = H, W, B, F0, k, depth
        self.batchnorm = batchnorm
        self.inf_vector_shape = tuple(inf_vector_shape)
        self.L = depth + 1
        self.ch = [F0 * 2 ** l for l in range(self.L)]
        self.hw = [(same_out(H, s0), same_out(W, s0))]
        for _ in range(depth):
            h, w = self.hw[-1]
            self.hw.append((same_out(h, 2), same_out(w, 2)))
        for l in range(depth):
            if self.hw[l][0] != 2 * self.hw[l + 1][0] or self.hw[l][1] != 2 * self.hw[l + 1][1]:
                raise ValueError("spatial size must halve exactly at every level that feeds a skip concat: H and W must be multiples "
                                 f"of resize_factor_0 * 2^depth = {s0 * 2 ** depth}")
        if (s0 * self.hw[0][0], s0 * self.hw[0][1]) != (H, W):
            raise ValueError(f"spatial size must halve exactly: H and W must be multiples of resize_factor_0 * 2^depth = {s0 * 2 ** depth}")
        self.h5, self.w5 = self.hw[-1]
        self.n_idx = int(math.prod(self.inf_vector_shape))
        self.vec_in = self.n_idx * EMB_DIM
        self.vec_dim = self.h5 * self.w5 * VEC_CH
        if share is not None and (share.H, share.W, share.F0, share.k, share.depth, share.batchnorm, share.dtype, share.inf_vector_shape,
                                  share.s0) != (H, W, F0, k, depth, batchnorm, dtype, self.inf_vector_shape, s0):
            raise ValueError("share= needs an engine of the same configuration (only the batch size may differ)")
        # stem_composite: the stem's kernel and bias gradients come from g_y[1], the input and the enc1.cb1 kernel in one op
        # (csrc/stem_composite.hip) instead of the full-resolution enc1.cb1 data gradient (155 GFLOP, 268 MB written at configs[1])
        # and a weight gradient that reads it back; g_down[1] is then never allocated.  bf16 storage, s0 = 1, 3x3 stem of 64 filters,
        # on a HIP device (the op has no other form); otherwise, or with the attribute set to False, the two-kernel path runs.
        self.stem_composite_supported = bool(dtype == "bf16" and s0 == 1 and k == 3 and self.device.type == "cuda" and
                                             ops.stem_composite_supported(B, H, W, self.ch[0], self.ch[0]))
        self.stem_composite = self.stem_composite_supported
        self._build_params(share)
        self._alloc()
        self.ws = ops.Workspace(self.device)
        self._reserve_workspace()
        # overlap_wgrad: weight gradients depend only on tensors the main stream has already produced, so they can run on a
        # side HIP stream (own scratch buffer) beside the dgrad -> BatchNorm-backward chain.  Measured -0.5 ms per step
        # (3 %) in bf16 at cfg 2 (scripts/overlap_ab.py, alternating engines in one process), 0 % in fp32.  bench.py turns
        # it on; the default stays off because overlapping launches make per-kernel event brackets (tests, roofline of the
        # backward kernels) ill-defined.
        # bf16 storage: the split-K reductions of weight gradients with SMALL slab sets (<= 16 MB: small images, narrow layers) are parked
        # and run together (ops.ReduceBatch); the 37.7 MB slab sets of configs[1] reduce at once, while they are still in the
        # Infinity Cache (parking them measured 0.06-0.09 ms per step slower)
        self._init_side_stream(share, overlap_wgrad, 96 << 20, park_max_bytes=16 << 20)
        if self.stem_composite_supported:
            self.ws.reserve(ops.stem_composite_ws_bytes(self.B))
        self.head_direct = ops.head6x6_supported(self.ch[0])
        if s0 == 2:     # the folded head: its own kernels in both storage types, reading the folded work copy of head.kernel
            if ops.head_up2_supported(self.ch[0], self.dtype) != (ops.UP2_FWD | ops.UP2_DGRAD | ops.UP2_WGRAD):
                raise ValueError("the head behind resize_factor_0=[2,2] needs number_filters_0 % 8 == 0")
            self._fold_copy("head.kernel", self.ch[0], share)
            need = ops.head_up2_wgrad_ws_bytes(self.B, *self.hw[0], self.ch[0])
            self.ws.reserve(need)
            self.ws_w.reserve(need)
        elif self.head_direct:
            self.ws.reserve(512 * 2 * 36 * self.ch[0] * 4)
            self.ws_w.reserve(512 * 2 * 36 * self.ch[0] * 4)
        elif self.dtype == "bf16":
            raise ValueError("the bf16 path needs number_filters_0 % 8 == 0 (direct head kernels)")

    # ------------------------------------------------------------------ parameters
    def _build_params(self, share=None):
        k, ch, L = self.k, self.ch, self.L
        specs = []

        def add(name, shape, kind, keras_shape):
            specs.append(ParamSpec(name, shape, kind, keras_shape))

        def bn(prefix, c):
            if self.batchnorm:
                add(prefix + ".gamma", (c,), "gamma", (c,))
                add(prefix + ".beta", (c,), "beta", (c,))

        # backward completion order: head, dec1..decD, vec, encL..enc1
        PAD = self.PAD
        add("head.kernel", (PAD, 6, 6, ch[0]), "conv_padout", (6, 6, ch[0], 2))
        add("head.bias", (PAD,), "bias_pad", (2,))
        for l in range(1, self.depth + 1):
            c = ch[l - 1]
            add(f"dec{l}.cb1b.kernel", (c, 3, 3, c), "conv", (3, 3, c, c))
            add(f"dec{l}.cb1b.bias", (c,), "bias", (c,))
            bn(f"dec{l}.cb1b", c)
            add(f"dec{l}.cb1a.kernel", (c, k, k, 2 * c), "conv", (k, k, 2 * c, c))
            add(f"dec{l}.cb1a.bias", (c,), "bias", (c,))
            bn(f"dec{l}.cb1a", c)
            add(f"dec{l}.up.kernel", (ch[l], k, k, c), "convT", (k, k, c, ch[l]))
            add(f"dec{l}.up.bias", (c,), "bias", (c,))
        add("vec.conv.kernel", (ch[-1], 1, 1, VEC_CH), "conv", (1, 1, VEC_CH, ch[-1]))
        add("vec.conv.bias", (ch[-1],), "bias", (ch[-1],))
        add("vec.dense.kernel", (self.vec_dim, self.vec_in), "dense", (self.vec_in, self.vec_dim))
        add("vec.dense.bias", (self.vec_dim,), "bias", (self.vec_dim,))
        add("vec.embedding", (VOCAB, EMB_DIM), "embedding", (VOCAB, EMB_DIM))
        for l in range(L, 0, -1):
            c = ch[l - 1]
            cin = ch[l - 2] if l > 1 else 2
            add(f"enc{l}.cb1.kernel", (c, 3, 3, c), "conv", (3, 3, c, c))
            add(f"enc{l}.cb1.bias", (c,), "bias", (c,))
            bn(f"enc{l}.cb1", c)
            if l > 1:
                add(f"enc{l}.down.kernel", (c, k, k, cin), "conv", (k, k, cin, c))
            else:
                add(f"enc{l}.down.kernel", (c, k, k, PAD), "conv_padin", (k, k, 2, c))
            add(f"enc{l}.down.bias", (c,), "bias", (c,))
        # the Dense kernel (49 % of the parameters) needs no transposed copy when its data gradient can read it as stored
        self.dense_direct = ops.dense_dgrad_supported(self.B, self.vec_in, self.vec_dim) if share is None else share.dense_direct
        if share is not None and self.dense_direct and not ops.dense_dgrad_supported(self.B, self.vec_in, self.vec_dim):
            raise ValueError("this batch size needs a transposed Dense kernel copy the shared parameter set does not hold")
        # transposed work copies: Conv2D kernels for their data gradient, Conv2DTranspose kernels for their forward; bf16 mode: bf16
        # work copies of every trunk kernel (the information-vector branch stays fp32), packed ones of the strided 3x3 kernels
        t_names = [s_.name for s_ in specs if s_.kind in ("conv", "convT", "conv_padout") or (s_.kind == "dense" and not self.dense_direct)]
        trunk = [s_ for s_ in specs if s_.kind in ("conv", "convT", "conv_padin", "conv_padout") and not s_.name.startswith("vec.")]
        trunk = trunk if self.dtype == "bf16" else []
        strided = lambda n: n.endswith(".up.kernel") or (n.endswith(".down.kernel") and not n.startswith("enc1."))
        self._layout_params(specs, t_names, [s_.name for s_ in trunk], [s_.name for s_ in trunk if strided(s_.name) and s_.shape[1] == 3], share)
        dev = self.device
        # BatchNorm moving statistics (non-trainable)
        self.bn_names = [n[:-len(".gamma")] for n in self.specs if n.endswith(".gamma")]
        self.moving = share.moving if share is not None else {}
        for b in self.bn_names if share is None else ():
            c = self.specs[b + ".gamma"].numel
            self.moving[b + ".moving_mean"] = torch.zeros(c, dtype=torch.float32, device=dev)
            self.moving[b + ".moving_variance"] = torch.ones(c, dtype=torch.float32, device=dev)
        self.l2_names = [f"enc{l}.down.kernel" for l in range(1, L + 1)] + [f"dec{l}.up.kernel" for l in range(1, self.depth + 1)]

    # ------------------------------------------------------------------ buffers
    def _alloc(self):
        B, dev, ch, hw, D = self.B, self.device, self.ch, self.hw, self.depth
        A = lambda h, w, c: ops.new_act(B, h, w, c, dev, dtype=self.adt)      # trunk activations (fp32 or bf16)
        F = lambda h, w, c: ops.new_act(B, h, w, c, dev)                      # always fp32
        PAD = self.PAD
        self.x4, self.down, self.y, self.a = A(self.H, self.W, PAD), {}, {}, {}
        self.x_in = self.x4
        self.cat, self.g_cat = {}, {}
        self.g_down, self.g_y = {}, {}
        for l in range(1, self.L + 1):
            h, w = hw[l - 1]
            c = ch[l - 1]
            self.down[l], self.y[l] = A(h, w, c), A(h, w, c)
            # g_down[1] has no reader under stem_composite: allocated on first use (_g_down1)
            self.g_down[l], self.g_y[l] = (None if l == 1 and self.stem_composite else A(h, w, c)), A(h, w, c)
            if l <= D:
                self.cat[l], self.g_cat[l] = A(h, w, 2 * c), A(h, w, 2 * c)
                self.a[l] = self.cat[l].slice(0, c)
            else:
                self.a[l] = A(h, w, c)
        cL = ch[-1]
        self.emb_out = torch.empty((B * self.n_idx, EMB_DIM), dtype=torch.float32, device=dev)
        self.g_emb_out = torch.empty_like(self.emb_out)
        self.flat = Act(self.emb_out.view(B, 1, 1, self.vec_in))
        self.g_flat = Act(self.g_emb_out.view(B, 1, 1, self.vec_in))
        self.v = ops.new_act(B, 1, 1, self.vec_dim, dev)
        self.vd = ops.new_act(B, 1, 1, self.vec_dim, dev)
        self.g_v = ops.new_act(B, 1, 1, self.vec_dim, dev)
        self.g_vd = ops.new_act(B, 1, 1, self.vec_dim, dev)
        self.vd_sp = Act(self.vd.base.view(B, self.h5, self.w5, VEC_CH))       # Reshape((h5,w5,16)) is NHWC
        self.g_vd_sp = Act(self.g_vd.base.view(B, self.h5, self.w5, VEC_CH))
        self.z, self.g_z = A(self.h5, self.w5, cL), A(self.h5, self.w5, cL)
        self.ya, self.aa, self.yb, self.ab = {}, {}, {}, {}
        self.g_ya, self.g_aa, self.g_yb, self.g_ab = {}, {}, {}, {}
        for l in range(1, D + 1):
            h, w = hw[l - 1]
            c = ch[l - 1]
            for d_ in (self.ya, self.aa, self.yb, self.ab, self.g_ya, self.g_aa, self.g_yb, self.g_ab):
                d_[l] = A(h, w, c)
        self.logits, self.g_logits = F(self.H, self.W, 4), A(self.H, self.W, PAD)      # logits stay fp32 for sigmoid + loss
        if self.dtype == "bf16":    # glue to the fp32 information-vector branch
            self.v1x1, self.g_z32 = F(self.h5, self.w5, cL), F(self.h5, self.w5, cL)
        self._alloc_outputs()
        self.bn_affine = {b: torch.empty(2 * self.specs[b + ".gamma"].numel, dtype=torch.float32, device=dev) for b in self.bn_names}
        self.bn_saved = {b: torch.empty(2 * self.specs[b + ".gamma"].numel, dtype=torch.float32, device=dev) for b in self.bn_names}
        self._mask = None             # the dropout keep mask of the last forward pass
        self.emb_idx = torch.zeros(B * self.n_idx, dtype=torch.int32, device=dev)
        # geometry descriptors
        G, k = ops.geom, self.k
        self.geo = {}
        for l in range(1, self.L + 1):
            h, w = hw[l - 1]
            c = ch[l - 1]
            if l == 1:
                self.geo["enc1.down"] = G(B, self.H, self.W, PAD, c, k, self.s0)
            else:
                hi, wi = hw[l - 2]
                self.geo[f"enc{l}.down"] = G(B, hi, wi, ch[l - 2], c, k, 2)
            self.geo[f"enc{l}.cb1"] = G(B, h, w, c, c, 3, 1)
        self.geo["vec.dense"] = G(B, 1, 1, self.vec_in, self.vec_dim, 1, 1)
        self.geo["vec.conv"] = G(B, self.h5, self.w5, VEC_CH, cL, 1, 1)
        for l in range(1, D + 1):
            h, w = hw[l - 1]
            c = ch[l - 1]
            hl, wl = hw[l]
            self.geo[f"dec{l}.up"] = G(B, hl, wl, ch[l], c, k, 2)
            self.geo[f"dec{l}.cb1a"] = G(B, h, w, 2 * c, c, k, 1)
            self.geo[f"dec{l}.cb1b"] = G(B, h, w, c, c, 3, 1)
        if self.s0 == 1:      # s0 = 2: the head runs on its own kernels alone and has no tap-table geometry
            self.geo["head"] = G(B, self.H, self.W, ch[0], PAD, 6, 1)

    def _reserve_workspace(self):
        need = 1 << 16
        for n, g in self.geo.items():
            if n.endswith(".up"):
                need = max(need, ops.conv2d_transpose_wgrad_ws_bytes(g))
            else:
                need = max(need, ops.conv2d_wgrad_ws_bytes(g))
        P0 = self.B * self.hw[0][0] * self.hw[0][1]
        need = max(need, ops.bn_ws_bytes(P0, max(self.ch[0], 4)), ops.bn_ws_bytes(self.B * self.h5 * self.w5, self.ch[-1]),
                   ops.bn_ws_bytes(self.B, self.vec_dim))
        for l in range(1, self.L + 1):
            h, w = self.hw[l - 1]
            need = max(need, ops.bn_ws_bytes(self.B * h * w, 2 * self.ch[l - 1]))
        if self.dense_direct:
            need = max(need, _lib.lib().unetrir_dense_dgrad_ws_bytes(self.B, self.vec_in, self.vec_dim))
        self.ws.reserve(need)

    # ------------------------------------------------------------------ helpers
    def wf(self, name):
        """Trunk kernel in its stored orientation, in the storage type of the trunk (fp32 master or bf16 work copy)."""
        return self.ph[name] if self.dtype == "bf16" else self.p[name]

    def wb(self, name):
        """Trunk kernel with the channel roles swapped ([C][T][N]) in the storage type of the trunk."""
        return self.pth[name] if self.dtype == "bf16" else self.pt[name]

    def _bn_relu_fwd(self, name, y: Act, out: Act):
        if self.batchnorm:
            if self.training:
                ops.bn_stats(y, self.p[name + ".gamma"], self.p[name + ".beta"], self.bn_affine[name], self.bn_saved[name],
                             self.ws, self.moving[name + ".moving_mean"], self.moving[name + ".moving_variance"],
                             BN_EPS, BN_MOMENTUM)
            else:
                ops.bn_inference_affine(self.p[name + ".gamma"], self.p[name + ".beta"], self.moving[name + ".moving_mean"],
                                        self.moving[name + ".moving_variance"], BN_EPS, self.bn_affine[name])
            ops.bn_apply(y, self.bn_affine[name], out, relu=True)
        else:
            ops.relu_fwd(y, out)

    def _colstat(self, name, dgrad, x: Act, n_out):
        """(rows, buffer) of fused column statistics for conv `name` (forward or data gradient), or (0, None)."""
        key = (name, dgrad)
        if self._cst_gen != ops.config_generation():     # the switches changed: another kernel may serve the layer, with other row counts
            self._cst_rows, self._cst_gen = {}, ops.config_generation()
        if key not in self._cst_rows:
            self._cst_rows[key] = ops.conv2d_colstat_rows(self.geo[name], dgrad, x) if self.dtype == "bf16" else 0
        rows = self._cst_rows[key]
        if rows == 0:
            return 0, None
        need = rows * n_out * 2
        if self._cst_buf is None or self._cst_buf.numel() < need:
            self._cst_buf = torch.empty(need, device=self.device, dtype=torch.float32)
        return rows, self._cst_buf

    def _conv_bn_relu_fwd(self, name, x: Act, y: Act, out: Act):
        """Conv2D -> BatchNormalization -> ReLU (conv_block_1, dl_models/u_net.py:364-371); in bf16 training the batch
        statistics come from the convolution's own epilogue where the serving kernel provides them."""
        p = self.p
        rows, buf = self._colstat(name, 0, x, y.C) if (self.batchnorm and self.training) else (0, None)
        if rows == 0:
            ops.conv2d_fwd(self.geo[name], x, self.wf(name + ".kernel"), p[name + ".bias"], y)
            self._bn_relu_fwd(name, y, out)
            return
        ops.conv2d_fwd_colstat(self.geo[name], x, self.wf(name + ".kernel"), p[name + ".bias"], y, buf)
        # statistics rows -> affine / moving statistics -> BatchNorm + ReLU: one call
        ops.bn_colstat_act_add(buf, rows, y, p[name + ".gamma"], p[name + ".beta"], self.bn_affine[name], self.bn_saved[name], out, 1, None,
                               self.moving[name + ".moving_mean"], self.moving[name + ".moving_variance"], BN_EPS, BN_MOMENTUM)

    def _dgrad_colsum(self, name, dy: Act, dx: Act, bias_grad, c0, c_n):
        """Data gradient of conv `name` plus the bias gradient of the layer that produced its input (channels
        [c0, c0+c_n) of dx summed over pixels), fused into the dgrad epilogue where the serving kernel allows."""
        rows, buf = self._colstat(name, 1, dy, dx.C)
        if rows == 0:
            ops.conv2d_dgrad(self.geo[name], dy, self.wb(name + ".kernel"), dx)
            return False
        ops.conv2d_dgrad_colstat(self.geo[name], dy, self.wb(name + ".kernel"), dx, buf)
        ops.colsum_colstat(buf, rows, dx.C, c0, c_n, bias_grad)
        return True

    def _g_down1(self):
        """dL/d(enc1.down output), for the path without stem_composite (an engine built with it on holds none until then)."""
        if self.g_down[1] is None:
            self.g_down[1] = ops.new_act(self.B, *self.hw[0], self.ch[0], self.device, dtype=self.adt)
        return self.g_down[1]

    def _bn_relu_bwd(self, name, da: Act, y: Act, dy: Act):
        if self.batchnorm:
            ops.bn_bwd(da, y, self.p[name + ".gamma"], self.bn_affine[name], self.bn_saved[name], dy,
                       self.g[name + ".gamma"], self.g[name + ".beta"], self.ws, relu=True)
        else:
            ops.relu_bwd(da, y, dy)

    # ------------------------------------------------------------------ forward
    def forward(self, spec, emb, dropout_mask=None, target=None, global_batch=None, alpha=0.9):
        """spec f32 [B,2,H,W] NCHW, emb int [B,2,16].  With `target` also evaluates compute_loss
        (main_training.py:203-235) and seeds the backward pass.  Returns the NCHW prediction buffer."""
        B, D, p = self.B, self.depth, self.p
        # EngineBase.load_input in pieces: the hand schedule refreshes the work copies before the index conversion and starts the
        # information-vector branch on the side stream before the input conversion, so every check comes first, here
        self._check_batch(spec, "spec")
        self._check_indices(emb)
        if target is not None:
            self._check_batch(target, "target")
        if self.t_dirty or self.training:
            self.refresh_transposed()
        self.set_indices(emb)
        self._last_spec = spec
        self._mask = dropout_mask

        def vec_branch(ws_):
            """information vector branch (dl_models/u_net.py:253-263) up to (bf16: including) its 1x1 conv"""
            ops.embedding_fwd(self.emb_idx, p["vec.embedding"], self.emb_out)
            ops.dense_fwd(self.flat, p["vec.dense.kernel"], p["vec.dense.bias"], self.v, ws_)
            if dropout_mask is not None:
                ops.mul(self.v.base, dropout_mask, self.vd.base)
                vsp_ = self.vd_sp
            else:
                vsp_ = Act(self.v.base.view(B, self.h5, self.w5, VEC_CH))
            if self.dtype != "f32":   # the branch is fp32; its 1x1 conv output joins the bf16 trunk through the Add()
                ops.conv2d_fwd(self.geo["vec.conv"], vsp_, p["vec.conv.kernel"], p["vec.conv.bias"], self.v1x1)
            return vsp_

        vsp = None
        if self.wg_stream is not None:      # independent of the encoder until the Add(): side stream, joined below
            with self._wg() as ws_:
                vsp = vec_branch(ws_)
        ops.nchw_to_nhwc_pad(spec, self.x4)
        prev = self.x4
        for l in range(1, self.L + 1):
            ops.conv2d_fwd(self.geo[f"enc{l}.down"], prev, self.wf(f"enc{l}.down.kernel"), p[f"enc{l}.down.bias"], self.down[l],
                           w_packed=self.ppk.get(f"enc{l}.down.kernel"))
            self._conv_bn_relu_fwd(f"enc{l}.cb1", self.down[l], self.y[l], self.a[l])
            prev = self.a[l]
        if self.wg_stream is None:
            vsp = vec_branch(self.ws)
        else:
            self._join_wg()
        # Add (dl_models/u_net.py:229)
        if self.dtype == "f32":
            ops.conv2d_fwd(self.geo["vec.conv"], vsp, p["vec.conv.kernel"], p["vec.conv.bias"], self.z, addend=self.a[self.L])
        else:
            ops.add_f32_to_bf16(self.a[self.L], self.v1x1, self.z)
        cur = self.z
        for l in range(D, 0, -1):
            c = self.ch[l - 1]
            ops.conv2d_transpose_fwd(self.geo[f"dec{l}.up"], cur, self.wb(f"dec{l}.up.kernel"), p[f"dec{l}.up.bias"],
                                     self.cat[l].slice(c, c))
            self._conv_bn_relu_fwd(f"dec{l}.cb1a", self.cat[l], self.ya[l], self.aa[l])
            self._conv_bn_relu_fwd(f"dec{l}.cb1b", self.aa[l], self.yb[l], self.ab[l])
            cur = self.ab[l]
        if self.s0 == 2:
            ops.head_up2_fwd(cur, self.pf["head.kernel"], p["head.bias"], self.logits)
        elif self.head_direct:
            ops.head6x6_fwd(cur, p["head.kernel"], p["head.bias"], self.logits)
        else:
            ops.conv2d_fwd(self.geo["head"], cur, p["head.kernel"], p["head.bias"], self.logits)
        return self.loss_or_sigmoid(target, global_batch, alpha)

    def loss_or_sigmoid(self, target, global_batch, alpha):
        """The end of a forward pass on the fp32 logits: sigmoid, and with a target compute_loss and dL/dlogits (which seeds backward())."""
        if target is not None:
            gb = self.B if global_batch is None else global_batch
            ops.sigmoid_loss(self.logits, target, alpha, 1.0 / (2.0 * self.H * self.W * gb), self.pred, self.g_logits, self.loss_out, self.ws,
                             **self._loss_extras())
        else:
            ops.sigmoid_nchw(self.logits, self.pred)
        return self.pred

    # ------------------------------------------------------------------ backward
    def backward(self, dpred=None, on_ready=None, include_reg=True):
        """Gradients of every trainable variable into the flat gradient buffer.  Seeds from the loss kernel's
        dL/dlogits (forward(target=...)) or from an upstream dL/dpred (NCHW).  `on_ready(offset_end)` is called
        after the launches that finalise the gradient range [0, offset_end) of the flat buffer have been enqueued."""
        D, p, pt, g, ws = self.depth, self.p, self.pt, self.g, self.ws
        # d/dw of (l2(0.001) * sum w^2) / replicas, folded into the split-K reduction of the weight gradient
        reg = 2.0 * L2_COEF / self.n_replicas if include_reg else 0.0
        if dpred is not None:
            self._check_batch(dpred, "dpred")
            ops.sigmoid_bwd(self.pred, dpred, self.g_logits)

        def ready(name):
            if on_ready is not None:
                self._ready(on_ready, self.specs[name].end)

        gl = self.g_logits
        if self.s0 == 2:
            with self._wg() as ws_:
                ops.head_up2_wgrad(self.ab[1] if D >= 1 else self.a[1], gl, g["head.kernel"], ws_)  # rows 2.. of the padded kernel stay 0
        elif self.head_direct:
            with self._wg() as ws_:
                ops.head6x6_wgrad(self.ab[1] if D >= 1 else self.a[1], gl, g["head.kernel"], ws_)   # rows 2,3 of the padded kernel stay 0
        else:
            with self._wg() as ws_:
                ops.conv2d_wgrad(self.geo["head"], self.ab[1] if D >= 1 else self.a[1], gl, g["head.kernel"], ws_)
        with self._wg() as ws_:
            ops.colsum(gl, g["head.bias"], ws_)
        top = self.ab[1] if D >= 1 else self.a[1]
        g_cur = self.g_ab[1] if D >= 1 else self.g_z
        if self.s0 == 2:
            ops.head_up2_dgrad(gl, self.pf["head.kernel"], g_cur)
        elif self.head_direct and self.dtype == "bf16" and ops.head6x6_dgrad_supported(self.W, self.ch[0]):
            ops.head6x6_dgrad(gl, self.p["head.kernel"], g_cur)         # reads the fp32 master kernel: before ready()
        else:
            ops.conv2d_dgrad(self.geo["head"], gl, self.wb("head.kernel"), g_cur)
        ready("head.bias")      # a group is handed over (all-reduce / optimizer) only after the last reader of its parameters
        for l in range(1, D + 1):
            c = self.ch[l - 1]
            # cb1b
            self._bn_relu_bwd(f"dec{l}.cb1b", self.g_ab[l], self.yb[l], self.g_yb[l])
            with self._wg() as ws_:
                ops.conv2d_wgrad(self.geo[f"dec{l}.cb1b"], self.aa[l], self.g_yb[l], g[f"dec{l}.cb1b.kernel"], ws_, defer=self._rb if self.park_reduces else None)
            if not self.batchnorm:      # a bias in front of BatchNorm has an identically zero gradient (dy sums to 0 per channel)
                with self._wg() as ws_:
                    ops.colsum(self.g_yb[l], g[f"dec{l}.cb1b.bias"], ws_)
            ops.conv2d_dgrad(self.geo[f"dec{l}.cb1b"], self.g_yb[l], self.wb(f"dec{l}.cb1b.kernel"), self.g_aa[l])
            # cb1a
            self._bn_relu_bwd(f"dec{l}.cb1a", self.g_aa[l], self.ya[l], self.g_ya[l])
            with self._wg() as ws_:
                ops.conv2d_wgrad(self.geo[f"dec{l}.cb1a"], self.cat[l], self.g_ya[l], g[f"dec{l}.cb1a.kernel"], ws_, defer=self._rb if self.park_reduces else None)
            if not self.batchnorm:      # a bias in front of BatchNorm has an identically zero gradient (dy sums to 0 per channel)
                with self._wg() as ws_:
                    ops.colsum(self.g_ya[l], g[f"dec{l}.cb1a.bias"], ws_)
            up_bias_done = self._dgrad_colsum(f"dec{l}.cb1a", self.g_ya[l], self.g_cat[l], g[f"dec{l}.up.bias"], c, c)
            # Conv2DTranspose
            g_up = self.g_cat[l].slice(c, c)
            x_in = self.ab[l + 1] if l < D else self.z
            g_in = self.g_ab[l + 1] if l < D else self.g_z
            with self._wg() as ws_:
                ops.conv2d_transpose_wgrad(self.geo[f"dec{l}.up"], x_in, g_up, g[f"dec{l}.up.kernel"], ws_, reg=reg,
                                           w=p[f"dec{l}.up.kernel"], defer=self._rb if self.park_reduces else None)
            if not up_bias_done:
                with self._wg() as ws_:
                    ops.colsum(g_up, g[f"dec{l}.up.bias"], ws_)
            ops.conv2d_transpose_dgrad(self.geo[f"dec{l}.up"], g_up, self.wf(f"dec{l}.up.kernel"), g_in,
                                       w_packed=self.ppk.get(f"dec{l}.up.kernel"))
            ready(f"dec{l}.up.bias")            # after the last reader of this group's parameters (fp32: wf() is the master kernel)
        # bottleneck: z = a_L + conv1x1(dropout(dense(embedding))).  Nothing downstream of the information-vector branch feeds the
        # encoder's backward chain (that needs only g_z), so the whole branch runs on the weight-gradient stream when there is one.
        B = self.B
        has_do = self._mask is not None
        vsp = self.vd_sp if has_do else Act(self.v.base.view(B, self.h5, self.w5, VEC_CH))
        with self._wg() as ws_:
            gz = self.g_z
            if self.dtype == "bf16":      # the information-vector branch is fp32: give it an fp32 copy of dL/dz
                ops.cast_bf16_to_f32(self.g_z, self.g_z32)
                gz = self.g_z32
            ops.conv2d_wgrad(self.geo["vec.conv"], vsp, gz, g["vec.conv.kernel"], ws_)
            ops.colsum(gz, g["vec.conv.bias"], ws_)
            ops.conv2d_dgrad(self.geo["vec.conv"], gz, pt["vec.conv.kernel"], self.g_vd_sp)
            if has_do:
                ops.mul(self.g_vd.base, self._mask, self.g_v.base)
                gv = self.g_v
            else:
                gv = self.g_vd
            ops.conv2d_wgrad(self.geo["vec.dense"], self.flat, gv, g["vec.dense.kernel"], ws_)
            ops.colsum(gv, g["vec.dense.bias"], ws_)
            if self.dense_direct:
                ops.dense_dgrad(gv, p["vec.dense.kernel"], self.g_flat, ws_)           # dL/dflat = dv . W from the kernel as stored
            else:
                ops.dense_fwd(gv, pt["vec.dense.kernel"], None, self.g_flat, ws_)      # the same through the [in][out] copy
            ops.embedding_bwd(self.emb_idx, self.g_emb_out, g["vec.embedding"])
        ready("vec.embedding")
        # encoder, deepest level first; the gradient of a_l is (skip half of g_cat_l) + dgrad of the next strided conv
        g_a = self.g_z
        for l in range(self.L, 0, -1):
            self._bn_relu_bwd(f"enc{l}.cb1", g_a, self.y[l], self.g_y[l])
            with self._wg() as ws_:
                ops.conv2d_wgrad(self.geo[f"enc{l}.cb1"], self.down[l], self.g_y[l], g[f"enc{l}.cb1.kernel"], ws_, defer=self._rb if self.park_reduces else None)
            if not self.batchnorm:
                with self._wg() as ws_:
                    ops.colsum(self.g_y[l], g[f"enc{l}.cb1.bias"], ws_)
            if l == 1 and self.stem_composite:
                # enc1.down and enc1.cb1 are linear with nothing between them and the stem has no data gradient: both stem
                # gradients straight from g_y[1], the input and the bf16 enc1.cb1 kernel the data gradient would have read
                if not self.stem_composite_supported:
                    raise RuntimeError("stem_composite is not available for this engine configuration")
                # on the MAIN stream, which has nothing else left, beside the enc1.cb1 weight gradient on the side stream (behind it on
                # the side stream: 0.07 ms per step slower, scripts/ab_switch.py); the hand-over below waits for both streams
                ops.stem_composite(self.g_y[1], self.x4, self.wb("enc1.cb1.kernel"), g["enc1.down.kernel"], g["enc1.down.bias"],
                                   self.ws, reg=reg, w0=p["enc1.down.kernel"])
                ready("enc1.down.bias")
                break
            g_dn = self.g_down[l] if l > 1 else self._g_down1()
            down_bias_done = self._dgrad_colsum(f"enc{l}.cb1", self.g_y[l], g_dn, g[f"enc{l}.down.bias"], 0, g_dn.C)
            x_in = self.a[l - 1] if l > 1 else self.x4
            with self._wg() as ws_:
                ops.conv2d_wgrad(self.geo[f"enc{l}.down"], x_in, g_dn, g[f"enc{l}.down.kernel"], ws_, reg=reg,
                                 w=p[f"enc{l}.down.kernel"], defer=self._rb if self.park_reduces else None)
            if not down_bias_done:
                with self._wg() as ws_:
                    ops.colsum(g_dn, g[f"enc{l}.down.bias"], ws_)
            ready(f"enc{l}.down.bias")
            if l > 1:
                skip = self.g_cat[l - 1].slice(0, self.ch[l - 2])
                ops.conv2d_dgrad(self.geo[f"enc{l}.down"], g_dn, self.wb(f"enc{l}.down.kernel"), skip, addend=skip)
                g_a = skip
        self._end_backward()

    # ------------------------------------------------------------------ optimizer: DeviceCounters.adam_step / adam_begin / adam_range

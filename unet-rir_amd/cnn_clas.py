"""deep_CNN (dl_models/cnn_clas.py), the room classifier over spectrograms, on graph.GraphEngine: three Conv2D(3x3, 'valid', relu)
blocks of 16 / 32 / 64 filters - each followed by BatchNormalization (optional) and AveragePooling2D(2x2), the last by
GlobalAveragePooling2D - then Dense(256, relu) -> BatchNormalization -> Dropout(.5) -> Dense(classes, softmax) (cnn_clas.py:19-53),
trained on categorical_crossentropy (:63).  The kernels are csrc/cnn_clas.hip; Dense, the Dense BatchNorm, ReLU, Dropout and the
optimizers are the library's existing entry points.  fp32 storage only.

The order inside a block is conv -> ReLU -> BatchNorm (the activation is the Conv2D layer's own), so the statistics are taken over
the ReLU output and nothing follows the normalisation but the pooling.  The BatchNorm affine is per channel and pooling is a mean,
so pool(x * scale + shift) = pool(x) * scale + shift: the normalised full-resolution tensor is never written, one kernel reads the
ReLU output once and writes the pooled, normalised quarter.  Backward composes the plain pooling adjoint with unetrir_bn_bwd_f32
("The room classifier").

PARITY UNPINNED like every graph here: TensorFlow cannot run in this project; the pin is tests/cnn_clas_ref.py, a restatement of
the source text.  Keras reaches the loss through the logits when the softmax op is in sight and through clipped probabilities
otherwise; this build takes the log-softmax of the max-subtracted logits.
"""
import os
import pickle

import numpy as np
import torch

from . import ops
from .ops import Act
from .engine_base import BN_EPS, BN_MOMENTUM
from .graph import GraphEngine, Node, RELU

FILTERS = (16, 32, 64)                    # Conv0_A, Conv1_A, Conv0_C (cnn_clas.py:25, :31, :37)
CONV_NAMES = ("Conv0_A", "Conv1_A", "Conv0_C")
DENSE_UNITS = 256                         # Dense(256, relu) (:43)


def _sizes(H, W):
    """Spatial sizes through the three blocks: [(conv out, pooled)] - 144 x 160: 142x158 -> 71x79 -> 69x77 -> 34x38 -> 32x36."""
    out = []
    for i in range(3):
        if H < 3 or W < 3:
            raise ValueError("deep_CNN: the input is too small for three 3x3 'valid' convolutions with two 2x2 poolings between them")
        H, W = H - 2, W - 2
        conv = (H, W)
        if i < 2:
            H, W = H // 2, W // 2
        out.append((conv, (H, W)))
    return out


def twin_forward(g, x: Act, w, bias, ys: Act, yc: Act, y: Act, relu=True):
    """The 'valid' forward pass composed from the library's 'same' convolution: its interior IS the 'valid' result.  ys: the 'same'
    output [B,H,W,Cout], yc: the cropped pre-activation [B,H-2,W-2,Cout] (a strided copy), y = max(yc, 0)."""
    ops.conv2d_fwd(g, x, w, bias, ys)
    (yc if relu else y).base.copy_(ys.base[:, 1:-1, 1:-1])
    if relu:
        ops.relu_fwd(yc, y)


def twin_dgrad(g, dy: Act, y: Act, wt, dx: Act, gm: Act, dys: Act, relu=True):
    """The 'valid' data gradient composed from the library's 'same' one: the gradients of a zero-ringed dy are the 'valid' gradients.
    gm: dy * [y > 0] [B,H-2,W-2,Cout]; dys [B,H,W,Cout], whose one-pixel ring is zero and stays zero (only the interior is written)."""
    if relu:
        ops.relu_bwd(dy, y, gm)
    dys.base[:, 1:-1, 1:-1].copy_((gm if relu else dy).base)
    ops.conv2d_dgrad(g, dys, wt, dx)


class DeepCNNEngine(GraphEngine):
    """One replica of deep_CNN for a fixed per-replica batch size.  `x` is NCHW [B, depth, H, W] (Keras reads the reference's
    (width, height, depth) as rows, columns, channels: width is H), `target` fp32 [B, classes], one-hot or soft rows.  `probs`
    (= `pred`) is the output buffer, `acc_out` the device count of rows with argmax(logits) == argmax(target) of the last pass with a
    target; `loss_out` = (sum CE / global batch, sum CE, 0, -).  No regulariser: `l2_names` is empty and `reg_out` stays 0."""
    n_dropout_draws = 1
    dropout_p = 0.5                      # Dropout(rate=0.5) (dl_models/cnn_clas.py:46)
    output_act = "softmax"
    # From the measured record (profiles/cnn_clas.json; DESIGN.md "The room classifier"): from this many stored input channels on,
    # a pass composed from the 'same' entry points (twin_forward / twin_dgrad, glue included) beats the 'valid' kernel, and the engine
    # runs the composition.  The weight gradient stays on the 'valid' kernel in every layer.
    TWIN_FWD_MIN_CIN = 32
    TWIN_DGRAD_MIN_CIN = 16

    def __init__(self, H, W, B, depth=2, classes=5, batchnorm=True, device="cuda:0", runtime=None, n_replicas=1, share=None,
                 overlap_wgrad=False, dtype="f32", valid_kernels_only=False):
        """valid_kernels_only: every convolution pass on csrc/cnn_clas.hip, none composed from the 'same' kernels (A/B, tests)."""
        self.valid_kernels_only = bool(valid_kernels_only)
        if dtype == "bf16":
            raise NotImplementedError("deep_CNN runs in fp32 storage; bf16 storage for this model is a follow-up (its largest tensor "
                                      "is cache-resident, so halving it has to be measured first)")
        if depth != 2:
            raise ValueError("deep_CNN: the library's input path carries the two spectrogram planes (depth = 2)")
        if not 1 <= classes <= 1024:
            raise ValueError("deep_CNN: classes must be in [1, 1024]")
        _sizes(H, W)
        super().__init__(B, device, n_replicas, runtime, share, dtype, overlap_wgrad)
        self.H, self.W, self.depth, self.classes, self.batchnorm = H, W, depth, classes, bool(batchnorm)
        self.twin_passes = {}            # layer name -> (forward, data gradient) composed from the 'same' entry points
        self._build()
        self._finalize_params()
        self._alloc_outputs()

    # ------------------------------------------------------------------ node builders
    def _conv_valid(self, x: Node, name, cout, relu=True):
        """Conv2D(cout, 3x3, strides 1, 'valid', activation='relu'); the node holds the ReLU output, whose sign masks dy on load
        in both gradient kernels.  x must have this op as its only consumer."""
        B, cin = self.B, x.a.C
        y = self._new(x.a.H - 2, x.a.W - 2, cout)
        kname, bname = name + ".kernel", name + ".bias"
        pad_in = x is self.x4
        self._param(kname, (cout, 3, 3, cin), "conv_padin" if pad_in else "conv", (3, 3, self.depth if pad_in else cin, cout))
        self._param(bname, (cout,), "bias", (cout,))
        g = ops.geom(B, x.a.H, x.a.W, cin, cout, 3, 1)
        need = ops.conv3x3_valid_wgrad_ws_bytes(g)
        self.ws.reserve(need)
        self.ws_w.reserve(need)
        twin_f = not self.valid_kernels_only and cin >= self.TWIN_FWD_MIN_CIN
        twin_d = not self.valid_kernels_only and cin >= self.TWIN_DGRAD_MIN_CIN and x.needs_grad
        self.twin_passes[name] = (twin_f, twin_d)
        new = lambda h, w: ops.new_act(B, h, w, cout, self.device)
        if twin_f:
            ys, yc = new(x.a.H, x.a.W), new(x.a.H - 2, x.a.W - 2)
        if twin_d:
            gm, dys = new(x.a.H - 2, x.a.W - 2), Act(torch.zeros((B, x.a.H, x.a.W, cout), dtype=torch.float32, device=self.device))

        def fwd():
            if twin_f:
                twin_forward(g, x.a, self.p[kname], self.p[bname], ys, yc, y.a, relu)
            else:
                ops.conv3x3_valid_fwd(g, x.a, self.p[kname], self.p[bname], y.a, relu)

        def dgrad(dst, add):
            if add is not None:
                raise NotImplementedError("the 'valid' convolution is the only consumer of its input")
            if twin_d:
                twin_dgrad(g, y.g, y.a, self.pt[kname], dst, gm, dys, relu)
            else:
                ops.conv3x3_valid_dgrad(g, y.g, y.a, self.pt[kname], dst, relu)

        def bwd():
            with self._wg() as ws_:
                ops.conv3x3_valid_wgrad(g, x.a, y.g, y.a, self.g[kname], self.g[bname], ws_, relu)
            self._emit(x, dgrad)
        self._push(fwd, bwd)
        return y

    def _bn_state(self, name, c):
        """Parameters and buffers of one BatchNormalization layer, as graph.GraphEngine._bn_act keeps them."""
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
        return aff, saved, mm, mv

    def _pool(self, x: Node, bn_name, pool_fwd, pool_bwd, y: Node):
        """(BatchNormalization ->) pooling: statistics of x, then ONE kernel that pools x and applies the affine to the pooled value.
        Backward: the pooling adjoint into a full-resolution buffer, then the BatchNorm backward of the un-pooled tensor."""
        bn = bn_name is not None
        if bn:
            aff, saved, mm, mv = self._bn_state(bn_name, x.a.C)
            da = Act(torch.empty_like(x.a.base))

        def fwd():
            if bn and self.training:
                ops.bn_stats(x.a, self.p[bn_name + ".gamma"], self.p[bn_name + ".beta"], aff, saved, self.ws, mm, mv, BN_EPS, BN_MOMENTUM)
            elif bn:
                ops.bn_inference_affine(self.p[bn_name + ".gamma"], self.p[bn_name + ".beta"], mm, mv, BN_EPS, aff)
            pool_fwd(x.a, aff if bn else None, y.a)

        def bwd():
            if bn:
                pool_bwd(y.g, da)
                ops.bn_bwd(da, x.a, None, aff, saved, x.g, self.g[bn_name + ".gamma"], self.g[bn_name + ".beta"], self.ws, relu=0)
            else:
                pool_bwd(y.g, x.g)
            x.g_set = True
        self._push(fwd, bwd)
        return y

    def _avgpool2(self, x: Node, bn_name=None):
        """(BatchNormalization `bn_name` ->) AveragePooling2D(2x2, strides 2, 'valid'): floor(h/2) x floor(w/2)."""
        return self._pool(x, bn_name, ops.avgpool2_fwd, ops.avgpool2_bwd, self._new(x.a.H // 2, x.a.W // 2, x.a.C))

    def _gap(self, x: Node, bn_name=None):
        """(BatchNormalization `bn_name` ->) GlobalAveragePooling2D: a [B,1,1,C] node."""
        return self._pool(x, bn_name, ops.gap_fwd, ops.gap_bwd, self._new(1, 1, x.a.C))

    def _build(self):
        """deep_CNN.build_model (dl_models/cnn_clas.py:19-53)."""
        bn = (lambda i: f"bn{i}") if self.batchnorm else (lambda i: None)
        x = self._input()
        for i, (name, c) in enumerate(zip(CONV_NAMES, FILTERS)):
            x = self._conv_valid(x, name, c)
            x = self._avgpool2(x, bn(i)) if i < 2 else self._gap(x, bn(i))
        x = self._bn_act(self._dense(x, "dense", DENSE_UNITS), "dense_relu", RELU, batchnorm=False)
        if self.batchnorm:
            x = self._bn_act(x, "bn3", 0)
        x = self._dropout(x, "fc")
        pad = -(-self.classes // 4) * 4          # the logits buffer keeps the 16-byte pixel stride: zero kernel rows behind `classes`
        self.logits = self._conv(x, "dense_1", self.classes, 1, 1, False, followed_by_bn=False, l2=False, dense=True,
                                 pad_out=pad if pad != self.classes else 0)

    # ------------------------------------------------------------------ outputs, gate, passes
    def _alloc_outputs(self):
        dev = self.device
        self.probs = torch.empty((self.B, self.classes), dtype=torch.float32, device=dev)
        self.pred = self.probs
        self.loss_out = torch.zeros(4, dtype=torch.float32, device=dev)
        self.reg_out = torch.zeros(1, dtype=torch.float32, device=dev)
        self.loss_tot = torch.zeros(1, dtype=torch.float32, device=dev)
        self.acc_out = torch.zeros(1, dtype=torch.float32, device=dev)

    def _check_rows(self, t, what):
        """`t` (target or dpred) goes to a kernel as a raw pointer: a contiguous float32 [B, classes] tensor on the engine's device."""
        if tuple(t.shape) != (self.B, self.classes) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
            raise ValueError(f"{what} must be a contiguous float32 [{self.B},{self.classes}] tensor on {self.device}, "
                             f"got {tuple(t.shape)} {t.dtype} on {t.device}")

    def forward(self, x, emb=None, dropout_mask=None, target=None, global_batch=None, alpha=None):
        """emb and alpha are the trainer's calling convention and unused; dropout_mask: what make_dropout_mask() returns."""
        self._check_batch(x, "x")
        if target is not None:
            self._check_rows(target, "target")
        if isinstance(dropout_mask, (tuple, list)):
            (dropout_mask,) = dropout_mask
        self._last_spec = x
        ops.nchw_to_nhwc_pad(x, self.x_in)
        self.masks["fc"] = dropout_mask
        self.run_forward()
        return self.loss_or_sigmoid(target, global_batch, alpha)

    def loss_or_sigmoid(self, target, global_batch, alpha=None):
        """The end of a forward pass: softmax, and with a target the cross-entropy, the accuracy count and dL/dlogits."""
        logits = self.logits
        if target is not None:
            gb = self.B if global_batch is None else global_batch
            ops.softmax_ce(logits.a, self.classes, target, 1.0 / gb, self.probs, logits.g, self.loss_out, self.acc_out)
            logits.g_set = True
        else:
            ops.softmax_fwd(logits.a, self.classes, self.probs)
        return self.probs

    def loss_from_logits(self, target, global_batch=None, alpha=None):
        self._check_rows(target, "target")
        self.loss_or_sigmoid(target, global_batch)

    def backward(self, on_ready=None, dpred=None, include_reg=True):
        """dpred: an upstream gradient on the probabilities [B, classes] instead of the loss kernel's dL/dlogits."""
        if dpred is not None:
            self._check_rows(dpred, "dpred")
            ops.softmax_bwd(self.probs, dpred, self.classes, self.logits.g)
            self.logits.g_set = True
        super().backward(on_ready=on_ready, include_reg=include_reg)

    def make_dropout_mask(self, generator=None):
        return self.dropout_mask(self.mask_width["fc"], generator).view(self.B, 1, 1, -1)


def categorical_crossentropy(y_true, y_pred):
    """tensorflow.keras.losses.categorical_crossentropy on probabilities, per sample: y_pred scaled to sum 1, clipped to
    [1e-7, 1 - 1e-7], -sum(y_true * log(y_pred)).  For callers; the train step computes its loss on the device."""
    p = y_pred / y_pred.sum(-1, keepdim=True)
    return -(y_true * torch.log(p.clamp(1e-7, 1.0 - 1e-7))).sum(-1)


class _ClassifierModel:
    """`model` of the reference class: `model(x, training=False)` -> probabilities [B, classes] (the engine's own output buffer;
    `predict` returns a copy).  x is the reference's NHWC [B, width, height, depth] or NCHW [B, depth, width, height]."""

    def __init__(self, owner):
        self._o = owner

    def __call__(self, x, training=False):
        o = self._o
        x = torch.as_tensor(x)
        if x.dim() != 4:
            raise ValueError("x must be [B, width, height, depth] or [B, depth, width, height]")
        if tuple(x.shape[1:]) != (o.depth, o.width, o.height):
            x = x.permute(0, 3, 1, 2)
        eng = o._engine_for(x.shape[0])
        eng.training = bool(training)
        eng.use_device_counters(False)
        x = x.to(eng.device, torch.float32).contiguous()
        return eng.forward(x, dropout_mask=eng.make_dropout_mask() if training else None)

    def predict(self, x):
        return self(x, training=False).clone()

    @property
    def trainable_variables(self):
        return list(self._o.engine.p.values())

    @property
    def losses(self):
        return []


class deep_CNN:
    """dl_models/cnn_clas.py:4-66 with the reference's constructor; keyword-only additions: `batch_size` (the engine `Trainer` drives),
    `device`, `runtime`.  `Trainer(model, optimizer=model.optimizer, lr=model.learning_rate)` trains it; `return_params()` returns the
    optimizer STRING, as the reference does (its set_optimizer_criterion builds the Keras optimizer and drops it)."""

    def __init__(self, width, height, depth, classes, batchNorm, optimizer, learning_rate, *, batch_size=1, device="cuda:0", runtime=None):
        self.width, self.height, self.depth, self.classes = width, height, depth, classes
        self.batchNorm, self.optimizer, self.learning_rate = batchNorm, optimizer, learning_rate
        self.batch_size, self.device, self.runtime = batch_size, device, runtime
        self.model = None
        self.criterion = None
        self.engine = None
        self._engines = {}

    def build_model(self):
        self.engine = self._new_engine(self.batch_size, None)
        self.engine.reset_parameters()
        self._engines = {self.batch_size: self.engine}
        self.model = _ClassifierModel(self)

    def _new_engine(self, B, share):
        return DeepCNNEngine(self.width, self.height, B, depth=self.depth, classes=self.classes, batchnorm=bool(self.batchNorm),
                             device=self.device, runtime=self.runtime, share=share)

    def _engine_for(self, B):
        if B not in self._engines:
            self._engines[B] = self._new_engine(B, self.engine)
        return self._engines[B]

    def set_optimizer_criterion(self):
        """cnn_clas.py:55-63: the optimizer by substring (nadam, sgd, adam, in that order), criterion = categorical_crossentropy."""
        name = str(self.optimizer)
        self.optimizer_kind = "nadam" if "nadam" in name else "sgd" if "sgd" in name else "adam" if "adam" in name else None
        self.criterion = categorical_crossentropy

    def return_params(self):
        return self.model, self.optimizer, self.criterion

    def save(self, save_folder="."):
        """parameters.pkl (the constructor's arguments) + weights.npz (Keras layouts: HWIO kernels, [in, out] Dense, moving statistics)."""
        os.makedirs(save_folder, exist_ok=True)
        with open(os.path.join(save_folder, "parameters.pkl"), "wb") as f:
            pickle.dump([self.width, self.height, self.depth, self.classes, self.batchNorm, self.optimizer, self.learning_rate], f)
        arrays = {n: np.asarray(v) for n, v in self.engine.export_keras_params().items()}
        arrays.update({"moving/" + n: b.detach().cpu().numpy() for n, b in self.engine.moving.items()})
        np.savez(os.path.join(save_folder, "weights.npz"), **arrays)

    def load_weights(self, weights_path):
        with np.load(weights_path) as z:
            self.engine.load_keras_params({n: z[n] for n in self.engine.specs})
            for n, b in self.engine.moving.items():
                b.copy_(torch.from_numpy(z["moving/" + n]).to(b.device))
        self.engine.t_dirty = True

    @classmethod
    def load(cls, save_folder=".", batch_size=1, device="cuda:0", runtime=None):
        with open(os.path.join(save_folder, "parameters.pkl"), "rb") as f:
            args = pickle.load(f)
        m = cls(*args, batch_size=batch_size, device=device, runtime=runtime)
        m.build_model()
        m.set_optimizer_criterion()
        m.load_weights(os.path.join(save_folder, "weights.npz"))
        return m

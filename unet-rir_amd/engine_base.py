"""What the two engine families share: engine.UNetEngine (the hand-scheduled U-Net) and graph.GraphEngine (the closure-list
executor under UNetGraphEngine and, through ae.AEFamilyEngine, under AutoencoderEngine, ResAEEngine and VAEEngine) differ in their
forward and backward passes only.  The input gate (every tensor a caller hands over is checked before the first launch), the
parameter store, its work copies and Keras layouts, the initialisers, the output buffers, the l2 term, the dropout mask buffers,
the per-step device counters and the side-stream hand-overs of the backward pass live here, once.

Parameters, gradients and Adam moments are four flat fp32 buffers with identical layout, ordered by backward completion so
gradient buckets for the all-reduce are contiguous slices that become final in order; every offset is a multiple of ALIGN.
Kernel layouts: Conv2D [Cout][k][k][Cin], Conv2DTranspose [Cin][k][k][Cout], Dense [out][in] (graph engines: [out][1][1][in]).
"""
import math
import struct
from collections import OrderedDict

import torch

from . import ops
from .device import HipRuntime

BN_EPS = 1e-3          # keras BatchNormalization default (dl_models/u_net.py:368)
BN_MOMENTUM = 0.99
L2_COEF = 1e-3         # l2(0.001) on strided Conv2D / Conv2DTranspose kernels (dl_models/u_net.py:274, :302)
DROPOUT_P = 0.3        # dl_models/u_net.py:260
VOCAB, EMB_DIM, VEC_CH = 2000, 256, 16   # information vector: Embedding(2000, 256), Reshape((h, w, 16)) (dl_models/u_net.py:255-257)
ALIGN = 64             # parameter offsets are multiples of 64 floats (256 B)
# parameter kinds that hold a kernel; *_padin / *_padout: the 2 real input / output channels zero-padded to PAD
KERNEL_KINDS = ("conv", "convT", "conv_padin", "convT_padout", "conv_padout", "dense")


def _aligned(n):
    return -(-n // ALIGN) * ALIGN


def _as_f32(v):
    """v rounded to fp32, as a Python float."""
    return struct.unpack("f", struct.pack("f", float(v)))[0]


class ParamSpec:
    __slots__ = ("name", "shape", "offset", "numel", "kind", "keras_shape")

    def __init__(self, name, shape, kind, keras_shape):
        self.name, self.shape, self.kind, self.keras_shape = name, tuple(shape), kind, tuple(keras_shape)
        self.numel = int(math.prod(shape))
        self.offset = -1

    @property
    def end(self):
        """End of this parameter's aligned range in the flat buffers."""
        return self.offset + _aligned(self.numel)


class _SideStream:
    """`with engine._wg() as ws:` - enqueue on the weight-gradient stream after everything the main stream has queued."""

    def __init__(self, eng):
        self.eng = eng
        self.ctx = None

    def __enter__(self):
        eng = self.eng
        if eng.wg_stream is None:
            return eng.ws
        eng.rt.wait(eng.wg_stream, eng.rt.record())
        self.ctx = eng.rt.on(eng.wg_stream)
        self.ctx.__enter__()
        eng._flush_ready()         # buckets whose hand-over was deferred to this event (see EngineBase._ready)
        return eng.ws_w

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


class DeviceCounters:
    """Mixin of the engines: the per-step scalars (Adam's bias-corrected rate, the dropout draw number) either travel as launch
    arguments computed on the host (default) or live in DEVICE memory, advanced by one tiny kernel at the start of every step
    (`use_device_counters()`): a step then consists of the same launches with the same arguments every time and can be captured
    once into a HIP graph and replayed (trainer.Trainer(graph=True)).  The host mirrors (`adam_t`, `dropout_step`) are kept in
    step either way; checkpoints hold the host values."""
    n_dropout_draws = 1          # dropout masks drawn per step
    dropout_p = DROPOUT_P        # rate of the engine's Dropout layers (aenet.AENetEngine: Dropout(.5), dl_models/ae_net.py:258, :267)
    n_noise_draws = 0            # draws of the same counter made in every forward pass, with or without Dropout (vae.VAEEngine: eps)
    # compute_loss switches (main_training.py:38-39, :214-222); set through trainer.Trainer(sigmoid_loss=, diff_loss=, beta=)
    loss_diff = False            # diff_loss: the phase target is phase_true - phase of the network input
    loss_phase_weight = None     # sigmoid_loss: fp32 [W] column weights of the phase term (device tensor)
    _last_spec = None            # the input of the last forward pass (diff_loss through loss_from_logits)

    def _loss_extras(self):
        ref = self._last_spec if self.loss_diff else None
        if self.loss_diff and ref is None:
            raise RuntimeError("diff_loss needs the network input of the last forward pass")
        return {"phase_ref": ref, "phase_weight": self.loss_phase_weight}

    def use_device_counters(self, on=True):
        dev = self._shared.get("dev")
        if not on:
            if dev is not None:
                dev["on"] = False          # the tensors stay alive: a captured graph may still reference them
            return
        if dev is None:
            dev = self._shared["dev"] = {"state": torch.zeros(3, dtype=torch.int64, device=self.device),
                                         "cfg": torch.zeros(8, dtype=torch.float32, device=self.device),
                                         "hyper": torch.zeros(8, dtype=torch.float32, device=self.device), "cfg_host": None, "offset": 0,
                                         "on": False}
        if not dev["on"]:
            dev["on"] = True
            self.sync_device_counters()

    def _dev(self):
        dev = self._shared.get("dev")
        return dev if (dev is not None and dev["on"]) else None

    def sync_device_counters(self):
        """Host counters -> device (when the mode is switched on, after reset_parameters, after a restored checkpoint)."""
        dev = self._dev()
        if dev is not None:
            dev["state"].copy_(torch.tensor([self.adam_t, self._shared["dropout_step"], self._shared["dropout_step"]], dtype=torch.int64))

    @property
    def device_counters(self):
        return self._dev()

    def begin_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, n_draws=None, forward_only=False):
        """Device counters only: the launch that opens a step (before the dropout masks are drawn; n_draws of them, default
        n_dropout_draws).  forward_only: a pass without an optimizer step (validation) - the Adam step count stays."""
        dev = self._dev()
        if dev is None:
            return
        self.set_step_cfg(lr, beta1, beta2, eps, grad_scale)
        ops.step_advance(dev["state"], dev["cfg"], dev["hyper"], self.n_dropout_draws if n_draws is None else n_draws, not forward_only)
        dev["offset"] = 0

    def set_step_cfg(self, lr, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
        """Device counters only: the optimizer's scalars as the next step_advance launch reads them.  Copies only when a value
        changed (the rate changes once per epoch, main_training.py:342-344): a blocking 20-byte transfer, outside any graph."""
        dev = self._dev()
        if self.optimizer == "lamb":               # the LAMB kernels read the betas and eps from cfg: the selected object's, not Adam's defaults
            o = self._shared["lamb"]["opt"]
            beta1, beta2, eps = o.beta_1, o.beta_2, o.epsilon
        cfg = (float(lr), beta1, beta2, eps, float(grad_scale))
        if dev is not None and dev["cfg_host"] != cfg:
            dev["cfg"][:5].copy_(torch.tensor(cfg, dtype=torch.float32))
            dev["cfg_host"] = cfg

    def _draw_mask(self, buf):
        """Fill `buf` with the next keep mask of this engine's dropout stream."""
        dev = self._dev()
        if dev is None:
            ops.dropout_mask(buf, self.dropout_p, self.dropout_seed, self._shared["dropout_step"])
        else:
            ops.dropout_mask_dev(buf, self.dropout_p, self.dropout_seed, dev["state"], dev["offset"])
            dev["offset"] += 1
        self._shared["dropout_step"] += 1
        return buf

    # "adam" | "nadam" | "sgd" (main_training.py:164-169) | "lamb" (trainer.py:37-38); set through trainer.Trainer(optimizer=)
    optimizer = "adam"

    def set_lamb(self, opt):
        """Select tfa.optimizers.LAMB with the hyperparameters of `opt` (lamb.LAMB).  The segment table - one entry per ParamSpec, the
        exclusion lists resolved into its flags - is built on first use and shared by every engine over this parameter set."""
        self.optimizer = "lamb"
        old = self._shared.get("lamb")
        same_flags = old is not None and opt.segments(self.specs) == old["opt"].segments(self.specs)
        self._shared["lamb"] = {"opt": opt, "table": old["table"] if same_flags else None}

    def _lamb_table(self):
        st = self._shared["lamb"]
        if st["table"] is None:
            st["table"] = ops.make_lamb_table(st["opt"].segments(self.specs), self.device)
        return st["table"]

    def _lamb(self, lo, hi, lr, beta1, beta2, eps, weight_decay, corr1, corr2, grad_scale):
        tab = self._lamb_table()
        if lo is None:
            lo, hi = tab.begin, tab.end
        if not tab.is_range(lo, hi):
            raise ValueError(f"LAMB needs a range of whole variables: [{lo}, {hi}) does not begin and end on a parameter boundary")
        dev = self._dev()
        if dev is None:
            ops.lamb(tab, self.theta, self.grad, self.adam_m, self.adam_v, lo, hi, lr, beta1, beta2, eps, weight_decay, corr1, corr2, grad_scale)
        else:
            ops.lamb_dev(tab, self.theta, self.grad, self.adam_m, self.adam_v, lo, hi, weight_decay, dev["state"], dev["cfg"])
        self.t_dirty = True

    def _adam(self, lo, hi, *args):
        if args[0] == "lamb":
            return self._lamb(lo, hi, *args[1:])
        dev = self._dev()
        th, g, m, v = (self.theta, self.grad, self.adam_m, self.adam_v) if lo is None else \
            (self.theta[lo:hi], self.grad[lo:hi], self.adam_m[lo:hi], self.adam_v[lo:hi])
        if args[0] == "sgd":
            ops.sgd(th, g, args[1], args[2])
        elif args[0] == "nadam":
            ops.nadam(th, g, m, v, *args[1:])
        elif dev is None:
            ops.adam(th, g, m, v, *args)
        else:
            ops.adam_dev(th, g, m, v, dev["hyper"])
        self.t_dirty = True

    def adam_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
        """One optimizer step over the whole flat parameter buffer in one launch (optimizer.apply_gradients, main_training.py:268)."""
        self._adam(None, None, *self.adam_begin(lr, beta1, beta2, eps, grad_scale))

    def adam_begin(self, lr, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
        """Advance the step count once and return the arguments of adam_range for this step (bucket-wise optimizer).  Adam: the
        bias-corrected rate; Nadam: the momentum-schedule coefficients of this step (the running product of the schedule lives
        beside the step count); SGD: the rate; LAMB: the hyperparameters of the selected object (not the beta / eps arguments) and
        the two bias corrections 1 - beta^t."""
        self.adam_t += 1
        t = self.adam_t
        if self.optimizer == "lamb":
            # in fp64 from the betas as the kernels see them (fp32): the expression the device form evaluates from state[0] and cfg
            o = self._shared["lamb"]["opt"]
            b1, b2 = _as_f32(o.beta_1), _as_f32(o.beta_2)
            return ("lamb", lr, o.beta_1, o.beta_2, o.epsilon, o.weight_decay, 1.0 - b1 ** t, 1.0 - b2 ** t, grad_scale)
        if self.optimizer == "sgd":
            return ("sgd", lr, grad_scale)
        if self.optimizer == "nadam":
            mu_t = beta1 * (1.0 - 0.5 * 0.96 ** (0.004 * t))
            mu_t1 = beta1 * (1.0 - 0.5 * 0.96 ** (0.004 * (t + 1)))
            ms_new = self._shared.get("m_schedule", 1.0) * mu_t
            self._shared["m_schedule"] = ms_new
            return ("nadam", lr, beta1, beta2, eps, (1.0 - mu_t) / (1.0 - ms_new), mu_t1 / (1.0 - ms_new * mu_t1), 1.0 / (1.0 - beta2 ** t), grad_scale)
        # the betas as the kernels see them (fp32), so that the launched step and the device-counter step (step_advance_kernel computes
        # the same expression from its fp32 cfg in fp64) produce the same bias-corrected rate bit for bit
        b1, b2 = _as_f32(beta1), _as_f32(beta2)
        return (lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t), beta1, beta2, eps, grad_scale)

    def adam_range(self, lo, hi, *args):
        """The optimizer on the flat parameter range [lo, hi) (element offsets, multiples of the 64-float alignment; LAMB: a range
        of whole parameters, else ValueError)."""
        self._adam(lo, hi, *args)


class EngineBase(DeviceCounters):
    """Construction, parameter store and side-stream plumbing common to every engine (one replica, fixed batch size)."""

    def __init__(self, device, n_replicas, dtype, runtime, share):
        """runtime: stream / event provider (device.HipRuntime by default; the CPU tests pass a simulated one).
        share: another engine of the same class and configuration whose parameters, gradients, Adam moments, work copies and
        BatchNorm moving statistics this one aliases (only the activation buffers depend on the batch size)."""
        self.rt = runtime if runtime is not None else HipRuntime(device)
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        # storage type of activations and their gradients; parameters, statistics and weight gradients are always fp32
        self.dtype = dtype
        self.adt = torch.float32 if dtype == "f32" else torch.bfloat16
        self.PAD = 4 if dtype == "f32" else 8          # channel granule = 16 bytes (zero-padded 2-channel ends)
        self.device = torch.device(device)
        self.n_replicas = n_replicas
        self.training = True
        # state shared by every engine built over one parameter set (the model classes keep one engine per batch size)
        self._shared = share._shared if share is not None else {"adam_t": 0, "t_dirty": True, "dropout_step": 0}
        self.dropout_seed = share.dropout_seed if share is not None else (torch.initial_seed() & 0xFFFFFFFF)
        self._mask_bufs = {}
        self._pending_ready = []
        self.pf = {}                   # folded work copies of a head behind UpSampling2D((2, 2)) (_fold_copy)

    def _init_side_stream(self, share, overlap_wgrad, arena_bytes, park_max_bytes=None):
        """The weight-gradient and optimizer streams (share's when it has them), the side stream's own scratch buffer (as large as
        self.ws is now) and the batch of parked split-K reductions (bf16 storage; ops.ReduceBatch)."""
        self._rb = ops.ReduceBatch(self.device, arena_bytes, park_max_bytes=park_max_bytes) if ops.wgrad_defer_supported(self.dtype) else None
        self.park_reduces = self._rb is not None          # False: every weight gradient reduces its slabs at once (A/B, scripts/ab_switch.py)
        # two probed streams: weight gradients, and the trainer's bucket-wise optimizer (trainer.py)
        if share is not None and overlap_wgrad and share.wg_stream is not None:
            self.wg_stream, self.opt_stream = share.wg_stream, share.opt_stream
        else:
            self.wg_stream, self.opt_stream = self.rt.concurrent_streams(2) if overlap_wgrad else (None, None)
        self.ws_w = ops.Workspace(self.device, self.ws.nbytes) if self.wg_stream is not None else self.ws

    @property
    def adam_t(self):
        return self._shared["adam_t"]

    @adam_t.setter
    def adam_t(self, v):
        self._shared["adam_t"] = v

    @property
    def t_dirty(self):
        """The work copies (transposed / bf16 kernels) are older than the master parameters."""
        return self._shared["t_dirty"]

    @t_dirty.setter
    def t_dirty(self, v):
        self._shared["t_dirty"] = v

    # ------------------------------------------------------------------ parameters
    def _layout_params(self, specs, t_names, h_names, s2_names, share=None):
        """Lay `specs` (backward-completion order) out in the flat buffers theta / grad / adam_m / adam_v (views p, g) and the
        kernels' work copies: fp32 with the channel roles swapped of t_names (theta_t, views pt), bf16 in both orientations of
        h_names (theta_h / theta_th, views ph / pth), and of the 3x3 stride-2 kernels s2_names a third bf16 copy in the order the
        stride-2 forward kernel's LDS-DMA reads it (ppk, csrc/conv3x3d.hip).  share: alias that engine's buffers."""
        for i, s_ in enumerate(specs):
            s_.offset = specs[i - 1].end if i else 0
        self.specs = OrderedDict((s_.name, s_) for s_ in specs)
        if share is not None and [(n, s_.shape) for n, s_ in share.specs.items()] != [(n, s_.shape) for n, s_ in self.specs.items()]:
            raise ValueError("share= needs an engine of the same configuration (only the batch size may differ)")

        def buf(attr, names, dtype, min_elems):
            if share is not None:
                return getattr(share, attr)
            return torch.zeros(max(sum(_aligned(self.specs[n].numel) for n in names), min_elems), dtype=dtype, device=self.device)

        def views(flat, names):
            out, o = {}, 0
            for n in names:
                out[n] = flat[o:o + self.specs[n].numel]
                o += _aligned(self.specs[n].numel)
            return out
        self.theta, self.grad, self.adam_m, self.adam_v = (buf(a, self.specs, torch.float32, 0) for a in ("theta", "grad", "adam_m", "adam_v"))
        self.p = {n: self.theta[s_.offset:s_.offset + s_.numel].view(s_.shape) for n, s_ in self.specs.items()}
        self.g = {n: self.grad[s_.offset:s_.offset + s_.numel].view(s_.shape) for n, s_ in self.specs.items()}
        self.theta_t = buf("theta_t", t_names, torch.float32, 4)
        self.pt = views(self.theta_t, t_names)
        self.ph, self.pth, self.ppk, self._cast_table = {}, {}, {}, None
        if h_names:
            self.theta_h, self.theta_th = buf("theta_h", h_names, torch.bfloat16, 8), buf("theta_th", h_names, torch.bfloat16, 8)
            self.ph, self.pth = views(self.theta_h, h_names), views(self.theta_th, h_names)
            if share is not None:
                self.ppk = share.ppk
            for n in s2_names if share is None else ():
                ne = ops.conv3x3s2_packed_elems(self.specs[n].shape[0], self.specs[n].shape[3])
                if ne:
                    self.ppk[n] = torch.zeros(ne, dtype=torch.bfloat16, device=self.device)

    def _fold_copy(self, kname, c, share=None):
        """The folded work copy [8][4][4][c] of the 6x6 head kernel `kname` behind UpSampling2D((2, 2)) (csrc/head_up2.hip): fp32, on
        a bf16 trunk every tap rounded to bf16 once.  Refreshed with the other work copies; share: alias that engine's."""
        self.pf[kname] = share.pf[kname] if share is not None else \
            torch.zeros(ops.head_up2_folded_elems(c), dtype=torch.float32, device=self.device)
        return self.pf[kname]

    def refresh_transposed(self):
        """Work copies from the fp32 masters: Conv2D / Dense kernels -> [Cin][T][Cout] for dgrad, Conv2DTranspose kernels ->
        [Cout][T][Cin] for forward; the bf16 kernels' copies (both orientations, packed) in one batched launch."""
        for n, t in self.pt.items():
            if n in self.ph:
                continue                                    # bf16 kernels: both work copies come from the cast below
            s_ = self.specs[n]
            N, C_ = s_.shape[0], s_.shape[-1]
            ops.transpose_weight(self.p[n], t, N, s_.numel // (N * C_), C_)
        if self.ph:
            if self._cast_table is None:
                ent = []
                for n in self.ph:
                    s_ = self.specs[n]
                    N, T, C_ = s_.shape[0], s_.shape[1] * s_.shape[2], s_.shape[3]
                    ent.append((self.p[n], self.ph[n], self.pth[n], N, T, C_, C_, N, self.ppk.get(n)))
                self._cast_table = ops.make_cast_table(ent, self.device)
            ops.cast_weights_batched(self._cast_table)
        for n, wf in self.pf.items():
            ops.head_up2_fold(self.p[n], wf, self.specs[n].shape[-1], self.dtype == "bf16")
        self.t_dirty = False

    def reset_parameters(self, generator=None):
        """Keras default initialisers (no initialiser argument in the reference models): glorot_uniform kernels, zero biases,
        gamma 1, beta 0, Embedding U(-0.05, 0.05)."""
        with torch.no_grad():
            for n, s_ in self.specs.items():
                t, ks = self.p[n], s_.keras_shape
                if s_.kind in ("embedding", "codebook"):        # codebook: tf.random_uniform_initializer() (dl_models/vqvae.py:52)
                    t.copy_((torch.rand(s_.shape, generator=generator) * 0.1 - 0.05).to(self.device))
                elif s_.kind in KERNEL_KINDS:
                    if len(ks) == 4:
                        rf = ks[0] * ks[1]
                        fan_in, fan_out = ks[2] * rf, ks[3] * rf
                    else:
                        fan_in, fan_out = ks
                    lim = math.sqrt(6.0 / (fan_in + fan_out))
                    w = ((torch.rand(s_.shape, generator=generator) * 2 - 1) * lim).to(self.device)
                    if s_.kind in ("conv_padin", "convT_padout"):
                        w[..., 2:] = 0
                    if s_.kind == "conv_padout":
                        w[2:] = 0
                    if s_.kind == "dense":             # output units padded to a multiple of 4 (cnn_clas.DeepCNNEngine): zero rows
                        w[ks[1]:] = 0
                    t.copy_(w)
                elif s_.kind == "gamma":
                    t.fill_(1.0)
                else:
                    t.zero_()
            for n, b in self.moving.items():
                b.fill_(1.0 if n.endswith("variance") else 0.0)
            self.adam_m.zero_(); self.adam_v.zero_(); self.adam_t = 0
            self._shared["m_schedule"] = 1.0
        self.t_dirty = True

    # ---- conversion to / from the reference's own (Keras) layouts -----------------------------
    def load_keras_params(self, params):
        """params: name -> array in Keras layout (HWIO Conv2D, HWOI Conv2DTranspose, [in,out] Dense)."""
        with torch.no_grad():
            for n, s_ in self.specs.items():
                a = torch.as_tensor(params[n]).to(torch.float32)
                if tuple(a.shape) != s_.keras_shape:
                    raise ValueError(f"{n}: expected Keras shape {s_.keras_shape}, got {tuple(a.shape)}")
                t = self.p[n]
                if s_.kind in ("conv", "convT"):
                    t.copy_(a.permute(3, 0, 1, 2).to(self.device))
                elif s_.kind in ("conv_padin", "convT_padout"):
                    t.zero_(); t[..., :2].copy_(a.permute(3, 0, 1, 2).to(self.device))
                elif s_.kind == "conv_padout":
                    t.zero_(); t[:2].copy_(a.permute(3, 0, 1, 2).to(self.device))
                elif s_.kind == "dense" and a.shape[1] == t.shape[0]:
                    t.copy_(a.t().reshape(t.shape).to(self.device))
                elif s_.kind == "dense":               # output units zero-padded to a multiple of 4
                    t.zero_(); t.view(t.shape[0], -1)[:a.shape[1]].copy_(a.t().to(self.device))
                elif s_.kind == "bias_pad":
                    t.zero_(); t[:a.shape[0]].copy_(a.to(self.device))
                else:
                    t.copy_(a.to(self.device))
        self.t_dirty = True

    def _to_keras(self, views):
        out = {}
        for n, s_ in self.specs.items():
            t = views[n].detach()
            if s_.kind in ("conv", "convT"):
                a = t.permute(1, 2, 3, 0)
            elif s_.kind in ("conv_padin", "convT_padout"):
                a = t[..., :2].permute(1, 2, 3, 0)
            elif s_.kind == "conv_padout":
                a = t[:2].permute(1, 2, 3, 0)
            elif s_.kind == "dense":
                a = t.reshape(t.shape[0], -1)[:s_.keras_shape[1]].t()
            elif s_.kind == "bias_pad":
                a = t[:s_.keras_shape[0]]
            else:
                a = t
            out[n] = a.contiguous().cpu()
        return out

    def export_keras_params(self):
        return self._to_keras(self.p)

    def export_keras_grads(self):
        return self._to_keras(self.g)

    def n_params(self):
        """Trainable parameter count in the reference's sense (padding excluded)."""
        return sum(int(math.prod(s_.keras_shape)) for s_ in self.specs.values())

    # ------------------------------------------------------------------ the input gate
    def _check_batch(self, t, what):
        """`t` (`what`: spec, target or dpred) goes to a kernel as a raw pointer: anything but a contiguous float32 [B,2,H,W]
        tensor on the engine's device is refused here, before any launch (a host pointer handed to a kernel is a GPU memory
        fault, not an exception)."""
        if tuple(t.shape) != (self.B, 2, self.H, self.W) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
            raise ValueError(f"{what} must be a contiguous float32 [{self.B},2,{self.H},{self.W}] tensor on {self.device}, "
                             f"got {tuple(t.shape)} {t.dtype} on {t.device}")

    def _check_indices(self, emb):
        if tuple(emb.shape) != (self.B,) + self.inf_vector_shape:
            raise ValueError(f"emb must be [{self.B},{self.inf_vector_shape}], got {tuple(emb.shape)}")

    def set_indices(self, emb):
        """The information vector's indices (any integer type, host or device) as int32 in the engine's index buffer."""
        self._check_indices(emb)
        if emb.dtype not in (torch.int32, torch.int64):
            emb = emb.to(torch.int64)
        if emb.device != self.device:      # DataGenerator.__getitem__ hands over host arrays: a small copy, never a host pointer
            emb = emb.to(self.device)
        ops.index_to_i32(emb.contiguous(), self.emb_idx)

    def load_input(self, spec, emb):
        """Check both inputs, then convert them into the engine's buffers: the indices, and the NCHW batch into the padded NHWC
        input `x_in`.  `spec` is remembered for diff_loss (the phase target is taken relative to the input's phase)."""
        self._check_batch(spec, "spec")
        self.set_indices(emb)
        self._last_spec = spec
        ops.nchw_to_nhwc_pad(spec, self.x_in)

    def _alloc_outputs(self):
        """The NCHW prediction and the loss scalars: loss_out = (data loss, amplitude sum, phase sum, -), the l2 terms, their sum."""
        dev = self.device
        self.pred = torch.empty((self.B, 2, self.H, self.W), dtype=torch.float32, device=dev)
        self.loss_out = torch.zeros(4, dtype=torch.float32, device=dev)
        self.reg_out = torch.zeros(1, dtype=torch.float32, device=dev)
        self.loss_tot = torch.zeros(1, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------ loss
    def loss_from_logits(self, target, global_batch=None, alpha=0.9):
        """compute_loss for the logits of the last forward pass: rewrites the prediction (same values), the data loss and
        dL/dlogits, which seeds backward()."""
        self._check_batch(target, "target")
        self.loss_or_sigmoid(target, global_batch, alpha)

    def reg_loss(self, into=None, accumulate=False):
        """sum(model.losses) / replicas (main_training.py:232-233), evaluated on device into reg_out[0] (or added to `into`[0])."""
        out = self.reg_out if into is None else into
        first = not accumulate
        for n in self.l2_names:
            s_ = self.specs[n]
            ops.sumsq(self.theta[s_.offset:s_.offset + s_.numel], L2_COEF / self.n_replicas, out, not first, self.ws)
            first = False
        if first:
            out.zero_()
        return out

    def loss_total(self):
        """Data loss + l2 terms as one device scalar (a 4-byte copy and the l2 reductions accumulating onto it)."""
        self.loss_tot.copy_(self.loss_out[0:1])
        self.reg_loss(into=self.loss_tot, accumulate=True)
        return self.loss_tot

    def make_dropout_mask(self, generator=None):
        """The U-Net engines' keep mask of Dropout(.3) on the information vector, [B, vec_dim] (the autoencoder family draws its own)."""
        return self.dropout_mask(self.vec_dim, generator)

    def dropout_mask(self, n, generator=None, slot=0):
        """Keep mask [B, n] of Dropout(dropout_p) scaled by 1/(1-p).  Default: the HIP generator kernel, draw number `dropout_step` of
        stream `dropout_seed` (reproducible; the trainer offsets the seed by the replica rank), written into one reused buffer
        per `slot`.  With a torch generator: torch's own stream of random numbers (tests)."""
        if generator is not None:
            return (torch.rand((self.B, n), device=self.device, generator=generator) >= self.dropout_p).to(torch.float32) / (1.0 - self.dropout_p)
        buf = self._mask_bufs.get(slot)
        if buf is None or buf.shape[1] != n:
            buf = self._mask_bufs[slot] = torch.empty((self.B, n), dtype=torch.float32, device=self.device)
        return self._draw_mask(buf)

    # ------------------------------------------------------------------ side stream
    def _wg(self):
        return _SideStream(self)

    def _ready(self, on_ready, off):
        """The gradient range [0, off) of the flat buffer is final once the launches queued so far have run: hand it over.
        A bucket's gradients come from both streams (weight gradients: side stream; BatchNorm / fused bias / data gradients:
        main stream).  With a side stream, the SIDE stream hands the bucket over once it has waited for the main stream's
        progress: the all-reduce orders after both and the main stream never blocks on the side stream.  That wait is the one the
        next `with self._wg()` performs anyway, so the hand-over is parked until then instead of putting an event record of its
        own into the main stream (each costs ~8 us of dispatch gap; later is always safe)."""
        if self.wg_stream is None:
            self._hand_over(on_ready, off)
        else:
            self._pending_ready.append((on_ready, off))

    def _hand_over(self, fn, off):
        """on_ready(off): the gradient range [0, off) is final.  A consumer that does not run the parked split-K reductions itself
        (the trainer's bucketer does, lazily, at its bucket boundaries: GradBucketer.before_bucket) gets them run first."""
        if getattr(getattr(fn, "__self__", None), "before_bucket", None) is None:
            self.flush_reduces()
        fn(off)

    def flush_reduces(self):
        """Run the parked split-K reductions (on the current stream: the one the weight gradients ran on).  Called by the trainer's
        bucketer before a bucket's gradients are first read, and at the end of backward()."""
        if self._rb is not None:
            self._rb.flush()

    def _flush_ready(self):
        """Called on the side stream right after it has waited for the main stream: hand over the parked buckets."""
        pend, self._pending_ready = self._pending_ready, []
        for fn, off in pend:
            self._hand_over(fn, off)

    def _join_wg(self):
        if self.wg_stream is not None:
            self.rt.wait(self.rt.current_stream(), self.rt.record(self.wg_stream))

    def _end_backward(self):
        """Hand over what is still parked (the bucketer runs the parked reductions first), run the reductions nobody asked for
        yet, and join the side stream: the optimizer and the next forward (which overwrites activations) must see every
        weight gradient."""
        if self._pending_ready or (self._rb is not None and len(self._rb)):
            with self._wg():
                self.flush_reduces()
        self._join_wg()

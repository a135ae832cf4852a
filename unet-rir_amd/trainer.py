"""Train step and data parallelism.

``Trainer.step`` is the counterpart of ``train_step`` in main_training.py:253-290 (and of the legacy
``Trainer.step`` of trainer.py:133-144): forward, compute_loss, gradients of every trainable variable, gradient
all-reduce across replicas, Adam apply.  Data parallelism follows tf.distribute.MirroredStrategy
(main_training.py:56, :114-117, :323-327): one process per GPU, the global batch is split evenly, every replica
holds the full model, BatchNorm statistics stay per replica, the loss is normalised by the GLOBAL batch so
gradients are SUM-reduced.  The collective is RCCL (torch.distributed backend "nccl") over xGMI, issued per
bucket while the backward pass is still running.
"""
import gc
import os

import torch
import torch.distributed as dist

from .lamb import LAMB


class GradBucketer:
    """Cuts a flat gradient buffer, laid out in backward-completion order, into contiguous buckets and all-reduces
    (SUM) each bucket as soon as the backward pass has produced it.  Device agnostic: the same object drives RCCL
    on GPUs and gloo in the CPU tests."""

    def __init__(self, flat_grad, boundaries, bucket_bytes=32 << 20, group=None, reduce=True, on_bucket=None, runtime=None,
                 before_bucket=None):
        """boundaries: increasing element offsets at which a gradient range [0, off) can become final.
        reduce=False: no collective (single replica), only the bucket schedule.  on_bucket(lo, hi, work) is called for
        every bucket right after its all-reduce has been launched (work is None without a collective): the hook the
        trainer uses to start the optimizer on finished buckets while the backward pass is still running."""
        self.flat = flat_grad
        self.group = group
        self.rt = runtime          # device.HipRuntime (or the tests' simulated one); None: plain torch.distributed calls
        self.reduce = reduce
        self.on_bucket = on_bucket
        # called (on the stream the engine hands buckets over from) before a bucket's gradients are first read: the engines park the
        # split-K reductions of their weight gradients until then and run them in one launch (engine.flush_reduces)
        self.before_bucket = before_bucket
        self.bounds = []
        last, limit = 0, max(bucket_bytes // 4, 1)
        for off in boundaries:
            if off - last >= limit:
                self.bounds.append(off)
                last = off
        n = flat_grad.numel()
        if not self.bounds or self.bounds[-1] != n:
            self.bounds.append(n)
        self.reset()

    def reset(self):
        self.next = 0
        self.sent = 0
        self.works = []

    def buckets(self):
        lo = 0
        for hi in self.bounds:
            yield lo, hi
            lo = hi

    def mark_ready(self, offset_end):
        """Everything in [0, offset_end) is final (the launches that write it are enqueued)."""
        while self.next < len(self.bounds) and self.bounds[self.next] <= offset_end:
            hi = self.bounds[self.next]
            work = None
            if self.before_bucket is not None:
                self.before_bucket()
            if self.reduce:
                if self.rt is not None:
                    work = self.rt.all_reduce_sum(self.flat[self.sent:hi], self.group)
                else:
                    work = dist.all_reduce(self.flat[self.sent:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                self.works.append(work)
            if self.on_bucket is not None:
                self.on_bucket(self.sent, hi, work)
            self.sent = hi
            self.next += 1

    def finish(self):
        self.mark_ready(self.flat.numel())
        for w in self.works:
            if self.rt is not None:
                self.rt.wait_work(w)
            else:
                w.wait()
        self.works = []
        self.next = 0
        self.sent = 0


def phase_weight(beta, W):
    """preprocess.sigmoid(beta, (H, W)) (preprocess.py:116-121): every row of the mask the `sigmoid_loss` switch multiplies into
    the phase term is z = 1 / (1 + exp(-(x + 5) beta)) on x = linspace(-10, 10, W), flipped.  fp32 [W]."""
    x = torch.linspace(-10.0, 10.0, W, dtype=torch.float64)
    return torch.flip(1.0 / (1.0 + torch.exp(-(x + 5.0) * beta)), dims=(0,)).to(torch.float32)


def lr_schedule(lr0, epoch, decay=(True, 80)):
    """main_training.py:342-344: from epoch >= 80 the rate is lr0 * 0.9 ** (epoch / 80)."""
    if decay and decay[0] and epoch >= decay[1]:
        return lr0 * 0.9 ** (epoch / decay[1])
    return lr0


# The engines' own metrics: (record key, device counter of the engine, index of the raw per-step sum in it, attribute holding the
# number of elements a step sums over - None: the batch size).  VAE: train_kl / val_kl, tf.keras.metrics.Mean over every (b, l) element
# of kl_loss_object (main_training.py:246-250, :286-288, :318-320); VQ-VAE: mean((q - x)^2) over every element of the quantiser's
# S (dl_models/vqvae.py:79-80); the classifier: correct rows over rows seen.  An engine with one of them has a loss term or target of
# its own, and takes no term on the waveform.
ENGINE_METRICS = (("kl", "kl_out", 1, "kl_elems"), ("vq", "vq_out", 1, "vq_elems"), ("acc", "acc_out", 0, None))


class _LossFunction(torch.autograd.Function):
    """compute_loss of main_training.py:203-235 as an autograd node over the engine's fused sigmoid + loss kernel: the value is
    the per-replica scalar, backward() runs the engine's whole backward pass (and, through the trainer, the gradient
    all-reduce and the optimizer of finished buckets)."""

    @staticmethod
    def forward(ctx, trainer, anchor, loss_value):
        ctx.trainer = trainer
        return loss_value.view(())

    @staticmethod
    def backward(ctx, g):
        ctx.trainer._backward_and_reduce()           # loss.backward() passes d(loss)/d(loss) = 1
        return None, None, None


class Trainer:
    """One call of ``step`` = one ``distributed_train_step`` of main_training.py:323-327 on this replica.

    `model` is an engine (UNetEngine, UNetGraphEngine, ResAEEngine) or a boundary module holding one (`UNet`, `ResAE`: then
    the engine built for the module's `batch_size` is driven).  Two ways to run a step:

      trainer.step(spec_in, emb, spec_out)                       # everything in one call (NCHW shards)

      pred = model.model([spec_in, emb], training=True)          # the reference's own loop shape, main_training.py:253-290
      loss = trainer.compute_loss(spec_out, pred)                #   compute_loss(spec_out, spec_generated, model.losses)
      loss.backward()                                            #   tape.gradient  (+ all-reduce + Adam of finished buckets)
      trainer.apply_gradients()                                  #   optimizer.apply_gradients
    """

    def __init__(self, model, lr=None, alpha=0.9, world_size=1, group=None, bucket_bytes=32 << 20, dropout=True, force_dp=False,
                 sigmoid_loss=False, diff_loss=False, beta=0.5, graph=False, dropout_seed=None, optimizer="adam", wave_loss=None, decay_loss=None,
                 spectral_loss=None):
        """force_dp: run the bucketed all-reduce path even at world_size 1 (needs an initialised process group; rehearsal).
        sigmoid_loss / diff_loss / beta: the switches of compute_loss (main_training.py:38-40, :214-222; both False in the
        reference's live configuration): column weights sigmoid(beta, ...) of preprocess.py:116-121 on the phase term, and the
        phase target taken relative to the input's phase.
        graph: capture `step` once into a HIP graph (after one ordinary step that is undone) and replay it - one host call per
        step instead of several hundred launches; single-replica steps without an externally supplied dropout mask only
        (anything else runs the ordinary way).
        optimizer: "adam" (the live configuration), "nadam" or "sgd" - main_training.py:164-169 selects by substring, so does this -
        or a `unet_rir_amd.LAMB(...)` object: tfa.optimizers.LAMB of the legacy trainer (trainer.py:37-38).
        lr: the rate of every step that is not given one (`step(..., lr=)`).  Default 5e-7, or the LAMB object's learning_rate.
        dropout_seed: base seed of the Dropout streams; replica r draws from stream seed + r (independent masks per replica, as
        under MirroredStrategy).  Default: the engine's own seed (torch.initial_seed()).
        wave_loss, decay_loss, spectral_loss: a `unet_rir_amd.WaveLoss`, `DecayLoss`, `SpectralLoss` - every step then also minimises
        the term on the waveform the prediction reconstructs to (`step(..., wav_true=)`), all of one geometry.  The loss kernel runs as
        before (loss_out[1:3] keep their meaning, loss_out[0] grows by every term); behind it runs one chain (`_waveform_terms`): the
        wave-loss call (csrc/waveloss.hip), which yields dL/dpred of its own and of the spectrogram term and hands over the waveform;
        the decay term, then the spectral term, the first writing its cotangent on the waveform and the next adding to it; and ONE
        vector-Jacobian product (csrc/istft_bwd.hip) that adds the sum onto dpred, from which the backward pass starts instead of the
        loss kernel's dL/dlogits.  For a decay_loss or spectral_loss without a `wave_loss` the trainer keeps one of weight 0 - an exact
        zero whose launch yields the waveform and the spectrogram loss's dL/dpred.  Engines with a loss term or target of their own
        (ENGINE_METRICS: VAE, VQ-VAE, the classifier) are refused."""
        self.module = None
        engine = model
        if not hasattr(model, "specs") and hasattr(model, "engine"):
            self.module = model
            engine = model.engine
            if engine is None:
                raise RuntimeError("build the model first (batch_size=...): the trainer drives the engine of one batch size")
        self.engine = engine
        self.rt = engine.rt
        self.wave_loss = wave_loss
        self.decay_loss = decay_loss
        self.spectral_loss = spectral_loss
        self._wave = wave_loss              # the WaveLoss the step calls: the user's, or for a decay_loss / spectral_loss without one, one of weight 0
        self._terms = tuple(t for t in (decay_loss, spectral_loss) if t is not None)       # on the waveform that call hands over, in launch order
        given = [(n, t, w) for n, t, w in (("wave_loss", wave_loss, "waveform"), ("decay_loss", decay_loss, "decay"),
                                           ("spectral_loss", spectral_loss, "spectral")) if t is not None]
        self._wave_option = given[0][0] if given else None        # the first of the options set: the one the messages name
        geo = lambda o: (o.des_shape, o.n_fft, o.win_length, o.hop_length)
        for name, term, what in given:
            own = [attr for _, attr, _, _ in ENGINE_METRICS if hasattr(engine, attr)]
            if own:
                raise ValueError(f"{name}: {type(engine).__name__} has a loss term or target of its own ({own[0]}); the {what} loss "
                                 "drives the spectrogram models only")
            if self._wave is None:
                from .waveloss import WaveLoss
                self._wave = WaveLoss(0.0, "mse", None, *geo(term))
                self._wave.prepare(engine.device, engine.B)
            elif geo(self._wave) != geo(term):
                raise ValueError(f"{name}: its geometry {geo(term)} differs from the {self._wave_option}'s {geo(self._wave)}")
            if term is not wave_loss:
                term.prepare(engine.device, engine.B)
        if lr is None:
            lr = optimizer.learning_rate if isinstance(optimizer, LAMB) else 5e-7
        self.lr, self.alpha = lr, alpha
        self.world_size = world_size
        self.group = group
        self.dropout = dropout
        self.bucketer = None
        engine.n_replicas = world_size
        dp = world_size > 1 or (force_dp and dist.is_initialized())
        # per-replica Dropout streams: the engine's seed is process-wide (torch.initial_seed()), identical in every rank
        if dropout_seed is not None:
            engine.dropout_seed = int(dropout_seed) & 0xFFFFFFFF
        self.rank = dist.get_rank(group) if (world_size > 1 and dist.is_initialized()) else 0
        if world_size > 1 and not getattr(engine, "_seed_offset_by_rank", False):
            engine.dropout_seed = (engine.dropout_seed + self.rank) & 0xFFFFFFFF
            engine._seed_offset_by_rank = True
        engine.loss_diff = bool(diff_loss)
        engine.loss_phase_weight = phase_weight(beta, engine.W).to(engine.device) if sigmoid_loss else None
        if isinstance(optimizer, LAMB):
            engine.set_lamb(optimizer)
        else:
            opt = str(optimizer).lower()
            if "adam" not in opt and "sgd" not in opt:
                raise ValueError("optimizer must name adam, nadam or sgd (main_training.py:164-169) or be a unet_rir_amd.LAMB object "
                                 "(trainer.py:37-38)")
            engine.optimizer = "nadam" if "nadam" in opt else ("sgd" if "sgd" in opt else "adam")
        self.use_graph = bool(graph) and not dp and engine.optimizer in ("adam", "lamb")
        self._graphs, self._g_in = {}, None
        # With a side stream in the engine (overlap_wgrad) the optimizer also leaves the critical path: Adam runs bucket by
        # bucket on a third stream as soon as a bucket's gradients are final (and, data-parallel, all-reduced), while the
        # backward pass continues.  A finished bucket's parameters are never read again by that backward pass.
        self.adam_stream = getattr(engine, "opt_stream", None) if getattr(engine, "wg_stream", None) is not None else None
        self._adam_args = None
        self._lr_now = lr
        self._pending = False
        self._total_on_device = False
        self._anchor = torch.zeros((), device=engine.device, requires_grad=True)     # makes compute_loss() a graph leaf's consumer
        if dp or self.adam_stream is not None:
            bounds = [s_.end for s_ in engine.specs.values()]
            self.bucketer = GradBucketer(engine.grad, bounds, bucket_bytes, group, reduce=dp,
                                         on_bucket=self._adam_bucket if self.adam_stream is not None else None, runtime=self.rt,
                                         before_bucket=getattr(engine, "flush_reduces", None))

    def broadcast_parameters(self, src=0):
        """Replicas start from identical variables (MirroredStrategy mirrors them at creation)."""
        if self.world_size > 1:
            self.rt.broadcast(self.engine.theta, src, self.group)
            for b in self.engine.moving.values():
                self.rt.broadcast(b, src, self.group)
            self.engine.t_dirty = True

    def _adam_bucket(self, lo, hi, work):
        """Adam on parameters [lo, hi) once everything queued so far on the calling stream (the engine hands buckets over
        from its side stream, which has waited for the main stream) and the bucket's all-reduce are done."""
        rt = self.rt
        ev = rt.record()
        with rt.on(self.adam_stream):
            rt.wait(self.adam_stream, ev)
            if work is not None:
                rt.wait_work(work)
            self.engine.adam_range(lo, hi, *self._adam_args)

    # ---- the three phases of a step after the forward pass
    def _backward_and_reduce(self, dpred=None):
        """tape.gradient + the cross-replica SUM (+ Adam of every bucket that is final, when the optimizer has its own stream).
        dpred: dL/dpred (NCHW) to start from instead of the loss kernel's dL/dlogits (the waveform loss)."""
        eng = self.engine
        if self.adam_stream is not None:
            self._adam_args = eng.adam_begin(self._lr_now)
        if self.bucketer is not None:
            self.bucketer.reset()
            eng.backward(on_ready=self.bucketer.mark_ready, dpred=dpred)
        else:
            eng.backward(dpred=dpred)
        self._pending = True

    def apply_gradients(self):
        """optimizer.apply_gradients (main_training.py:268): waits for the all-reduce, applies Adam (the part of it that has not
        already run bucket by bucket), joins the optimizer stream."""
        if not self._pending:
            raise RuntimeError("apply_gradients() without a backward pass")
        eng, rt = self.engine, self.rt
        if self.bucketer is not None:
            self.bucketer.finish()              # hands over the last bucket(s); every all-reduce is waited for
        if self.adam_stream is not None:
            rt.wait(rt.current_stream(), rt.record(self.adam_stream))
            eng.t_dirty = True
        else:
            eng.adam_step(self._lr_now)
        self._pending = False

    def _make_mask(self):
        eng = self.engine
        side = getattr(eng, "wg_stream", None) if getattr(eng, "mask_on_side_stream", False) else None
        if side is not None:       # its only consumers (the information-vector branch, forward and backward) run on that stream
            if eng.device_counters is not None:          # the draw number comes from the step_advance launch of the main stream
                self.rt.wait(side, self.rt.record())
            with self.rt.on(side):
                return eng.make_dropout_mask()
        return eng.make_dropout_mask()

    def _step_body(self, spec_in, emb, spec_out, dropout_mask, with_reg, wav_true=None):
        """The launches of one step (what a HIP graph captures)."""
        eng = self.engine
        # device counters only; an engine's own noise (VAE: eps of the sampling layer) is drawn whatever the Dropout setting
        eng.begin_step(self._lr_now, n_draws=(eng.n_dropout_draws if (dropout_mask is None and self.dropout) else 0) + eng.n_noise_draws)
        if dropout_mask is None and self.dropout:
            dropout_mask = self._make_mask()
        gb = eng.B * self.world_size
        eng.forward(spec_in, emb, dropout_mask=dropout_mask, target=spec_out, global_batch=gb, alpha=self.alpha)
        if with_reg:
            eng.reg_loss()                      # on the pre-update weights, as compute_loss sees them
        dpred = None if self._wave is None else self._waveform_terms(spec_in, spec_out, wav_true)
        self._backward_and_reduce(dpred)
        self.apply_gradients()

    def _waveform_terms(self, spec_in, spec_out, wav_true, backward=True):
        """Everything on the current stream behind the loss kernel: the wave-loss call - dL/dpred of the waveform term and of the
        spectrogram term in one launch, and the waveform for the terms on it; those terms in order, the first writing its cotangent on
        the waveform into its own buffer, the next adding to that buffer; and, issued by the last of them, the one vector-Jacobian
        product that adds the sum onto dpred.  -> dpred.  backward=False (a validation batch): the losses alone, -> None."""
        eng = self.engine
        gb = eng.B * self.world_size
        phase_ref = spec_in if eng.loss_diff else None
        fused = dict(spec_target=spec_out, alpha=self.alpha, inv_norm=1.0 / (2.0 * eng.H * eng.W * gb),
                     phase_weight=eng.loss_phase_weight) if backward else {}
        dpred = self._wave(eng.pred, wav_true, phase_ref=phase_ref, global_batch=gb, loss_out=eng.loss_out, want_wav=bool(self._terms),
                           backward=backward, **fused)
        dwav = None
        for term in self._terms:
            onto_dpred = dict(pred=eng.pred, phase_ref=phase_ref, dpred=dpred, accumulate=True) if backward and term is self._terms[-1] else {}
            dwav = term(self._wave.wav_pred, wav_true, dwav=dwav, global_batch=gb, loss_out=eng.loss_out, backward=backward, **onto_dpred)
        return dpred

    def step(self, spec_in, emb, spec_out, dropout_mask=None, lr=None, return_loss=False, wav_true=None):
        """inputs as DataGenerator.__getitem__ yields them (datageneratorv2.py:101-102), NCHW, per-replica shard.  wav_true fp32
        [B, T]: the target waveforms, with a `wave_loss` (DataGenerator(characteristics=True) delivers them)."""
        eng = self.engine
        if self._wave is None:
            wav_true = None
        elif wav_true is None:
            raise ValueError(f"this trainer has a {self._wave_option}: step(..., wav_true=) needs the target waveforms")
        eng.training = True
        self._total_on_device = False
        self._lr_now = self.lr if lr is None else lr
        if self.use_graph and dropout_mask is None:
            self._graph_step(spec_in, emb, spec_out, bool(return_loss), wav_true)
        else:
            if self.use_graph:
                eng.use_device_counters(False)     # e.g. an externally supplied mask: launch arguments from the host again
            self._step_body(spec_in, emb, spec_out, dropout_mask, return_loss, wav_true)
        if return_loss:
            return self.last_loss()
        return None

    # ---- the step as a HIP graph
    def _snapshot(self):
        eng = self.engine
        return {"theta": eng.theta.clone(), "m": eng.adam_m.clone(), "v": eng.adam_v.clone(), "adam_t": eng.adam_t,
                "moving": {k: v.clone() for k, v in eng.moving.items()}, "dropout_step": eng._shared["dropout_step"]}

    def _restore(self, snap):
        eng = self.engine
        eng.theta.copy_(snap["theta"]); eng.adam_m.copy_(snap["m"]); eng.adam_v.copy_(snap["v"])
        for k, v in snap["moving"].items():
            eng.moving[k].copy_(v)
        eng.adam_t = snap["adam_t"]
        eng._shared["dropout_step"] = snap["dropout_step"]
        eng.t_dirty = True
        eng.sync_device_counters()

    def _graph_step(self, spec_in, emb, spec_out, with_reg, wav_true=None):
        """Replay the captured step on copies of the inputs.  First call (per variant: with / without the l2 terms of the reported
        loss): one ordinary step with the counters in device memory - every lazily created buffer, table and workspace then
        exists - undone from a snapshot, then the capture."""
        eng, rt = self.engine, self.rt
        eng.use_device_counters(True)          # (re-)synchronises the device counters when another path ran in between
        if self._g_in is None:
            if emb is not None and emb.dtype not in (torch.int32, torch.int64):
                emb = emb.to(torch.int64)
            self._g_in = (spec_in.to(eng.device, torch.float32).contiguous().clone(),
                          None if emb is None else emb.to(eng.device).contiguous().clone(),      # None: an engine without an information vector
                          spec_out.to(eng.device, torch.float32).contiguous().clone(),
                          None if wav_true is None else wav_true.to(eng.device, torch.float32).contiguous().clone())    # with a wave_loss
        for dst, src in zip(self._g_in, (spec_in, emb, spec_out, wav_true)):
            if dst is None and src is None:
                continue
            if dst is None or src is None or tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"graph step: input shape {None if src is None else tuple(src.shape)} differs from the captured "
                                 f"{None if dst is None else tuple(dst.shape)}")
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src, non_blocking=True)
        eng.set_step_cfg(self._lr_now)
        g = self._graphs.get(with_reg)
        if g is None:
            snap = self._snapshot()
            self._step_body(*self._g_in[:3], None, with_reg, self._g_in[3])
            rt.synchronize()
            self._restore(snap)
            rt.synchronize()
            g = torch.cuda.CUDAGraph()
            # No cyclic garbage collection inside the capture.  A trainer whose optimizer runs on its own stream is a reference cycle
            # (trainer -> bucketer -> on_bucket, a bound method of the trainer), so a dropped one - and the CUDAGraph objects it holds
            # - is freed whenever the collector runs.  torch's ~CUDAGraph synchronises the device on ROCm under a throwing check, a
            # synchronisation is not permitted on a capturing thread, and an exception out of a destructor ends the process
            # (SIGABRT, no message).  torch.cuda.graph no longer collects before a capture by itself
            # (torch.compiler.config.force_cudagraph_gc is off), so: collect here, outside, and hold the collector until the capture ends.
            gc.collect()
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._step_body(*self._g_in[:3], None, with_reg, self._g_in[3])
            finally:
                if gc_was_on:
                    gc.enable()
            # the capture pass advanced the host mirrors as a step does, but ran nothing: undo it on the host only
            eng.adam_t = snap["adam_t"]
            eng._shared["dropout_step"] = snap["dropout_step"]
            self._graphs[with_reg] = g
        g.replay()
        eng.adam_t += 1                          # host mirrors of the device counters
        eng._shared["dropout_step"] += (eng.n_dropout_draws if self.dropout else 0) + eng.n_noise_draws
        eng.t_dirty = True

    def compute_loss(self, y_true, y_pred, lr=None):
        """compute_loss(spec_out, spec_generated, model.model.losses) of main_training.py:203-235 for the prediction the model has
        just produced (`y_pred` must be the output of the last forward call of this trainer's model: NHWC from `model.model(...)`
        or NCHW from `model(...)`).  Returns a differentiable 0-dim tensor: data term / global batch + l2 terms / replicas."""
        eng = self.engine
        eng.use_device_counters(False)             # the module path passes its per-step scalars as launch arguments
        if y_pred.data_ptr() != eng.pred.data_ptr():
            raise ValueError("compute_loss needs the prediction of the model's last forward pass (its own output buffer)")
        tgt = y_true
        if tgt.dim() == 4 and tgt.shape[1] != 2 and tgt.shape[-1] == 2:
            tgt = tgt.permute(0, 3, 1, 2)
        tgt = tgt.to(eng.device, torch.float32).contiguous()
        self._lr_now = self.lr if lr is None else lr
        eng.loss_from_logits(tgt, eng.B * self.world_size, self.alpha)       # fused sigmoid + loss + dL/dlogits (seeds backward)
        self._total_on_device = True
        return _LossFunction.apply(self, self._anchor, eng.loss_total())

    def last_loss(self):
        """Scalar loss of the last step incl. the l2 term (host sync).  Per-replica share: SUM over replicas gives the
        value strategy.reduce(SUM, ...) returns (main_training.py:326)."""
        eng = self.engine
        if self._total_on_device:                # compute_loss() path: data + l2 terms were summed on the device
            return float(eng.loss_tot[0])
        return float(eng.loss_out[0]) + float(eng.reg_out[0])


class CheckpointManager:
    """tf.train.CheckpointManager(checkpoint, directory, max_to_keep=2) of main_training.py:171-172: numbered checkpoints
    holding the model variables (incl. the BatchNorm moving statistics) and the optimizer state, oldest ones deleted."""

    def __init__(self, trainer: "Trainer", directory, max_to_keep=2):
        self.trainer, self.directory, self.max_to_keep = trainer, directory, max_to_keep
        os.makedirs(directory, exist_ok=True)

    def _paths(self):
        out = []
        for f in os.listdir(self.directory):
            if f.startswith("ckpt-") and f.endswith(".pt"):
                try:
                    out.append((int(f[5:-3]), os.path.join(self.directory, f)))
                except ValueError:
                    pass
        return sorted(out)

    @property
    def latest_checkpoint(self):
        p = self._paths()
        return p[-1][1] if p else None

    def save(self, epoch=None):
        """manager.save() (main_training.py:364-365).  Rank 0 only writes in a multi-process job."""
        if dist.is_initialized() and dist.get_rank() != 0:
            return None
        eng = self.trainer.engine
        p = self._paths()
        n = (p[-1][0] + 1) if p else 1
        path = os.path.join(self.directory, f"ckpt-{n}.pt")
        state = {
            "format": 1, "epoch": epoch, "lr": self.trainer.lr, "adam_t": eng.adam_t,
            # the BASE seed of the Dropout streams: replica r draws from stream base + r (Trainer.__init__), and every rank restores
            # this one file (rank 0 writes it)
            "dropout_step": int(eng._shared["dropout_step"]),
            "dropout_seed": int((eng.dropout_seed - (self.trainer.rank if getattr(eng, "_seed_offset_by_rank", False) else 0)) & 0xFFFFFFFF),
            "optimizer": eng.optimizer, "m_schedule": float(eng._shared.get("m_schedule", 1.0)),
            "lamb": eng._shared["lamb"]["opt"].get_config() if eng.optimizer == "lamb" else None,
            "layout": [(k, tuple(s_.shape), int(s_.offset)) for k, s_ in eng.specs.items()],
            "theta": eng.theta.detach().cpu(), "adam_m": eng.adam_m.detach().cpu(), "adam_v": eng.adam_v.detach().cpu(),
            "moving": {k: v.detach().cpu() for k, v in eng.moving.items()},
        }
        tmp = path + ".tmp"
        torch.save(state, tmp)
        os.replace(tmp, path)
        for _, old in self._paths()[:-self.max_to_keep]:
            os.remove(old)
        return path

    def restore(self, path=None):
        """checkpoint.restore(manager.latest_checkpoint): variables, moving statistics and Adam slots / step count."""
        path = path or self.latest_checkpoint
        if path is None:
            return None
        eng = self.trainer.engine
        state = torch.load(path, map_location="cpu", weights_only=True)
        layout = [(k, tuple(s_.shape), int(s_.offset)) for k, s_ in eng.specs.items()]
        if [tuple(x) for x in state["layout"]] != layout:
            raise ValueError("checkpoint was written for a different model configuration")
        eng.theta.copy_(state["theta"]); eng.adam_m.copy_(state["adam_m"]); eng.adam_v.copy_(state["adam_v"])
        for k, v in state["moving"].items():
            eng.moving[k].copy_(v)
        eng.adam_t = int(state["adam_t"])
        if "dropout_step" in state:              # the Dropout stream continues where it stopped (older checkpoints: from draw 0)
            eng._shared["dropout_step"] = int(state["dropout_step"])
            # base seed + this replica's rank: the replicas keep independent masks after a resume (MirroredStrategy draws per replica)
            by_rank = self.trainer.world_size > 1
            eng.dropout_seed = (int(state["dropout_seed"]) + (self.trainer.rank if by_rank else 0)) & 0xFFFFFFFF
            eng._seed_offset_by_rank = by_rank
            self.trainer._graphs = {}            # the seed is a launch argument frozen into a captured step: capture again
        if "m_schedule" in state:
            eng._shared["m_schedule"] = float(state["m_schedule"])
        eng.t_dirty = True
        eng.sync_device_counters()
        return state.get("epoch")


class _Meter:
    """A mean `fit` reports: the fp64 sums over an epoch of what `source()` - a view of a device counter, no copy - holds after every
    batch, row 0 for the training and row 1 for the validation batches, and the rule that makes record entries of the summed rows.
    count: the sums are divided by steps x count (per step, replicas included); None: the counter's last entry counts the samples that
    entered the sums before it, which are divided by max(that, 1)."""

    def __init__(self, keys, source, count, device):
        self.keys, self.source, self.count = keys, source, count
        self.tot = torch.zeros((2, len(keys) + (count is None)), dtype=torch.float64, device=device)

    def add(self, row):
        self.tot[row] += self.source()

    def entries(self, tot, steps):
        """tot: the sums, reduced over the replicas, on the host; steps: {"train": batches seen} and, with a validation pass, "val" """
        out = {}
        for row, (prefix, n) in enumerate(steps.items()):
            den = max(float(tot[row, -1]), 1.0) if self.count is None else n * self.count
            out.update({f"{prefix}_{key}": float(tot[row, i]) / den for i, key in enumerate(self.keys)})
        return out


def fit(trainer: "Trainer", train_batches, n_epochs, val_batches=None, manager: CheckpointManager = None, lr0=None,
        lr_exp_decay=(True, 80), start_epoch=0, log=print, val_updates_moving=True):
    """The epoch loop of main_training.py:336-390: exponential rate from epoch 80, running means of the amplitude / phase
    loss terms, a checkpoint every second epoch.  `train_batches` / `val_batches` are callables returning an iterable of
    (spec_in, emb, spec_out) per-replica shards for the epoch.

    Reported values are the reference's: `train_loss` = mean over steps of the cross-replica SUM of the per-replica loss
    (data term / global batch + l2 terms / replicas: strategy.reduce(SUM, ...), main_training.py:323-327, :345-352);
    `*_amp` / `*_phase` = tf.keras.metrics.Mean over every (b, h, w) element of (a - a^)^2 and 1 - cos(...) across steps and
    replicas (main_training.py:239-244, :279-284).  The validation pass calls the model with training=True as the reference's
    test_step does (main_training.py:297-300): batch statistics, dropout active - and, as in Keras, the BatchNorm moving
    statistics move during it (`val_updates_moving=False` keeps them at their post-training values instead).

    Further means are summed on the device as fp64 and read back once per epoch, behind the validation pass where there is one
    (`_Meter`); the keys of a validation pass are absent without one.  An engine with a counter of ENGINE_METRICS adds its metric,
    the raw sum over steps x elements per step x replicas: `train_kl` / `val_kl` (VAE: kl_loss_object over every (b, l) element),
    `train_vq` / `val_vq` (VQ-VAE: (q - x)^2 over every element) or `train_acc` / `val_acc` (cnn_clas.DeepCNNEngine, a classifier whose
    batches are (x, None, one-hot target): correct rows over rows seen, History.train_acc_history of the legacy trainer.py:230; for such
    an engine `train_amp` / `val_amp` carry the mean cross-entropy per row and `train_phase` / `val_phase` are 0).

    With a term on the waveform (`trainer.wave_loss`, `decay_loss`, `spectral_loss`) a batch is (spec_in, emb, spec_out, wav_true) or
    DataGenerator(characteristics=True)'s (spec_in, emb, spec_out, (room, wav_true)); `train_loss` / `val_loss` carry the terms, and the
    validation pass runs the trainer's chain for the losses alone, without gradients.  The record gains, per term the user gave:
    `train_wave` / `val_wave`, the sum of E_b / D_b over steps x batch size x replicas; `train_decay` / `val_decay`, the sum of Q_b (dB^2)
    over max(samples counted, 1) - a sample with a silent target is not counted; `train_sc` / `val_sc` and `train_logmag` /
    `val_logmag`, the sums of mean_r SC and mean_r LM over max(samples counted, 1)."""
    eng = trainer.engine
    world = trainer.world_size

    def unpack(batch):
        """(spec_in, emb, spec_out, wav_true or None)"""
        if trainer._wave is None:
            spec_in, emb, spec_out = batch
            return spec_in, emb, spec_out, None
        if len(batch) != 4:
            raise ValueError(f"a trainer with a {trainer._wave_option} takes batches (spec_in, emb, spec_out, wav_true) or (..., (room, wav_true))")
        spec_in, emb, spec_out, extra = batch
        return spec_in, emb, spec_out, extra[1] if isinstance(extra, (tuple, list)) else extra
    lr0 = trainer.lr if lr0 is None else lr0
    has_acc = hasattr(eng, "acc_out")          # a classifier: loss_out[1] is the raw cross-entropy sum over the rows
    per_elem = 1.0 / ((1 if has_acc else eng.H * eng.W) * eng.B * world)       # loss_out[1:3] are raw per-replica sums of the two terms
    history = []

    def reduce_(t):
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=trainer.group)
        return t.cpu()

    # the sources are looked up at every batch: a loss object allocates its result vector at its first call
    meters = [_Meter((key,), lambda a=attr, i=i: getattr(eng, a)[i:i + 1], (eng.B if count is None else getattr(eng, count)) * world, eng.device)
              for key, attr, i, count in ENGINE_METRICS if hasattr(eng, attr)]
    if trainer.wave_loss is not None:
        meters.append(_Meter(("wave",), lambda: trainer.wave_loss.wave_out[0:1], eng.B * world, eng.device))
    if trainer.decay_loss is not None:
        meters.append(_Meter(("decay",), lambda: trainer.decay_loss.decay_out, None, eng.device))
    if trainer.spectral_loss is not None:
        meters.append(_Meter(("sc", "logmag"), lambda: trainer.spectral_loss.spectral_out, None, eng.device))

    for epoch in range(start_epoch, n_epochs):
        lr = lr_schedule(lr0, epoch, lr_exp_decay)
        tot = torch.zeros(4, dtype=torch.float64, device=eng.device)      # data loss, amplitude sum, phase sum, l2 terms
        nb = 0
        for mt in meters:
            mt.tot.zero_()
        eng.reg_loss()
        reg0 = eng.reg_out[0].double()           # l2 terms on the weights the first step of the epoch sees
        for batch in train_batches(epoch):
            spec_in, emb, spec_out, wav_true = unpack(batch)
            trainer.step(spec_in, emb, spec_out, lr=lr, wav_true=wav_true)
            tot[:3] += eng.loss_out[:3].double()     # total data loss, amplitude term, phase term of this step (raw sums ~1e5: fp64)
            for mt in meters:
                mt.add(0)
            nb += 1
        # the l2 terms drift over an epoch (Adam moves every weight by ~lr per step whatever the gradient's scale): the reported
        # mean takes the trapezoid of their value before the first and after the last step instead of nine reductions per step
        eng.reg_loss()
        tot[3] = 0.5 * (reg0 + eng.reg_out[0].double()) * max(nb, 1)
        tot = reduce_(tot)
        n = max(nb, 1)
        rec = {"epoch": epoch + 1, "lr": lr, "train_loss": float(tot[0] + tot[3]) / n,
               "train_amp": float(tot[1]) * per_elem / n, "train_phase": float(tot[2]) * per_elem / n}
        steps = {"train": n}
        if val_batches is not None:
            vt = torch.zeros(3, dtype=torch.float64, device=eng.device)
            vb = 0
            saved_moving = None if val_updates_moving else {k: v.clone() for k, v in eng.moving.items()}
            for batch in val_batches(epoch):
                spec_in, emb, spec_out, wav_true = unpack(batch)
                eng.training = True
                eng.begin_step(lr, n_draws=(eng.n_dropout_draws if trainer.dropout else 0) + eng.n_noise_draws, forward_only=True)     # device counters only
                mask = eng.make_dropout_mask() if trainer.dropout else None
                eng.forward(spec_in, emb, dropout_mask=mask, target=spec_out, global_batch=eng.B * world, alpha=trainer.alpha)
                if trainer._wave is not None:
                    trainer._waveform_terms(spec_in, spec_out, wav_true, backward=False)
                vt += eng.loss_out[:3].double()
                for mt in meters:
                    mt.add(1)
                vb += 1
            if saved_moving is not None:
                for k, v in saved_moving.items():
                    eng.moving[k].copy_(v)
            vt = reduce_(vt)
            m = steps["val"] = max(vb, 1)
            rec.update(val_loss=float(vt[0]) / m, val_amp=float(vt[1]) * per_elem / m, val_phase=float(vt[2]) * per_elem / m)
        for mt in meters:          # one reduction and one read-back each, the same on every rank
            rec.update(mt.entries(reduce_(mt.tot), steps))
        if manager is not None and epoch % 2 == 0:
            rec["checkpoint"] = manager.save(epoch=epoch)
        history.append(rec)
        if log is not None:
            log(rec)
    return history

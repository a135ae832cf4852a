"""Scoring of generated impulse responses on the device, per room: the capability behind the reference's evaluation script.

`rir_generation.py` walks the test partition, generates (`trained_model.model([spec_in, emb], training=False)`, :165),
reconstructs each waveform (`PostProcess.post_process`, :173-178), computes seven figures per sample (:185-225: spectrogram
MSE, magnitude MSE, `1 - cos` phase error, magnitude misalignment in dB, waveform MSE, waveform MSE over the first 50 ms,
waveform misalignment in dB), keeps them in lists per room type (:227-290), averages (:311-357) and writes three report files
(:363-532).  Here one kernel scores a whole batch (`ops.eval_metrics`), a second folds the batch into running sums per room
that live on the device (`ops.eval_accumulate`), and `Evaluator.result()` is the only place that reads anything back:

    ev = Evaluator(model, diff_gen=False)
    for spec_in, emb, spec_out, wav_true, room in test_batches:
        ev.update(spec_in, emb, spec_out, wav_true, room)        # generate -> reconstruct -> score -> accumulate, no host sync
    write_report(ev.result(), folder, name)

Spectrograms are accepted NHWC `[B, H, W, 2]` as the reference's generator yields them or NCHW `[B, 2, H, W]` as the engine
produces them (the rule of `PostProcess.post_process`); waveforms are fp32 `[B, T]`.  There is no CPU path: tensors live on
the GPU or the calls raise `ValueError`.  `algorithm` selects the reconstruction that is scored, as the reference's argument of
that name does (rir_generation.py:62, :137): 'ph' from the predicted phase (`features.PostProcess`), 'gl' by Griffin-Lim from
the predicted magnitude alone (`features.GriffinLim`).

Opt-in, `Evaluator(acoustics=True)` adds what a listener asks of a generated response: does the direct sound arrive on time, is the
direct / reverberant and the early / late balance right, does the energy decay at the room's rate.  `ops.acoustic_figures` takes
the figures of `ACOUSTIC_FIGURES` from the predicted and the true waveform in one launch, `ops.acoustic_accumulate` folds the
errors of `ACOUSTIC_ERRORS` per room next to the other running sums; `result()` gains the key "acoustics" and `write_report` a
fourth file.  The waveforms are the reference's 0.2 s window: where a room's decay outlasts it, `c50`, `ts` and `edt` are figures
of the truncated response - like for like between prediction and truth, not ISO 3382 values (which is also why there is no
T20 / T30).
"""
import csv
import os
import time

import numpy as np
import torch

from . import ops
from .features import HOP_LENGTH, N_FFT, STFT_SHAPE, WIN_LENGTH, GriffinLim, PostProcess
from .rooms import UTS_ROOMS

ROOMS = ("HemiAnechoicRoom", "LargeMeetingRoom", "MediumMeetingRoom", "ShoeBoxRoom", "SmallMeetingRoom")
METRICS = ("mse_spec", "mse_amp", "phase", "mis_amp", "mse_wav", "mse_wav50", "mis_wav")
# a row of `acoustics`: the peak index, four energy sums and the length of the 0 .. -10 dB stretch (the "raw" columns), then
# direct-to-reverberant ratio and clarity in dB, centre time in ms, early decay time in s
ACOUSTIC_FIGURES = ("n0", "e_tot", "e_dir", "e_early", "m1", "n_fit", "drr", "c50", "ts", "edt")
# errors of a (pred, true) pair: time of arrival in ms, drr and c50 in dB, centre time in ms, early decay time in percent of the truth
ACOUSTIC_ERRORS = ("toa_ms", "drr_db", "c50_db", "ts_ms", "edt_pct")

# (pinned by tests/test_evaluate.py; `acoustics` and its two name tuples are imported by name)
__all__ = ["ROOMS", "METRICS", "score", "Evaluator", "write_report"]


def _nchw(x, what, nhwc=None):
    """A [B, 2, H, W] view of a device spectrogram batch handed over in either layout (no copy)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor (there is no CPU path)")
    if x.dim() != 4:
        raise ValueError(f"{what} must be [B, H, W, 2] or [B, 2, H, W]")
    if nhwc is None:
        nhwc = x.shape[-1] == 2 and x.shape[1] != 2
    x = x.permute(0, 3, 1, 2) if nhwc else x
    if x.shape[1] != 2:
        raise ValueError(f"{what} must have two planes (magnitude, phase)")
    return x


def _wav(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor (there is no CPU path)")
    if x.dim() != 2:
        raise ValueError(f"{what} must be [B, T]")
    return x


def _dense(x):
    return x if x.dtype == torch.float32 and x.is_contiguous() else x.contiguous().float()


def score(pred, target, wav_pred=None, wav_true=None, phase_ref=None, n50=2400, nhwc=None):
    """The seven figures of rir_generation.py:185-225 for every sample of a batch -> fp64 [B, 7] on the device, columns in the
    order of `METRICS`.  `phase_ref` is the network input under `diff_gen` (:190-193); without the waveform pair columns 4-6
    are NaN.  Nothing is read back."""
    p = _dense(_nchw(pred, "pred", nhwc))
    t = _dense(_nchw(target, "target", nhwc))
    r = None if phase_ref is None else _dense(_nchw(phase_ref, "phase_ref", nhwc))
    if (wav_pred is None) != (wav_true is None):
        raise ValueError("wav_pred and wav_true come as a pair")
    wp = None if wav_pred is None else _dense(_wav(wav_pred, "wav_pred"))
    wt = None if wav_true is None else _dense(_wav(wav_true, "wav_true"))
    out = torch.empty((p.shape[0], 7), dtype=torch.float64, device=p.device)
    ops.eval_metrics(p, t, out, wp, wt, r, n50)
    return out


def acoustics(wav_pred, wav_true=None, n_pre=120, n_dir=120, n_early=2400, fs=48000):
    """The room-acoustic figures of every waveform of a batch -> fp64 [B, 2, 10] on the device (pred, true), or [B, 1, 10] without
    `wav_true`; columns in the order of `ACOUSTIC_FIGURES`.  With e = h*h in fp64: n0 = argmax |h| (the direct sound), s = max(0, n0 -
    n_pre), S[n] = sum_{k >= n} e[k] (the Schroeder backward integral), E_tot = S[s], E_dir over s .. n0 + n_dir, E_early over s ..
    s + n_early - 1, M1 = sum (n - s) e[n], N_fit = #{n >= s: 10 S[n] >= E_tot}; drr = 10 log10(E_dir / (E_tot - E_dir)), c50 the same
    of E_early, ts = M1 / E_tot / fs in ms, edt = -60 / (slope of the least-squares line through 10 log10(S[s+k] / E_tot), k <
    N_fit, in dB/s).  The defaults are 2.5 ms, 2.5 ms and 50 ms at 48 kHz.  Degenerate rows follow IEEE arithmetic (an all-zero
    row gives NaN, no late energy +inf dB).  Nothing is read back."""
    wp = _dense(_wav(wav_pred, "wav_pred"))
    wt = None if wav_true is None else _dense(_wav(wav_true, "wav_true"))
    fig = torch.empty((wp.shape[0], 1 if wt is None else 2, len(ACOUSTIC_FIGURES)), dtype=torch.float64, device=wp.device)
    ops.acoustic_figures(wp, wt, fig, n_pre, n_dir, n_early, fs)
    return fig


class Evaluator:
    """The loop body of rir_generation.py:160-293 for whole batches, with the per-room lists (:143-153) replaced by running
    sums on the device.

    `model`: anything with the reference's call shape, `model.model([spec_in, emb], training=False)` (`UNet`, `ResAE`,
    `Autoencoder` of this package).  `diff_gen` (:173-176, :190-193): the phase that is scored and reconstructed is
    `pred[..., 1] + spec_in[..., 1]` while `mse_spec` keeps the raw prediction.  `room` of a batch is a sequence of names out
    of `rooms` or an integer tensor of indices into it, on the device; anything else counts in the global figures only.
    `algorithm` 'gl' (:176-178 with algorithm='gl'): the waveform comes from `GriffinLim(gl_iters, gl_momentum, seed=gl_seed,
    method=gl_method)` on the predicted magnitude ("fft": the fp32 form, the one meant for evaluation runs); the phase plane - and
    `diff_gen`'s sum - still feed the phase figure but not the waveform.
    `acoustics=True` adds the room-acoustic errors of `ACOUSTIC_ERRORS` (windows `n_pre`, `n_dir`, `n_early` in samples at `fs`, see
    `acoustics`) of every batch that comes with its waveform pair: two more launches behind the accumulation, inside the scoring
    stage's time, and their running sums share the one read-back.

    Between construction and `result()` nothing waits for the device.  The running sums, the [B, 7] figures, the waveform
    buffer and the layout staging buffers are allocated for the first batch and reused while the batch size holds.  Stage
    times come from HIP events recorded on the stream and are read in `result()`."""

    def __init__(self, model, diff_gen=False, rooms=ROOMS, n50=2400, des_shape=STFT_SHAPE, n_fft=N_FFT, win_length=WIN_LENGTH,
                 hop_length=HOP_LENGTH, algorithm="ph", gl_iters=32, gl_momentum=0.99, gl_seed=0, gl_method="dft", acoustics=False,
                 n_pre=120, n_dir=120, n_early=2400, fs=48000):
        self.model, self.diff_gen, self.rooms, self.n50 = model, bool(diff_gen), tuple(rooms), int(n50)
        if not self.rooms:
            raise ValueError("at least one room")
        if algorithm not in ("ph", "gl"):
            raise ValueError("algorithm must be 'ph' or 'gl'")
        if gl_method not in ("dft", "fft"):
            raise ValueError(f'gl_method must be "dft" or "fft", not {gl_method!r}')
        self.algorithm = algorithm
        self.des_shape, self.n_fft, self.win_length, self.hop_length = tuple(des_shape), n_fft, win_length, hop_length
        self._index = {r: i for i, r in enumerate(self.rooms)}
        self._post = (PostProcess(algorithm="ph") if algorithm == "ph" else
                      GriffinLim(gl_iters, gl_momentum, seed=gl_seed, method=gl_method))
        self.acoustics, self.n_pre, self.n_dir, self.n_early, self.fs = bool(acoustics), int(n_pre), int(n_dir), int(n_early), float(fs)
        if min(self.n_pre, self.n_dir, self.n_early) < 0 or not self.fs > 0:
            raise ValueError("n_pre, n_dir and n_early are sample counts >= 0 and fs is positive")
        self._acc = None
        self._sums = None           # with acoustics: the running sums of both kinds in one buffer, so that one copy reads them back
        self._aacc = None
        self._buf = {}              # name -> kept device buffer
        self._pinned = []           # [pinned int32 buffer, event of the last copy out of it]
        self._events = []           # per batch: (B, start, after inference, after reconstruction, after scoring); None = not run
        self._t0 = None

    # ---- kept buffers ---------------------------------------------------------------------------
    def _kept(self, name, shape, dtype, device):
        b = self._buf.get(name)
        if b is None or tuple(b.shape) != tuple(shape) or b.device != device:
            b = torch.empty(tuple(shape), dtype=dtype, device=device)
            self._buf[name] = b
        return b

    def _stage(self, name, x):
        """x as a contiguous fp32 tensor: itself when it already is one, else a copy in a kept buffer."""
        if x.dtype == torch.float32 and x.is_contiguous():
            return x
        b = self._kept(name, x.shape, torch.float32, x.device)
        b.copy_(x)
        return b

    def _group(self, room, B, device):
        g = self._kept("group", (B,), torch.int32, device)
        if isinstance(room, torch.Tensor):
            if not room.is_cuda or room.dim() != 1 or room.shape[0] != B or room.dtype.is_floating_point:
                raise ValueError(f"room must be {B} names or an integer CUDA tensor [{B}]")
            g.copy_(room)
            return g
        room = list(room)
        if len(room) != B:
            raise ValueError(f"room must be {B} names or an integer CUDA tensor [{B}]")
        # names: indices go through a pinned buffer that is reused only once the copy out of it has finished (checked, never
        # waited for: a busy buffer means another one is taken)
        slot = next((s for s in self._pinned if s[0].shape[0] == B and s[1].query()), None)
        if slot is None:
            slot = [torch.empty((B,), dtype=torch.int32).pin_memory(), torch.cuda.Event()]
            self._pinned.append(slot)
        slot[0].copy_(torch.tensor([self._index.get(r, -1) for r in room], dtype=torch.int32))
        g.copy_(slot[0], non_blocking=True)
        slot[1].record()
        return g

    # ---- one batch --------------------------------------------------------------------------------
    def update(self, spec_in, emb, spec_out, wav_true, room):
        """One test batch: generate (:165), reconstruct (:173-178), score (:185-225), accumulate (:199-290)."""
        x = _nchw(spec_in, "spec_in")
        y = _nchw(spec_out, "spec_out")
        wt = _wav(wav_true, "wav_true")
        B = x.shape[0]
        T = self.hop_length * (self.des_shape[1] - 1)
        if tuple(wt.shape) != (B, T):
            raise ValueError(f"wav_true must be [{B}, {T}], the length the reconstruction produces")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        with torch.no_grad():
            pred = _nchw(self.model.model([x.permute(0, 2, 3, 1), emb], training=False), "prediction", nhwc=True)
        ev[1].record()
        feat = self._stage("pred", pred)
        if self.diff_gen and self.algorithm == "ph":    # :174-175: magnitude as predicted, phase = predicted + input phase (fp32, as
                                                        # there); Griffin-Lim reads the magnitude alone
            xs = self._stage("spec_in", x)
            s = self._kept("diff", feat.shape, torch.float32, feat.device)
            s[:, 0].copy_(feat[:, 0])
            torch.add(feat[:, 1], xs[:, 1], out=s[:, 1])
            feat = s
        wav_pred = self._post.post_process(feat, des_shape=self.des_shape, n_fft=self.n_fft, win_length=self.win_length,
                                           hop_length=self.hop_length, nhwc=False,
                                           out=self._kept("wav", (B, T), torch.float32, x.device))
        ev[2].record()
        self._score(pred, x, y, wav_pred, wt, room, ev)

    def update_scored(self, pred, spec_in, spec_out, wav_pred, wav_true, room):
        """Score and accumulate from tensors the caller holds (`pred` the raw network output; `wav_pred` its reconstruction,
        under `diff_gen` that of the summed phase).  The waveform pair may be None: the three waveform figures are then NaN."""
        if (wav_pred is None) != (wav_true is None):
            raise ValueError("wav_pred and wav_true come as a pair")
        args = (_nchw(pred, "pred"), _nchw(spec_in, "spec_in") if self.diff_gen else None, _nchw(spec_out, "spec_out"),
                None if wav_pred is None else _wav(wav_pred, "wav_pred"), None if wav_true is None else _wav(wav_true, "wav_true"))
        ev = [None, None, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]
        ev[2].record()
        self._score(*args, room, ev)

    def _score(self, pred, x, spec_out, wav_pred, wav_true, room, ev):
        if self._t0 is None:
            self._t0 = time.perf_counter()
        B, dev = pred.shape[0], pred.device
        p = self._stage("pred", pred)
        t = self._stage("spec_out", spec_out)
        r = self._stage("spec_in", x) if self.diff_gen else None
        wp = None if wav_pred is None else self._stage("wav_pred", wav_pred)
        wt = None if wav_true is None else self._stage("wav_true", wav_true)
        g = self._group(room, B, dev)
        out = self._kept("out", (B, 7), torch.float64, dev)
        if self._acc is None:
            if self.acoustics:
                rows = len(self.rooms) + 1
                self._sums = torch.zeros((rows * (8 + 4 * len(ACOUSTIC_ERRORS)),), dtype=torch.float64, device=dev)
                self._acc = self._sums[:rows * 8].view(rows, 8)
                self._aacc = self._sums[rows * 8:].view(rows, 4 * len(ACOUSTIC_ERRORS))
            else:
                self._acc = torch.zeros((len(self.rooms) + 1, 8), dtype=torch.float64, device=dev)
        ops.eval_metrics(p, t, out, wp, wt, r, self.n50)
        ops.eval_accumulate(out, g, self._acc)
        if self.acoustics and wp is not None:
            fig = self._kept("fig", (B, 2, len(ACOUSTIC_FIGURES)), torch.float64, dev)
            ops.acoustic_figures(wp, wt, fig, self.n_pre, self.n_dir, self.n_early, self.fs)
            ops.acoustic_accumulate(fig, g, self._aacc, self.fs)
        ev[3].record()
        self._events.append((B, ev))

    # ---- the read-back ----------------------------------------------------------------------------
    def result(self):
        """{"rooms": names, "n": [global, room0, ...], <metric>: [global, room0, ...] for each of `METRICS`, "timing": {...}}.
        Means are Python floats; a room without samples gives NaN, as np.mean([]) does in the reference (:319-357).  Stage times
        are seconds: inference per batch, reconstruction and scoring per sample (the reference's units, :164-181, :292-293),
        each averaged without the first batch (:359-361); NaN for a stage that never ran or ran once.  With `acoustics=True` also
        "acoustics": {<error>: {"err": [...], "pred": [...], "true": [...], "n": [...]} for each of `ACOUSTIC_ERRORS`}, each list
        [global, room0, ...]: the mean error, the mean predicted and true value of the figure, and the number of pairs in which the
        figure counted (both sides finite; edt: and positive) - NaN means where that is 0."""
        G = len(self.rooms)
        aacc = np.zeros((G + 1, 4 * len(ACOUSTIC_ERRORS)))
        if self._acc is None:
            acc = np.zeros((G + 1, 8))
        elif self._sums is not None:
            sums = self._sums.cpu().numpy()                    # the one synchronising copy
            acc, aacc = sums[:(G + 1) * 8].reshape(G + 1, 8), sums[(G + 1) * 8:].reshape(G + 1, -1)
        else:
            acc = self._acc.cpu().numpy()                      # the one synchronising copy
        total = time.perf_counter() - self._t0 if self._t0 is not None else 0.0
        n = acc[:, 7]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = acc[:, :7] / n[:, None]
        res = {"rooms": list(self.rooms), "n": [int(v) for v in n]}
        for k, name in enumerate(METRICS):
            res[name] = [float(v) for v in mean[:, k]]
        if self.acoustics:
            res["acoustics"] = {}
            for k, name in enumerate(ACOUSTIC_ERRORS):
                cnt = aacc[:, 4 * k + 3]
                with np.errstate(invalid="ignore", divide="ignore"):
                    m = aacc[:, 4 * k:4 * k + 3] / cnt[:, None]
                res["acoustics"][name] = {"err": [float(v) for v in m[:, 0]], "pred": [float(v) for v in m[:, 1]],
                                          "true": [float(v) for v in m[:, 2]], "n": [int(v) for v in cnt]}

        def stage(i, per_sample):
            v = [e[i].elapsed_time(e[i + 1]) * 1e-3 / (B if per_sample else 1)
                 for B, e in self._events[1:] if e[i] is not None and e[i + 1] is not None]
            return float(np.mean(v)) if v else float("nan")

        res["timing"] = {"n_batches": len(self._events), "batch_size": self._events[-1][0] if self._events else 0,
                         "inference_s": stage(0, False), "postprocess_s": stage(1, True), "loss_s": stage(2, True),
                         "total_s": float(total)}
        return res


# ---- report files (rir_generation.py:363-532) -----------------------------------------------------

_LABELS = {"HemiAnechoicRoom": "HemiAnechoic", "LargeMeetingRoom": "Large", "MediumMeetingRoom": "Medium", "ShoeBoxRoom": "Shoe",
           "SmallMeetingRoom": "Small"}
_COLUMNS = (("mse_spec", "MSE spectrogram"), ("mse_amp", "MSE magnitude"), ("phase", "1-cos(y-y_) phase"),
            ("mse_wav", "MSE waveform"), ("mse_wav50", "MSE waveform 50ms"), ("mis_amp", "Misalignment magnitude"),
            ("mis_wav", "Misalignment waveform"))
_POSITIONAL = ("mse_spec", "mse_amp", "phase")


def _fmt(metric, v):
    if metric in _POSITIONAL:
        return np.format_float_positional(v, precision=4)
    return np.format_float_scientific(v, precision=4)


def _sec(v):
    return np.format_float_positional(v, precision=5)


def write_report(result, folder, name):
    """`{name}_losses.csv`, `{name}_infer_time.csv` and `{name}_results_inference.txt` in `folder`, from `Evaluator.result()`:
    the column headers, row labels and number formats of the reference's files (:363-425).  Needs no device.  A result with the key
    "acoustics" also gives `{name}_acoustics.csv`: one row per (room, figure of `ACOUSTIC_ERRORS`) with the mean error, the mean
    predicted and true value, the count and - for the rooms `rooms.UTS_ROOMS` knows - the room's RT60 in ms, the decay the figures
    of that room are to be read against; numbers in full precision (`repr`)."""
    os.makedirs(folder, exist_ok=True)
    labels = ["Global"] + [_LABELS.get(r, r) for r in result["rooms"]]
    n = result["n"]
    tm = result.get("timing", {})
    nan = float("nan")
    times = [tm.get(k, nan) for k in ("inference_s", "postprocess_s", "loss_s", "total_s")]
    batch = tm.get("batch_size", 0)
    paths = [os.path.join(folder, f"{name}_{s}") for s in ("losses.csv", "infer_time.csv", "results_inference.txt")]

    with open(paths[0], "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["room", "n samples"] + [title for _, title in _COLUMNS])
        for i, label in enumerate(labels):
            w.writerow([label, n[i]] + [_fmt(m, result[m][i]) for m, _ in _COLUMNS])

    with open(paths[1], "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["n_samples", "t_model_inference_avg", "batch_size", "t_postprocess", "t_loss_calc", "t_global"])
        w.writerow([n[0], _sec(times[0]), batch, _sec(times[1]), _sec(times[2]), _sec(times[3])])

    with open(paths[2], "w") as f:
        f.write(f"{name} results:\n\n")
        f.write(f"Took {_sec(times[0])} s on average to infer spectrograms with batch size of {batch}\n")
        f.write(f"Took {_sec(times[1])} s on average to postprocess and generate each spectrogram and waveform\n")
        f.write(f"Took {_sec(times[2])} s on average to obtain the losses for each waveform\n")
        f.write(f"Took {_sec(times[3])} s to generate, postprocess and obtain loss for {n[0]} samples\n\n")
        for i in range(len(labels)):
            v = {m: _fmt(m, result[m][i]) for m in METRICS}
            f.write("Total losses:\n" if i == 0 else f"{result['rooms'][i - 1]} losses ({n[i]} samples):\n")
            f.write(f"Total loss: {v['mse_spec']} (MSE whole spectrogram)\t|\tAmplitude loss: {v['mse_amp']} (MSE amplitude)"
                    f"\t|\tPhase loss: {v['phase']} (1-cos(y_true - y_pred))\n")
            f.write(f"Waveform loss: {v['mse_wav']} (MSE)\t|\t 50 ms waveform loss: {v['mse_wav50']} (MSE)\n")
            f.write(f"Misalignment loss (amplitude): {v['mis_amp']} (dB)\t|\t Misalignment loss (wav): {v['mis_wav']} (dB)\n")
            if i + 1 < len(labels):
                f.write("\n")

    if "acoustics" in result:
        paths.append(os.path.join(folder, f"{name}_acoustics.csv"))
        rt60 = [""] + [UTS_ROOMS[r][-1] if r in UTS_ROOMS else "" for r in result["rooms"]]
        with open(paths[3], "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(["room", "figure", "mean error", "mean pred", "mean true", "n samples", "rt60 ms"])
            for i, label in enumerate(labels):
                for fig, v in result["acoustics"].items():
                    w.writerow([label, fig, repr(float(v["err"][i])), repr(float(v["pred"][i])), repr(float(v["true"][i])), v["n"][i],
                                rt60[i]])
    return paths

"""Waveform <-> feature transforms on the device: the host-side mirror of the reference's pre- and post-processing classes.

The reference builds its network inputs on the host, one file at a time (`Dataset.load_data`, dataset.py:146-176:
`Loader.load` -> `FeatureExtractor.extract` -> `Normalizer.normalize` -> `TensorPadder.pad_amp_phase`, preprocess.py) and
turns predictions back into impulse responses the same way (`PostProcess.post_process`, postprocess.py:51-73).  Here both
directions are one HIP kernel each over a whole batch that is already in HBM (csrc/features.hip), behind classes that keep
the reference's names, constructor arguments and call shapes:

    FeatureExtractor(n_fft, win_length, hop_length).extract(waveform)   -> (amp, phase)          preprocess.py:7-18
    Normalizer().normalize / .denormalize                                                        preprocess.py:21-41
    TensorPadder(desired_shape)                                                                  preprocess.py:60-113
    PreProcess(...)(waveforms)  = mean removal + extract + normalize + pad, fused               dataset.py:146-176
    PostProcess().post_process(feature, ...) -> waveform (un_pad + denormalize + istft, fused)   postprocess.py:51-73 'ph'
    GriffinLim().post_process(feature, ...)  -> waveform (un_pad + denormalize + griffinlim)     postprocess.py:47-50, :130-131 'gl'

Layouts: waveforms fp32 `[B, T]` (or `[T]`), features fp32 NCHW `[B, 2, H, W]` (plane 0 amplitude, plane 1 phase; row =
frequency bin, column = frame) - the engine's boundary, so a `PreProcess` output feeds `Trainer.step` / `UNet.forward`
directly; `PostProcess.post_process` and `GriffinLim.post_process` also accept the reference's NHWC `[H, W, 2]` /
`[B, H, W, 2]` features.  The Griffin-Lim branch (`algorithm='gl'`) is the whole iteration for a batch in one library call
(csrc/griffinlim.hip).  File decoding and writing (`librosa.load`, `scipy.io.wavfile.write`, `np.save`) stay on the host side
of the boundary and are not reimplemented.  There is no CPU path: tensors must live on the GPU and the calls raise otherwise.
"""
import torch

from . import ops

N_FFT, WIN_LENGTH, HOP_LENGTH = 256, 128, 64        # dataset.py:62-64
SAMPLE_RATE, DURATION = 48000, 0.2                  # dataset.py:66-67
INPUT_SHAPE = (144, 160)                            # dataset.py:70
STFT_SHAPE = (129, 151)                             # postprocess.py:51 des_shape


def _wav2d(waveform):
    if not isinstance(waveform, torch.Tensor) or not waveform.is_cuda:
        raise ValueError("waveforms must be CUDA tensors (there is no CPU path)")
    w = waveform if waveform.dim() == 2 else waveform.unsqueeze(0)
    if w.dim() != 2:
        raise ValueError("waveform must be [T] or [B, T]")
    return w.contiguous().float(), waveform.dim() == 1


class FeatureExtractor:
    """preprocess.py:7-18.  extract(waveform [T] or [B, T]) -> (amp, phase), each [n_fft/2+1, frames] or [B, ...]."""

    def __init__(self, n_fft, win_length, hop_length, pad_mode="reflect"):
        self.n_fft, self.win_length, self.hop_length, self.pad_mode = n_fft, win_length, hop_length, pad_mode

    def extract(self, waveform):
        w, single = _wav2d(waveform)
        B, T = w.shape
        out = torch.empty((B, 2, self.n_fft // 2 + 1, ops.stft_frames(T, self.hop_length)), dtype=torch.float32, device=w.device)
        ops.stft_features(w, out, self.n_fft, self.win_length, self.hop_length, self.pad_mode, remove_mean=False, normalize=False)
        return (out[0, 0], out[0, 1]) if single else (out[:, 0], out[:, 1])


class Normalizer:
    """preprocess.py:21-41 as constants + elementwise forms; the fused kernels apply them in fp64 (`PreProcess`, `PostProcess`).
    These two methods exist for callers that hold raw (amp, phase) tensors; they are plain tensor expressions."""

    def __init__(self):
        self.md = 100
        self.ep = 10 ** (-1 * self.md / 20)

    def normalize(self, amp, phase):
        return (20 * torch.log10(amp / 128 + self.ep) + self.md) / self.md, (phase + torch.pi) / (2 * torch.pi)

    def denormalize(self, amp_norm, phase_norm):
        amp = (10 ** ((amp_norm * self.md - self.md) / 20) - self.ep) * 128
        phase = torch.remainder(phase_norm * 2 * torch.pi, 2 * torch.pi) - torch.pi
        return amp, phase


class TensorPadder:
    """preprocess.py:60-113 on [..., rows, cols] tensors."""

    def __init__(self, desired_shape):
        self.desired_shape = tuple(desired_shape)

    def transform(self, tensor):
        r, c = tensor.shape[-2:]
        if r > self.desired_shape[0] or c > self.desired_shape[1]:        # get_needed_transform: larger inputs pass through
            return tensor
        return torch.nn.functional.pad(tensor, (0, self.desired_shape[1] - c, 0, self.desired_shape[0] - r))

    def pad_amp_phase(self, amp, phase):
        return self.transform(amp), self.transform(phase)

    @staticmethod
    def un_pad(amp, phase, desired_shape):
        return amp[..., :desired_shape[0], :desired_shape[1]], phase[..., :desired_shape[0], :desired_shape[1]]


class PreProcess:
    """The per-file chain of Dataset.load_data (dataset.py:146-176) for a batch of decoded waveforms, as one kernel:
    `signal -= mean` (preprocess.py:56) -> extract -> normalize -> pad -> features fp32 [B, 2, H, W]."""

    def __init__(self, n_fft=N_FFT, win_length=WIN_LENGTH, hop_length=HOP_LENGTH, desired_shape=INPUT_SHAPE, pad_mode="reflect",
                 remove_mean=True):
        self.n_fft, self.win_length, self.hop_length = n_fft, win_length, hop_length
        self.desired_shape, self.pad_mode, self.remove_mean = tuple(desired_shape), pad_mode, remove_mean

    def __call__(self, waveforms, out=None):
        w, _ = _wav2d(waveforms)
        if out is None:
            out = torch.empty((w.shape[0], 2) + self.desired_shape, dtype=torch.float32, device=w.device)
        ops.stft_features(w, out, self.n_fft, self.win_length, self.hop_length, self.pad_mode, self.remove_mean, normalize=True)
        return out


def _feature_nchw(feature, nhwc):
    """The layout rules of PostProcess.post_process: [H, W, 2], [B, H, W, 2] or [B, 2, H, W] -> (contiguous fp32 [B, 2, H, W],
    whether a single feature came in)."""
    if not isinstance(feature, torch.Tensor) or not feature.is_cuda:
        raise ValueError("features must be CUDA tensors (there is no CPU path)")
    f = feature
    single = f.dim() == 3
    if single:
        f = f.unsqueeze(0)
    if nhwc is None:                               # the reference hands over [H, W, 2]; the engine produces [B, 2, H, W]
        nhwc = f.shape[-1] == 2 and f.shape[1] != 2
    if nhwc:
        f = f.permute(0, 3, 1, 2)
    return f.contiguous().float(), single


class PostProcess:
    """postprocess.py:21-73 without the file writes: post_process(feature) -> waveform(s).  This class is the 'ph' (predicted
    phase) algorithm; 'gl' (librosa.griffinlim) is `GriffinLim` below, which has arguments of its own (iterations, momentum,
    seed) and keeps a workspace."""

    def __init__(self, folder=None, algorithm=None):
        if algorithm == "gl":
            raise NotImplementedError("PostProcess reconstructs from the predicted phase; Griffin-Lim is features.GriffinLim")
        self.algorithm = "ph"
        self.waveform = None

    def post_process(self, feature, vector=None, des_shape=STFT_SHAPE, n_fft=N_FFT, win_length=WIN_LENGTH, hop_length=HOP_LENGTH,
                     sr=SAMPLE_RATE, nhwc=None, out=None):
        f, single = _feature_nchw(feature, nhwc)
        wav = out if out is not None else torch.empty((f.shape[0], hop_length * (des_shape[1] - 1)), dtype=torch.float32,
                                                      device=f.device)
        ops.istft_features(f, wav, des_shape[0], des_shape[1], n_fft, win_length, hop_length, denormalize=True)
        self.waveform = wav[0] if single else wav
        return self.waveform

    @staticmethod
    def differentiable(pred, phase_ref=None, des_shape=STFT_SHAPE, n_fft=N_FFT, win_length=WIN_LENGTH, hop_length=HOP_LENGTH):
        """post_process as an autograd node: pred fp32 [B, 2, H, W] (a leaf that requires grad, e.g. a detached copy of an engine's
        prediction) -> waveforms fp32 [B, T].  Any torch expression on the result then trains a model: its backward() leaves
        dL/dpred in pred.grad (csrc/istft_bwd.hip) for an engine's backward(dpred=...).  phase_ref: the network input of a
        phase-difference model (the phase plane is pred + phase_ref); it gets no gradient."""
        return _PostProcessFunction.apply(pred, phase_ref, (int(des_shape[0]), int(des_shape[1])), int(n_fft), int(win_length), int(hop_length))


class _PostProcessFunction(torch.autograd.Function):
    """forward: ops.istft_features on pred (+ phase_ref on the phase plane, in fp32); backward: ops.istft_features_bwd."""

    @staticmethod
    def forward(ctx, pred, phase_ref, des_shape, n_fft, win_length, hop_length):
        if not isinstance(pred, torch.Tensor) or not pred.is_cuda or pred.dim() != 4 or pred.shape[1] != 2:
            raise ValueError("PostProcess.differentiable: pred must be a CUDA tensor [B, 2, H, W]")
        p = pred.detach().contiguous().float()
        r = None if phase_ref is None else phase_ref.detach().contiguous().float()
        feat = p
        if r is not None:
            feat = p.clone()
            feat[:, 1] += r[:, 1]
        wav = torch.empty((p.shape[0], hop_length * (des_shape[1] - 1)), dtype=torch.float32, device=p.device)
        ops.istft_features(feat, wav, des_shape[0], des_shape[1], n_fft, win_length, hop_length, denormalize=True)
        ctx.save_for_backward(p, r)
        ctx.geo = (des_shape, n_fft, win_length, hop_length)
        return wav

    @staticmethod
    def backward(ctx, dwav):
        p, r = ctx.saved_tensors
        des_shape, n_fft, win_length, hop_length = ctx.geo
        dpred = torch.empty_like(p)
        ops.istft_features_bwd(p, dwav.contiguous().float(), dpred, des_shape[0], des_shape[1], n_fft, win_length, hop_length, phase_ref=r)
        return dpred, None, None, None, None, None


class GriffinLim:
    """PostProcess with algorithm='gl' (postprocess.py:47-50, :130-131): post_process(feature) -> waveform(s) from the magnitude
    plane alone, librosa.griffinlim at librosa 0.9.x defaults (PARITY UNPINNED, see csrc/griffinlim.hip) for the whole batch in
    one call of the library, in fp64 with one rounding to fp32.

    The random initial phases are draw number `draws` of stream `seed` (ops.uniform); the counter advances by one per call, so
    successive calls get fresh phases and a rebuilt object with the same seed repeats them.  `init_phase` (fp32
    [B, n_bins, n_frames] or [n_bins, n_frames], turns in [0, 1)) replaces the draw and leaves the counter alone.  The fp64
    workspace is kept while the shape holds.

    `method` "dft" (the default) is that fp64 form, the one to hold a result to a bound; "fft" runs the same loop with fp32 state and
    fp32 FFTs in LDS (csrc/griffinlim_fft.hip): librosa's own complex64 precision, n_iter + 2 launches instead of 2 n_iter + 3 - the
    form for evaluation runs.  It takes n_fft 128 ... 1024 with hop_length >= win_length / 4 (ops.griffinlim_fft_supported); any other
    geometry raises in post_process.  The draws, `init_phase`, the layouts, `out=` and the kept workspace are the same for both."""

    def __init__(self, n_iter=32, momentum=0.99, pad_mode="reflect", seed=0, method="dft"):
        if n_iter < 0 or momentum < 0:
            raise ValueError("n_iter and momentum must not be negative")
        if pad_mode not in ops.PAD_MODES:
            raise ValueError(f"pad_mode must be one of {sorted(ops.PAD_MODES)}")
        if method not in ("dft", "fft"):
            raise ValueError(f'method must be "dft" or "fft", not {method!r}')
        self.method = method
        self.n_iter, self.momentum, self.pad_mode, self.seed = int(n_iter), float(momentum), pad_mode, int(seed)
        self.algorithm = "gl"
        self.waveform = None
        self.draws = 0
        self._ws = None

    def post_process(self, feature, vector=None, des_shape=STFT_SHAPE, n_fft=N_FFT, win_length=WIN_LENGTH, hop_length=HOP_LENGTH,
                     sr=SAMPLE_RATE, nhwc=None, out=None, init_phase=None):
        f, single = _feature_nchw(feature, nhwc)
        if self.method == "fft" and not ops.griffinlim_fft_supported(des_shape[0], des_shape[1], n_fft, win_length, hop_length):
            raise ValueError(f'GriffinLim(method="fft") does not take des_shape {tuple(des_shape)}, n_fft {n_fft}, win_length '
                             f'{win_length}, hop_length {hop_length} (n_fft 128 ... 1024, n_bins = n_fft / 2 + 1, hop_length >= '
                             f'win_length / 4, hop_length (n_frames - 1) > n_fft / 2); use method="dft"')
        wav = out if out is not None else torch.empty((f.shape[0], hop_length * (des_shape[1] - 1)), dtype=torch.float32,
                                                      device=f.device)
        if init_phase is not None:
            if not isinstance(init_phase, torch.Tensor) or not init_phase.is_cuda:
                raise ValueError("init_phase must be a CUDA tensor (there is no CPU path)")
            init_phase = (init_phase.unsqueeze(0) if init_phase.dim() == 2 else init_phase).contiguous().float()
        if self._ws is None or self._ws.device != f.device:
            self._ws = ops.Workspace(f.device)
        op = ops.griffinlim_fft if self.method == "fft" else ops.griffinlim
        op(f, wav, des_shape[0], des_shape[1], n_fft, win_length, hop_length, self._ws, pad_mode=self.pad_mode, denormalize=True,
           n_iter=self.n_iter, momentum=self.momentum, init_phase=init_phase, seed=self.seed, draw=self.draws)
        if init_phase is None:
            self.draws += 1
        self.waveform = wav[0] if single else wav
        return self.waveform

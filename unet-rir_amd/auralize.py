"""Auralization: dry audio rendered through impulse responses on the device (csrc/auralize.hip).

Nobody listens to an impulse response; they convolve a dry recording with it and listen to the result, at every microphone of an array
at once.  `auralize` is that last link behind `PostProcess` / `GriffinLim`:

    wav = PostProcess().post_process(model.predict(spec_in, emb))        # fp32 [B, 9600]: one response per position
    wet = auralize(wav, dry)                                             # fp32 [B, N + 9599]: the dry signal heard at each of them

    y_b[n] = sum_k h_b[k] x_b[n - k]       direct form on the fp32 matrix cores, one launch, fp32 fma chain in ascending k:
                                           exact on integer data, the same bits on every run (include/unetrir.h)

    wet = auralize(wav, dry, method="fft")                               # the same, by partitioned overlap-save (csrc/auralize_fft.hip):
                                           block 2048, FFTs in LDS, two launches and a workspace; within a derived rounding bound
                                           (include/unetrir.h) instead of exact, its own reproducible bits

Which one (profiles/auralize_fft.json, B = 32, x shared): at K = 9600 "fft" is 15 x faster for 2 s of audio and 27 x for 10 s (0.048 and
0.103 ms against 0.715 and 2.77), and 2.7 - 4 x faster than torch.fft.rfft . irfft; "direct" wins below K of a hundred or two (K = 32:
0.031 against 0.037 ms; K = 256: 0.048 against 0.036) and wherever the result must be exact or must not change with the method.

    walk = auralize_path(wavs, dry, spacing=12000)                       # fp32 [1, N + 9599]: ONE listener who walks past the R
                                           positions of wavs [R, 9600], a quarter of a second apart: the outputs crossfaded with
                                           hat-function gains, rendered per block of 2048 through the two or three responses whose
                                           gains touch it - what a generator conditioned on position offers and a measured response
                                           does not (the kernels of method="fft" plus one; its bits wherever one response has gain 1)

`write_wav` is the counterpart of `PostProcess.save_wav` (postprocess.py:135-149) for the rendered signals.
"""
import struct

import numpy as np
import torch

from . import ops


def auralize(rir, dry, length="full", out=None, method="direct"):
    """rir fp32 [B, K] or [K], dry fp32 [N] (one source heard through every response: the microphone-array case) or [B, N] (one source
    per row) -> fp32 [B, L]: the first L samples of the convolution.  length: "full" (N + K - 1), "same" (N) or an int in 1 ... N + K - 1;
    a shorter L returns the head of the full result, bit for bit.  out: a contiguous fp32 [B, L] tensor to write instead of a new one.
    method: "direct" (the default: exact on integer data, one rounding per tap) or "fft" (partitioned overlap-save, block 2048, two
    launches and a workspace of 16 KB per spectrum that lives for the call: within the bound of include/unetrir.h, not exact, other
    bits than "direct" but as reproducible).
    CUDA tensors, contiguous fp32, on one device (checked before the launch: ValueError); the launches go to the current stream and
    nothing synchronises with the host."""
    if method not in ("direct", "fft"):
        raise ValueError(f'auralize: method must be "direct" or "fft", not {method!r}')
    if not isinstance(rir, torch.Tensor) or not isinstance(dry, torch.Tensor):
        raise ValueError("auralize: rir and dry must be tensors")
    if rir.dim() == 1:
        rir = rir.unsqueeze(0)
    if rir.dim() != 2 or dry.dim() not in (1, 2):
        raise ValueError("auralize: rir [B, K] or [K], dry [N] or [B, N]")
    B, K = rir.shape
    N = dry.shape[-1]
    if dry.dim() == 2 and dry.shape[0] != B:
        raise ValueError(f"auralize: batch sizes differ: {dry.shape[0]} dry signals for {B} impulse responses")
    if B < 1 or K < 1 or N < 1:
        raise ValueError("auralize: empty input")
    if length == "full":
        L = N + K - 1
    elif length == "same":
        L = N
    elif isinstance(length, int) and not isinstance(length, bool) and 1 <= length <= N + K - 1:
        L = length
    else:
        raise ValueError(f'length must be "full", "same" or an int in 1 ... N + K - 1 = {N + K - 1}')
    if out is None:
        out = torch.empty((B, L), dtype=torch.float32, device=rir.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, L):
        raise ValueError(f"auralize: out must be a tensor of shape {(B, L)}")
    if method == "fft":
        ops.auralize_fft_f32(rir, dry, out)
    else:
        ops.auralize_f32(rir, dry, out)
    return out


PATH_MIN_SPACING = 32           # samples between neighbouring nodes: at most 66 nodes touch a block of 2048, so cost follows the audio
PATH_MAX_TIME = 1 << 30


def _path_times(times, spacing, start, R):
    """The host checks of a schedule -> int64 numpy [R]"""
    if (times is None) == (spacing is None):
        raise ValueError("auralize_path: give either times or spacing")
    if times is None:
        if isinstance(spacing, bool) or isinstance(start, bool) or int(spacing) != spacing or int(start) != start:
            raise ValueError("auralize_path: spacing and start are whole numbers of samples")
        tau = int(start) + int(spacing) * np.arange(R, dtype=np.int64)
    else:
        if isinstance(times, torch.Tensor):
            if times.is_cuda:
                raise ValueError("auralize_path: times is a host sequence (ops.auralize_path_f32 takes a device tensor)")
            times = times.numpy()
        tau = np.asarray(times)
        if tau.ndim != 1 or tau.shape[0] != R:
            raise ValueError(f"auralize_path: {tau.shape} times for {R} nodes")
        if tau.dtype.kind not in "iu":
            if tau.dtype.kind != "f" or not np.all(np.isfinite(tau)) or np.any(tau != np.rint(tau)):
                raise ValueError("auralize_path: times are whole sample indices")
        tau = tau.astype(np.int64)
    gap = int(np.diff(tau).min()) if R > 1 else PATH_MIN_SPACING
    if gap <= 0:
        raise ValueError("auralize_path: times must be strictly increasing")
    if tau[0] < -PATH_MAX_TIME or tau[-1] > PATH_MAX_TIME:           # increasing: the ends are the extremes
        raise ValueError(f"auralize_path: times out of range: |tau| <= 2^30, got {int(tau[0])} ... {int(tau[-1])}")
    if gap < PATH_MIN_SPACING:
        raise ValueError(f"auralize_path: neighbouring nodes must be at least {PATH_MIN_SPACING} samples apart (the closest are {gap})")
    return tau


def auralize_path(rir, dry, times=None, *, spacing=None, start=0, length="full", out=None):
    """A listener (or source) that moves through the room: dry rendered along a path of impulse responses.

    rir fp32 [R, K] (one listener) or [B, R, K] (the B microphones of an array moved along one schedule), dry fp32 [N] or [B, N],
    times: a host sequence (list, numpy array or CPU tensor) of R strictly increasing sample indices tau_r of the OUTPUT at which the
    listener is at position r (negative or beyond the output is fine), or spacing=D, start=s for tau_r = s + r D.  -> fp32 [B, L]:

        n <= tau_0: y_0[n]      n >= tau_{R-1}: y_{R-1}[n]      tau_r <= n < tau_{r+1}: (1 - a) y_r[n] + a y_{r+1}[n],  a = (n - tau_r) / (tau_{r+1} - tau_r)

    with y_r = h_r * x: the outputs crossfaded linearly, which is a filter interpolated per output sample.  Rendered per output block of
    2048 samples through the nodes whose gains touch it only (csrc/auralize_fft.hip: the spectra of `auralize(method="fft")`, then one
    product chain and inverse transform per block and node, blended in registers): two launches, no intermediate y_r, a workspace of 16
    KB per spectrum.  Where a single node has gain 1 (before tau_0, after tau_{R-1}, at every tau_r, R = 1) the bits are those of
    `auralize(h_r, dry, method="fft")`; error bound in include/unetrir.h.  length and out as `auralize`.
    Checked on the host before any launch (ValueError): shapes, dtypes, devices; times strictly increasing, |tau| <= 2^30, neighbours at
    least 32 samples apart.  times is uploaded once as int32 without blocking; `ops.auralize_path_f32` takes a device tensor instead."""
    if not isinstance(rir, torch.Tensor) or not isinstance(dry, torch.Tensor):
        raise ValueError("auralize: rir and dry must be tensors")
    if rir.dim() == 2:
        rir = rir.unsqueeze(0)
    if rir.dim() != 3 or dry.dim() not in (1, 2):
        raise ValueError("auralize: rir [R, K] or [B, R, K], dry [N] or [B, N]")
    B, R, K = rir.shape
    N = dry.shape[-1]
    if dry.dim() == 2 and dry.shape[0] != B:
        raise ValueError(f"auralize: batch sizes differ: {dry.shape[0]} dry signals for {B} paths")
    if B < 1 or R < 1 or K < 1 or N < 1:
        raise ValueError("auralize: empty input")
    if length == "full":
        L = N + K - 1
    elif length == "same":
        L = N
    elif isinstance(length, int) and not isinstance(length, bool) and 1 <= length <= N + K - 1:
        L = length
    else:
        raise ValueError(f'length must be "full", "same" or an int in 1 ... N + K - 1 = {N + K - 1}')
    tau = _path_times(times, spacing, start, R)
    if out is None:
        out = torch.empty((B, L), dtype=torch.float32, device=rir.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, L):
        raise ValueError(f"auralize: out must be a tensor of shape {(B, L)}")
    host = torch.from_numpy(tau.astype(np.int32))
    if rir.is_cuda:
        host = host.pin_memory()
    ops.auralize_path_f32(rir, host.to(rir.device, non_blocking=True), dry, out)
    return out


def write_wav(path, data, rate):
    """A 32-bit IEEE-float RIFF file (format tag 3) of data [T] or [T, channels], values written as they are (no scaling, no clipping);
    `read_wav` returns them minus their mean."""
    if isinstance(data, torch.Tensor):
        data = data.detach().cpu().numpy()
    x = np.ascontiguousarray(data, dtype="<f4")
    if x.ndim not in (1, 2) or x.shape[0] < 1 or (x.ndim == 2 and not 1 <= x.shape[1] <= 65535):
        raise ValueError("write_wav: data must be [T] or [T, channels] with T >= 1")
    rate = int(rate)
    if rate < 1:
        raise ValueError("write_wav: the sample rate must be positive")
    channels = 1 if x.ndim == 1 else x.shape[1]
    raw = x.tobytes()
    if len(raw) + 50 > 0xffffffff:
        raise ValueError("write_wav: more than 4 GB of samples do not fit a RIFF file")
    fmt = struct.pack("<4sIHHIIHHH", b"fmt ", 18, 3, channels, rate, rate * channels * 4, channels * 4, 32, 0)
    fact = struct.pack("<4sII", b"fact", 4, x.shape[0])
    body = b"WAVE" + fmt + fact + struct.pack("<4sI", b"data", len(raw)) + raw
    with open(path, "wb") as f:
        f.write(struct.pack("<4sI", b"RIFF", len(body)) + body)

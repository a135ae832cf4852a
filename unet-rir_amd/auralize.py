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

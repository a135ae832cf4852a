"""Sample-rate conversion on the device (csrc/resample.hip): the link in front of `read_wav`, `Dataset` and `auralize` for audio that
is not at the model's rate - speech at 16 kHz, music at 44.1 kHz.

    r = Resampler(44100, 48000)                      # ratio reduced to L / M = 160 / 147, table [160, 128] built in fp64, uploaded once
    y = r(x)                                         # fp32 [B, ceil(N 160 / 147)]: one launch on the current stream
    y = resample(x, 16000, 48000, "kaiser_fast")     # the same through a small cache of plans

A polyphase FIR with a Kaiser-windowed sinc, evaluated at the exact phase of every output (no interpolated filter table):

    y[m] = sum_n h(m M / L - n) x[n]     0 <= m < ceil(N L / M)          the definition, the table and the summation order: include/unetrir.h

The output length is librosa's, the signal is extended with zeros, the gain at DC is 1 in both directions.  The presets carry librosa's
`res_type` names and resampy's filter parameters; neither package is a dependency, and the fp64 restatement in tests/resample_ref.py
is what the kernel is held to.
"""
import math

import torch

from . import ops

__all__ = ["Resampler", "resample", "PRESETS"]

PRESETS = {                                         # res_type: (zeros, rolloff, beta)
    "kaiser_best": (64, 0.9475937167399596, 14.769656459379492),
    "kaiser_fast": (16, 0.85, 8.555504641634386),
}
MAX_RATIO, MAX_ZEROS, MAX_TAPS, MAX_TABLE = 2048, 64, 8192, 1 << 20


def _whole(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or int(v) < 1:
        raise ValueError(f"resample: {what} must be a whole number >= 1, not {v!r}")
    return int(v)


class Resampler:
    """rate_in -> rate_out with the filter of `res_type` ("kaiser_best", "kaiser_fast"); zeros / rolloff / beta replace single values
    of the preset.  device: where the table lives (default: the current CUDA device).  `.L`, `.M`: the reduced ratio rate_out / rate_in;
    `.taps`: T; `.table`: fp32 [L, T] on the device (None for equal rates).
    ValueError: an unknown res_type, a rate below 1, or a ratio the kernel does not take - the message names L, M and the limit."""

    def __init__(self, rate_in, rate_out, res_type="kaiser_best", *, zeros=None, rolloff=None, beta=None, device=None):
        if res_type not in PRESETS:
            raise ValueError(f"resample: res_type must be one of {sorted(PRESETS)}, not {res_type!r}")
        rate_in, rate_out = _whole(rate_in, "rate_in"), _whole(rate_out, "rate_out")
        z, r, b = PRESETS[res_type]
        self.zeros = z if zeros is None else _whole(zeros, "zeros")
        self.rolloff = float(r if rolloff is None else rolloff)
        self.beta = float(b if beta is None else beta)
        if not 0.0 < self.rolloff <= 1.0 or not 0.0 <= self.beta <= 32.0:
            raise ValueError(f"resample: rolloff {self.rolloff} outside (0, 1] or beta {self.beta} outside [0, 32]")
        g = math.gcd(rate_in, rate_out)
        self.rate_in, self.rate_out, self.res_type = rate_in, rate_out, res_type
        self.L, self.M = rate_out // g, rate_in // g
        L, M = self.L, self.M
        T = 2 * -(-self.zeros * max(L, M) // L)
        for what, value, limit in (("L", L, MAX_RATIO), ("M", M, MAX_RATIO), ("zeros", self.zeros, MAX_ZEROS), ("T", T, MAX_TAPS),
                                   ("L T", L * T, MAX_TABLE)):
            if value > limit:
                raise ValueError(f"resample: {rate_in} -> {rate_out} Hz reduces to L = {L}, M = {M}: {what} = {value} is beyond the "
                                 f"limit of {limit}")
        self.taps = T
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cuda"
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None and torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise ValueError(f"resample: the resampler runs on a CUDA device, not on {self.device} (there is no CPU path)")
        self.table = None
        if L != M:                                  # equal rates: no table, no launch
            if not torch.cuda.is_available():
                raise ValueError(f"resample: no CUDA device is available for {self.device} (there is no CPU path)")
            self.table = ops.resample_table(L, M, self.zeros, self.rolloff, self.beta).to(self.device)

    def out_length(self, N):
        """ceil(N L / M): librosa's int(np.ceil(n * ratio)) in integers."""
        return -(-int(N) * self.L // self.M)

    def __call__(self, x, length=None, out=None):
        """x fp32 [N] or [B, N] on the resampler's device -> fp32 [B, length]; length: None (out_length(N)) or an int in 1 ... that,
        which returns the head of the full result bit for bit.  out: a contiguous fp32 [B, length] tensor to write instead of a new one.
        One launch on the current stream, nothing synchronises with the host.  Equal rates: a copy of the input, no launch."""
        if not isinstance(x, torch.Tensor):
            raise ValueError("resample: x must be a tensor")
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("resample: x [N] or [B, N], not empty")
        B, N = x.shape
        full = self.out_length(N)
        if length is None:
            length = full
        elif isinstance(length, bool) or not isinstance(length, int) or not 1 <= length <= full:
            raise ValueError(f"resample: length must be None or an int in 1 ... {full}")
        if out is None:
            out = torch.empty((B, length), dtype=torch.float32, device=x.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, length):
            raise ValueError(f"resample: out must be a tensor of shape {(B, length)}")
        if self.table is None:
            if x.dtype != torch.float32 or out.dtype != torch.float32:
                raise ValueError("resample: x and out must be float32")
            out.copy_(x[:, :length])
            return out
        if x.is_cuda and x.device != self.device:
            raise ValueError(f"resample: x is on {x.device}, the resampler on {self.device}")
        with torch.cuda.device(self.device):
            ops.resample_f32(x, self.table, self.L, self.M, out)
        return out


_PLANS = {}
_MAX_PLANS = 16


def resample(x, rate_in, rate_out, res_type="kaiser_best", *, length=None, out=None, **kw):
    """`Resampler(rate_in, rate_out, res_type, **kw)(x, length, out)` through a cache of the last 16 plans, keyed by the reduced ratio,
    the filter parameters and the device of x: the table of a ratio is built and uploaded once."""
    if not isinstance(x, torch.Tensor):
        raise ValueError("resample: x must be a tensor")
    if not x.is_cuda:
        raise ValueError(f"resample: x must be a CUDA tensor, not on {x.device} (there is no CPU path)")
    unknown = sorted(set(kw) - {"zeros", "rolloff", "beta"})
    if unknown:
        raise ValueError(f"resample: unknown arguments {unknown}")
    if isinstance(rate_in, int) and isinstance(rate_out, int) and rate_in >= 1 and rate_out >= 1:
        g = math.gcd(rate_in, rate_out)
        key = (rate_out // g, rate_in // g, res_type, kw.get("zeros"), kw.get("rolloff"), kw.get("beta"), str(x.device))
    else:
        key = None                                  # the constructor raises
    plan = _PLANS.pop(key, None) if key is not None else None
    if plan is None:
        plan = Resampler(rate_in, rate_out, res_type, device=x.device, **kw)
    if key is not None:
        _PLANS[key] = plan                          # most recently used last
        while len(_PLANS) > _MAX_PLANS:
            _PLANS.pop(next(iter(_PLANS)))
    return plan(x, length, out)

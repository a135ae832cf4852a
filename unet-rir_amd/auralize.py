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

    s = AuralizeStream(wav, max_blocks=8); y = s.push(chunk); s.update(new_wav); tail = s.flush()
                                           method="fft" for audio that arrives over time: chunks of any length in, whole blocks of 2048
                                           out, the bits of the one-shot call however the input was cut; the response exchanged with a
                                           crossfade of one block; a device state that does not grow, three launches per push
                                           (profiles/auralize_stream.json: 0.023 - 0.034 ms per push for up to 8 blocks x 32 rows)

`write_wav` is the counterpart of `PostProcess.save_wav` (postprocess.py:135-149) for the rendered signals; `WavWriter` writes the same
file piece by piece.
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


class AuralizeStream:
    """`auralize(rir, dry, method="fft")` for a dry signal that arrives over time, and a response that can be exchanged while it runs.

        s = AuralizeStream(rir, dry_rows="shared", max_blocks=8)      # rir fp32 [B, K] on the device
        for chunk in source:                                            # fp32 [n] (shared) or [B, n] (dry_rows="rows"), any n >= 0
            y = s.push(chunk)                                           # [B, m]: the output blocks that are complete, maybe [B, 0]
            ...                                                         # s.update(new_rir) whenever the listener has moved
        tail = s.flush()                                                # the rest, K - 1 samples of reverberation included

    The concatenation of every `push` and the `flush` is `auralize(rir, all_chunks, method="fft", length="full")` BIT FOR BIT, however
    the input was cut into chunks: the kernels are those of the FFT form on the same block grid (block `s.block` = 2048), with the last
    spectra of the input in a ring on the device (csrc/auralize_fft.hip, include/unetrir.h).  Memory does not grow with the stream:
    `s.state_bytes` of state and a staging buffer of (max_blocks + 1) blocks per dry row.

    Latency: output comes in whole blocks, so it lags the input by up to block - 1 = 2047 samples (42.6 ms at 48 kHz); `samples_in` and
    `samples_out` count both ends.  Smaller blocks are not offered.

    `update(rir)` exchanges the response: the new one is heard from output sample `samples_out` on (the next block), faded in linearly
    across exactly that block - `auralize_path` with the old response at that sample and the new one a block later, bit for bit - and
    alone from the block after.  Several updates before the next block is rendered: the last one wins.

    dry_rows: "shared" - chunks are [n], one signal heard through every response - or "rows" - chunks are [B, n].  max_blocks (1 ... 64):
    the most blocks one kernel call renders; longer chunks become several calls.  A chunk that is a whole number of blocks with nothing
    pending is rendered from where it lies; anything else goes through the staging buffer.  state: a uint8 tensor on the device of rir
    to keep the state in instead of a new one (`ops.auralize_stream_state_bytes` bytes or more, 16-byte aligned).  All bookkeeping is on the host, which knows
    every length: nothing here synchronises with the device, and the launches go to the current stream."""

    def __init__(self, rir, dry_rows="shared", max_blocks=8, state=None):
        if dry_rows not in ("shared", "rows"):
            raise ValueError(f'AuralizeStream: dry_rows must be "shared" or "rows", not {dry_rows!r}')
        if not isinstance(rir, torch.Tensor):
            raise ValueError("AuralizeStream: rir must be a tensor")
        if rir.dim() == 1:
            rir = rir.unsqueeze(0)
        if rir.dim() != 2 or rir.shape[0] < 1 or rir.shape[1] < 1:
            raise ValueError("AuralizeStream: rir [B, K] or [K], not empty")
        if isinstance(max_blocks, bool) or not isinstance(max_blocks, int) or not 1 <= max_blocks <= 64:
            raise ValueError(f"AuralizeStream: max_blocks must be an int in 1 ... 64, not {max_blocks!r}")
        B, K = rir.shape
        if not ops.auralize_stream_supported(K):
            raise ValueError(f"auralize: impulse responses of {K} taps are not supported (1 ... 16384)")
        if rir.dtype != torch.float32:
            raise ValueError(f"AuralizeStream: rir must be float32, not {rir.dtype}")
        if not rir.is_cuda:
            raise ValueError("AuralizeStream: rir must be a CUDA tensor (there is no CPU path)")
        self.rows = dry_rows == "rows"
        self._state = ops.AuralizeStreamState(rir.device, B, K, B if self.rows else 1, max_blocks, buf=state)
        self.B, self.K, self.max_blocks = B, K, max_blocks
        self.block = self._state.block
        self._stage = torch.empty((self._state.dry_rows, (max_blocks + 1) * self.block), dtype=torch.float32, device=rir.device)
        self._rir = None
        self.reset(rir)

    @property
    def state_bytes(self):
        return self._state.need

    def reset(self, rir=None):
        """Back to the first sample: silence before it, nothing pending, the response rir - or, with None, the latest one given."""
        if rir is not None:
            if isinstance(rir, torch.Tensor) and rir.dim() == 1:
                rir = rir.unsqueeze(0)
            ops._stream_rir(self._state, rir, "AuralizeStream.reset")
            self._rir = rir.clone()
        ops.auralize_stream_init(self._state, self._rir)
        self.samples_in = self.samples_out = self._pending = 0

    def update(self, rir):
        """A new response fp32 [B, K], heard from output sample `samples_out` on and faded in across one block."""
        if isinstance(rir, torch.Tensor) and rir.dim() == 1:
            rir = rir.unsqueeze(0)
        ops._stream_rir(self._state, rir, "AuralizeStream.update")
        self._rir = rir.clone()
        ops.auralize_stream_update(self._state, self._rir)

    def _render(self, dry, out, at):
        """the whole blocks of dry (or as many blocks of zeros as fit the rest of out) -> out[:, at:], in calls of at most max_blocks"""
        P, step = self.block, self.max_blocks * self.block
        n = dry.shape[-1] if dry is not None else out.shape[1] - at
        for lo in range(0, n, step):
            hi = min(lo + step, n)
            ops.auralize_stream_push_f32(self._state, None if dry is None else dry[..., lo:hi], out[:, at + lo:at + hi])
        self.samples_out += n
        return at + n

    def push(self, chunk, out=None):
        """chunk fp32 [n] or [B, n] (as dry_rows says), n >= 0 -> fp32 [B, m], m = block * floor((pending + n) / block): every output
        block the input completes, possibly none.  out: a contiguous fp32 [B, m] tensor to write instead of a new one."""
        st, P = self._state, self.block
        if not isinstance(chunk, torch.Tensor):
            raise ValueError("AuralizeStream.push: chunk must be a tensor")
        if chunk.dim() != (2 if self.rows else 1) or (self.rows and chunk.shape[0] != self.B):
            raise ValueError(f"AuralizeStream.push: chunk must be {'[' + str(self.B) + ', n]' if self.rows else '[n]'} for dry_rows = "
                             f"{'rows' if self.rows else 'shared'!r}, not {tuple(chunk.shape)}")
        if chunk.dtype != torch.float32:
            raise ValueError(f"AuralizeStream.push: chunk must be float32, not {chunk.dtype}")
        if not chunk.is_cuda or chunk.device != st.buf.device:
            raise ValueError("AuralizeStream.push: chunk must be a CUDA tensor on the device of the stream (there is no CPU path)")
        if chunk.stride(-1) != 1 and chunk.shape[-1] > 1:
            chunk = chunk.contiguous()
        n = chunk.shape[-1]
        m = (self._pending + n) // P * P
        if out is None:
            out = torch.empty((self.B, m), dtype=torch.float32, device=chunk.device)
        elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != (self.B, m) or out.dtype != torch.float32 or
              not out.is_contiguous() or out.device != chunk.device):
            raise ValueError(f"AuralizeStream.push: out must be a contiguous float32 tensor of shape {(self.B, m)} on {chunk.device}")
        self.samples_in += n
        pos = at = 0
        cap = self._stage.shape[1]
        while True:
            if self._pending == 0 and n - pos >= P:                 # whole blocks with nothing pending: rendered where they lie
                whole = (n - pos) // P * P
                at = self._render(chunk[..., pos:pos + whole], out, at)
                pos += whole
            if pos < n:
                c = min(n - pos, cap - self._pending)
                self._stage[:, self._pending:self._pending + c].copy_(chunk[..., pos:pos + c])
                self._pending += c
                pos += c
            whole = self._pending // P * P
            if not whole:
                break
            whole = min(whole, self.max_blocks * P)
            at = self._render(self._stage[:, :whole], out, at)
            rest = self._pending - whole                             # at most one block: it cannot overlap where it goes
            if rest:
                self._stage[:, :rest].copy_(self._stage[:, whole:whole + rest])
            self._pending = rest
        assert at == m and pos == n
        return out

    def flush(self):
        """The rest of the output - the pending input followed by zeros: samples_in + K - 1 - samples_out samples, fp32 [B, that many]
        ([B, 0] for a stream that took no input) - and then `reset()`."""
        P = self.block
        need = self.samples_in + self.K - 1 - self.samples_out if self.samples_in else 0
        out = torch.empty((self.B, -(-need // P) * P), dtype=torch.float32, device=self._stage.device)
        at = 0
        if out.shape[1]:
            if self._pending:
                self._stage[:, self._pending:P].zero_()
                at = self._render(self._stage[:, :P], out, 0)
            if at < out.shape[1]:
                self._render(None, out, at)
        self.reset()
        return out[:, :need].contiguous()


class WavWriter:
    """`write_wav` piece by piece, for a signal that is never whole in memory: the same 32-bit float file, byte for byte, with the lengths
    of the header patched in by `close` (also at the end of a `with` block).

        with WavWriter(path, rate) as w:
            for block in blocks:          # [t] or [t, channels], values written as they are
                w.write(block)"""

    def __init__(self, path, rate, channels=1):
        rate, channels = int(rate), int(channels)
        if rate < 1 or not 1 <= channels <= 65535:
            raise ValueError("WavWriter: the sample rate must be positive and the channels 1 ... 65535")
        self.channels, self.frames = channels, 0
        self._f = open(path, "wb")
        fmt = struct.pack("<4sIHHIIHHH", b"fmt ", 18, 3, channels, rate, rate * channels * 4, channels * 4, 32, 0)
        self._f.write(struct.pack("<4sI", b"RIFF", 0) + b"WAVE" + fmt + struct.pack("<4sII", b"fact", 4, 0) + struct.pack("<4sI", b"data", 0))

    def write(self, data):
        if isinstance(data, torch.Tensor):
            data = data.detach().cpu().numpy()
        x = np.ascontiguousarray(data, dtype="<f4")
        if x.ndim not in (1, 2) or (1 if x.ndim == 1 else x.shape[1]) != self.channels:
            raise ValueError(f"WavWriter: data must be [t] or [t, channels] with {self.channels} channels")
        if 4 * self.channels * (self.frames + x.shape[0]) + 50 > 0xffffffff:
            raise ValueError("WavWriter: more than 4 GB of samples do not fit a RIFF file")
        self._f.write(x.tobytes())
        self.frames += x.shape[0]

    def close(self):
        if self._f is None:
            return
        size = 4 * self.channels * self.frames
        for at, value in ((4, 50 + size), (46, self.frames), (54, size)):           # RIFF, fact and data lengths
            self._f.seek(at)
            self._f.write(struct.pack("<I", value))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


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

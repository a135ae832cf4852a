"""Render a dry recording through impulse responses, on the device: one .wav per position (unet_rir_amd.auralize), or with --walk one
.wav of a listener who moves from position to position (unet_rir_amd.auralize_path).

    python scripts/auralize.py --rirs RIR_DIR --dry speech.wav --out OUT_DIR
    python scripts/auralize.py --checkpoint CKPT_DIR --filters 32 --kernels 3 --data BATCH_DIR --dry speech.wav --out OUT_DIR
    python scripts/auralize.py --load SAVED_MODEL_DIR --arch aenet --synthetic 1 --dry speech.wav --out OUT_DIR [--diff-gen]
    python scripts/auralize.py --rirs RIR_DIR --dry speech.wav --out OUT_DIR --walk 250
    python scripts/auralize.py --rirs RIR_DIR --dry hour_long.wav --out OUT_DIR --stream

--rirs         a directory of impulse-response .wav files (sorted by name), read by `read_wav`'s rules: --sr Hz, the first --duration
               seconds, mean removed; files at another rate need --resample
--load / --checkpoint / --arch / --filters / --kernels / --latent / --height / --width
               a model, as scripts/evaluate.py takes it; its responses are generated from --data (a directory of .npz batches with
               spec_in and emb, as scripts/evaluate.py reads them) or --synthetic N batches, and reconstructed by PostProcess
               (--diff-gen: the predicted phase is a difference to the input's)
--dry          the dry recording: a .wav file, read whole by the same rules (channels averaged, mean removed); at --sr, or at any
               rate with --resample
--resample     none (default: a file that is not at --sr is an error), kaiser_best or kaiser_fast: --dry and --rirs files at another
               rate are converted to --sr on the device (unet_rir_amd.Resampler; the names are librosa's res_type)
--length       full (default: N + K - 1 samples), same (N) or a number of samples
--method       direct (default: one fma per tap on the matrix cores, exact on integer data) or fft (partitioned overlap-save: the fast
               one for long recordings, within a rounding bound instead of exact)
--walk MS      the responses become ONE path, neighbouring positions MS milliseconds apart, the first at the start of the output: the
               files of --rirs in sorted order, or a model's responses in the order they are generated, over all batches.  One file,
               OUT_DIR/walk.wav; --length and --peak as without it; on the FFT form whatever --method says (MS at --sr must come to
               at least 32 samples)
--stream       render block by block (unet_rir_amd.AuralizeStream): --dry is read in chunks of --chunk-ms milliseconds (default 1000), in two
               passes - the mean that `read_wav` removes, then the rendering - and every output file is written as it is produced, so
               memory does not depend on the length of the recording.  The files are those of --method fft, byte for byte.  The dry file
               is read once per batch of responses (--batch).  Not with --resample, --peak or --walk: each needs the whole signal
--out          OUT_DIR/NAME.wav per position, 32-bit float at --sr: NAME is the response's file name, or b{batch}_{row} for generated ones
--peak         scale every output file so that the loudest sample of the whole set is this (default: values as computed)
"""
import argparse
import glob
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import unet_rir_amd as U
from unet_rir_amd.auralize import WavWriter, write_wav
from unet_rir_amd.dataset import _pcm
from unet_rir_amd.features import PostProcess


def wav_frames(path):
    """(frames, rate) of a RIFF/WAVE file, from its 'fmt ' and 'data' chunks."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise SystemExit(f"{path}: not a RIFF/WAVE file")
        align = rate = None
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                raise SystemExit(f"{path}: no data chunk")
            name, size = struct.unpack("<4sI", ck)
            if name == b"fmt ":
                fmt = struct.unpack("<HHIIHH", f.read(16))
                rate, align = fmt[2], fmt[4]
                f.seek(size - 16 + (size & 1), 1)
            elif name == b"data":
                if not align:
                    raise SystemExit(f"{path}: data before fmt")
                return size // align, rate
            else:
                f.seek(size + (size & 1), 1)


def dry_chunks(path, frames_per_chunk):
    """-> (frames, rate, chunks): chunks() yields the file as fp32 [n, channels] pieces of frames_per_chunk frames (the last shorter),
    decoded as `read_wav` decodes them: PCM of 16, 24 or 32 bits through the standard `wave` module, 32- and 64-bit IEEE float (which
    `wave` does not take) from the data chunk itself."""
    import wave
    try:
        with wave.open(path, "rb") as f:
            rate, channels, width, total = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()

        def chunks():
            with wave.open(path, "rb") as f:
                for _ in range(0, total, frames_per_chunk):
                    yield _pcm(f.readframes(frames_per_chunk), width, channels, path)
        return total, rate, chunks
    except wave.Error:
        pass
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise SystemExit(f"{path}: not a RIFF/WAVE file")
        fmt = None
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                raise SystemExit(f"{path}: no data chunk")
            name, size = struct.unpack("<4sI", ck)
            if name == b"fmt ":
                fmt = struct.unpack("<HHIIHH", f.read(16))
                f.seek(size - 16 + (size & 1), 1)
            elif name == b"data":
                start = f.tell()
                break
            else:
                f.seek(size + (size & 1), 1)
    if fmt is None or fmt[0] != 3 or fmt[5] not in (32, 64):
        raise SystemExit(f"{path}: --stream reads PCM and IEEE-float wav files")
    channels, rate, width = fmt[1], fmt[2], fmt[5] // 8
    total = size // (width * channels)

    def chunks():
        with open(path, "rb") as f:
            f.seek(start)
            for at in range(0, total, frames_per_chunk):
                n = min(frames_per_chunk, total - at)
                raw = np.frombuffer(f.read(n * width * channels), dtype="<f4" if width == 4 else "<f8")
                yield raw.astype(np.float32).reshape(n, channels)
    return total, rate, chunks


def dry_mean(chunks):
    """The mean `read_wav` removes - np.mean of the channel-averaged fp32 signal - from the signal in pieces: numpy sums an fp32 array
    in runs of np.getbufsize() elements, each pairwise, and adds the runs up in order; so do we, one run at a time.  -> (fp32 mean, n)"""
    run = np.getbufsize()
    total, n, rest = np.float32(0.0), 0, np.zeros(0, dtype=np.float32)
    for x in chunks():
        mono = np.concatenate([rest, x.mean(axis=1, dtype=np.float32)])
        whole = mono.shape[0] // run * run
        for at in range(0, whole, run):
            total = np.float32(total + np.add.reduce(mono[at:at + run]))
        n += whole
        rest = mono[whole:]
    if rest.shape[0]:
        total = np.float32(total + np.add.reduce(rest))
        n += rest.shape[0]
    return np.float32(total / np.float32(n)), n


def stream(a, dev, batches, length):
    """--stream: per batch of responses one AuralizeStream, the dry file pushed through it chunk by chunk, the output files written as
    the blocks arrive and cut to the --length asked for"""
    per_chunk = max(1, int(round(a.chunk_ms * a.sr / 1000.0)))
    per_chunk = -(-per_chunk // np.getbufsize()) * np.getbufsize()                          # whole runs of the mean's summation
    frames, rate, chunks = dry_chunks(a.dry, per_chunk)
    if rate != a.sr:
        raise SystemExit(f"{a.dry}: sample rate {rate} Hz, expected {a.sr} Hz (--stream does not resample)")
    if frames < 1:
        raise SystemExit(f"{a.dry}: no samples")
    mean, n = dry_mean(chunks)
    assert n == frames
    count = L = 0
    for names, wav in batches:
        wav = wav.float().contiguous()
        K = wav.shape[1]
        L = frames + K - 1 if length == "full" else frames if length == "same" else length
        if not 1 <= L <= frames + K - 1:
            raise SystemExit(f"--length must be full, same or 1 ... N + K - 1 = {frames + K - 1}")
        s = U.AuralizeStream(wav, "shared", max_blocks=8)
        writers = [WavWriter(os.path.join(a.out, name + ".wav"), a.sr) for name in names]
        done = 0

        def emit(y):
            nonlocal done
            y = y[:, :max(0, min(y.shape[1], L - done))].cpu().numpy()
            for w, row in zip(writers, y):
                w.write(row)
            done += y.shape[1]
        for x in chunks():
            mono = x.mean(axis=1, dtype=np.float32)
            mono -= mean
            emit(s.push(torch.from_numpy(mono).to(dev)))
        emit(s.flush())
        for w in writers:
            w.close()
        assert done == L
        count += len(names)
    print(f"streamed {count} files of {L} samples to {a.out} (dry: {frames} samples at {rate} Hz, in chunks of {per_chunk}; "
          f"mean removed {float(mean):.6g})")


def rir_batches(a, dev):
    files = sorted(glob.glob(os.path.join(a.rirs, "*.wav")))
    if not files:
        raise SystemExit(f"no .wav files in {a.rirs}")
    for i in range(0, len(files), a.batch):
        part = files[i:i + a.batch]
        wav = np.stack([U.read_wav(f, a.sr, a.duration, resample=a.resample) for f in part])
        yield [os.path.splitext(os.path.basename(f))[0] for f in part], torch.from_numpy(wav).to(dev)


def model_batches(a, dev):
    import evaluate as E                                         # scripts/evaluate.py: the same model and batch sources
    model = E.build_model(a, dev)
    post = PostProcess()
    for k, batch in enumerate(E.file_batches(a.data, dev) if a.data else E.synthetic(a, dev)):
        spec_in, emb = batch[0], batch[1]
        nhwc = spec_in if spec_in.shape[-1] == 2 else spec_in.permute(0, 2, 3, 1)
        with torch.no_grad():
            pred = model.model([nhwc, emb], training=False)      # NHWC
        feat = pred.permute(0, 3, 1, 2).contiguous().float()
        if a.diff_gen:
            feat[:, 1] += nhwc.permute(0, 3, 1, 2)[:, 1]
        wav = post.post_process(feat, nhwc=False)
        yield [f"b{k:04d}_{j:02d}" for j in range(wav.shape[0])], wav


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rirs")
    ap.add_argument("--load")
    ap.add_argument("--checkpoint")
    ap.add_argument("--arch", choices=("unet", "resae", "ae", "vae", "vqvae", "aenet", "diffunet", "diffvae"), default="unet")
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--filters", type=int, default=32)
    ap.add_argument("--kernels", type=int, default=3)
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--data")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--diff-gen", action="store_true")
    ap.add_argument("--name", default="unet")
    ap.add_argument("--dry", required=True)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--duration", type=float, default=0.2, help="seconds of every --rirs file that are used")
    ap.add_argument("--length", default="full")
    ap.add_argument("--method", choices=("direct", "fft"), default="direct")
    ap.add_argument("--peak", type=float, default=None)
    ap.add_argument("--walk", type=float, default=None, metavar="MS")
    ap.add_argument("--resample", choices=("none", "kaiser_best", "kaiser_fast"), default="none")
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--chunk-ms", type=float, default=1000.0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    a.resample = None if a.resample == "none" else a.resample
    generated = bool(a.load or a.checkpoint or a.data or a.synthetic)
    if bool(a.rirs) == generated:
        raise SystemExit("give either --rirs, or a model (--load / --checkpoint) with --data or --synthetic")
    if generated and bool(a.data) == bool(a.synthetic):
        raise SystemExit("a model needs exactly one of --data and --synthetic")
    length = a.length if a.length in ("full", "same") else int(a.length)
    if a.stream:
        for given, option in ((a.resample is not None, "--resample"), (a.peak is not None, "--peak"), (a.walk is not None, "--walk")):
            if given:
                raise SystemExit(f"--stream does not go with {option}: it needs the whole signal (or a schedule) before the first block")
        if a.chunk_ms <= 0:
            raise SystemExit("--chunk-ms must be positive")
    if not torch.cuda.is_available():
        raise SystemExit("auralization runs on the GPU; there is none here")
    dev = torch.device("cuda:0")
    if a.stream:
        os.makedirs(a.out, exist_ok=True)
        with torch.cuda.device(dev):
            stream(a, dev, rir_batches(a, dev) if a.rirs else model_batches(a, dev), length)
        return
    frames, rate = wav_frames(a.dry)
    # the whole file: int(duration * rate) = frames, and int(duration * sr) <= ceil(frames * sr / rate), what resampling yields
    duration = (frames + min(0.5, 0.5 * rate / a.sr)) / rate
    with torch.cuda.device(dev):
        dry = torch.from_numpy(U.read_wav(a.dry, a.sr, duration, resample=a.resample)).to(dev)
    os.makedirs(a.out, exist_ok=True)
    rendered = []
    batches = rir_batches(a, dev) if a.rirs else model_batches(a, dev)
    if a.walk is not None:
        spacing = int(round(a.walk * a.sr / 1000.0))
        path = torch.cat([wav.float() for _, wav in batches]).contiguous()                 # [R, K]: one listener, R positions
        wet = U.auralize_path(path, dry, spacing=spacing, start=0, length=length)[0].cpu().numpy()
        batches = []
        rendered = [("walk", wet)]
    for names, wav in batches:
        wet = U.auralize(wav, dry, length=length, method=a.method).cpu().numpy()
        rendered += list(zip(names, wet))
    gain = 1.0
    if a.peak is not None:
        top = max(float(np.abs(w).max()) for _, w in rendered)
        gain = a.peak / top if top > 0 else 1.0
    for name, w in rendered:
        write_wav(os.path.join(a.out, name + ".wav"), w * np.float32(gain), a.sr)
    if a.walk is not None:
        print(f"walked {path.shape[0]} positions, {spacing} samples apart")
    print(f"wrote {len(rendered)} files of {rendered[0][1].shape[0]} samples to {a.out} (dry: {frames} samples at {rate} Hz, gain {gain:.6g})")


if __name__ == "__main__":
    main()

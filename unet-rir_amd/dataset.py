"""The reference's data set and batch generator, with the features resident on the device.

`Dataset` (dataset.py:11-244) walks a tree of impulse responses

    dir_dataset/dataset_name/Room/ZoneX/YMicrophoneArray/Room_ZoneX_YMicrophoneArray_Ll_Mm.wav

keeps the files whose room and array are asked for (:147-154), numbers them in walk order, builds the information vector of
each (`rooms.uts_room_embedding`; :185-212) and the per-room index lists, and pairs every position with a shuffled position of
the same room (:173-182).  `DataGenerator` (datageneratorv2.py:8-102) shuffles the pairs with the data set's seed, cuts the
70 / 20 / 10 partitions and hands out batches `(spec_in, emb, spec_out)`.  Names, argument order and defaults are the
reference's; what differs:

  * the whole data set lives in HBM as one feature bank fp32 `[N, 2, H, W]` (N x 184 320 bytes at 144 x 160), produced from the
    decoded waveforms by the package's own `PreProcess` kernel, and a batch is ONE gather launch (`ops.gather_batch`,
    csrc/dataset.hip) on the current stream: no host -> device copy, no permute, no host synchronisation per step.  Batches
    are contiguous NCHW fp32 (`Trainer.step`'s boundary), not NHWC;
  * directory entries are visited in sorted order (the reference takes `os.listdir` order, which is arbitrary), so sample
    numbers - and with them the pairs and the partitions - are the same on every machine;
  * `debugging=True` stops after the first array folder that yielded a sample.  The reference's flag is overwritten by every
    file it lists (:169-171), so whether it stops depends on whether the LAST file of a folder passed the filter;
  * a file whose rate is not `sr` is resampled only when asked: `Dataset(..., resample="kaiser_best")` (or "kaiser_fast",
    librosa's `res_type` names) converts it on the device (resample.py, csrc/resample.hip), one file at a time, in the
    reference's order - read, average, resample, cut, remove the mean; with the default resample=None `read_wav` raises for
    it (the reference goes through librosa, which always resamples).  There is no padding of short files: `read_wav` raises
    for a file shorter than `duration`, which librosa would pass on short, to fail later in `np.stack`;
  * `DataGenerator.on_epoch_end()` reshuffles with `random.Random` seeded from (seed, epoch count) instead of the unseeded
    global generator (:55-62), so two equal generators yield equal epochs.  `main_training.py` never calls it, `fit` does not
    either;
  * with `characteristics=True` the fourth item of a batch is `(room, wav_true)` of the TARGET positions - int32 indices into
    `evaluate.ROOMS` (-1: none of them) and the decoded waveforms - shaped for `Evaluator.update`, instead of the stacked file
    name fields (:95); `rir_generation.py:67-70` uses them for the same purpose;
  * `batch_size` is the GLOBAL batch (main_training.py:60, :78); replica `rank` of `world_size` receives rows
    [rank b / w, (rank + 1) b / w) of each global batch, the split `strategy.experimental_distribute_dataset` makes (:114).

Everything up to the index lists is host-only: `Dataset(..., device=None)` scans, parses and pairs without touching a GPU (and
without decoding a file), and a `DataGenerator` over it answers `len()` and `batch_indices()`.

Output tensors come from a ring of `DataGenerator.RING` = 3 slots per generator: batch i is overwritten by batch i + 3 of the
same generator.  A step has consumed its inputs when the next but one is assembled (all on one stream), so a training loop needs
no copy; a caller who keeps batches for longer than two further `__getitem__` calls, or reads them on another stream, clones
them (and, across streams, waits on an event).
"""
import os
import random
import wave
import zipfile

import numpy as np
import torch

from . import ops
from .evaluate import ROOMS
from .features import PreProcess
from .resample import PRESETS, resample as _resample
from .rooms import uts_room_embedding

__all__ = ["Dataset", "DataGenerator", "read_wav", "ALL_ROOMS", "ARRAYS"]

ALL_ROOMS = ["HemiAnechoicRoom", "LargeMeetingRoom", "MediumMeetingRoom", "ShoeBoxRoom", "SmallMeetingRoom"]      # dataset.py:34
ARRAYS = ["PlanarMicrophoneArray", "CircularMicrophoneArray"]                                                     # dataset.py:21
# get_embedding's lists (dataset.py:192-210) in the order index_in / index_out concatenate them (:174, :182)
_ROOM_LISTS = (("HemiAnechoicRoom", "index_hemi"), ("LargeMeetingRoom", "index_large"), ("MediumMeetingRoom", "index_medium"),
               ("SmallMeetingRoom", "index_small"), ("ShoeBoxRoom", "index_shoe"))
_UPLOAD_CHUNK = 512          # waveforms decoded, uploaded and transformed at a time (512 x 9600 floats = 19 MB)


def _pcm(raw, width, channels, path):
    """Interleaved little-endian PCM bytes -> fp32 [frames, channels] in [-1, 1): scaled by 2^-(bits-1)."""
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) * np.float32(2.0 ** -15)
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) << 8            # into the top three bytes: the sign bit lands in place
        x = (v >> 8).astype(np.float32) * np.float32(2.0 ** -23)
    elif width == 4:
        x = (np.frombuffer(raw, dtype="<i4").astype(np.float64) * 2.0 ** -31).astype(np.float32)
    else:
        raise ValueError(f"{path}: {8 * width}-bit PCM is not supported")
    return x.reshape(-1, channels)


def _read_float_wav(path, frames):
    """-> (rate, fp32 [frames(rate) at most, channels])"""
    try:
        from scipy.io import wavfile
    except ImportError:
        raise ValueError(f"{path}: not a PCM wav file, and scipy.io.wavfile is not available to read other formats") from None
    try:
        rate, data = wavfile.read(path)
    except Exception as e:          # scipy's own errors do not say which file
        raise ValueError(f"{path}: cannot be read as a wav file ({e})") from e
    data = data[:frames(rate)]
    if data.dtype.kind == "f":
        x = data.astype(np.float32)
    elif data.dtype.kind == "i":
        x = (data.astype(np.float64) * 2.0 ** -(8 * data.dtype.itemsize - 1)).astype(np.float32)
    else:
        raise ValueError(f"{path}: samples of type {data.dtype} are not supported")
    return rate, x.reshape(len(x), -1)


def read_wav(path, sample_rate, duration, mono=True, resample=None):
    """What `Loader.load` (preprocess.py:51-57) yields for this data set: the first int(duration * sample_rate) samples as fp32
    in [-1, 1), channels averaged when `mono`, then `signal -= np.mean(signal)` in fp32.  -> [T] (or [channels, T]).

    PCM 16 / 24 / 32 bit is decoded with the standard library; anything else goes through scipy.io.wavfile when it
    imports.  resample=None: a file whose rate is not `sample_rate` raises a ValueError naming it.  resample="kaiser_best" or
    "kaiser_fast" (librosa's `res_type`): such a file is read for `duration` seconds at its own rate, averaged when `mono` (else
    every channel for itself), resampled on the current CUDA device (`resample.Resampler`; a ValueError without one), cut to
    int(duration * sample_rate) samples, and the mean removed on the host as before - the reference's order.  A file at
    `sample_rate` takes the same path, bit for bit, whatever `resample` is; one that is shorter than `duration` raises either way."""
    if resample is not None and resample not in PRESETS:
        raise ValueError(f"read_wav: resample must be None or one of {sorted(PRESETS)}, not {resample!r}")
    frames = int(duration * sample_rate)
    try:
        with wave.open(path, "rb") as f:
            rate, channels, width, total = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
            want = frames if rate == sample_rate else int(duration * rate) if resample is not None else 0
            raw = f.readframes(min(want, total))
        x = _pcm(raw, width, channels, path) if want or rate == sample_rate else None
    except wave.Error:
        rate, x = _read_float_wav(path, lambda rate: frames if rate == sample_rate else int(duration * rate))
    if rate != sample_rate:
        if resample is None:
            raise ValueError(f"{path}: sample rate {rate} Hz, expected {sample_rate} Hz (pass resample='kaiser_best' or "
                             "'kaiser_fast' to convert it)")
        if x is None or x.shape[0] < 1:
            raise ValueError(f"{path}: no samples within {duration} s")
        x = _to_rate(x, rate, sample_rate, resample, mono, frames, path)
        if x.shape[0] < frames:
            raise ValueError(f"{path}: {x.shape[0]} samples after resampling from {rate} Hz, shorter than the {frames} that "
                             f"{duration} s at {sample_rate} Hz take")
    elif x.shape[0] < frames:
        raise ValueError(f"{path}: {x.shape[0]} samples, shorter than the {frames} that {duration} s at {sample_rate} Hz take")
    signal = x.mean(axis=1, dtype=np.float32) if mono else np.ascontiguousarray(x.T)
    signal -= np.mean(signal)
    return signal


def _to_rate(x, rate, sample_rate, res_type, mono, frames, path):
    """x fp32 [n, channels] at `rate` -> fp32 [min(frames, ceil(n L / M)), 1 or channels] at `sample_rate`: the channels averaged
    first when `mono` (librosa's order), one launch on the current CUDA device, the head of the result copied back."""
    if not torch.cuda.is_available():
        raise ValueError(f"{path}: sample rate {rate} Hz, expected {sample_rate} Hz, and resampling runs on a CUDA device: none is "
                         "available (there is no CPU path)")
    rows = x.mean(axis=1, dtype=np.float32)[None] if mono else np.ascontiguousarray(x.T)
    dev = torch.device("cuda", torch.cuda.current_device())
    y = _resample(torch.from_numpy(np.ascontiguousarray(rows)).to(dev), int(rate), int(sample_rate), res_type)
    return np.ascontiguousarray(y[:, :frames].cpu().numpy().T)


class Dataset:
    """dataset.py:11-244.  Host part: `files`, `Embeddings`, `characteristics`, the per-room lists, `index_in`, `index_out`.
    With `device`: `bank` fp32 [N, 2, H, W], `emb_bank` int32 [N, 16], `room_bank` int32 [N] (indices into `evaluate.ROOMS`,
    -1 for a room that is none of them) and, with `keep_waveforms`, `wav_bank` fp32 [N, T] (mean removed, as decoded)."""

    def __init__(self, dir_dataset, dataset_name, extract=False, normalization=True, debugging=False, room_characteristics=False,
                 room=None, array=None, *, device=None, keep_waveforms=False, n_fft=256, win_length=128, hop_length=64,
                 duration=0.2, sr=48000, input_shape=(144, 160), resample=None):
        if room is None:
            room = ["All"]
        self.array = list(ARRAYS) if array is None else array
        self.rooms = list(ALL_ROOMS) if room == ["All"] else room
        self.dir_dataset, self.dataset_name = dir_dataset, dataset_name
        self.n_fft, self.win_length, self.hop_length = n_fft, win_length, hop_length
        self.duration, self.sr, self.mono = duration, sr, True
        if resample is not None and resample not in PRESETS:
            raise ValueError(f"Dataset: resample must be None or one of {sorted(PRESETS)}, not {resample!r}")
        self.resample = resample
        self.input_shape = tuple(input_shape)
        self.normalization, self.debugging, self.room_characteristics = normalization, debugging, room_characteristics
        self.seed = 500          # dataset.py:76: one seed for the pairing and for the partitions

        self.files, self.Embeddings, self.characteristics = [], [], []
        self.index_ane = []      # never filled, as in the reference: AnechoicRoom files belong to no list
        for _, name in _ROOM_LISTS:
            setattr(self, name, [])
        self.index_in, self.index_out = [], []
        self.device = None
        self.bank = self.emb_bank = self.room_bank = self.wav_bank = None

        if extract:
            self.extract_files()
        self._scan()
        if device is not None:
            self._upload(torch.device(device), keep_waveforms)

    # ---- host part ------------------------------------------------------------------------------------
    def _root(self):
        return os.path.join(self.dir_dataset, self.dataset_name)

    def extract_files(self):
        """dataset.py:93-115: every .zip in a zone folder is unpacked into that folder and removed."""
        root = self._root()
        for room_folder in sorted(os.listdir(root)):
            room_path = os.path.join(root, room_folder)
            for zone_folder in sorted(os.listdir(room_path)):
                zone_path = os.path.join(room_path, zone_folder)
                for entry in sorted(os.listdir(zone_path)):
                    if entry.endswith(".zip"):
                        file_name = os.path.join(zone_path, entry)
                        with zipfile.ZipFile(file_name, "r") as z:
                            z.extractall(zone_path)
                        os.remove(file_name)

    def _scan(self):
        """load_data without the decoding (dataset.py:123-182): walk, filter, parse, information vectors, index lists."""
        root = self._root()
        lists = dict(_ROOM_LISTS)
        done = False
        for room_folder in sorted(os.listdir(root)):
            room_path = os.path.join(root, room_folder)
            if done or not os.path.isdir(room_path):
                continue
            for zone_folder in sorted(os.listdir(room_path)):
                zone_path = os.path.join(room_path, zone_folder)
                if done or not os.path.isdir(zone_path):
                    continue
                for array_folder in sorted(os.listdir(zone_path)):
                    array_path = os.path.join(zone_path, array_folder)
                    if done or not os.path.isdir(array_path):
                        continue
                    before = len(self.files)
                    for rir_file in sorted(os.listdir(array_path)):
                        c = rir_file.split("_")
                        if len(c) < 5 or not (c[0] in self.rooms and c[2] in self.array):
                            continue
                        c[1] = c[1].replace("Zone", "")
                        c[2] = c[2].replace("MicrophoneArray", "")
                        c[3] = c[3].replace("L", "")
                        c[4] = c[4].replace("M", "").replace(".wav", "")
                        index = len(self.files)
                        self.Embeddings.append(uts_room_embedding(c[0], c[1], c[2], c[3], c[4]))
                        if c[0] in lists:
                            getattr(self, lists[c[0]]).append(index)
                        self.files.append(os.path.join(array_path, rir_file))
                        self.characteristics.append(c[:5])
                    done = self.debugging and len(self.files) > before
        per_room = [getattr(self, name) for _, name in _ROOM_LISTS]
        self.index_in = [i for lst in per_room for i in lst]
        for lst in per_room:                                   # dataset.py:176-180: Python's generator, a fresh one per list
            random.Random(self.seed).shuffle(lst)
        self.index_out = [i for lst in per_room for i in lst]

    def waveform(self, index):
        """The decoded file of sample `index` (host, fp32 [T]): `read_wav` with the data set's rate, duration and `resample`."""
        return read_wav(self.files[index], self.sr, self.duration, self.mono, self.resample)

    def return_characteristics(self):
        return self.characteristics if self.room_characteristics else None

    def __len__(self):
        return len(self.files)

    # ---- device part ------------------------------------------------------------------------------------
    def _upload(self, device, keep_waveforms):
        if device.type != "cuda":
            raise ValueError("the feature bank lives on a GPU (device=None gives the host-only data set)")
        N, T = len(self.files), int(self.duration * self.sr)
        H, W = self.input_shape
        chunk = min(_UPLOAD_CHUNK, max(N, 1))
        need = N * (2 * H * W * 4 + 16 * 4 + 4) + (N * T * 4 if keep_waveforms else 0) + chunk * T * 4
        free, _ = torch.cuda.mem_get_info(device)
        if need > free:
            raise MemoryError(f"the data set needs {need / 2**30:.2f} GiB of device memory ({N} files, features {2 * H * W * 4} bytes"
                              f"{f' + waveform {T * 4} bytes' if keep_waveforms else ''} each), {free / 2**30:.2f} GiB are free on "
                              f"{device}; a bank larger than device memory is not supported")
        self.device = device
        self.bank = torch.empty((N, 2, H, W), dtype=torch.float32, device=device)
        self.emb_bank = torch.tensor(np.asarray(self.Embeddings, dtype=np.int32).reshape(N, 16), device=device)
        group = {r: i for i, r in enumerate(ROOMS)}
        self.room_bank = torch.tensor(np.asarray([group.get(c[0], -1) for c in self.characteristics], dtype=np.int32).reshape(N),
                                      device=device)
        self.wav_bank = torch.empty((N, T), dtype=torch.float32, device=device) if keep_waveforms else None
        pre = PreProcess(self.n_fft, self.win_length, self.hop_length, self.input_shape, remove_mean=False)
        with torch.cuda.device(device):
            for i0 in range(0, N, chunk):
                i1 = min(N, i0 + chunk)
                host = np.stack([self.waveform(i) for i in range(i0, i1)])
                wav = self.wav_bank[i0:i1] if keep_waveforms else torch.empty((i1 - i0, T), dtype=torch.float32, device=device)
                wav.copy_(torch.from_numpy(host))
                if self.normalization:          # the reference's chain in its order (dataset.py:214-223); the mean is already removed
                    pre(wav, out=self.bank[i0:i1])
                else:                           # :221: the raw amplitude / phase, padded
                    ops.stft_features(wav, self.bank[i0:i1], self.n_fft, self.win_length, self.hop_length, "reflect",
                                      remove_mean=False, normalize=False)

    def __getitem__(self, index):
        """-> (amp, phase, emb): views [H, W] of the sample's bank row and its information vector (a list of 16 ints)."""
        if self.bank is None:
            raise RuntimeError("this Dataset was built with device=None: it has no feature bank (see waveform())")
        return self.bank[index, 0], self.bank[index, 1], self.Embeddings[index]


class DataGenerator:
    """datageneratorv2.py:8-102 over a `Dataset`.  `gen[i]` -> (spec_in, emb, spec_out): fp32 [b, 2, H, W], int32 [b, 2, 16], fp32
    [b, 2, H, W] with b = batch_size / world_size, assembled by one kernel launch on the current stream; with
    `characteristics=True` a fourth item (room int32 [b], wav_true fp32 [b, T]) of the target positions (the data set needs
    `keep_waveforms=True`).  `batches(epoch)` is the iterable `fit` asks for."""

    RING = 3

    def __init__(self, dataset, batch_size=32, partition="train", shuffle=True, characteristics=False, *, rank=0, world_size=1):
        self.dataset, self.batch_size, self.partition, self.shuffle = dataset, int(batch_size), partition, shuffle
        self.characteristics = characteristics
        self.rank, self.world_size = int(rank), int(world_size)
        if self.batch_size <= 0 or self.world_size <= 0 or not 0 <= self.rank < self.world_size:
            raise ValueError("batch_size and world_size must be positive and 0 <= rank < world_size")
        if self.batch_size % self.world_size:
            raise ValueError(f"the global batch {self.batch_size} is not divisible by world_size {self.world_size}")
        self.local_batch = self.batch_size // self.world_size
        if characteristics and dataset.device is not None and dataset.wav_bank is None:
            raise ValueError("characteristics=True hands out the target waveforms: build the Dataset with keep_waveforms=True")

        temp = list(zip(dataset.index_in, dataset.index_out))          # :25-30
        random.Random(dataset.seed).shuffle(temp)
        n = len(temp)
        if partition == "train":                                        # :35-43
            temp = temp[:int(0.7 * n)]
        elif partition == "val":
            temp = temp[int(0.7 * n):int(0.9 * n)]
        elif partition == "test":
            temp = temp[int(0.9 * n):]
        else:
            raise ValueError("partition must be 'train', 'val' or 'test'")
        self.index_in = [p[0] for p in temp]
        self.index_out = [p[1] for p in temp]
        self.characteristics_list = dataset.return_characteristics()
        self._epochs = 0
        self._slots = [None] * self.RING
        self._next = 0
        self._table = None
        self._upload_table()

    def __len__(self):
        return len(self.index_in) // self.batch_size

    def batch_indices(self, idx):
        """(input sample numbers, target sample numbers) of this replica's rows of global batch `idx` (host lists)."""
        if not 0 <= idx < len(self):
            raise IndexError(f"batch {idx} of {len(self)}")
        lo = idx * self.batch_size + self.rank * self.local_batch
        return self.index_in[lo:lo + self.local_batch], self.index_out[lo:lo + self.local_batch]

    def _upload_table(self):
        """The epoch's index table int32 [2, len, local batch], range-checked here - the kernel trusts it - and uploaded once."""
        if self.dataset.device is None:
            return
        n = len(self)
        tab = np.zeros((2, n, self.local_batch), dtype=np.int32)
        for i in range(n):
            tab[0, i], tab[1, i] = self.batch_indices(i)
        if n and (tab.min() < 0 or tab.max() >= len(self.dataset)):
            raise IndexError("the index lists point outside the data set")
        self._table = torch.from_numpy(tab).to(self.dataset.device)      # a new tensor: launches in flight keep reading the old one

    def on_epoch_end(self):
        """:55-62, seeded: the pairs of the partition are reshuffled by random.Random(seed, epoch count) when `shuffle`."""
        if not self.shuffle:
            return
        self._epochs += 1
        temp = list(zip(self.index_in, self.index_out))
        random.Random(self.dataset.seed * 1000003 + self._epochs).shuffle(temp)
        self.index_in = [p[0] for p in temp]
        self.index_out = [p[1] for p in temp]
        self._upload_table()

    def _slot(self):
        ds, b = self.dataset, self.local_batch
        k = self._next % self.RING
        self._next += 1
        if self._slots[k] is None:
            shape = (b,) + tuple(ds.bank.shape[1:])
            s = {"spec_in": torch.empty(shape, dtype=torch.float32, device=ds.device),
                 "spec_out": torch.empty(shape, dtype=torch.float32, device=ds.device),
                 "emb": torch.empty((b, 2, ds.emb_bank.shape[1]), dtype=torch.int32, device=ds.device)}
            if self.characteristics:
                s["room"] = torch.empty((b,), dtype=torch.int32, device=ds.device)
                s["wav_true"] = torch.empty((b, ds.wav_bank.shape[1]), dtype=torch.float32, device=ds.device)
            self._slots[k] = s
        return self._slots[k]

    def __getitem__(self, idx):
        ds = self.dataset
        if ds.device is None:
            raise RuntimeError("the Dataset was built with device=None: there is no bank to gather from (see batch_indices())")
        if not 0 <= idx < len(self):
            raise IndexError(f"batch {idx} of {len(self)}")
        s = self._slot()
        with torch.cuda.device(ds.device):
            if self.characteristics:
                ops.gather_batch(ds.bank, ds.emb_bank, self._table[0, idx], self._table[1, idx], s["spec_in"], s["spec_out"], s["emb"],
                                 wav_bank=ds.wav_bank, room_bank=ds.room_bank, wav_true=s["wav_true"], room=s["room"])
                return s["spec_in"], s["emb"], s["spec_out"], (s["room"], s["wav_true"])
            ops.gather_batch(ds.bank, ds.emb_bank, self._table[0, idx], self._table[1, idx], s["spec_in"], s["spec_out"], s["emb"])
        return s["spec_in"], s["emb"], s["spec_out"]

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    def batches(self, epoch=None):
        """The iterable of an epoch, for `fit(trainer, train.batches, n_epochs, val.batches, ...)`."""
        return iter(self)

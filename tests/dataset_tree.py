"""A small impulse-response tree in the reference data set's layout, written with the standard library's `wave`:

    root/name/Room/ZoneX/YMicrophoneArray/Room_ZoneX_YMicrophoneArray_Ll_Mm.wav

Rooms HemiAnechoicRoom, SmallMeetingRoom and AnechoicRoom; zones A and B; both arrays; L1-L3, M1-M4: 48 files per room, 96 of
them in a room that has an index list, so the partitions hold 67 / 19 / 10 pairs.  Each file is 0.25 s of seeded, exponentially
decaying noise as PCM16 at 48 kHz; one file of the tree (STEREO) has two channels.  `make_single` writes a one-file tree, for
the files the loader must refuse (44.1 kHz, 0.1 s)."""
import os
import wave

import numpy as np

ROOMS = ("HemiAnechoicRoom", "SmallMeetingRoom", "AnechoicRoom")
ZONES = ("A", "B")
ARRAYS = ("PlanarMicrophoneArray", "CircularMicrophoneArray")
SPEAKERS = (1, 2, 3)
MICS = (1, 2, 3, 4)
RATE, SECONDS = 48000, 0.25
STEREO = ("SmallMeetingRoom", "B", "PlanarMicrophoneArray", 2, 3)
NAME = "room_impulse"


def file_name(room, zone, array, l, m):
    return f"{room}_Zone{zone}_{array}_L{l}_M{m}.wav"


def rel_path(room, zone, array, l, m):
    return os.path.join(room, f"Zone{zone}", array, file_name(room, zone, array, l, m))


def samples(seed, n, channels=1, rate=RATE):
    """int16 [n, channels]: white noise under exp(-t / 30 ms), peak about 0.6 of full scale, plus a small offset so that the
    mean removal has something to remove."""
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None] / rate
    x = rng.standard_normal((n, channels)) * 0.2 * np.exp(-t / 0.03) + 0.01
    return np.clip(np.round(x * 32767), -32768, 32767).astype("<i2")


def write_wav(path, data, rate, width=2):
    """data: integer array [frames, channels] already in the range of `width` bytes per sample (little endian, signed)."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = np.asarray(data)
    if width == 2:
        raw = data.astype("<i2").tobytes()
    elif width == 4:
        raw = data.astype("<i4").tobytes()
    elif width == 3:
        raw = data.astype("<i4").reshape(-1, 1).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    else:
        raise ValueError(width)
    with wave.open(path, "wb") as f:
        f.setnchannels(data.shape[1])
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(raw)


def positions():
    """Every position of the tree in the order a SORTED walk visits it."""
    out = []
    for room in sorted(ROOMS):
        for zone in sorted(ZONES):
            for array in sorted(ARRAYS):
                names = sorted((file_name(room, zone, array, l, m), l, m) for l in SPEAKERS for m in MICS)
                out += [(room, zone, array, l, m) for _, l, m in names]
    return out


def make_tree(root, name=NAME):
    """-> the positions in sorted-walk order.  The seed of a file is its number in that order."""
    pos = positions()
    n = int(RATE * SECONDS)
    for k, p in enumerate(pos):
        write_wav(os.path.join(root, name, rel_path(*p)), samples(1000 + k, n, 2 if p == STEREO else 1), RATE)
    return pos


def make_single(root, name, rate=RATE, seconds=SECONDS, room="HemiAnechoicRoom"):
    """A tree with one file; -> its path."""
    path = os.path.join(root, name, rel_path(room, "A", ARRAYS[0], 1, 1))
    write_wav(path, samples(7, int(rate * seconds), 1, rate), rate)
    return path

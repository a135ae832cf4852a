"""Host side of the data set classes (unet-rir_amd/dataset.py): the tree walk, the file-name fields, the index lists, the
pairing and the partitions against a restatement of the reference's list operations (dataset.py:147-182,
datageneratorv2.py:25-49), the wav loader, and the argument validation of the gather entry point.  No GPU."""
import ctypes as C
import os
import random
import zipfile

import numpy as np
import pytest

import dataset_tree as DT

THREE = list(DT.ROOMS)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("rir"))
    return root, DT.make_tree(root)


@pytest.fixture(scope="module")
def D():
    from unet_rir_amd import dataset
    return dataset


def fields(p):
    room, zone, array, l, m = p
    return [room, zone, array.replace("MicrophoneArray", ""), str(l), str(m)]


def restated_lists(chars, seed=500):
    """dataset.py:174-182 and :192-210 on the walk-ordered name fields: -> index_in, index_out."""
    order = ["HemiAnechoicRoom", "LargeMeetingRoom", "MediumMeetingRoom", "SmallMeetingRoom", "ShoeBoxRoom"]
    lists = {r: [] for r in order}
    for index, c in enumerate(chars):
        if c[0] in lists:
            lists[c[0]].append(index)
    index_in = sum((lists[r] for r in order), [])
    for r in order:
        random.Random(seed).shuffle(lists[r])
    index_out = sum((lists[r] for r in order), [])
    return index_in, index_out


def restated_partition(index_in, index_out, partition, seed=500):
    """datageneratorv2.py:25-43."""
    temp = list(zip(index_in, index_out))
    random.Random(seed).shuffle(temp)
    a, b = zip(*temp)
    a, b = list(a), list(b)
    n = len(a)
    cut = {"train": slice(None, int(0.7 * n)), "val": slice(int(0.7 * n), int(0.9 * n)), "test": slice(int(0.9 * n), None)}[partition]
    return a[cut], b[cut]


def test_walk_fields_and_filters(tree, D):
    root, pos = tree
    ds = D.Dataset(root, DT.NAME, room=THREE, room_characteristics=True)
    assert len(ds) == 144 and ds.device is None and ds.bank is None
    assert ds.files == [os.path.join(root, DT.NAME, DT.rel_path(*p)) for p in pos]          # sorted walk, sample number = position
    assert ds.return_characteristics() == [fields(p) for p in pos]
    assert D.Dataset(root, DT.NAME, room=THREE).return_characteristics() is None
    # room=None is ['All']: the five rooms that have an index list (dataset.py:33-34) - the anechoic room is not among them
    allr = D.Dataset(root, DT.NAME, room_characteristics=True)
    assert len(allr) == 96 and {c[0] for c in allr.return_characteristics()} == {"HemiAnechoicRoom", "SmallMeetingRoom"}
    planar = D.Dataset(root, DT.NAME, room=["SmallMeetingRoom"], array=["PlanarMicrophoneArray"], room_characteristics=True)
    assert len(planar) == 24 and {(c[0], c[2]) for c in planar.return_characteristics()} == {("SmallMeetingRoom", "Planar")}
    assert planar.files == [f for f, p in zip(ds.files, pos) if p[0] == "SmallMeetingRoom" and p[2] == "PlanarMicrophoneArray"]
    assert ds.seed == 500 and ds.sr == 48000 and ds.duration == 0.2 and ds.input_shape == (144, 160)
    with pytest.raises(RuntimeError):
        ds[0]                                                                               # no bank without a device


def test_debugging_stops_after_the_first_array_folder_with_a_sample(tree, D):
    root, pos = tree
    ds = D.Dataset(root, DT.NAME, debugging=True, room_characteristics=True)
    want = [fields(p) for p in pos if p[:3] == ("HemiAnechoicRoom", "A", "CircularMicrophoneArray")]
    assert len(want) == 12 and ds.return_characteristics() == want


def test_embeddings_and_room_lists(tree, D):
    from unet_rir_amd import rooms
    root, pos = tree
    ds = D.Dataset(root, DT.NAME, room=THREE)
    assert len(ds.Embeddings) == 144
    for p, e in zip(pos, ds.Embeddings):
        room, zone, array, l, m = p
        assert list(e) == rooms.uts_room_embedding(room, zone, array.replace("MicrophoneArray", ""), l, m)
    ane = {i for i, p in enumerate(pos) if p[0] == "AnechoicRoom"}
    assert len(ane) == 48                                                                   # loaded ...
    every = ds.index_ane + ds.index_hemi + ds.index_large + ds.index_medium + ds.index_shoe + ds.index_small
    assert not ane & set(every) and not ane & set(ds.index_in) and not ane & set(ds.index_out)      # ... but in no list
    assert sorted(ds.index_hemi) == [i for i, p in enumerate(pos) if p[0] == "HemiAnechoicRoom"]
    assert sorted(ds.index_small) == [i for i, p in enumerate(pos) if p[0] == "SmallMeetingRoom"]
    assert ds.index_large == ds.index_medium == ds.index_shoe == []


def test_index_lists_and_partitions_equal_the_restatement(tree, D):
    root, pos = tree
    ds = D.Dataset(root, DT.NAME, room=THREE)
    index_in, index_out = restated_lists([fields(p) for p in pos])
    assert len(index_in) == 96 and ds.index_in == index_in and ds.index_out == index_out
    assert index_in != index_out and sorted(index_in) == sorted(index_out)
    sizes = {}
    for part in ("train", "val", "test"):
        g = D.DataGenerator(ds, batch_size=4, partition=part)
        a, b = restated_partition(index_in, index_out, part)
        assert g.index_in == a and g.index_out == b
        assert all(pos[i][0] == pos[o][0] for i, o in zip(g.index_in, g.index_out))         # every pair within one room
        assert len(g) == len(a) // 4                                                        # datageneratorv2.py:45-49
        sizes[part] = len(a)
        for i in range(len(g)):
            assert g.batch_indices(i) == (a[4 * i:4 * i + 4], b[4 * i:4 * i + 4])
        with pytest.raises(IndexError):
            g.batch_indices(len(g))
        with pytest.raises(RuntimeError):
            g[0]                                                                            # host-only data set
    assert sizes == {"train": 67, "val": 19, "test": 10}
    assert len(D.DataGenerator(ds)) == 67 // 32                                             # default batch 32
    with pytest.raises(ValueError):
        D.DataGenerator(ds, partition="all")


def test_shards_concatenate_to_the_global_batch(tree, D):
    root, _ = tree
    ds = D.Dataset(root, DT.NAME, room=THREE)
    one = D.DataGenerator(ds, batch_size=8, partition="train")
    for w in (2, 4):
        shards = [D.DataGenerator(ds, batch_size=8, partition="train", rank=r, world_size=w) for r in range(w)]
        assert all(len(s) == len(one) and s.local_batch == 8 // w for s in shards)
        for i in range(len(one)):
            parts = [s.batch_indices(i) for s in shards]
            assert (sum((p[0] for p in parts), []), sum((p[1] for p in parts), [])) == one.batch_indices(i)
    with pytest.raises(ValueError, match="divisible"):
        D.DataGenerator(ds, batch_size=8, world_size=3)
    with pytest.raises(ValueError):
        D.DataGenerator(ds, batch_size=8, rank=2, world_size=2)


def test_on_epoch_end_is_seeded_and_obeys_shuffle(tree, D):
    root, _ = tree
    ds = D.Dataset(root, DT.NAME, room=THREE)
    a, b, fixed = (D.DataGenerator(ds, batch_size=4, shuffle=s) for s in (True, True, False))
    first = (list(a.index_in), list(a.index_out))
    for g in (a, b, fixed):
        g.on_epoch_end()
    assert (fixed.index_in, fixed.index_out) == first
    assert (a.index_in, a.index_out) != first and (a.index_in, a.index_out) == (b.index_in, b.index_out)
    assert sorted(zip(a.index_in, a.index_out)) == sorted(zip(*first))                      # the pairs stay pairs
    second = list(a.index_in)
    a.on_epoch_end()
    assert a.index_in != second


def test_extract_unpacks_zone_archives(tmp_path, D):
    src = DT.make_single(str(tmp_path / "src"), "x")
    zone = tmp_path / "data" / "set" / "HemiAnechoicRoom" / "ZoneA"
    zone.mkdir(parents=True)
    arc = zone / (DT.ARRAYS[0] + ".zip")
    with zipfile.ZipFile(arc, "w") as z:
        z.write(src, os.path.join(DT.ARRAYS[0], os.path.basename(src)))
    ds = D.Dataset(str(tmp_path / "data"), "set", extract=True)
    assert len(ds) == 1 and not arc.exists() and os.path.isfile(ds.files[0])
    assert ds.files[0] == str(zone / DT.ARRAYS[0] / os.path.basename(src))


def test_read_wav_scaling_truncation_mono_and_mean(tree, tmp_path, D):
    root, pos = tree
    k = pos.index(DT.STEREO)
    mono_k = 5
    assert pos[mono_k] != DT.STEREO
    raw = DT.samples(1000 + mono_k, 12000)                                                  # what the helper wrote: int16 [12000, 1]
    got = D.read_wav(os.path.join(root, DT.NAME, DT.rel_path(*pos[mono_k])), 48000, 0.2, True)
    assert got.dtype == np.float32 and got.shape == (9600,)                                 # int(0.2 * 48000) samples of the 12000
    x = raw[:9600, 0].astype(np.float32) * np.float32(2.0 ** -15)                           # scaled by 2^-(bits-1)
    x -= np.mean(x)                                                                         # preprocess.py:56, fp32
    assert np.array_equal(got, x)
    assert abs(float(got.astype(np.float64).mean())) < 1e-7 and float(np.abs(got).max()) > 0.1
    # the stereo file: channel mean first, then the mean removal
    raw2 = DT.samples(1000 + k, 12000, 2)
    got2 = D.read_wav(os.path.join(root, DT.NAME, DT.rel_path(*DT.STEREO)), 48000, 0.2, True)
    y = (raw2[:9600].astype(np.float32) * np.float32(2.0 ** -15)).mean(axis=1, dtype=np.float32)
    y -= np.mean(y)
    assert got2.shape == (9600,) and np.array_equal(got2, y)
    both = D.read_wav(os.path.join(root, DT.NAME, DT.rel_path(*DT.STEREO)), 48000, 0.2, False)
    assert both.shape == (2, 9600)
    # 24- and 32-bit PCM: the same waveform to the precision of the narrower format
    base = raw[:, :1].astype(np.int64)
    for width in (3, 4):
        p = str(tmp_path / f"w{width}" / "a.wav")
        DT.write_wav(p, base << (8 * (width - 2)), 48000, width)
        assert np.array_equal(D.read_wav(p, 48000, 0.2, True), got)
    p = str(tmp_path / "neg24" / "a.wav")
    DT.write_wav(p, np.array([[-(1 << 23)], [(1 << 23) - 1], [-1], [1]] * 2400, dtype=np.int64), 48000, 3)
    v = D.read_wav(p, 48000, 0.2, True)
    assert np.allclose(v[:4] - v[2], np.array([-1.0, 1.0 - 2.0 ** -23, -2.0 ** -23, 2.0 ** -23]) + 2.0 ** -23, atol=1e-7)


def test_read_wav_refuses_other_rates_and_short_files(tmp_path, D):
    p441 = DT.make_single(str(tmp_path), "r441", rate=44100)
    short = DT.make_single(str(tmp_path), "short", seconds=0.1)
    with pytest.raises(ValueError) as e:
        D.read_wav(p441, 48000, 0.2, True)
    assert p441 in str(e.value) and "44100" in str(e.value)
    with pytest.raises(ValueError) as e:
        D.read_wav(short, 48000, 0.2, True)
    assert short in str(e.value)
    # the data set's own accessor goes through the same loader
    ds = D.Dataset(str(tmp_path), "r441")
    assert len(ds) == 1
    with pytest.raises(ValueError, match="r441"):
        ds.waveform(0)


def _float_wav(path, data, rate):
    """IEEE-float wav (format tag 3), which the standard library's `wave` refuses."""
    import struct
    data = np.asarray(data, dtype="<f4")
    body = data.tobytes()
    fmt = struct.pack("<HHIIHH", 3, data.shape[1], rate, rate * data.shape[1] * 4, data.shape[1] * 4, 32)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt +
                b"data" + struct.pack("<I", len(body)) + body)


def test_read_wav_formats_beyond_pcm(tmp_path, D, monkeypatch):
    import sys
    x = (DT.samples(3, 12000, 2).astype(np.float32) * np.float32(2.0 ** -15))
    p = str(tmp_path / "f" / "float.wav")
    _float_wav(p, x, 48000)
    junk = str(tmp_path / "junk.wav")
    with open(junk, "wb") as f:
        f.write(b"this is not a wav file at all, whatever its name says" * 10)
    eight = str(tmp_path / "e" / "eight.wav")
    os.makedirs(os.path.dirname(eight))
    import wave
    with wave.open(eight, "wb") as f:
        f.setnchannels(1); f.setsampwidth(1); f.setframerate(48000); f.writeframes(bytes(12000))
    with pytest.raises(ValueError, match="eight.wav.*8-bit"):
        D.read_wav(eight, 48000, 0.2, True)
    try:
        import scipy.io.wavfile  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    if have_scipy:
        want = x[:9600].mean(axis=1, dtype=np.float32)
        want -= np.mean(want)
        got = D.read_wav(p, 48000, 0.2, True)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        with pytest.raises(ValueError, match="44100"):
            D.read_wav(p, 44100, 0.2, True)
        with pytest.raises(ValueError) as e:
            D.read_wav(junk, 48000, 0.2, True)                         # the reader's own error, with the file's name in front
        assert junk in str(e.value)
    # without scipy: the error names the file and says what is missing
    monkeypatch.setitem(sys.modules, "scipy.io", None)
    monkeypatch.setitem(sys.modules, "scipy", None)
    for path in (p, junk):
        with pytest.raises(ValueError) as e:
            D.read_wav(path, 48000, 0.2, True)
        assert path in str(e.value) and "scipy" in str(e.value)


def test_gather_entry_point_rejects_bad_geometry_without_a_gpu():
    """UNETRIR_EINVAL = 10001 before the device is touched; the pointers are made-up addresses that are never read."""
    import unet_rir_amd
    L = unet_rir_amd._lib.lib()
    f = L.unetrir_gather_batch_f32
    P = 4096                                     # any non-null value
    #            bank N  row emb L   wav T  room idx_in idx_out B spec_in spec_out emb wav_true room stream
    good = [P, 8, 64, P, 16, None, 0, None, P, P, 4, P, P, P, None, None, None]
    slot = {"bank": 0, "N": 1, "row_elems": 2, "emb_bank": 3, "wav_bank": 5, "wav_len": 6, "room_bank": 7, "idx_in": 8, "idx_out": 9,
            "B": 10, "spec_in": 11, "spec_out": 12, "emb": 13, "wav_true": 14, "room": 15}

    def call(**change):
        a = list(good)
        for k, v in change.items():
            a[slot[k]] = v
        return f(*a)

    for name in ("bank", "emb_bank", "idx_in", "idx_out", "spec_in", "spec_out", "emb"):
        assert call(**{name: None}) == 10001, name
    for name in ("B", "N", "row_elems"):
        for bad in (0, -1):
            assert call(**{name: bad}) == 10001, (name, bad)
    assert call(wav_true=P) == 10001                                     # wav_true without wav_bank
    assert call(wav_bank=P, wav_len=9600) == 10001                       # and the reverse
    assert call(room=P) == 10001                                         # room numbers without their bank
    assert "unetrir_gather_batch_f32" in unet_rir_amd._lib.EXPORTS
    assert C.sizeof(C.c_longlong) == 8

"""The device-resident data set on the GPU (unet-rir_amd/dataset.py, csrc/dataset.hip): the feature bank against the package's
own PreProcess (bit for bit) and the fp64 oracle, every batch of every partition against torch indexing of the banks, the
gather entry point on odd geometry between canaries, training from the generator against training from host-assembled
batches, the evaluator on the test partition, and the determinism of the epoch tables.

Tolerances against the oracle are those of tests/test_features_gpu.py (one fp32 rounding of an fp64 DFT: 2e-6 on the amplitude
plane, 2e-5 on the phase circle above the -100 dB floor and on the denormalised complex value)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dataset_tree as DT
from oracle import features as FO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THREE = list(DT.ROOMS)


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    return unet_rir_amd


@pytest.fixture(scope="module")
def data(U, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("rir"))
    pos = DT.make_tree(root)
    ds = U.Dataset(root, DT.NAME, room=THREE, room_characteristics=True, device=DEV, keep_waveforms=True)
    return root, pos, ds


def circ(a, b):
    d = np.abs(a - b) % 1.0
    return np.minimum(d, 1.0 - d)


def test_feature_bank(U, data):
    from unet_rir_amd import features as F
    from unet_rir_amd.evaluate import ROOMS
    root, pos, ds = data
    N = len(ds)
    assert N == 144
    assert ds.bank.shape == (N, 2, 144, 160) and ds.bank.dtype == torch.float32 and ds.bank.is_contiguous()
    assert ds.emb_bank.shape == (N, 16) and ds.emb_bank.dtype == torch.int32
    assert ds.room_bank.shape == (N,) and ds.room_bank.dtype == torch.int32
    assert ds.wav_bank.shape == (N, 9600) and ds.wav_bank.dtype == torch.float32
    waves = np.stack([ds.waveform(i) for i in range(N)])
    assert torch.equal(ds.wav_bank.cpu(), torch.from_numpy(waves))
    want = F.PreProcess(remove_mean=False)(torch.from_numpy(waves).to(DEV))
    assert torch.equal(ds.bank, want)                                                  # bit for bit, whatever the upload chunks were
    assert torch.equal(ds.emb_bank.cpu(), torch.tensor(ds.Embeddings, dtype=torch.int32))
    assert ds.room_bank.cpu().tolist() == [ROOMS.index(p[0]) if p[0] in ROOMS else -1 for p in pos]
    amp, phase, emb = ds[17]
    assert torch.equal(amp, ds.bank[17, 0]) and torch.equal(phase, ds.bank[17, 1]) and emb == ds.Embeddings[17]
    # the oracle, on a sample of the files (the stereo one among them)
    bank = ds.bank.cpu().numpy()
    nb, nf = 129, 151
    for i in sorted(set(range(0, N, 12)) | {pos.index(DT.STEREO)}):
        ref = FO.wav_to_feature(waves[i], remove_mean=False)
        got = bank[i]
        amp_err = float(np.abs(got[0] - ref[0]).max())
        loud = ref[0, :nb, :nf] > 0.05
        ph_err = float(circ(got[1, :nb, :nf], ref[1, :nb, :nf])[loud].max())
        a1, p1 = FO.denormalize(got[0, :nb, :nf].astype(np.float64), got[1, :nb, :nf].astype(np.float64))
        a2, p2 = FO.denormalize(ref[0, :nb, :nf].astype(np.float64), ref[1, :nb, :nf].astype(np.float64))
        c_err = float((np.abs(a1 * np.exp(1j * p1) - a2 * np.exp(1j * p2)) / (a2 + 128 * FO.EP)).max())
        print(f"sample {i}: amplitude {amp_err:.3g} phase {ph_err:.3g} complex {c_err:.3g}")
        assert amp_err <= 2e-6 and ph_err <= 2e-5 and c_err <= 2e-5
        assert not got[:, nb:, :].any() and not got[:, :, nf:].any()


def test_raw_bank_without_normalization(U, data):
    from unet_rir_amd import features as F
    root, _, _ = data
    ds = U.Dataset(root, DT.NAME, normalization=False, room=["SmallMeetingRoom"], array=["PlanarMicrophoneArray"], device=DEV)
    assert len(ds) == 24 and ds.wav_bank is None
    waves = torch.from_numpy(np.stack([ds.waveform(i) for i in range(24)])).to(DEV)
    amp, phase = F.FeatureExtractor(256, 128, 64).extract(waves)
    assert torch.equal(ds.bank[:, 0, :129, :151], amp) and torch.equal(ds.bank[:, 1, :129, :151], phase)
    assert not bool(ds.bank[:, :, 129:, :].any()) and not bool(ds.bank[:, :, :, 151:].any())
    assert float(amp.max()) > 1.0                                                      # raw STFT magnitudes, not the [0, 1] plane


def test_bank_larger_than_free_memory_is_refused(U, data, monkeypatch):
    root, _, _ = data
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1 << 20, 1 << 30))
    with pytest.raises(MemoryError, match="device memory"):
        U.Dataset(root, DT.NAME, device=DEV)


def expected(ds, ii, oo):
    ii, oo = torch.tensor(ii, device=DEV), torch.tensor(oo, device=DEV)
    return (ds.bank[ii], torch.stack((ds.emb_bank[ii], ds.emb_bank[oo]), dim=1), ds.bank[oo], ds.room_bank[oo], ds.wav_bank[oo])


def test_every_batch_of_every_partition(U, data):
    _, pos, ds = data
    for part, n in (("train", 67), ("val", 19), ("test", 10)):
        g = U.DataGenerator(ds, batch_size=4, partition=part, characteristics=True)
        assert len(g) == n // 4
        recent = []                                    # the previous two batches: (tensors, clones taken when they were handed out)
        count = 0
        for i, (spec_in, emb, spec_out, (room, wav_true)) in enumerate(g):
            ii, oo = g.batch_indices(i)
            w_in, w_emb, w_out, w_room, w_wav = expected(ds, ii, oo)
            assert torch.equal(spec_in, w_in) and torch.equal(spec_out, w_out) and torch.equal(emb, w_emb)
            assert torch.equal(room, w_room) and torch.equal(wav_true, w_wav)
            assert spec_in.shape == spec_out.shape == (4, 2, 144, 160) and emb.shape == (4, 2, 16)
            assert room.shape == (4,) and wav_true.shape == (4, 9600)
            assert spec_in.dtype == spec_out.dtype == wav_true.dtype == torch.float32 and emb.dtype == room.dtype == torch.int32
            assert all(t.is_contiguous() and t.device == ds.bank.device for t in (spec_in, emb, spec_out, room, wav_true))
            assert all(pos[a][0] == pos[b][0] for a, b in zip(ii, oo))
            now = (spec_in, emb, spec_out, room, wav_true)
            for old, kept in recent:                   # the ring: the previous two batches are other memory and still intact
                assert not {t.data_ptr() for t in old} & {t.data_ptr() for t in now}
                assert all(torch.equal(a, b) for a, b in zip(old, kept))
            recent = (recent + [(now, tuple(t.clone() for t in now))])[-2:]
            count += 1
        assert count == len(g)
        with pytest.raises(IndexError):
            g[len(g)]
    # without characteristics: the reference's triple; shards of a global batch are its rows
    g1 = U.DataGenerator(ds, batch_size=8, partition="train")
    shards = [U.DataGenerator(ds, batch_size=8, partition="train", rank=r, world_size=2) for r in range(2)]
    for i in range(len(g1)):
        whole = g1[i]
        assert len(whole) == 3
        parts = [s[i] for s in shards]
        for k in range(3):
            assert parts[0][k].shape[0] == 4 and torch.equal(torch.cat([p[k] for p in parts]), whole[k])
    with pytest.raises(ValueError, match="keep_waveforms"):
        U.DataGenerator(U.Dataset(data[0], DT.NAME, room=["SmallMeetingRoom"], device=DEV), characteristics=True)


GUARD = 1024          # floats / ints of canary on either side of every output


def guarded(n, dtype, shift):
    """A poisoned buffer [GUARD + shift | n | GUARD]: -> (whole buffer, payload view).  `shift` elements move the payload off
    the 16-byte boundary the allocator gives."""
    poison = float("nan") if dtype == torch.float32 else -0x5A5A5A5B
    whole = torch.full((GUARD + shift + n + GUARD,), poison, dtype=dtype, device=DEV)
    return whole, whole[GUARD + shift:GUARD + shift + n]


def untouched(whole, n, shift):
    head, tail = whole[:GUARD + shift], whole[GUARD + shift + n:]
    if whole.dtype == torch.float32:
        return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())
    return bool((head == -0x5A5A5A5B).all()) and bool((tail == -0x5A5A5A5B).all())


@pytest.mark.parametrize("row_shape,T,shift", [((2, 33, 37), 1000, 0),        # row_elems % 4 == 2: the 4-byte path, tails in both
                                               ((2, 33, 37), 1000, 1),        # and every buffer off the 16-byte boundary
                                               ((2, 32, 40), 1000, 3),        # divisible rows, misaligned bases: still 4 bytes
                                               ((2, 64, 33), 4100, 0),        # 16-byte path with a second, short piece (4224 = 4096 + 128)
                                               ((1, 1, 3), 1, 0)])            # rows shorter than a lane group
def test_odd_geometry_through_the_c_abi(U, row_shape, T, shift):
    L = U._lib.lib()
    N, B, E = 7, 5, 16
    row = int(np.prod(row_shape))
    g = torch.Generator().manual_seed(row + T + shift)
    hold = []

    def dev(t, s):               # a device copy whose base is `s` elements off the allocator's alignment
        buf = torch.empty(t.numel() + s, dtype=t.dtype, device=DEV)
        hold.append(buf)
        v = buf[s:].view(t.shape)
        v.copy_(t)
        return v

    bank = dev(torch.rand((N, row), generator=g), shift)
    emb_bank = dev(torch.randint(26, 1282, (N, E), generator=g, dtype=torch.int32), 0)
    wav_bank = dev(torch.rand((N, T), generator=g) - 0.5, shift)
    room_bank = dev(torch.randint(-1, 5, (N,), generator=g, dtype=torch.int32), 0)
    ii = torch.tensor([6, 0, 3, 3, 5], dtype=torch.int32, device=DEV)
    oo = torch.tensor([1, 6, 2, 4, 0], dtype=torch.int32, device=DEV)
    w_in, in_ = guarded(B * row, torch.float32, shift)
    w_out, out = guarded(B * row, torch.float32, shift)
    w_emb, emb = guarded(B * 2 * E, torch.int32, 0)
    w_wav, wav = guarded(B * T, torch.float32, shift)
    w_room, room = guarded(B, torch.int32, 0)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = L.unetrir_gather_batch_f32(p(bank), N, row, p(emb_bank), E, p(wav_bank), T, p(room_bank), p(ii), p(oo), B,
                                     p(in_), p(out), p(emb), p(wav), p(room), stream)
    assert err == 0
    torch.cuda.synchronize()
    li, lo = ii.long(), oo.long()
    assert torch.equal(in_.view(B, row), bank[li]) and torch.equal(out.view(B, row), bank[lo])
    assert torch.equal(emb.view(B, 2, E), torch.stack((emb_bank[li], emb_bank[lo]), dim=1))
    assert torch.equal(wav.view(B, T), wav_bank[lo]) and torch.equal(room, room_bank[lo])
    assert untouched(w_in, B * row, shift) and untouched(w_out, B * row, shift) and untouched(w_wav, B * T, shift)
    assert untouched(w_emb, B * 2 * E, 0) and untouched(w_room, B, 0)
    # the optional outputs left out: the three required ones are the same, nothing else is written
    in_.fill_(float("nan")); out.fill_(float("nan")); emb.fill_(0); wav.fill_(float("nan")); room.fill_(77)
    err = L.unetrir_gather_batch_f32(p(bank), N, row, p(emb_bank), E, None, 0, p(room_bank), p(ii), p(oo), B, p(in_), p(out), p(emb),
                                     None, None, stream)
    assert err == 0
    torch.cuda.synchronize()
    assert torch.equal(in_.view(B, row), bank[li]) and torch.equal(out.view(B, row), bank[lo])
    assert torch.equal(emb.view(B, 2, E), torch.stack((emb_bank[li], emb_bank[lo]), dim=1))
    assert bool(torch.isnan(wav).all()) and bool((room == 77).all())
    assert untouched(w_in, B * row, shift) and untouched(w_out, B * row, shift) and untouched(w_emb, B * 2 * E, 0)


def small_unet(U, batch):
    m = U.UNet((144, 160, 2), (2, 16), number_filters_0=8, kernels=3, batch_size=batch, device=DEV)
    m.engine.reset_parameters(generator=torch.Generator().manual_seed(11))
    return m


def host_batches(ds, gen, bank, emb):
    """DataGenerator.__getitem__ the reference's way (datageneratorv2.py:64-102): per-sample lists, np.stack, NHWC."""
    for idx in range(len(gen)):
        ii, oo = gen.batch_indices(idx)
        stft_in, phase_in, emb_in = [bank[i, 0] for i in ii], [bank[i, 1] for i in ii], [emb[i] for i in ii]
        stft_out, phase_out, emb_out = [bank[i, 0] for i in oo], [bank[i, 1] for i in oo], [emb[i] for i in oo]
        yield (np.stack((stft_in, phase_in), axis=-1).astype("float32"), np.stack((emb_in, emb_out), axis=1).astype("int32"),
               np.stack((stft_out, phase_out), axis=-1).astype("float32"))


def test_training_from_the_generator_equals_training_from_host_batches(U, data):
    _, _, ds = data
    bank, emb = ds.bank.cpu().numpy(), np.asarray(ds.Embeddings)
    train = U.DataGenerator(ds, batch_size=4, partition="train")
    val = U.DataGenerator(ds, batch_size=4, partition="val")
    assert len(train) == 16 and len(val) == 4
    runs = []
    for fed_by_generator in (True, False):
        m = small_unet(U, 4)
        tr = U.Trainer(m, lr=1e-3, dropout=True, dropout_seed=1234)
        if fed_by_generator:
            hist = U.fit(tr, train.batches, 2, val.batches, log=None)
        else:
            hist = U.fit(tr, lambda ep: U.DeviceBatchPipeline(host_batches(ds, train, bank, emb), DEV), 2,
                         lambda ep: U.DeviceBatchPipeline(host_batches(ds, val, bank, emb), DEV), log=None)
        torch.cuda.synchronize()
        eng = tr.engine
        runs.append((hist, eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), {k: v.clone() for k, v in eng.moving.items()}))
    (h1, t1, m1, v1, mv1), (h2, t2, m2, v2, mv2) = runs
    assert len(h1) == 2 and h1 == h2                                   # every figure of every record, as floats
    assert all(np.isfinite(h[k]) for h in h1 for k in ("train_loss", "train_amp", "train_phase", "val_loss", "val_amp", "val_phase"))
    assert torch.equal(t1, t2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    assert all(torch.equal(mv1[k], mv2[k]) for k in mv1)
    assert h1[0]["train_loss"] != h1[1]["train_loss"]                  # it did train


def test_evaluator_on_the_test_partition(U, data):
    from unet_rir_amd.evaluate import METRICS, ROOMS
    _, pos, ds = data
    gen = U.DataGenerator(ds, batch_size=4, partition="test", shuffle=False, characteristics=True)      # rir_generation.py:67-70
    ev = U.Evaluator(small_unet(U, 4))
    targets = []
    for i, (spec_in, emb, spec_out, (room, wav_true)) in enumerate(gen):
        ev.update(spec_in, emb, spec_out, wav_true, room)
        targets += gen.batch_indices(i)[1]
    res = ev.result()
    assert res["n"][0] == (10 // 4) * 4 == len(targets)
    assert res["n"][1:] == [sum(pos[t][0] == r for t in targets) for r in ROOMS]
    assert all(np.isfinite(res[m][0]) for m in METRICS)
    for k, r in enumerate(ROOMS):
        if res["n"][1 + k]:
            assert all(np.isfinite(res[m][1 + k]) for m in METRICS), r


def test_epoch_tables_are_deterministic(U, data):
    _, _, ds = data
    a, b = (U.DataGenerator(ds, batch_size=4, partition="train", shuffle=True) for _ in range(2))
    fixed = U.DataGenerator(ds, batch_size=4, partition="train", shuffle=False)
    epoch0 = [tuple(t.clone() for t in batch) for batch in a]
    for x, y in zip(epoch0, fixed):
        assert all(torch.equal(p, q) for p, q in zip(x, y))            # the first epoch does not depend on `shuffle`
    for g in (a, b, fixed):
        g.on_epoch_end()
    for x, y in zip(epoch0, fixed):
        assert all(torch.equal(p, q) for p, q in zip(x, y))            # shuffle=False: the same order again
    epoch1 = [tuple(t.clone() for t in batch) for batch in a]
    assert len(epoch1) == len(epoch0) == 16
    assert any(not torch.equal(x[0], y[0]) for x, y in zip(epoch0, epoch1))        # shuffle=True: another order
    for i, (x, y) in enumerate(zip(epoch1, b)):
        assert all(torch.equal(p, q) for p, q in zip(x, y))            # equal arguments, equal epochs
        ii, oo = a.batch_indices(i)
        assert torch.equal(x[0], ds.bank[torch.tensor(ii, device=DEV)]) and torch.equal(x[2], ds.bank[torch.tensor(oo, device=DEV)])


def run_script(monkeypatch, name, argv):
    """main() of scripts/<name>.py with `argv`, in this process."""
    import importlib.util
    import os
    import sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", name + ".py")
    spec = importlib.util.spec_from_file_location("script_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", [path] + [str(a) for a in argv])
    mod.main()


@pytest.mark.parametrize("name,extra", [("unet", ["--filters", 8]), ("resae", []), ("vae", [])])
def test_train_script_trains_resumes_and_is_scored(U, data, tmp_path, monkeypatch, name, extra):
    """scripts/train.py on the tree: three epochs, then a second call that continues from the latest checkpoint; for the
    models scripts/evaluate.py can rebuild from a checkpoint, --dataset scores the test partition and writes the reports."""
    import json
    import os
    root = data[0]
    out = str(tmp_path / "ckpt")
    common = ["--dataset", root, DT.NAME, "--rooms", "HemiAnechoicRoom", "SmallMeetingRoom", "--no-debug", "--name", name, "--batch", 4,
              "--lr", 1e-4, "--out", out] + extra
    run_script(monkeypatch, "train", common + ["--epochs", 3])
    hist = json.load(open(os.path.join(out, "history.json")))
    assert [h["epoch"] for h in hist] == [1, 2, 3] and all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in hist)
    assert sorted(f for f in os.listdir(out) if f.endswith(".pt")) == ["ckpt-1.pt", "ckpt-2.pt"]      # epochs 0 and 2 (:363-364)
    run_script(monkeypatch, "train", common + ["--epochs", 5])
    again = json.load(open(os.path.join(out, "history.json")))
    assert [h["epoch"] for h in again] == [4, 5]                       # restored after epoch 3, not started over
    assert all(np.isfinite(h["train_loss"]) for h in again)
    if name == "resae":                                                # evaluate.py rebuilds a U-Net or a VAE from a checkpoint
        return
    rep = str(tmp_path / "report")
    args = ["--checkpoint", out, "--arch", name, "--dataset", root, DT.NAME, "--rooms", "HemiAnechoicRoom", "SmallMeetingRoom",
            "--batch", 4, "--out", rep, "--name", name] + (["--filters", 8] if name == "unet" else ["--latent", 64])
    run_script(monkeypatch, "evaluate", args)
    assert sorted(os.listdir(rep)) == sorted(f"{name}_{s}" for s in ("losses.csv", "infer_time.csv", "results_inference.txt"))
    rows = open(os.path.join(rep, f"{name}_losses.csv")).read().splitlines()
    assert rows[1].split(",")[:2] == ["Global", "8"]                   # 10 test pairs, two whole batches of 4

"""Generates tests/golden/loss_chain.json: what `Trainer` and `fit` launch behind the loss kernel, and which keys a `fit` record
carries, for every combination of the terms on the waveform - recorded before the terms were given one base and the trainer one chain,
so that tests/test_loss_chain_sim.py can hold the code to it.  Strings only: exact, and the same on every machine.

Everything runs on the simulated runtime (tests/sim_runtime.py) with the kernels' CPU stand-ins (tests/spectral_loss_fft_cpu_ops.py,
which installs the wave, decay and both spectral stand-ins beneath it).  Per configuration

    wave_loss in {none, set}  x  decay_loss in {none, set}  x  spectral_loss in {none, "dft", "fft"}

and per engine ("unet" and "ae" of tests/test_schedule_sim.py's `_build`):
    step      the op names one `Trainer.step` launches, from the loss kernel up to and including the first kernel of the backward pass
    val       the op names one validation batch of `fit` launches, from the loss kernel to the end of the batch
    keys      the sorted keys of the `fit` record without `val_batches`
    keys_val  the same with `val_batches`
The geometry and batch are those of tests/test_wave_loss_sim.py (T = 48; the DFT form looks at it through the resolutions of
tests/test_spectral_loss_sim.py).  The FFT form's smallest transform needs 65 samples, so its configurations take the geometry (T = 96),
batch and resolutions of tests/test_spectral_loss_fft_sim.py.

"engines" holds the two key sets for a VAE, a VQ-VAE and the classifier (the builders of tests/test_vae_sim.py, test_vqvae_sim.py and
test_cnn_clas_sim.py): the engines with a metric of their own.

    python tests/golden/make_loss_chain_golden.py
"""
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:          # run as a script (under pytest, tests/conftest.py has put ROOT there)
        sys.path.insert(0, p)

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "loss_chain.json")

CONFIGS = list(itertools.product((False, True), (False, True), (None, "dft", "fft")))       # (wave, decay, spectral)
KINDS = ("unet", "ae")
LOSS_KERNEL = "sigmoid_loss"


def config_name(wave, decay, spectral):
    return f"wave={int(wave)},decay={int(decay)},spectral={spectral or 'none'}"


def is_backward(what):
    """a kernel of the engine's backward pass (the adjoint of `PostProcess` runs in front of it and is not one)"""
    return "wgrad" in what or "dgrad" in what or (what.endswith("_bwd") and what != "istft_features_bwd")


def install(monkeypatch):
    import spectral_loss_fft_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    return rt, spectral_loss_fft_cpu_ops.install(monkeypatch, rt)


def logged(monkeypatch, rt):
    """the `what` of every launch reported to the runtime from here on"""
    log, touch = [], rt.touch

    def touch_and_log(reads=(), writes=(), what="", stream=None):
        log.append(what)
        return touch(reads, writes, what, stream)
    monkeypatch.setattr(rt, "touch", touch_and_log)
    return log


def setup(spectral):
    """(geometry, batch, resolutions) of a configuration"""
    import test_spectral_loss_fft_sim as FS
    import test_spectral_loss_sim as PS
    import test_wave_loss_sim as WS
    if spectral == "fft":
        return FS.GEO, FS._batch(), FS.RES
    return WS.GEO, WS._batch(), PS.RES


def terms(wave, decay, spectral):
    """the keyword arguments of `Trainer` for a configuration"""
    import unet_rir_amd as U
    geo, _, res = setup(spectral)
    kw = {}
    if wave:
        kw["wave_loss"] = U.WaveLoss(weight=0.3, norm="energy", **geo)
    if decay:
        kw["decay_loss"] = U.DecayLoss(weight=0.05, floor_db=30.0, **geo)
    if spectral:
        kw["spectral_loss"] = U.SpectralLoss(weight=0.05, resolutions=res, sc_weight=0.8, log_weight=1.3, floor_db=30.0, method=spectral, **geo)
    return kw


def build(rt, kind, wave, decay, spectral, lr=0.0, **kw):
    import test_schedule_sim as SS
    import test_wave_loss_sim as WS
    import unet_rir_amd as U
    _, eng, _ = SS._build(rt, WS.B, False, world=1, bucket_bytes=8192, kind=kind)
    return eng, U.Trainer(eng, lr=lr, dropout=False, bucket_bytes=8192, **terms(wave, decay, spectral), **kw)


def batch_of(wave, decay, spectral):
    """three inputs, and the target waveforms where a term needs them"""
    spec_in, emb, spec_out, wav = setup(spectral)[1]
    return (spec_in, emb, spec_out, wav) if (wave or decay or spectral) else (spec_in, emb, spec_out)


def step_span(log):
    i = log.index(LOSS_KERNEL)
    j = next(k for k in range(i + 1, len(log)) if is_backward(log[k]))
    return log[i:j + 1]


def record_config(monkeypatch, rt, kind, wave, decay, spectral):
    import unet_rir_amd as U
    eng, tr = build(rt, kind, wave, decay, spectral)
    batch = batch_of(wave, decay, spectral)
    log = logged(monkeypatch, rt)
    tr.step(*batch[:3], wav_true=batch[3] if len(batch) == 4 else None)
    out = {"step": step_span(list(log))}
    out["keys"] = sorted(U.fit(tr, lambda ep: [batch], 1, log=None)[0])
    mark = []

    def val(ep):
        mark.append(len(log))
        return [batch]
    rec = U.fit(tr, lambda ep: [batch], 1, val_batches=val, log=None)[0]
    tail = list(log)[mark[0]:]
    out["val"] = tail[tail.index(LOSS_KERNEL):]
    out["keys_val"] = sorted(rec)
    return out


def _key_sets(tr, batch):
    import unet_rir_amd as U
    return {"keys": sorted(U.fit(tr, lambda ep: [batch], 1, log=None)[0]),
            "keys_val": sorted(U.fit(tr, lambda ep: [batch], 1, val_batches=lambda ep: [batch], log=None)[0])}


def record_engines(monkeypatch):
    """the key sets of the engines with a metric of their own"""
    import cnn_clas_cpu_ops
    import test_cnn_clas_sim as CS
    import test_vae_sim as VS
    import test_vqvae_sim as QS
    import vae_cpu_ops
    from oracle import torch_ref as R
    from sim_runtime import SimRuntime
    out = {}
    rt = SimRuntime()
    vae_cpu_ops.install(monkeypatch, rt)
    _, _, _, tr = VS._build(rt, 2, False, lr=0.0)
    out["vae"] = _key_sets(tr, tuple(torch.tensor(a) for a in R.synthetic_batch(R.Config(VS.H, VS.W), 2)))
    rt, _ = QS._install(monkeypatch)
    _, _, _, tr = QS._build(rt, 2, False, lr=0.0)
    out["vqvae"] = _key_sets(tr, tuple(torch.tensor(a) for a in QS._batch(2)))
    rt = SimRuntime()
    cnn_clas_cpu_ops.install(monkeypatch, rt)
    cfg, params, (x, y, _) = CS._setup(True)
    _, tr = CS._build(rt, cfg, params, lr=0.0)
    out["cnn_clas"] = _key_sets(tr, (torch.tensor(x), None, torch.tensor(y)))
    return out


def record(configs=CONFIGS, kinds=KINDS, engines=True):
    doc = {"configs": {}}
    for wave, decay, spectral in configs:
        entry = doc["configs"][config_name(wave, decay, spectral)] = {}
        for kind in kinds:
            mp = pytest.MonkeyPatch()
            try:
                rt, _ = install(mp)
                entry[kind] = record_config(mp, rt, kind, wave, decay, spectral)
            finally:
                mp.undo()
    if engines:
        mp = pytest.MonkeyPatch()
        try:
            doc["engines"] = record_engines(mp)
        finally:
            mp.undo()
    return doc


if __name__ == "__main__":
    doc = record()
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(doc['configs'])} configurations x {len(KINDS)} engines, {len(doc['engines'])} engines with a metric", file=sys.stderr)

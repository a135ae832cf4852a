"""The terms on the waveform share one base (unet_rir_amd/waveterm.py) and the trainer runs them through one chain
(`Trainer._waveform_terms`); `fit` keeps its means in meters.  On the simulated runtime with the kernels' CPU stand-ins, for every
combination of wave_loss, decay_loss and spectral_loss ("dft" / "fft"):

  * what a step and a validation batch launch behind the loss kernel, and the keys of the `fit` records, are those recorded in
    tests/golden/loss_chain.json before the chain existed (tests/golden/make_loss_chain_golden.py), exactly;
  * the second pass through `_step_body` - the one a HIP graph capture records - moves no buffer of any loss object;
  * the values of the records are the means `fit`'s docstring defines, formed here from the counters copied after every batch;
  * a `DecayLoss` / `SpectralLoss` called on its own returns what its docstring says.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_loss_chain_golden", os.path.join(GOLDEN, "make_loss_chain_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _generator()
WITH_A_TERM = [c for c in G.CONFIGS if any(c)]
_id = lambda c: G.config_name(*c)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "loss_chain.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("config", G.CONFIGS, ids=_id)
def test_launches_and_record_keys_are_the_recorded_ones(golden, config):
    name = G.config_name(*config)
    got = G.record(configs=[config], engines=False)["configs"][name]
    assert got == golden["configs"][name]


def test_the_recording_covers_every_configuration_and_the_table_of_the_issue(golden):
    assert sorted(golden["configs"]) == sorted(G.config_name(*c) for c in G.CONFIGS) and len(G.CONFIGS) == 12
    for wave, decay, spectral in G.CONFIGS:
        op = {None: [], "dft": ["spectral_loss"], "fft": ["spectral_loss_fft"]}[spectral]
        terms = (["decay_loss"] if decay else []) + op
        chain = (["wave_loss"] if (wave or terms) else []) + terms
        for kind in G.KINDS:
            rec = golden["configs"][G.config_name(wave, decay, spectral)][kind]
            assert rec["step"][:-1] == ["sigmoid_loss"] + chain + (["istft_features_bwd"] if terms else [])
            assert rec["val"] == ["sigmoid_loss"] + chain


def test_record_keys_of_the_engines_with_a_metric_of_their_own(golden, monkeypatch):
    assert G.record_engines(monkeypatch) == golden["engines"]


def _buffers(tr):
    """the address of every buffer of every loss object of a trainer"""
    ptr = lambda t: None if t is None else t.data_ptr()
    w = tr._wave
    out = [ptr(w._ws.buf), ptr(w._dpred), ptr(w.wav_pred), ptr(w.wave_out)]
    for t in (tr.decay_loss, tr.spectral_loss):
        if t is not None:
            out += [ptr(t._ws.buf), ptr(t._dwav), ptr(t._dpred), ptr(t.out)]
    return out


@pytest.mark.parametrize("config", WITH_A_TERM, ids=_id)
def test_the_second_pass_through_the_step_body_moves_no_buffer(monkeypatch, config):
    rt, _ = G.install(monkeypatch)
    eng, tr = G.build(rt, "unet", *config, lr=1e-3, graph=True)
    assert tr.use_graph
    spec_in, emb, spec_out, wav = G.batch_of(*config)
    prepared = [(t._ws.buf.data_ptr(), t._dwav.data_ptr(), t.out.data_ptr()) for t in tr._terms]       # from `prepare` at construction
    tr._step_body(spec_in, emb, spec_out, None, True, wav)              # the ordinary pass
    first = _buffers(tr)
    assert [(t._ws.buf.data_ptr(), t._dwav.data_ptr(), t.out.data_ptr()) for t in tr._terms] == prepared
    assert first[0] is not None and first[1] is not None and first[3] is not None and (first[2] is not None) == bool(tr._terms)
    tr._step_body(spec_in, emb, spec_out, None, True, wav)              # the pass a capture records
    assert _buffers(tr) == first


# ---- the values of the records

def _close(got, want):
    """1e-12 relative: the sums are a handful of fp64 additions; a wrong denominator or a swapped row is off by a factor"""
    return abs(got - want) <= 1e-12 * abs(want)


def _fit_and_watch(monkeypatch, tr, counters, train, val):
    """One epoch of `fit`; -> (record, {"train": [...], "val": [...]}: what `counters()` held after every batch).  A training batch ends
    with `trainer.step`; a validation batch ends when `fit` asks for the next one (its counters are written by the forward pass and by
    the chain behind it, so a copy behind the forward pass alone would be one batch late for the terms on the waveform)."""
    import unet_rir_amd as U
    seen = {"train": [], "val": []}
    step = tr.step

    def watched_step(*a, **k):
        out = step(*a, **k)
        seen["train"].append(counters())
        return out
    monkeypatch.setattr(tr, "step", watched_step)

    def watched_val(ep):
        for b in val:
            yield b
            seen["val"].append(counters())
    rec = U.fit(tr, lambda ep: train, 1, val_batches=watched_val, log=None)[0]
    assert len(seen["train"]) == len(train) and len(seen["val"]) == len(val)
    return rec, seen


@pytest.mark.parametrize("config", WITH_A_TERM, ids=_id)
def test_record_values_are_the_means_of_the_counters(monkeypatch, config):
    wave, decay, spectral = config
    rt, _ = G.install(monkeypatch)
    eng, tr = G.build(rt, "unet", *config, lr=0.0)
    spec_in, emb, spec_out, wav = G.batch_of(*config)
    B = wav.shape[0]
    quiet = wav.clone()
    quiet[1] = 0.0                                           # a silent target: the samples counted differ from B
    train, val = [(spec_in, emb, spec_out, wav), (spec_in, emb, spec_out, quiet)], [(spec_in, emb, spec_out, (torch.zeros(B), wav))]

    def counters():
        return {k: getattr(t, k).clone().numpy() for k, t in (("wave_out", tr.wave_loss), ("decay_out", tr.decay_loss),
                                                               ("spectral_out", tr.spectral_loss)) if t is not None}
    rec, seen = _fit_and_watch(monkeypatch, tr, counters, train, val)
    for part, rows in seen.items():
        total = lambda k: np.sum([r[k] for r in rows], axis=0)
        if wave:                                             # the sum of E_b / D_b over steps x batch size x replicas
            assert _close(rec[f"{part}_wave"], total("wave_out")[0] / (len(rows) * B * 1))
        if decay:                                            # the sum of Q_b over max(samples counted, 1)
            assert _close(rec[f"{part}_decay"], total("decay_out")[0] / max(total("decay_out")[1], 1.0))
        if spectral:
            s = total("spectral_out")
            assert _close(rec[f"{part}_sc"], s[0] / max(s[2], 1.0)) and _close(rec[f"{part}_logmag"], s[1] / max(s[2], 1.0))
    # the two rows are told apart, and the silent sample is left out of the count
    if decay:
        assert [r["decay_out"][1] for r in seen["train"]] == [B, B - 1] and rec["train_decay"] != rec["val_decay"]
    if spectral:
        assert [r["spectral_out"][2] for r in seen["train"]] == [B, B - 1] and rec["train_sc"] != rec["val_sc"]
    if wave:
        assert rec["train_wave"] != rec["val_wave"] and rec["train_wave"] > 0


def test_record_values_of_the_vae(monkeypatch):
    import test_vae_sim as VS
    import vae_cpu_ops
    from oracle import torch_ref as R
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    vae_cpu_ops.install(monkeypatch, rt)
    B = 2
    _, _, eng, tr = VS._build(rt, B, False, lr=0.0)
    six = [torch.tensor(a) for a in R.synthetic_batch(R.Config(VS.H, VS.W), 3 * B)]
    batches = [tuple(a[i * B:(i + 1) * B].contiguous() for a in six) for i in range(3)]
    rec, seen = _fit_and_watch(monkeypatch, tr, lambda: float(eng.kl_out[1]), batches[:2], batches[2:])
    for part, rows in seen.items():                          # the raw KL sums over steps x elements per step x replicas
        assert _close(rec[f"{part}_kl"], sum(rows) / (len(rows) * eng.kl_elems * 1)) and rec[f"{part}_kl"] > 0
    assert len(set(seen["train"] + seen["val"])) == 3 and rec["train_kl"] != rec["val_kl"]          # three batches, three KL sums


def test_record_values_of_the_classifier(monkeypatch):
    import cnn_clas_ref as A
    import test_cnn_clas_sim as CS
    rt, _ = CS._install(monkeypatch)
    cfg, params, _ = CS._setup(True)
    eng, tr = CS._build(rt, cfg, params, lr=0.0)
    batches = [tuple(None if a is None else torch.tensor(a) for a in (x, None, y))
               for x, y, _ in (A.synthetic_batch(cfg, CS.B, f"sim/{tag}") for tag in ("fit0", "fit1", "val"))]
    rec, seen = _fit_and_watch(monkeypatch, tr, lambda: float(eng.acc_out[0]), batches[:2], batches[2:])
    for part, rows in seen.items():                          # correct rows over steps x batch size x replicas
        want = sum(rows) / (len(rows) * CS.B * 1)
        assert rec[f"{part}_acc"] == want if want == 0 else _close(rec[f"{part}_acc"], want)


# ---- a term called on its own

def _term(which):
    import test_spectral_loss_fft_sim as FS
    import test_spectral_loss_sim as PS
    import unet_rir_amd as U
    if which == "decay":
        return U.DecayLoss(weight=0.05, floor_db=30.0, **FS.GEO)
    return U.SpectralLoss(weight=0.05, resolutions=FS.RES if which == "fft" else PS.RES, floor_db=30.0, method=which, **FS.GEO)


@pytest.mark.parametrize("which", ["decay", "dft", "fft"])
def test_a_term_called_on_its_own(monkeypatch, which):
    import test_spectral_loss_fft_sim as FS
    rt, _ = G.install(monkeypatch)
    term = _term(which)
    gen = torch.Generator().manual_seed(5)
    decay = torch.exp(-torch.arange(FS.T, dtype=torch.float32) / 12.0)
    wav_pred, wav_true = (torch.randn((FS.B, FS.T), generator=gen) * decay for _ in range(2))
    pred = torch.rand((FS.B, 2, 16, 16), generator=gen)
    log = G.logged(monkeypatch, rt)
    own = term(wav_pred, wav_true)
    assert own is term._dwav and tuple(own.shape) == (FS.B, FS.T) and float(own.abs().max()) > 0 and "istft_features_bwd" not in log
    assert term(wav_pred, wav_true, pred=pred) is term._dpred and tuple(term._dpred.shape) == tuple(pred.shape)
    assert log.count("istft_features_bwd") == 1
    given = torch.zeros_like(pred)
    assert term(wav_pred, wav_true, pred=pred, dpred=given) is given and torch.equal(given, term._dpred)
    assert term(wav_pred, wav_true, pred=pred, dpred=given, accumulate=True) is given
    with pytest.raises(ValueError, match="accumulate=True adds to a dpred the caller gives"):
        term(wav_pred, wav_true, pred=pred, accumulate=True)
    del log[:]
    assert term(wav_pred, wav_true, pred=pred, backward=False) is None and "istft_features_bwd" not in log and len(log) == 1
    buf = torch.ones_like(wav_pred)
    if which == "decay":
        with pytest.raises(ValueError, match="cannot add"):
            term(wav_pred, wav_true, dwav=buf)
        assert torch.equal(buf, torch.ones_like(buf))
    else:
        kept = own.clone()
        assert term(wav_pred, wav_true, dwav=buf) is buf and torch.equal(term._dwav, kept)       # its own buffer is left alone
        # fl32(1 + g) against 1 + fl32(g): half an ulp of each
        assert float((buf - 1.0 - kept).abs().max()) <= 2.0 ** -23 * (1.0 + float(kept.abs().max()))

"""The kernel plan of the bf16 convolutions (plan_conv, api.hip) gives the answers the library gave before it existed: which kernel
serves each convolution layer of the benchmarked workloads and how many rows of fused column statistics it reports, under the
default switches, under each dispatch switch set to 0 on its own and with conv3x3g_pair = 2 (tests/golden/conv_dispatch.json,
recorded by tests/golden/make_conv_dispatch_golden.py).  The weight-gradient workspace query, computed from the weight-gradient
plans (plan_wgrad), keeps the values the library gave before they existed (tests/golden/wgrad_ws.json, same generator).  The
library loads without a GPU; no compute calls here."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_conv_dispatch_golden", os.path.join(GOLDEN, "make_conv_dispatch_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def expected(setting, layer, default, rec):
    """The recorded answer, except where the recording contradicted the launch it describes:
    - conv3x3g = 0 on a layer of the paired tile: the launch falls through to conv3x3r (N > 64: the <2, 2> tile, which writes no
      statistics), while the queries answered "tap-table" and the paired tile's row count;
    - conv3x3r = 0: the generic patch-staged kernel runs where the kernel id said "conv3x3r"."""
    rec = list(rec)
    if setting == "conv3x3g=0" and default[0] == "conv3x3g pair":
        assert layer[4] > 64 and default[1] == "conv3x3g pair"
        return ["conv3x3r", "conv3x3r", 0, 0, 0]
    if setting == "conv3x3r=0":
        rec[:2] = ["patch" if k == "conv3x3r" else k for k in rec[:2]]
    return rec


def test_plan_reproduces_the_recorded_dispatch():
    gen = _generator()
    doc = json.load(open(os.path.join(GOLDEN, "conv_dispatch.json")))
    layers = [tuple(x) for x in doc["layers"]]
    assert [s for s, _ in gen.SETTINGS] == list(doc["settings"])
    got = gen.query(layers)
    bad = []
    for setting, recs in doc["settings"].items():
        for layer, default, rec, now in zip(layers, doc["settings"]["default"], recs, got[setting]):
            want = expected(setting, layer, default, rec)
            if now != want:
                bad.append((setting, layer, want, now))
    assert not bad, bad[:10]
    # the recording covers every kind of kernel the queries can name, the paired 16-wide levels included
    seen = {k for recs in doc["settings"].values() for r in recs for k in r[:2]}
    assert {"tap-table", "conv3x3r", "conv3x3g", "conv3x3g pair", "conv3x3h", "conv3x3s", "conv3x3p", "stem"} <= seen


def test_plan_reproduces_the_recorded_dispatch_of_the_autoencoder_and_vae_layers():
    """The entry "ae_vae_reference_geometry": the bf16 layers of main_training.py's Autoencoder and VAE at their own size, collected
    from the engines on the simulated runtime.  The recording is the geometry table of tests/ae_vae_cases.py and nothing else, and
    the library still answers what was recorded: the stride-1 Conv2DTranspose on the paired tile with 16 rows of statistics, no
    fused statistics on any 3x3 stride-2 layer."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ae_vae_cases as T
    gen = _generator()
    doc = json.load(open(os.path.join(GOLDEN, "conv_dispatch.json")))["ae_vae_reference_geometry"]
    layers = [tuple(x) for x in doc["layers"]]
    assert [list(x) for x in layers] == gen.ae_vae_entry()["layers"]          # what the engines launch today
    table = {T.conv_geom(c, "bf16") for c in T.CONV_LAYERS} | {T.convt_geom(c, "bf16") for c in T.CONVT_LAYERS}
    assert {l[:7] for l in layers} == table
    assert [s for s, _ in gen.SETTINGS] == list(doc["settings"])
    got = gen.query(layers)
    bad = [(s, l, r, n) for s, recs in doc["settings"].items() for l, r, n in zip(layers, recs, got[s]) if r != n]
    assert not bad, bad[:10]
    for layer, rec in zip(layers, doc["settings"]["default"]):
        if layer[6] == 1:
            assert rec == ["conv3x3g pair", "conv3x3g pair", 16, 16, 16], (layer, rec)
        else:
            assert rec[2:] == [0, 0, 0], (layer, rec)


def test_wgrad_workspace_query_keeps_the_recorded_values():
    doc = json.load(open(os.path.join(GOLDEN, "wgrad_ws.json")))
    layers = [tuple(x) for x in doc["layers"]]
    got = _generator().query_ws(layers)
    bad = [(layer, want, now) for layer, want, now in zip(layers, doc["ws"], got) if now != want]
    assert not bad, bad[:10]
    # the recording covers stride-1 and stride-2 3x3 layers, the 1x1 layers of the residual graphs and transposed layers
    kinds = {(k, s) for (B, H, W, Ci, Co, k, s, ldx, lddy, tr) in layers}
    assert {(3, 1), (3, 2), (1, 1), (1, 2)} <= kinds
    assert any(tr for *_, tr in layers) and not all(tr for *_, tr in layers)

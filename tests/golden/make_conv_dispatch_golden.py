"""Generates tests/golden/conv_dispatch.json: which bf16 convolution kernel the library picks for every convolution layer of
the benchmarked workloads, and how many rows of fused column statistics it reports, under the default kernel-selection switches,
under each dispatch switch set to 0 on its own, and with conv3x3g_pair = 2; the same for the bf16 layers of main_training.py's
Autoencoder and VAE at their own size, as the entry "ae_vae_reference_geometry" of the same file.  Also tests/golden/wgrad_ws.json: the workspace the
library asks for every weight-gradient layer of the same workloads.

The layers are collected from one train step of each workload on the simulated runtime (tests/sim_runtime.py) with the
convolution launches recorded instead of computed: the geometry of every Conv2D / Conv2DTranspose call and the pixel stride of
the tensor it reads (forward: the layer input, backward: the output gradient).  Every (geometry, stride) pair is then asked
of the library - no GPU needed:
    k3_fwd / k3_dgrad      unetrir_conv3x3_kernel_id_bf16 (ops.K3_NAMES), forward and data gradient
    rows_fwd / rows_dgrad  unetrir_conv2d_colstat_rows_bf16, forward and data gradient
    rows_t                 unetrir_conv2d_transpose_colstat_rows_bf16
The weight-gradient calls are recorded with both pixel strides (x, dy) and whether the layer is a Conv2DTranspose; every layer's
geometry is asked of
    ws / ws_t              unetrir_conv2d_wgrad_ws_bytes / unetrir_conv2d_transpose_wgrad_ws_bytes

    python tests/golden/make_conv_dispatch_golden.py [libunetrir.so to ask instead of the in-tree build]
    python tests/golden/make_conv_dispatch_golden.py --ae-vae-only     (re-records the "ae_vae_reference_geometry" entry alone)
"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:          # run as a script (under pytest, tests/conftest.py has put it there)
    sys.path.insert(0, ROOT)
import unet_rir_amd as U  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "conv_dispatch.json")
WS_OUT = os.path.join(HERE, "wgrad_ws.json")

# the switches the dispatch of forward / data-gradient / Conv2DTranspose-forward launches reads
SWITCHES = ("conv3x3", "conv3x3g", "conv3x3g_pair", "conv3x3h", "conv3x3s", "conv3x3r", "stem", "conv3x3p", "conv3x3d",
            "upconv3x3g", "upconv3x3q", "pw1x1")
SETTINGS = [("default", {})] + [(f"{s}=0", {s: 0}) for s in SWITCHES] + [("conv3x3g_pair=2", {"conv3x3g_pair": 2})]

# bench.py's workloads: configs[1] (headline), configs[3]'s model on one GPU, the reference geometry, configs[0], configs[4] ResAE
WORKLOADS = {
    "cfg1": lambda rt: U.UNetEngine(256, 256, 32, F0=64, k=3, depth=4, device="cpu", runtime=rt, dtype="bf16"),
    "cfg4_model": lambda rt: U.UNetEngine(512, 512, 16, F0=128, k=3, depth=5, device="cpu", runtime=rt, dtype="bf16"),
    "reference_geometry": lambda rt: U.UNetEngine(144, 160, 32, F0=32, k=3, depth=4, device="cpu", runtime=rt, dtype="bf16"),
    "cfg0": lambda rt: U.UNetEngine(256, 256, 4, F0=16, k=3, depth=4, device="cpu", runtime=rt, dtype="bf16"),
    "resae": lambda rt: U.ResAE((256, 256, 2), (2, 16), (32, 64, 128, 256), (3, 3, 3, 3), (2, 2, 2, 2), 32, 16 * 64, name="resae",
                                batch_size=32, device="cpu", runtime=rt, dtype="bf16"),
}
# main_training.py's Autoencoder and VAE at their own size (144 x 160, batch 32, filters 64 ... 512, latent 64, n_neurons 2048): recorded
# as an entry of its own, "ae_vae_reference_geometry", so that the lines recorded for the workloads above stay as they are
AE_VAE_WORKLOADS = {
    "ae": lambda rt: U.AutoencoderEngine(144, 160, 32, device="cpu", runtime=rt, dtype="bf16"),
    "vae": lambda rt: U.VAEEngine(144, 160, 32, device="cpu", runtime=rt, dtype="bf16"),
}
CONV_CALLS = ("conv2d_fwd", "conv2d_fwd_colstat", "conv2d_dgrad", "conv2d_dgrad_colstat", "conv2d_transpose_fwd",
              "conv2d_transpose_fwd_colstat", "conv2d_transpose_dgrad")
WGRAD_CALLS = ("conv2d_wgrad", "conv2d_transpose_wgrad")
# simulated operators whose answer the engines use; every other one is skipped (only the calls are of interest, not the values)
KEEP = ("_elems", "_supported", "_rows", "_ws_bytes", "_table")


def collect_layers(workloads=None, bf16_only=False):
    """{(B, H, W, Cin, Cout, k, stride, ld)} over every convolution call of one train step of each workload, and
    {(B, H, W, Cin, Cout, k, stride, ldx, lddy, transposed)} over every weight-gradient call.  bf16_only: leave out the calls on fp32
    tensors (the Dense branch of the auto-encoders: its data gradient with an addend is a 1x1 convolution in fp32)."""
    workloads = WORKLOADS if workloads is None else workloads
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vae_cpu_ops
    from oracle import torch_ref as R
    from sim_runtime import SimRuntime
    seen, wseen = set(), set()

    def recorder(name):
        def rec(g, x, *a, **k):
            if not bf16_only or x.sfx == "bf16":
                seen.add((g.B, g.H, g.W, g.Cin, g.Cout, g.k, g.stride, x.ld))
        rec.__name__ = name
        return rec

    def wgrad_recorder(name):
        def rec(g, x, dy, *a, **k):
            if bf16_only and x.sfx != "bf16":
                return
            wseen.add((g.B, g.H, g.W, g.Cin, g.Cout, g.k, g.stride, x.ld, dy.ld, int(name == "conv2d_transpose_wgrad")))
        rec.__name__ = name
        return rec

    for name, make in workloads.items():
        mp = pytest.MonkeyPatch()
        try:
            rt = SimRuntime()
            impl = vae_cpu_ops.install(mp, rt)          # tests/cpu_ops.py and the VAE's operators on top
            for c in dir(impl) + dir(vae_cpu_ops.VaeCpuOps):
                if not c.startswith("_") and c != "rt" and not c.endswith(KEEP):
                    mp.setattr(U.ops, c, recorder(c) if c in CONV_CALLS else wgrad_recorder(c) if c in WGRAD_CALLS else
                               (lambda *a, **k: None))
            model = make(rt)
            tr = U.Trainer(model, lr=1e-3, dropout=False) if name != "resae" else U.Trainer(model, lr=1e-3)
            eng = getattr(model, "engine", model)
            H, W, B = eng.H, eng.W, eng.B
            spec_in, emb, spec_out = (torch.tensor(a) for a in R.synthetic_batch(R.Config(H, W, 16, 3), B))
            tr.step(spec_in, emb, spec_out)
            del tr, model, eng
        finally:
            mp.undo()
        print(f"{name}: {len(seen)} layers, {len(wseen)} weight-gradient layers so far", file=sys.stderr)
    return sorted(seen), sorted(wseen)


def query(layers):
    import ctypes as C
    from unet_rir_amd import _lib
    L = _lib.lib()
    out = {}
    old = U.ops.get_config()
    try:
        for sname, sw in SETTINGS:
            U.ops.set_config(**{**old, **sw})
            rows = []
            for (B, H, W, Cin, Cout, k, s, ld) in layers:
                g = _lib.ConvGeom(B, H, W, Cin, Cout, k, s)
                rows.append([U.ops.K3_NAMES[L.unetrir_conv3x3_kernel_id_bf16(C.byref(g), 0, ld)],
                             U.ops.K3_NAMES[L.unetrir_conv3x3_kernel_id_bf16(C.byref(g), 1, ld)],
                             int(L.unetrir_conv2d_colstat_rows_bf16(C.byref(g), 0, ld)),
                             int(L.unetrir_conv2d_colstat_rows_bf16(C.byref(g), 1, ld)),
                             int(L.unetrir_conv2d_transpose_colstat_rows_bf16(C.byref(g), ld))])
            out[sname] = rows
    finally:
        U.ops.set_config(**old)
    return out


def query_ws(wlayers):
    """[ws, ws_t] per weight-gradient layer: the two workspace queries on its geometry (they read no switch and no pixel stride)."""
    import ctypes as C
    from unet_rir_amd import _lib
    L = _lib.lib()
    out = []
    for (B, H, W, Cin, Cout, k, s, ldx, lddy, tr) in wlayers:
        g = _lib.ConvGeom(B, H, W, Cin, Cout, k, s)
        out.append([int(L.unetrir_conv2d_wgrad_ws_bytes(C.byref(g))), int(L.unetrir_conv2d_transpose_wgrad_ws_bytes(C.byref(g)))])
    return out


def ae_vae_entry():
    layers, _ = collect_layers(AE_VAE_WORKLOADS, bf16_only=True)
    return {"layers": [list(x) for x in layers], "settings": query(layers)}


if __name__ == "__main__":
    if sys.argv[1:2] == ["--ae-vae-only"]:      # add or replace that entry alone: every other recorded line stays as it is
        with open(OUT) as f:
            doc = json.load(f)
        doc["ae_vae_reference_geometry"] = ae_vae_entry()
        with open(OUT, "w") as f:
            json.dump(doc, f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {OUT}: {len(doc['ae_vae_reference_geometry']['layers'])} auto-encoder layers x {len(SETTINGS)} settings", file=sys.stderr)
        sys.exit(0)
    if len(sys.argv) > 1:
        U._lib.use_library(os.path.abspath(sys.argv[1]))
    layers, wlayers = collect_layers()
    doc = {"fields": ["k3_fwd", "k3_dgrad", "rows_fwd", "rows_dgrad", "rows_t"],
           "layer_fields": ["B", "H", "W", "Cin", "Cout", "k", "stride", "ld"],
           "layers": [list(x) for x in layers], "settings": query(layers)}
    doc["ae_vae_reference_geometry"] = ae_vae_entry()
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {OUT}: {len(layers)} layers x {len(SETTINGS)} settings", file=sys.stderr)
    doc = {"fields": ["ws", "ws_t"], "layer_fields": ["B", "H", "W", "Cin", "Cout", "k", "stride", "ldx", "lddy", "transposed"],
           "layers": [list(x) for x in wlayers], "ws": query_ws(wlayers)}
    with open(WS_OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {WS_OUT}: {len(wlayers)} weight-gradient layers", file=sys.stderr)

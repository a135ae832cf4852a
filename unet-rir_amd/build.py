"""Build the gfx950 shared library (C ABI of include/unetrir.h) in-tree with hipcc.

One object per translation unit (compiled in parallel, only those whose source or headers changed), then one link:
editing a single kernel rebuilds in seconds instead of a minute."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libunetrir.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "unetrir.h")      # the C ABI: compiled into the library, parsed by _lib
SOURCES = ["igemm.hip", "api.hip", "elementwise.hip", "head.hip", "head_mfma.hip", "head1x1.hip", "head_up2.hip", "wgrad3x3.hip", "wgrad3x3r.hip", "wgrad3x3g.hip", "wgrad3x3d.hip", "igemm_bf16.hip", "conv3x3.hip", "conv3x3r.hip", "conv3x3g.hip", "conv3x3h.hip", "conv3x3s.hip", "conv3x3d.hip", "conv3x3p.hip", "upconv3x3.hip", "upconv3x3g.hip", "upconv3x3q.hip", "features.hip", "dense.hip", "stem3x3.hip", "stem_composite.hip", "pw1x1.hip", "conv2x2.hip", "igemm2_bf16.hip", "weights.hip", "splitk_reduce.hip", "evalmetrics.hip", "acoustics.hip", "vae.hip", "vq.hip", "dataset.hip", "griffinlim.hip", "griffinlim_fft.hip", "lamb.hip", "cnn_clas.hip", "waveloss.hip", "auralize.hip", "auralize_fft.hip", "istft_bwd.hip", "decayloss.hip", "spectralloss.hip", "spectralloss_fft.hip", "resample.hip"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wno-unused-value"]


def _headers():
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [HEADER]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def needs_build():
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + _headers()
    return _stale(LIB, deps)


def build(force=False, verbose=False, extra_flags=(), lib=LIB, obj_dir=OBJ):
    """hipcc cross-compiles for gfx950 without a GPU present."""
    if not force and lib == LIB and not needs_build():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(obj_dir, exist_ok=True)
    hdrs = _headers()
    jobs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(obj_dir, s[:-4] + ".o")
        if force or _stale(obj, [src] + hdrs):
            jobs.append([hipcc] + FLAGS + list(extra_flags) + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(run, jobs))
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] +
        [os.path.join(obj_dir, s[:-4] + ".o") for s in SOURCES])
    return lib


ABL_LIB = os.path.join(HERE, "libunetrir_abl.so")


def build_ablations(verbose=False):
    """The timing-ablation build for scripts/ (kernels with a stage switched off; results invalid).  Not loaded by the package
    unless a script asks for it with _lib.use_library(build.ABL_LIB)."""
    return build(force=False, verbose=verbose, extra_flags=["-DUNETRIR_ABLATIONS"], lib=ABL_LIB, obj_dir=os.path.join(HERE, "build_abl"))


PROBE_DIR = os.path.join(os.path.dirname(HERE), "tests", "probe")
PROBE_SRC = os.path.join(PROBE_DIR, "fft_probe.hip")
PROBE_LIB = os.path.join(HERE, "libunetrir_probe.so")


def probe_needs_build():
    return _stale(PROBE_LIB, [PROBE_SRC, os.path.join(PROBE_DIR, "fft_walk.h"), os.path.join(CSRC, "fft_lds.h")])


def build_probe(force=False, verbose=False):
    """The tests' probe of csrc/fft_lds.h (tests/probe/fft_probe.hip: the header walked on the host and run on the device with no
    consumer around it; loaded by tests/fft_probe.py).  A library of its own: nothing of it is in libunetrir.so or include/unetrir.h."""
    if not force and not probe_needs_build():
        return PROBE_LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + FLAGS + ["-shared", "-I", CSRC, PROBE_SRC, "-o", PROBE_LIB]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return PROBE_LIB


if __name__ == "__main__":
    if "--probe" in sys.argv:
        print(build_probe(force="--force" in sys.argv, verbose=True))
    elif "--ablations" in sys.argv:
        print(build_ablations(verbose=True))
    else:
        print(build(force="--force" in sys.argv, verbose=True))

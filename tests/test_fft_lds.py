"""csrc/fft_lds.h walked thread by thread on the host (tests/probe/fft_walk.h through tests/fft_probe.py) against fp64, for every M the
header promises (64 ... 2048; 1024 is instantiated by nothing else) and the four modes of tests/fft_lds_ref.py: the twiddle table
against mpmath, the criteria C1 - C3 defined there, the three thread orders bit for bit, the mutations (each must fail), and the walk as
a stand-alone program under the host sanitizers.  No GPU; tests/test_fft_lds_gpu.py holds the device to the same walk bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import fft_lds_ref as FR
import fft_probe as FP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(M, mode) for M in FR.SIZES for mode in FR.MODES]
IDS = [f"M{M}-mode{mode}" for M, mode in CASES]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the probe stays outside the product ----

def test_the_product_library_exports_no_probe_symbol():
    import unet_rir_amd
    L = unet_rir_amd._lib.lib()
    P = FP.lib()
    for name in FP.EXPORTS:
        assert hasattr(P, name) and not hasattr(L, name), name
    assert not any("probe" in n or n.startswith("fl_") for n in unet_rir_amd._lib.EXPORTS)
    assert "fft_probe.hip" not in unet_rir_amd.build.SOURCES
    assert os.path.basename(unet_rir_amd.build.PROBE_LIB) == "libunetrir_probe.so" and unet_rir_amd.build.PROBE_LIB != unet_rir_amd.build.LIB
    out = subprocess.run(["strings", "-n", "8", unet_rir_amd.build.LIB], capture_output=True, text=True, check=True).stdout
    assert "fftprobe" not in out


# ---- the table ----

def test_every_table_entry_is_the_correctly_rounded_value():
    """cos and -sin(pi t / 2048) at 200 bits, rounded ONCE to fp32 (through fp64 would round twice), against all 4096 components"""
    import mpmath
    tab = FP.tab_host()
    want = np.empty((2048, 2), dtype=np.float32)
    with mpmath.workprec(200):
        for t in range(2048):
            a = mpmath.pi * t / 2048
            want[t, 0] = _fp32(mpmath, mpmath.cos(a))
            want[t, 1] = _fp32(mpmath, -mpmath.sin(a))
    diff = np.argwhere(tab != want)                                 # on values: the table's -sin(0) is -0
    assert diff.size == 0, (len(diff), diff[:8], tab[tab != want][:8], want[tab != want][:8])
    assert np.all(np.abs(want) >= 2.0 ** -10 * (want != 0))         # every non-zero entry is a normal number: 24 bits is fp32's rounding
    assert tab[1024, 0] == 0.0                                      # cos(pi / 2): the exact 0, where pi in fp64 gives 6e-17
    assert tab[0, 0] == 1.0 and tab[0, 1] == 0.0 and tab[1024, 1] == -1.0


def _fp32(mpmath, v):
    """a 200-bit value rounded once to 24 bits, nearest even; below half of fp32's smallest subnormal it is 0 (cos(pi / 2) at 200 bits
    is 1e-61, not 0)"""
    if abs(v) < mpmath.mpf(2) ** -150:
        return 0.0
    with mpmath.workprec(24):
        return float(+v)


def test_fl_w_is_the_table_with_the_sign_rules():
    tab, w = FP.tab_host(), FP.table_host()
    t = np.arange(4096)
    base = tab[t & 2047]
    sign = np.where(t & 2048, np.float32(-1), np.float32(1))[:, None]
    fwd = base * sign                                               # exp(-2 pi i t / 4096): the other half circle by a sign
    inv = fwd * np.array([1, -1], dtype=np.float32)                 # the conjugate
    assert np.array_equal(w[0], fwd) and np.array_equal(w[1], inv)  # == on values: -0 and +0 are the same twiddle
    assert np.all(np.isfinite(w))
    ang = 2 * np.pi * t / 4096
    assert np.max(np.abs(w[0][:, 0] - np.cos(ang))) <= 2.0 ** -24 and np.max(np.abs(w[0][:, 1] + np.sin(ang))) <= 2.0 ** -24
    assert np.max(np.abs(w[1][:, 1] - np.sin(ang))) <= 2.0 ** -24


# ---- the host walk against fp64 ----

@pytest.mark.parametrize("M,mode", CASES, ids=IDS)
def test_host_walk_random_data_c1(M, mode):
    FR.check_c1(M, mode, FP.host_random(M, mode))


@pytest.mark.parametrize("M,mode", CASES, ids=IDS)
def test_host_walk_impulses_c2(M, mode):
    FR.check_c2(M, mode, FP.host_impulses(M, mode))


@pytest.mark.parametrize("M", FR.SIZES)
def test_host_walk_round_trip_c3(M):
    FR.check_c3(M, FP.host_roundtrip(M))


@pytest.mark.parametrize("M,mode", CASES, ids=IDS)
def test_thread_order_does_not_change_a_bit(M, mode):
    """A pass's stores are disjoint and a thread owns the pairs of the split it touches: walking the threads of the store half and of
    the split in ascending, descending or shuffled order gives the same bits, on random data and on impulses across the image."""
    imp = FR.impulse_input(M, mode)
    imp = imp[::max(1, imp.shape[0] // 64)]                         # 64 positions spread over the image
    for x, base in ((FR.random_input(M, mode), FP.host_random(M, mode)), (imp, FP.host(M, mode, imp))):
        for order in FP.ORDERS[1:]:
            assert np.array_equal(bits(FP.host(M, mode, x, order=order)), bits(base)), (M, mode, order)


# ---- the checks see what they are there to see ----

@pytest.mark.parametrize("M", FR.SIZES)
@pytest.mark.parametrize("name", FR.MUTATIONS)
def test_every_mutation_fails_a_check(name, M):
    for mode in FR.MUTATION_MODES[name]:
        x = FR.random_input(M, mode)
        rs = FR.random_reference(M, mode)[1]
        imp = FR.impulse_input(M, mode)[:8]                         # the first impulses do: the mutation goes into image 3 (in mode 3
                                                                    # image 1 is the constant 1 - i, which no exchange changes)
        ri = FR.restate(mode, imp)
        n_all = imp.shape[0]

        def c2_head(got):                                           # C2 on the first images, by the same function
            d = got.astype(np.complex128) - FR.impulse_closed_form(M, mode, 0, n_all)
            err = np.maximum(np.abs(d.real), np.abs(d.imag)) if mode == 3 else np.abs(d)
            tol = FR.EL_LEVEL * FR.U * FR.levels(M, mode) * (2.0 if mode == 3 else 1.0)
            assert np.all(err <= tol)

        FR.check_c1(M, mode, rs, quiet=True)                        # unmutated, the restatement passes
        c2_head(ri)
        with pytest.raises(AssertionError):
            FR.check_c1(M, mode, FR.mutate(name, M, mode, rs, x), quiet=True)
        with pytest.raises(AssertionError):
            c2_head(FR.mutate(name, M, mode, ri, imp, img=3))


# ---- the host sanitizers, on a stand-alone program ----

def test_host_walk_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/probe/fft_walk_main.cpp: image buffers of exactly M elements, host-only compile (no device code, no HIP call), run as a
    child process of its own.  Exit status 0 is the assertion."""
    import unet_rir_amd
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "fft_walk_main")
    # host code only: no device pass is compiled (--offload-host-only) and none would be instrumented (-fno-gpu-sanitize)
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g", "-std=c++17",
           "-I", unet_rir_amd.build.CSRC, os.path.join(ROOT, "tests", "probe", "fft_walk_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok"

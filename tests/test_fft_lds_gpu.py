"""csrc/fft_lds.h on the device, by itself (tests/probe/fft_probe.hip): every M the header promises (64 ... 2048; nothing else
instantiates 1024), the four modes of tests/fft_lds_ref.py and both workgroup forms - G = 1, one image worked by M / 8 threads (8 at
M = 64), and G = 2048 / M images side by side in 256 threads, the form of spectralloss_fft.hip.

The device must give the bits of the host walk of the same header (tests/test_fft_lds.py holds that walk to fp64): the header promises
bits that do not depend on how the surrounding code was compiled.  C1 - C3 are asserted on the device outputs in their own right first,
so that a wrong transform reads as an accuracy failure.  Every output is carved out of a NaN-prefilled buffer with a canary either side.

Worst figures of a run are printed (pytest -s) and recorded in DESIGN.md, section 7.12."""
import numpy as np
import pytest
import torch

import fft_lds_ref as FR
import fft_probe as FP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 1234.5
GUARD = 1024                # floats: the carved output stays 8-byte aligned
CASES = [(M, mode) for M in FR.SIZES for mode in FR.MODES]
IDS = [f"M{M}-mode{mode}" for M, mode in CASES]


def forms(M):
    """images per workgroup: the header's own contract and the many-images form (the same thing at M = 2048)"""
    return sorted({1, 2048 // M})


class Guarded:
    def __init__(self, n, M):
        self.big = torch.full((n * M * 2 + 2 * GUARD,), CANARY, dtype=torch.float32, device=DEV)
        self.out = self.big[GUARD:GUARD + n * M * 2].view(n, M, 2)
        self.out.fill_(float("nan"))

    def result(self):
        torch.cuda.synchronize()
        assert bool((self.big[:GUARD] == CANARY).all()) and bool((self.big[GUARD + self.out.numel():] == CANARY).all()), "written outside out"
        return self.out


def to_dev(x):
    x = np.array(x, dtype=np.complex64)                               # a copy: the cached arrays are read-only
    return torch.from_numpy(x.view(np.float32).reshape(x.shape[0], x.shape[1], 2)).to(DEV)


def to_host(t):
    return t.cpu().numpy().view(np.complex64)[..., 0]


def run(M, mode, G, x, stop=-1):
    """one launch on complex64 [n, M] -> complex64 [n, M]; exactly n M float2 written (no NaN left, canaries intact)"""
    xd = x if isinstance(x, torch.Tensor) else to_dev(x)
    g = Guarded(xd.shape[0], M)
    FP.device(M, mode, G, xd, g.out, stop=stop)
    out = to_host(g.result())
    assert not np.any(np.isnan(out.view(np.float32))), (M, mode, G, "an element left unwritten")
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (what, f"{len(bad)} of {bits(want).size} words differ; first (image, 2 element + component):", bad[:8],
                           got.view(np.float32)[tuple(bad[:8].T)], want.view(np.float32)[tuple(bad[:8].T)])


def test_device_table_is_the_host_table_bit_for_bit():
    out = torch.full((2 * 4096 * 2 + 2 * GUARD,), CANARY, dtype=torch.float32, device=DEV)
    err = FP.lib().fftprobe_table_device(out[GUARD:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert err == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.all(host[:GUARD] == CANARY) and np.all(host[-GUARD:] == CANARY)
    assert np.array_equal(bits(host[GUARD:-GUARD].reshape(2, 4096, 2)), bits(FP.table_host()))


@pytest.mark.parametrize("M,mode", CASES, ids=IDS)
def test_random_data_c1_and_the_bits_of_the_host_walk(M, mode):
    x = FR.random_input(M, mode)
    for G in forms(M):
        got = run(M, mode, G, x)
        ratio, top = FR.check_c1(M, mode, got, quiet=True)
        print(f"device C1 M={M} mode={mode} G={G}: worst e / e(restatement) = {ratio:.3g}, worst e / ceiling = {top:.3g}")
        same_bits(got, FP.host_random(M, mode), f"M={M} mode={mode} G={G} random")


@pytest.mark.parametrize("M,mode", CASES, ids=IDS)
def test_impulses_c2_and_the_bits_of_the_host_walk(M, mode):
    xd = to_dev(FR.impulse_input(M, mode))
    for G in forms(M):
        got = run(M, mode, G, xd)
        worst = FR.check_c2(M, mode, got, quiet=True)
        print(f"device C2 M={M} mode={mode} G={G}: largest element error = {worst:.3g} u")
        same_bits(got, FP.host_impulses(M, mode), f"M={M} mode={mode} G={G} impulses")


@pytest.mark.parametrize("M", FR.SIZES)
def test_round_trip_c3_and_the_bits_of_the_host_walk(M):
    for G in forms(M):
        spec = run(M, 2, G, FR.random_images(M))
        got = run(M, 3, G, spec)
        ratio = FR.check_c3(M, got, quiet=True)
        print(f"device C3 M={M} G={G}: worst e / e(restatement) = {ratio:.3g}")
        same_bits(got, FP.host_roundtrip(M), f"M={M} G={G} round trip")


@pytest.mark.parametrize("M,mode", [c for c in CASES if c[0] < 2048], ids=[i for c, i in zip(CASES, IDS) if c[0] < 2048])
def test_images_do_not_see_each_other(M, mode):
    """An image's bits are the same worked alone (G = 1) as at any group position of a G = 2048 / M workgroup among different images:
    the random set in its own order, in another order (every image at another group position, with other neighbours), and cut so that
    the last workgroup is ragged at another place."""
    G = 2048 // M
    x = np.asarray(FR.random_input(M, mode))
    n = x.shape[0]                                                    # 2 G + 1: the third workgroup holds one image
    alone = run(M, mode, 1, x)
    other = np.roll(np.arange(n)[::-1], 1)                            # position p holds image other[p]
    assert np.mean(other % G != np.arange(n) % G) >= 0.75             # most images sit at another group position than in their own order
    for name, idx in (("own order", np.arange(n)), ("other order", other), ("cut", np.arange(G + max(1, G // 2))),
                      ("cut, other order", other[:2 * G - 1])):
        got = run(M, mode, G, x[idx])
        same_bits(got, alone[idx], f"M={M} mode={mode} G={G} {name}")


@pytest.mark.parametrize("M", FR.SIZES)
def test_two_runs_and_a_captured_graph_give_the_same_bits(M):
    """mode 2 then mode 3 in the many-images form, eagerly twice and captured once on a side stream and replayed twice"""
    G = 2048 // M
    xd = to_dev(FR.random_images(M))
    mid, out = torch.empty_like(xd), torch.empty_like(xd)

    def both():
        FP.device(M, 2, G, xd, mid)
        FP.device(M, 3, G, mid, out)

    both()
    torch.cuda.synchronize()
    eager = out.clone()
    same_bits(to_host(eager), FP.host_roundtrip(M), f"M={M} eager")
    both()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both()                                                        # on the side stream, outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            both()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        mid.fill_(CANARY)
        out.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32))

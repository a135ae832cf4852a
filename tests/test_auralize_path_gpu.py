"""`auralize_path` (csrc/auralize_fft.hip) on the device against the fp64 definition of tests/auralize_path_ref.py.

The block is fixed at P = 2048, so the cases of auralize_path_ref.CASES are the smallest shapes that span its edges: one node; 32 nodes
inside one block with a tail after the last; spacings of one, two and four blocks off the block grid, with K across one, two and five
partitions; nodes exactly on block edges; uneven spacings with a node before the output, two 32 samples apart and one far beyond the
end.  Every case runs with B = 1 and 3 and with x shared and per row, into the middle of a canary-filled buffer.

1. uniform data: every element within the bound of include/unetrir.h (auralize_path_ref.bound) - loose, it catches gross errors only;
2. sharp: per row the largest error over the row's peak at most 4 times that of the fp32 restatement (auralize_path_ref.path_ols_ref)
   on the same data, plus 2^-22 - the factor and the floor of tests/test_spectral_loss_fft_gpu.py for the same transforms;
3. integer data with power-of-two spacings D (exact gains): round(D out) == D y everywhere, on the cases whose restatement stays within
   1 / 8 (tests/test_auralize_path_ref.py);
4. wherever one node has gain 1 - all of R = 1, n <= tau_0, n >= tau_{R-1}, every n = tau_r - the bits of auralize(h_r, x, method="fft");
5. bits independent of the run, B, the row's place, shared or per-row x, a truncated L and a larger workspace;
6. exactly the advertised workspace, between canaries; 7. a captured graph replays the same bits and follows a rewritten `times`."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from auralize_path_ref import (CASES, INT_CASES, P, bound, bound_figure, case, int_figure, path_ols_ref, peak_error, sharp_figure,
                               single_node)

pytestmark = pytest.mark.gpu

NAMES = sorted(CASES)
CANARY = 12345.678          # no integer, so no sum of integer data


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()           # a copy: the cached arrays are read-only


def _run(h, x, times, L=None, pad=(1, 64)):
    """auralize_path into the middle of a canary-filled buffer (the front pad also puts `out` off 8-byte alignment); returns the result
    on the device after checking that nothing around it was written and every element of it was."""
    import unet_rir_amd as U
    B, N, K = h.shape[0], x.shape[-1], h.shape[-1]
    L = N + K - 1 if L is None else L
    buf = torch.full((pad[0] + B * L + pad[1],), CANARY, dtype=torch.float32, device="cuda")
    out = buf[pad[0]:pad[0] + B * L].view(B, L)
    got = U.auralize_path(h, x, times, length=L, out=out)
    assert got is out
    assert torch.all(buf[:pad[0]] == CANARY) and torch.all(buf[pad[0] + B * L:] == CANARY), "written outside out"
    assert not torch.any(out == CANARY), "an element of out was not written"
    return out.clone()


def _variants(name, kind):
    """(label, device h, device x, host h, host x, nodes64, path_ref64) for B = 1 and 3, x shared and per row"""
    h, x, times, rows, shared = case(name, kind)
    hd, xd = _dev(h), _dev(x)
    for B in (1, 3):
        yield f"B={B} rows", "rows", hd[:B].contiguous(), xd[:B].contiguous(), h[:B], x[:B], rows[0][:B], rows[1][:B]
        yield f"B={B} shared", "shared", hd[:B].contiguous(), xd[0].contiguous(), h[:B], x[0], shared[0][:B], shared[1][:B]


@functools.lru_cache(maxsize=None)
def _restated(name, layout):
    """the fp32 restatement on the case's data, all three rows (a row's result does not depend on the others)"""
    h, x, times, _, _ = case(name, "uniform")
    return path_ols_ref(h, x if layout == "rows" else x[0], times)


@pytest.mark.parametrize("name", NAMES)
def test_uniform_data_bound_sharp_check_and_stationary_bits(name):
    import unet_rir_amd as U
    R, K, N, times = CASES[name]
    L = N + K - 1
    for label, layout, hd, xd, h, x, nodes, ref in _variants(name, "uniform"):
        out = _run(hd, xd, times)
        got = out.cpu().numpy()
        assert np.all(np.isfinite(got)), label
        f1 = bound_figure(got, ref, bound(h, x, times, nodes))                                  # check 1
        f2 = sharp_figure(got, ref, _restated(name, layout)[:h.shape[0]])                       # check 2
        ratio = peak_error(got, ref) / peak_error(_restated(name, layout)[:h.shape[0]], ref)
        print(f"case {name} {label}: error / bound = {f1:.3g}, peak error / (4 restatement's + 2^-22) = {f2:.3g}, "
              f"peak error / restatement's = {ratio.min():.3g} ... {ratio.max():.3g}")
        assert f1 <= 1.0, label
        assert f2 <= 1.0, label
        for r, idx in single_node(times, L):                                                    # check 4
            still = U.auralize(hd[:, r].contiguous(), xd, method="fft")
            i = torch.from_numpy(idx).cuda()
            assert torch.equal(out[:, i], still[:, i]), (label, r)
        if R == 1:
            assert torch.equal(out, U.auralize(hd[:, 0].contiguous(), xd, method="fft")), label


@pytest.mark.parametrize("name", sorted(INT_CASES))
def test_integer_data_with_exact_gains_rounds_to_the_exact_result(name):
    amp, D = INT_CASES[name]
    R, K, N, times = CASES[name]
    for label, layout, hd, xd, h, x, nodes, ref in _variants(name, "int"):
        got = _run(hd, xd, times).cpu().numpy().astype(np.float64)
        print(f"case {name} {label}, |h|, |x| <= {amp}: largest |D out - D y| = {int_figure(got, ref, D) / 2:.3g}")
        bad = np.flatnonzero(np.rint(D * got) != D * ref)                                       # check 3
        assert bad.size == 0, (label, bad[:8], (D * got).ravel()[bad[:8]], (D * ref).ravel()[bad[:8]])


@pytest.mark.parametrize("name", ["b", "e", "g"])
def test_bits_do_not_depend_on_run_batch_layout_length_or_workspace(name):
    import unet_rir_amd as U
    R, K, N, times = CASES[name]
    h, x, _, _, _ = case(name, "uniform")
    hd, xd = _dev(h), _dev(x)
    f = U.auralize_path
    full = f(hd, xd, times)
    assert full.shape == (3, N + K - 1) and full.dtype == torch.float32
    assert torch.equal(f(hd, xd, times), full)                                                  # two runs
    for b in range(3):                                                                          # a row alone, [R, K] and [1, R, K]
        assert torch.equal(f(hd[b], xd[b], times), full[b:b + 1]) and torch.equal(f(hd[b:b + 1], xd[b:b + 1], times), full[b:b + 1])
    assert torch.equal(f(hd.flip(0).contiguous(), xd.flip(0).contiguous(), times), full.flip(0))              # its place in the batch
    sh = f(hd, xd[1], times)
    assert torch.equal(sh, f(hd, xd[1].repeat(3, 1), times))                                    # shared x = x repeated per row
    assert torch.equal(sh[1], full[1])
    same = f(hd, xd, times, length="same")
    assert same.shape == (3, N) and torch.equal(same, full[:, :N])                              # a truncated L = the head of the full result
    for L in (1, 31, P - 1, P, P + 1, times[1] + 1, N + K - 2):
        if 1 <= L <= N + K - 1:
            assert torch.equal(f(hd, xd, times, length=L), full[:, :L]), L
    assert torch.equal(f(hd, xd, np.asarray(times)), full) and torch.equal(f(hd, xd, torch.tensor(times)), full)
    tdev = torch.tensor(times, dtype=torch.int32, device="cuda")
    need = U.ops.auralize_path_ws_bytes(3, R, K, N, N, N + K - 1)
    for ws in (U.ops.Workspace(hd.device), U.ops.Workspace(hd.device, 2 * need + 4096)):        # grown by the call; larger than needed
        out = torch.empty_like(full)
        U.ops.auralize_path_f32(hd, tdev, xd, out, ws=ws)
        assert ws.nbytes >= need and torch.equal(out, full)


def test_an_even_schedule_is_spacing_and_start():
    import unet_rir_amd as U
    R, K, N, times = CASES["c"]
    h, x, _, _, _ = case("c", "uniform")
    hd, xd = _dev(h), _dev(x[0])
    assert torch.equal(U.auralize_path(hd, xd, spacing=2048, start=300), U.auralize_path(hd, xd, times))


@pytest.mark.parametrize("dry_rows", (0, 1), ids=("shared", "rows"))
def test_exactly_the_advertised_workspace_is_used(dry_rows):
    """The C entry point with a workspace of exactly ws_bytes between canaries, and one byte less refused."""
    import unet_rir_amd as U
    R, K, N, times = CASES["c"]
    B, L = 3, N + K - 1
    h, x, _, rows, shared = case("c", "int")
    hd, xd = _dev(h), _dev(x if dry_rows else x[0])
    td = torch.tensor(times, dtype=torch.int32, device="cuda")
    stride = N if dry_rows else 0
    need = U.ops.auralize_path_ws_bytes(B, R, K, N, stride, L)
    assert need == 16384 * (B * R * 2 + (B if dry_rows else 1) * 6)
    buf = torch.full((4096 + need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = buf[4096:4096 + need]
    obuf = torch.full((64 + B * L + 64,), CANARY, dtype=torch.float32, device="cuda")
    out = obuf[64:64 + B * L].view(B, L)
    lib = U._lib.lib()
    args = (C.c_void_p(hd.data_ptr()), C.c_void_p(td.data_ptr()), C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr()), B, R, K, N, stride, L)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.unetrir_auralize_path_f32(*args, C.c_void_p(ws.data_ptr()), need - 1, stream) == 10001
    assert lib.unetrir_auralize_path_f32(*args, C.c_void_p(ws.data_ptr() + 8), need, stream) == 10001
    torch.cuda.synchronize()
    assert torch.all(buf == 0xA5) and torch.all(obuf == CANARY), "a refused call wrote"
    assert lib.unetrir_auralize_path_f32(*args, C.c_void_p(ws.data_ptr()), need, stream) == 0
    torch.cuda.synchronize()
    assert torch.all(buf[:4096] == 0xA5) and torch.all(buf[4096 + need:] == 0xA5), "written outside the advertised workspace"
    assert torch.all(obuf[:64] == CANARY) and torch.all(obuf[64 + B * L:] == CANARY), "written outside out"
    D = INT_CASES["c"][1]
    assert np.array_equal(np.rint(D * out.cpu().numpy().astype(np.float64)), D * (rows if dry_rows else shared)[1])


def test_graph_capture_replays_the_same_bits_and_follows_a_rewritten_schedule():
    import unet_rir_amd as U
    R, K, N, times = CASES["d"]
    other = tuple(t + 1500 for t in times[:-1]) + (times[-1] + 40,)
    h, x, _, _, _ = case("d", "uniform")
    hd, xd = _dev(h), _dev(x[0])
    eager, eager_other = U.auralize_path(hd, xd, times), U.auralize_path(hd, xd, other)
    assert not torch.equal(eager, eager_other)
    td = torch.tensor(times, dtype=torch.int32, device="cuda")
    out = torch.zeros_like(eager)
    ws = U.ops.Workspace(hd.device, U.ops.auralize_path_ws_bytes(3, R, K, N, 0, N + K - 1))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        U.ops.auralize_path_f32(hd, td, xd, out, ws=ws)       # on the side stream, outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            U.ops.auralize_path_f32(hd, td, xd, out, ws=ws)
    torch.cuda.current_stream().wait_stream(s)
    for sched, want in ((times, eager), (other, eager_other), (times, eager)):
        td.copy_(torch.tensor(sched, dtype=torch.int32))
        out.fill_(CANARY)
        ws.buf.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), sched


def test_a_schedule_that_breaks_the_precondition_stays_inside_out():
    """ops.auralize_path_f32 does not look at the contents of times: a table that is not increasing gives unspecified values, written
    to every element of out and nowhere else."""
    import unet_rir_amd as U
    R, K, N, times = CASES["c"]
    h, x, _, _, _ = case("c", "uniform")
    hd, xd = _dev(h), _dev(x[0])
    L = N + K - 1
    for table in ((5000, 300, 300, -7, 2048), (2 ** 31 - 1, -2 ** 31, 0, 0, 2 ** 31 - 1)):
        td = torch.tensor(table, dtype=torch.int32, device="cuda")
        buf = torch.full((64 + 3 * L + 64,), CANARY, dtype=torch.float32, device="cuda")
        out = buf[64:64 + 3 * L].view(3, L)
        U.ops.auralize_path_f32(hd, td, xd, out)
        torch.cuda.synchronize()
        assert torch.all(buf[:64] == CANARY) and torch.all(buf[64 + 3 * L:] == CANARY) and not torch.any(out == CANARY), table


def test_the_script_walks_a_directory_of_responses(tmp_path):
    """scripts/auralize.py --walk MS: the files in sorted order become one path, MS milliseconds apart; one file, scaled by --peak."""
    import subprocess
    import sys
    import unet_rir_amd as U
    from unet_rir_amd.auralize import write_wav
    sr, dur, ms = 8000, 0.2, 100
    rng = np.random.default_rng(11)
    rirs = tmp_path / "rirs"
    rirs.mkdir()
    for name in ("p2", "p0", "p1"):                               # written out of order: the path is p0, p1, p2
        write_wav(str(rirs / (name + ".wav")), rng.uniform(-0.5, 0.5, int(sr * dur)).astype(np.float32), sr)
    write_wav(str(tmp_path / "dry.wav"), rng.uniform(-0.5, 0.5, 5000).astype(np.float32), sr)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, os.path.join(root, "scripts", "auralize.py"), "--rirs", str(rirs), "--dry", str(tmp_path / "dry.wav"),
                          "--sr", str(sr), "--duration", str(dur), "--walk", str(ms), "--method", "direct", "--peak", "0.5", "--length",
                          "same", "--out", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert os.listdir(tmp_path / "out") == ["walk.wav"]
    h = torch.from_numpy(np.stack([U.read_wav(str(rirs / f"p{i}.wav"), sr, dur) for i in range(3)])).cuda()
    x = torch.from_numpy(U.read_wav(str(tmp_path / "dry.wav"), sr, 5000.5 / sr)).cuda()
    want = U.auralize_path(h, x, spacing=800, length="same")[0].cpu().numpy()
    want = want * np.float32(0.5 / np.abs(want).max())
    got = U.read_wav(str(tmp_path / "out" / "walk.wav"), sr, 5000.5 / sr)
    assert got.shape == (5000,) and np.allclose(got + (want.mean() - got.mean()), want, rtol=0, atol=1e-6)       # read_wav removes the mean


def test_the_largest_supported_response_and_the_first_unsupported():
    import unet_rir_amd as U
    with pytest.raises(ValueError, match="supported"):
        U.auralize_path(torch.zeros(1, 2, 16385, device="cuda"), torch.zeros(300, device="cuda"), [0, 100])

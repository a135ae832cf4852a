"""`AuralizeStream` (csrc/auralize_fft.hip) on the device, held to the one-shot kernels with ==.

The yardstick is code of this tree that is itself held to its fp64 definition (tests/test_auralize_fft_gpu.py,
tests/test_auralize_path_gpu.py): the concatenation of every `push` and the `flush` must be `auralize(rir, x, method="fft")` bit for bit,
and after an update at block j the blocks from j on must be `auralize_path` with the old response at jP and the new one at (j+1)P.
The block is fixed at P = 2048, so the shapes are those around the partition (K), ring (S = Q + max_blocks - 1) and push edges.  The
state lies between canaries, and every `out` in a canary-filled buffer off 8-byte alignment.

1. stationary ==, uniform and integer data, total blocks 2 S + 1 (the ring wraps twice), single-block, full and mixed pushes;
2. chunks of 1, 2047, 2049, 5000, 0 and max_blocks P + 1 samples: the same bits, and samples_in / samples_out right after every call;
3. updates: == piecewise, and against fp64 within auralize_path_ref.bound and e <= 4 e(fp32 restatement) + 2^-22;
4. bits independent of run, B, the row's place, shared or per-row dry, max_blocks, the chunking and a larger state; reset;
5. exactly the advertised state; 6. a captured single-block push replayed 2 S + 1 times, an update between replays followed;
7. scripts/auralize.py --stream writes the bytes of --method fft; 8. limits."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from auralize_fft_ref import bound as stationary_bound
from auralize_path_ref import bound as path_bound
from auralize_path_ref import nodes64, path_ref64, peak_error
from auralize_ref import convolve_ref
from auralize_stream_ref import P, run

pytestmark = pytest.mark.gpu

CANARY = 12345.678          # no integer, so no sum of integer data
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(B, K, N, kind, seed=0):
    """device h [B, K], x [B, N]: uniform in [-1, 1], or integers |h| <= 3, |x| <= 7"""
    g = torch.Generator(device="cuda")
    g.manual_seed(1000 * seed + K + N)
    if kind == "int":
        return (torch.randint(-3, 4, (B, K), generator=g, device="cuda").float(), torch.randint(-7, 8, (B, N), generator=g, device="cuda").float())
    return (torch.rand((B, K), generator=g, device="cuda") * 2 - 1, torch.rand((B, N), generator=g, device="cuda") * 2 - 1)


def _stream(h, layout, mb, pad=4096):
    """an AuralizeStream whose state is exactly state_bytes between canaries -> (stream, check)"""
    import unet_rir_amd as U
    B, K = h.shape
    need = U.ops.auralize_stream_state_bytes(B, K, B if layout == "rows" else 1, mb)
    buf = torch.full((pad + need + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    s = U.AuralizeStream(h, layout, mb, state=buf[pad:pad + need])
    assert s.state_bytes == need

    def check():
        assert torch.all(buf[:pad] == 0xA5) and torch.all(buf[pad + need:] == 0xA5), "written outside the advertised state"
    return s, check


def _push(s, chunk):
    """push into the middle of a canary-filled buffer that puts `out` off 8-byte alignment; nothing around it written, all of it written"""
    n_in, n_out, pend = s.samples_in, s.samples_out, s.samples_in - s.samples_out
    m = (pend + chunk.shape[-1]) // P * P
    buf = torch.full((1 + s.B * m + 64,), CANARY, dtype=torch.float32, device="cuda")
    out = buf[1:1 + s.B * m].view(s.B, m)
    got = s.push(chunk, out=out)
    assert got is out
    assert s.samples_in == n_in + chunk.shape[-1] and s.samples_out == n_out + m and s.samples_in - s.samples_out < P
    assert buf[0] == CANARY and torch.all(buf[1 + s.B * m:] == CANARY), "written outside out"
    assert not torch.any(out == CANARY), "a sample of out was not written"
    return out


def _feed(s, x, sizes):
    """x cut into chunks of `sizes` (cycled) -> the concatenation of the pushes and the flush"""
    parts, pos, k, N = [], 0, 0, x.shape[-1]
    while pos < N:
        n = min(sizes[k % len(sizes)], N - pos)
        k += 1
        parts.append(_push(s, x[..., pos:pos + n]))
        pos += n
    assert s.samples_in == N
    want_tail = N + s.K - 1 - s.samples_out
    tail = s.flush()
    assert tail.shape == (s.B, want_tail) and s.samples_in == 0 and s.samples_out == 0
    return torch.cat(parts + [tail], dim=1)


@pytest.mark.parametrize("mb", (1, 2, 8))
@pytest.mark.parametrize("K", (1, 2047, 2048, 2049, 4097, 9600, 16384))
def test_stationary_stream_equals_the_one_shot_form_bit_for_bit(K, mb):
    import unet_rir_amd as U
    S = -(-K // P) + mb - 1
    total = 2 * S + 1
    N = total * P
    sizes = [n * P for n in (1, mb, max(1, mb // 2), mb, 1, 1, mb)]      # single-block, full and mixed pushes
    for kind in ("uniform", "int"):
        h3, x3 = _data(3, K, N, kind)
        for B in (1, 3):
            for layout in ("shared", "rows"):
                h = h3[:B].contiguous()
                x = x3[:B].contiguous() if layout == "rows" else x3[0].contiguous()
                want = U.auralize(h, x, method="fft", length="full")
                s, check = _stream(h, layout, mb)
                got = _feed(s, x, sizes)
                check()
                assert got.shape == want.shape and torch.equal(got, want), (kind, B, layout)


@pytest.mark.parametrize("mb", (1, 2, 8))
@pytest.mark.parametrize("layout", ("shared", "rows"))
def test_arbitrary_chunk_lengths_give_the_same_bits(layout, mb):
    import unet_rir_amd as U
    K, B = 4097, 3
    N = (2 * (3 + mb - 1) + 1) * P - 777
    h, x = _data(B, K, N, "uniform", seed=1)
    if layout == "shared":
        x = x[0].contiguous()
    want = U.auralize(h, x, method="fft", length="full")
    s, check = _stream(h, layout, mb)
    got = _feed(s, x, (1, 2047, 2049, 5000, 0, mb * P + 1, 3, 2 * P, 4095, mb * P, 1 << 30))
    check()
    assert torch.equal(got, want)
    s2, _ = _stream(h, layout, mb)
    assert torch.equal(_feed(s2, x, (N,)), want)                                # one chunk: several kernel calls inside
    empty = s2.push(x[..., :0])
    assert empty.shape == (B, 0) and s2.flush().shape == (B, 0)                 # a stream that took no input has no tail


# ---- updates.  A scenario is a list of steps: ("push", samples) or ("update", index into the responses, 0 = junk that must be lost)
K_UP, B_UP, MB_UP = 2049, 2, 3
N_UP = 9 * P - 300
SCENARIOS = {
    "before_the_first_push": [("update", 1), ("push", 2 * P), ("push", P), ("push", 1 << 30)],
    "adjacent_blocks": [("push", 3 * P), ("update", 1), ("push", P), ("update", 2), ("push", 2 * P), ("push", 1 << 30)],
    "mid_sequence": [("push", 2 * P), ("push", 3 * P), ("update", 1), ("push", 3 * P), ("push", 1 << 30)],
    "the_last_of_two_wins": [("push", 2 * P), ("update", 0), ("update", 1), ("push", 2 * P), ("push", 1 << 30)],
    "samples_pending": [("push", 2 * P + 700), ("update", 1), ("push", 3 * P), ("push", 1 << 30)],
    "within_the_first_Q_blocks": [("push", P), ("update", 1), ("push", 1 << 30)],
    "pending_at_flush": [("push", 1 << 30), ("update", 1)],
}


@functools.lru_cache(maxsize=None)
def _update_data():
    rng = np.random.default_rng(17)
    hs = rng.uniform(-1, 1, size=(3, B_UP, K_UP)).astype(np.float32)
    x = rng.uniform(-1, 1, size=(N_UP,)).astype(np.float32)
    hs.setflags(write=False)
    x.setflags(write=False)
    return hs, x


@functools.lru_cache(maxsize=None)
def _segment64(u, j):
    """fp64, computed once per (response pair, fade block): (path_ref64, bound) of the nodes (h_u at jP, h_{u+1} at (j+1)P)"""
    hs, x = _update_data()
    hh = np.stack([hs[u], hs[u + 1]], axis=1)
    times = [j * P, (j + 1) * P]
    nodes = nodes64(hh, x)
    return path_ref64(hh, x, times, nodes=nodes), path_bound(hh, x, times, nodes)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_updates_are_the_path_form_piecewise(name):
    import unet_rir_amd as U
    hs, x = _update_data()
    hd, xd = torch.from_numpy(np.array(hs)).cuda(), torch.from_numpy(np.array(x)).cuda()
    junk = torch.ones_like(hd[0])
    s, check = _stream(hd[0].contiguous(), "shared", MB_UP)
    parts, pos, at = [], 0, []
    for what, arg in SCENARIOS[name]:
        if what == "update":
            s.update(junk if arg == 0 else hd[arg].contiguous())
            if arg:
                assert s.samples_out % P == 0
                at.append(s.samples_out // P)
        else:
            n = min(arg, N_UP - pos)
            parts.append(_push(s, xd[pos:pos + n]))
            pos += n
    assert pos == N_UP
    parts.append(s.flush())
    check()
    got = torch.cat(parts, dim=1)
    L = N_UP + K_UP - 1
    assert got.shape == (B_UP, L)
    # == piecewise: blocks [0, j_1) of the stationary form for h_0, blocks [j_u, j_{u+1}) of the path (h_{u-1} at j_u P, h_u a block on)
    edges = at + [1 << 30]
    still = U.auralize(hd[0].contiguous(), xd, method="fft")
    hi = min(at[0] * P, L)
    assert torch.equal(got[:, :hi], still[:, :hi])
    ref, lim = np.zeros((B_UP, L)), np.zeros((B_UP, L))
    ref[:, :hi] = convolve_ref(hs[0], x)[0][:, :hi]
    lim[:, :hi] = stationary_bound(hs[0], x, P)[:, :hi]
    for u, j in enumerate(at):
        lo, hi = j * P, min(edges[u + 1] * P, L)
        want = U.auralize_path(torch.stack([hd[u], hd[u + 1]], dim=1).contiguous(), xd, times=[j * P, (j + 1) * P])
        assert torch.equal(got[:, lo:hi], want[:, lo:hi]), (name, u, j)
        r64, b64 = _segment64(u, j)
        ref[:, lo:hi], lim[:, lo:hi] = r64[:, lo:hi], b64[:, lo:hi]
    # and against the definition: within the bound, and at most 4 times the fp32 restatement's error plus 2^-22
    g = got.cpu().numpy()
    restated = run(hs[0], x_blocks(x), 1, MB_UP, (MB_UP,), tuple((j, hs[u + 1]) for u, j in enumerate(at)),
                   flush_blocks=2)[:, :L]
    f1 = float(np.max(np.abs(g.astype(np.float64) - ref) / lim))
    e, er = peak_error(g, ref), peak_error(restated, ref)
    f2 = float(np.max(e / (4.0 * er + 2.0 ** -22)))
    print(f"{name}: fades at blocks {at}; error / bound = {f1:.3g}, peak error / (4 restatement's + 2^-22) = {f2:.3g}")
    assert f1 <= 1.0 and f2 <= 1.0


def x_blocks(x):
    """x followed by zeros up to a whole number of blocks (the restatement takes whole blocks; zeros are what flush pushes)"""
    n = -(-x.shape[0] // P) * P
    return np.concatenate([x, np.zeros(n - x.shape[0], dtype=x.dtype)])


def test_bits_do_not_depend_on_run_batch_layout_max_blocks_chunking_or_state():
    import unet_rir_amd as U
    K, B, N = 4097, 3, 11 * P + 5
    h, x = _data(B, K, N, "uniform", seed=2)
    h1 = _data(B, K, N, "uniform", seed=3)[0]

    def play(hh, h_new, xx, layout, mb, sizes, stream=None):
        s = U.AuralizeStream(hh, layout, mb) if stream is None else stream
        a = s.push(xx[..., :3 * P + 100])
        s.update(h_new)
        rest = xx[..., 3 * P + 100:]
        parts, pos, k = [a], 0, 0
        while pos < rest.shape[-1]:
            n = min(sizes[k % len(sizes)], rest.shape[-1] - pos)
            k += 1
            parts.append(s.push(rest[..., pos:pos + n]))
            pos += n
        return torch.cat(parts + [s.flush()], dim=1)

    full = play(h, h1, x, "rows", 2, (P, 2 * P, 333))
    assert full.shape == (B, N + K - 1)
    assert torch.equal(play(h, h1, x, "rows", 2, (P, 2 * P, 333)), full)                                # two runs
    for b in range(B):                                                                                  # a row alone
        assert torch.equal(play(h[b:b + 1], h1[b:b + 1], x[b:b + 1], "rows", 2, (P, 2 * P, 333)), full[b:b + 1])
    assert torch.equal(play(h.flip(0).contiguous(), h1.flip(0).contiguous(), x.flip(0).contiguous(), "rows", 2, (P,)), full.flip(0))
    sh = play(h, h1, x[1].contiguous(), "shared", 2, (P, 2 * P, 333))
    assert torch.equal(sh, play(h, h1, x[1].repeat(B, 1), "rows", 2, (P, 2 * P, 333))) and torch.equal(sh[1], full[1])
    for mb, sizes in ((1, (P,)), (8, (8 * P,)), (3, (1, 5000, 0, 2047)), (64, (1 << 30,))):            # max_blocks and the chunking
        assert torch.equal(play(h, h1, x, "rows", mb, sizes), full), (mb, sizes)
    need = U.ops.auralize_stream_state_bytes(B, K, B, 2)
    big = torch.full((2 * need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    s = U.AuralizeStream(h, "rows", 2, state=big)
    assert torch.equal(play(h, h1, x, "rows", 2, (P, 2 * P, 333), stream=s), full)                      # a larger state
    assert torch.all(big[need:] == 0xA5), "more than the advertised state was touched"
    # reset: the same input gives the bits of a fresh stream - no stale ring slot, carry or pending fade leaks
    s.push(x[..., :5 * P + 9])
    s.update(h1)
    s.reset()
    assert s.samples_in == 0 and s.samples_out == 0
    stationary = U.auralize(h1, x, method="fft")                                                        # the latest response given
    assert torch.equal(torch.cat([s.push(x), s.flush()], dim=1), stationary)
    s.reset(h)
    assert torch.equal(play(h, h1, x, "rows", 2, (2 * P,), stream=s), full)


@pytest.mark.parametrize("layout", ("shared", "rows"))
def test_exactly_the_advertised_state_is_used(layout):
    """The C entry points on a state of exactly state_bytes between canaries, after init, update, push and a push of zeros; one byte less
    and a misaligned state refused without a write."""
    import unet_rir_amd as U
    B, K, mb, pad = 3, 4097, 2, 4096
    rows = B if layout == "rows" else 1
    h, x = _data(B, K, 2 * P, "int", seed=4)
    xd = x if rows > 1 else x[0].contiguous()
    need = U.ops.auralize_stream_state_bytes(B, K, rows, mb)
    assert need == 64 + 16384 * (2 * B * 3 + rows * 4) + 8192 * rows
    buf = torch.full((pad + need + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    obuf = torch.full((64 + B * 2 * P + 64,), CANARY, dtype=torch.float32, device="cuda")
    out = obuf[64:64 + B * 2 * P].view(B, 2 * P)
    lib = U._lib.lib()
    st, stream = buf.data_ptr() + pad, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    for state, size in ((st, need - 1), (st + 8, need)):
        assert lib.unetrir_auralize_stream_init(C.c_void_p(state), size, p(h), B, K, rows, mb, stream) == 10001
        assert lib.unetrir_auralize_stream_update(C.c_void_p(state), size, p(h), B, K, rows, mb, stream) == 10001
        assert lib.unetrir_auralize_stream_push(C.c_void_p(state), size, B, K, rows, mb, p(xd), 2 * P if rows > 1 else 0, p(out), 2 * P, 2,
                                                stream) == 10001
    torch.cuda.synchronize()
    assert torch.all(buf == 0xA5) and torch.all(obuf == CANARY), "a refused call wrote"

    def around(what):
        torch.cuda.synchronize()
        assert torch.all(buf[:pad] == 0xA5) and torch.all(buf[pad + need:] == 0xA5), f"{what} wrote outside the advertised state"
        assert torch.all(obuf[:64] == CANARY) and torch.all(obuf[64 + B * 2 * P:] == CANARY), f"{what} wrote outside out"

    assert lib.unetrir_auralize_stream_init(C.c_void_p(st), need, p(h), B, K, rows, mb, stream) == 0
    around("init")
    assert lib.unetrir_auralize_stream_update(C.c_void_p(st), need, p(h), B, K, rows, mb, stream) == 0
    around("update")
    assert lib.unetrir_auralize_stream_push(C.c_void_p(st), need, B, K, rows, mb, p(xd), 2 * P if rows > 1 else 0, p(out), 2 * P, 2, stream) == 0
    around("push")
    assert not torch.any(out == CANARY)
    want = U.auralize(h, xd, method="fft")                  # the update was to the same response: a fade from h to h over block 0
    assert torch.equal(out[:, P:], want[:, P:2 * P])
    assert lib.unetrir_auralize_stream_push(C.c_void_p(st), need, B, K, rows, mb, None, 0, p(out), 2 * P, 2, stream) == 0
    around("a push of zeros")
    assert torch.equal(out, want[:, 2 * P:4 * P])


def test_a_captured_push_replays_the_next_block_and_follows_an_update():
    import unet_rir_amd as U
    B, K, mb = 3, 4097, 1
    S = 3 + mb - 1
    total = 2 * S + 1
    h, x = _data(B, K, total * P, "uniform", seed=5)
    h1 = _data(B, K, 1, "uniform", seed=6)[0]
    x = x[0].contiguous()
    jup = 4
    want0 = U.auralize(h, x, method="fft")
    want1 = U.auralize_path(torch.stack([h, h1], dim=1).contiguous(), x, times=[jup * P, (jup + 1) * P])
    state = U.ops.AuralizeStreamState(h.device, B, K, 1, mb)
    dry = torch.zeros(P, device="cuda")
    out = torch.zeros(B, P, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        U.ops.auralize_stream_init(state, h)
        U.ops.auralize_stream_push_f32(state, dry, out)     # on the side stream, outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            U.ops.auralize_stream_push_f32(state, dry, out)
    torch.cuda.current_stream().wait_stream(side)
    U.ops.auralize_stream_init(state, h)                    # what the warm-up and the capture may have rendered is forgotten
    got = []
    for j in range(total):
        if j == jup:
            U.ops.auralize_stream_update(state, h1)         # outside the graph, between two replays
        dry.copy_(x[j * P:(j + 1) * P])
        out.fill_(CANARY)
        g.replay()
        got.append(out.clone())
    torch.cuda.synchronize()
    got = torch.cat(got, dim=1)
    assert torch.equal(got[:, :jup * P], want0[:, :jup * P]), "the replays before the update"
    assert torch.equal(got[:, jup * P:], want1[:, jup * P:total * P]), "the replays from the update on"


def test_the_script_streams_the_bytes_of_the_fft_method(tmp_path):
    """scripts/auralize.py --stream: the files of --method fft, byte for byte, from a dry file read in chunks (what --stream refuses is
    in tests/test_auralize_stream_io.py: it needs no device)"""
    from unet_rir_amd.auralize import write_wav
    sr, dur = 8000, 0.3
    rng = np.random.default_rng(23)
    rirs = tmp_path / "rirs"
    rirs.mkdir()
    for name in ("a", "b", "c"):
        write_wav(str(rirs / (name + ".wav")), rng.uniform(-0.5, 0.5, int(sr * dur)).astype(np.float32), sr)
    write_wav(str(tmp_path / "dry.wav"), (rng.uniform(-0.5, 0.5, 3 * P + 1234) + 0.25).astype(np.float32), sr)
    base = [sys.executable, os.path.join(ROOT, "scripts", "auralize.py"), "--rirs", str(rirs), "--dry", str(tmp_path / "dry.wav"), "--sr", str(sr),
            "--duration", str(dur), "--batch", "2"]
    for extra, out in ((["--method", "fft"], "whole"), (["--stream", "--chunk-ms", "100"], "stream")):
        run_ = subprocess.run(base + extra + ["--out", str(tmp_path / out)], capture_output=True, text=True, timeout=120)
        assert run_.returncode == 0, run_.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "stream")) == ["a.wav", "b.wav", "c.wav"]
    for name in ("a.wav", "b.wav", "c.wav"):
        whole, streamed = (tmp_path / "whole" / name).read_bytes(), (tmp_path / "stream" / name).read_bytes()
        assert len(whole) == 58 + 4 * (3 * P + 1234 + int(sr * dur) - 1) and streamed == whole, name


def test_the_largest_supported_response_and_the_first_unsupported():
    import unet_rir_amd as U
    s = U.AuralizeStream(torch.zeros(1, 16384, device="cuda"), max_blocks=64)
    assert s.block == P and s.state_bytes == 64 + 16384 * (2 * 8 + 71) + 8192
    with pytest.raises(ValueError, match="supported"):
        U.AuralizeStream(torch.zeros(1, 16385, device="cuda"))
    with pytest.raises(ValueError, match="max_blocks"):
        U.AuralizeStream(torch.zeros(1, 50, device="cuda"), max_blocks=65)
    with pytest.raises(ValueError, match="blocks"):
        U.ops.auralize_stream_push_f32(s._state, None, torch.zeros(1, 65 * P, device="cuda"))

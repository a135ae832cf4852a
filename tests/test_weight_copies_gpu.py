"""The weight layout kernels of csrc/weights.hip against a restatement of their contract, BIT for bit: the fp32 transpose, the two
per-layer bf16 work copies and the batched refresh with its four routes (the fused 64 x 64 one-read kernel, the flat 8-wide copy,
the element-wise padded copy, the 32 x 32 transposing kernel) and its two writers of the packed stride-2 copy.  The restatement
(tests/reduction_ref.py: work_copy_ref, packed_ref - the latter from the prose of include/unetrir.h, not from a kernel) is proven
on mutants by tests/test_reduction_ref.py.  Every destination lies in a NaN canary band; every master carries exact bf16 ties of
both parities, +-0, an fp32 subnormal and a value near the top of the range.

Contract pinned here for a descriptor with same == NULL and packed_s2 != NULL: the packed copy IS written (T == 9, C % 16 == 0),
whatever other destinations the descriptor carries; with T != 9 the packed destination stays as given."""
import functools

import pytest
import torch

import exact_data as X
import reduction_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64                     # canary elements on each side of a destination (a multiple of 8: 16-byte alignment is kept)
NAN = float("nan")
GIVEN = 1.5                  # what a packed destination that must not be written holds

# N, T, C, Cp, Np
SHAPES = [(1, 1, 1, 8, 8), (5, 9, 3, 8, 8), (33, 9, 31, 32, 40), (72, 9, 40, 40, 72),
          (136, 9, 264, 264, 136),        # 9 * 5 * 9 = 405 transposing tiles: more than the 256-block grid; generic routes
          (64, 1, 64, 64, 64),            # fused, T = 1
          (64, 9, 64, 64, 64),            # fused and packed: half of the four 32-blocks used
          (192, 9, 128, 128, 192),        # the second 128-group half filled
          (64, 36, 64, 64, 64),           # fused, T != 9: the packed destination stays as given
          (512, 9, 512, 512, 512)]        # 576 fused tiles (> 256); 9216 blocks' worth for cast_weight (> its 8192-block cap)
ROUTES = ("both", "same", "transposed", "offset", "none")


def fused_eligible(shape):
    N, T, C, Cp, Np = shape
    return C == Cp and N == Np and C % 64 == 0 and N % 64 == 0


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    yield unet_rir_amd
    print("\nexact comparisons of this process so far:", X.STATS)


@functools.lru_cache(maxsize=None)
def ref(shape):
    """(master, same, transposed, packed or None, ties) of a shape on the CPU, computed once."""
    N, T, C, Cp, Np = shape
    w, ties = RR.master(N, T, C)
    same, tr = RR.work_copy_ref(w, Cp, Np)
    pk = RR.packed_ref(w, N, C) if T == 9 and fused_eligible(shape) else None
    return w, same, tr, pk, ties


def band(numel, dtype, fill=NAN):
    """A destination of numel elements inside a NaN band: (whole buffer, the destination as a view)."""
    buf = torch.full((numel + 2 * PAD,), NAN, dtype=dtype, device=DEV)
    buf[PAD:PAD + numel] = fill
    return buf, buf[PAD:PAD + numel]


def band_intact(buf):
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all())


class Layer:
    """One descriptor of a cast table: the master on the device (one float off a 16-byte boundary for route "offset") and
    its destinations, each in a band.  Destinations start as NaN; the packed one as zeros (the caller's duty) where the
    layout is defined for T == 9, as GIVEN where T != 9 (it must not be touched)."""

    def __init__(self, U, shape, route, packed=True):
        N, T, C, Cp, Np = self.shape = shape
        self.route = route
        w = ref(shape)[0]
        self.wbuf = torch.zeros(w.numel() + 8, dtype=torch.float32, device=DEV)
        o = 1 if route == "offset" else 0
        self.w = self.wbuf[o:o + w.numel()]
        self.w.copy_(w.reshape(-1))
        assert self.w.data_ptr() % 16 == (4 if o else 0)
        self.same_buf, self.same = band(N * T * Cp, torch.bfloat16) if route in ("both", "same", "offset") else (None, None)
        self.tr_buf, self.tr = band(C * T * Np, torch.bfloat16) if route in ("both", "transposed", "offset") else (None, None)
        ne = U.ops.conv3x3s2_packed_elems(N, C) if packed else 0
        self.pk_written = bool(ne) and T == 9
        self.pk_buf, self.pk = band(ne, torch.bfloat16, 0.0 if T == 9 else GIVEN) if ne else (None, None)

    def entry(self):
        N, T, C, Cp, Np = self.shape
        return (self.w, self.same, self.tr, N, T, C, Cp, Np, self.pk)

    def verify(self, what):
        w, same, tr, pk, ties = ref(self.shape)
        assert torch.equal(self.w.cpu(), w.reshape(-1)), f"{what}: the master changed"
        n = 0
        if self.same is not None:
            RR.assert_bits(self.same, same.reshape(-1), f"{what} same")
            assert band_intact(self.same_buf), what
            n += 1
        if self.tr is not None:
            RR.assert_bits(self.tr, tr.reshape(-1), f"{what} transposed")
            assert band_intact(self.tr_buf), what
            n += 1
        if self.pk is not None:
            want = pk if self.pk_written else torch.full_like(self.pk, GIVEN).cpu()
            assert want.numel() == self.pk.numel()
            RR.assert_bits(self.pk, want, f"{what} packed")               # unmapped blocks: still the caller's zeros
            assert band_intact(self.pk_buf), what
            n += 1
        return n

    def outputs(self):
        return [t for t in (self.same_buf, self.tr_buf, self.pk_buf) if t is not None]


def routes_of(shape):
    return ROUTES if fused_eligible(shape) else ("both", "same", "transposed", "none")


def run_table(U, layers):
    U.ops.cast_weights_batched(U.ops.make_cast_table([l.entry() for l in layers], DEV))
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_single_entry_points(U, shape):
    """unetrir_transpose_weight_f32 against a plain permute, unetrir_cast_weight_bf16 and unetrir_transpose_cast_weight_bf16
    against work_copy_ref."""
    ops = U.ops
    N, T, C, Cp, Np = shape
    w, same, tr, _, ties = ref(shape)
    X.note_ties(ties)
    assert ties > 0
    wd = w.to(DEV)
    tbuf, t32 = band(C * T * N, torch.float32)
    ops.transpose_weight(wd, t32, N, T, C)
    sbuf, s16 = band(N * T * Cp, torch.bfloat16)
    ops.cast_weight_bf16(wd, s16, N, T, C, Cp)
    rbuf, r16 = band(C * T * Np, torch.bfloat16)
    ops.transpose_cast_weight_bf16(wd, r16, N, T, C, Np)
    torch.cuda.synchronize()
    RR.assert_bits(t32, w.permute(2, 1, 0).contiguous().reshape(-1), f"{shape} transpose_weight_f32")
    RR.assert_bits(s16, same.reshape(-1), f"{shape} cast_weight_bf16")
    RR.assert_bits(r16, tr.reshape(-1), f"{shape} transpose_cast_weight_bf16")
    assert band_intact(tbuf) and band_intact(sbuf) and band_intact(rbuf)
    assert torch.equal(wd.cpu(), w)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_batched_routes_layer_by_layer(U, shape):
    """Every route of unetrir_cast_weights_batched_bf16 for one shape, one table per route."""
    compared = 0
    for route in routes_of(shape):
        layer = Layer(U, shape, route, packed=route != "none")
        run_table(U, [layer])
        compared += layer.verify(f"{shape} route {route}")
    assert compared >= 4
    X.note_ties(ref(shape)[4])


@pytest.mark.parametrize("shape", [(64, 9, 64, 64, 64), (192, 9, 128, 128, 192), (64, 36, 64, 64, 64), (72, 9, 48, 48, 72)],
                         ids=lambda s: "-".join(map(str, s)))
def test_packed_destination_without_same(U, shape):
    """same == NULL with a packed destination: the packed copy is written all the same (T == 9, C % 16 == 0) - with the transposed
    copy or with no other destination at all - and it equals what the fused kernel writes; T != 9: it stays as given.  A layer for
    which no packed layout is defined (N not a multiple of 64) carries no packed destination and is unaffected."""
    N, T, C, Cp, Np = shape
    layers = [Layer(U, shape, route) for route in ("transposed", "none", "both")]
    run_table(U, layers)
    for layer in layers:
        layer.verify(f"{shape} route {layer.route} + packed")
    if fused_eligible(shape):
        assert all(l.pk is not None for l in layers)
        assert torch.equal(layers[0].pk_buf.view(torch.int16), layers[2].pk_buf.view(torch.int16))
        assert torch.equal(layers[1].pk_buf.view(torch.int16), layers[2].pk_buf.view(torch.int16))
        assert layers[0].pk_written == (T == 9)
    else:
        assert all(l.pk is None for l in layers)


def test_one_mixed_table(U):
    """Every shape and route as one table in ONE call (a layer per blockIdx.y): equal to the restatement and, buffer for buffer
    (canary bands included), to the same layers refreshed one table each."""
    cases = [(shape, route) for shape in SHAPES for route in routes_of(shape)]
    mixed = [Layer(U, shape, route, packed=route != "none") for shape, route in cases]
    run_table(U, mixed)
    compared = 0
    for layer in mixed:
        compared += layer.verify(f"mixed table {layer.shape} route {layer.route}")
        single = Layer(U, layer.shape, layer.route, packed=layer.route != "none")
        run_table(U, [single])
        for a, b in zip(layer.outputs(), single.outputs()):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (layer.shape, layer.route)
        del single
    assert compared > 2 * len(SHAPES)
    print(f"mixed table: {len(mixed)} layers, {compared} destinations compared")

"""CPU proof of the criteria of tests/reduction_ref.py.  The GPU tests can only show that the kernels pass; here the split-K
reduction and the weight work copies are emulated in fp32 torch arithmetic on the sweep's OWN data, the true result must pass and
each of ten realistic mutants - a slab dropped, a slab added twice, a wrong slab stride, an unwritten tail, a forgotten reg * w,
half-precision partial sums, a truncating cast, a transpose with N and C swapped, an unwritten pad, two lanes of the packed
order exchanged - must be rejected.  The packed order restated from include/unetrir.h is held to the library's own element count
and to the blocks no channel maps to."""
import pytest
import torch

import exact_data as X
import reduction_ref as RR
import streaming_check as S

NAN = float("nan")
# cases of the sweep that the emulation runs: every form, tails of 1, 3 and 3 outputs, the deepest loops of both bodies
PROOF = [(1, 5), (3, 255), (5, 63), (9, 257), (33, 260), (57, 257), (225, 252), (300, 1000)]


def _emulated(data, variant, i, **mut):
    """Case i of the sweep through RR.emulate with the form the library would take for aligned (or, variant "offset", one float
    off) pointers.  mut: drop / twice (a slab index), stride, tail (leave the last n % 4 outputs at the canary), noreg, acc."""
    nsplit, n = RR.CASES[i]
    mis = variant == "offset"
    kind = RR.expected_kind(nsplit, n, 4 if mis else 0, 4 if mis else 0, 4 if mis else 0)
    flat = RR.pool(data)[0][RR.pool_offset(i, mis):]
    w = RR.pool(data)[1][(1 if mis else 0):][:n]
    reg = 0.0 if mut.get("noreg") else RR.reg_of(data, variant)
    stride = mut.get("stride", n)
    if "drop" in mut or "twice" in mut:
        order = [k for k in range(nsplit) if k != mut.get("drop")] + ([mut["twice"]] if "twice" in mut else [])
        flat = flat.as_strided((nsplit, n), (stride, 1))[order].contiguous().reshape(-1)
        nsplit = len(order)
    got = RR.emulate(flat, nsplit, n, stride, reg, w, kind, mut.get("acc", torch.float32))
    if mut.get("tail"):
        got[n - n % 4:] = NAN
    return got, kind


@pytest.mark.parametrize("data", ["int", "uniform"])
@pytest.mark.parametrize("variant", RR.VARIANTS)
def test_true_reduction_is_accepted_and_every_mutant_rejected(data, variant, capsys):
    kinds = []
    for case in PROOF:
        i = RR.CASES.index(case)
        nsplit, n = case
        what = f"{data} {variant} nsplit {nsplit} n {n}"
        good, kind = _emulated(data, variant, i)
        kinds.append(kind)
        RR.check_reduction(good, data, variant, i, what, kernel="(cpu proof)")
        # the assembled reference IS reduce_ref on the case's slabs
        mis = variant == "offset"
        ref, bound = RR.reduce_ref(RR.slabs(data, i, mis).double(), RR.reg_of(data, variant),
                                   None if variant == "noreg" else RR.pool(data)[1][(1 if mis else 0):][:n].double())
        cref, cbound, _ = RR.case_ref(data, variant, i)
        assert torch.equal(ref, cref) and torch.equal(bound, cbound)
        mutants = {"slab stride n + 1": dict(stride=n + 1), "fp16-width partial sums": dict(acc=torch.float16)}
        if nsplit > 1:
            mutants["one slab dropped"] = dict(drop=nsplit // 2)
            mutants["the last slab dropped"] = dict(drop=nsplit - 1)
        mutants["one slab added twice"] = dict(twice=nsplit // 2)
        if n % 4:
            mutants["the last n % 4 outputs left at the canary"] = dict(tail=True)
        if variant != "noreg":
            mutants["reg * w omitted"] = dict(noreg=True)
        if nsplit == 1:
            del mutants["slab stride n + 1"]                                       # one slab: no stride
        if nsplit < 9:
            del mutants["fp16-width partial sums"]                                 # sums of a few integers below 2048: fp16 holds them
        for name, kw in mutants.items():
            got, _ = _emulated(data, variant, i, **kw)
            wrong = int((got.double() != good.double()).sum()) if not kw.get("tail") else n % 4
            assert wrong > 0, (what, name)
            assert not RR.accepts(RR.check_reduction, got, data, variant, i, what, "(cpu proof)"), f"{what}: mutant '{name}' accepted"
    assert set(kinds) == ({1, 2, 4, 8} if variant == "offset" else {0, 1, 2, 4, 8})
    with capsys.disabled():
        print(f"\n  reduction criterion ({data}, {variant}): {len(PROOF)} emulated cases accepted, every mutant rejected")


def test_the_sweep_enters_every_form_with_and_without_a_tail():
    """From nsplit, n and the alignment alone: what tests/test_reductions_gpu.py asserts again with the addresses it uses."""
    kinds = [(RR.expected_kind(s, n, 0, 0, 0), n) for s, n in RR.CASES]
    RR.assert_every_form_is_entered(kinds)
    assert RR.expected_kind(32, 32512, 0, 0, 0) == 0 and RR.expected_kind(32, 32516, 0, 0, 0) == 8
    assert RR.expected_kind(32, 256, 0, 0, 0) == 0 and RR.expected_kind(31, 256, 0, 0, 0) == 8 and RR.expected_kind(32, 255, 0, 0, 0) == 8
    for addr in ((4, 0, 0), (0, 4, 0), (0, 0, 4)):
        assert RR.expected_kind(64, 256, *addr) == 8                       # any pointer one float off: the wide form is refused
    assert RR.expected_kind(64, 256, 16, 32, None) == 0
    assert [RR.expected_kind(s, 8, 0, 0, 0) for s in (1, 2, 3, 4, 7, 8, 31)] == [1, 2, 2, 4, 4, 8, 8]
    # the 8-deep loops: narrow needs nsplit > 7 G (so only G = 8 can enter it: fewer groups mean nsplit < 2 G), wide nsplit > 224
    assert any(s > 56 and RR.expected_kind(s, n, 0, 0, 0) == 8 for s, n in RR.CASES)
    assert any(s > 224 and RR.expected_kind(s, n, 0, 0, 0) == 0 for s, n in RR.CASES)
    with pytest.raises(AssertionError):
        RR.assert_every_form_is_entered([k for k in kinds if k[0] != 2])


def test_int_data_meets_the_exactness_condition():
    for variant in RR.VARIANTS:
        worst = max(float(RR.case_ref("int", variant, i)[2].max()) for i in range(len(RR.CASES)))
        assert worst < X.EXACT_LIMIT * X.REG
        assert worst > 1e5                                                   # and partial sums do grow past what fp16 holds


# ----------------------------------------------------------------------------------------------------------------------
# work copies
# ----------------------------------------------------------------------------------------------------------------------
def _copy_mutants(w, Cp, Np):
    N, T, C = w.shape
    h = S.bf16_trunc(w.double()).to(torch.bfloat16)
    same, tr = RR.work_copy_ref(w, Cp, Np)
    trunc_same = torch.zeros_like(same); trunc_same[:, :, :C] = h
    trunc_tr = torch.zeros_like(tr); trunc_tr[:, :, :N] = h.permute(2, 1, 0)
    out = {"a truncating bf16 cast (same)": ("same", trunc_same), "a truncating bf16 cast (transposed)": ("tr", trunc_tr)}
    if Cp > C:
        m = same.clone(); m[:, :, C:] = NAN
        out["pad left at the canary (same)"] = ("same", m)
    if Np > N:
        m = tr.clone(); m[:, :, N:] = NAN
        out["pad left at the canary (transposed)"] = ("tr", m)
    if N == C and Np == Cp:                       # N and C swapped: the copy of the master read as [C][T][N]
        out["N and C swapped in the transpose"] = ("tr", RR.work_copy_ref(w.reshape(C, T, N), Np, Cp)[0].reshape(tr.shape))
    else:
        sw = torch.zeros_like(tr)
        flat = RR.work_copy_ref(w, C, N)[0].reshape(-1)
        sw.reshape(-1)[:min(flat.numel(), sw.numel())] = flat[:sw.numel()]
        out["N and C swapped in the transpose"] = ("tr", sw)
    return out


@pytest.mark.parametrize("shape", [(5, 9, 3, 8, 8), (33, 9, 31, 32, 40), (64, 9, 64, 64, 64), (64, 9, 64, 72, 80)])
def test_work_copy_restatement_and_its_mutants(shape):
    N, T, C, Cp, Np = shape
    w, ties = RR.master(N, T, C)
    assert ties > 0
    same, tr = RR.work_copy_ref(w, Cp, Np)
    assert same.shape == (N, T, Cp) and tr.shape == (C, T, Np)
    # against an element-by-element loop over a few coordinates, torch's own conversion (fp32 -> bf16 rounds once) and a permute
    assert torch.equal(same[:, :, :C], w.to(torch.bfloat16)) and torch.equal(tr[:, :, :N], w.to(torch.bfloat16).permute(2, 1, 0))
    assert float(same[:, :, C:].float().abs().sum()) == 0 and float(tr[:, :, N:].float().abs().sum()) == 0
    for n, t, c in [(0, 0, 0), (N - 1, T - 1, C - 1), (N // 2, T // 3, C // 2)]:
        assert float(same[n, t, c]) == float(tr[c, t, n]) == float(S.bf16_rne(w[n, t, c].double()))
    RR.assert_bits(same, same.clone(), "same"); RR.assert_bits(tr, tr.clone(), "transposed")
    for name, (which, m) in _copy_mutants(w, Cp, Np).items():
        want = same if which == "same" else tr
        assert not RR.accepts(RR.assert_bits, m, want, name), f"{shape}: mutant '{name}' accepted"
    # the special values: ties go to even in both directions, zeros keep their sign, the subnormal and the large value survive
    flat, sv = same[:, :, :C].reshape(-1) if Cp == C else None, RR.special_values()
    if flat is not None and flat.numel() >= sv.numel():
        got = flat[:sv.numel()].double()
        assert bool((got[:-8:2] < sv[:-8:2].double()).logical_xor(sv[:-8:2] < 0).all())       # even neighbour below: rounds toward zero
        assert bool((got[1:-8:2] > sv[1:-8:2].double()).logical_xor(sv[1:-8:2] < 0).all())    # odd neighbour below: rounds away
        assert got[-8:].tolist()[2:6] == [2.0 ** -130, -2.0 ** -130, float(torch.tensor(3.0e38).to(torch.bfloat16)), -float(torch.tensor(3.0e38).to(torch.bfloat16))]
        assert torch.signbit(flat[:sv.numel()][-8:]).tolist() == [False, True, False, True, False, True, False, True]


def _lib():
    import unet_rir_amd
    return unet_rir_amd._lib.lib()


@pytest.mark.parametrize("N", [64, 128, 192])
@pytest.mark.parametrize("C", [64, 128])
def test_packed_order_is_a_bijection_into_the_library_s_element_count(N, C):
    idx = RR.packed_index(N, C).reshape(-1)
    elems = int(_lib().unetrir_conv3x3s2_packed_elems(N, C))
    assert elems == RR.packed_elems(N, C) > 0
    assert int(idx.min()) >= 0 and int(idx.max()) < elems
    assert torch.unique(idx).numel() == idx.numel() == N * 9 * C                          # distinct destinations
    # a slower restatement with an explicit loop over the named dimensions, for two taps and a lattice of channel pairs (n, c)
    full = RR.packed_index(N, C)
    for t in (0, 7):
        for n in range(0, N, 5):
            for c in range(0, C, 3):
                m = n % 32
                row = (m & 16) + 8 * ((m // 4) % 2) + 4 * ((m // 8) % 2) + m % 4
                lane = row + 32 * ((c // 8) % 2)
                want = (((((n // 128) * (C // 16) + c // 16) * 9 + t) * 4 + (n // 32) % 4) * 64 + lane) * 8 + c % 8
                assert int(full[n, t, c]) == want


@pytest.mark.parametrize("N", [64, 192])
def test_blocks_no_channel_maps_to_are_exactly_the_zeros_of_packed_ref(N):
    C = 64
    w = RR.master(N, 9, C)[0].clone()
    w[w == 0] = 0.25                                                                       # every mapped element non-zero
    pk = RR.packed_ref(w, N, C).view(-(-N // 128), C // 16, 9, 4, 64 * 8)
    zero = (pk.float() == 0).all(dim=-1)                                                   # [group, chunk, tap, block]
    assert bool(((pk.float() == 0).any(dim=-1) == zero).all())                             # a block is all zero or has none
    unmapped = torch.ones_like(zero)
    for n in range(0, N, 32):
        unmapped[n // 128, :, :, (n // 32) % 4] = False
    assert torch.equal(zero, unmapped)
    assert int(unmapped.sum()) == (C // 16) * 9 * 2 and not bool(unmapped[:-1].any())       # blocks 2 and 3 of the last group


def test_packed_mutant_two_lanes_swapped_is_rejected():
    N, C = 128, 64
    w = RR.master(N, 9, C)[0]
    good = RR.packed_ref(w, N, C)
    RR.assert_bits(good, good.clone(), "packed")
    m = good.clone().view(-1, 64, 8)
    m[5, [3, 4]] = m[5, [4, 3]]
    assert not RR.accepts(RR.assert_bits, m.view(-1), good, "two lanes swapped")
    plain = torch.zeros_like(good)                       # the row permutation forgotten: rows in channel order
    n = torch.arange(N).view(N, 1, 1); t = torch.arange(9).view(1, 9, 1); c = torch.arange(C).view(1, 1, C)
    idx = (((((n // 128) * (C // 16) + c // 16) * 9 + t) * 4 + (n // 32) % 4) * 64 + n % 32 + 32 * ((c // 8) % 2)) * 8 + c % 8
    plain[idx.reshape(-1)] = w.to(torch.bfloat16).reshape(-1)
    assert not RR.accepts(RR.assert_bits, plain, good, "row permutation forgotten")

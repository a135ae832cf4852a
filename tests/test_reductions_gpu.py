"""The fixed-order weight-slab reduction of csrc/splitk_reduce.hip, driven DIRECTLY through unetrir_splitk_reduce_batched with
hand-built descriptors over synthetic slabs: all five forms (narrow with 1 / 2 / 4 / 8 slab groups, wide), the scalar tails of
n % 4 != 0, the alignment fallback, and the three ways a reduction can be launched - alone (the single kernels), inside one call
that holds the whole sweep (the batched kernel, more than 16 descriptors: several launches of mixed forms) and inside the same
call in reverse order.  The three must agree bit for bit, run after run.

Criteria (tests/reduction_ref.py, proven on mutants by tests/test_reduction_ref.py):
  "int"      slabs and w are integers in [-1000, 1000], reg = 0.5: every output is determined - equality with the fp64 sum.
  "uniform"  uniform(-1, 1) * 2^k, k in [-8, 8], reg = 2e-3: |got - ref| <= (nsplit + 1) * 2^-24 * (sum |part| + |reg w|).
No tolerance here is a measured number."""
import pytest
import torch

import exact_data as X
import reduction_ref as RR
import streaming_check as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8                      # floats of NaN canary on each side of every output
NAN = float("nan")
FORMS = {}                   # kind -> [cases, cases with n % 4 != 0] that ran on the device


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    yield unet_rir_amd
    print("\nexact comparisons of this process so far:", X.STATS)
    print("element-wise comparisons of this process so far:")
    for k, v in sorted(S.STATS.items()):
        if k.startswith("splitk_reduce"):
            print(f"  {k}: {v}")
    print("reductions run per form (kind: [cases, of which n % 4 != 0]):", dict(sorted(FORMS.items())))


def _call(U, descs):
    arr = (U._lib.ReduceDesc * max(len(descs), 1))(*descs)
    return U._lib.lib().unetrir_splitk_reduce_batched(arr, len(descs), U.ops._stream())


def _layout(mis):
    """Where every case's output begins in ONE out buffer (floats): 16-byte aligned starts (+ 1 float when `mis`), PAD floats of
    canary around each; the last slot (100 floats) belongs to the descriptor with nsplit == 0."""
    starts, cur = [], PAD
    for _, n in RR.CASES + ((0, 100),):
        starts.append(cur + (1 if mis else 0))
        cur = -(-(cur + n + 1 + PAD) // 4) * 4
    return starts, cur + PAD


def _descs(U, data, variant, pool_d, w_d, out):
    mis = variant == "offset"
    starts, _ = _layout(mis)
    reg = RR.reg_of(data, variant)
    wp = None if variant == "noreg" else w_d.data_ptr() + (4 if mis else 0)
    descs, kinds = [], []
    for i, (nsplit, n) in enumerate(RR.CASES):
        part = pool_d.data_ptr() + 4 * RR.pool_offset(i, mis)
        o = out.data_ptr() + 4 * starts[i]
        descs.append(U._lib.ReduceDesc(part, nsplit, n, o, reg, wp))
        kinds.append(RR.expected_kind(nsplit, n, part, o, wp))
    skipped = U._lib.ReduceDesc(pool_d.data_ptr(), 0, 100, out.data_ptr() + 4 * starts[-1], reg, wp)     # nsplit == 0: nothing to do
    return descs, kinds, skipped


@pytest.mark.parametrize("variant", RR.VARIANTS)
@pytest.mark.parametrize("data", ["int", "uniform"])
def test_sweep_three_launch_forms(U, data, variant):
    mis = variant == "offset"
    pool, w = RR.pool(data)
    pool_d, w_d = pool.to(DEV), w.to(DEV)
    starts, total = _layout(mis)
    assert pool_d.data_ptr() % 16 == 0 and w_d.data_ptr() % 16 == 0
    outs = {}
    for form in ("alone", "batch", "reversed"):
        for run in (0, 1):
            out = torch.full((total,), NAN, dtype=torch.float32, device=DEV)
            assert out.data_ptr() % 16 == 0
            descs, kinds, skipped = _descs(U, data, variant, pool_d, w_d, out)
            if form == "alone":
                for d in descs:
                    assert _call(U, [d]) == 0
            else:
                half = len(descs) // 2
                seq = descs[:half] + [skipped] + descs[half:]
                assert len(seq) > 16
                assert _call(U, seq if form == "batch" else seq[::-1]) == 0
            outs[form, run] = out
    torch.cuda.synchronize()
    # which form each case must have taken, from nsplit, n and the addresses alone
    RR.assert_every_form_is_entered([(k, n) for k, (_, n) in zip(kinds, RR.CASES)], wide=not mis)
    if mis:
        assert 0 not in kinds                     # one float off: the wide form must be refused ...
    else:
        assert kinds[RR.CASES.index((32, 32512))] == 0 and kinds[RR.CASES.index((32, 32516))] == 8
        assert sum(k == 0 for k in kinds) > 50
    for k, (_, n) in zip(kinds, RR.CASES):
        f = FORMS.setdefault(k, [0, 0])
        f[0] += 1
        f[1] += int(n % 4 != 0)
    # the slabs and w are as they were
    assert torch.equal(pool_d.cpu(), pool) and torch.equal(w_d.cpu(), w)
    # the three forms, twice each: bit-identical, canaries included
    first = outs["alone", 0].view(torch.int32)
    for key, o in outs.items():
        assert torch.equal(o.view(torch.int32), first), f"{data} {variant}: {key} differs from the single launches"
    # canaries: everything outside the outputs is still NaN (the slot of the nsplit == 0 descriptor as a whole)
    got = outs["alone", 0].cpu()
    written = torch.zeros(total, dtype=torch.bool)
    for st, (_, n) in zip(starts, RR.CASES):
        written[st:st + n] = True
    assert bool(torch.isnan(got[~written]).all()), f"{data} {variant}: a canary was overwritten"
    assert int(written.sum()) == sum(n for _, n in RR.CASES)
    # ... and the result must be right, case by case
    for i, (nsplit, n) in enumerate(RR.CASES):
        RR.check_reduction(got[starts[i]:starts[i] + n], data, variant, i, f"{data} {variant} nsplit {nsplit} n {n} kind {kinds[i]}",
                           kernel=f"splitk_reduce kind {kinds[i]}")


def _refusal_descs(U, pool_d, w_d, out):
    """name -> descriptor that must be refused; all would be valid reductions of 3 slabs of 40 floats but for the one field."""
    D = U._lib.ReduceDesc
    p, o, w = pool_d.data_ptr(), out.data_ptr() + 4 * PAD, w_d.data_ptr()
    return {"NULL part": D(None, 3, 40, o, 0.0, None), "NULL out": D(p, 3, 40, None, 0.0, None), "nsplit < 0": D(p, -1, 40, o, 0.0, None),
            "n == 0": D(p, 3, 0, o, 0.0, None), "reg != 0 with w == NULL": D(p, 3, 40, o, 0.5, None)}, D(p, 3, 40, o, 0.5, w)


def test_refusals_return_einval_and_write_nothing(U):
    """Every refusal returns before any launch (unetrir_splitk_reduce_batched validates each descriptor before it joins the batch,
    and a batch is flushed only by a later descriptor or the end of the loop), so nothing may be written - not even by a valid
    descriptor in front of the refused one."""
    pool_d, w_d = (t.to(DEV) for t in RR.pool("int"))
    out = torch.full((2, 40 + 2 * PAD), NAN, dtype=torch.float32, device=DEV)
    bad, good = _refusal_descs(U, pool_d, w_d, out[0])
    valid_first = U._lib.ReduceDesc(pool_d.data_ptr(), 3, 40, out[1].data_ptr() + 4 * PAD, 0.0, None)
    lib = U._lib.lib()
    assert lib.unetrir_splitk_reduce_batched((U._lib.ReduceDesc * 1)(good), -1, U.ops._stream()) == RR.EINVAL          # n < 0
    assert lib.unetrir_splitk_reduce_batched(None, 1, U.ops._stream()) == RR.EINVAL                                    # desc == NULL, n > 0
    for name, d in bad.items():
        assert _call(U, [d]) == RR.EINVAL, name
        assert _call(U, [valid_first, d]) == RR.EINVAL, name
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the same buffers through accepted calls: n == 0 descriptors, and the valid ones
    assert lib.unetrir_splitk_reduce_batched(None, 0, U.ops._stream()) == 0
    assert _call(U, []) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert _call(U, [valid_first, good]) == 0
    torch.cuda.synchronize()
    p, w = (t.double() for t in RR.pool("int"))
    want = p[:120].view(3, 40).sum(0)
    X.assert_exact(out[1, PAD:PAD + 40], want, "valid descriptor, no reg")
    X.assert_exact(out[0, PAD:PAD + 40], want + 0.5 * w[:40], "valid descriptor, reg")
    assert bool(torch.isnan(out[:, :PAD]).all()) and bool(torch.isnan(out[:, PAD + 40:]).all())

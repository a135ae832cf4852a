"""The references of tests/spectral_loss_fft_ref.py on the CPU: the fp32 / complex64 restatement against the fp64 truth on every case
of the GPU test (what the kernels' tolerance is made of), and the four one-line mutations, each of which must fail the checks the
kernels are held to - on every case, or the checks would let that mistake through."""
import numpy as np
import pytest

import spectral_loss_fft_ref as FR

WORST = {}


@pytest.mark.parametrize("floor_db", FR.FLOORS)
@pytest.mark.parametrize("T,res", FR.CASES, ids=FR.IDS)
def test_the_restatement_against_fp64(T, res, floor_db):
    tr, rs = FR.truth(T, res, floor_db), FR.restated(T, res, floor_db)
    e = FR.rel_err(rs["dwav"], tr["dwav"])
    want, loss = FR.truth_scalars(tr, 3)
    rel = np.abs(rs["spectral_out"][:2] - want[:2]) / want[:2]
    WORST[(T, res, floor_db)] = float(e.max())
    print(f"T {T} {res} floor {floor_db}: e(restatement) per row {e}, scalars rel {rel} of the bound {FR.scalar_bound(res):.3e}; "
          f"largest e so far {max(WORST.values()):.3e}")
    # an fp32 transform: far below the mutations' 1e-3, and the scalars inside the bound the kernels get
    assert (e < 1e-3).all() and (np.abs(tr["dwav"]).max(axis=1) > 0).all()
    assert (rel <= FR.scalar_bound(res)).all() and abs(rs["loss"] - loss) <= FR.scalar_bound(res) * loss
    assert FR.passes(rs, T, res, floor_db) == (True, True)


@pytest.mark.parametrize("mutation", FR.MUTATIONS)
@pytest.mark.parametrize("floor_db", FR.FLOORS)
@pytest.mark.parametrize("T,res", FR.CASES, ids=FR.IDS)
def test_each_mutation_fails_the_kernels_checks(T, res, floor_db, mutation):
    mu = FR.restated(T, res, floor_db, mutation)
    tr = FR.truth(T, res, floor_db)
    e = FR.rel_err(mu["dwav"], tr["dwav"])
    dwav_ok, scalars_ok = FR.passes(mu, T, res, floor_db)
    print(f"T {T} {res} floor {floor_db} {mutation}: e {e}; dwav check {'passes' if dwav_ok else 'fails'}, scalar check "
          f"{'passes' if scalars_ok else 'fails'}")
    assert not (dwav_ok and scalars_ok)


def test_a_silent_target_counts_nothing_and_a_silent_prediction_counts():
    T, res = FR.CASES[2]
    yp, yt = (np.array(a) for a in FR.inputs(T))
    yt[1] = 0.0
    yp[2] = 0.0
    rs = FR.restatement(yp, yt, res, 60.0, **FR.KW)
    assert rs["spectral_out"][2] == 2 and not rs["dwav"][1].any() and not rs["dwav"][2].any() and rs["dwav"][0].any()
    assert not rs["SC"][1].any() and rs["SC"][2].all()

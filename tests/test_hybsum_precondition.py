"""The cases of tests/_hybsum_cases.py have the properties their names claim, checked on the CPU with
the oracle alone: the planted row of the "between" case has the best sum, stands outside the best 200
of both rankings and is missing from the RRF of two fetched lists; ties are ties; the signed case
ranks a row whose value is +0.0 and rows below 0; and the (1, 0) and (0, 1) identities of the
contract hold in the oracle.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hybsum_cases as hs  # noqa: E402

sp, fc = hs.sp, hs.fc


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_planted_row_wins_the_sum_and_stands_in_neither_fetched_list():
    V, Q, col, qs, planted = hs.between_case()
    assert V.shape == (1300, 16)
    rows, c, kd, ks = hs.one_list(V, Q[0], col, *qs[0], 1300, "cosine", (1.0, 1.0))
    assert rows[0] == planted and c[0] > c[1]
    dense, _ = fc.one_list(Q[0], V, 1300, "cosine")
    assert int(np.nonzero(dense == planted)[0][0]) >= 200
    sparse, _ = sp.one_list(col, *qs[0], 1300)
    assert int(np.nonzero(sparse == planted)[0][0]) >= 200
    # the 250 rows near the query share no term with it; the 250 with high sparse keys are nearly orthogonal
    kd_all, ks_all = hs.parts_of(V, Q[0], col, *qs[0], "cosine")
    assert (ks_all[dense[:250]] == 0).all() and (np.abs(kd_all[sparse[:250]]) < 0.1).all()
    # the RRF of two fetched lists of 200 cannot return it
    sc, idx, fu, hi = sp.expected_hybrid(V, Q, col, qs, 10, 200, "cosine")
    assert planted not in idx[0].tolist()
    assert hs.expected(V, Q, col, qs, 10, "cosine", (1.0, 1.0))[1][0, 0] == planted


def test_ties_are_ties_and_cross_the_cut():
    V, Q, col, qs = hs.tie_case()
    assert (V == V[0]).all()
    for b, (qt, qw) in enumerate(qs):
        rows, c, kd, ks = hs.one_list(V, Q[b], col, qt, qw, 100, "cosine", (1.0, 1.0))
        assert rows.size == 100 and np.unique(_bits(kd)).size == 1
        same = np.diff(c) == 0
        assert same.sum() >= 30, "few exact ties among the first 100"
        assert (np.diff(rows)[same] > 0).all()  # the row-id rule
        # ties in ks are ties in c, bit for bit
        assert ((np.diff(ks) == 0) == (_bits(c)[1:] == _bits(c)[:-1])).all()
    rows, c, kd, ks = hs.one_list(V, Q[0], col, *qs[0], 100, "cosine", (1.0, 1.0))
    assert c[9] == c[10], "no tie crosses the cut at k = 10"


def test_the_signed_case_ranks_a_positive_zero_and_values_below_zero():
    V, Q, col, qs, copy = hs.signed_case()
    assert (V[copy] == Q[0]).all()
    kd, ks = hs.parts_of(V, Q[0], col, *qs[0], "euclidean")
    assert kd[copy] == 0 and np.signbit(kd[copy]) and ks[copy] == 0 and not np.signbit(ks[copy])
    sc, idx, fu, de, spk = hs.expected(V, Q, col, qs, 1024, "euclidean", (1.0, 1.0))
    at = idx[0].tolist().index(copy)
    assert fu[0, at] == 0 and not np.signbit(fu[0, at]) and np.signbit(de[0, at])
    assert ((fu[0] < 0) & (idx[0] >= 0)).any() and (fu[0][idx[0] >= 0] > 0).any()
    assert (idx[0] >= 0).sum() == 513  # every row is a candidate, matched or not
    assert ((spk[0] < 0) & (idx[0] >= 0)).any()  # sparse keys of both signs
    # no value anywhere is -0.0
    for w in hs.WEIGHTS:
        f = hs.expected(V, Q, col, qs, 600, "euclidean", w)[2]
        assert not np.signbit(f[f == 0]).any(), w


def test_the_short_case_has_fewer_eligible_rows_than_k():
    V, Q, col, qs, mask, k = hs.short_case()
    assert 0 < mask.sum() < k
    sc, idx, fu, de, spk = hs.expected(V, Q, col, qs, k, "cosine", (1.0, 1.0), mask)
    assert ((idx >= 0).sum(axis=1) == mask.sum()).all()
    e = idx == -1
    assert (sc[e] == 0).all() and np.isneginf(fu[e]).all() and np.isneginf(de[e]).all() and np.isneginf(spk[e]).all()


def test_the_identities_of_the_contract_hold_in_the_oracle():
    n = 513
    col = sp.column(n, 30522)
    qs = sp.queries(30522)
    mask = np.random.default_rng(5).random(n) < 0.5
    for metric in hs.METRICS:
        V, Q = hs.dense_rows(n, sp.DIM)
        for m in (None, mask):
            for b, (qt, qw) in enumerate(qs):
                # (1, 0): the dense search's rows in its order, fused = its keys + 0.0
                rows, c, kd, ks = hs.one_list(V, Q[b], col, qt, qw, 50, metric, (1.0, 0.0), m)
                drows, dkeys = fc.one_list(Q[b], V, 50, metric, m)
                assert (rows == drows).all() and (_bits(c) == _bits(dkeys + 0.0)).all()
                assert (_bits(kd) == _bits(dkeys)).all()
                # (0, 1): the leading slots with ks > 0 are the sparse search's leading slots with keys > 0
                rows, c, kd, ks = hs.one_list(V, Q[b], col, qt, qw, 50, metric, (0.0, 1.0), m)
                srows, skeys = sp.one_list(col, qt, qw, 50, m)
                lead = int(np.argmin(ks > 0)) if not (ks > 0).all() else ks.size
                slead = int(np.argmin(skeys > 0)) if skeys.size and not (skeys > 0).all() else skeys.size
                assert lead == slead and (rows[:lead] == srows[:lead]).all()
                assert (_bits(c[:lead]) == _bits(skeys[:lead])).all()
                if qt.size == 8:
                    assert lead > 0
    # a euclidean copy of the query: key -0.0, fused +0.0
    V, Q, col2, qs2, copy = hs.signed_case()
    rows, c, kd, ks = hs.one_list(V, Q[0], col2, *qs2[0], 1, "euclidean", (1.0, 0.0))
    assert rows[0] == copy and np.signbit(kd[0]) and not np.signbit(c[0])


def test_combine_is_four_separate_operations():
    rng = np.random.default_rng(2)
    kd, ks = rng.standard_normal(1000), rng.standard_normal(1000) * 7
    for wd, ws in hs.WEIGHTS + ((0.1, 1e-3),):
        want = np.asarray([(np.float64(wd) * a + np.float64(ws) * b) + 0.0 for a, b in zip(kd, ks)])
        assert (_bits(hs.combine(wd, kd, ws, ks)) == _bits(want)).all()
    assert not np.signbit(hs.combine(1.0, -0.0, 1.0, 0.0)) and not np.signbit(hs.combine(0.0, 0.5, 0.0, 3.0))
    assert not np.signbit(hs.combine(0.0, -0.5, 0.0, 0.0))
    assert np.isfinite(hs.combine(hs.MAX_WEIGHT, -2.0 ** 279, hs.MAX_WEIGHT, 2.0 ** 279))

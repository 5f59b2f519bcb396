"""The cases of tests/_recommend_cases.py have the properties their names claim, checked on the CPU
with the reference arithmetic alone (no GPU): planted near-copies taken as positives bring the other
copies and would return themselves without the exclusion; negatives change the answer; the
sequential fp64 sum differs in bits from numpy's own mean; the k = 136 / 64-example case has most of
its examples inside the fetched 200; the overflow case's vector is non-finite."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _recommend_cases as rc  # noqa: E402
from oracle import ref_cpu  # noqa: E402


def _ranking(q, V, metric, xn):
    keys = ref_cpu.exact_keys(q, V, metric, xn if metric == "cosine" else None)
    rows = np.arange(V.shape[0])
    return rows[np.lexsort((rows, -keys))]


@pytest.mark.parametrize("metric", rc.METRICS)
@pytest.mark.parametrize("d", (33, 100, 260))
def test_planted_copies_as_positives_bring_the_other_copies(d, metric):
    V, _, rows = rc.planted_case(d)
    assert rows.size == 12
    pos = [int(r) for r in rows[[1, 5, 9]]]
    xn = rc.norms(V)
    q = rc.build_query(V, pos, [], metric, xn)
    top12 = _ranking(q, V, metric, xn)[:12]
    assert np.isin(pos, top12).all(), "without the exclusion the examples are not in the top 12"
    _, idx, _, _ = rc.expected(V, [pos], None, 9, metric)
    assert sorted(idx[0].tolist()) == sorted(set(rows.tolist()) - set(pos)), "the top 9 are not the other 9 copies"


@pytest.mark.parametrize("metric", rc.METRICS)
def test_negatives_change_the_result(metric):
    V, _ = rc.corpus(700, 100)
    pos, neg = rc.example_lists(700)
    changed = 0
    for p, g in zip(pos, neg):
        if not g:
            continue
        _, with_neg, _, _ = rc.expected(V, [p], [g], 10, metric)
        _, alone, _, _ = rc.expected(V, [p], None, 10, metric)
        changed += int((with_neg != alone).any())
    assert changed >= 1


@pytest.mark.parametrize("metric", rc.METRICS)
def test_the_sequential_sum_is_not_numpys_mean(metric):
    """An implementation that sums in another order (pairwise, as numpy's reduction does from 8
    addends on) fails the bit-for-bit comparison on this case."""
    V, pos, neg = rc.order_case()
    xn = rc.norms(V)
    differs = 0
    for p in pos + neg[2:]:
        p = list(p)
        seq = rc._mean(V, p, metric, xn)
        E = V[p].astype(np.float64)
        if metric == "cosine":
            E = E / np.maximum(xn[p], 1e-8)[:, None]
        other = np.mean(np.ascontiguousarray(E.T), axis=1, dtype=np.float64)  # pairwise along the examples
        differs += int((seq.view(np.uint64) != other.view(np.uint64)).any())
    assert differs >= 1


@pytest.mark.parametrize("metric", rc.METRICS)
def test_full_house_examples_crowd_the_fetched_list(metric):
    V, pos, neg = rc.full_house()
    assert len(pos) + len(neg) == rc.MAX_EXAMPLES
    xn = rc.norms(V)
    q = rc.build_query(V, pos, neg, metric, xn)
    top = _ranking(q, V, metric, xn)[:rc.MAX_K + rc.MAX_EXAMPLES]
    inside = np.isin(top, pos + neg)
    # (every kept entry of positions 64 .. 199 then lands at least 32 slots below its position: all
    # four lane positions of the select write through a non-zero prefix)
    assert inside.sum() >= 32
    _, idx, _, _ = rc.expected(V, [pos], [neg], rc.MAX_K, metric)
    assert (idx[0] >= 0).all() and not np.isin(idx[0], pos + neg).any()


def test_overflow_case_builds_a_non_finite_vector():
    V, pos, neg = rc.overflow_case()
    assert np.isfinite(V).all()
    xn = rc.norms(V)
    q0 = rc.build_query(V, pos[0], neg[0], "euclidean", xn)
    q1 = rc.build_query(V, pos[1], neg[1], "euclidean", xn)
    assert not np.isfinite(q0).all() and np.isfinite(q1).all()
    sc, idx, ks, qs = rc.expected(V, pos, neg, 3, "euclidean")
    assert (idx[0] == -1).all() and (qs[0] == 0).all() and (idx[1] >= 0).all()

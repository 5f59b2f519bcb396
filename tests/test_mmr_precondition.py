"""The cases of tests/_mmr_cases.py have the properties their names claim, checked on the CPU with
the reference arithmetic alone (no GPU): the planted near-copies fill plain top-10 and MMR keeps one
of them, the one-dim cosine case is full of tied values that the position rule decides, the
duplicate rows open a list with equal keys, the pair matrix is bitwise symmetric on every case, and
lambda = 1 is the plain exact search."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mmr_cases as mc  # noqa: E402
from oracle import ref_cpu  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("d", mc.PLANT_DIMS)
def test_planted_copies_fill_top_k_and_mmr_keeps_one(d):
    V, q, rows = mc.planted_case(d)
    assert rows.size == mc.PLANT_COPIES and V.shape == (mc.PLANT_N, d)
    for metric, lam in (("cosine", 0.5), ("euclidean", 0.0)):
        top = ref_cpu.exact_search(q[None], V, mc.PLANT_K, metric)[1][0]
        assert np.isin(top, rows).sum() == mc.PLANT_K, f"{metric}: plain top-{mc.PLANT_K} is not all copies"
        _, idx, _, _ = mc.expected(q[None], V, mc.PLANT_K, mc.PLANT_FETCH, lam, metric)
        assert (idx[0] >= 0).all() and np.unique(idx[0]).size == mc.PLANT_K
        assert np.isin(idx[0], rows).sum() == 1, f"{metric} lambda {lam}: MMR keeps {np.isin(idx[0], rows).sum()} copies"
        assert idx[0, 0] == top[0]  # slot 0 is the best row


def test_tie_case_values_tie_and_the_position_decides():
    V, Q = mc.tie_case()
    xn = ref_cpu.canonical_norm64(V)
    for q in Q:
        c, rel = mc.candidates(q, V, 64, "cosine", None, xn)
        S = mc.pair_matrix(V, c, "cosine", xn)
        assert set(np.unique(rel)) <= {-1.0, 1.0} and set(np.unique(S)) <= {-1.0, 1.0}
        assert (np.diff(c[rel == rel[0]]) > 0).all()  # equal keys: ascending rows
        # the second pick chooses between equal values: every unpicked position with pen = +1 ties
        lam = np.float64(0.5)
        v = lam * rel - (np.float64(1.0) - lam) * S[:, 0]
        assert np.sum(v[1:] == v[1:].max()) > 1
        pos, _ = mc.select(rel, S, 10, 0.5)
        assert pos[1] == 1 + int(np.argmax(v[1:]))  # the lowest position among them
    # both signs occur among the rows, so both key values occur in a long list
    c, rel = mc.candidates(Q[0], V, 700, "cosine", None, xn)
    assert {-1.0, 1.0} == set(np.unique(rel))


def test_duplicates_case_opens_with_equal_keys():
    V, Q, rows = mc.duplicates_case()
    for metric in mc.METRICS:
        xn = ref_cpu.canonical_norm64(V) if metric == "cosine" else None
        for j in range(3):
            c, rel = mc.candidates(Q[j], V, 64, metric, None, xn)
            n = rows.shape[1]
            np.testing.assert_array_equal(c[:n], rows[j])  # equal keys in row order
            assert np.unique(_bits(rel[:n])).size == 1 and rel[n] < rel[0]
            S = mc.pair_matrix(V, c, metric, xn)
            assert np.unique(_bits(S[:n, :n][~np.eye(n, dtype=bool)])).size == 1


def _cases():
    for d in (1, 33, 100, 260):
        V, Q = mc.corpus(700, d)
        yield f"corpus {d}", V, Q[0]
    for d in mc.PLANT_DIMS:
        V, q, _ = mc.planted_case(d)
        yield f"planted {d}", V, q
    V, Q = mc.tie_case()
    yield "tie", V, Q[0]
    V, Q, _ = mc.duplicates_case()
    yield "duplicates", V, Q[0]


@pytest.mark.parametrize("metric", mc.METRICS)
def test_pair_matrix_is_bitwise_symmetric(metric):
    for name, V, q in _cases():
        xn = ref_cpu.canonical_norm64(V) if metric == "cosine" else None
        c, _ = mc.candidates(q, V, 64, metric, None, xn)
        S = mc.pair_matrix(V, c, metric, xn)
        assert S.shape == (64, 64) and np.isfinite(S).all()
        np.testing.assert_array_equal(_bits(S), _bits(S.T), err_msg=f"{name} {metric}")


@pytest.mark.parametrize("metric", mc.METRICS)
def test_lambda_one_is_the_plain_search(metric):
    for name, V, q in _cases():
        for k, fetch in ((10, 64), (64, 64), (1, 200)):
            s, i, ks, mm = mc.expected(q[None], V, k, fetch, 1.0, metric)
            es, ei, ek = ref_cpu.exact_search(q[None], V, k, metric)
            np.testing.assert_array_equal(i, ei, err_msg=f"{name} {metric}")
            np.testing.assert_array_equal(_bits(ks), _bits(ek))
            np.testing.assert_array_equal(s.view(np.uint32), es.view(np.uint32))


def test_short_lists_masks_and_offsets_in_the_oracle():
    V, Q = mc.corpus(63, 100)
    mask = np.zeros(63, bool)
    mask[[3, 40]] = True
    s, i, ks, mm = mc.expected(Q[:2], V, 10, 64, 0.5, "cosine", mask, index_offset=2 ** 40)
    assert set(i[0, :2] - 2 ** 40) == {3, 40} and (i[:, 2:] == -1).all()
    assert (s[:, 2:] == 0).all() and np.isneginf(ks[:, 2:]).all() and np.isneginf(mm[:, 2:]).all()
    s, i, ks, mm = mc.expected(Q[:1], V, 5, 5, 0.5, "euclidean", np.zeros(63, bool))
    assert (i == -1).all() and np.isneginf(mm).all()
    assert mc.query_block(200) == 209 and mc.query_block(1) == 32768

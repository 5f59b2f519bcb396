"""CPU preconditions of tests/test_gpu_search_range.py (case builders: tests/_range_cases.py).

With the oracle alone: every case has the property its name claims -- the midpoint thresholds
pass exactly the intended number of rows, the equality rows sit exactly on kt, the planted squared
distances are exact integers, duplicates have equal keys, the density cases pass exactly their
rows -- so that a GPU failure is the kernel's and not the data's.  No GPU.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _range_cases as rc  # noqa: E402
from oracle import ref_cpu  # noqa: E402


def _count(keys_row, metric, t):
    return int(rc.expected(keys_row[None, :], rc.kt_of(metric, [t]), 0, metric)[0][0])


@pytest.mark.parametrize("metric", rc.METRICS)
@pytest.mark.parametrize("n,d,cap", [(1000, 100, 10), (33, 1, 5), (1537, 260, 64)])
def test_midpoint_thresholds_pass_exactly_m_rows(n, d, cap, metric):
    V, Q = rc.corpus(n, d)
    keys = rc.oracle_keys(Q[:2], V, metric)
    for b in range(2):
        assert np.unique(keys[b]).size == n or d == 1  # distinct keys: a midpoint separates them
        for m in rc.midpoint_ms(n, cap):
            t = rc.midpoint_threshold(keys[b], m, metric)
            s = np.sort(keys[b])[::-1]
            if d == 1 and 0 < m < n and s[m - 1] == s[m]:
                continue  # (one-dim cosine keys are +-1: no midpoint between equal keys)
            assert _count(keys[b], metric, t) == m, (n, d, m, metric)


def test_query_block_sizes_differ_between_the_batch_test_dims():
    assert rc.query_block(100) == 64 and rc.query_block(1536) == 21
    assert rc.query_block(1) == 64 and rc.query_block(2100) == 15


def test_kt_formula():
    np.testing.assert_array_equal(rc.kt_of("cosine", [0.25, -np.inf]), [0.25, -np.inf])
    np.testing.assert_array_equal(rc.kt_of("euclidean", [5.0, np.inf, 0.0]), [-25.0, -np.inf, -0.0])


@pytest.mark.parametrize("d", [1, 33, 100, 768])
def test_cosine_equality_row_sits_on_kt(d):
    V, Q = rc.corpus(700, d)
    keys = rc.oracle_keys(Q[:1], V, "cosine")[0]
    row = 123
    t_in, t_out = rc.cosine_equality(keys, row)
    assert rc.kt_of("cosine", t_in) == keys[row] and t_out > t_in
    inc = rc.expected(keys[None], [t_in], 700, "cosine")
    exc = rc.expected(keys[None], [t_out], 700, "cosine")
    assert row in inc[1][0] and row not in exc[1][0]
    assert inc[0][0] - exc[0][0] == np.count_nonzero(keys == keys[row])


@pytest.mark.parametrize("d", [1, 2, 33, 100, 260, 1536])
def test_euclid_equality_distances_are_exact(d):
    V, q, planted = rc.euclid_equality_case(600, d)
    keys = ref_cpu.exact_keys(q, V, "euclidean")
    np.testing.assert_array_equal(keys[planted], -rc.EUCLID_SQ)  # exactly -25: integer arithmetic
    assert rc.kt_of("euclidean", rc.EUCLID_RADIUS) == -rc.EUCLID_SQ
    t_out = np.nextafter(rc.EUCLID_RADIUS, 0.0)
    assert rc.kt_of("euclidean", t_out) > -rc.EUCLID_SQ
    inc = rc.expected(keys[None], rc.kt_of("euclidean", [rc.EUCLID_RADIUS]), 600, "euclidean")
    exc = rc.expected(keys[None], rc.kt_of("euclidean", [t_out]), 600, "euclidean")
    assert set(planted) <= set(inc[1][0]) and not (set(planted) & set(exc[1][0]))
    assert inc[0][0] - exc[0][0] == planted.size  # no other row lies on the radius


@pytest.mark.parametrize("metric", rc.METRICS)
def test_duplicates_have_equal_keys(metric):
    V, Q, groups = rc.duplicates_case(900, 100)
    keys = rc.oracle_keys(Q[:2], V, metric)
    for g in groups:
        assert np.unique(V[g], axis=0).shape[0] == 1
        for b in range(2):
            assert np.unique(keys[b, g]).size == 1
            t = float(keys[b, g[0]]) if metric == "cosine" else None
            if t is not None:
                assert set(g) <= set(rc.expected(keys[b][None], [t], 900, metric)[1][0])


@pytest.mark.parametrize("metric", rc.METRICS)
@pytest.mark.parametrize("name", rc.DENSITIES)
@pytest.mark.parametrize("n", [rc.WG_ROWS + 1, 1000])
def test_density_cases_pass_exactly_their_rows(name, n, metric):
    V, q, rows, t = rc.density_case(name, n, metric)
    keys = ref_cpu.exact_keys(q, V, metric)
    c, i, _, _ = rc.expected(keys[None], rc.kt_of(metric, [t]), n, metric)
    assert c[0] == rows.size
    np.testing.assert_array_equal(i[0, :c[0]], np.sort(rows))
    n_words = (n + 31) // 32
    if name == "first_word":
        assert (rows < 32).all() and rows.size == 32
    if name == "last_word":
        assert (rows >= (n_words - 1) * 32).all() and rows.size == n - (n_words - 1) * 32
    if name == "one_per_word":
        assert np.unique(rows // 32).size == n_words == rows.size


def test_words_layout_matches_row_mask():
    m = np.zeros(70, bool)
    m[[0, 31, 32, 69]] = True
    w = rc.words(m)
    assert w.dtype == np.uint32 and w.tolist() == [0x80000001, 1, 1 << 5]

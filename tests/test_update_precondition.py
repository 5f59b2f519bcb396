"""CPU preconditions of tests/test_gpu_update.py (case tables: tests/_update_cases.py).

* Each pattern updates what its name says, with pairwise distinct ids, and carries its plants.
* Under every pattern and both metrics the oracle's answer over the updated corpus V2 differs from
  its answer over V for at least one query: an update that wrote nothing would fail the GPU test.
* The two planted effects hold: wherever row 0 is updated it becomes Q[2]'s top 1, and wherever
  row N - 1 (Q[1]'s self-match) is updated Q[1] no longer finds it.
* The chunked cases have several chunks with a partial last one; the large case is past the phase
  in which an add re-derives the centring row, the step and the direction.
* The certification case permutes rows among themselves: the multiset of rows is unchanged.
Measured with the reference arithmetic alone, never with the library.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _planted as pl  # noqa: E402
import _remove_cases as rc  # noqa: E402
import _update_cases as uc  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_patterns_update_what_their_names_say():
    for name in uc.PATTERNS:
        rows = uc.pattern_rows(name)
        assert rows.size == np.unique(rows).size and rows.min() >= 0 and rows.max() < uc.N
    assert uc.pattern_rows("first").tolist() == [0] and uc.pattern_rows("last").tolist() == [uc.N - 1]
    assert uc.pattern_rows("word").tolist() == list(range(544, 576))
    assert uc.pattern_rows("block").tolist() == list(range(1000, 1500))
    assert uc.pattern_rows("every_other").size == (uc.N + 1) // 2
    assert uc.pattern_rows("rand1").size == uc.N // 100 and uc.pattern_rows("rand50").size == uc.N // 2
    assert uc.pattern_rows("all").size == uc.N
    rev = uc.pattern_rows("reversed_ids")
    assert (np.diff(rev) < 0).all() and np.array_equal(rev[::-1], uc.pattern_rows("rand50"))
    assert set(uc.REDUCED) <= set(uc.PATTERNS)


@pytest.mark.parametrize("D", uc.DIMS)
def test_plants_are_in_the_new_rows(D):
    V, Q = rc.rows_data(uc.N, D, 100 + D)
    scale = float(np.linalg.norm(V, axis=1).mean())
    for name in uc.PATTERNS:
        rows, new = uc.pattern_rows(name), uc.new_rows(name, D)
        assert new.shape == (rows.size, D) and np.isfinite(new).all()
        z, loud = uc.zero_and_loud(name)
        if rows.size >= 32:
            assert z is not None
        if z is not None:
            assert not new[z].any()
            assert np.linalg.norm(new[loud]) > 30 * scale  # far past the int8 copy's range: it clips
        if 0 in rows:
            np.testing.assert_array_equal(new[np.nonzero(rows == 0)[0][0]], Q[2])


@pytest.mark.parametrize("metric", pl.BOTH)
@pytest.mark.parametrize("D", uc.DIMS)
def test_every_pattern_changes_an_answer_and_the_plants_take_effect(D, metric):
    V, Q = rc.rows_data(uc.N, D, 100 + D)
    (_, i0, k0), _ = uc.base_oracle(D, metric)
    assert i0[1, 0] == uc.N - 1  # Q[1]'s self-match before any update
    for name in uc.PATTERNS:
        rows = uc.pattern_rows(name)
        V2, (_, i2, k2), (_, im, _) = uc.pattern_oracle(name, D, metric)
        changed = np.setdiff1d(np.nonzero((V2 != V).any(axis=1))[0], rows)
        assert changed.size == 0  # only the pattern's rows differ
        assert (i2 != i0).any() or (k2 != k0).any(), name
        if 0 in rows:
            assert i2[2, 0] == 0, name
        if uc.N - 1 in rows:
            assert uc.N - 1 not in i2[1], name


def test_chunked_cases_have_a_partial_last_chunk():
    n = uc.pattern_rows("rand50").size
    assert n == 2501 and -(-n // uc.CHUNK) == 3 and n % uc.CHUNK not in (0,)
    big = uc.big_rows()
    assert big.size == np.unique(big).size == uc.BIG_N * 3 // 10 and big.size % uc.CHUNK != 0
    assert (np.diff(big) < 0).any()  # not sorted: any order


def test_large_case_is_past_the_rederivation_phase():
    src = open(os.path.join(ROOT, "mlx-vector-db_amd", "csrc", "vdb_api.cpp")).read()
    m = re.search(r"kDirRows\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == uc.DIR_ROWS
    assert uc.BIG_N > uc.DIR_ROWS  # one add: derived from DIR_ROWS rows, final
    # the small case: derived from its N rows; the add of N more doubles the index inside the phase
    dir_rows = min(uc.N, uc.DIR_ROWS)
    assert dir_rows == uc.N < uc.DIR_ROWS and uc.N + uc.N >= 2 * dir_rows


def test_long_list_case_takes_the_long_column_sum_form():
    src = open(os.path.join(ROOT, "mlx-vector-db_amd", "csrc", "vdb_update.hip")).read()
    m = re.search(r"kUpdColsumLongFrom\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == uc.COLSUM_LONG_FROM
    m = re.search(r"kUpdColsumRowsLong\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == uc.COLSUM_ROWS_LONG
    rows = uc.long_rows()
    assert rows.size == np.unique(rows).size >= uc.COLSUM_LONG_FROM and rows.size % uc.COLSUM_ROWS_LONG != 0
    assert uc.big_rows().size < uc.COLSUM_LONG_FROM  # (the chunked large case stays on the short form)
    V, Q = rc.rows_data(uc.BIG_N, uc.BIG_D, 7)
    V2, (_, i2, _) = uc.long_oracle()
    assert i2[2, 0] == rows[-1] and (V2 != V).any(axis=1).sum() == rows.size


DATASETS = sorted({c[:5] for c in rc.cert_cases()})


@pytest.mark.parametrize("key", DATASETS, ids=[k[0] for k in DATASETS])
def test_certification_case_keeps_the_multiset_of_rows(key):
    name, n, d, b, k = key
    V, _, _ = pl.data(n, d, b, k, rc.cert_seed(n, d, b, k))
    rows, V2 = uc.cert_updated(n, d, b, k)
    assert rows.size == n // 2 == np.unique(rows).size
    assert (V2 != V).any()
    order = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
    np.testing.assert_array_equal(order(V2), order(V))
    untouched = np.setdiff1d(np.arange(n), rows)
    np.testing.assert_array_equal(V2[untouched], V[untouched])

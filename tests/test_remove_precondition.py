"""CPU preconditions of tests/test_gpu_remove.py (case tables: tests/_remove_cases.py).

* Each removal pattern removes what its name says (partial last word, a whole word, a whole
  1024-row granule, a block that starts and ends inside a word, ...).
* The chunked case has more bitmap words than one workgroup of the keep-count scan handles,
  chunks with no surviving row and chunks with no removed row.
* Certification survives a remove: on every planted-gap case the removed rows are in no query's
  planted top k, and each query's gap s_k - s_{k+1} over the SURVIVING rows is at least
  6 eps_upper of the ORIGINAL corpus -- the factor of tests/test_planted_precondition.py.  The
  centring row, the quantisation step, the direction and the running statistics stay those of the
  original one-add corpus (or lower), so eps_upper(V_original) still bounds the finish's eps, and
  deleting rows outside the top k can only widen the gap.  Measured with the reference arithmetic
  alone (the oracle's exact keys, numpy models of the bounds), never with the library.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _planted as pl  # noqa: E402
import _remove_cases as rc  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_patterns_remove_what_their_names_say():
    assert rc.N % 32 != 0 and rc.N % 1024 != 0
    for name in rc.PATTERNS:
        rows = rc.pattern_rows(name)
        words = rc.pattern_words(name)
        assert words.dtype == np.uint32 and words.size == rc.n_words(rc.N)
        assert np.array_equal(rows, np.unique(rows)) and (rows.size == 0 or (rows[0] >= 0 and rows[-1] < rc.N))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        np.testing.assert_array_equal(np.nonzero(bits[: rc.N])[0], rows)
        if name == "past_count":
            assert bits[rc.N:].all() and bits[rc.N:].size == 32 - rc.N % 32 and not bits[: rc.N].any()
        else:
            assert not bits[rc.N:].any()
    assert rc.pattern_rows("first").tolist() == [0] and rc.pattern_rows("last").tolist() == [rc.N - 1]
    w = rc.pattern_rows("word")
    assert w.size == 32 and w[0] % 32 == 0
    g = rc.pattern_rows("granule")
    assert g.size == 1024 and g[0] % 1024 == 0
    blk = rc.pattern_rows("block")
    assert blk[0] % 32 not in (0, 31) and (blk[-1] + 1) % 32 not in (0, 1) and np.array_equal(blk, np.arange(blk[0], blk[-1] + 1))
    assert rc.pattern_rows("every_other").size == (rc.N + 1) // 2
    assert rc.pattern_rows("rand1").size == rc.N // 100 and rc.pattern_rows("rand50").size == rc.N // 2
    assert rc.pattern_rows("all_but_one").size == rc.N - 1
    assert rc.pattern_rows("none").size == 0
    assert set(rc.REDUCED) <= set(rc.PATTERNS)


def test_scan_workgroup_size_matches_the_library():
    src = open(os.path.join(ROOT, "mlx-vector-db_amd", "csrc", "vdb_compact_plan.h")).read()
    m = re.search(r"kScanWgWords\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == rc.SCAN_WG_WORDS


def test_chunked_case_crosses_scan_blocks_and_has_empty_and_full_chunks():
    words = rc.n_words(rc.BIG_N)
    assert words == 2189 and words > rc.SCAN_WG_WORDS  # more than one workgroup of the scan
    assert rc.BIG_N % 32 != 0
    gone = np.zeros(rc.BIG_N, bool)
    gone[rc.big_rows()] = True
    assert gone[0]  # chunks start at word 0
    cr = rc.BIG_CHUNK_ROWS
    assert cr == 992
    per_chunk = [gone[c * cr:(c + 1) * cr] for c in range((rc.BIG_N + cr - 1) // cr)]
    assert len(per_chunk) > 60
    assert per_chunk[rc.BIG_ALL_REMOVED].all() and not per_chunk[rc.BIG_ALL_KEPT].any()
    frac = gone.mean()
    assert 0.28 < frac < 0.33
    # the small chunked case: every other row at 32 rows per chunk
    assert rc.n_words(rc.N) > 100


CERT_DATASETS = sorted({c[:6] for c in rc.cert_cases()})


@pytest.mark.parametrize("key", CERT_DATASETS, ids=[f"{k[0]}-{k[5]}" for k in CERT_DATASETS])
def test_gap_over_the_survivors_is_six_eps_of_the_original(key):
    name, n, d, b, k, metric = key
    V, Q, pos = pl.data(n, d, b, k, rc.cert_seed(n, d, b, k))
    removed = rc.cert_removed(n, d, b, k)
    assert removed.size == (n - b * k) // 4
    assert np.intersect1d(removed, pos.ravel()).size == 0  # disjoint from every pos[b]
    es, ei, ek, gap = rc.cert_oracle(n, d, b, k, metric)
    # the planted rows, renumbered, are still each query's k nearest
    new_id = np.cumsum(~np.isin(np.arange(n), removed)) - 1
    np.testing.assert_array_equal(np.sort(ei, axis=1), np.sort(new_id[pos], axis=1))
    # ... and the gap can only have widened
    _, _, _, gap0 = pl.oracle(n, d, b, k, rc.cert_seed(n, d, b, k), metric)
    assert (gap >= gap0).all()
    for prec in sorted({pl.resolved(p, metric, k) for p in rc.CERT_PRECISIONS}):
        eps = pl.eps_upper(V, Q, metric, prec)  # of the ORIGINAL corpus
        ratio = float((gap / eps).min())
        print(f"{name} {metric} {prec}: min gap over survivors / eps_upper(original) = {ratio:.1f}")
        assert ratio >= 6.0, (prec, ratio)

"""Certificate soundness on the device: rows whose candidate-pass error reaches the bound, where
the row that sets the running maximum arrives by each ingest route in turn (tests/_tight_cases.py,
DESIGN.md §5.4).

On this data a maximum that misses the planted rows -- not raised by the route's kernel, lost in a
rollback, a re-derivation or a late copy build, left behind by a clear -- either drops the true
top-1 from the rerank set of a query that still certifies (a wrong answer) or trips the
consistency guard (tests/test_tight_precondition.py (c), on the CPU, from the models alone); a
sound bound does neither ((a), (b) there).  So for every route, precision and metric: one
host-memory search into poisoned buffers must return the oracle's indices, fp64 keys and scores
bit for bit, with no query fallen back, overflowed, flagged inconsistent or re-passed, by the
intended pass.  No knob corrupts the maxima on the device: the teeth rest on (c).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # tests/_planted.py, under any pytest import mode
import _tight_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

POISON_IDX = -7
NETS = ("fallback_queries", "overflow_queries", "inconsistent_queries", "repass_queries")
PASSES = ("fp32", "bf16x3", "bf16", "i8", "i8x3", "i8q")
# data set by data set, so that each is built once
CASES = sorted(tc.cases(), key=lambda c: (tc.DATASET[c[0]], c[1], c[2], tc.ROUTES.index(c[0])))


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def _search(vdb, ix, Q, k):
    """A host-memory search into poisoned buffers."""
    q = np.ascontiguousarray(Q, dtype=np.float32)
    nq = q.shape[0]
    s = np.full((nq, k), np.nan, np.float32)
    i = np.full((nq, k), POISON_IDX, np.int64)
    kk = np.full((nq, k), np.nan, np.float64)
    vdb._check(ix._lib.vdb_index_search(ix._h, q.ctypes.data, nq, int(k), None, vdb.MEM_HOST, s.ctypes.data,
                                        i.ctypes.data, kk.ctypes.data, 0, None))
    return s, i, kk


def _run(vdb, route, precision, metric, ran):
    d = tc.dataset(tc.DATASET[route], ran, metric)
    ix = vdb.NativeIndex(tc.D, metric, precision="fp32" if route == "R9" else precision)
    ix.set_param("i8_refine", 0)  # the models do not cover the finish's I8 refinement
    tc.ingest(ix, route, d, precision)
    before = {n: ix.stat(n) for n in NETS}
    count = {p: ix.stat(f"searches_{p}") for p in PASSES}
    s, i, kk = _search(vdb, ix, d["Q"], tc.K)
    es, ei, ek = tc.oracle(tc.DATASET[route], ran, metric)
    np.testing.assert_array_equal(i, ei)
    np.testing.assert_array_equal(kk, ek)
    np.testing.assert_array_equal(s, es)
    assert {n: ix.stat(n) for n in NETS} == before
    assert {p: ix.stat(f"searches_{p}") - count[p] for p in PASSES} == {p: int(p == ran) for p in PASSES}
    ix.close()


@pytest.mark.parametrize("c", CASES, ids=[tc.case_id(c) for c in CASES])
def test_the_bound_covers_rows_at_the_bound(vdb, c):
    route, precision, metric = c
    _run(vdb, route, precision, metric, precision)


@pytest.mark.parametrize("metric", tc.BOTH)
def test_auto_takes_the_i8_pass_on_the_same_rows(vdb, metric):
    _run(vdb, "R1", "auto", metric, "i8")  # k = 10 <= 16: I8

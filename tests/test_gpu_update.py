"""In-place row update on the device (include/vdb.h vdb_index_update; csrc/vdb_update.hip).

After every update the index must be what an index holding ``V2 = V.copy(); V2[rows] = new`` is:
the rows bit for bit (``get_vectors``), every search bit for bit -- indices, fp64 keys and fp32
scores -- equal to ``oracle.ref_cpu.exact_search`` over V2, under the index's candidate pass and
with force_exact, unmasked and with a row_mask, and no query flagged by the int8 pass's checksum
(``inconsistent_queries``: the column sums are exact integers, so sums that are stale, subtracted
twice or never subtracted show there and nowhere else).  count and capacity stay.

Case tables and their CPU preconditions: tests/_update_cases.py, tests/test_update_precondition.py.
Output buffers hold a poison value before each call (index -7, key and score NaN).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _planted as pl  # noqa: E402
import _remove_cases as rc  # noqa: E402
import _update_cases as uc  # noqa: E402
from oracle import ref_cpu  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def _search(vdb, ix, Q, k, words=None):
    """A host-memory search into poisoned buffers."""
    q = np.ascontiguousarray(Q, dtype=np.float32)
    nq = q.shape[0]
    s = np.full((nq, k), np.nan, np.float32)
    i = np.full((nq, k), uc.POISON_IDX, np.int64)
    kk = np.full((nq, k), np.nan, np.float64)
    if words is not None:
        words = np.ascontiguousarray(words, dtype=np.uint32)
    vdb._check(ix._lib.vdb_index_search(ix._h, q.ctypes.data, nq, int(k), words.ctypes.data if words is not None else None,
                                        vdb.MEM_HOST, s.ctypes.data, i.ctypes.data, kk.ctypes.data, 0, None))
    return s, i, kk


def _assert_same(got, want, what=""):
    (s, i, k), (es, ei, ek) = got, want[:3]
    np.testing.assert_array_equal(i, ei, err_msg=f"indices {what}")
    np.testing.assert_array_equal(k, ek, err_msg=f"keys {what}")
    np.testing.assert_array_equal(s, es, err_msg=f"scores {what}")


def _index(vdb, V, metric, precision):
    ix = vdb.NativeIndex(V.shape[1], metric, precision=precision)  # the precision before the add:
    ix.add(V)                                                     # its eager copy is the one updated
    assert ix.count() == V.shape[0]
    return ix


def _check_searches(vdb, ix, S, Q, k, metric, want=None, want_masked=None, what=""):
    """Unmasked and masked searches, under the index's pass and with force_exact, against the
    oracle over the rows S; no query flagged as inconsistent."""
    mask = rc.filter_mask(S.shape[0])
    if want is None:
        want = ref_cpu.exact_search(Q, S, k, metric)
    if want_masked is None:
        want_masked = ref_cpu.exact_search(Q, S, k, metric, row_mask=mask)
    words = rc.mask_words(mask)
    incons = ix.stat("inconsistent_queries")
    for force in (0, 1):
        ix.set_param("force_exact", force)
        _assert_same(_search(vdb, ix, Q, k), want, f"{what} force_exact={force}")
        _assert_same(_search(vdb, ix, Q, k, words), want_masked, f"{what} masked force_exact={force}")
    ix.set_param("force_exact", 0)
    assert ix.stat("inconsistent_queries") - incons == 0, what


def _update(ix, rows, new):
    """ix.update with the bookkeeping every case asserts: count and capacity stay, rows_updated
    rises by the rows given."""
    before = (ix.count(), ix.stat("capacity"), ix.stat("rows_updated"))
    assert ix.update(rows, new) == len(rows)
    assert (ix.count(), ix.stat("capacity"), ix.stat("rows_updated")) == (before[0], before[1], before[2] + len(rows))


# =============================================================================
# patterns
# =============================================================================
@pytest.mark.parametrize("c", uc.pattern_cases(), ids=[uc.pattern_id(c) for c in uc.pattern_cases()])
def test_update_patterns(vdb, c):
    D, metric, precision, name = c
    V, Q = rc.rows_data(uc.N, D, 100 + D)
    ix = _index(vdb, V, metric, precision)
    _update(ix, uc.pattern_rows(name), uc.new_rows(name, D))
    V2, want, want_masked = uc.pattern_oracle(name, D, metric)
    np.testing.assert_array_equal(ix.get_vectors(), V2)
    _check_searches(vdb, ix, V2, Q, uc.K, metric, want, want_masked, name)
    ix.close()


def test_any_integer_dtype(vdb):
    V, Q = rc.rows_data(uc.N, 96, 196)
    rows, new = uc.pattern_rows("rand1"), uc.new_rows("rand1", 96)
    ix = _index(vdb, V, "cosine", "auto")
    _update(ix, rows.astype(np.int32), new)
    _update(ix, rows.astype(np.uint16).tolist(), np.array(new))  # the same rows again: the same V2
    np.testing.assert_array_equal(ix.get_vectors(), uc.updated("rand1", 96))
    assert ix.update(np.zeros(0, np.int64), np.zeros((0, 96), np.float32)) == 0
    ix.close()


# =============================================================================
# chunks
# =============================================================================
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("D", uc.DIMS)
def test_several_chunks(vdb, D, mem):
    """update_chunk = 1000 with rand50's 2 501 rows: three chunks, the last partial; host-memory
    arguments (staged, sent twice) and device-memory ones (ids and rows written on a side stream
    just before the call)."""
    V, Q = rc.rows_data(uc.N, D, 100 + D)
    rows, new = uc.pattern_rows("reversed_ids"), uc.new_rows("reversed_ids", D)
    ix = _index(vdb, V, "cosine", "auto")
    ix.set_param("update_chunk", uc.CHUNK)
    if mem == "host":
        _update(ix, rows, new)
    else:
        import torch
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            rd = torch.from_numpy(rows.astype(np.int64)).cuda(non_blocking=True)
            vd = torch.from_numpy(np.array(new)).cuda(non_blocking=True)
        n0 = ix.stat("rows_updated")
        assert ix.update_device(rd.data_ptr(), vd.data_ptr(), rows.size, stream=st.cuda_stream) == rows.size
        assert ix.stat("rows_updated") - n0 == rows.size and ix.count() == uc.N
    V2, want, want_masked = uc.pattern_oracle("reversed_ids", D, "cosine")
    np.testing.assert_array_equal(ix.get_vectors(), V2)
    _check_searches(vdb, ix, V2, Q, uc.K, "cosine", want, want_masked, f"chunks {mem}")
    ix.close()


# =============================================================================
# the frozen centring row, step and direction
# =============================================================================
def test_past_the_rederivation_phase(vdb):
    """70 017 rows in one add: mu / sx / dir are final (dir_rows = 65 536).  A random 30 % updated
    in 1000-row chunks."""
    V, Q = rc.rows_data(uc.BIG_N, uc.BIG_D, 7)
    V2, want = uc.big_oracle()
    rows = uc.big_rows()
    ix = _index(vdb, V, "cosine", "auto")
    ix.set_param("update_chunk", uc.CHUNK)
    _update(ix, rows, V2[rows])
    np.testing.assert_array_equal(ix.get_vectors(), V2)
    _check_searches(vdb, ix, V2, Q, uc.K, "cosine", want, None, "past the phase")
    ix.close()


def test_long_list_in_one_chunk(vdb):
    """35 008 rows in one chunk: the list column sums run their long form (512 entries per
    workgroup from 32 768 entries, the last workgroup partial)."""
    V, Q = rc.rows_data(uc.BIG_N, uc.BIG_D, 7)
    V2, want = uc.long_oracle()
    rows = uc.long_rows()
    ix = _index(vdb, V, "cosine", "auto")
    _update(ix, rows, V2[rows])
    np.testing.assert_array_equal(ix.get_vectors(), V2)
    _check_searches(vdb, ix, V2, Q, uc.K, "cosine", want, None, "long list")
    ix.close()


@pytest.mark.parametrize("metric", pl.BOTH)
def test_inside_the_rederivation_phase(vdb, metric):
    """5 003 rows, half of them updated, then 5 003 more added: the add doubles the index inside
    the phase and re-derives mu / sx / dir over all rows, the updated ones as they now are."""
    V, Q = rc.rows_data(uc.N, 96, 196)
    ix = _index(vdb, V, metric, "auto")
    _update(ix, uc.pattern_rows("rand50"), uc.new_rows("rand50", 96))
    more = np.random.default_rng(77).standard_normal((uc.N, 96)).astype(np.float32)
    ix.add(more)
    S = np.concatenate([uc.updated("rand50", 96), more])
    assert ix.count() == 2 * uc.N
    np.testing.assert_array_equal(ix.get_vectors(), S)
    _check_searches(vdb, ix, S, Q, uc.K, metric, what="update then add")
    ix.close()


# =============================================================================
# rejected calls leave no trace
# =============================================================================
@pytest.mark.parametrize("precision", ["auto", "bf16x3"])
@pytest.mark.parametrize("chunk", [0, uc.CHUNK])
def test_rejected_calls_leave_no_trace(vdb, precision, chunk):
    V, Q = rc.rows_data(uc.N, 96, 196)
    rows, new = uc.pattern_rows("rand50"), np.array(uc.new_rows("rand50", 96))
    ix = _index(vdb, V, "cosine", precision)
    ix.set_param("update_chunk", chunk)
    want = ref_cpu.exact_search(Q, V, uc.K, "cosine")
    want_masked = ref_cpu.exact_search(Q, V, uc.K, "cosine", row_mask=rc.filter_mask(uc.N))

    def call(r, v):
        r = np.ascontiguousarray(r, np.int64)
        v = np.ascontiguousarray(v, np.float32)
        return ix._lib.vdb_index_update(ix._h, r.ctypes.data, v.ctypes.data, r.size, vdb.MEM_HOST, None)

    past = rows.copy()
    past[-1] = uc.N  # an id equal to count, after 2 500 good ones
    twice = rows.copy()
    twice[-1] = twice[3]  # a repeat, the two in different chunks when there are chunks
    nan = new.copy()
    nan[-1, 95] = np.nan  # in the last updated row
    for r, v, code in ((past, new, vdb.VDB_ERR_INVALID), (twice, new, vdb.VDB_ERR_INVALID),
                       (rows, nan, vdb.VDB_ERR_NONFINITE), (np.array([-1]), new[:1], vdb.VDB_ERR_INVALID)):
        assert call(r, v) == code
        assert ix.stat("rows_updated") == 0 and ix.count() == uc.N
        np.testing.assert_array_equal(ix.get_vectors(), V)
        _check_searches(vdb, ix, V, Q, uc.K, "cosine", want, want_masked, f"after error {code}")
    with pytest.raises(ValueError):
        ix.update(rows, new[:-1])  # shape
    with pytest.raises(ValueError):
        ix.update(rows.astype(np.float64), new)
    with pytest.raises(ValueError):
        ix.set_param("update_chunk", -1)
    assert ix._lib.vdb_index_update(ix._h, None, None, 0, vdb.MEM_HOST, None) == vdb.VDB_OK  # n == 0
    assert ix._lib.vdb_index_update(ix._h, None, None, 1, vdb.MEM_HOST, None) == vdb.VDB_ERR_INVALID
    _update(ix, rows, new)  # and the same call, valid, goes through
    np.testing.assert_array_equal(ix.get_vectors(), uc.updated("rand50", 96))
    ix.close()


# =============================================================================
# composes with the other mutations
# =============================================================================
@pytest.mark.parametrize("metric,precision", [("cosine", "auto"), ("euclidean", "auto"), ("cosine", "bf16x3")])
def test_update_remove_update_add(vdb, metric, precision):
    V, Q = rc.rows_data(uc.N, 96, 196)
    rng = np.random.default_rng(91)
    ix = _index(vdb, V, metric, precision)
    _update(ix, uc.pattern_rows("rand50"), uc.new_rows("rand50", 96))
    S = np.array(uc.updated("rand50", 96))
    _check_searches(vdb, ix, S, Q, uc.K, metric, what="update")
    gone = rc.pattern_rows("block")
    assert ix.remove(gone) == gone.size
    S = np.delete(S, gone, axis=0)
    _check_searches(vdb, ix, S, Q, uc.K, metric, what="remove")
    rows2 = rng.permutation(S.shape[0])[:700]
    new2 = rng.standard_normal((700, 96)).astype(np.float32)
    _update(ix, rows2, new2)
    S[rows2] = new2
    np.testing.assert_array_equal(ix.get_vectors(), S)
    _check_searches(vdb, ix, S, Q, uc.K, metric, what="second update")
    fresh = rng.standard_normal((300, 96)).astype(np.float32)
    ix.add(fresh)
    S = np.concatenate([S, fresh])
    np.testing.assert_array_equal(ix.get_vectors(), S)
    _check_searches(vdb, ix, S, Q, uc.K, metric, what="add")
    assert ix.stat("rows_updated") == uc.N // 2 + 700
    ix.close()


# =============================================================================
# a copy the precision does not read is rebuilt when a setting starts to
# =============================================================================
@pytest.mark.parametrize("metric", pl.BOTH)
def test_precision_switch_after_an_update(vdb, metric):
    V, Q = rc.rows_data(uc.N, 200, 300)
    ix = _index(vdb, V, metric, "bf16x3")
    _update(ix, uc.pattern_rows("rand50"), uc.new_rows("rand50", 200))
    V2 = uc.updated("rand50", 200)
    want = ref_cpu.exact_search(Q, V2, uc.K, metric)
    want_masked = ref_cpu.exact_search(Q, V2, uc.K, metric, row_mask=rc.filter_mask(uc.N))
    _check_searches(vdb, ix, V2, Q, uc.K, metric, want, want_masked, "bf16x3")
    for precision in ("auto", "i8x3"):
        ix.set_precision(precision)  # the int8 copy is built now, from the updated rows
        _check_searches(vdb, ix, V2, Q, uc.K, metric, want, want_masked, precision)
    ix.close()


@pytest.mark.parametrize("metric", pl.BOTH)
def test_lazy_split_copy_is_updated(vdb, metric):
    """Under auto the split copy exists only once a search needed one; an update keeps it up to
    date, so a bf16x3 search afterwards reads it without a rebuild."""
    V, Q = rc.rows_data(uc.N, 200, 300)
    ix = _index(vdb, V, metric, "auto")
    ix.set_precision("bf16x3")
    _search(vdb, ix, Q, uc.K)
    ix.set_precision("auto")
    assert ix.stat("split_copy") == 1
    _update(ix, uc.pattern_rows("rand50"), uc.new_rows("rand50", 200))
    ix.set_precision("bf16x3")
    builds = ix.stat("split_copy_builds")
    _check_searches(vdb, ix, uc.updated("rand50", 200), Q, uc.K, metric, what="bf16x3 after update")
    assert ix.stat("split_copy_builds") == builds
    ix.close()


# =============================================================================
# a graph built before an update is stale
# =============================================================================
def test_graph_is_stale_after_an_update(vdb):
    V, Q = rc.rows_data(uc.N, 96, 196)
    ix = _index(vdb, V[:2000], "cosine", "auto")
    g = vdb.NativeGraph.build(ix, degree=16, knn=16, n_entries=64)
    labels, _ = g.search(Q, 5, ef=32)
    assert (labels >= 0).all()
    _update(ix, np.arange(100, 110), V[3000:3010])
    assert ix.count() == g.info()[0] == 2000
    with pytest.raises(ValueError, match="stale"):
        g.search(Q, 5, ef=32)
    with pytest.raises(ValueError, match="stale"):
        g.add()
    g2 = vdb.NativeGraph.build(ix, degree=16, knn=16, n_entries=64)  # a rebuild serves again
    labels, _ = g2.search(Q, 5, ef=32)
    assert (labels >= 0).all() and (labels < 2000).all()
    g.close()
    g2.close()
    ix.close()


# =============================================================================
# certification survives
# =============================================================================
@pytest.mark.parametrize("c", rc.cert_cases(), ids=[rc.cert_id(c) for c in rc.cert_cases()])
def test_certification_survives_an_update(vdb, c):
    """Planted-gap data (tests/_planted.py): a random half of the rows take a shuffle of their own
    old values.  The multiset of rows -- the planted gap, mu / sx / dir and every statistic with
    it -- is the one tests/test_planted_precondition.py certifies, so every query must still
    certify unaided: exact results and no fallback, overflow or inconsistent query."""
    name, n, d, b, k, metric, precision = c
    V, Q, _ = pl.data(n, d, b, k, rc.cert_seed(n, d, b, k))
    rows, V2 = uc.cert_updated(n, d, b, k)
    ix = _index(vdb, V, metric, precision)
    _update(ix, rows, V2[rows])
    np.testing.assert_array_equal(ix.get_vectors(), V2)
    before = {s: ix.stat(s) for s in ("fallback_queries", "overflow_queries", "inconsistent_queries")}
    ran = ix.stat("searches_" + pl.resolved(precision, metric, k))
    got = _search(vdb, ix, Q, k)
    _assert_same(got, uc.cert_oracle(n, d, b, k, metric), rc.cert_id(c))
    assert ix.stat("searches_" + pl.resolved(precision, metric, k)) - ran == 1
    for s, v in before.items():
        assert ix.stat(s) - v == 0, s
    ix.close()

"""Row removal on the device (include/vdb.h vdb_index_remove; csrc/vdb_compact.hip).

After every remove the index must be what an index holding only the surviving rows is: the rows
bit for bit (``get_vectors`` against ``np.delete``), every search bit for bit -- indices, fp64 keys
and fp32 scores -- equal to ``oracle.ref_cpu.exact_search`` over ``np.delete(V, rows, axis=0)``,
under the index's candidate pass and with force_exact, unmasked and with a row_mask over the new
numbering, and no query flagged by the int8 pass's checksum (``inconsistent_queries``: the column
sums are exact integers, so stale sums or a non-zero vacated tail show there and nowhere else).

Case tables and their CPU preconditions: tests/_remove_cases.py, tests/test_remove_precondition.py.
Output buffers hold a poison value before each call (index -7, key and score NaN).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _planted as pl  # noqa: E402
import _remove_cases as rc  # noqa: E402
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
    i = np.full((nq, k), rc.POISON_IDX, np.int64)
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
    ix.add(V)                                                     # its eager copy is the one rebuilt
    assert ix.count() == V.shape[0]
    return ix


def _check_searches(vdb, ix, S, Q, k, metric, want=None, want_masked=None, what=""):
    """Unmasked and masked searches, under the index's pass and with force_exact, against the
    oracle over the surviving rows S; no query flagged as inconsistent."""
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


# =============================================================================
# patterns
# =============================================================================
@pytest.mark.parametrize("c", rc.pattern_cases(), ids=[rc.pattern_id(c) for c in rc.pattern_cases()])
def test_remove_patterns(vdb, c):
    D, metric, precision, name = c
    V, Q = rc.rows_data(rc.N, D, 100 + D)
    rows = rc.pattern_rows(name)
    ix = _index(vdb, V, metric, precision)
    cap, removed0 = ix.stat("capacity"), ix.stat("rows_removed")
    n = ix.remove(rc.pattern_words(name))
    S, want, want_masked = rc.pattern_oracle(name, D, metric)
    assert n == rows.size and ix.count() == rc.N - rows.size == S.shape[0]
    assert ix.stat("rows_removed") - removed0 == rows.size and ix.stat("capacity") == cap
    np.testing.assert_array_equal(ix.get_vectors(), S)
    _check_searches(vdb, ix, S, Q, rc.K, metric, want, want_masked, name)
    ix.close()


def test_remove_by_row_ids_equals_the_bitmap(vdb):
    V, Q = rc.rows_data(rc.N, 96, 196)
    rows = rc.pattern_rows("rand50")
    ix = _index(vdb, V, "cosine", "auto")
    assert ix.remove(rows[::-1].astype(np.int32)) == rows.size  # any order, any integer type
    np.testing.assert_array_equal(ix.get_vectors(), np.delete(V, rows, axis=0))
    ix.close()


# =============================================================================
# chunks and scan blocks
# =============================================================================
def test_many_chunks_and_scan_workgroups(vdb):
    """70 017 rows: 2 189 bitmap words, more than the 1024 one workgroup of the keep-count scan
    handles; remove_chunk = 1000 -> 71 chunks of 992 rows, one with no survivor, one with no
    removed row (tests/test_remove_precondition.py checks both)."""
    V, Q = rc.rows_data(rc.BIG_N, rc.BIG_D, 7)
    rows = rc.big_rows()
    ix = _index(vdb, V, "cosine", "auto")
    ix.set_param("remove_chunk", rc.BIG_CHUNK)
    assert ix.remove(rc.words_of(rows, rc.BIG_N)) == rows.size
    S, want = rc.big_oracle()
    assert ix.count() == S.shape[0]
    np.testing.assert_array_equal(ix.get_vectors(), S)
    _check_searches(vdb, ix, S, Q, rc.K, "cosine", want, None, "chunked")
    ix.close()


@pytest.mark.parametrize("D", rc.DIMS)
def test_one_word_per_chunk(vdb, D):
    V, Q = rc.rows_data(rc.N, D, 100 + D)
    ix = _index(vdb, V, "cosine", "auto")
    ix.set_param("remove_chunk", 32)
    assert ix.remove(rc.pattern_words("every_other")) == rc.pattern_rows("every_other").size
    S, want, want_masked = rc.pattern_oracle("every_other", D, "cosine")
    np.testing.assert_array_equal(ix.get_vectors(), S)
    _check_searches(vdb, ix, S, Q, rc.K, "cosine", want, want_masked, "32-row chunks")
    ix.close()


# =============================================================================
# the lazily built split copy
# =============================================================================
@pytest.mark.parametrize("metric", pl.BOTH)
def test_lazy_split_copy_is_rebuilt(vdb, metric):
    """Under auto the split copy exists only once a search needed one.  A bf16x3 search makes it
    exist (the precision set and set back: the copy stays allocated and auto keeps it up to
    date); after the remove a bf16x3 search reads it without another rebuild (same copy kind)."""
    V, Q = rc.rows_data(rc.N, 200, 300)
    ix = _index(vdb, V, metric, "auto")
    assert ix.stat("split_copy") == 0
    ix.set_precision("bf16x3")
    _assert_same(_search(vdb, ix, Q, rc.K), ref_cpu.exact_search(Q, V, rc.K, metric), "before")
    ix.set_precision("auto")
    assert ix.stat("split_copy") == 1
    rows = rc.pattern_rows("rand50")
    assert ix.remove(rows) == rows.size
    S = np.delete(V, rows, axis=0)
    ix.set_precision("bf16x3")
    builds = ix.stat("split_copy_builds")
    _check_searches(vdb, ix, S, Q, rc.K, metric, what="bf16x3 after remove")
    assert ix.stat("searches_bf16x3") >= 3 and ix.stat("split_copy_builds") == builds
    ix.close()


# =============================================================================
# remove, add, remove
# =============================================================================
@pytest.mark.parametrize("metric,precision", [("cosine", "auto"), ("euclidean", "auto"), ("cosine", "bf16x3")])
def test_remove_then_add_then_remove(vdb, metric, precision):
    V, Q = rc.rows_data(rc.N, 96, 196)
    fresh = np.random.default_rng(55).standard_normal((300, 96)).astype(np.float32)
    ix = _index(vdb, V, metric, precision)
    rows = rc.pattern_rows("block")
    assert ix.remove(rows) == rows.size
    ix.add(fresh)
    S = np.concatenate([np.delete(V, rows, axis=0), fresh])
    assert ix.count() == S.shape[0]
    np.testing.assert_array_equal(ix.get_vectors(), S)
    _check_searches(vdb, ix, S, Q, rc.K, metric, what="after add")
    rows2 = np.sort(np.random.default_rng(56).permutation(S.shape[0])[:900])  # old and fresh rows
    assert ix.remove(rows2) == rows2.size
    S2 = np.delete(S, rows2, axis=0)
    np.testing.assert_array_equal(ix.get_vectors(), S2)
    _check_searches(vdb, ix, S2, Q, rc.K, metric, what="after the second remove")
    assert ix.stat("rows_removed") == rows.size + rows2.size
    ix.close()


# =============================================================================
# remove all
# =============================================================================
@pytest.mark.parametrize("metric", pl.BOTH)
def test_remove_all(vdb, metric):
    V, Q = rc.rows_data(rc.N, 96, 196)
    ix = _index(vdb, V, metric, "auto")
    cap = ix.stat("capacity")
    assert ix.remove(np.arange(rc.N)) == rc.N
    assert ix.count() == 0 and ix.stat("capacity") == cap
    s, i, kk = _search(vdb, ix, Q, rc.K)
    assert (i == -1).all() and (s == 0).all() and (kk == -np.inf).all()
    assert ix.remove(np.zeros(1, np.uint32)) == 0  # an empty index: nothing to remove
    W = V[:1777] * np.float32(0.5)
    ix.add(W)
    np.testing.assert_array_equal(ix.get_vectors(), W)
    _check_searches(vdb, ix, W, Q, rc.K, metric, what="add after remove-all")
    ix.close()


# =============================================================================
# a queued search sees the rows as they were
# =============================================================================
@pytest.mark.parametrize("metric", pl.BOTH)
def test_queued_search_then_remove_without_synchronising(vdb, metric):
    import torch
    V, Q = rc.rows_data(rc.N, 96, 196)
    ix = _index(vdb, V, metric, "auto")
    qd = torch.from_numpy(np.array(Q)).cuda()
    outs = []
    for _ in range(3):
        outs.append((torch.full((rc.B, rc.K), float("nan"), dtype=torch.float32, device="cuda"),
                     torch.full((rc.B, rc.K), rc.POISON_IDX, dtype=torch.int64, device="cuda"),
                     torch.full((rc.B, rc.K), float("nan"), dtype=torch.float64, device="cuda")))
    torch.cuda.synchronize()  # (the poison fills run on torch's stream)
    st = torch.cuda.Stream()
    for bufs in outs:
        ix.search_device(qd.data_ptr(), rc.B, rc.K, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                         stream=st.cuda_stream)
    rows = rc.pattern_rows("rand50")
    assert ix.remove(rows) == rows.size  # at once: the remove itself waits for the queued searches
    torch.cuda.synchronize()
    want_before = ref_cpu.exact_search(Q, V, rc.K, metric)
    for n, bufs in enumerate(outs):
        _assert_same(tuple(b.cpu().numpy() for b in bufs), want_before, f"queued search {n}: the pre-remove rows")
    S, want, want_masked = rc.pattern_oracle("rand50", 96, metric)  # (the same rows and queries)
    _check_searches(vdb, ix, S, Q, rc.K, metric, want, want_masked, "after")
    ix.close()


def test_device_memory_mask(vdb):
    """The bitmap in device memory, written on a side stream just before the call."""
    import torch
    V, Q = rc.rows_data(rc.N, 96, 196)
    rows = rc.pattern_rows("rand50")
    ix = _index(vdb, V, "cosine", "auto")
    words = torch.from_numpy(rc.words_of(rows, rc.N).view(np.int32))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        md = words.cuda(non_blocking=True)
    assert ix.remove_device(md.data_ptr(), stream=st.cuda_stream) == rows.size
    S = np.delete(V, rows, axis=0)
    np.testing.assert_array_equal(ix.get_vectors(), S)
    _check_searches(vdb, ix, S, Q, rc.K, "cosine", what="device mask")
    ix.close()


# =============================================================================
# certification survives
# =============================================================================
@pytest.mark.parametrize("c", rc.cert_cases(), ids=[rc.cert_id(c) for c in rc.cert_cases()])
def test_certification_survives_a_remove(vdb, c):
    """Planted-gap data (tests/_planted.py): a quarter of the rows outside every query's top k
    removed.  The gap over the survivors is >= 6 eps_upper of the original corpus
    (tests/test_remove_precondition.py), and mu / sx / dir / the statistics are the original's,
    so every query must still certify unaided: exact results and no fallback, overflow or
    inconsistent query."""
    name, n, d, b, k, metric, precision = c
    V, Q, _ = pl.data(n, d, b, k, rc.cert_seed(n, d, b, k))
    removed = rc.cert_removed(n, d, b, k)
    ix = _index(vdb, V, metric, precision)
    assert ix.remove(removed) == removed.size
    before = {s: ix.stat(s) for s in ("fallback_queries", "overflow_queries", "inconsistent_queries")}
    ran = ix.stat("searches_" + pl.resolved(precision, metric, k))
    got = _search(vdb, ix, Q, k)
    _assert_same(got, rc.cert_oracle(n, d, b, k, metric), rc.cert_id(c))
    assert ix.stat("searches_" + pl.resolved(precision, metric, k)) - ran == 1
    for s, v in before.items():
        assert ix.stat(s) - v == 0, s
    ix.close()


# =============================================================================
# errors
# =============================================================================
def test_errors_change_nothing(vdb):
    V, Q = rc.rows_data(rc.N, 96, 196)
    ix = _index(vdb, V[:500], "cosine", "auto")
    n = ctypes.c_int64(-5)
    assert ix._lib.vdb_index_remove(ix._h, None, vdb.MEM_HOST, None, ctypes.byref(n)) == vdb.VDB_ERR_INVALID
    assert n.value == 0
    assert ix._lib.vdb_index_remove(ix._h, None, vdb.MEM_DEVICE, None, None) == vdb.VDB_ERR_INVALID
    with pytest.raises(ValueError):
        ix.remove_device(0)
    for bad in ([500], [-1], [3, 4, 500], np.array([2 ** 40])):
        with pytest.raises(ValueError):
            ix.remove(bad)
    with pytest.raises(ValueError):
        ix.remove(np.zeros(3, np.uint32))  # a bitmap too short for 500 rows
    with pytest.raises(ValueError):
        ix.remove(np.array([1.0, 2.0]))
    with pytest.raises(ValueError):
        ix.set_param("remove_chunk", -1)
    assert ix.count() == 500 and ix.stat("rows_removed") == 0
    np.testing.assert_array_equal(ix.get_vectors(), V[:500])
    _assert_same(_search(vdb, ix, Q, rc.K), ref_cpu.exact_search(Q, V[:500], rc.K, "cosine"))
    ix.close()


# =============================================================================
# a graph built before a remove is stale for good
# =============================================================================
def test_graph_is_stale_after_a_remove_even_at_equal_count(vdb):
    V, Q = rc.rows_data(rc.N, 96, 196)
    ix = _index(vdb, V[:2000], "cosine", "auto")
    g = vdb.NativeGraph.build(ix, degree=16, knn=16, n_entries=64)
    labels, _ = g.search(Q, 5, ef=32)
    assert (labels >= 0).all()
    assert ix.remove(np.arange(100, 110)) == 10
    with pytest.raises(ValueError, match="stale"):
        g.search(Q, 5, ef=32)
    ix.add(V[2000:2010])
    assert ix.count() == g.info()[0] == 2000  # the count is what the graph recorded
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

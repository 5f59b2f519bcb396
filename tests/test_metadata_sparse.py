"""The store's sparse column builder and query normaliser
(mlx-vector-db_amd/service/optimized_vector_store.py build_sparse_column, normalize_sparse_query,
clip_sparse_query): a row's sparse vector is its metadata under a key, sorted per row; a repeated index
is refused; a row without the key is empty; n_terms is one more than the largest index seen.  What they
build is what vdb_index_set_sparse / vdb_index_search_sparse accept (the same rules the plan header
checks).  No GPU."""
import json

import numpy as np
import pytest

from service import _vdb
from service import optimized_vector_store as ovs


def _meta():
    return [
        {"id": 0, "sparse": {"indices": [9, 2, 5], "values": [0.5, 1.5, -2.0]}},   # unsorted
        {"id": 1},                                                                   # no key
        {"id": 2, "sparse": {"indices": [], "values": []}},                          # empty
        {"id": 3, "sparse": {"indices": [30521], "values": [3.0]}, "lexical": {"indices": [1], "values": [1.0]}},
        {"id": 4, "sparse": {"indices": [0, 30521], "values": [0.0, 1.0]}},          # a stored zero weight stays
    ]


def test_column_sorts_rows_skips_missing_keys_and_counts_terms():
    indptr, terms, weights, n_terms = ovs.build_sparse_column(_meta(), 5)
    assert indptr.dtype == np.int64 and terms.dtype == np.int32 and weights.dtype == np.float32
    assert indptr.tolist() == [0, 3, 3, 3, 4, 6]
    assert terms.tolist() == [2, 5, 9, 30521, 0, 30521]
    assert weights.tolist() == [1.5, -2.0, 0.5, 3.0, 0.0, 1.0]
    assert n_terms == 30522
    # another key, the first rows only, rows past the metadata, and no entry at all
    indptr, terms, weights, n_terms = ovs.build_sparse_column(_meta(), 5, "lexical")
    assert indptr.tolist() == [0, 0, 0, 0, 1, 1] and terms.tolist() == [1] and n_terms == 2
    indptr, terms, weights, n_terms = ovs.build_sparse_column(_meta(), 2)
    assert indptr.tolist() == [0, 3, 3] and n_terms == 10
    indptr, terms, weights, n_terms = ovs.build_sparse_column(_meta(), 7)
    assert indptr.tolist() == [0, 3, 3, 3, 4, 6, 6, 6]
    indptr, terms, weights, n_terms = ovs.build_sparse_column(_meta(), 5, "absent")
    assert indptr.tolist() == [0] * 6 and terms.size == 0 and n_terms == 0
    # every row the builder returns is strictly ascending: what the library requires
    indptr, terms, _, _ = ovs.build_sparse_column(_meta(), 5)
    for r in range(5):
        assert (np.diff(terms[indptr[r]:indptr[r + 1]].astype(np.int64)) > 0).all()
    # the metadata survives the store's JSON lines unchanged
    again = [json.loads(json.dumps(m)) for m in _meta()]
    for a, b in zip(ovs.build_sparse_column(again, 5), ovs.build_sparse_column(_meta(), 5)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("bad, word", [
    ({"indices": [3, 7, 3], "values": [1, 1, 1]}, "repeated"),
    ({"indices": [3, 7], "values": [1.0]}, "values"),
    ({"indices": [-1], "values": [1.0]}, "indices"),
    ({"indices": [2 ** 31 - 1], "values": [1.0]}, "indices"),
    ({"indices": [1.5], "values": [1.0]}, "integers"),
    ({"indices": [1], "values": [float("nan")]}, "finite"),
    ({"indices": [1], "values": [1e39]}, "finite"),
    ({"indices": [1]}, "indices"),
    ([1, 2], "indices"),
])
def test_bad_sparse_vectors_are_refused(bad, word):
    with pytest.raises(ValueError, match=word):
        ovs.build_sparse_column([{"sparse": bad}], 1)
    with pytest.raises(ValueError, match=word):
        ovs.normalize_sparse_query(bad)


def test_query_normalisation():
    idx, val = ovs.normalize_sparse_query({"indices": [9, 2, 5, 7], "values": [0.5, 1.5, 0.0, -2.0]})
    assert idx.tolist() == [2, 7, 9] and val.tolist() == [1.5, -2.0, 0.5] and val.dtype == np.float32
    idx, val = ovs.normalize_sparse_query(None)
    assert idx.size == 0 and val.size == 0
    idx, val = ovs.normalize_sparse_query({"indices": [], "values": []})
    assert idx.size == 0
    n = ovs.SPARSE_MAX_QUERY_TERMS
    assert n == 1024 and ovs.SPARSE_MAX_K == 1024
    ok = ovs.normalize_sparse_query({"indices": list(range(n)), "values": [1.0] * n})
    assert ok[0].size == n
    # zeros are dropped before the length is judged
    ok = ovs.normalize_sparse_query({"indices": list(range(n + 5)), "values": [1.0] * n + [0.0] * 5})
    assert ok[0].size == n
    with pytest.raises(ValueError, match="1024"):
        ovs.normalize_sparse_query({"indices": list(range(n + 1)), "values": [1.0] * (n + 1)})
    # indices at or past n_terms are dropped: no row can hold them
    t, w = ovs.clip_sparse_query(ovs.normalize_sparse_query({"indices": [1, 10, 11, 2 ** 31 - 2], "values": [1, 2, 3, 4]}), 11)
    assert t.tolist() == [1, 10] and w.tolist() == [1.0, 2.0] and t.dtype == np.int32
    # and the packed triple is what the binding takes
    ip, tt, ww = _vdb.pack_sparse_vectors([(t, w), None, ((), ())])
    assert ip.tolist() == [0, 2, 2, 2] and tt.tolist() == [1, 10] and ww.dtype == np.float32 and ip.dtype == np.int64

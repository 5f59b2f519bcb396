"""Recommend reads through the store (service/optimized_vector_store.py ``recommend`` /
``batch_recommend``), on the GPU: the rows, their order and their scores are exactly the oracle's
(tests/_recommend_cases.py ``expected`` with the filter as the mask), with each row's metadata; by
row index and by a metadata key's value."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _recommend_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
N, D = 600, 48
METRICS = rc.METRICS


@pytest.fixture(scope="module")
def store_mod():
    from service import _vdb, optimized_vector_store
    assert _vdb.device_count() >= 1, "no GPU visible"
    return optimized_vector_store


def _mk(store_mod, path, metric="cosine", **kw):
    return store_mod.MLXVectorStore(str(path), store_mod.MLXVectorStoreConfig(dimension=D, metric=metric, **kw))


def _data():
    V, _ = rc.corpus(N, D, seed=4)
    # three chunks per document (doc 0 = rows 0, 200, 400), and one document of 70 chunks
    meta = [{"id": i, "doc_id": f"doc_{i % 200}", "lang": "en" if i % 3 else "de"} for i in range(N)]
    for i in range(70):
        meta[5 + 7 * i]["big"] = "yes"
    return V, meta


def _rows_of(meta, key, value):
    return [i for i, m in enumerate(meta) if m.get(key) == value]


def _want(V, meta, metric, pos, neg, k, filt=None):
    """The contract for one query: (indices, scores, metadata)."""
    mask = None if not filt else np.array([all(m.get(a) == b for a, b in filt.items()) for m in meta])
    s, i, _, _ = rc.expected(V, [pos], [neg or []], k, metric, mask)
    rows = i[0][i[0] >= 0].tolist()
    return rows, s[0][:len(rows)].astype(np.float64).tolist(), [meta[r] for r in rows]


@pytest.mark.parametrize("metric", METRICS)
def test_recommend_reads_match_the_oracle(store_mod, tmp_path, metric):
    V, meta = _data()
    st = _mk(store_mod, tmp_path / "s", metric, persist=False)
    st.add_vectors(V, meta)
    before = st._index.stat("recommend_searches")
    for filt in (None, {"lang": "de"}):
        for pos, neg, k in (([17], None, 5), ([17, 240, 3], [9], 10), ([599], [0, 1, 2, 3], 136), ([4, 4, 8], [8], 1)):
            assert st.recommend(pos, neg, k=k, filter_metadata=filt) == _want(V, meta, metric, pos, neg, k, filt), (pos, k)
    assert st.recommend([17]) == _want(V, meta, metric, [17], None, 10)  # the defaults
    assert st.recommend(np.asarray([17, 3]), np.asarray([5])) == _want(V, meta, metric, [17, 3], [5], 10)
    # by key: every row holding the value is an example
    d7 = _rows_of(meta, "doc_id", "doc_7")
    assert d7 == [7, 207, 407]
    assert st.recommend(["doc_7"], key="doc_id", k=8) == _want(V, meta, metric, d7, None, 8)
    d9 = _rows_of(meta, "doc_id", "doc_9")
    got = st.recommend(["doc_7", "doc_9"], ["doc_30"], key="doc_id", k=8, filter_metadata={"lang": "en"})
    assert got == _want(V, meta, metric, d7 + d9, _rows_of(meta, "doc_id", "doc_30"), 8, {"lang": "en"})
    assert not set(got[0]) & set(d7 + d9)
    assert st.recommend([7], key="id", k=3) == _want(V, meta, metric, [7], None, 3)
    # one device call for a batch
    calls = st._index.stat("recommend_searches")
    reqs = [([17], None), ([17, 240, 3], [9]), ([], [4]), ([2], [])]
    batch = st.batch_recommend(reqs, k=6, filter_metadata={"lang": "en"})
    assert st._index.stat("recommend_searches") == calls + 1
    assert batch == [_want(V, meta, metric, p, g, 6, {"lang": "en"}) if p else ([], [], []) for p, g in reqs]
    assert st._index.stat("recommend_searches") > before and st._index.stat("recommend_bad_queries") == 0


def test_recommend_limits_and_empty_answers(store_mod, tmp_path):
    V, meta = _data()
    st = _mk(store_mod, tmp_path / "s", "cosine", persist=False)
    # an empty store answers without a device call
    assert st.recommend([], k=5) == ([], [], [])
    st.add_vectors(V, meta)
    calls = st._index.stat("recommend_searches")
    assert st.recommend([], k=5) == ([], [], [])
    assert st.recommend([], [3], k=5) == ([], [], [])
    assert st.recommend([3], filter_metadata={"lang": "xx"}) == ([], [], [])
    assert st.batch_recommend([], k=5) == []
    assert st._index.stat("recommend_searches") == calls
    with pytest.raises(ValueError, match="doc_nope"):
        st.recommend(["doc_nope"], key="doc_id")
    with pytest.raises(ValueError, match="64"):
        st.recommend(["yes"], key="big")  # 70 rows hold it
    with pytest.raises(ValueError, match="64"):
        st.recommend(list(range(40)), list(range(100, 125)))
    for k in (0, 137, -1):
        with pytest.raises(ValueError, match="136"):
            st.recommend([3], k=k)
    for bad in ([N], [-1], [1.5], ["7"], [True]):
        with pytest.raises(ValueError):
            st.recommend(bad)
        with pytest.raises(ValueError):
            st.recommend([3], bad)
    assert st._index.stat("recommend_searches") == calls
    assert len(st.recommend(list(range(40)), list(range(100, 124)), k=136)[0]) == 136


def test_recommend_by_key_after_delete(store_mod, tmp_path):
    V, meta = _data()
    st = _mk(store_mod, tmp_path / "s", "euclidean", persist=False)
    st.add_vectors(V, meta)
    gone = [0, 7, 100, 350]
    st.delete_rows(gone)
    keep = np.setdiff1d(np.arange(N), gone)
    V2, meta2 = V[keep], [meta[i] for i in keep]
    d7 = _rows_of(meta2, "doc_id", "doc_7")
    assert len(d7) == 2 and d7 != [207, 407]  # the ids moved down
    assert st.recommend(["doc_7"], ["doc_150"], key="doc_id", k=9) == \
        _want(V2, meta2, "euclidean", d7, _rows_of(meta2, "doc_id", "doc_150"), 9)
    assert st.recommend([N - 5]) == _want(V2, meta2, "euclidean", [N - 5], None, 10)
    with pytest.raises(ValueError):
        st.recommend([N - 4])

"""Weighted-sum hybrid reads through the store (service/optimized_vector_store.py ``hybrid_sum_query`` /
``batch_hybrid_sum_query``), on the GPU: the rows, their order, scores and the two parts are exactly
the oracle's (tests/_hybsum_cases.py ``expected`` over the column the rows' metadata describes, with
the filter as the mask), with each row's metadata: with a metadata filter, on a store where no row has
a sparse entry, after an upsert that changes a row's sparse metadata (the column survives the vector
update and is rebuilt for the metadata) and after an add and a delete."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hybsum_cases as hs  # noqa: E402

sp, fc = hs.sp, hs.fc
pytestmark = pytest.mark.gpu
N, D = 600, 48
METRICS = hs.METRICS
EMPTY5 = ([], [], [], [], [])
VOCAB = 400


@pytest.fixture(scope="module")
def store_mod():
    from service import _vdb, optimized_vector_store
    assert _vdb.device_count() >= 1, "no GPU visible"
    return optimized_vector_store


def _mk(store_mod, path, metric="cosine", **kw):
    return store_mod.MLXVectorStore(str(path), store_mod.MLXVectorStoreConfig(dimension=D, metric=metric, **kw))


def _data():
    V, Q = fc.corpus(N, D, seed=4)
    rng = np.random.default_rng(2)
    meta = []
    for i in range(N):
        m = {"id": i, "lang": "en" if i % 3 else "de", "section": int(rng.integers(0, 4))}
        if i % 11:  # every eleventh row has no sparse vector
            t = rng.choice(VOCAB, size=int(rng.integers(1, 40)), replace=False)  # unsorted, as a tokenizer gives them
            m["sparse"] = {"indices": t.tolist(), "values": [float(v) for v in rng.integers(1, 4, size=t.size)]}
            m["title"] = {"indices": [int(i % 5)], "values": [1.0 + (i % 2)]}
        meta.append(m)
    qs = []
    for j in range(3):
        t = rng.choice(VOCAB + 20, size=12, replace=False)  # some terms no row holds
        qs.append({"indices": t.tolist(), "values": [float(v) for v in rng.integers(1, 3, size=12)]})
    return V, meta, Q, qs


def _column(store_mod, meta, key="sparse"):
    ip, t, w, nt = store_mod.build_sparse_column(meta, len(meta), key)
    return sp.Column([(t[ip[r]:ip[r + 1]], w[ip[r]:ip[r + 1]]) for r in range(len(meta))], max(nt, 1)), max(nt, 1)


def _mask(meta, filt):
    return None if not filt else np.array([all(m.get(a) == b for a, b in filt.items()) for m in meta])


def _want(store_mod, q, sparse, V, meta, metric, k, weights=(1.0, 1.0), filt=None, key="sparse"):
    col, nt = _column(store_mod, meta, key)
    sq = store_mod.clip_sparse_query(store_mod.normalize_sparse_query(sparse), nt)
    s, i, f, d, p = hs.expected(V, np.asarray(q, np.float32)[None, :], col, [sq], k, metric, weights, _mask(meta, filt))
    rows = i[0][i[0] >= 0].tolist()
    n = len(rows)
    return (rows, s[0][:n].astype(np.float64).tolist(), [meta[r] for r in rows], d[0][:n].tolist(), p[0][:n].tolist())


@pytest.mark.parametrize("metric", METRICS)
def test_reads_match_the_oracle(store_mod, tmp_path, metric):
    V, meta, Q, qs = _data()
    st = _mk(store_mod, tmp_path / "s", metric, persist=False)
    st.add_vectors(V, meta)
    for filt in (None, {"lang": "de"}, {"lang": "de", "section": 1}):
        for k, weights in ((1, (1.0, 1.0)), (10, (0.3, 0.7)), (600, (1.0, 0.05))):
            batch = st.batch_hybrid_sum_query(Q[:3], qs, k=k, weights=weights, filter_metadata=filt)
            assert len(batch) == 3
            for b in range(3):
                assert batch[b] == _want(store_mod, Q[b], qs[b], V, meta, metric, k, weights, filt), (b, filt, k)
            assert st.hybrid_sum_query(Q[1], qs[1], k=k, weights=weights, filter_metadata=filt) == batch[1]
    assert st._index.stat("sparse_sets") == 1  # the column was built once
    # every row is a candidate, the rows without a sparse vector included (sparse part 0)
    got = st.hybrid_sum_query(Q[0], qs[0], k=600)
    assert len(got[0]) == N and {r for r in got[0] if r % 11 == 0} and all(p == 0 for r, p in zip(got[0], got[4]) if r % 11 == 0)
    # Pinecone's alpha: weights = (alpha, 1 - alpha); alpha = 1 is the plain query's rows, in its order
    assert st.hybrid_sum_query(Q[2], qs[2], k=7, weights=(1.0, 0.0))[0] == list(st.query(Q[2], k=7, use_hnsw=False)[0])
    # alpha = 0: the sparse query's rows first, in its order
    srows = st.sparse_query(qs[2], k=7)[0]
    assert st.hybrid_sum_query(Q[2], qs[2], k=7, weights=(0.0, 1.0))[0] == srows
    # another key: its own column replaces the first
    sv = {"indices": [3], "values": [1.0]}
    assert st.hybrid_sum_query(Q[0], sv, k=20, sparse_key="title") == _want(store_mod, Q[0], sv, V, meta, metric, 20, key="title")
    # no row has the key: the read ranks by the dense key alone, every sparse part 0
    got = st.hybrid_sum_query(Q[0], qs[0], k=5, sparse_key="absent")
    assert got == _want(store_mod, Q[0], qs[0], V, meta, metric, 5, key="absent")
    assert got[0] == list(st.query(Q[0], k=5, use_hnsw=False)[0]) and got[4] == [0.0] * 5
    # a query without terms, and None: the dense ranking
    for none in ({"indices": [], "values": []}, None):
        assert st.hybrid_sum_query(Q[0], none, k=5)[0] == got[0]


def test_a_store_where_no_row_has_a_sparse_entry(store_mod, tmp_path):
    V, meta, Q, qs = _data()
    bare = [{"id": m["id"], "lang": m["lang"]} for m in meta]
    st = _mk(store_mod, tmp_path / "b", persist=False)
    st.add_vectors(V, bare)
    got = st.hybrid_sum_query(Q[0], qs[0], k=10, weights=(0.5, 0.5), filter_metadata={"lang": "en"})
    assert got == _want(store_mod, Q[0], qs[0], V, bare, "cosine", 10, (0.5, 0.5), {"lang": "en"})
    assert len(got[0]) == 10 and got[4] == [0.0] * 10
    assert st.hybrid_sum_query(Q[0], qs[0], k=10, weights=(0.0, 1.0))[0] == list(range(10))  # every value +0.0: id order


def test_column_follows_upsert_add_and_delete(store_mod, tmp_path):
    V0, meta0, Q, qs = _data()
    V, meta = V0.copy(), [dict(m) for m in meta0]
    st = _mk(store_mod, tmp_path / "p", persist=False)
    st.add_vectors(V, meta)
    assert st.hybrid_sum_query(Q[0], qs[0], k=10) == _want(store_mod, Q[0], qs[0], V, meta, "cosine", 10)
    sets = st._index.stat("sparse_sets")
    # an upsert gives row 5 every term of the query with a large weight (the column is rebuilt for the
    # changed metadata), and adds a row with no sparse vector (an add drops the column)
    t = qs[0]["indices"]
    new_meta = [dict(meta[5], sparse={"indices": t, "values": [9.0] * len(t)}), {"id": "new", "lang": "de", "section": 0}]
    new_vecs = np.stack([V[5], -Q[0]]).astype(np.float32)
    assert st.upsert_vectors(new_vecs, new_meta, key="id")["updated"] == 1
    meta[5] = new_meta[0]
    meta.append(new_meta[1])
    V = np.concatenate([V, new_vecs[1:]])
    got = st.hybrid_sum_query(Q[0], qs[0], k=10)
    assert got == _want(store_mod, Q[0], qs[0], V, meta, "cosine", 10) and got[0][0] == 5
    assert st._index.stat("sparse_sets") > sets
    # a vector-only upsert: the index keeps its column through the update and the read sees the new vector
    st.upsert_vectors(Q[1][None, :], [dict(meta[9])], key="id")
    V[9] = Q[1]
    got = st.hybrid_sum_query(Q[1], qs[1], k=10, weights=(5.0, 0.01))
    assert got == _want(store_mod, Q[1], qs[1], V, meta, "cosine", 10, (5.0, 0.01)) and got[0][0] == 9
    # a delete moves the rows: the column follows
    st.delete_rows([0])
    V, meta = V[1:], meta[1:]
    for b in range(3):
        assert st.hybrid_sum_query(Q[b], qs[b], k=10, filter_metadata={"lang": "en"}) == \
            _want(store_mod, Q[b], qs[b], V, meta, "cosine", 10, filt={"lang": "en"})


def test_no_device_call_when_nothing_can_match_and_bad_arguments(store_mod, tmp_path):
    V, meta, Q, qs = _data()
    st = _mk(store_mod, tmp_path / "s", persist=False)
    assert st.hybrid_sum_query(Q[0], qs[0]) == EMPTY5 and st.batch_hybrid_sum_query(Q[:2], qs[:2]) == [EMPTY5, EMPTY5]  # empty store
    st.add_vectors(V, meta)
    assert st.hybrid_sum_query(Q[0], qs[0], filter_metadata={"lang": "xx"}) == EMPTY5  # a filter nothing matches
    assert st.batch_hybrid_sum_query(Q[:0], []) == []
    assert st._index.stat("hybrid_sum_searches") == 0 and st._index.stat("sparse_sets") == 0
    nan = float("nan")
    for bad_sv, word in (({"indices": [3, 3], "values": [1.0, 1.0]}, "repeated"),
                         ({"indices": list(range(1025)), "values": [1.0] * 1025}, "1024"), ({"indices": [1]}, "indices")):
        with pytest.raises(ValueError, match=word):
            st.hybrid_sum_query(Q[0], bad_sv)
    for bad, word in ((dict(k=0), "k must"), (dict(k=1025), "1024"), (dict(weights=(1.0,)), "weights"),
                      (dict(weights=(1.0, nan)), "weights"), (dict(weights=(-1.0, 1.0)), "weights"),
                      (dict(weights=(1.0, float("inf"))), "weights"), (dict(weights=(1.0, 2.0 ** 65)), "weights"),
                      (dict(weights=(1.0, 1.0, 1.0)), "weights")):
        with pytest.raises(ValueError, match=word):
            st.hybrid_sum_query(Q[0], qs[0], **bad)
    with pytest.raises(ValueError, match="Dimension mismatch"):
        st.hybrid_sum_query(np.ones(D + 1, np.float32), qs[0])
    with pytest.raises(ValueError, match="batch_hybrid_sum_query"):
        st.hybrid_sum_query(np.ones((2, D), np.float32), qs[0])
    with pytest.raises(ValueError, match="sparse vectors"):
        st.batch_hybrid_sum_query(Q[:2], qs[:1])
    assert st._index.stat("hybrid_sum_searches") == 0
    assert len(st.hybrid_sum_query(Q[0], qs[0], k=1024, weights=(2.0 ** 64, 0.0))[0]) == N
    assert st._index.stat("hybrid_sum_searches") == 1 and st._index.stat("hybrid_sum_queries") == 1


def test_multi_device_store_refuses(store_mod, tmp_path):
    st = _mk(store_mod, tmp_path / "m", devices=[0, 0], persist=False)
    V, meta, Q, qs = _data()
    st.add_vectors(V[:100], meta[:100])
    for call in (lambda: st.hybrid_sum_query(Q[0], qs[0]), lambda: st.batch_hybrid_sum_query(Q[:2], qs[:2])):
        with pytest.raises(NotImplementedError, match="hybrid sum query is not supported on a multi-device store"):
            call()

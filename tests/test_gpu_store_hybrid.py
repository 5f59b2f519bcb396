"""Sparse and hybrid reads through the store (service/optimized_vector_store.py ``sparse_query`` /
``hybrid_query`` and their batch forms), on the GPU: the rows, their order, scores, fused values and hit
counts are exactly the oracle's (tests/_sparse_cases.py ``expected`` / ``expected_hybrid`` over the
column the rows' metadata describes, with the filter as the mask), with each row's metadata: with a
metadata filter, after an upsert that changes a row's sparse metadata (the column is rebuilt) and after
save and load."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sparse_cases as sp  # noqa: E402

fc = sp.fc
pytestmark = pytest.mark.gpu
N, D = 600, 48
METRICS = sp.METRICS
EMPTY3 = ([], [], [])
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
    return sp.Column([(t[ip[r]:ip[r + 1]], w[ip[r]:ip[r + 1]]) for r in range(len(meta))], max(nt, 1)), nt


def _q(store_mod, sparse, nt):
    return store_mod.clip_sparse_query(store_mod.normalize_sparse_query(sparse), nt)


def _mask(meta, filt):
    return None if not filt else np.array([all(m.get(a) == b for a, b in filt.items()) for m in meta])


def _want_sparse(store_mod, sparse, meta, k, filt=None, key="sparse"):
    col, nt = _column(store_mod, meta, key)
    s, i, ke = sp.expected(col, [_q(store_mod, sparse, nt)], k, _mask(meta, filt))
    rows = i[0][i[0] >= 0].tolist()
    return rows, s[0][:len(rows)].astype(np.float64).tolist(), [meta[r] for r in rows]


def _want_hybrid(store_mod, q, sparse, V, meta, metric, k, fetch_k, weights=(1.0, 1.0), rrf_c=60.0, filt=None, key="sparse"):
    col, nt = _column(store_mod, meta, key)
    s, i, f, h = sp.expected_hybrid(V, np.asarray(q, np.float32)[None, :], col, [_q(store_mod, sparse, nt)], k, fetch_k, metric,
                                    weights, rrf_c, _mask(meta, filt))
    rows = i[0][i[0] >= 0].tolist()
    n = len(rows)
    return (rows, s[0][:n].astype(np.float64).tolist(), [meta[r] for r in rows], f[0][:n].tolist(), h[0][:n].tolist())


@pytest.mark.parametrize("metric", METRICS)
def test_sparse_and_hybrid_reads_match_the_oracle(store_mod, tmp_path, metric):
    V, meta, Q, qs = _data()
    st = _mk(store_mod, tmp_path / "s", metric, persist=False)
    st.add_vectors(V, meta)
    for filt in (None, {"lang": "de"}, {"lang": "de", "section": 1}):
        for k in (1, 10, 600):
            batch = st.batch_sparse_query(qs, k=k, filter_metadata=filt)
            assert len(batch) == 3
            for b in range(3):
                assert batch[b] == _want_sparse(store_mod, qs[b], meta, k, filt), (b, filt, k)
            assert st.sparse_query(qs[1], k=k, filter_metadata=filt) == batch[1]
        for k, fetch in ((1, 1), (5, 20), (200, 200)):
            batch = st.batch_hybrid_query(Q[:3], qs, k=k, fetch_k=fetch, filter_metadata=filt)
            for b in range(3):
                assert batch[b] == _want_hybrid(store_mod, Q[b], qs[b], V, meta, metric, k, fetch, filt=filt), (b, filt, k)
            assert st.hybrid_query(Q[1], qs[1], k=k, fetch_k=fetch, filter_metadata=filt) == batch[1]
    assert st._index.stat("sparse_sets") == 1  # the column was built once
    # weights and rrf_c travel; the default fetch_k is min(200, max(k, 4 k))
    assert st.hybrid_query(Q[0], qs[0], k=10, weights=(2.0, 0.5), rrf_c=10.0) == \
        _want_hybrid(store_mod, Q[0], qs[0], V, meta, metric, 10, 40, (2.0, 0.5), 10.0)
    for k, fetch in ((1, 4), (10, 40), (60, 200)):
        assert st.hybrid_query(Q[0], qs[0], k=k) == _want_hybrid(store_mod, Q[0], qs[0], V, meta, metric, k, fetch), k
    # a sparse weight of 0: the plain query's rows, in its order
    rows = st.hybrid_query(Q[2], qs[2], k=7, weights=(1.0, 0.0))[0]
    assert rows == list(st.query(Q[2], k=7, use_hnsw=False)[0])
    # another key: its own column replaces the first, and the first comes back
    assert st.sparse_query({"indices": [3], "values": [1.0]}, k=20, sparse_key="title") == \
        _want_sparse(store_mod, {"indices": [3], "values": [1.0]}, meta, 20, key="title")
    assert st.sparse_query(qs[0], k=5) == _want_sparse(store_mod, qs[0], meta, 5)
    assert st._index.stat("sparse_sets") == 3
    # no row has the key: nothing matches; the hybrid read ranks by the dense list alone
    assert st.sparse_query(qs[0], sparse_key="absent") == EMPTY3
    got = st.hybrid_query(Q[0], qs[0], k=5, sparse_key="absent")
    assert got[0] == list(st.query(Q[0], k=5, use_hnsw=False)[0]) and got[4] == [1] * 5
    # a query without terms, and None
    assert st.sparse_query({"indices": [], "values": []}) == EMPTY3 and st.sparse_query(None) == EMPTY3


def test_column_follows_upsert_and_reload(store_mod, tmp_path):
    V0, meta0, Q, qs = _data()
    V, meta = V0.copy(), [dict(m) for m in meta0]
    st = _mk(store_mod, tmp_path / "p", persist=True)
    st.add_vectors(V, meta)
    assert st.sparse_query(qs[0], k=10) == _want_sparse(store_mod, qs[0], meta, 10)
    # an upsert gives row 5 every term of the query with a large weight, and adds a row with none
    t = qs[0]["indices"]
    new_meta = [dict(meta[5], sparse={"indices": t, "values": [9.0] * len(t)}), {"id": "new", "lang": "de", "section": 0}]
    new_vecs = np.stack([V[5], -Q[0]]).astype(np.float32)
    assert st.upsert_vectors(new_vecs, new_meta, key="id")["updated"] == 1
    meta[5] = new_meta[0]
    meta.append(new_meta[1])
    V = np.concatenate([V, new_vecs[1:]])
    got = st.sparse_query(qs[0], k=10)
    assert got == _want_sparse(store_mod, qs[0], meta, 10) and got[0][0] == 5
    assert st.hybrid_query(Q[0], qs[0], k=10) == _want_hybrid(store_mod, Q[0], qs[0], V, meta, "cosine", 10, 40)
    # a metadata-only change of an existing row also rebuilds the column (an update bumps "rows_updated")
    new_meta = [dict(meta[7], sparse={"indices": [t[0]], "values": [100.0]})]
    st.upsert_vectors(V[7][None, :], new_meta, key="id")
    meta[7] = new_meta[0]
    got = st.sparse_query(qs[0], k=10, filter_metadata={"lang": meta[7]["lang"]})
    assert got == _want_sparse(store_mod, qs[0], meta, 10, {"lang": meta[7]["lang"]}) and 7 in got[0][:2]
    # a delete moves the rows: the column follows
    st.delete_rows([0])
    V, meta = V[1:], meta[1:]
    assert st.sparse_query(qs[1], k=10) == _want_sparse(store_mod, qs[1], meta, 10)
    # a second store over the same files: the sparse vectors came through the metadata file
    st._save_store(force=True)
    st2 = _mk(store_mod, tmp_path / "p", persist=True)
    assert st2._vector_count == N
    for b in range(3):
        assert st2.sparse_query(qs[b], k=10) == st.sparse_query(qs[b], k=10) == _want_sparse(store_mod, qs[b], meta, 10)
        assert st2.hybrid_query(Q[b], qs[b], k=10, filter_metadata={"lang": "en"}) == \
            _want_hybrid(store_mod, Q[b], qs[b], V, meta, "cosine", 10, 40, filt={"lang": "en"})


def test_no_device_call_when_nothing_can_match_and_bad_arguments(store_mod, tmp_path):
    V, meta, Q, qs = _data()
    st = _mk(store_mod, tmp_path / "s", persist=False)
    assert st.sparse_query(qs[0]) == EMPTY3 and st.batch_sparse_query(qs[:2]) == [EMPTY3, EMPTY3]  # empty store
    assert st.hybrid_query(Q[0], qs[0]) == EMPTY5 and st.batch_hybrid_query(Q[:2], qs[:2]) == [EMPTY5, EMPTY5]
    st.add_vectors(V, meta)
    assert st.sparse_query(qs[0], filter_metadata={"lang": "xx"}) == EMPTY3  # a filter nothing matches
    assert st.hybrid_query(Q[0], qs[0], filter_metadata={"lang": "xx"}) == EMPTY5
    assert st.batch_sparse_query([]) == [] and st.batch_hybrid_query(Q[:0], []) == []
    assert st._index.stat("sparse_searches") == 0 and st._index.stat("hybrid_searches") == 0 and st._index.stat("sparse_sets") == 0
    nan = float("nan")
    for bad, word in ((dict(k=0), "k must"), (dict(k=1025), "1024")):
        with pytest.raises(ValueError, match=word):
            st.sparse_query(qs[0], **bad)
    for bad_sv, word in (({"indices": [3, 3], "values": [1.0, 1.0]}, "repeated"),
                         ({"indices": list(range(1025)), "values": [1.0] * 1025}, "1024"), ({"indices": [1]}, "indices")):
        with pytest.raises(ValueError, match=word):
            st.sparse_query(bad_sv)
        with pytest.raises(ValueError, match=word):
            st.hybrid_query(Q[0], bad_sv)
    for bad, word in ((dict(k=0), "k must"), (dict(k=201), "200"), (dict(k=10, fetch_k=9), "fetch_k"), (dict(k=10, fetch_k=201), "200"),
                      (dict(rrf_c=-1.0), "rrf_c"), (dict(rrf_c=nan), "rrf_c"), (dict(weights=(1.0,)), "weights"),
                      (dict(weights=(1.0, nan)), "weights"), (dict(weights=(-1.0, 1.0)), "weights")):
        with pytest.raises(ValueError, match=word):
            st.hybrid_query(Q[0], qs[0], **bad)
    with pytest.raises(ValueError, match="Dimension mismatch"):
        st.hybrid_query(np.ones(D + 1, np.float32), qs[0])
    with pytest.raises(ValueError, match="batch_hybrid_query"):
        st.hybrid_query(np.ones((2, D), np.float32), qs[0])
    with pytest.raises(ValueError, match="sparse vectors"):
        st.batch_hybrid_query(Q[:2], qs[:1])
    assert st._index.stat("sparse_searches") == 0 and st._index.stat("hybrid_searches") == 0
    # a row whose stored sparse vector repeats an index is refused when the column is built
    st.upsert_vectors(V[3][None, :], [dict(meta[3], sparse={"indices": [4, 4], "values": [1.0, 1.0]})], key="id")
    with pytest.raises(ValueError, match="repeated"):
        st.sparse_query(qs[0])


def test_multi_device_store_refuses(store_mod, tmp_path):
    st = _mk(store_mod, tmp_path / "m", devices=[0, 0], persist=False)
    V, meta, Q, qs = _data()
    st.add_vectors(V[:100], meta[:100])
    for call, word in ((lambda: st.sparse_query(qs[0]), "sparse"), (lambda: st.batch_sparse_query(qs[:2]), "sparse"),
                       (lambda: st.hybrid_query(Q[0], qs[0]), "hybrid"), (lambda: st.batch_hybrid_query(Q[:2], qs[:2]), "hybrid")):
        with pytest.raises(NotImplementedError, match=f"{word} query is not supported on a multi-device store"):
            call()

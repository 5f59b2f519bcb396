"""MMR reads through the store (service/optimized_vector_store.py ``mmr_query`` /
``batch_mmr_query``), on the GPU: the rows, their order and their scores are exactly the oracle's
(tests/_mmr_cases.py ``expected`` with the filter as the mask), with each row's metadata."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mmr_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu
N, D = 600, 48
METRICS = mc.METRICS


@pytest.fixture(scope="module")
def store_mod():
    from service import _vdb, optimized_vector_store
    assert _vdb.device_count() >= 1, "no GPU visible"
    return optimized_vector_store


def _mk(store_mod, path, metric="cosine", **kw):
    return store_mod.MLXVectorStore(str(path), store_mod.MLXVectorStoreConfig(dimension=D, metric=metric, **kw))


def _data():
    V, Q = mc.corpus(N, D, seed=4)
    V = V.copy()
    rng = np.random.default_rng(2)
    # eight near-copies of query 0, as overlapping chunks of one paragraph would be
    V[rng.choice(N, size=8, replace=False)] = Q[0] + 0.01 * rng.standard_normal((8, D)).astype(np.float32)
    meta = [{"id": i, "lang": "en" if i % 3 else "de", "section": int(rng.integers(0, 4))} for i in range(N)]
    return V, meta, Q


def _want(q, V, meta, metric, k, fetch_k, lam, filt=None):
    """The contract for one query: (indices, scores, metadata)."""
    mask = None if not filt else np.array([all(m.get(a) == b for a, b in filt.items()) for m in meta])
    s, i, _, _ = mc.expected(q[None], V, k, fetch_k, lam, metric, mask)
    rows = i[0][i[0] >= 0].tolist()
    return rows, s[0][:len(rows)].astype(np.float64).tolist(), [meta[r] for r in rows]


@pytest.mark.parametrize("metric", METRICS)
def test_mmr_reads_match_the_oracle(store_mod, tmp_path, metric):
    V, meta, Q = _data()
    st = _mk(store_mod, tmp_path / "s", metric, persist=False)
    st.add_vectors(V, meta)
    for filt in (None, {"lang": "de"}, {"lang": "de", "section": 1}):
        for k, fetch, lam in ((1, 1, 0.5), (5, 20, 0.5), (10, 64, 0.0), (10, 64, 1.0), (200, 200, 0.25)):
            batch = st.batch_mmr_query(Q[:3], k=k, fetch_k=fetch, lambda_mult=lam, filter_metadata=filt)
            assert len(batch) == 3
            for b in range(3):
                assert batch[b] == _want(Q[b], V, meta, metric, k, fetch, lam, filt), (b, filt, k, fetch, lam)
            assert st.mmr_query(Q[1], k=k, fetch_k=fetch, lambda_mult=lam, filter_metadata=filt) == batch[1]
    # the default fetch_k is min(200, max(4 k, 20)) and the default lambda_mult 0.5
    for k, fetch in ((1, 20), (5, 20), (10, 40), (60, 200)):
        assert st.mmr_query(Q[0], k=k) == _want(Q[0], V, meta, metric, k, fetch, 0.5), k
    assert st.mmr_query(Q[0][None, :]) == _want(Q[0], V, meta, metric, 10, 40, 0.5)
    # lambda_mult = 1 is the plain query
    rows, scores, metas = st.mmr_query(Q[2], k=7, lambda_mult=1.0)
    plain = st.query(Q[2], k=7, use_hnsw=False)
    assert rows == list(plain[0]) and metas == list(plain[2])
    assert st._index.stat("mmr_searches") > 0


def test_mmr_drops_the_near_copies(store_mod, tmp_path):
    V, meta, Q = _data()
    st = _mk(store_mod, tmp_path / "s", "cosine", persist=False)
    st.add_vectors(V, meta)
    copies = set(np.nonzero(np.abs(V - Q[0]).max(axis=1) < 0.1)[0].tolist())
    assert len(copies) == 8
    plain = st.query(Q[0], k=8, use_hnsw=False)[0]
    assert set(plain) == copies
    rows = st.mmr_query(Q[0], k=8, fetch_k=64, lambda_mult=0.5)[0]
    assert rows[0] == plain[0] and len(copies & set(rows)) < 8


def test_no_device_call_when_nothing_can_match(store_mod, tmp_path):
    V, meta, Q = _data()
    st = _mk(store_mod, tmp_path / "s", persist=False)
    assert st.mmr_query(Q[0]) == ([], [], []) and st.batch_mmr_query(Q[:2]) == [([], [], []), ([], [], [])]  # empty
    st.add_vectors(V, meta)
    assert st.mmr_query(Q[0], filter_metadata={"lang": "xx"}) == ([], [], [])  # a filter nothing matches
    assert st.batch_mmr_query(Q[:0]) == []
    assert st._index.stat("mmr_searches") == 0
    for bad, word in ((dict(k=0), "k must"), (dict(k=201), "200"), (dict(k=10, fetch_k=9), "fetch_k"),
                      (dict(k=10, fetch_k=201), "200"), (dict(lambda_mult=-0.1), "lambda_mult"),
                      (dict(lambda_mult=1.1), "lambda_mult"), (dict(lambda_mult=float("nan")), "lambda_mult")):
        with pytest.raises(ValueError, match=word):
            st.mmr_query(Q[0], **bad)
    with pytest.raises(ValueError, match="Dimension mismatch"):
        st.mmr_query(np.ones(D + 1, np.float32))
    with pytest.raises(ValueError, match="batch_mmr_query"):
        st.mmr_query(Q[:2])
    assert st._index.stat("mmr_searches") == 0


def test_multi_device_store_refuses(store_mod, tmp_path):
    st = _mk(store_mod, tmp_path / "m", devices=[0, 0], persist=False)
    V, meta, Q = _data()
    st.add_vectors(V[:100], meta[:100])
    for call in (lambda: st.mmr_query(Q[0]), lambda: st.batch_mmr_query(Q[:2])):
        with pytest.raises(NotImplementedError, match="MMR query is not supported on a multi-device store"):
            call()


def test_graph_store_never_takes_the_graph(store_mod, tmp_path):
    V, meta, Q = _data()
    st = _mk(store_mod, tmp_path / "h", enable_hnsw=True, persist=False)
    st.add_vectors(V, meta)
    assert st._hnsw_index.is_loaded
    before = st._hnsw_index.index.stat("queries")
    for b in range(2):
        assert st.mmr_query(Q[b], k=5) == _want(Q[b], V, meta, "cosine", 5, 20, 0.5)
    assert st._hnsw_index.index.stat("queries") == before

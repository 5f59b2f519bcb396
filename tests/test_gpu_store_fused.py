"""Fused reads through the store (service/optimized_vector_store.py ``fused_query`` /
``batch_fused_query``), on the GPU: the rows, their order, scores, fused values and hit counts are
exactly the oracle's (tests/_fused_cases.py ``expected`` with the filter as the mask), with each row's
metadata."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fused_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
N, D = 600, 48
METRICS = fc.METRICS
EMPTY = ([], [], [], [], [])


@pytest.fixture(scope="module")
def store_mod():
    from service import _vdb, optimized_vector_store
    assert _vdb.device_count() >= 1, "no GPU visible"
    return optimized_vector_store


def _mk(store_mod, path, metric="cosine", **kw):
    return store_mod.MLXVectorStore(str(path), store_mod.MLXVectorStoreConfig(dimension=D, metric=metric, **kw))


def _data():
    V, _ = fc.corpus(N, D, seed=4)
    rng = np.random.default_rng(2)
    base = rng.standard_normal((3, D)).astype(np.float32)
    # three questions, each with four paraphrases
    sets = [(base[j] + 0.4 * rng.standard_normal((4, D))).astype(np.float32) for j in range(3)]
    meta = [{"id": i, "lang": "en" if i % 3 else "de", "section": int(rng.integers(0, 4))} for i in range(N)]
    return V, meta, sets


def _want(Qs, V, meta, metric, k, fetch_k, fusion, weights=None, rrf_c=60.0, filt=None):
    """The contract for one set: (indices, scores, metadata, fused, hits)."""
    mask = None if not filt else np.array([all(m.get(a) == b for a, b in filt.items()) for m in meta])
    Qs = np.asarray(Qs, np.float32).reshape(-1, D)
    s, i, f, h = fc.expected(Qs, fc.offsets_of([Qs.shape[0]]), V, k, fetch_k, fusion, metric, weights, rrf_c, mask)
    rows = i[0][i[0] >= 0].tolist()
    n = len(rows)
    return (rows, s[0][:n].astype(np.float64).tolist(), [meta[r] for r in rows], f[0][:n].tolist(), h[0][:n].tolist())


@pytest.mark.parametrize("metric", METRICS)
def test_fused_reads_match_the_oracle(store_mod, tmp_path, metric):
    V, meta, sets = _data()
    st = _mk(store_mod, tmp_path / "s", metric, persist=False)
    st.add_vectors(V, meta)
    for filt in (None, {"lang": "de"}, {"lang": "de", "section": 1}):
        for fusion in fc.FUSIONS:
            for k, fetch in ((1, 1), (5, 20), (10, 64), (200, 200)):
                batch = st.batch_fused_query(sets, k=k, fusion=fusion, fetch_k=fetch, filter_metadata=filt)
                assert len(batch) == 3
                for b in range(3):
                    assert batch[b] == _want(sets[b], V, meta, metric, k, fetch, fusion, filt=filt), (b, filt, k, fetch)
                assert st.fused_query(sets[1], k=k, fusion=fusion, fetch_k=fetch, filter_metadata=filt) == batch[1]
    # weights and rrf_c travel; one vector is a set of one; sets of different sizes and an empty one
    w = [0.0, 0.5, 3.0, 1.0]
    assert st.fused_query(sets[0], k=10, weights=w, rrf_c=10.0) == _want(sets[0], V, meta, metric, 10, 40, "rrf", w, 10.0)
    got = st.batch_fused_query([sets[0], sets[1][:2]], k=5, weights=[w, [2.0, 1.0]])
    assert got[0] == _want(sets[0], V, meta, metric, 5, 20, "rrf", w)
    assert got[1] == _want(sets[1][:2], V, meta, metric, 5, 20, "rrf", [2.0, 1.0])
    assert st.fused_query(sets[2][0], k=5, fusion="max") == _want(sets[2][:1], V, meta, metric, 5, 20, "max")
    got = st.batch_fused_query([sets[0], [], sets[2][:1]], k=5)
    assert got[1] == EMPTY and got[0] == _want(sets[0], V, meta, metric, 5, 20, "rrf")
    # the default fetch_k is min(200, max(k, 4 k)) and the default fusion rrf with rrf_c 60
    for k, fetch in ((1, 4), (5, 20), (10, 40), (60, 200), (200, 200)):
        assert st.fused_query(sets[0], k=k) == _want(sets[0], V, meta, metric, k, fetch, "rrf"), k
    # one vector under max with fetch_k == k is the plain query
    rows, scores, metas, fused, hits = st.fused_query(sets[2][0], k=7, fusion="max", fetch_k=7)
    plain = st.query(sets[2][0], k=7, use_hnsw=False)
    assert rows == list(plain[0]) and metas == list(plain[2]) and hits == [1] * 7
    assert st._index.stat("fused_searches") > 0


def test_no_device_call_when_nothing_can_match_and_bad_arguments(store_mod, tmp_path):
    V, meta, sets = _data()
    st = _mk(store_mod, tmp_path / "s", persist=False)
    assert st.fused_query(sets[0]) == EMPTY and st.batch_fused_query(sets[:2]) == [EMPTY, EMPTY]  # empty store
    st.add_vectors(V, meta)
    assert st.fused_query(sets[0], filter_metadata={"lang": "xx"}) == EMPTY  # a filter nothing matches
    assert st.batch_fused_query([]) == []
    assert st._index.stat("fused_searches") == 0
    nan = float("nan")
    for bad, word in ((dict(k=0), "k must"), (dict(k=201), "200"), (dict(k=10, fetch_k=9), "fetch_k"),
                      (dict(k=10, fetch_k=201), "200"), (dict(fusion="sum"), "fusion"), (dict(rrf_c=-1.0), "rrf_c"),
                      (dict(rrf_c=nan), "rrf_c"), (dict(rrf_c=float("inf")), "rrf_c"),
                      (dict(weights=[1, 1, 1]), "weights"), (dict(weights=[1, 1, nan, 1]), "weights"),
                      (dict(weights=[1, -1, 1, 1]), "weights"), (dict(fusion="max", weights=[1, 1, 1, 1]), "weights")):
        with pytest.raises(ValueError, match=word):
            st.fused_query(sets[0], **bad)
    with pytest.raises(ValueError, match="Dimension mismatch"):
        st.fused_query(np.ones((2, D + 1), np.float32))
    with pytest.raises(ValueError, match="16"):
        st.fused_query(np.ones((17, D), np.float32))
    with pytest.raises(ValueError, match="batch_fused_query"):
        st.fused_query(np.ones((2, 2, D), np.float32))
    with pytest.raises(ValueError, match="weights"):
        st.batch_fused_query(sets[:2], weights=[[1, 1, 1, 1]])
    assert st._index.stat("fused_searches") == 0
    assert len(st.fused_query(np.ones((16, D), np.float32))[0]) == 10  # 16 vectors are a set


def test_multi_device_store_refuses(store_mod, tmp_path):
    st = _mk(store_mod, tmp_path / "m", devices=[0, 0], persist=False)
    V, meta, sets = _data()
    st.add_vectors(V[:100], meta[:100])
    for call in (lambda: st.fused_query(sets[0]), lambda: st.batch_fused_query(sets[:2])):
        with pytest.raises(NotImplementedError, match="fused query is not supported on a multi-device store"):
            call()

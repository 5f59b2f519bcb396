"""MaxSim reads through the store (service/optimized_vector_store.py ``maxsim_query`` /
``batch_maxsim_query``), on the GPU: the groups, their order, scores and sums are exactly the oracle's
(tests/_maxsim_cases.py ``expected`` over the column the store builds from the metadata key, with the
filter as the mask)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _maxsim_cases as mc  # noqa: E402

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
    V, _ = mc.corpus(N, D, seed=4)
    rng = np.random.default_rng(2)
    # documents of 1 .. 12 consecutive chunks; every eleventh row has no document
    doc = np.repeat(np.arange(N), rng.integers(1, 13, size=N))[:N]
    meta = [{"id": i, "lang": "en" if i % 3 else "de"} for i in range(N)]
    for i in range(N):
        if i % 11:
            meta[i]["doc"] = f"doc_{int(doc[i])}"
    # three questions of 4, 9 and 1 token vectors
    sets = [rng.standard_normal((m, D)).astype(np.float32) for m in (4, 9, 1)]
    return V, meta, sets


def _want(Qs, V, meta, key, metric, k, filt=None):
    """The contract for one set: [{"group", "score", "sum"}], group id = order of first appearance."""
    values, col = [], np.full(len(meta), -1, np.int32)
    for i, m in enumerate(meta):
        if key in m:
            if m[key] not in values:
                values.append(m[key])
            col[i] = values.index(m[key])
    if not values:
        return []
    mask = None if not filt else np.array([all(m.get(a) == b for a, b in filt.items()) for m in meta])
    Qs = np.asarray(Qs, np.float32).reshape(-1, D)
    sc, gr, sm = mc.expected(Qs, mc.offsets_of([Qs.shape[0]]), V, col, len(values), k, metric, mask)
    n = int((gr[0] >= 0).sum())
    return [{"group": values[g], "score": float(s), "sum": float(u)} for g, s, u in zip(gr[0][:n], sc[0][:n], sm[0][:n])]


@pytest.mark.parametrize("metric", METRICS)
def test_maxsim_reads_match_the_oracle(store_mod, tmp_path, metric):
    V, meta, sets = _data()
    st = _mk(store_mod, tmp_path / "s", metric, persist=False)
    st.add_vectors(V, meta)
    for filt in (None, {"lang": "de"}):
        for k in (1, 10, 128):
            batch = st.batch_maxsim_query(sets, "doc", k=k, filter_metadata=filt)
            assert len(batch) == 3
            for b in range(3):
                assert batch[b] == _want(sets[b], V, meta, "doc", metric, k, filt), (b, filt, k)
            assert st.maxsim_query(sets[1], "doc", k=k, filter_metadata=filt) == batch[1]
    got = st.maxsim_query(sets[0], "doc")
    assert len(got) == 10 and [g["sum"] for g in got] == sorted((g["sum"] for g in got), reverse=True)
    assert all(set(g) == {"group", "score", "sum"} and g["score"] == float(np.float32(g["sum"])) for g in got)
    # one vector is a set of one; an empty set among others has no result; another key, another column
    assert st.maxsim_query(sets[2][0], "doc", k=5) == _want(sets[2], V, meta, "doc", metric, 5)
    got = st.batch_maxsim_query([sets[0], [], sets[2]], "doc", k=5)
    assert got[1] == [] and got[0] == _want(sets[0], V, meta, "doc", metric, 5) and got[2] == _want(sets[2], V, meta, "doc", metric, 5)
    assert st.maxsim_query(sets[0], "lang", k=5) == _want(sets[0], V, meta, "lang", metric, 5)
    assert st.maxsim_query(sets[0], "doc", k=5) == _want(sets[0], V, meta, "doc", metric, 5)
    # a one-vector set ranks the groups as query_groups does
    one = st.maxsim_query(sets[2], "doc", k=8)
    assert [g["group"] for g in one] == [g["group"] for g in st.query_groups(sets[2][0], "doc", k=8)]
    assert st._index.stat("maxsim_searches") > 0 and st._index.stat("maxsim_skipped_rows") == 0


def test_no_device_call_when_nothing_can_match_and_bad_arguments(store_mod, tmp_path):
    V, meta, sets = _data()
    st = _mk(store_mod, tmp_path / "s", persist=False)
    assert st.maxsim_query(sets[0], "doc") == [] and st.batch_maxsim_query(sets[:2], "doc") == [[], []]  # empty store
    st.add_vectors(V, meta)
    assert st.maxsim_query(sets[0], "doc", filter_metadata={"lang": "xx"}) == []  # a filter nothing matches
    assert st.maxsim_query(sets[0], "no_such_key") == []  # a key no row has
    assert st.batch_maxsim_query([], "doc") == []
    assert st._index.stat("maxsim_searches") == 0
    for bad in (0, -1, 129):
        with pytest.raises(ValueError, match="k must"):
            st.maxsim_query(sets[0], "doc", k=bad)
    with pytest.raises(ValueError, match="at most 64"):
        st.maxsim_query(np.ones((65, D), np.float32), "doc")
    with pytest.raises(ValueError, match="Dimension mismatch"):
        st.maxsim_query(np.ones((2, D + 1), np.float32), "doc")
    with pytest.raises(ValueError):
        st.maxsim_query(np.ones((2, 2, D), np.float32), "doc")
    assert st._index.stat("maxsim_searches") == 0
    assert len(st.maxsim_query(np.ones((64, D), np.float32), "doc", k=128)) == min(128, len({m["doc"] for m in meta if "doc" in m}))
    assert st._index.stat("maxsim_searches") == 1 and st._index.stat("searches") == 0


def test_multi_device_store_refuses(store_mod, tmp_path, monkeypatch):
    V, meta, sets = _data()
    st = _mk(store_mod, tmp_path / "s", persist=False)
    st.add_vectors(V, meta)
    monkeypatch.setattr(st, "_devices", lambda: [0, 1])
    with pytest.raises(NotImplementedError, match="multi-device"):
        st.maxsim_query(sets[0], "doc")

"""Grouped reads through the store (service/optimized_vector_store.py ``query_groups`` /
``batch_query_groups``), on the GPU: the groups are exactly the oracle's -- the eligible rows ordered
by (``ref_cpu.exact_keys`` desc, row asc), each ``group_by`` value's first occurrence kept, the first
k taken -- and with ``group_size`` > 1 each group lists its own best rows, the first of them the row
the grouped search returned."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _group_cases as gc  # noqa: E402
from oracle import ref_cpu  # noqa: E402

pytestmark = pytest.mark.gpu
N, D = 1800, 48
METRICS = gc.METRICS


@pytest.fixture(scope="module")
def store_mod():
    from service import _vdb, optimized_vector_store
    assert _vdb.device_count() >= 1, "no GPU visible"
    return optimized_vector_store


def _mk(store_mod, path, metric="cosine", **kw):
    return store_mod.MLXVectorStore(str(path), store_mod.MLXVectorStoreConfig(dimension=D, metric=metric, **kw))


def _data():
    V, Q = gc.corpus(N, D, seed=4)
    V = V.copy()
    V[[40, 901]] = V[7]  # equal keys for every query: row 40 has no document, 7 and 901 different ones
    rng = np.random.default_rng(2)
    meta = []
    for i in range(N):
        m = {"id": i, "lang": "en" if i % 3 else "de", "section": int(rng.integers(0, 4))}
        if i % 10:  # every tenth row has no document
            m["doc"] = f"doc_{int(rng.integers(0, 60))}"
        meta.append(m)
    return V, meta, Q


def _want(keys_row, metric, meta, group_by, k, group_size=1, filt=None):
    """The contract for one query: [{"group": value, "hits": (indices, scores, metadata)}]."""
    ok = np.array([group_by in m and (not filt or all(m.get(a) == b for a, b in filt.items())) for m in meta])
    rows = np.nonzero(ok)[0]
    rows = rows[np.lexsort((rows, -keys_row[rows]))]
    by_group = {}
    for r in rows.tolist():
        by_group.setdefault(meta[r][group_by], []).append(r)  # (insertion order = the groups' ranking)
    out = []
    for value, rs in list(by_group.items())[:k]:
        rs = rs[:group_size]
        out.append({"group": value,
                    "hits": (rs, ref_cpu.keys_to_scores(keys_row[rs], metric).astype(np.float64).tolist(),
                             [meta[r] for r in rs])})
    return out


@pytest.mark.parametrize("metric", METRICS)
def test_grouped_reads_match_the_oracle(store_mod, tmp_path, metric):
    V, meta, Q = _data()
    st = _mk(store_mod, tmp_path / "s", metric, persist=False)
    st.add_vectors(V, meta)
    keys = gc.oracle_keys(Q[:4], V, metric)
    for filt in (None, {"lang": "de"}, {"lang": "de", "section": 1}):
        for k, gs in ((1, 1), (5, 1), (5, 3), (128, 1), (7, 100)):
            batch = st.batch_query_groups(Q[:4], "doc", k=k, group_size=gs, filter_metadata=filt)
            assert len(batch) == 4
            for b in range(4):
                want = _want(keys[b], metric, meta, "doc", k, gs, filt)
                assert batch[b] == want, (b, filt, k, gs)
            assert st.query_groups(Q[1], "doc", k=k, group_size=gs, filter_metadata=filt) == batch[1]
    # group_size > 1: each group's first hit is the row the grouped search returned, bit for bit
    one = st.query_groups(Q[0], "doc", k=9)
    three = st.query_groups(Q[0], "doc", k=9, group_size=3)
    assert [g["group"] for g in one] == [g["group"] for g in three]
    for a, b in zip(one, three):
        assert a["hits"][0][0] == b["hits"][0][0] and a["hits"][1][0] == b["hits"][1][0]
        assert all(m["doc"] == a["group"] for m in b["hits"][2])
    # rows lacking the key are in no group, although they rank
    got = st.query_groups(V[10], "doc", k=3)
    assert "doc" not in meta[10] and all(10 not in g["hits"][0] for g in got)
    assert st.query(V[10], k=1, use_hnsw=False)[0] == [10]
    # equal keys: the lower row's document first
    k7 = gc.oracle_keys(V[7:8], V, metric)[0]
    assert k7[7] == k7[40] == k7[901] and "doc" not in meta[40] and meta[7]["doc"] != meta[901]["doc"]
    got = st.query_groups(V[7], "doc", k=3)
    assert got == _want(k7, metric, meta, "doc", 3) and [g["hits"][0][0] for g in got][:2] == [7, 901]
    assert st._index.stat("group_searches") > 0 and st._index.stat("subset_searches") > 0


def test_no_device_call_when_nothing_can_match(store_mod, tmp_path):
    V, meta, Q = _data()
    st = _mk(store_mod, tmp_path / "s", persist=False)
    assert st.query_groups(Q[0], "doc") == [] and st.batch_query_groups(Q[:2], "doc") == [[], []]  # empty store
    st.add_vectors(V, meta)
    assert st.query_groups(Q[0], "doc", filter_metadata={"lang": "xx"}) == []  # a filter nothing matches
    assert st.query_groups(Q[0], "no_such_key") == []  # a key no row has
    assert st._index.stat("group_searches") == 0 and st._index.stat("group_sets") == 0
    for bad in (dict(k=0), dict(k=129), dict(group_size=0), dict(group_size=101)):
        with pytest.raises(ValueError):
            st.query_groups(Q[0], "doc", **bad)
    with pytest.raises(ValueError, match="Dimension mismatch"):
        st.query_groups(np.ones(D + 1, np.float32), "doc")


def test_column_follows_mutations_and_keys(store_mod, tmp_path):
    V, meta, Q = _data()
    st = _mk(store_mod, tmp_path / "s", persist=False)
    st.add_vectors(V[:1000], meta[:1000])
    cur_v, cur_m = V[:1000].copy(), list(meta[:1000])

    def check(what):
        keys = gc.oracle_keys(Q[:2], cur_v, "cosine")
        for key in ("doc", "section", "doc"):  # alternating two keys
            for b in range(2):
                assert st.query_groups(Q[b], key, k=6) == _want(keys[b], "cosine", cur_m, key, 6), (what, key, b)

    check("first")
    sets = st._index.stat("group_sets")
    st.query_groups(Q[0], "doc", k=2)
    st.query_groups(Q[1], "doc", k=3, filter_metadata={"lang": "en"})
    assert st._index.stat("group_sets") == sets  # the same key again: the attached column serves
    assert st._index.stat("group_rows") == 1000
    assert st.query_groups(Q[0], "no_such_key") == [] and st._index.stat("group_rows") == 0  # nothing stays attached
    check("after a key no row has")
    st.add_vectors(V[1000:], meta[1000:])
    cur_v, cur_m = V.copy(), list(meta)
    check("after add")
    st.delete_vectors({"section": 2})
    keep = [i for i, m in enumerate(cur_m) if m["section"] != 2]
    cur_v, cur_m = cur_v[keep], [cur_m[i] for i in keep]
    check("after delete")
    # an upsert that moves a row to another document and to the top of query 0
    target = cur_m[5]["id"]
    new_meta = dict(cur_m[5], doc="doc_moved")
    st.upsert_vectors(Q[0][None, :] * 2.0, [new_meta], key="id")
    cur_v[5], cur_m[5] = Q[0] * 2.0, new_meta
    assert cur_m[5]["id"] == target
    check("after upsert")
    assert st.query_groups(Q[0], "doc", k=1)[0]["group"] == "doc_moved"


def test_multi_device_store_refuses(store_mod, tmp_path):
    st = _mk(store_mod, tmp_path / "m", devices=[0, 0], persist=False)
    V, meta, Q = _data()
    st.add_vectors(V[:100], meta[:100])
    for call in (lambda: st.query_groups(Q[0], "doc"), lambda: st.batch_query_groups(Q[:2], "doc")):
        with pytest.raises(NotImplementedError, match="grouped query is not supported on a multi-device store"):
            call()


def test_graph_store_never_takes_the_graph(store_mod, tmp_path):
    V, meta, Q = _data()
    st = _mk(store_mod, tmp_path / "h", enable_hnsw=True, persist=False)
    st.add_vectors(V, meta)
    assert st._hnsw_index.is_loaded
    before = st._hnsw_index.index.stat("queries")
    keys = gc.oracle_keys(Q[:2], V, "cosine")
    for b in range(2):
        assert st.query_groups(Q[b], "doc", k=5, group_size=2) == _want(keys[b], "cosine", meta, "doc", 5, 2)
    assert st._hnsw_index.index.stat("queries") == before

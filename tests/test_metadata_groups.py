"""MetadataIndex.group_column (mlx-vector-db_amd/service/metadata_index.py): the int32 group column
of a metadata key, built from the postings, across extend / remove / replace.  CPU only; the
expectation is a plain scan of the dicts."""
import numpy as np

from service.metadata_index import MetadataIndex


def _scan(rows, key, n):
    """The contract by a scan: ids 0..G-1 in order of each value's first row, -1 without the key or
    with an unhashable / NaN value."""
    col = np.full(n, -1, np.int32)
    values = []
    for r, m in enumerate(rows[:n]):
        if not isinstance(m, dict) or key not in m:
            continue
        v = m[key]
        try:
            hash(v)
        except TypeError:
            continue
        if isinstance(v, float) and v != v:
            continue
        if v not in values:
            values.append(v)
        col[r] = values.index(v)
    return col, values


def _check(ix, rows, key, n=None):
    n = len(rows) if n is None else n
    col, values = ix.group_column(key, n)
    want_col, want_values = _scan(rows, key, n)
    assert col.dtype == np.int32 and col.shape == (n,)
    np.testing.assert_array_equal(col, want_col)
    assert values == want_values


def _rows(n, seed=0):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        m = {"id": i}
        if i % 7:
            m["doc"] = f"d{int(rng.integers(0, 9))}"
        if i % 5 == 0:
            m["tag"] = [1, 2]  # unhashable: skipped by the postings
        if i % 11 == 0:
            m["score"] = float("nan")
        elif i % 3 == 0:
            m["score"] = int(rng.integers(0, 3))
        rows.append(m)
    return rows


def test_group_column_across_mutations():
    rows = _rows(300)
    ix = MetadataIndex()
    ix.extend(rows[:120])
    for key in ("doc", "id", "tag", "score", "missing"):
        _check(ix, rows[:120], key)
    _check(ix, rows[:120], "doc", n=50)  # fewer rows than indexed: ids still from the first rows < n
    ix.extend(rows[120:])
    for key in ("doc", "score", "tag"):
        _check(ix, rows, key)
    gone = [0, 1, 2, 50, 51, 299, 130]  # among them the first rows of several values
    ix.remove(gone)
    cur = [m for i, m in enumerate(rows) if i not in set(gone)]
    for key in ("doc", "score", "id"):
        _check(ix, cur, key)
    ids = [3, 4, 100]
    new = [{"id": "a", "doc": "brand_new"}, {"id": "b"}, {"id": "c", "doc": cur[0].get("doc", "d0"), "score": 1}]
    ix.replace(ids, new)
    for r, m in zip(ids, new):
        cur[r] = m
    for key in ("doc", "score", "id"):
        _check(ix, cur, key)
    col, values = ix.group_column("doc", len(cur))
    assert "brand_new" in values and col[3] == values.index("brand_new") and col[4] == -1


def test_group_column_edges():
    ix = MetadataIndex()
    col, values = ix.group_column("doc", 0)
    assert col.shape == (0,) and values == []
    ix.extend([{"doc": None}, {}, {"doc": 1}, {"doc": True}, {"doc": 1.0}, "not a dict", {"doc": "x"}])
    col, values = ix.group_column("doc", 7)
    np.testing.assert_array_equal(col, [0, -1, 1, 1, 1, -1, 2])  # None is a value; 1 == True == 1.0
    assert values == [None, 1, "x"]
    col, values = ix.group_column(["unhashable"], 7)
    assert (col == -1).all() and values == []
    ix.clear()
    assert ix.group_column("doc", 0)[1] == []

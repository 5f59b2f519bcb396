"""MetadataIndex.rows_with and MetadataIndex.replace (service/metadata_index.py) against a
brute-force recomputation over random metadata: after rows take new dicts, every filter's bitmap
equals that of a fresh index built from the resulting metadata list and the reference's scan over
it; no row is renumbered.  CPU only."""
import numpy as np
import pytest

from service.metadata_index import MetadataIndex

N = 203

FILTERS = [
    {"doc": "a"}, {"doc": "b", "n": 3}, {"doc": "zzz"}, {"n": 1}, {"n": 1.0}, {"n": True},
    {"tag": None}, {"tag": "x"}, {"tag": None, "doc": "c"}, {"missing": None}, {"missing": 1},
    {"list": [0, "v"]}, {"list": [1, "v"], "doc": "a"}, {"list": None}, {"f": 1}, {"f": None}, {"id": 7}, {},
]


def _random_metadata(rng, n, id0=0):
    out = []
    for i in range(n):
        m = {"id": id0 + i, "doc": "abc"[int(rng.integers(3))], "n": int(rng.integers(5))}
        t = int(rng.integers(4))
        if t == 0:
            m["tag"] = None           # an explicit None
        elif t == 1:
            m["tag"] = "x"            # (otherwise the row lacks the key)
        if rng.random() < 0.15:
            m["list"] = [int(rng.integers(2)), "v"]  # an unhashable value
        if rng.random() < 0.1:
            m["f"] = 1.0              # hashes like 1 and True
        if rng.random() < 0.05:
            m["nan"] = float("nan")   # never equal to anything
        out.append(m)
    return out


def _fresh(meta):
    ix = MetadataIndex()
    ix.extend(meta)
    return ix


def _assert_same_as_fresh(ix, meta):
    fresh = _fresh(meta)
    assert len(ix) == len(meta) == len(fresh)
    for f in FILTERS:
        for n in {len(meta), max(len(meta) - 3, 0)}:
            got, want = ix.bitmap(f, n), fresh.bitmap(f, n)
            np.testing.assert_array_equal(got[0], want[0], err_msg=f"{f} n={n}")
            assert got[1] == want[1], (f, n)
            scan = [i for i, m in enumerate(meta[:n]) if all(m.get(a) == b for a, b in f.items())]
            bits = np.unpackbits(got[0].view(np.uint8), bitorder="little")
            assert np.nonzero(bits)[0].tolist() == scan, (f, n)
    _assert_rows_with(ix, meta)


def _assert_rows_with(ix, meta):
    """rows_with(key, value) = the rows that HOLD the key with an equal hashable value."""
    pairs = [("doc", "a"), ("doc", "zzz"), ("n", 1), ("n", 1.0), ("n", True), ("tag", None), ("tag", "x"),
             ("missing", None), ("missing", 1), ("list", [0, "v"]), ("f", 1), ("id", 7), ("id", N + 3),
             ("nan", float("nan")), (["unhashable"], 1)]
    for key, value in pairs:
        try:
            hash((key, value))
            want = [i for i, m in enumerate(meta) if key in m and m[key] == value]
        except TypeError:
            want = []
        got = ix.rows_with(key, value)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64
        assert got.tolist() == want, (key, value)


ROW_SETS = {
    "first": [0],
    "last": [N - 1],
    "every_third": list(range(0, N, 3)),
    "block": list(range(40, 110)),
    "unsorted": [17, 5, 200, 64, 3],
    "random": np.random.default_rng(3).permutation(N)[:77].tolist(),
    "all": list(range(N)),
    "none": [],
}


def test_rows_with_on_a_fresh_index():
    meta = _random_metadata(np.random.default_rng(1), N)
    ix = _fresh(meta)
    _assert_rows_with(ix, meta)
    assert not ix._cache  # no bitmap was built


@pytest.mark.parametrize("name", sorted(ROW_SETS))
def test_replace_equals_a_fresh_index_of_the_result(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    meta = _random_metadata(rng, N)
    rows = ROW_SETS[name]
    new = _random_metadata(rng, len(rows), id0=1000)
    ix = _fresh(meta)
    ix.replace(rows, new)
    want = list(meta)
    for r, m in zip(rows, new):
        want[r] = m
    _assert_same_as_fresh(ix, want)


def test_replace_with_the_same_or_empty_dicts():
    meta = _random_metadata(np.random.default_rng(4), N)
    ix = _fresh(meta)
    ix.replace([3, 9], [meta[3], dict(meta[9])])  # unchanged pairs keep their postings
    _assert_same_as_fresh(ix, meta)
    ix.replace([3, 9, 11], [{}, {"only": 1}, {"list": [9]}])
    want = list(meta)
    want[3], want[9], want[11] = {}, {"only": 1}, {"list": [9]}
    _assert_same_as_fresh(ix, want)
    assert ix.rows_with("only", 1).tolist() == [9]
    ix.replace([9], [meta[9]])  # the last row of a posting leaves: the pair is gone
    want[9] = meta[9]
    assert ix.rows_with("only", 1).size == 0 and "only" not in ix._post
    _assert_same_as_fresh(ix, want)


def test_stale_cache_entry_is_dropped():
    meta = _random_metadata(np.random.default_rng(5), N)
    ix = _fresh(meta)
    before = ix.bitmap({"doc": "a"}, N)
    assert ix.bitmap({"doc": "a"}, N) is before  # cached
    rows = [i for i, m in enumerate(meta) if m["doc"] == "a"][:4]
    ix.replace(rows, [dict(meta[r], doc="b") for r in rows])
    after = ix.bitmap({"doc": "a"}, N)
    assert after[1] == before[1] - 4 and not np.array_equal(after[0], before[0])


def test_replace_composes_with_extend_and_remove():
    rng = np.random.default_rng(6)
    meta = _random_metadata(rng, N)
    ix = _fresh(meta)
    ix.replace([0, 100], _random_metadata(rng, 2, id0=500))
    want = list(meta)
    want[0], want[100] = ix._rows[0], ix._rows[100]
    ix.remove([5, 100])
    want = [m for i, m in enumerate(want) if i not in (5, 100)]
    extra = _random_metadata(rng, 7, id0=700)
    ix.extend(extra)
    want += extra
    new = _random_metadata(rng, 3, id0=900)
    ix.replace([len(want) - 1, 4, 99], new)
    for r, m in zip([len(want) - 1, 4, 99], new):
        want[r] = m
    _assert_same_as_fresh(ix, want)


def test_bad_arguments_raise_and_change_nothing():
    meta = _random_metadata(np.random.default_rng(7), 20)
    ix = _fresh(meta)
    for rows, new in (([20], [{}]), ([-1], [{}]), ([3, 3], [{}, {}]), ([1, 2], [{}])):
        with pytest.raises(ValueError):
            ix.replace(rows, new)
    _assert_same_as_fresh(ix, meta)

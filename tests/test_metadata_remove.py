"""MetadataIndex.remove (service/metadata_index.py): after rows are dropped, every filter's bitmap
equals that of a fresh index built from the surviving metadata (the renumbering the device index
applies: row r becomes r - removed rows below r).  CPU only."""
import numpy as np
import pytest

from service.metadata_index import MetadataIndex


def _metadata(n):
    out = []
    for i in range(n):
        m = {"doc": "abc"[i % 3], "n": i % 5}
        if i % 4 == 0:
            m["tag"] = None           # an explicit None
        elif i % 4 == 1:
            m["tag"] = "x"            # (rows 2, 3 mod 4 lack the key)
        if i % 7 == 0:
            m["list"] = [i % 2, "v"]  # an unhashable value
        if i % 11 == 0:
            m["f"] = 1.0              # hashes like 1 and True
        out.append(m)
    return out


FILTERS = [
    {"doc": "a"}, {"doc": "b", "n": 3}, {"doc": "zzz"}, {"n": 1}, {"n": 1.0}, {"n": True},
    {"tag": None}, {"tag": "x"}, {"tag": None, "doc": "c"}, {"missing": None}, {"missing": 1},
    {"list": [0, "v"]}, {"list": [1, "v"], "doc": "a"}, {"list": None}, {"f": 1}, {"f": None}, {},
]


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
            # the reference's scan over the survivors
            scan = [i for i, m in enumerate(meta[:n]) if all(m.get(a) == b for a, b in f.items())]
            bits = np.unpackbits(got[0].view(np.uint8), bitorder="little")
            assert np.nonzero(bits)[0].tolist() == scan, (f, n)


N = 203

ROW_SETS = {
    "first": [0],
    "last": [N - 1],
    "first_and_last": [0, N - 1],
    "every_third": list(range(0, N, 3)),
    "block": list(range(40, 110)),
    "repeats_unsorted": [17, 5, 17, 200, 5],
    "random": sorted(np.random.default_rng(3).permutation(N)[:77].tolist()),
    "none": [],
}


@pytest.mark.parametrize("name", sorted(ROW_SETS))
def test_remove_equals_a_fresh_index_of_the_survivors(name):
    meta = _metadata(N)
    rows = ROW_SETS[name]
    ix = _fresh(meta)
    assert ix.remove(rows) == len(set(rows))
    gone = set(rows)
    _assert_same_as_fresh(ix, [m for i, m in enumerate(meta) if i not in gone])


def test_remove_all_rows_then_extend():
    meta = _metadata(N)
    ix = _fresh(meta)
    assert ix.remove(np.arange(N)) == N
    assert len(ix) == 0
    _assert_same_as_fresh(ix, [])
    ix.extend(meta[:50])  # rows number from 0 again
    _assert_same_as_fresh(ix, meta[:50])


def test_stale_cache_entry_is_dropped():
    meta = _metadata(N)
    ix = _fresh(meta)
    # the same (filter, row count) key before and after: remove 3 rows, add 3 back
    before = ix.bitmap({"doc": "a"}, N)
    assert ix.bitmap({"doc": "a"}, N) is before  # cached
    ix.remove([0, 3, 6])
    extra = [{"doc": "b"}, {"doc": "b"}, {"doc": "a"}]
    ix.extend(extra)
    assert len(ix) == N
    survivors = [m for i, m in enumerate(meta) if i not in (0, 3, 6)] + extra
    _assert_same_as_fresh(ix, survivors)
    assert not np.array_equal(ix.bitmap({"doc": "a"}, N)[0], before[0])


def test_remove_then_remove_again():
    meta = _metadata(N)
    ix = _fresh(meta)
    ix.remove(list(range(0, N, 2)))
    meta = [m for i, m in enumerate(meta) if i % 2]
    ix.remove([0, len(meta) - 1, 10])
    meta = [m for i, m in enumerate(meta) if i not in (0, len(meta) - 1, 10)]
    _assert_same_as_fresh(ix, meta)


def test_out_of_range_rows_raise_and_change_nothing():
    meta = _metadata(20)
    ix = _fresh(meta)
    for bad in ([20], [-1], [3, 25]):
        with pytest.raises(ValueError):
            ix.remove(bad)
    _assert_same_as_fresh(ix, meta)

"""MetadataIndex.rows (service/metadata_index.py): the sorted matching rows of a filter, the row
list the device's row-list search takes.  It is the set ``bitmap`` marks -- ascending, unique,
int64 -- for every kind of filter, for a row count below the metadata length, and after the
postings were renumbered (remove) or rewritten (replace).  ``bitmap`` itself is unchanged:
same words, same count, same cache behaviour.  No GPU."""
import numpy as np
import pytest

from service.metadata_index import MetadataIndex


def _meta(n=500):
    out = []
    for i in range(n):
        m = {"tenant": i % 7, "kind": "a" if i % 3 else "b"}
        if i % 5 == 0:
            m["opt"] = None if i % 10 == 0 else i % 4
        if i % 11 == 0:
            m["tags"] = ["x", i % 2]      # unhashable
        if i % 13 == 0:
            m["f"] = 1.0 if i % 2 else True  # 1 == 1.0 == True
        out.append(m)
    out[17] = {}          # no keys at all
    return out


FILTERS = [
    {"tenant": 3}, {"kind": "b"}, {"tenant": 3, "kind": "a"}, {"tenant": 3, "kind": "a", "opt": 1},
    {"opt": None}, {"opt": None, "tenant": 0}, {"missing": None}, {"missing": 1},
    {"tags": ["x", 1]}, {"tags": ["x", 1], "tenant": 4}, {"f": 1}, {"tenant": 99}, {},
    {"tenant": float("nan")},
]


def _naive(meta, filt, n):
    return [i for i, m in enumerate(meta[:n]) if all(m.get(k) == v for k, v in filt.items())] \
        if filt else list(range(n))


def _check(mi, meta, n):
    for filt in FILTERS:
        rows = mi.rows(filt, n)
        assert rows.dtype == np.int64 and rows.ndim == 1
        assert (np.diff(rows) > 0).all(), filt                      # ascending and unique
        words, hits = mi.bitmap(filt, n)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        np.testing.assert_array_equal(rows, np.nonzero(bits)[0], err_msg=str(filt))
        assert hits == rows.size
        want = _naive(meta, filt, n)
        if filt and all(v is None for v in filt.values()):
            want += list(range(len(meta), n))  # rows past the metadata list hold no key: get() is None
        assert rows.tolist() == want, filt


@pytest.mark.parametrize("n", [500, 499, 321, 32, 1, 0])
def test_rows_equal_the_bitmap_and_the_scan(n):
    meta = _meta()
    mi = MetadataIndex()
    mi.extend(meta)
    _check(mi, meta, n)


def test_rows_past_the_metadata_have_no_keys():
    meta = _meta(100)
    mi = MetadataIndex()
    mi.extend(meta)
    mi._n = 100
    _check(mi, meta, 130)  # (persistence pads: more vectors than metadata entries)


def test_after_remove_and_replace():
    meta = _meta()
    mi = MetadataIndex()
    mi.extend(meta)
    gone = [0, 3, 17, 21, 250, 499]
    mi.remove(gone)
    meta = [m for i, m in enumerate(meta) if i not in set(gone)]
    _check(mi, meta, len(meta))
    ids = [5, 40, 41, 300]
    new = [{"tenant": 3, "kind": "b"}, {}, {"tenant": 3, "tags": ["x", 1]}, {"opt": None, "tenant": 0}]
    mi.replace(ids, new)
    for i, m in zip(ids, new):
        meta[i] = m
    _check(mi, meta, len(meta))
    _check(mi, meta, 200)


def test_rows_is_the_callers_copy_and_bitmap_cache_is_untouched():
    mi = MetadataIndex()
    mi.extend(_meta())
    a = mi.rows({"tenant": 3}, 500)
    a[:] = -1
    b = mi.rows({"tenant": 3}, 500)
    assert (b >= 0).all()                           # the postings were not handed out
    assert len(mi._cache) == 0                      # rows() caches nothing
    w1 = mi.bitmap({"tenant": 3}, 500)
    assert len(mi._cache) == 1 and mi.bitmap({"tenant": 3}, 500) is w1   # the cached tuple, as before
    mi.rows({"tenant": 3}, 500)
    assert len(mi._cache) == 1

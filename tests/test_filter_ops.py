"""The filter language on the host (service/filter_ops.py, service/metadata_index.py): parsing and
every ValueError; ``numeric_column`` with bool, string, NaN and 2^53 + 1 values, its ``exact`` flag
and rows without a metadata entry; the host evaluation of every operator against the per-row oracle
of tests/_filter_cases.py; ``bitmap`` / ``rows`` on plain filters unchanged; and ``_filter_key``
grouping equal condition dicts together.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _filter_cases as fc  # noqa: E402

from service import filter_ops  # noqa: E402
from service.metadata_index import MetadataIndex  # noqa: E402

N = 300


@pytest.fixture(scope="module")
def metadata():
    md = fc.store_metadata(N)
    md[5]["big"] = 2**53 + 1
    md[6]["big"] = 7
    return md


@pytest.fixture(scope="module")
def index(metadata):
    mi = MetadataIndex()
    mi.extend(metadata)
    return mi


# ---- parsing -------------------------------------------------------------------------------------
def test_what_is_a_condition():
    assert filter_ops.is_condition({"$gt": 1}) and filter_ops.is_condition({"$gt": 1, "$lt": 2})
    for v in ({}, {"a": 1}, {"$gt": 1, "a": 2}, 5, "x", None, [1], {1: 2}):
        assert not filter_ops.is_condition(v), v
    plain, conds = filter_ops.split_filter({"a": 1, "b": {"x": 1}, "c": {"$gte": 2, "$in": [1, 2]}, "d": {}})
    assert plain == {"a": 1, "b": {"x": 1}, "d": {}}
    assert conds == {"c": [("$gte", 2), ("$in", (1, 2))]}
    assert filter_ops.split_filter(None) == ({}, {})
    assert filter_ops.has_conditions({"a": {"$ne": 1}}) and not filter_ops.has_conditions({"a": {"b": 1}})


@pytest.mark.parametrize("cond", [
    {"$foo": 1}, {"$gt": 1, "$regex": "x"}, {"$or": [{"a": 1}]},
    {"$gt": "5"}, {"$gte": None}, {"$lt": True}, {"$lte": float("nan")}, {"$gt": [1]},
    {"$in": 5}, {"$nin": "abc"}, {"$exists": 1}, {"$exists": "yes"},
])
def test_malformed_conditions_raise(cond, index):
    with pytest.raises(ValueError):
        filter_ops.split_filter({"k": cond})
    with pytest.raises(ValueError):
        index.bitmap({"k": cond}, N)
    with pytest.raises(ValueError):
        filter_ops.row_matches({"k": 1}, {"k": cond})


def test_fold_range_is_the_intersection():
    inf = math.inf
    assert filter_ops.fold_range([]) == (-inf, True, inf, True)
    assert filter_ops.fold_range([("$gt", 1), ("$gte", 1)]) == (1, False, inf, True)
    assert filter_ops.fold_range([("$gte", 1), ("$gt", 1)]) == (1, False, inf, True)
    assert filter_ops.fold_range([("$gte", 1), ("$gte", 3), ("$lt", 9), ("$lte", 9)]) == (3, True, 9, False)
    assert filter_ops.fold_range([("$lte", 2**53 + 1)]) == (-inf, True, 2**53 + 1, True)
    for v in (0, 1, 2, 3, 8.5, 9, 10):
        ops = [("$gte", 1), ("$gt", 2), ("$lt", 9), ("$lte", 20)]
        assert filter_ops.in_interval(v, filter_ops.fold_range(ops)) == (2 < v < 9)
    assert filter_ops.float_exact(5) and filter_ops.float_exact(2.5) and filter_ops.float_exact(2**53)
    assert not filter_ops.float_exact(2**53 + 1) and not filter_ops.float_exact(10**400)


# ---- numeric_column --------------------------------------------------------------------------------
def test_numeric_column_values_and_missing_rows(index, metadata):
    col, exact = index.numeric_column("ts", N)
    assert exact and col.dtype == np.float64 and col.shape == (N,)
    for r, m in enumerate(metadata):
        v = m.get("ts")
        if isinstance(v, (int, float)) and not isinstance(v, bool):
            assert col[r] == v, r
        else:
            assert math.isnan(col[r]), (r, v)  # string, bool, missing
    price, exact = index.numeric_column("price", N)
    assert exact
    for r, m in enumerate(metadata):
        v = m.get("price")
        assert (math.isnan(price[r]) if v is None or math.isnan(v) else price[r] == v), r
    none, exact = index.numeric_column("no such key", N)
    assert exact and np.isnan(none).all()
    tenant, _ = index.numeric_column("tenant", N)
    assert np.isnan(tenant).all()


def test_numeric_column_exact_flag_and_rows_past_the_metadata(index):
    big, exact = index.numeric_column("big", N)
    assert not exact and big[6] == 7.0 and big[5] == float(2**53)
    # rows with no metadata entry (fewer dicts than vectors) and a shorter n
    col, exact = index.numeric_column("ts", N + 10)
    assert col.shape == (N + 10,) and np.isnan(col[N:]).all()
    assert index.numeric_column("ts", 7)[0].shape == (7,)
    mi = MetadataIndex()
    mi.extend([{"v": True}, {"v": 1}, {"v": 1.0}, {"v": False}, {"v": 0}, {"v": -0.0}, "not a dict", {"v": float("nan")}])
    col, exact = mi.numeric_column("v", 8)
    assert exact
    np.testing.assert_array_equal(np.isnan(col), [True, False, False, True, False, False, True, True])
    np.testing.assert_array_equal(col[[1, 2, 4, 5]], [1.0, 1.0, 0.0, 0.0])


# ---- host evaluation against the per-row oracle ----------------------------------------------------------
OPERATOR_FILTERS = fc.STORE_FILTERS + [
    {"ts": {"$eq": 5}}, {"tenant": {"$eq": "t2"}}, {"ts": {"$eq": None}}, {"ts": {"$eq": True}},
    {"ts": {"$ne": "yesterday"}}, {"ts": {"$ne": None}}, {"tenant": {"$ne": "t0"}},
    {"tenant": {"$in": ["t1", "t3", "nobody"]}}, {"tenant": {"$in": []}}, {"ts": {"$in": [None, "yesterday"]}},
    {"tenant": {"$nin": ["t1"]}}, {"tenant": {"$nin": []}}, {"ts": {"$nin": [True, "yesterday"]}},
    {"ts": {"$exists": True}}, {"ts": {"$exists": False}}, {"price": {"$exists": True}},
    {"ts": {"$gt": 500}}, {"ts": {"$gte": 500}}, {"ts": {"$lt": 500}}, {"ts": {"$lte": 500}},
    {"ts": {"$gt": 500.25}}, {"ts": {"$lt": -1}}, {"ts": {"$gte": -math.inf}}, {"ts": {"$gt": math.inf}},
    {"ts": {"$gte": 900, "$lt": 100}}, {"price": {"$gte": 0}}, {"price": {"$lte": 4.75, "$ne": 2.5}},
    {"big": {"$gt": 2**53}}, {"big": {"$gte": 2**53 + 1}}, {"big": {"$lt": 2**53 + 1}}, {"big": {"$lte": float(2**53)}},
    {"tenant": {"$gt": 0}}, {"no such key": {"$lt": 5}}, {"no such key": {"$exists": False}},
    {"tenant": "t1", "ts": {"$gte": 100, "$lte": 800}, "price": {"$exists": True}},
]


@pytest.mark.parametrize("filt", OPERATOR_FILTERS, ids=repr)
def test_host_evaluation_equals_the_per_row_oracle(index, metadata, filt):
    want = fc.meta_bits(metadata, filt)
    words, count = index.bitmap(filt, N)
    np.testing.assert_array_equal(fc.unwords(words, N), want)
    assert count == int(want.sum())
    np.testing.assert_array_equal(index.rows(filt, N), np.nonzero(want)[0])
    assert [filter_ops.row_matches(m, filt) for m in metadata] == want.tolist()
    # cached: the same answer again, and for an equal filter written as new dict objects
    again = {k: (dict(v) if isinstance(v, dict) else v) for k, v in filt.items()}
    np.testing.assert_array_equal(index.bitmap(again, N)[0], words)


def test_range_rows_alone_and_a_shorter_n(index, metadata):
    rows = index.range_rows("ts", [("$gte", 200), ("$lt", 700)], N)
    np.testing.assert_array_equal(rows, np.nonzero(fc.meta_bits(metadata, {"ts": {"$gte": 200, "$lt": 700}}))[0])
    short = index.range_rows("ts", [("$gte", 200), ("$lt", 700)], 50)
    np.testing.assert_array_equal(short, rows[rows < 50])
    want = fc.meta_bits(metadata, {"ts": {"$ne": 3}}, n=N + 5)  # rows past the metadata hold no key
    np.testing.assert_array_equal(fc.unwords(index.bitmap({"ts": {"$ne": 3}}, N + 5)[0], N + 5), want)
    assert want[N:].all()


def test_evaluation_follows_remove_and_replace(metadata):
    md = [dict(m) for m in metadata]
    mi = MetadataIndex()
    mi.extend(md)
    filt = {"ts": {"$gte": 300, "$lt": 900}}
    mi.replace([0, 1], [{"ts": 400}, {"ts": True}])
    md[0], md[1] = {"ts": 400}, {"ts": True}
    np.testing.assert_array_equal(mi.rows(filt, N), np.nonzero(fc.meta_bits(md, filt))[0])
    mi.remove([0, 10, 11])
    md = [m for r, m in enumerate(md) if r not in (0, 10, 11)]
    np.testing.assert_array_equal(mi.rows(filt, N - 3), np.nonzero(fc.meta_bits(md, filt))[0])
    col, _ = mi.numeric_column("ts", N - 3)
    assert math.isnan(col[0])  # the row that now holds True


# ---- plain filters unchanged ----------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [{"tenant": "t1"}, {"tenant": "t1", "id": 5}, {"ts": None}, {"ts": 1}, {"ts": True},
                                  {"tenant": {"a": 1}}, {"tenant": ["t1"]}, {"ts": "yesterday"}, {},
                                  {"tenant": {"$gt": 1, "x": 2}}], ids=repr)
def test_plain_filters_keep_the_equality_meaning(index, metadata, filt):
    want = np.array([all(m.get(k) == v for k, v in filt.items()) for m in metadata])
    words, count = index.bitmap(filt, N)
    np.testing.assert_array_equal(fc.unwords(words, N), want)
    assert count == int(want.sum())
    np.testing.assert_array_equal(index.rows(filt, N), np.nonzero(want)[0])


def test_plain_bitmaps_are_still_cached(index):
    a = index.bitmap({"tenant": "t2"}, N)
    assert index.bitmap({"tenant": "t2"}, N) is a


def test_range_bitmaps_take_no_cache_entry(metadata):
    mi = MetadataIndex()
    mi.extend(metadata)
    plain = mi.bitmap({"tenant": "t2"}, N)
    for t in range(2 * MetadataIndex.CACHE):  # per-request bounds, more of them than the cache holds
        mi.bitmap({"ts": {"$gte": t}}, N)
        mi.bitmap({"tenant": "t1", "ts": {"$lt": t}}, N)
    assert mi.bitmap({"tenant": "t2"}, N) is plain, "the recurring bitmap was evicted by range filters"
    a = mi.bitmap({"tenant": {"$in": ["t1", "t2"]}}, N)
    assert mi.bitmap({"tenant": {"$in": ("t1", "t2")}}, N) is a, "a posting-only condition is cached"


def test_version_moves_with_every_change(metadata):
    mi = MetadataIndex()
    seen = [mi.version]
    for change in (lambda: mi.extend(metadata[:10]), lambda: mi.replace([0], [{"ts": 1}]), lambda: mi.remove([1]),
                   lambda: mi.clear()):
        change()
        seen.append(mi.version)
    assert len(set(seen)) == len(seen)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 1000, 100_003])
def test_mask_rows_reads_the_set_bits_of_the_non_zero_words(n):
    from service.optimized_vector_store import _mask_rows
    rng = np.random.default_rng(n)
    for hits in (0, 1, min(n, 7), min(n, 68)):
        rows = np.sort(rng.choice(n, size=hits, replace=False)).astype(np.int64)
        bits = np.zeros(n, bool)
        bits[rows] = True
        got = _mask_rows(fc.words(bits), n)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, rows)
    full = np.ones(n, bool)
    np.testing.assert_array_equal(_mask_rows(fc.words(full), n), np.arange(n))
    # bits at or past n (a caller's padded mask) name no row; extra words are ignored
    padded = np.concatenate([np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32), np.full(3, 0xFFFFFFFF, np.uint32)])
    np.testing.assert_array_equal(_mask_rows(padded, n), np.arange(n))


# ---- grouping ----------------------------------------------------------------------------------------
def test_filter_key_groups_equal_condition_dicts():
    from service.optimized_vector_store import _filter_key
    a = {"ts": {"$gte": 5, "$lt": 9}, "tenant": "t1"}
    b = {"tenant": "t1", "ts": {"$lt": 9, "$gte": 5}}
    assert a is not b and a["ts"] is not b["ts"]
    assert _filter_key(a) == _filter_key(b) and hash(_filter_key(a)) == hash(_filter_key(b))
    assert _filter_key({"t": {"$in": ["a", "b"]}}) == _filter_key({"t": {"$in": ("a", "b")}})
    assert _filter_key(a) != _filter_key({"ts": {"$gte": 5, "$lt": 10}, "tenant": "t1"})
    assert _filter_key({"ts": {"$gte": 5}}) != _filter_key({"ts": {"$gt": 5}})
    assert _filter_key({"tenant": "t1"}) == _filter_key({"tenant": "t1"})
    u = {"tenant": ["unhashable"]}
    assert _filter_key(u) == ("unhashable", id(u))

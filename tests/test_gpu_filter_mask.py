"""Numeric columns and predicate masks on the device (include/vdb.h vdb_index_set_column /
vdb_index_filter_mask; csrc/vdb_filter.hip).

The contract: bit r of predicate p's mask is set iff r < count, every clause of the predicate holds
for row r's column values (plain IEEE fp64 compares; NaN = no value) and the base mask has the bit;
counts are the bits set; bits at or past count are 0; nothing past [P][W] is written.  Every case
compares masks and counts with the numpy restatement of tests/_filter_cases.py with
``assert_array_equal`` -- the answer is a set, so no tolerance appears anywhere -- and the
restatement is checked once against the per-row Python oracle.

Shapes: dim 8 and the row counts of _filter_cases.SIZES -- odd and even W, below, at and above one
wave's 64 rows and one workgroup's 256, a partial last word, and 4099 rows for more than one
workgroup -- with three columns and 1, 3 and 256 predicates (0, 1 and 8 clauses, every flag
combination, bounds equal to stored values, +-inf bounds, lo > hi).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _filter_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu

DIM = 8
GUARD = 67  # guard words / counts past the last mask / count of a device call
S_WORD, S_CNT = 0xDEADBEEF, -9
FILTER_STATS = ("filter_calls", "filter_preds", "column_sets", "column_slots")
SEARCH_STATS = ("searches", "queries", "searches_fp32", "searches_bf16x3", "searches_bf16", "searches_i8",
                "searches_i8x3", "searches_i8q", "searches_q4", "searches_wide", "range_searches")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _vectors(n, seed=0):
    return np.random.default_rng(50 + seed).standard_normal((n, DIM)).astype(np.float32)


def _index(vdb, n, cols=None):
    ix = vdb.NativeIndex(DIM, "cosine")
    if n:
        ix.add(_vectors(n))
    if cols is not None:
        for s in range(cols.shape[0]):
            ix.set_column(s, cols[s])
    return ix


@pytest.fixture(scope="module")
def indexes(vdb):
    """One index per row count with the three columns attached, shared by the read-only cases."""
    made = {}

    def get(n):
        if n not in made:
            cols = fc.columns(n)
            made[n] = (_index(vdb, n, cols), cols)
        return made[n]

    yield get
    for ix, _ in made.values():
        ix.close()


@pytest.fixture(scope="module")
def expected():
    """The restatement per (n, P, with base), computed once."""
    memo = {}

    def get(n, P, based):
        key = (n, P, based)
        if key not in memo:
            base = fc.base_masks(P, n) if based else None
            memo[key] = (base,) + fc.restate(fc.columns(n), fc.predicates(P), base)
        return memo[key]

    return get


def _stats(ix, names):
    return {s: ix.stat(s) for s in names}


def _device_call(vdb, torch, ix, preds, base, n, offset_words=0):
    """filter_mask_device with guarded outputs -> (masks [P, W], counts [P]); the guards checked."""
    clauses, offs = vdb.pack_predicates(preds)
    P, W = len(preds), fc.n_words(n)
    out = torch.full((offset_words + P * W + GUARD,), S_WORD - 2**32, dtype=torch.int32, device="cuda")
    cnt = torch.full((P + GUARD,), S_CNT, dtype=torch.int64, device="cuda")
    base_t = None
    if base is not None:
        base_t = torch.from_numpy(np.ascontiguousarray(base).view(np.int32)).to("cuda")
    torch.cuda.synchronize()
    ix.filter_mask_device(clauses, offs, base_t.data_ptr() if base_t is not None else 0,
                          out.data_ptr() + 4 * offset_words, cnt.data_ptr(), stream=0)
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    c = cnt.cpu().numpy()
    assert (o[:offset_words] == S_WORD).all(), "words before the masks touched"
    assert (o[offset_words + P * W:] == S_WORD).all(), "mask guard touched"
    assert (c[P:] == S_CNT).all(), "count guard touched"
    return o[offset_words:offset_words + P * W].reshape(P, W), c[:P]


def test_restatement_agrees_with_the_per_row_oracle():
    n = 257
    cols = fc.columns(n)
    preds = fc.predicates(256)
    masks, counts = fc.restate(cols, preds)
    for p, pred in enumerate(preds):
        bits = fc.oracle_bits(cols, pred)
        np.testing.assert_array_equal(fc.unwords(masks[p], n), bits, err_msg=f"predicate {p}")
        assert counts[p] == bits.sum()


@pytest.mark.parametrize("based", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("P", fc.PREDS)
@pytest.mark.parametrize("n", fc.SIZES)
def test_host_masks_and_counts_equal_the_restatement(vdb, indexes, expected, n, P, based):
    ix, _ = indexes(n)
    base, em, ec = expected(n, P, based)
    before = _stats(ix, FILTER_STATS + SEARCH_STATS)
    masks, counts = ix.filter_mask(fc.predicates(P), base)
    np.testing.assert_array_equal(masks, em)
    np.testing.assert_array_equal(counts, ec)
    tail = n % 32
    if tail:
        assert not (masks[:, -1] >> np.uint32(tail)).any(), "bits at or past n in the last word"
    after = _stats(ix, FILTER_STATS + SEARCH_STATS)
    assert after["filter_calls"] == before["filter_calls"] + 1
    assert after["filter_preds"] == before["filter_preds"] + P
    for s in SEARCH_STATS + ("column_sets", "column_slots"):
        assert after[s] == before[s], s


@pytest.mark.parametrize("based", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("P", fc.PREDS)
@pytest.mark.parametrize("n", fc.SIZES)
def test_device_masks_and_counts_equal_the_restatement_guards_untouched(vdb, torch, indexes, expected, n, P, based):
    ix, _ = indexes(n)
    base, em, ec = expected(n, P, based)
    masks, counts = _device_call(vdb, torch, ix, fc.predicates(P), base, n)
    np.testing.assert_array_equal(masks, em)
    np.testing.assert_array_equal(counts, ec)


@pytest.mark.parametrize("n", [33, 97, 257, 4099])
def test_device_output_offset_by_one_word(vdb, torch, indexes, expected, n):
    ix, _ = indexes(n)
    base, em, ec = expected(n, 3, True)
    masks, counts = _device_call(vdb, torch, ix, fc.predicates(3), base, n, offset_words=1)
    np.testing.assert_array_equal(masks, em)
    np.testing.assert_array_equal(counts, ec)


def test_device_set_column_and_no_counts(vdb, torch, expected):
    n = 257
    cols = fc.columns(n)
    ix = _index(vdb, n)
    try:
        for s in range(fc.N_COLS):
            t = torch.from_numpy(cols[s]).to("cuda")
            ix.set_column_device(s, t.data_ptr(), n)
        assert ix.stat("column_slots") == 0b111 and ix.stat("column_sets") == 3
        _, em, ec = expected(n, 3, False)
        masks, counts = ix.filter_mask(fc.predicates(3))
        np.testing.assert_array_equal(masks, em)
        np.testing.assert_array_equal(counts, ec)
        # no counts wanted: NULL out_counts
        clauses, offs = vdb.pack_predicates(fc.predicates(3))
        out = torch.zeros(3 * fc.n_words(n), dtype=torch.int32, device="cuda")
        ix.filter_mask_device(clauses, offs, 0, out.data_ptr(), 0)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32).reshape(3, -1), em)
    finally:
        ix.close()


@pytest.mark.parametrize("n", [97, 4099])
def test_device_mask_feeds_a_device_search_on_the_same_stream(vdb, torch, indexes, n):
    ix, cols = indexes(n)
    pred = [(0, 0.0, 5.0, fc.LO | fc.HI), (1, 2.0, 2.0, fc.LO | fc.HI | fc.NEG)]
    bits = fc.oracle_bits(cols, pred)
    assert 0 < bits.sum() < n
    Q = _vectors(4, seed=9)
    k = int(min(10, bits.sum()))
    es, ei = ix.search(Q, k, row_mask=fc.words(bits))
    clauses, offs = vdb.pack_predicates([pred])
    stream = torch.cuda.Stream()
    q_t = torch.from_numpy(Q).to("cuda")
    mask_t = torch.zeros(fc.n_words(n), dtype=torch.int32, device="cuda")
    s_t = torch.empty((4, k), dtype=torch.float32, device="cuda")
    i_t = torch.empty((4, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        # no synchronisation between the two calls: the search reads the mask in stream order
        ix.filter_mask_device(clauses, offs, 0, mask_t.data_ptr(), 0, stream=stream.cuda_stream)
        ix.search_device(q_t.data_ptr(), 4, k, s_t.data_ptr(), i_t.data_ptr(), mask_ptr=mask_t.data_ptr(),
                         stream=stream.cuda_stream)
    stream.synchronize()
    np.testing.assert_array_equal(i_t.cpu().numpy(), ei)
    np.testing.assert_array_equal(s_t.cpu().numpy(), es)


def _raw(ix, clauses, offs, n_preds, out, counts=None, base=None, mem=0):
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    return ix._lib.vdb_index_filter_mask(ix._h, p(clauses), p(offs), n_preds, p(base), mem, p(out), p(counts), None)


def test_every_listed_error_is_invalid_and_moves_no_stat(vdb, indexes):
    n = 97
    ix, _ = indexes(n)
    W = fc.n_words(n)
    out = np.zeros(300 * W, np.uint32)
    dt = vdb.FILTER_CLAUSE_DTYPE
    ok = (0, 3, 1.0, 3.0)  # (column, flags, lo, hi)

    def cl(*rows):
        return np.array(list(rows), dtype=dt)

    offs1 = np.array([0, 1], np.int32)
    bad = {
        "slot -1": (cl((-1, 3, 1.0, 3.0)), offs1, 1),
        "slot 16": (cl((16, 3, 1.0, 3.0)), offs1, 1),
        "slot not attached": (cl((7, 3, 1.0, 3.0)), offs1, 1),
        "unknown flag bits": (cl((0, 8, 1.0, 3.0)), offs1, 1),
        "NaN lo": (cl((0, 3, np.nan, 3.0)), offs1, 1),
        "NaN hi": (cl((0, 3, 1.0, np.nan)), offs1, 1),
        "nine clauses": (cl(*([ok] * 9)), np.array([0, 9], np.int32), 1),
        "n_preds -1": (cl(ok), offs1, -1),
        "n_preds 257": (cl(*([ok] * 257)), np.arange(258, dtype=np.int32), 257),
        "offsets start at 1": (cl(ok, ok), np.array([1, 2], np.int32), 1),
        "offsets decrease": (cl(ok, ok), np.array([0, 2, 1], np.int32), 2),
    }
    before = _stats(ix, FILTER_STATS + SEARCH_STATS)
    for what, (c, o, P) in bad.items():
        for mem in (0, 1):  # the clauses are checked on the host for both memory kinds, before any launch
            assert _raw(ix, c, o, P, out, mem=mem) == vdb.VDB_ERR_INVALID, (what, mem)
    assert _raw(ix, cl(ok), offs1, 1, None) == vdb.VDB_ERR_INVALID, "NULL out_masks"
    assert _raw(ix, cl(ok), offs1, 1, out, mem=2) == vdb.VDB_ERR_INVALID, "bad mem"
    with pytest.raises(ValueError):
        ix.set_column(16, np.zeros(n))
    with pytest.raises(ValueError):
        ix.set_column(-1, np.zeros(n))
    with pytest.raises(ValueError):
        ix.set_column(3, np.zeros(n + 1))
    assert _stats(ix, FILTER_STATS + SEARCH_STATS) == before
    # the limits themselves are fine: 256 predicates, 8 clauses, no predicate at all
    assert _raw(ix, cl(*([ok] * 8)), np.array([0, 8], np.int32), 1, out) == 0
    assert _raw(ix, cl(*([ok] * 256)), np.arange(257, dtype=np.int32), 256, out) == 0
    assert _raw(ix, None, None, 0, None) == 0


def test_empty_index_gives_no_words_and_zero_counts(vdb):
    ix = _index(vdb, 0)
    try:
        ix.set_column(0, np.zeros(0))
        assert ix.stat("column_slots") == 1
        masks, counts = ix.filter_mask([[(0, 0.0, 1.0, 3)], []])
        assert masks.shape == (2, 0)
        np.testing.assert_array_equal(counts, [0, 0])
    finally:
        ix.close()


def test_lifecycle_add_remove_clear_drop_the_slots_update_keeps_them(vdb):
    n = 65
    cols = fc.columns(n)
    ix = _index(vdb, n, cols)
    pred = [[(1, 1.0, 3.0, 3)]]
    try:
        bytes0 = ix.stat("device_bytes")
        assert ix.stat("column_slots") == 0b111 and ix.stat("column_sets") == 3
        em, ec = fc.restate(cols, pred)
        # an update keeps them
        ix.update(np.array([3, 40], np.int64), _vectors(2, seed=5))
        assert ix.stat("column_slots") == 0b111
        m, c = ix.filter_mask(pred)
        np.testing.assert_array_equal(m, em)
        np.testing.assert_array_equal(c, ec)
        # detaching one slot leaves the others
        ix.set_column(1, None)
        assert ix.stat("column_slots") == 0b101
        with pytest.raises(ValueError):
            ix.filter_mask(pred)
        ix.set_column(1, cols[1])
        # an add drops them
        ix.add(_vectors(3, seed=6))
        assert ix.stat("column_slots") == 0
        with pytest.raises(ValueError):
            ix.filter_mask(pred)
        # a remove drops them
        for s in range(fc.N_COLS):
            ix.set_column(s, np.concatenate([cols[s], [1.0, 2.0, 3.0]]))
        assert ix.stat("column_slots") == 0b111
        ix.remove(np.array([n, n + 1, n + 2], np.int64))
        assert ix.stat("column_slots") == 0 and ix.count() == n
        with pytest.raises(ValueError):
            ix.filter_mask(pred)
        # a clear drops them
        for s in range(fc.N_COLS):
            ix.set_column(s, cols[s])
        m, c = ix.filter_mask(pred)
        np.testing.assert_array_equal(m, em)
        ix.clear()
        assert ix.stat("column_slots") == 0
        with pytest.raises(ValueError):
            ix.filter_mask(pred)
        assert ix.stat("column_sets") == 3 + 1 + 3 + 3
        assert ix.stat("device_bytes") >= bytes0
    finally:
        ix.close()


def test_device_bytes_counts_the_columns(vdb):
    n = 64
    ix = _index(vdb, n)
    try:
        b0 = ix.stat("device_bytes")
        ix.set_column(5, np.zeros(n))
        assert ix.stat("device_bytes") >= b0 + n * 8
        assert ix.stat("column_slots") == 1 << 5
    finally:
        ix.close()

"""Recommend search (include/vdb.h vdb_index_search_recommend; csrc/vdb_recommend.hip).

The contract: query b's vector is built from its positive and negative example rows, element by
element in fp64 in list order (mean of the positives, or (mp + mp) - mn with negatives; cosine over
rows divided by their canonical norms), rounded to fp32; the answer is what a search ranks for that
vector with the examples left out.  Every case compares the scores, indices, keys and the built
vectors with the literal oracle of tests/_recommend_cases.py (preconditions:
tests/test_recommend_precondition.py) BIT FOR BIT: the fp64 arrays as uint64, the fp32 arrays as
uint32; no tolerance appears anywhere.

Every host call goes through ``_call``: the output arrays carry a guard region of 257 sentinel
entries past [B][k] (past [B][dim] for the built vectors), which must be untouched afterwards.

Shapes are the smallest at which the kernels can go wrong: dims that leave pad columns (1, 33, 100),
one thread-stride of 256 plus 4 (260), three strides (768) and rows longer than the held-row key form
(2100); example counts from 1 to the limit of 64; k = 136 with 64 examples (the inner fetch at its
limit of 200); batches around the select's four waves per workgroup (1, 3, 4, 5, 130)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _recommend_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 257
S_IDX = -7
METRICS = rc.METRICS
VDB_ERR_INVALID = -1
STATS = ("searches", "queries", "recommend_searches", "recommend_queries", "recommend_bad_queries")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    assert _vdb.VDB_ERR_INVALID == VDB_ERR_INVALID
    return _vdb


def _index(vdb, V, metric, precision=None):
    ix = vdb.NativeIndex(V.shape[1], metric, precision=precision)
    if V.shape[0]:
        ix.add(V)
    assert ix.count() == V.shape[0]
    return ix


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what=""):
    """The outputs bit for bit (got / want: (scores, idx, keys, queries); None entries skipped)."""
    for name, g, w in zip(("scores", "indices", "keys", "queries"), got, want):
        if g is None or w is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} {what}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{name} {what}")


def _csr(lists):
    offs = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=offs[1:])
    rows = np.asarray([r for x in lists for r in x], np.int64)
    return offs, rows


def _call(ix, pos, neg, k, mask=None, index_offset=0, with_keys=True, with_queries=True, B=None, raw=None):
    """The C-ABI call in host memory with guarded outputs -> (rc, (scores, idx, keys, queries)).
    ``raw``: a dict overriding the arguments as sent (po, pr, n_pos, no, nr, n_neg, scores, idx)."""
    po, pr = _csr(pos)
    no, nr = _csr(neg) if neg is not None else (None, None)
    B = len(pos) if B is None else B
    n = max(B, 0) * max(k, 0)
    nq = max(B, 0) * ix.dim
    sc = np.full(n + GUARD, np.nan, np.float32)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    ks = np.full(n + GUARD, np.nan, np.float64) if with_keys else None
    qs = np.full(nq + GUARD, np.nan, np.float32) if with_queries else None
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    a = dict(po=po, pr=pr if pr.size else None, n_pos=pr.size, no=no, nr=nr if nr is not None and nr.size else None,
             n_neg=0 if nr is None else nr.size, scores=sc, idx=idx)
    a.update(raw or {})
    code = ix._lib.vdb_index_search_recommend(ix._h, B, k, _p(a["po"]), _p(a["pr"]), a["n_pos"], _p(a["no"]), _p(a["nr"]),
                                              a["n_neg"], _p(m), 0, _p(a["scores"]), _p(a["idx"]), _p(ks), _p(qs),
                                              index_offset, None)
    assert np.isnan(sc[n:]).all(), "scores guard touched"
    assert (idx[n:] == S_IDX).all(), "indices guard touched"
    assert ks is None or np.isnan(ks[n:]).all(), "keys guard touched"
    assert qs is None or np.isnan(qs[nq:]).all(), "queries guard touched"
    shape = (max(B, 0), max(k, 0))
    return code, (sc[:n].reshape(shape), idx[:n].reshape(shape), None if ks is None else ks[:n].reshape(shape),
                  None if qs is None else qs[:nq].reshape(max(B, 0), ix.dim))


def _check(ix, V, pos, neg, k, metric, mask=None, words=None, index_offset=0, what=""):
    """Call and compare with the oracle; ``mask``: bool [N] (``words``: the bitmap sent, if not its
    plain packing).  Returns the outputs."""
    want = rc.expected(V, pos, neg, k, metric, mask, index_offset)
    if words is None and mask is not None:
        words = rc.bitmap_words(mask)
    code, got = _call(ix, pos, neg, k, words, index_offset)
    what = f"{what} ({metric}, k {k})"
    assert code == 0, f"status {code} {what}: {ix._lib.vdb_last_error()}"
    _same(got, want, what)
    return got


def _empty(got, b=None):
    s, i, ks, qs = (x if b is None else x[b] for x in got)
    return (s == 0).all() and (i == -1).all() and np.isneginf(ks).all() and (qs == 0).all()


# =============================================================================
# shapes
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 33, 100, 260, 768, 2100])
def test_dims(vdb, dim, metric):
    V, _ = rc.corpus(700, dim)
    pos, neg = rc.example_lists(700)
    assert [len(p) + len(g) for p, g in zip(pos, neg)] == list(rc.EXAMPLE_COUNTS)
    ix = _index(vdb, V, metric)
    _check(ix, V, pos, neg, 10, metric, what=f"dim {dim}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_k(vdb, metric):
    V, _ = rc.corpus(700, 100)
    pos, neg = rc.example_lists(700)
    ix = _index(vdb, V, metric)
    for k in (1, 10):
        _check(ix, V, pos, neg, k, metric)
    ix.close()
    V, p, g = rc.full_house()  # k = 136 with 64 examples: the inner fetch is 200
    ix = _index(vdb, V, metric)
    s, i, ks, qs = _check(ix, V, [p, p[:1]], [g, ()], rc.MAX_K, metric, what="full house")
    assert (i >= 0).all()
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_the_order_of_the_additions(vdb, metric):
    """Rows of magnitudes 2^-20 .. 2^20: the fp64 sums round, so only the list order gives these bits."""
    V, pos, neg = rc.order_case()
    ix = _index(vdb, V, metric)
    _check(ix, V, pos, neg, 10, metric, what="order case")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_short_corpora(vdb, metric):
    V, _ = rc.corpus(50, 33)
    ix = _index(vdb, V, metric)
    rows = np.random.default_rng(1).permutation(50).tolist()
    s, i, ks, qs = _check(ix, V, [rows[:30]], [rows[30:45]], 10, metric, what="45 of 50 rows are examples")
    assert (i[0, :5] >= 0).all() and (i[0, 5:] == -1).all() and sorted(i[0, :5].tolist()) == sorted(rows[45:])
    s, i, ks, qs = _check(ix, V, [rows[:40]], [rows[40:]], 10, metric, what="every row is an example")
    assert (i == -1).all() and (s == 0).all() and np.isneginf(ks).all() and np.isfinite(qs).all() and qs.any()
    ix.close()
    empty = vdb.NativeIndex(33, metric)
    for neg in (None, [(), ()]):
        code, got = _call(empty, [(), ()], neg, 7)
        assert code == 0 and _empty(got)
    assert [empty.stat(s) for s in STATS] == [2, 4, 2, 4, 0]
    empty.close()


@pytest.mark.parametrize("metric", METRICS)
def test_odd_lists(vdb, metric):
    V, _ = rc.corpus(300, 100)
    ix = _index(vdb, V, metric)
    pos = [(5, 9, 5, 5), (17, 40), (), (), (250,)]
    neg = [(), (40, 3), (7, 8), (), (250,)]
    got = _check(ix, V, pos, neg, 10, metric, what="a repeated positive, a row in both lists, no positive")
    assert _empty(got, 2) and _empty(got, 3) and not _empty(got, 0)
    # the repeat counts: the same rows once each give another vector
    once = rc.expected(V, [(5, 9)], None, 10, metric)
    assert (_bits(once[3][0]) != _bits(got[3][0])).any()
    # no negatives at all: neg_offsets NULL
    _check(ix, V, [p for p in pos], None, 10, metric, what="neg_offsets NULL")
    assert ix.stat("recommend_bad_queries") == 0
    ix.close()


# =============================================================================
# masks, index_offset, batches
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_masks(vdb, metric):
    n = 300
    V, _ = rc.corpus(n, 100)
    ix = _index(vdb, V, metric)
    rng = np.random.default_rng(11)
    pos, neg = rc.example_lists(n, counts=(1, 4, 17))
    ex = sorted({r for l in pos + neg for r in l})
    half = rng.random(n) < 0.5
    _check(ix, V, pos, neg, 10, metric, mask=half, what="half")
    # bits at or past count name no row (n = 300: 20 spare bits in the last word, then a whole word)
    words = rc.bitmap_words(half, extra_bits=52)
    assert words.size == (n + 31) // 32 + 1
    _check(ix, V, pos, neg, 10, metric, mask=half, words=words, what="mask bits past count")
    only_ex = np.zeros(n, bool)
    only_ex[ex] = True
    # (another query's examples are rows like any other: they are all this batch returns)
    s, i, ks, qs = _check(ix, V, pos, neg, 10, metric, mask=only_ex, what="only examples are eligible")
    assert np.isin(i[i >= 0], ex).all()
    own = np.zeros(n, bool)
    own[list(pos[2] + neg[2])] = True
    s, i, ks, qs = _check(ix, V, pos[2:], neg[2:], 10, metric, mask=own, what="no non-example row is eligible")
    assert (i == -1).all() and qs.any()
    no_ex = ~only_ex
    masked = _check(ix, V, pos, neg, 10, metric, mask=no_ex, what="the examples themselves are not eligible")
    plain = _check(ix, V, pos, neg, 10, metric)
    _same((None, None, None, masked[3]), (None, None, None, plain[3]), "masked examples still count in the mean")
    few = np.zeros(n, bool)
    few[rng.choice(n, size=6, replace=False)] = True
    s, i, ks, qs = _check(ix, V, pos, neg, 10, metric, mask=few, what="fewer eligible rows than k")
    assert (i[:, 6:] == -1).all()
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_index_offset_moves_the_ids_only(vdb, metric):
    V, _ = rc.corpus(65, 33)
    pos, neg = rc.example_lists(65, counts=(1, 5, 17))
    ix = _index(vdb, V, metric)
    off = 2 ** 40
    base = _check(ix, V, pos, neg, 60, metric)
    moved = _check(ix, V, pos, neg, 60, metric, index_offset=off)
    np.testing.assert_array_equal(moved[1], np.where(base[1] >= 0, base[1] + off, -1))
    _same((moved[0], None, moved[2], moved[3]), (base[0], None, base[2], base[3]))
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("B", [1, 3, 4, 5, 130])
def test_batches(vdb, B, metric):
    V, _ = rc.corpus(300, 33)
    counts = tuple((1, 2, 3, 5, 17, 64)[b % 6] for b in range(B))
    pos, neg = rc.example_lists(300, seed=B, counts=counts)
    ix = _index(vdb, V, metric)
    _check(ix, V, pos, neg, 5, metric, what=f"B {B}")
    ix.close()


# =============================================================================
# properties
# =============================================================================
def test_euclidean_single_positive_is_a_search_by_that_row(vdb):
    V, _ = rc.corpus(700, 100)
    ix = _index(vdb, V, "euclidean")
    k = 10
    # p = the best row of some other row, so p really is slot 0 of its own search
    ps = [int(ix.search(V[r:r + 1], 2)[1][0, 1]) for r in (3, 44, 500)]
    code, got = _call(ix, [(p,) for p in ps], None, k)
    assert code == 0
    Q = np.ascontiguousarray(V[ps])
    _same((None, None, None, got[3]), (None, None, None, Q), "the built vector is the row")
    mask = np.random.default_rng(5).random(700) < 0.5
    for m in (None, mask):
        words = None if m is None else rc.bitmap_words(m)
        code, got = _call(ix, [(p,) for p in ps], None, k, words)
        assert code == 0
        s, i, ks = ix.search(Q, k + 1, row_mask=words, with_keys=True)
        for b, p in enumerate(ps):
            if m is None or m[p]:
                assert i[b, 0] == p
            keep = i[b] != p
            want = [x[b][keep][:k] for x in (s, i, ks)]
            _same([g[b] for g in got[:3]], want, f"row {p} struck out of search(k + 1)")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_precisions_give_the_same_bytes(vdb, metric):
    V, _ = rc.corpus(700, 100)
    pos, neg = rc.example_lists(700)
    mask = np.random.default_rng(4).random(700) < 0.6
    want = rc.expected(V, pos, neg, 10, metric)
    want_m = rc.expected(V, pos, neg, 10, metric, mask)
    for prec in ("auto", "i8", "i8x3", "bf16", "bf16x3", "fp32"):
        ix = _index(vdb, V, metric, precision=prec)
        code, got = _call(ix, pos, neg, 10)
        assert code == 0, prec
        _same(got, want, f"precision {prec}")
        code, got = _call(ix, pos, neg, 10, rc.bitmap_words(mask))
        assert code == 0, prec
        _same(got, want_m, f"precision {prec}, masked")
        ix.close()


def _device_call(ix, torch, st, pos, neg, k, words=None, opt=True, raw=None):
    """The call over torch tensors on stream ``st`` -> (scores, idx, keys, queries) as numpy, guards
    checked.  ``raw``: (po, pr, no, nr) numpy arrays sent as they are."""
    dev = torch.device("cuda")
    B = len(pos)
    po, pr = _csr(pos)
    no, nr = _csr(neg) if neg is not None else (None, None)
    if raw is not None:
        po, pr, no, nr = raw
    n, nq = B * k, B * ix.dim
    with torch.cuda.stream(st):
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        dpo, dpr, dno, dnr = up(po), up(pr if pr.size else np.zeros(1, np.int64)), up(no), up(
            None if nr is None else (nr if nr.size else np.zeros(1, np.int64)))
        dm = up(words.view(np.int32)) if words is not None else None
        ds = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        di = torch.full((n + GUARD,), S_IDX, dtype=torch.int64, device=dev)
        dk = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device=dev)
        dq = torch.full((nq + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        ix.search_recommend_device(B, k, dpo.data_ptr(), dpr.data_ptr(), pr.size, ds.data_ptr(), di.data_ptr(),
                                   neg_offsets_ptr=dno.data_ptr() if dno is not None else 0,
                                   neg_rows_ptr=dnr.data_ptr() if dnr is not None else 0,
                                   n_neg=0 if nr is None else nr.size, out_keys_ptr=dk.data_ptr() if opt else 0,
                                   out_queries_ptr=dq.data_ptr() if opt else 0,
                                   mask_ptr=dm.data_ptr() if dm is not None else 0, stream=st.cuda_stream)
    st.synchronize()
    s, i, kk, qq = (x.cpu().numpy() for x in (ds, di, dk, dq))
    assert np.isnan(s[n:]).all() and (i[n:] == S_IDX).all()
    assert np.isnan(kk[n if opt else 0:]).all() and np.isnan(qq[nq if opt else 0:]).all()
    return s[:n].reshape(B, k), i[:n].reshape(B, k), kk[:n].reshape(B, k), qq[:nq].reshape(B, ix.dim)


@pytest.mark.parametrize("metric", METRICS)
def test_device_memory(vdb, metric):
    import torch
    n, k = 700, 10
    V, _ = rc.corpus(n, 100)
    pos, neg = rc.example_lists(n)
    B = len(pos)
    ix = _index(vdb, V, metric)
    st = torch.cuda.Stream()
    mask = np.random.default_rng(3).random(n) < 0.7
    before = {s: ix.stat(s) for s in STATS}
    calls = 0
    for m, g, opt in ((None, neg, True), (mask, neg, True), (None, None, False)):
        words = None if m is None else rc.bitmap_words(m)
        code, host = _call(ix, pos, g, k, words)
        assert code == 0
        got = _device_call(ix, torch, st, pos, g, k, words, opt)
        calls += 2
        _same(got if opt else got[:2], host if opt else host[:2], "device against host memory")
        _same(host, rc.expected(V, pos, g, k, metric, m), "host against the oracle")
    after = {s: ix.stat(s) for s in STATS}
    assert [after[s] - before[s] for s in STATS] == [calls, calls * B, calls, calls * B, 0]
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_device_memory_bad_lists_come_back_empty(vdb, metric):
    """A device-memory call is not validated: a query with an id equal to count and one with 65
    examples come back empty and are counted; their neighbours match the oracle; offsets outside the
    id array are clamped."""
    import torch
    n, k = 300, 10
    V, _ = rc.corpus(n, 100)
    ix = _index(vdb, V, metric)
    st = torch.cuda.Stream()
    rng = np.random.default_rng(9)
    long = rng.choice(n, size=65, replace=False).tolist()
    pos = [(4, 8), (12, n, 13), (20,), tuple(long[:40]), (33, 34), ()]
    neg = [(1,), (), (21, 22), tuple(long[40:]), (), (5,)]
    before = ix.stat("recommend_bad_queries")
    got = _device_call(ix, torch, st, pos, neg, k)
    assert ix.stat("recommend_bad_queries") - before == 2
    want = rc.expected(V, [pos[0], (), pos[2], (), pos[4], ()], [neg[0], (), neg[2], (), neg[4], ()], k, metric)
    _same(got, want, "bad queries empty, neighbours as the oracle")
    assert _empty(got, 1) and _empty(got, 3) and _empty(got, 5)
    # offsets past the id arrays and below zero: clamped, nothing out of bounds is read
    po, pr = _csr([(4, 8), (20,)])
    no, nr = _csr([(1,), (21, 22)])
    po2 = po.copy()
    po2[2] = 10 ** 12
    no2 = no.copy()
    no2[0] = -5
    got = _device_call(ix, torch, st, [(), ()], None, k, raw=(po2, pr, no2, nr))
    _same(got, rc.expected(V, [(4, 8), (20,)], [(1,), (21, 22)], k, metric), "clamped offsets")
    ix.close()


# =============================================================================
# errors, stats, reuse
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_refused_calls_leave_the_stats_untouched(vdb, metric):
    n = 300
    V, _ = rc.corpus(n, 33)
    ix = _index(vdb, V, metric)
    pos, neg = [(1, 2), (3,)], [(4,), ()]
    _check(ix, V, pos, neg, 5, metric)
    before = {s: ix.stat(s) for s in STATS}
    i64 = lambda *a: np.asarray(a, np.int64)  # noqa: E731
    bad = [dict(k=0), dict(k=137), dict(k=-1), dict(B=-1),
           dict(raw=dict(po=None)), dict(raw=dict(scores=None)), dict(raw=dict(idx=None)),
           dict(raw=dict(po=i64(0, 2, 1))),                       # decreasing offsets
           dict(raw=dict(po=i64(0, 2, 4))),                       # an offset past n_pos
           dict(raw=dict(po=i64(-1, 2, 3))),                      # an offset below zero
           dict(raw=dict(pr=i64(1, -1, 3))), dict(raw=dict(pr=i64(1, n, 3))),   # id -1, id count
           dict(raw=dict(nr=i64(n))), dict(raw=dict(no=i64(0, 0, 2))),
           dict(raw=dict(no=None, nr=None)),                      # n_neg > 0 with NULL neg_offsets
           dict(raw=dict(n_pos=-1))]
    for kw in bad:
        code, got = _call(ix, pos, neg, kw.get("k", 5), B=kw.get("B"), raw=kw.get("raw"))
        assert code == VDB_ERR_INVALID, kw
        assert np.isnan(got[0]).all() and (got[1] == S_IDX).all() and np.isnan(got[3]).all(), f"outputs written on {kw}"
    rows = np.random.default_rng(2).permutation(n)[:65].tolist()
    for p, g in (([rows], None), ([rows[:64]], [rows[64:]]), ([rows[:1]], [rows[1:]]), ([()], [rows])):
        assert _call(ix, p, g, 5)[0] == VDB_ERR_INVALID, "65 examples"
    assert _call(ix, pos, neg, 5)[0] == 0  # (the one good call the stats below show)
    f = ix._lib.vdb_index_search_recommend
    po, pr = _csr(pos)
    sc, idx = np.zeros(10, np.float32), np.zeros(10, np.int64)
    assert f(ix._h, 2, 5, _p(po), _p(pr), 3, None, None, 0, None, 7, _p(sc), _p(idx), None, None, 0, None) == VDB_ERR_INVALID
    after = {s: ix.stat(s) for s in STATS}
    assert [after[s] - before[s] for s in STATS] == [1, 2, 1, 2, 0]
    # the binding raises ValueError with the limit in the message
    with pytest.raises(ValueError, match="136"):
        ix.search_recommend(pos, neg, 137)
    with pytest.raises(ValueError, match="64"):
        ix.search_recommend([rows], None, 5)
    with pytest.raises(ValueError):
        ix.search_recommend(pos, [(4,)], 5)
    with pytest.raises(ValueError, match="row_mask"):
        ix.search_recommend(pos, neg, 5, row_mask=np.zeros(3, np.uint32))
    assert {s: ix.stat(s) for s in STATS} == after
    _check(ix, V, pos, neg, 5, metric, what="the next good call")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_stats_no_queries_and_the_binding(vdb, metric):
    V, _ = rc.corpus(300, 33)
    pos, neg = rc.example_lists(300, counts=(1, 3, 17))
    ix = _index(vdb, V, metric)
    before = {s: ix.stat(s) for s in STATS}
    assert _call(ix, [], None, 5)[0] == 0 and _call(ix, [], [], 5)[0] == 0  # n_queries == 0 is OK and counts nothing
    assert {s: ix.stat(s) for s in STATS} == before
    want = rc.expected(V, pos, neg, 7, metric)
    for with_keys, with_queries in ((False, False), (True, False), (False, True)):
        code, got = _call(ix, pos, neg, 7, with_keys=with_keys, with_queries=with_queries)
        assert code == 0
        assert (got[2] is None) == (not with_keys) and (got[3] is None) == (not with_queries)
        _same(got, want, f"keys {with_keys} queries {with_queries}")
    after = {s: ix.stat(s) for s in STATS}
    assert [after[s] - before[s] for s in STATS] == [3, 9, 3, 9, 0]
    s, i = ix.search_recommend(pos, neg, 7)
    s2, i2, qs = ix.search_recommend(pos, neg, 7, with_queries=True)
    s3, i3, ks, qs3 = ix.search_recommend(pos, neg, 7, with_keys=True, with_queries=True)
    _same((s, i, None, None), want)
    _same((s2, i2, None, qs), want)
    _same((s3, i3, ks, qs3), want)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_workspace_reuse_add_update_remove(vdb, metric):
    V, _ = rc.corpus(400, 100)
    V = V.copy()
    ix = _index(vdb, V[:300], metric)
    pos, neg = rc.example_lists(300)
    first = _check(ix, V[:300], pos, neg, 10, metric)
    _check(ix, V[:300], pos[:3], neg[:3], 136, metric, what="another B and k on the same workspace")
    ix.add(V[300:])
    _check(ix, V, pos + ((399, 2),), neg + ((350,),), 10, metric, what="after add")
    # an example row changes: the new vector is used
    row = pos[1][0]
    V2 = V.copy()
    V2[row] = -V[row] + np.float32(0.25)
    assert ix.update(np.asarray([row]), V2[row:row + 1]) == 1
    second = _check(ix, V2, pos, neg, 10, metric, what="after update")
    assert (_bits(second[3][1]) != _bits(first[3][1])).any()
    gone = np.asarray([0, 7, 399, int(second[1][0, 0])])
    keep = np.setdiff1d(np.arange(400), gone)
    assert ix.remove(gone) == np.unique(gone).size
    p2, g2 = rc.example_lists(keep.size, seed=4)
    _check(ix, V2[keep], p2, g2, 10, metric, what="after remove")
    ix.close()


def test_non_finite_built_vector(vdb):
    """Euclidean rows of +-1.2e38 are finite, the index takes them and its exact path ranks them
    exactly (both checked here first); 2 * 1.2e38 + 1.2e38 is not an fp32: that query is all "no
    result" with a zero vector and is counted, its neighbour matches the oracle."""
    from oracle import ref_cpu
    V, pos, neg = rc.overflow_case()
    ix = vdb.NativeIndex(V.shape[1], "euclidean")
    ix.set_param("force_exact", 1)
    ix.add(V)
    assert ix.count() == 8
    Q = np.ascontiguousarray(V[[2, 7]])
    s, i, ks = ix.search(Q, 8, with_keys=True)
    es, ei, ek = ref_cpu.exact_search(Q, V, 8, "euclidean")
    np.testing.assert_array_equal(i, ei)
    np.testing.assert_array_equal(_bits(ks), _bits(ek))
    before = ix.stat("recommend_bad_queries")
    got = _check(ix, V, pos, neg, 3, "euclidean", what="overflow")
    assert _empty(got, 0) and (got[1][1] >= 0).all()
    assert ix.stat("recommend_bad_queries") - before == 1
    ix.close()

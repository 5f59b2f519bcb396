"""MMR search (include/vdb.h vdb_index_search_mmr; csrc/vdb_mmr.hip).

The contract: of query b's candidate list (the best fetch_k eligible rows by (canonical fp64 key
desc, row asc)) slot t holds the t-th greedy pick, the unpicked position with the greatest lambda *
rel_i - (1 - lambda) * (greatest pair similarity to a picked position), ties to the lower position;
with its fp32 score, fp64 key and fp64 mmr value; slots past min(k, list length) hold 0 / -1 / -inf /
-inf.  Every case compares all four outputs with the literal oracle of tests/_mmr_cases.py
(preconditions: tests/test_mmr_precondition.py) BIT FOR BIT: the fp64 arrays as uint64, the fp32
scores as uint32; no tolerance appears anywhere.

Every host call goes through ``_call``: the four output arrays carry a guard region past [B][k]
filled with a sentinel, which must be untouched afterwards.

Shapes are the smallest at which the kernels can go wrong: dims that leave pad columns (1, 33, 100),
one 256-dim piece plus 4 (260), three pieces (768) and rows too long to hold (2100: the any-length
key form); list lengths around a wave (63, 64, 65) and around the limit (199, 200, 201 rows); 210
queries at fetch_k = 200, which crosses the 209-query block of the pair scratch.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mmr_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 257
S_IDX = -7
METRICS = mc.METRICS
VDB_ERR_INVALID = -1
VDB_ERR_NONFINITE = -4
STATS = ("searches", "queries", "mmr_searches", "mmr_queries")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    assert _vdb.VDB_ERR_INVALID == VDB_ERR_INVALID and _vdb.VDB_ERR_NONFINITE == VDB_ERR_NONFINITE
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
    """The four outputs bit for bit (got / want: (scores, idx, keys, mmr); None entries skipped)."""
    for name, g, w in zip(("scores", "indices", "keys", "mmr"), got, want):
        if g is None or w is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} {what}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{name} {what}")


def _call(ix, Q, k, fetch_k, lam, mask=None, index_offset=0, with_keys=True, with_mmr=True, B=None):
    """The C-ABI call in host memory with guarded outputs -> (rc, (scores, idx, keys, mmr))."""
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    B = Q.shape[0] if B is None else B
    n = max(B, 0) * max(k, 0)
    sc = np.full(n + GUARD, np.nan, np.float32)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    ks = np.full(n + GUARD, np.nan, np.float64) if with_keys else None
    mm = np.full(n + GUARD, np.nan, np.float64) if with_mmr else None
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    code = ix._lib.vdb_index_search_mmr(ix._h, _p(Q), B, k, fetch_k, ctypes.c_double(lam), _p(m), 0, _p(sc), _p(idx),
                                        _p(ks), _p(mm), index_offset, None)
    assert np.isnan(sc[n:]).all(), "scores guard touched"
    assert (idx[n:] == S_IDX).all(), "indices guard touched"
    assert ks is None or np.isnan(ks[n:]).all(), "keys guard touched"
    assert mm is None or np.isnan(mm[n:]).all(), "mmr guard touched"
    shape = (max(B, 0), max(k, 0))
    return code, (sc[:n].reshape(shape), idx[:n].reshape(shape), None if ks is None else ks[:n].reshape(shape),
                  None if mm is None else mm[:n].reshape(shape))


def _check(ix, V, Q, k, fetch_k, lam, metric, mask=None, words=None, index_offset=0, what=""):
    """Call and compare with the oracle; ``mask``: bool [N] (``words``: the bitmap sent, if not its
    plain packing).  Returns the outputs."""
    Q = np.asarray(Q, np.float32).reshape(-1, ix.dim)
    want = mc.expected(Q, V, k, fetch_k, lam, metric, mask, index_offset)
    if words is None and mask is not None:
        words = mc.bitmap_words(mask)
    code, got = _call(ix, Q, k, fetch_k, lam, words, index_offset)
    what = f"{what} ({metric}, k {k}, fetch {fetch_k}, lambda {lam})"
    assert code == 0, f"status {code} {what}: {ix._lib.vdb_last_error()}"
    _same(got, want, what)
    return got


# =============================================================================
# shapes
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 33, 100, 260, 768, 2100])
def test_dims(vdb, dim, metric):
    V, Q = mc.corpus(700, dim)
    ix = _index(vdb, V, metric)
    _check(ix, V, Q[:3], 10, 64, 0.5, metric, what=f"dim {dim}")
    _check(ix, V, Q[3:4], 10, 64, 0.25, metric, what=f"dim {dim}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 199, 200, 201, 513])
def test_row_counts(vdb, n, metric):
    V, Q = mc.corpus(n, 100)
    ix = _index(vdb, V, metric)
    for k, fetch in ((200, 200), (10, 200)):
        s, i, ks, mm = _check(ix, V, Q[:2], k, fetch, 0.5, metric, what=f"n {n}")
        filled = min(k, n)
        assert (i[:, :filled] >= 0).all() and (i[:, filled:] == -1).all()
        assert (s[:, filled:] == 0).all() and np.isneginf(ks[:, filled:]).all() and np.isneginf(mm[:, filled:]).all()
        assert all(np.unique(r[:filled]).size == filled for r in i)  # no row twice
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_k_and_fetch_pairs(vdb, metric):
    V, Q = mc.corpus(700, 33)
    ix = _index(vdb, V, metric)
    for k, fetch in ((1, 1), (1, 200), (10, 10), (65, 65), (128, 129), (200, 200)):
        _check(ix, V, Q[:2], k, fetch, 0.5, metric)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_lambdas(vdb, metric):
    V, Q = mc.corpus(700, 100)
    ix = _index(vdb, V, metric)
    picks = []
    for lam in mc.LAMBDAS:
        picks.append(_check(ix, V, Q[:2], 10, 64, lam, metric)[1])
    assert any((picks[0] != p).any() for p in picks[1:]), "lambda never changed a pick"
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("B", [1, 2, 64, 65])
def test_batches(vdb, B, metric):
    V, Q = mc.corpus(300, 33, n_queries=65)
    ix = _index(vdb, V, metric)
    _check(ix, V, Q[:B], 5, 20, 0.5, metric, what=f"B {B}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_query_block_boundary(vdb, metric):
    """210 queries at fetch_k = 200: two blocks of the pair scratch (209 + 1).  The query of the
    second block equals the same query sent alone; it and queries of the first block equal the
    oracle."""
    B, k, fetch = 210, 10, 200
    assert mc.query_block(fetch) == 209
    V, Q = mc.corpus(300, 8, n_queries=B)
    ix = _index(vdb, V, metric)
    code, got = _call(ix, Q, k, fetch, 0.5)
    assert code == 0
    code, alone = _call(ix, Q[209:], k, fetch, 0.5)
    assert code == 0
    _same([g[209:] for g in got], alone, "the second block's query against itself alone")
    for b in (0, 208, 209):
        _same([g[b:b + 1] for g in got], mc.expected(Q[b:b + 1], V, k, fetch, 0.5, metric), f"query {b}")
    ix.close()


# =============================================================================
# masks
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_masks(vdb, metric):
    n = 300
    V, Q = mc.corpus(n, 100)
    ix = _index(vdb, V, metric)
    rng = np.random.default_rng(11)
    half = rng.random(n) < 0.5
    few = np.zeros(n, bool)
    few[rng.choice(n, size=40, replace=False)] = True
    one = np.zeros(n, bool)
    one[217] = True
    none = np.zeros(n, bool)
    _check(ix, V, Q[:3], 10, 64, 0.5, metric, what="no mask")
    _check(ix, V, Q[:3], 10, 64, 0.5, metric, mask=half, what="half")
    s, i, ks, mm = _check(ix, V, Q[:3], 50, 64, 0.5, metric, mask=few, what="fewer eligible rows than fetch_k")
    assert (i[:, :40] >= 0).all() and (i[:, 40:] == -1).all() and few[i[:, :40]].all()
    s, i, ks, mm = _check(ix, V, Q[:3], 10, 64, 0.5, metric, mask=one, what="one eligible row")
    assert (i[:, 0] == 217).all() and (i[:, 1:] == -1).all()
    s, i, ks, mm = _check(ix, V, Q[:3], 10, 64, 0.5, metric, mask=none, what="no eligible row")
    assert (i == -1).all() and (s == 0).all() and np.isneginf(ks).all() and np.isneginf(mm).all()
    # bits at or past count name no row (n = 300: 20 spare bits in the last word, then a whole word)
    words = mc.bitmap_words(half, extra_bits=52)
    assert words.size == (n + 31) // 32 + 1
    _check(ix, V, Q[:3], 10, 64, 0.5, metric, mask=half, words=words, what="mask bits past count")
    ix.close()


# =============================================================================
# equal keys: the position rule
# =============================================================================
@pytest.mark.parametrize("d", mc.PLANT_DIMS)
def test_planted_copies(vdb, d):
    V, q, rows = mc.planted_case(d)
    for metric, lam in (("cosine", 0.5), ("euclidean", 0.0)):
        ix = _index(vdb, V, metric)
        s, i, ks, mm = _check(ix, V, q, mc.PLANT_K, mc.PLANT_FETCH, lam, metric, what=f"planted dim {d}")
        assert np.isin(i[0], rows).sum() == 1
        plain = ix.search(q[None], mc.PLANT_K)[1][0]
        assert np.isin(plain, rows).sum() == mc.PLANT_K
        _check(ix, V, q, mc.PLANT_K, mc.PLANT_FETCH, 0.5, metric, what=f"planted dim {d}")
        ix.close()


def test_tied_values_follow_the_position_rule(vdb):
    V, Q = mc.tie_case()
    ix = _index(vdb, V, "cosine")
    for lam in mc.LAMBDAS:
        _check(ix, V, Q, 10, 64, lam, "cosine", what="one dim")
    _check(ix, V, Q, 200, 200, 0.5, "cosine", what="one dim")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_duplicate_rows(vdb, metric):
    V, Q, rows = mc.duplicates_case()
    ix = _index(vdb, V, metric)
    for lam in (0.0, 0.5, 1.0):
        _check(ix, V, Q, 10, 64, lam, metric, what="duplicates")
    s, i, ks, mm = _check(ix, V, Q, 5, 64, 1.0, metric, what="duplicates")
    np.testing.assert_array_equal(i, rows)  # equal keys in row order
    ix.close()


# =============================================================================
# properties
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_lambda_one_is_search(vdb, metric):
    V, Q = mc.corpus(700, 100)
    ix = _index(vdb, V, metric)
    mask = np.random.default_rng(2).random(700) < 0.5
    for k, fetch, m in ((10, 64, None), (64, 64, None), (1, 200, None), (10, 40, mask)):
        words = None if m is None else mc.bitmap_words(m)
        code, got = _call(ix, Q[:4], k, fetch, 1.0, words)
        assert code == 0
        s, i, ks = ix.search(Q[:4], k, row_mask=words, with_keys=True)
        _same(got[:3], (s, i, ks), f"lambda 1 against search, k {k} fetch {fetch}")
        _same((got[3],), (ks,), "mmr = rel at lambda 1")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_precisions_give_the_same_bytes(vdb, metric):
    V, Q = mc.corpus(700, 100)
    mask = np.random.default_rng(4).random(700) < 0.6
    want = mc.expected(Q[:3], V, 10, 64, 0.5, metric)
    want_m = mc.expected(Q[:3], V, 10, 64, 0.5, metric, mask)
    for prec in ("auto", "i8", "i8x3", "bf16", "bf16x3", "fp32"):
        ix = _index(vdb, V, metric, precision=prec)
        code, got = _call(ix, Q[:3], 10, 64, 0.5)
        assert code == 0, prec
        _same(got, want, f"precision {prec}")
        code, got = _call(ix, Q[:3], 10, 64, 0.5, mc.bitmap_words(mask))
        assert code == 0, prec
        _same(got, want_m, f"precision {prec}, masked")
        ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_device_memory(vdb, metric):
    import torch
    n, B, k, fetch = 700, 5, 10, 64
    V, Q = mc.corpus(n, 100)
    Q = Q[:B]
    ix = _index(vdb, V, metric)
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    mask = np.random.default_rng(3).random(n) < 0.7
    before = {s: ix.stat(s) for s in STATS}
    calls = 0
    for m, opt in ((None, True), (mask, True), (None, False)):
        words = None if m is None else mc.bitmap_words(m)
        code, host = _call(ix, Q, k, fetch, 0.5, words)
        assert code == 0
        with torch.cuda.stream(st):
            dq = torch.from_numpy(Q.copy()).to(dev)
            dm = torch.from_numpy(words.view(np.int32)).to(dev) if m is not None else None
            ds = torch.full((B * k + GUARD,), float("nan"), dtype=torch.float32, device=dev)
            di = torch.full((B * k + GUARD,), S_IDX, dtype=torch.int64, device=dev)
            dk = torch.full((B * k + GUARD,), float("nan"), dtype=torch.float64, device=dev)
            dmm = torch.full((B * k + GUARD,), float("nan"), dtype=torch.float64, device=dev)
            ix.search_mmr_device(dq.data_ptr(), B, k, fetch, 0.5, ds.data_ptr(), di.data_ptr(),
                                 dk.data_ptr() if opt else 0, dmm.data_ptr() if opt else 0,
                                 mask_ptr=dm.data_ptr() if dm is not None else 0, stream=st.cuda_stream)
        st.synchronize()
        calls += 2
        s, i, kk, mm = (x.cpu().numpy() for x in (ds, di, dk, dmm))
        got = [x[:B * k].reshape(B, k) for x in (s, i, kk, mm)]
        _same(got if opt else got[:2], host if opt else host[:2], "device against host memory")
        assert np.isnan(s[B * k:]).all() and (i[B * k:] == S_IDX).all()
        assert np.isnan(kk[B * k if opt else 0:]).all() and np.isnan(mm[B * k if opt else 0:]).all()
        _same(host, mc.expected(Q, V, k, fetch, 0.5, metric, m), "host against the oracle")
    after = {s: ix.stat(s) for s in STATS}
    assert [after[s] - before[s] for s in STATS] == [calls, calls * B, calls, calls * B]
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_index_offset_moves_the_ids_only(vdb, metric):
    V, Q = mc.corpus(65, 33)
    ix = _index(vdb, V, metric)
    off = 2 ** 40
    base = _check(ix, V, Q[:2], 70, 70, 0.5, metric)
    moved = _check(ix, V, Q[:2], 70, 70, 0.5, metric, index_offset=off)
    np.testing.assert_array_equal(moved[1], np.where(base[1] >= 0, base[1] + off, -1))
    _same((moved[0], None, moved[2], moved[3]), (base[0], None, base[2], base[3]))
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_optional_outputs(vdb, metric):
    V, Q = mc.corpus(300, 33)
    ix = _index(vdb, V, metric)
    want = mc.expected(Q[:3], V, 10, 20, 0.5, metric)
    for with_keys, with_mmr in ((False, False), (True, False), (False, True)):
        code, got = _call(ix, Q[:3], 10, 20, 0.5, with_keys=with_keys, with_mmr=with_mmr)
        assert code == 0
        assert (got[2] is None) == (not with_keys) and (got[3] is None) == (not with_mmr)
        _same(got, want, f"keys {with_keys} mmr {with_mmr}")
    # the binding returns what was asked for, in order
    s, i = ix.search_mmr(Q[:3], 10, 20, 0.5)
    s2, i2, mm = ix.search_mmr(Q[:3], 10, 20, 0.5, with_mmr=True)
    s3, i3, ks, mm3 = ix.search_mmr(Q[:3], 10, 20, 0.5, with_keys=True, with_mmr=True)
    _same((s, i, None, None), want)
    _same((s2, i2, None, mm), want)
    _same((s3, i3, ks, mm3), want)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_after_update_and_remove(vdb, metric):
    V, Q = mc.corpus(300, 100)
    ix = _index(vdb, V, metric)
    first = _check(ix, V, Q[:2], 10, 64, 0.5, metric)
    # the picked rows of query 0 become copies of one another: MMR must now avoid them
    V2 = V.copy()
    rows = first[1][0, :6]
    V2[rows] = V[rows[0]] + np.float32(0.001) * np.arange(6, dtype=np.float32)[:, None]
    assert ix.update(rows, V2[rows]) == 6
    second = _check(ix, V2, Q[:2], 10, 64, 0.5, metric, what="after update")
    assert (second[1][0] != first[1][0]).any()
    gone = np.concatenate([second[1][0, :3], [0, 299]])
    keep = np.setdiff1d(np.arange(300), gone)
    assert ix.remove(gone) == np.unique(gone).size
    _check(ix, V2[keep], Q[:2], 10, 64, 0.5, metric, what="after remove")
    ix.close()


# =============================================================================
# errors, stats, the empty index
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_errors_leave_the_stats_untouched(vdb, metric):
    V, Q = mc.corpus(300, 33)
    ix = _index(vdb, V, metric)
    assert _call(ix, Q[:2], 5, 20, 0.5)[0] == 0
    before = {s: ix.stat(s) for s in STATS}
    bad = [dict(k=0, fetch_k=10), dict(k=201, fetch_k=201), dict(k=10, fetch_k=9), dict(k=10, fetch_k=201),
           dict(k=5, fetch_k=20, lam=-0.1), dict(k=5, fetch_k=20, lam=1.1), dict(k=5, fetch_k=20, lam=float("nan")),
           dict(k=5, fetch_k=20, lam=float("inf")), dict(k=-1, fetch_k=-1)]
    for kw in bad:
        code, got = _call(ix, Q[:2], kw["k"], kw["fetch_k"], kw.get("lam", 0.5))
        assert code == VDB_ERR_INVALID, kw
        assert np.isnan(got[0]).all() and (got[1] == S_IDX).all(), f"outputs written on {kw}"
    assert _call(ix, Q[:2], 5, 20, 0.5, B=-1)[0] == VDB_ERR_INVALID
    # NULL pointers
    sc, idx = np.zeros(10, np.float32), np.zeros(10, np.int64)
    q = np.ascontiguousarray(Q[:2])
    f = ix._lib.vdb_index_search_mmr
    lam = ctypes.c_double(0.5)
    assert f(ix._h, None, 2, 5, 20, lam, None, 0, _p(sc), _p(idx), None, None, 0, None) == VDB_ERR_INVALID
    assert f(ix._h, _p(q), 2, 5, 20, lam, None, 0, None, _p(idx), None, None, 0, None) == VDB_ERR_INVALID
    assert f(ix._h, _p(q), 2, 5, 20, lam, None, 0, _p(sc), None, None, None, 0, None) == VDB_ERR_INVALID
    assert f(ix._h, _p(q), 2, 5, 20, lam, None, 7, _p(sc), _p(idx), None, None, 0, None) == VDB_ERR_INVALID
    # a NaN / Inf in a host query
    for v in (np.nan, np.inf):
        Qb = Q[:2].copy()
        Qb[1, 3] = v
        assert _call(ix, Qb, 5, 20, 0.5)[0] == VDB_ERR_NONFINITE
    # the binding raises ValueError with the limit in the message
    with pytest.raises(ValueError, match="200"):
        ix.search_mmr(Q[:2], 201, 201, 0.5)
    with pytest.raises(ValueError, match="fetch_k"):
        ix.search_mmr(Q[:2], 10, 5, 0.5)
    with pytest.raises(ValueError, match="lambda"):
        ix.search_mmr(Q[:2], 5, 20, 1.5)
    with pytest.raises(ValueError):
        ix.search_mmr(Q[:2, :5], 5, 20, 0.5)
    with pytest.raises(ValueError, match="row_mask"):
        ix.search_mmr(Q[:2], 5, 20, 0.5, row_mask=np.zeros(3, np.uint32))
    assert {s: ix.stat(s) for s in STATS} == before
    assert _call(ix, Q[:2], 5, 20, 0.5)[0] == 0  # and the index still answers
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_stats_no_queries_and_the_empty_index(vdb, metric):
    V, Q = mc.corpus(300, 33)
    ix = _index(vdb, V, metric)
    before = {s: ix.stat(s) for s in STATS}
    assert _call(ix, Q[:0], 5, 20, 0.5)[0] == 0  # n_queries == 0 is OK and counts nothing
    assert {s: ix.stat(s) for s in STATS} == before
    assert _call(ix, Q[:3], 5, 20, 0.5)[0] == 0
    assert _call(ix, Q[:1], 1, 1, 1.0)[0] == 0
    after = {s: ix.stat(s) for s in STATS}
    assert [after[s] - before[s] for s in STATS] == [2, 4, 2, 4]
    ix.close()
    # an empty index: every slot "no result", counted as a search
    empty = vdb.NativeIndex(33, metric)
    for m in (None, np.zeros(1, np.uint32)):
        code, (s, i, ks, mm) = _call(empty, Q[:3], 7, 20, 0.5, m)
        assert code == 0
        assert (s == 0).all() and (i == -1).all() and np.isneginf(ks).all() and np.isneginf(mm).all()
    assert _call(empty, Q[:3], 7, 20, 0.5, with_keys=False, with_mmr=False)[0] == 0
    assert [empty.stat(s) for s in STATS] == [3, 9, 3, 9]
    empty.close()

"""Weighted-sum hybrid search (include/vdb.h vdb_index_search_hybrid_sum; csrc/vdb_hybsum.hip).

The contract: row r of query b has the value ``c = (w_dense * kd + w_sparse * ks) + 0.0`` in fp64, kd
the canonical dense key and ks the sparse key; every row whose mask bit is set is a candidate and they
rank by (c desc, row asc); slots past min(k, candidates) hold 0 / -1 / -inf.  Every case compares every
output with the literal oracle of tests/_hybsum_cases.py (preconditions:
tests/test_hybsum_precondition.py) BIT FOR BIT: the fp64 values as uint64, the fp32 scores as uint32;
no tolerance appears anywhere.

``_check`` runs a case in host memory and in device memory.  Every output carries a guard region past
[n_queries][k] filled with a sentinel, which must be untouched afterwards.

Shapes are the smallest at which the kernel can go wrong: 3, 37, 513 and 1 300 rows (below a wave trip,
below a chunk, two chunks plus one row, more than four chunks), each with auto, 1, 2 and 7 workgroups
per query so that the merge tail and the idle segments run; 16, 260, 1 100 and 2 100 dims (the 4-piece,
the 8-piece and the any-length dense key; 260 is no multiple of 256); queries of 0, 1, 8 and 1 024
terms; k of 1, 10, 200 and 1 024.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hybsum_cases as hs  # noqa: E402

sp, fc = hs.sp, hs.fc
pytestmark = pytest.mark.gpu

GUARD = 257
S_IDX = -7
METRICS = hs.METRICS
VDB_ERR_INVALID = -1
VDB_ERR_NONFINITE = -4
STATS = ("searches", "queries", "sparse_searches", "sparse_queries", "sparse_bad_queries", "hybrid_searches",
         "hybrid_queries", "hybrid_sum_searches", "hybrid_sum_queries", "sparse_sets", "searches_fp32", "searches_bf16x3",
         "searches_bf16", "searches_i8", "searches_i8x3", "searches_i8q", "subset_searches")
NAMES = ("scores", "indices", "fused", "dense", "sparse")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    assert _vdb.VDB_ERR_INVALID == VDB_ERR_INVALID and _vdb.VDB_ERR_NONFINITE == VDB_ERR_NONFINITE
    return _vdb


def _index(vdb, V, metric="cosine", precision=None, col=None):
    V = np.asarray(V, np.float32)
    ix = vdb.NativeIndex(V.shape[1], metric, precision=precision)
    if V.shape[0]:
        ix.add(V)
    assert ix.count() == V.shape[0]
    if col is not None:
        ix.set_sparse(col.indptr, col.terms, col.weights, col.n_terms)
    return ix


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        if g is None or w is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} {what}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{name} {what}")


def _cut(want, k):
    """The expectation for a smaller k: the first k slots of the same ranking."""
    return tuple(np.ascontiguousarray(x[:, :k]) for x in want)


def _call(ix, Q, qs, k, weights=(1.0, 1.0), mask=None, index_offset=0, with_fused=True, with_parts=True, mem=0,
          n_queries=None, q_nnz=None, csr=None):
    """vdb_index_search_hybrid_sum in host memory with guarded outputs -> (rc, (scores, idx, fused, dense, sparse))."""
    ip, t, w = sp.pack(qs) if csr is None else csr
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    B = ip.size - 1 if n_queries is None else n_queries
    n = max(B, 0) * max(k, 0)
    sc = np.full(n + GUARD, np.nan, np.float32)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    fu = np.full(n + GUARD, np.nan, np.float64) if with_fused else None
    de = np.full(n + GUARD, np.nan, np.float64) if with_parts else None
    spk = np.full(n + GUARD, np.nan, np.float64) if with_parts else None
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    code = ix._lib.vdb_index_search_hybrid_sum(ix._h, _p(Q), _p(ip), _p(t), _p(w), B, t.size if q_nnz is None else q_nnz, k,
                                               ctypes.c_double(weights[0]), ctypes.c_double(weights[1]), _p(m), mem,
                                               _p(sc), _p(idx), _p(fu), _p(de), _p(spk), index_offset, None)
    assert np.isnan(sc[n:]).all() and (idx[n:] == S_IDX).all(), "guard touched"
    for x in (fu, de, spk):
        assert x is None or np.isnan(x[n:]).all(), "fp64 guard touched"
    shape = (max(B, 0), max(k, 0))
    return code, tuple(None if x is None else x[:n].reshape(shape) for x in (sc, idx, fu, de, spk))


def _dev(a, torch):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to("cuda")


def _call_device(ix, Q, qs, k, weights=(1.0, 1.0), mask=None, index_offset=0, with_parts=True, csr=None, q_nnz=None):
    """The same call with every argument in device memory on a side stream."""
    import torch
    ip, t, w = sp.pack(qs) if csr is None else csr
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    B = ip.size - 1
    n = B * k
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dq, dip, dt, dw = _dev(Q, torch), _dev(ip, torch), _dev(t, torch), _dev(w, torch)
        dm = _dev(mask, torch) if mask is not None else None
        ds = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        di = torch.full((n + GUARD,), S_IDX, dtype=torch.int64, device="cuda")
        df, dd, dp = (torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3))
        ix.search_hybrid_sum_device(dq.data_ptr(), dip.data_ptr(), dt.data_ptr() if t.size else 0,
                                    dw.data_ptr() if w.size else 0, B, t.size if q_nnz is None else q_nnz, k,
                                    ds.data_ptr(), di.data_ptr(), weights=weights, out_fused_ptr=df.data_ptr(),
                                    out_dense_ptr=dd.data_ptr() if with_parts else 0,
                                    out_sparse_ptr=dp.data_ptr() if with_parts else 0,
                                    mask_ptr=dm.data_ptr() if dm is not None else 0, index_offset=index_offset,
                                    stream=st.cuda_stream)
    st.synchronize()
    s, i, f, d, p = (x.cpu().numpy() for x in (ds, di, df, dd, dp))
    assert np.isnan(s[n:]).all() and (i[n:] == S_IDX).all() and np.isnan(f[n:]).all(), "guard touched (device)"
    assert np.isnan(d[n if with_parts else 0:]).all() and np.isnan(p[n if with_parts else 0:]).all(), "guard touched (device)"
    out = (s, i, f, d, p) if with_parts else (s, i, f)
    return tuple(x[:n].reshape(B, k) for x in out) + (() if with_parts else (None, None))


def _check(ix, V, Q, col, qs, k, metric, weights=(1.0, 1.0), mask=None, words=None, index_offset=0, what="", device=True,
           want=None):
    want = hs.expected(V, Q, col, qs, k, metric, weights, mask, index_offset) if want is None else want
    if words is None and mask is not None:
        words = fc.bitmap_words(mask)
    what = f"{what} ({metric}, k {k}, weights {weights})"
    code, got = _call(ix, Q, qs, k, weights, words, index_offset)
    assert code == 0, f"status {code} {what}: {ix._lib.vdb_last_error()}"
    _same(got, want, what + " host")
    # the parts recombine to the fused value: hybsum_combine's four operations
    valid = got[1] >= 0
    re = hs.combine(weights[0], got[3][valid], weights[1], got[4][valid])
    np.testing.assert_array_equal(_bits(re), _bits(got[2][valid]), err_msg=what + " recombined")
    if device:
        _same(_call_device(ix, Q, qs, k, weights, words, index_offset), want, what + " device")  # same bytes as host
    return got


# =============================================================================
# shapes
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", hs.ROWS)
def test_rows_workgroups_and_k(vdb, n, metric):
    V, Q = hs.dense_rows(n, sp.DIM)
    col = sp.column(n, 30522)
    qs = sp.queries(30522)  # 8, 0, 1, 1 024 and 8 terms
    ix = _index(vdb, V, metric, col=col)
    full = hs.expected(V, Q[:5], col, qs, 1024, metric, (1.0, 1.0))
    for wgs in (1, 2, 7, 0):
        ix.set_param("hybrid_sum_wgs", wgs)
        for k in (1, 10, 200, 1024):
            got = _check(ix, V, Q[:5], col, qs, k, metric, what=f"n {n} wgs {wgs}", device=wgs in (2, 0), want=_cut(full, k))
            assert ((got[1] >= 0).sum(axis=1) == min(k, n)).all()  # every row is a candidate, terms or none
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n", [(260, 513), (1100, 37), (2100, 300)])
def test_dims_take_the_three_key_paths(vdb, d, n, metric):
    V, Q = hs.dense_rows(n, d, seed=2)
    col = sp.column(n, 30522)
    qs = sp.queries(30522)[:3]
    mask = np.random.default_rng(d).random(n) < 0.5
    ix = _index(vdb, V, metric, col=col)
    full = hs.expected(V, Q[:3], col, qs, 64, metric, (1.0, 1.0))
    full_m = hs.expected(V, Q[:3], col, qs, 64, metric, (0.3, 0.7), mask)
    for wgs in (0, 2):
        ix.set_param("hybrid_sum_wgs", wgs)
        _check(ix, V, Q[:3], col, qs, 64, metric, what=f"dim {d} wgs {wgs}", want=full, device=wgs == 2)
        _check(ix, V, Q[:3], col, qs, 10, metric, (0.3, 0.7), mask, what=f"dim {d} wgs {wgs} masked", want=_cut(full_m, 10),
               device=wgs == 0)
    ix.close()


@pytest.mark.parametrize("n_terms", sp.VOCABS)
def test_vocabularies_and_query_lengths(vdb, n_terms):
    n = 513
    V, Q = hs.dense_rows(n, sp.DIM, seed=1)
    col = sp.column(n, n_terms)
    qs = sp.queries(n_terms)
    assert [t.size for t, _ in qs] == [min(L, n_terms) for L in (8, 0, 1, 1024, 8)]
    ix = _index(vdb, V, col=col)
    ix.set_param("hybrid_sum_wgs", 2)
    for k in (10, 600):
        _check(ix, V, Q[:5], col, qs, k, "cosine", (0.3, 0.7), what=f"vocabulary {n_terms}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_weights(vdb, metric):
    n = 513
    V, Q = hs.dense_rows(n, sp.DIM, seed=3)
    col = sp.column(n, 30522, "signed")
    qs = sp.queries(30522, "signed")
    ix = _index(vdb, V, metric, col=col)
    for weights in hs.WEIGHTS:
        got = _check(ix, V, Q[:5], col, qs, 40, metric, weights, what="weights")
        assert np.isfinite(got[2]).all()
        if weights == (0.0, 0.0):  # every value +0.0: the rows in id order
            assert (got[1] == np.arange(40)).all() and (_bits(got[2]) == 0).all()
    ix.close()


def test_masks_offset_and_optional_outputs(vdb):
    n = 300
    V, Q = hs.dense_rows(n, sp.DIM, seed=4)
    col = sp.column(n, 30522)
    qs = sp.queries(30522)
    ix = _index(vdb, V, col=col)
    half = np.random.default_rng(6).random(n) < 0.5
    one = np.zeros(n, bool)
    one[257] = True
    for wgs in (0, 2):
        ix.set_param("hybrid_sum_wgs", wgs)
        _check(ix, V, Q[:5], col, qs, 10, "cosine", mask=half, what="half")
        got = _check(ix, V, Q[:5], col, qs, 10, "cosine", mask=one, what="one row")
        assert (got[1][:, 0] == 257).all() and (got[1][:, 1:] == -1).all()
        got = _check(ix, V, Q[:5], col, qs, 10, "cosine", mask=np.zeros(n, bool), what="no eligible row")
        assert (got[1] == -1).all() and (got[0] == 0).all() and all(np.isneginf(x).all() for x in got[2:])
    words = fc.bitmap_words(half, extra_bits=52)  # bits at or past count name no row
    _check(ix, V, Q[:5], col, qs, 200, "cosine", mask=half, words=words, what="mask bits past count")
    off = 2 ** 40
    base = _check(ix, V, Q[:5], col, qs, 400, "cosine", what="offset 0")
    moved = _check(ix, V, Q[:5], col, qs, 400, "cosine", index_offset=off, what="offset 2^40")
    np.testing.assert_array_equal(moved[1], np.where(base[1] >= 0, base[1] + off, -1))
    # the optional outputs, and the binding
    want = hs.expected(V, Q[:5], col, qs, 7, "cosine", (1.0, 1.0))
    code, got = _call(ix, Q[:5], qs, 7, with_fused=False, with_parts=False)
    assert code == 0 and got[2] is None and got[3] is None and got[4] is None
    _same(got, want, "two outputs")
    code, got = _call(ix, Q[:5], qs, 7, with_fused=True, with_parts=False)
    assert code == 0
    _same(got, want, "without parts")
    _same(_call_device(ix, Q[:5], qs, 7, with_parts=False), want, "without parts, device")
    ip, t, w = sp.pack(qs)
    _same(ix.search_hybrid_sum(Q[:5], ip, t, w, 7, with_fused=True, with_parts=True), want, "binding")
    _same(ix.search_hybrid_sum(Q[:5], ip, t, w, 7), want[:2], "binding, two outputs")
    got = ix.search_hybrid_sum(Q[:5], ip, t, w, 7, weights=(0.3, 0.7), row_mask=fc.bitmap_words(half), with_parts=True)
    wm = hs.expected(V, Q[:5], col, qs, 7, "cosine", (0.3, 0.7), half)
    _same(got, (wm[0], wm[1], wm[3], wm[4]), "binding, masked, parts without fused")
    assert vdb.HYBRID_SUM_MAX_K == hs.MAX_K
    ix.close()


# =============================================================================
# the named cases
# =============================================================================
def test_the_planted_row_between_the_two_rankings_wins(vdb):
    V, Q, col, qs, planted = hs.between_case()
    ix = _index(vdb, V, col=col)
    for wgs in (0, 1):
        ix.set_param("hybrid_sum_wgs", wgs)
        got = _check(ix, V, Q, col, qs, 10, "cosine", what=f"between wgs {wgs}")
        assert got[1][0, 0] == planted
    s, i = ix.search_hybrid(Q, *sp.pack(qs), 10, 200)  # the RRF of two fetched lists of 200 misses it
    assert planted not in i[0].tolist()
    ix.close()


def test_ties_go_to_the_lower_row(vdb):
    V, Q, col, qs = hs.tie_case()
    ix = _index(vdb, V, col=col)
    for wgs in (1, 7):
        ix.set_param("hybrid_sum_wgs", wgs)
        for k in (10, 11, 100, 1024):
            _check(ix, V, Q, col, qs, k, "cosine", what=f"ties wgs {wgs}", device=wgs == 7)
    ix.close()


def test_signed_keys_and_the_copy_of_the_query(vdb):
    V, Q, col, qs, copy = hs.signed_case()
    ix = _index(vdb, V, "euclidean", col=col)
    for wgs in (1, 2):
        ix.set_param("hybrid_sum_wgs", wgs)
        s, i, f, d, p = _check(ix, V, Q, col, qs, 1024, "euclidean", what=f"signed wgs {wgs}")
        at = i[0].tolist().index(copy)
        assert _bits(f[0, at:at + 1])[0] == 0 and np.signbit(d[0, at]) and d[0, at] == 0  # kd -0.0, c +0.0
        assert ((f < 0) & (i >= 0)).any() and (i[0] >= 0).sum() == 513
        _check(ix, V, Q, col, qs, 10, "euclidean", what=f"signed wgs {wgs}")
    ix.close()


def test_k_beyond_the_eligible_rows(vdb):
    V, Q, col, qs, mask, k = hs.short_case()
    ix = _index(vdb, V, col=col)
    s, i, f, d, p = _check(ix, V, Q, col, qs, k, "cosine", mask=mask, what="short")
    e = i == -1
    assert (e.sum(axis=1) == k - mask.sum()).all() and (s[e] == 0).all()
    assert np.isneginf(f[e]).all() and np.isneginf(d[e]).all() and np.isneginf(p[e]).all()
    ix.close()
    V3, Q3 = hs.dense_rows(3, sp.DIM)
    col3 = sp.column(3, 30522)
    ix = _index(vdb, V3, col=col3)
    _check(ix, V3, Q3[:5], col3, qs, 1024, "cosine", what="three rows, k 1 024")
    ix.close()


# =============================================================================
# identities, on the device
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_identities_against_search_and_search_sparse(vdb, metric):
    n = 1300
    V, Q = hs.dense_rows(n, sp.DIM, seed=6)
    col = sp.column(n, 30522)
    qs = sp.queries(30522)
    ip, t, w = sp.pack(qs)
    half = np.random.default_rng(9).random(n) < 0.5
    ix = _index(vdb, V, metric, col=col)
    for mask in (None, fc.bitmap_words(half)):
        # (1, 0): the dense search's rows in its order, fused = its keys + 0.0
        code, got = _call(ix, Q[:5], qs, 50, (1.0, 0.0), mask)
        assert code == 0
        ds, di, dk = ix.search(Q[:5], 50, row_mask=mask, with_keys=True)
        np.testing.assert_array_equal(got[1], di)
        np.testing.assert_array_equal(_bits(got[2]), _bits(dk + 0.0))
        np.testing.assert_array_equal(_bits(got[3]), _bits(dk))
        # (0, 1): the leading slots with out_sparse > 0 are the sparse search's leading slots with keys > 0
        code, got = _call(ix, Q[:5], qs, 50, (0.0, 1.0), mask)
        assert code == 0
        ss, si, sk = ix.search_sparse(ip, t, w, 50, row_mask=mask, with_keys=True)
        leads = []
        for b in range(5):
            lead = int(np.argmin(got[4][b] > 0)) if not (got[4][b] > 0).all() else 50
            slead = int(np.argmin(sk[b] > 0)) if not (sk[b] > 0).all() else 50
            assert lead == slead, b
            np.testing.assert_array_equal(got[1][b, :lead], si[b, :lead])
            np.testing.assert_array_equal(_bits(got[2][b, :lead]), _bits(sk[b, :lead]))
            leads.append(lead)
        assert max(leads) >= 10  # the identity is not vacuous
    # a query without terms ranks by its dense key alone; the result of a query depends only on that query
    code, alone = _call(ix, Q[1:2], qs[1:2], 20)
    code2, batch = _call(ix, Q[:5], qs, 20)
    assert code == 0 and code2 == 0 and qs[1][0].size == 0
    _same(alone, tuple(x[1:2] for x in batch), "one query alone and in a batch")
    np.testing.assert_array_equal(alone[1], ix.search(Q[1:2], 20)[1])
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_precisions_and_force_exact_give_the_same_bytes(vdb, metric):
    n = 513
    V, Q = hs.dense_rows(n, sp.DIM, seed=7)
    col = sp.column(n, 30522)
    qs = sp.queries(30522)
    mask = np.random.default_rng(3).random(n) < 0.5
    want, want_m = hs.expected(V, Q[:5], col, qs, 50, metric, (0.3, 0.7)), hs.expected(V, Q[:5], col, qs, 50, metric, (0.3, 0.7), mask)
    for prec, force in [(p, 0) for p in ("fp32", "bf16x3", "i8", "auto")] + [("auto", 1)]:
        ix = _index(vdb, V, metric, precision=prec, col=col)
        if force:
            ix.set_param("force_exact", 1)
        before = {s: ix.stat(s) for s in STATS}
        _check(ix, V, Q[:5], col, qs, 50, metric, (0.3, 0.7), what=f"{prec} force {force}", want=want)
        _check(ix, V, Q[:5], col, qs, 50, metric, (0.3, 0.7), mask, what=f"{prec} force {force} masked", want=want_m)
        after = {s: ix.stat(s) for s in STATS}
        moved = {s: after[s] - before[s] for s in STATS if after[s] != before[s]}
        assert moved == {"hybrid_sum_searches": 4, "hybrid_sum_queries": 20}, moved  # no other stat moves
        ix.close()


def test_two_calls_back_to_back_leave_the_counters_zero(vdb):
    n = 1300
    V, Q = hs.dense_rows(n, sp.DIM, seed=8)
    col = sp.column(n, 30522)
    qs = sp.queries(30522)
    ix = _index(vdb, V, col=col)
    ix.set_param("hybrid_sum_wgs", 3)
    want = hs.expected(V, Q[:5], col, qs, 10, "cosine", (1.0, 1.0))
    for j in range(3):  # the same workspace: a counter left non-zero would end the second call's merge early
        code, got = _call(ix, Q[:5], qs, 10)
        assert code == 0
        _same(got, want, f"call {j}")
    ix.close()


# =============================================================================
# errors, bad device input, the empty index, stats
# =============================================================================
def test_errors_leave_the_stats_and_the_outputs_untouched(vdb):
    n = 37
    V, Q = hs.dense_rows(n, sp.DIM)
    col = sp.column(n, 30522)
    qs = sp.queries(30522)
    ix = _index(vdb, V, col=col)
    assert _call(ix, Q[:5], qs, 5)[0] == 0
    before = {s: ix.stat(s) for s in STATS}
    ip, t, w = sp.pack(qs)
    big = 2.0 ** 64
    for kw in (dict(k=0), dict(k=1025), dict(k=-1), dict(mem=7), dict(n_queries=-1), dict(q_nnz=-1), dict(n_queries=65536),
               dict(weights=(-1.0, 1.0)), dict(weights=(1.0, np.nan)), dict(weights=(np.inf, 1.0)),
               dict(weights=(1.0, np.nextafter(big, np.inf))), dict(weights=(-0.5, 0.0))):
        for mem in (0, 1):  # both memory kinds, before anything is launched (mem 1: the pointers are never read)
            a = dict(k=5, mem=mem)
            a.update(kw)
            code, got = _call(ix, Q[:5], qs, a.pop("k"), **a)
            assert code == VDB_ERR_INVALID, (kw, mem)
            assert np.isnan(got[0]).all() and (got[1] == S_IDX).all(), f"outputs written on {kw}"
    long_t = np.arange(1025, dtype=np.int32)
    bad = [
        ("decreasing offsets", (np.asarray([0, 3, 2], np.int64), t[:3], w[:3]), VDB_ERR_INVALID),
        ("offsets past q_nnz", (np.asarray([0, 2, 4], np.int64), t[:3], w[:3]), VDB_ERR_INVALID),
        ("a negative offset", (np.asarray([-1, 2, 3], np.int64), t[:3], w[:3]), VDB_ERR_INVALID),
        ("1 025 terms", (np.asarray([0, 1025], np.int64), long_t, np.ones(1025, np.float32)), VDB_ERR_INVALID),
        ("a term out of range", (np.asarray([0, 2], np.int64), np.asarray([3, 30522], np.int32), np.ones(2, np.float32)), VDB_ERR_INVALID),
        ("a negative term", (np.asarray([0, 2], np.int64), np.asarray([-3, 5], np.int32), np.ones(2, np.float32)), VDB_ERR_INVALID),
        ("a repeated term", (np.asarray([0, 2], np.int64), np.asarray([5, 5], np.int32), np.ones(2, np.float32)), VDB_ERR_INVALID),
        ("a NaN weight", (np.asarray([0, 2], np.int64), np.asarray([3, 5], np.int32), np.asarray([1, np.nan], np.float32)), VDB_ERR_NONFINITE),
        ("an Inf weight", (np.asarray([0, 2], np.int64), np.asarray([3, 5], np.int32), np.asarray([-np.inf, 1], np.float32)), VDB_ERR_NONFINITE),
    ]
    for name, csr, err in bad:
        code, got = _call(ix, Q[:csr[0].size - 1], None, 5, csr=csr)
        assert code == err, name
        assert np.isnan(got[0]).all() and (got[1] == S_IDX).all(), f"outputs written on {name}"
    for v in (np.nan, np.inf):
        Qb = Q[:5].copy()
        Qb[2, 1] = v
        assert _call(ix, Qb, qs, 5)[0] == VDB_ERR_NONFINITE
    # NULL pointers
    sc, idx = np.zeros(25, np.float32), np.zeros(25, np.int64)
    Q5 = np.ascontiguousarray(Q[:5])
    f = ix._lib.vdb_index_search_hybrid_sum
    one = ctypes.c_double(1.0)
    for mem in (0, 1):
        assert f(ix._h, None, _p(ip), _p(t), _p(w), 5, t.size, 5, one, one, None, mem, _p(sc), _p(idx), None, None, None, 0, None) == VDB_ERR_INVALID
        assert f(ix._h, _p(Q5), None, _p(t), _p(w), 5, t.size, 5, one, one, None, mem, _p(sc), _p(idx), None, None, None, 0, None) == VDB_ERR_INVALID
        assert f(ix._h, _p(Q5), _p(ip), None, _p(w), 5, t.size, 5, one, one, None, mem, _p(sc), _p(idx), None, None, None, 0, None) == VDB_ERR_INVALID
        assert f(ix._h, _p(Q5), _p(ip), _p(t), _p(w), 5, t.size, 5, one, one, None, mem, None, _p(idx), None, None, None, 0, None) == VDB_ERR_INVALID
        assert f(ix._h, _p(Q5), _p(ip), _p(t), _p(w), 5, t.size, 5, one, one, None, mem, _p(sc), None, None, None, None, 0, None) == VDB_ERR_INVALID
    with pytest.raises(ValueError, match="1024"):
        ix.search_hybrid_sum(Q[:5], ip, t, w, 1025)
    with pytest.raises(ValueError, match="2\\^64"):
        ix.search_hybrid_sum(Q[:5], ip, t, w, 5, weights=(-1.0, 1.0))
    with pytest.raises(ValueError, match="row_mask"):
        ix.search_hybrid_sum(Q[:5], ip, t, w, 5, row_mask=np.zeros(1, np.uint32))
    with pytest.raises(ValueError, match="sparse ones"):
        ix.search_hybrid_sum(Q[:4], ip, t, w, 5)
    with pytest.raises(ValueError):
        ix.set_param("hybrid_sum_wgs", 513)
    with pytest.raises(ValueError):
        ix.set_param("hybrid_sum_wgs", -1)
    assert {s: ix.stat(s) for s in STATS} == before
    # what is no error: no queries; the largest weights
    assert _call(ix, Q[:0], [], 5)[0] == 0
    assert {s: ix.stat(s) for s in STATS} == before
    assert _call(ix, Q[:5], qs, 5, weights=(big, big))[0] == 0
    ix.close()
    # no column attached
    ix = _index(vdb, V)
    assert _call(ix, Q[:5], qs, 5)[0] == VDB_ERR_INVALID and _call(ix, Q[:5], qs, 5, mem=1)[0] == VDB_ERR_INVALID
    ix.close()


def _garbage(qs, n_terms):
    """Five good queries with bad ones between them -> (csr, q_nnz, the bad queries' numbers, the good
    queries by number)."""
    g = {0: qs[0], 2: qs[2], 4: qs[3], 6: qs[4], 8: qs[1]}
    bad_term = (np.asarray([3, n_terms], np.int32), np.ones(2, np.float32))       # a term out of range
    nan_w = (np.asarray([3, 9], np.int32), np.asarray([1.0, np.nan], np.float32))  # a NaN weight
    unsorted = (np.asarray([9, 3], np.int32), np.ones(2, np.float32))             # not ascending
    long_q = (np.arange(1025, dtype=np.int32), np.ones(1025, np.float32))         # 1 025 terms
    parts = [g[0], bad_term, g[2], nan_w, g[4], unsorted, g[6], long_q, g[8]]
    ip, t, w = sp.pack(parts)
    # two more queries whose offsets lie outside [0, q_nnz]: 9 = [nnz, nnz + 50), 10 = [nnz + 50, -4)
    nnz = int(ip[-1])
    ip = np.concatenate([ip, [nnz + 50, -4]]).astype(np.int64)
    return (ip, t, w), nnz, {1, 3, 5, 7, 9, 10}, g


def test_device_memory_garbage_is_answered_per_query(vdb):
    import torch
    n = 513
    V, Q11 = hs.dense_rows(n, sp.DIM, seed=1, n_queries=11)
    col = sp.column(n, 30522)
    qs = sp.queries(30522)
    ix = _index(vdb, V, col=col)
    csr, nnz, bad, good = _garbage(qs, 30522)
    empty = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    want = hs.expected(V, Q11, col, [good.get(b, empty) for b in range(11)], 10, "cosine", (1.0, 1.0), bad=bad)
    for wgs in (1, 2):
        ix.set_param("hybrid_sum_wgs", wgs)
        before = ix.stat("sparse_bad_queries")
        got = _call_device(ix, Q11, None, 10, csr=csr, q_nnz=nnz)
        torch.cuda.synchronize()
        assert ix.stat("sparse_bad_queries") - before == len(bad)
        _same(got, want, f"good queries beside bad ones, wgs {wgs}")
        for b in sorted(bad):
            assert (got[1][b] == -1).all() and (got[0][b] == 0).all() and all(np.isneginf(x[b]).all() for x in got[2:]), b
    # no HIP error afterwards: the device and the index still answer
    _check(ix, V, Q11[:5], col, qs, 10, "cosine", what="after the bad input")
    ix.close()


def test_the_empty_index(vdb):
    ix = vdb.NativeIndex(sp.DIM, "cosine")
    _, Q = hs.dense_rows(3, sp.DIM)
    q7 = sp.queries(5)
    assert _call(ix, Q[:5], q7, 3)[0] == VDB_ERR_INVALID  # no column
    ix.set_sparse(np.zeros(1, np.int64), None, None, 7)
    code, got = _call(ix, Q[:5], q7, 3)
    assert code == 0
    for g in (got, _call_device(ix, Q[:5], q7, 3)):
        assert (g[1] == -1).all() and (g[0] == 0).all() and all(np.isneginf(x).all() for x in g[2:])
    assert (ix.stat("hybrid_sum_searches"), ix.stat("hybrid_sum_queries")) == (2, 10)
    ix.close()


def test_stats_move_once_per_call(vdb):
    n = 37
    V, Q = hs.dense_rows(n, sp.DIM)
    col = sp.column(n, 30522)
    qs = sp.queries(30522)
    ix = _index(vdb, V, col=col)
    before = {s: ix.stat(s) for s in STATS}
    assert _call(ix, Q[:5], qs, 5)[0] == 0
    _call_device(ix, Q[:2], qs[:2], 5)
    after = {s: ix.stat(s) for s in STATS}
    moved = {s: after[s] - before[s] for s in STATS if after[s] != before[s]}
    assert moved == {"hybrid_sum_searches": 2, "hybrid_sum_queries": 7}, moved
    ix.close()

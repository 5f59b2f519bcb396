"""Sparse and hybrid search (include/vdb.h vdb_index_set_sparse, vdb_index_search_sparse,
vdb_index_search_hybrid; csrc/vdb_sparse.hip).

The contract: a row's key is the fp64 dot product of its sparse vector with the query's, summed over
the row's entries in stored order; the rows that match rank by (key desc, row asc); slots past min(k,
matches) hold 0 / -1 / -inf.  The hybrid call fuses that list with the dense search's by weighted
reciprocal rank.  Every case compares every output with the literal oracle of tests/_sparse_cases.py
(preconditions: tests/test_sparse_precondition.py) BIT FOR BIT: the fp64 values as uint64, the fp32
scores as uint32; no tolerance appears anywhere.

``_check`` runs a case in host memory and in device memory.  Every output carries a guard region past
[n_queries][k] filled with a sentinel, which must be untouched afterwards.

Shapes are the smallest at which the kernel can go wrong: 3, 37, 513 and 1 300 rows (below a wave trip,
across a wave trip and a workgroup trip, several chunks), each with 1, 2 and 7 workgroups per query so
that the merge tail runs; rows of 0, 1, 63, 64, 65 and 300 entries; vocabularies of 5, 30 522 and 2^31 -
1; queries of 0, 1 and 1 024 terms; k of 1, 10 and 1 024.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sparse_cases as sp  # noqa: E402

fc = sp.fc
pytestmark = pytest.mark.gpu

GUARD = 257
S_IDX = -7
S_HIT = -9
METRICS = sp.METRICS
VDB_ERR_INVALID = -1
VDB_ERR_NONFINITE = -4
STATS = ("searches", "queries", "sparse_searches", "sparse_queries", "sparse_bad_queries", "hybrid_searches",
         "hybrid_queries", "sparse_sets", "searches_fp32", "searches_bf16", "searches_i8")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    assert _vdb.VDB_ERR_INVALID == VDB_ERR_INVALID and _vdb.VDB_ERR_NONFINITE == VDB_ERR_NONFINITE
    return _vdb


def _index(vdb, n, metric="cosine", precision=None, col=None, seed=0):
    V, Q = sp.dense_rows(n, seed)
    ix = vdb.NativeIndex(sp.DIM, metric, precision=precision)
    if n:
        ix.add(V)
    assert ix.count() == n
    if col is not None:
        ix.set_sparse(col.indptr, col.terms, col.weights, col.n_terms)
    return ix, V, Q


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what=""):
    for name, g, w in zip(("scores", "indices", "keys/fused", "hits"), got, want):
        if g is None or w is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} {what}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{name} {what}")


def _call(ix, qs, k, mask=None, index_offset=0, with_keys=True, mem=0, n_queries=None, q_nnz=None, csr=None):
    """vdb_index_search_sparse in host memory with guarded outputs -> (rc, (scores, idx, keys))."""
    ip, t, w = sp.pack(qs) if csr is None else csr
    B = ip.size - 1 if n_queries is None else n_queries
    n = max(B, 0) * max(k, 0)
    sc = np.full(n + GUARD, np.nan, np.float32)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    ke = np.full(n + GUARD, np.nan, np.float64) if with_keys else None
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    code = ix._lib.vdb_index_search_sparse(ix._h, _p(ip), _p(t), _p(w), B, t.size if q_nnz is None else q_nnz, k, _p(m), mem,
                                           _p(sc), _p(idx), _p(ke), index_offset, None)
    assert np.isnan(sc[n:]).all(), "scores guard touched"
    assert (idx[n:] == S_IDX).all(), "indices guard touched"
    assert ke is None or np.isnan(ke[n:]).all(), "keys guard touched"
    shape = (max(B, 0), max(k, 0))
    return code, (sc[:n].reshape(shape), idx[:n].reshape(shape), None if ke is None else ke[:n].reshape(shape))


def _dev(a, torch, dtype=None):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a.copy()).to("cuda")
    return t


def _call_device(ix, qs, k, mask=None, index_offset=0, with_keys=True, csr=None, q_nnz=None):
    """The same call with every argument in device memory on a side stream -> (scores, idx, keys)."""
    import torch
    ip, t, w = sp.pack(qs) if csr is None else csr
    B = ip.size - 1
    n = B * k
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dip, dt, dw = _dev(ip, torch), _dev(t, torch), _dev(w, torch)
        dm = _dev(mask, torch) if mask is not None else None
        ds = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        di = torch.full((n + GUARD,), S_IDX, dtype=torch.int64, device="cuda")
        dk = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        ix.search_sparse_device(dip.data_ptr(), dt.data_ptr() if t.size else 0, dw.data_ptr() if w.size else 0, B,
                                t.size if q_nnz is None else q_nnz, k, ds.data_ptr(), di.data_ptr(),
                                out_keys_ptr=dk.data_ptr() if with_keys else 0,
                                mask_ptr=dm.data_ptr() if dm is not None else 0, index_offset=index_offset,
                                stream=st.cuda_stream)
    st.synchronize()
    s, i, kk = (x.cpu().numpy() for x in (ds, di, dk))
    assert np.isnan(s[n:]).all() and (i[n:] == S_IDX).all() and np.isnan(kk[n if with_keys else 0:]).all(), "guard touched (device)"
    return s[:n].reshape(B, k), i[:n].reshape(B, k), kk[:n].reshape(B, k) if with_keys else None


def _check(ix, col, qs, k, mask=None, words=None, index_offset=0, what="", device=True, want=None):
    want = sp.expected(col, qs, k, mask, index_offset) if want is None else want
    if words is None and mask is not None:
        words = fc.bitmap_words(mask)
    what = f"{what} (k {k})"
    code, got = _call(ix, qs, k, words, index_offset)
    assert code == 0, f"status {code} {what}: {ix._lib.vdb_last_error()}"
    _same(got, want, what + " host")
    if device:
        _same(_call_device(ix, qs, k, words, index_offset), want, what + " device")
    return got


def _call_hybrid(ix, Q, qs, k, fetch_k, weights=(1.0, 1.0), rrf_c=fc.RRF_C, mask=None, index_offset=0, with_fused=True,
                 with_hits=True, mem=0, csr=None):
    ip, t, w = sp.pack(qs) if csr is None else csr
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    B = ip.size - 1
    n = max(B, 0) * max(k, 0)
    sc = np.full(n + GUARD, np.nan, np.float32)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    fu = np.full(n + GUARD, np.nan, np.float64) if with_fused else None
    hi = np.full(n + GUARD, S_HIT, np.int32) if with_hits else None
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    code = ix._lib.vdb_index_search_hybrid(ix._h, _p(Q), _p(ip), _p(t), _p(w), B, t.size, k, fetch_k,
                                           ctypes.c_double(weights[0]), ctypes.c_double(weights[1]), ctypes.c_double(rrf_c),
                                           _p(m), mem, _p(sc), _p(idx), _p(fu), _p(hi), index_offset, None)
    assert np.isnan(sc[n:]).all() and (idx[n:] == S_IDX).all(), "guard touched"
    assert fu is None or np.isnan(fu[n:]).all(), "fused guard touched"
    assert hi is None or (hi[n:] == S_HIT).all(), "hits guard touched"
    shape = (max(B, 0), max(k, 0))
    return code, (sc[:n].reshape(shape), idx[:n].reshape(shape), None if fu is None else fu[:n].reshape(shape),
                  None if hi is None else hi[:n].reshape(shape))


def _call_hybrid_device(ix, Q, qs, k, fetch_k, weights=(1.0, 1.0), rrf_c=fc.RRF_C, mask=None, index_offset=0, csr=None):
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
        df = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        dh = torch.full((n + GUARD,), S_HIT, dtype=torch.int32, device="cuda")
        ix.search_hybrid_device(dq.data_ptr(), dip.data_ptr(), dt.data_ptr() if t.size else 0,
                                dw.data_ptr() if w.size else 0, B, t.size, k, fetch_k, ds.data_ptr(), di.data_ptr(),
                                weights=weights, rrf_c=rrf_c, out_fused_ptr=df.data_ptr(), out_hits_ptr=dh.data_ptr(),
                                mask_ptr=dm.data_ptr() if dm is not None else 0, index_offset=index_offset,
                                stream=st.cuda_stream)
    st.synchronize()
    s, i, f, h = (x.cpu().numpy() for x in (ds, di, df, dh))
    assert np.isnan(s[n:]).all() and (i[n:] == S_IDX).all() and np.isnan(f[n:]).all() and (h[n:] == S_HIT).all(), "guard"
    return s[:n].reshape(B, k), i[:n].reshape(B, k), f[:n].reshape(B, k), h[:n].reshape(B, k)


# =============================================================================
# sparse search: the cases
# =============================================================================
@pytest.mark.parametrize("n", sp.ROWS)
def test_rows_workgroups_and_k(vdb, n):
    col = sp.column(n, 30522)
    qs = sp.queries(30522)
    ix, V, Q = _index(vdb, n, col=col)
    wants = {k: sp.expected(col, qs, k) for k in (1, 10, 1024)}
    for wgs in (1, 2, 7, 0):
        ix.set_param("sparse_wgs", wgs)
        for k in (1, 10, 1024):
            got = _check(ix, col, qs, k, what=f"n {n} wgs {wgs}", device=wgs in (2, 0), want=wants[k])
            assert (got[1][1] == -1).all()  # the query without terms
    if n >= 513:
        assert (wants[1024][1][3] >= 0).sum() > 256  # the 1 024-term query fills more than one segment's share
    ix.close()


@pytest.mark.parametrize("n_terms", sp.VOCABS)
def test_vocabularies_and_edge_terms(vdb, n_terms):
    col = sp.column(513, n_terms)
    qs = sp.queries(n_terms)
    ix, V, Q = _index(vdb, 513, col=col)
    ix.set_param("sparse_wgs", 2)
    mask = np.random.default_rng(8).random(513) < 0.5
    for k in (1, 10, 600):
        _check(ix, col, qs, k, what=f"vocabulary {n_terms}")
        _check(ix, col, qs, k, mask=mask, what=f"vocabulary {n_terms} masked")
    ix.close()
    col, qs = sp.edge_terms_case(n_terms)
    ix, V, Q = _index(vdb, col.n, col=col)
    _check(ix, col, qs, 4, what=f"terms 0 and {n_terms - 1}")
    ix.close()


def test_ties_go_to_the_lower_row(vdb):
    col, qs = sp.tie_case()
    ix, V, Q = _index(vdb, col.n, col=col)
    for wgs in (1, 7):
        ix.set_param("sparse_wgs", wgs)
        for k in (10, 11, 100, 1024):
            _check(ix, col, qs, k, what=f"ties wgs {wgs}", device=wgs == 7)
    ix.close()


def test_keys_of_zero_and_below_rank_and_unmatched_rows_never_return(vdb):
    col, qs = sp.signed_case()
    ix, V, Q = _index(vdb, col.n, col=col)
    for wgs in (1, 2):
        ix.set_param("sparse_wgs", wgs)
        s, i, k = _check(ix, col, qs, 1024, what=f"signed wgs {wgs}")
        assert ((k <= 0) & (i >= 0)).any()
        _check(ix, col, qs, 10, what=f"signed wgs {wgs}")
    ix.close()
    col, qs = sp.zero_key_case()
    ix, V, Q = _index(vdb, col.n, col=col)
    s, i, k = _check(ix, col, qs, 5, what="zero key")
    assert i[0].tolist() == [0, 1, 2, -1, -1]
    ix.close()


def test_k_beyond_the_matches_mask_words_and_offset(vdb):
    col, qs = sp.beyond_case()
    ix, V, Q = _index(vdb, col.n, col=col)
    s, i, k = _check(ix, col, qs, 10, what="beyond")
    assert (i[0] == -1).any() and (i[0] >= 0).any() and (s[0][i[0] == -1] == 0).all() and np.isneginf(k[0][i[0] == -1]).all()
    ix.close()
    col = sp.column(300, 30522)
    qs = sp.queries(30522)
    ix, V, Q = _index(vdb, 300, col=col)
    half = np.random.default_rng(6).random(300) < 0.5
    _check(ix, col, qs, 10, mask=np.zeros(300, bool), what="no eligible row")
    words = fc.bitmap_words(half, extra_bits=52)  # bits at or past count name no row
    _check(ix, col, qs, 400, mask=half, words=words, what="mask bits past count")
    off = 2 ** 40
    base = _check(ix, col, qs, 400, what="offset 0")
    moved = _check(ix, col, qs, 400, index_offset=off, what="offset 2^40")
    np.testing.assert_array_equal(moved[1], np.where(base[1] >= 0, base[1] + off, -1))
    # the optional output, and the binding
    code, got = _call(ix, qs, 7, with_keys=False)
    assert code == 0 and got[2] is None
    _same(got, sp.expected(col, qs, 7), "without keys")
    _same(_call_device(ix, qs, 7, with_keys=False), sp.expected(col, qs, 7), "without keys, device")
    ip, t, w = sp.pack(qs)
    _same(ix.search_sparse(ip, t, w, 7, with_keys=True), sp.expected(col, qs, 7), "binding")
    _same(ix.search_sparse(ip, t, w, 7, row_mask=fc.bitmap_words(half)), sp.expected(col, qs, 7, half)[:2], "binding, masked")
    ip2, t2, w2 = vdb.pack_sparse_vectors(qs)
    assert (ip2 == ip).all() and (t2 == t).all() and (w2 == w).all()
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_dense_variants_give_the_same_bytes(vdb, metric):
    col = sp.column(513, 30522)
    qs = sp.queries(30522)
    mask = np.random.default_rng(3).random(513) < 0.5
    want, want_m = sp.expected(col, qs, 50), sp.expected(col, qs, 50, mask)
    for prec in ("auto", "fp32"):
        ix, V, Q = _index(vdb, 513, metric, precision=prec, col=col)
        before = {s: ix.stat(s) for s in STATS}
        _check(ix, col, qs, 50, what=f"{metric} {prec}", want=want)
        _check(ix, col, qs, 50, mask=mask, what=f"{metric} {prec} masked", want=want_m)
        after = {s: ix.stat(s) for s in STATS}
        moved = {s: after[s] - before[s] for s in STATS if after[s] != before[s]}
        assert moved == {"sparse_searches": 4, "sparse_queries": 20}, moved  # no dense stat moves
        ix.close()


# =============================================================================
# the column's lifetime
# =============================================================================
def test_add_remove_clear_drop_the_column_update_keeps_it(vdb):
    col = sp.column(37, 30522)
    qs = sp.queries(30522)
    ix, V, Q = _index(vdb, 37, col=col)
    assert (ix.stat("sparse_rows"), ix.stat("sparse_nnz"), ix.stat("sparse_sets")) == (37, col.nnz, 1)
    want = sp.expected(col, qs, 10)
    _check(ix, col, qs, 10, want=want)
    ix.update(np.asarray([3, 5], np.int64), V[:2] * 2)  # an update keeps it
    assert ix.stat("sparse_rows") == 37
    _check(ix, col, qs, 10, want=want, what="after an update")
    ix.set_groups(np.arange(37) % 3)  # the group column is independent
    assert ix.stat("sparse_rows") == 37 and ix.stat("group_rows") == 37
    ix.set_groups(None)
    assert ix.stat("sparse_rows") == 37

    def gone(what):
        assert ix.stat("sparse_rows") == 0 and ix.stat("sparse_nnz") == 0, what
        assert _call(ix, qs, 10)[0] == VDB_ERR_INVALID, what
        assert _call_hybrid(ix, Q[:5], qs, 5, 10)[0] == VDB_ERR_INVALID, what

    ix.add(V[:1])
    gone("after an add")
    col38 = sp.Column(col.rows + [col.rows[0]], col.n_terms)
    ix.set_sparse(col38.indptr, col38.terms, col38.weights, col38.n_terms)
    _check(ix, col38, qs, 10, what="re-attached after the add")
    bits = np.zeros(38, bool)
    bits[37] = True
    ix.remove(fc.bitmap_words(bits))
    gone("after a remove")
    ix.set_sparse(col.indptr, col.terms, col.weights, col.n_terms)
    _check(ix, col, qs, 10, want=want, what="re-attached after the remove")
    ix.set_sparse(None)  # detach
    gone("after a detach")
    ix.set_sparse(col.indptr, col.terms, col.weights, col.n_terms)
    ix.clear()
    gone("after a clear")
    # an empty index with an empty column attached: "no result" everywhere
    ix.set_sparse(np.zeros(1, np.int64), None, None, 7)
    q7 = sp.queries(5)  # (terms below the empty column's n_terms)
    code, (s, i, k) = _call(ix, q7, 3)
    assert code == 0 and (i == -1).all() and (s == 0).all() and np.isneginf(k).all()
    s, i, k = _call_device(ix, q7, 3)
    assert (i == -1).all() and (s == 0).all() and np.isneginf(k).all()
    code, (s, i, f, h) = _call_hybrid(ix, Q[:5], q7, 3, 3)
    assert code == 0 and (i == -1).all() and (s == 0).all() and np.isneginf(f).all() and (h == 0).all()
    assert ix.stat("sparse_sets") == 5
    ix.close()


def _bad_columns(col):
    """(name, indptr, terms, weights, n_terms, error) for each way a column can be refused."""
    ip, t, w, nt = col.indptr, col.terms, col.weights, col.n_terms
    r = int(np.argmax(np.diff(ip) >= 2))  # a row of two entries or more
    e = int(ip[r])
    assert ip[r + 1] - ip[r] >= 2 and ip[4] > 0
    out = []
    tt = t.copy(); tt[e + 1] = tt[e]
    out.append(("a non-ascending term", ip, tt, w, nt, VDB_ERR_INVALID))
    tt = t.copy(); tt[int(ip[r + 1]) - 1] = nt
    out.append(("an out-of-range term", ip, tt, w, nt, VDB_ERR_INVALID))
    ww = w.copy(); ww[e] = np.inf
    out.append(("an Inf weight", ip, t, ww, nt, VDB_ERR_NONFINITE))
    ww = w.copy(); ww[-1] = np.nan
    out.append(("a NaN weight", ip, t, ww, nt, VDB_ERR_NONFINITE))
    ii = ip.copy(); ii[5] = ii[4] - 1 if ii[4] > 0 else ii[6] + 1
    out.append(("a decreasing indptr", ii, t, w, nt, VDB_ERR_INVALID))
    ii = ip.copy(); ii[0] = 1
    out.append(("indptr[0] != 0", ii, t, w, nt, VDB_ERR_INVALID))
    ii = ip.copy(); ii[-1] -= 1
    out.append(("indptr[n] != nnz", ii, t, w, nt, VDB_ERR_INVALID))
    out.append(("n != count", ip[:-1], t[:int(ip[-2])], w[:int(ip[-2])], nt, VDB_ERR_INVALID))
    out.append(("n_terms 0", ip, t, w, 0, VDB_ERR_INVALID))
    return out


def test_a_failed_set_sparse_leaves_the_earlier_column(vdb):
    import torch
    col = sp.column(37, 30522)
    other = sp.column(37, 30522, seed=5)
    qs = sp.queries(30522)
    ix, V, Q = _index(vdb, 37, col=col)
    want = sp.expected(col, qs, 10)
    f = ix._lib.vdb_index_set_sparse
    for name, ip, t, w, nt, err in _bad_columns(other):
        ip, t, w = (np.ascontiguousarray(x) for x in (ip, t, w))
        assert f(ix._h, _p(ip), _p(t), _p(w), ip.size - 1, t.size, nt, 0, None) == err, name
        dip, dt, dw = _dev(ip, torch), _dev(t, torch), _dev(w, torch)
        torch.cuda.synchronize()
        assert f(ix._h, ctypes.c_void_p(dip.data_ptr()), ctypes.c_void_p(dt.data_ptr()), ctypes.c_void_p(dw.data_ptr()),
                 ip.size - 1, t.size, nt, 1, None) == err, name + " (device)"
        assert (ix.stat("sparse_rows"), ix.stat("sparse_nnz"), ix.stat("sparse_sets")) == (37, col.nnz, 1), name
        _check(ix, col, qs, 10, want=want, what="after " + name, device=False)
    assert f(ix._h, _p(other.indptr), _p(other.terms), _p(other.weights), 37, other.nnz, other.n_terms, 7, None) == VDB_ERR_INVALID
    assert f(ix._h, None, None, None, 37, 0, 1, 0, None) == VDB_ERR_INVALID  # NULL detaches only with n == 0
    assert f(ix._h, _p(other.indptr), None, _p(other.weights), 37, other.nnz, other.n_terms, 0, None) == VDB_ERR_INVALID
    with pytest.raises(ValueError, match="ascending"):
        ix.set_sparse(other.indptr, other.terms[::-1].copy(), other.weights, other.n_terms)
    _check(ix, col, qs, 10, want=want, what="after every refusal")
    # a device-memory column attaches and gives the same bytes
    dip, dt, dw = _dev(other.indptr, torch), _dev(other.terms, torch), _dev(other.weights, torch)
    torch.cuda.synchronize()
    ix.set_sparse_device(dip.data_ptr(), dt.data_ptr(), dw.data_ptr(), 37, other.nnz, other.n_terms)
    del dip, dt, dw
    assert ix.stat("sparse_sets") == 2 and ix.stat("sparse_nnz") == other.nnz
    _check(ix, other, qs, 10, what="a device-memory column")
    ix.close()


# =============================================================================
# errors, bad device input, stats
# =============================================================================
def test_host_errors_leave_the_stats_untouched(vdb):
    col = sp.column(37, 30522)
    qs = sp.queries(30522)
    ix, V, Q = _index(vdb, 37, col=col)
    assert _call(ix, qs, 5)[0] == 0
    before = {s: ix.stat(s) for s in STATS}
    ip, t, w = sp.pack(qs)
    for kw in (dict(k=0), dict(k=1025), dict(k=-1), dict(mem=7), dict(n_queries=-1), dict(q_nnz=-1)):
        a = dict(k=5)
        a.update(kw)
        code, got = _call(ix, qs, a.pop("k"), **a)
        assert code == VDB_ERR_INVALID, kw
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
        code, got = _call(ix, None, 5, csr=csr)
        assert code == err, name
        assert np.isnan(got[0]).all() and (got[1] == S_IDX).all(), f"outputs written on {name}"
        code, got = _call_hybrid(ix, Q[:csr[0].size - 1], None, 5, 10, csr=csr)
        assert code == err, name + " (hybrid)"
    # NULL pointers
    sc, idx = np.zeros(25, np.float32), np.zeros(25, np.int64)
    f = ix._lib.vdb_index_search_sparse
    assert f(ix._h, None, _p(t), _p(w), 5, t.size, 5, None, 0, _p(sc), _p(idx), None, 0, None) == VDB_ERR_INVALID
    assert f(ix._h, _p(ip), _p(t), _p(w), 5, t.size, 5, None, 0, None, _p(idx), None, 0, None) == VDB_ERR_INVALID
    assert f(ix._h, _p(ip), _p(t), _p(w), 5, t.size, 5, None, 0, _p(sc), None, None, 0, None) == VDB_ERR_INVALID
    # the hybrid call's own checks
    for kw in (dict(k=0, fetch_k=10), dict(k=201, fetch_k=201), dict(k=10, fetch_k=9), dict(k=10, fetch_k=201),
               dict(weights=(-1.0, 1.0)), dict(weights=(1.0, np.nan)), dict(weights=(np.inf, 1.0)), dict(rrf_c=-1.0),
               dict(rrf_c=np.nan), dict(mem=7)):
        a = dict(k=5, fetch_k=10)
        a.update(kw)
        code, got = _call_hybrid(ix, Q[:5], qs, a.pop("k"), a.pop("fetch_k"), **a)
        assert code == VDB_ERR_INVALID, kw
        assert np.isnan(got[0]).all() and (got[1] == S_IDX).all(), f"outputs written on {kw}"
    Qb = Q[:5].copy()
    Qb[2, 1] = np.nan
    assert _call_hybrid(ix, Qb, qs, 5, 10)[0] == VDB_ERR_NONFINITE
    with pytest.raises(ValueError, match="1024"):
        ix.search_sparse(ip, t, w, 1025)
    with pytest.raises(ValueError, match="fetch_k"):
        ix.search_hybrid(Q[:5], ip, t, w, 10, 5)
    with pytest.raises(ValueError, match="row_mask"):
        ix.search_sparse(ip, t, w, 5, row_mask=np.zeros(1, np.uint32))
    assert {s: ix.stat(s) for s in STATS} == before
    # what is no error: no queries; queries without terms
    assert _call(ix, [], 5)[0] == 0 and _call_hybrid(ix, Q[:0], [], 5, 10)[0] == 0
    assert {s: ix.stat(s) for s in STATS} == before
    code, got = _call(ix, [qs[1], qs[1]], 5)
    assert code == 0 and (got[1] == -1).all()
    after = {s: ix.stat(s) for s in STATS}
    assert (after["sparse_searches"] - before["sparse_searches"], after["sparse_queries"] - before["sparse_queries"]) == (1, 2)
    ix.close()
    # no column attached
    ix, V, Q = _index(vdb, 37)
    assert _call(ix, qs, 5)[0] == VDB_ERR_INVALID and _call_hybrid(ix, Q[:5], qs, 5, 10)[0] == VDB_ERR_INVALID
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
    col = sp.column(513, 30522)
    qs = sp.queries(30522)
    ix, V, Q11 = _index(vdb, 513, col=col, seed=1)
    V, Q11 = sp.dense_rows(513, 1, n_queries=11)
    csr, nnz, bad, good = _garbage(qs, 30522)
    for wgs in (1, 2):
        ix.set_param("sparse_wgs", wgs)
        before = ix.stat("sparse_bad_queries")
        s, i, k = _call_device(ix, None, 10, csr=csr, q_nnz=nnz)
        torch.cuda.synchronize()
        assert ix.stat("sparse_bad_queries") - before == len(bad)
        for b in range(11):
            one = (s[b:b + 1], i[b:b + 1], k[b:b + 1])
            if b in bad:
                assert (one[1] == -1).all() and (one[0] == 0).all() and np.isneginf(one[2]).all(), b
            else:
                _same(one, sp.expected(col, [good[b]], 10), f"good query {b} beside bad ones")
    # the hybrid call: a bad query contributes an empty sparse list, its dense list still ranks
    before = ix.stat("sparse_bad_queries")
    empty = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    got = _call_hybrid_device(ix, Q11, None, 10, 40, csr=csr)
    torch.cuda.synchronize()
    assert ix.stat("sparse_bad_queries") - before == len(bad)
    want = sp.expected_hybrid(V, Q11, col, [good.get(b, empty) for b in range(11)], 10, 40, "cosine", sparse_empty=bad)
    _same(got, want, "hybrid beside bad sparse queries")
    assert (got[3][sorted(bad)] == 1).all() and (got[1][sorted(bad)] >= 0).all()
    # no HIP error afterwards: the device and the index still answer
    _check(ix, col, qs, 10, what="after the bad input")
    ix.close()


def test_stats_move_once_per_call(vdb):
    col = sp.column(37, 30522)
    qs = sp.queries(30522)
    ix, V, Q = _index(vdb, 37, col=col)
    before = {s: ix.stat(s) for s in STATS}
    assert _call(ix, qs, 5)[0] == 0
    _call_device(ix, qs[:2], 5)
    assert _call_hybrid(ix, Q[:5], qs, 5, 10)[0] == 0
    _call_hybrid_device(ix, Q[:2], qs[:2], 5, 10)
    after = {s: ix.stat(s) for s in STATS}
    d = {s: after[s] - before[s] for s in STATS}
    assert (d["sparse_searches"], d["sparse_queries"], d["hybrid_searches"], d["hybrid_queries"]) == (2, 7, 2, 7)
    assert (d["searches"], d["queries"], d["sparse_bad_queries"], d["sparse_sets"]) == (2, 7, 0, 0)
    ix.close()


# =============================================================================
# hybrid search
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_hybrid_is_the_rrf_of_the_two_lists(vdb, metric):
    n = 513
    col = sp.column(n, 30522)
    qs = sp.queries(30522)
    mask = np.random.default_rng(12).random(n) < 0.5
    ix, V, Q = _index(vdb, n, metric, col=col)
    for B in (1, 5):
        for k, F in ((10, 10), (10, 200)):
            for weights in ((1.0, 1.0), (2.0, 0.5), (1.0, 0.0), (0.0, 1.0)):
                for c in (0.0, 60.0):
                    what = f"{metric} B {B} k {k} fetch {F} weights {weights} rrf_c {c}"
                    want = sp.expected_hybrid(V, Q[:B], col, qs[:B], k, F, metric, weights, c)
                    code, got = _call_hybrid(ix, Q[:B], qs[:B], k, F, weights, c)
                    assert code == 0, f"{what}: {ix._lib.vdb_last_error()}"
                    _same(got, want, what + " host")
                    if c == 60.0:
                        _same(_call_hybrid_device(ix, Q[:B], qs[:B], k, F, weights, c), want, what + " device")
                    if weights[1] == 0.0 and weights[0] > 0:  # the dense search's rows, in its order
                        s, i = ix.search(Q[:B], k)
                        np.testing.assert_array_equal(got[1], i)
    # a mask, an offset, and the sparse kernel's merge tail under the fusion
    ix.set_param("sparse_wgs", 2)
    want = sp.expected_hybrid(V, Q[:5], col, qs, 10, 40, metric, (1.0, 1.0), 60.0, mask, 2 ** 40)
    words = fc.bitmap_words(mask)
    code, got = _call_hybrid(ix, Q[:5], qs, 10, 40, mask=words, index_offset=2 ** 40)
    assert code == 0
    _same(got, want, "masked host")
    _same(_call_hybrid_device(ix, Q[:5], qs, 10, 40, mask=words, index_offset=2 ** 40), want, "masked device")
    # a query with no matching term (and one without terms) equals its dense-only fusion
    cold = (np.asarray([t for t in range(1, 40) if t not in sp.hot_terms(30522) and not (col.terms == t).any()][:3], np.int32),
            np.ones(3, np.float32))
    code, got = _call_hybrid(ix, Q[:2], [cold, qs[1]], 10, 40)
    assert code == 0 and (got[3] == 1).all()
    empty = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    _same(got, sp.expected_hybrid(V, Q[:2], col, [empty, empty], 10, 40, metric), "dense-only fusion")
    # the optional outputs and the binding
    ip, t, w = sp.pack(qs)
    code, got = _call_hybrid(ix, Q[:5], qs, 10, 40, with_fused=False, with_hits=False)
    assert code == 0 and got[2] is None and got[3] is None
    want = sp.expected_hybrid(V, Q[:5], col, qs, 10, 40, metric)
    _same(got, want, "without fused and hits")
    _same(ix.search_hybrid(Q[:5], ip, t, w, 10, 40, with_fused=True, with_hits=True), want, "binding")
    _same(ix.search_hybrid(Q[:5], ip, t, w, 10, 40), want[:2], "binding, two outputs")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_hybrid_precisions_give_the_same_bytes(vdb, metric):
    n = 1300
    col, qs = sp.tie_case(n)  # tied sparse keys under the fusion: the row-id rule twice over
    V, Q = sp.dense_rows(n)
    want = sp.expected_hybrid(V, Q[:2], col, qs, 50, 200, metric, (1.0, 2.0))
    for prec in ("auto", "fp32"):
        ix, V, Q = _index(vdb, n, metric, precision=prec, col=col)
        code, got = _call_hybrid(ix, Q[:2], qs, 50, 200, (1.0, 2.0))
        assert code == 0
        _same(got, want, f"{metric} {prec} host")
        _same(_call_hybrid_device(ix, Q[:2], qs, 50, 200, (1.0, 2.0)), want, f"{metric} {prec} device")
        ix.close()

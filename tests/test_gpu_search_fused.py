"""Fused search (include/vdb.h vdb_index_search_fused; csrc/vdb_fuse.hip).

The contract: list l of a set is what a search for its l-th sub-query returns (the best fetch_k
eligible rows by (canonical fp64 key desc, row asc)); a row's fused value is the weighted sum of its
reciprocal ranks in list order (RRF) or its greatest key (MAX); the candidates rank by (fused desc,
row asc); slots past min(k, candidates) hold 0 / -1 / -inf / 0.  Every case compares all four outputs
with the literal oracle of tests/_fused_cases.py (preconditions: tests/test_fused_precondition.py)
BIT FOR BIT: the fp64 values as uint64, the fp32 scores as uint32; no tolerance appears anywhere.

``_check`` runs a case in host memory and in device memory.  Every output carries a guard region past
[n_sets][k] filled with a sentinel, which must be untouched afterwards.

Shapes are the smallest at which the kernel can go wrong: sets of 0, 1, 2, 3, 5 and 16 lists, list
lengths around a wave (63, 64, 65) and at the limit (200), 3 200 entries (the largest sort), 70 sets in
one call, fewer eligible rows than fetch_k and none.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fused_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 257
S_IDX = -7
S_HIT = -9
METRICS = fc.METRICS
FUSION = {"rrf": 0, "max": 1}
VDB_ERR_INVALID = -1
VDB_ERR_NONFINITE = -4
STATS = ("searches", "queries", "fused_searches", "fused_sets", "fused_bad_sets")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    assert _vdb.VDB_ERR_INVALID == VDB_ERR_INVALID and _vdb.VDB_ERR_NONFINITE == VDB_ERR_NONFINITE
    assert _vdb.FUSION_IDS == FUSION
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
    """The four outputs bit for bit (got / want: (scores, idx, fused, hits); None entries skipped)."""
    for name, g, w in zip(("scores", "indices", "fused", "hits"), got, want):
        if g is None or w is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} {what}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{name} {what}")


def _call(ix, Q, offs, k, fetch_k, fusion="rrf", weights=None, rrf_c=fc.RRF_C, mask=None, index_offset=0,
          with_fused=True, with_hits=True, n_sub=None, n_sets=None, mem=0):
    """The C-ABI call in host memory with guarded outputs -> (rc, (scores, idx, fused, hits))."""
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    offs = np.ascontiguousarray(offs, np.int64)
    n_sub = Q.shape[0] if n_sub is None else n_sub
    S = offs.size - 1 if n_sets is None else n_sets
    n = max(S, 0) * max(k, 0)
    sc = np.full(n + GUARD, np.nan, np.float32)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    fu = np.full(n + GUARD, np.nan, np.float64) if with_fused else None
    hi = np.full(n + GUARD, S_HIT, np.int32) if with_hits else None
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    code = ix._lib.vdb_index_search_fused(ix._h, _p(Q) if Q.size else None, n_sub, _p(offs), S, _p(w), k, fetch_k,
                                          FUSION.get(fusion, fusion), ctypes.c_double(rrf_c), _p(m), mem, _p(sc), _p(idx),
                                          _p(fu), _p(hi), index_offset, None)
    assert np.isnan(sc[n:]).all(), "scores guard touched"
    assert (idx[n:] == S_IDX).all(), "indices guard touched"
    assert fu is None or np.isnan(fu[n:]).all(), "fused guard touched"
    assert hi is None or (hi[n:] == S_HIT).all(), "hits guard touched"
    shape = (max(S, 0), max(k, 0))
    return code, (sc[:n].reshape(shape), idx[:n].reshape(shape), None if fu is None else fu[:n].reshape(shape),
                  None if hi is None else hi[:n].reshape(shape))


def _call_device(ix, Q, offs, k, fetch_k, fusion="rrf", weights=None, rrf_c=fc.RRF_C, mask=None, index_offset=0,
                 with_fused=True, with_hits=True):
    """The same call with every argument in device memory on a side stream -> the four outputs."""
    import torch
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    offs = np.ascontiguousarray(offs, np.int64)
    S, n_sub = offs.size - 1, Q.shape[0]
    n = S * k
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dq = torch.from_numpy(Q.copy()).to(dev) if n_sub else None
        do = torch.from_numpy(offs.copy()).to(dev)
        dw = torch.from_numpy(np.asarray(weights, np.float64).copy()).to(dev) if weights is not None else None
        dm = torch.from_numpy(np.ascontiguousarray(mask, np.uint32).view(np.int32).copy()).to(dev) if mask is not None else None
        ds = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        di = torch.full((n + GUARD,), S_IDX, dtype=torch.int64, device=dev)
        df = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device=dev)
        dh = torch.full((n + GUARD,), S_HIT, dtype=torch.int32, device=dev)
        ix.search_fused_device(dq.data_ptr() if dq is not None else 0, n_sub, do.data_ptr(), S, k, fetch_k,
                               ds.data_ptr(), di.data_ptr(), fusion=fusion,
                               weights_ptr=dw.data_ptr() if dw is not None and dw.numel() else 0, rrf_c=rrf_c,
                               out_fused_ptr=df.data_ptr() if with_fused else 0,
                               out_hits_ptr=dh.data_ptr() if with_hits else 0,
                               mask_ptr=dm.data_ptr() if dm is not None else 0, index_offset=index_offset,
                               stream=st.cuda_stream)
    st.synchronize()
    s, i, f, h = (x.cpu().numpy() for x in (ds, di, df, dh))
    assert np.isnan(s[n:]).all() and (i[n:] == S_IDX).all(), "guard touched (device)"
    assert np.isnan(f[n if with_fused else 0:]).all() and (h[n if with_hits else 0:] == S_HIT).all(), "guard touched (device)"
    return (s[:n].reshape(S, k), i[:n].reshape(S, k), f[:n].reshape(S, k) if with_fused else None,
            h[:n].reshape(S, k) if with_hits else None)


def _check(ix, V, Q, offs, k, fetch_k, fusion, metric, weights=None, rrf_c=fc.RRF_C, mask=None, words=None,
           index_offset=0, what="", device=True):
    """Call in host and in device memory and compare both with the oracle; ``mask``: bool [N]
    (``words``: the bitmap sent, if not its plain packing).  Returns the host outputs."""
    want = fc.expected(Q, offs, V, k, fetch_k, fusion, metric, weights, rrf_c, mask, index_offset)
    if words is None and mask is not None:
        words = fc.bitmap_words(mask)
    what = f"{what} ({metric}, {fusion}, k {k}, fetch {fetch_k})"
    code, got = _call(ix, Q, offs, k, fetch_k, fusion, weights, rrf_c, words, index_offset)
    assert code == 0, f"status {code} {what}: {ix._lib.vdb_last_error()}"
    _same(got, want, what + " host")
    if device:
        _same(_call_device(ix, Q, offs, k, fetch_k, fusion, weights, rrf_c, words, index_offset), want, what + " device")
    return got


# =============================================================================
# the cases
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", [2, 16])
def test_identical_lists(vdb, m, metric):
    V, Qs = fc.identical_case(m)
    ix = _index(vdb, V, metric)
    for fusion in fc.FUSIONS:
        s, i, f, h = _check(ix, V, Qs, fc.offsets_of([m]), 64, 64, fusion, metric, what=f"identical m {m}")
        assert (h == m).all()
        _check(ix, V, Qs, fc.offsets_of([m]), 10, 64, fusion, metric, what=f"identical m {m}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", [2, 16])
def test_disjoint_lists_tie_rank_by_rank(vdb, m, metric):
    V, Qs = fc.disjoint_case(m)
    ix = _index(vdb, V, metric)
    offs = fc.offsets_of([m])
    s, i, f, h = _check(ix, V, Qs, offs, 200, 200, "rrf", metric, what=f"disjoint m {m}")
    assert (h == 1).all() and (np.diff(i[0, :200 // m * m].reshape(-1, m), axis=1) > 0).all()  # ties in row order
    _check(ix, V, Qs, offs, 200, 200, "max", metric, what=f"disjoint m {m}")
    _check(ix, V, Qs, offs, 7, 200, "rrf", metric, what=f"disjoint m {m}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", [3, 5])
def test_overlapping_lists_and_weights(vdb, m, metric):
    V, Qs = fc.overlap_case(m, metric)
    ix = _index(vdb, V, metric)
    offs = fc.offsets_of([m])
    F = fc.OVERLAP_FETCH
    s, i, f, h = _check(ix, V, Qs, offs, 200, F, "rrf", metric, what=f"overlap m {m}")
    assert h.min() >= 1 and h.max() == m
    _check(ix, V, Qs, offs, 200, F, "max", metric, what=f"overlap m {m}")
    _check(ix, V, Qs, offs, 10, 40, "rrf", metric, what=f"overlap m {m}")
    for c in (0.0, 1.0, 1e6):
        _check(ix, V, Qs, offs, 50, F, "rrf", metric, rrf_c=c, what=f"overlap m {m} rrf_c {c}", device=False)
    # weights 0.0, 0.5, 3.0; and NULL weights are all-ones
    w = np.asarray(fc.WEIGHTS[m])
    ws, wi, wf, wh = _check(ix, V, Qs, offs, 200, F, "rrf", metric, weights=w, what=f"weighted m {m}")
    assert (wi != i).any()
    ones = _check(ix, V, Qs, offs, 200, F, "rrf", metric, weights=np.ones(m), what="all-ones weights")
    _same(ones, (s, i, f, h), "all-ones weights against NULL")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_short_lists_and_padding(vdb, metric):
    n = 300
    V, Q = fc.corpus(n, 32, seed=2)
    ix = _index(vdb, V, metric)
    few = np.zeros(n, bool)
    few[np.random.default_rng(5).choice(n, size=20, replace=False)] = True
    half = np.random.default_rng(6).random(n) < 0.5
    offs = fc.offsets_of([3])
    for fusion in fc.FUSIONS:
        s, i, f, h = _check(ix, V, Q[:3], offs, 50, 50, fusion, metric, mask=few, what="fewer eligible rows than fetch_k")
        assert (i[0, :20] >= 0).all() and few[i[0, :20]].all() and (i[0, 20:] == -1).all()
        assert (s[0, 20:] == 0).all() and np.isneginf(f[0, 20:]).all() and (h[0, 20:] == 0).all()
        s, i, f, h = _check(ix, V, Q[:3], offs, 5, 40, fusion, metric, mask=np.zeros(n, bool), what="no eligible row")
        assert (i == -1).all() and (s == 0).all() and np.isneginf(f).all() and (h == 0).all()
        _check(ix, V, Q[:3], offs, 10, 40, fusion, metric, mask=half, what="half")
        # k > the union without a mask: a corpus smaller than k
        _check(ix, V, Q[:3], offs, 10, 40, fusion, metric, what="no mask")
        # bits at or past count name no row (n = 300: 20 spare bits in the last word, then a whole word)
        words = fc.bitmap_words(half, extra_bits=52)
        assert words.size == (n + 31) // 32 + 1
        _check(ix, V, Q[:3], offs, 10, 40, fusion, metric, mask=half, words=words, what="mask bits past count")
    ix.close()
    V, Q = fc.corpus(7, 16, seed=2)
    ix = _index(vdb, V, metric)
    s, i, f, h = _check(ix, V, Q[:2], fc.offsets_of([2]), 10, 20, "rrf", metric, what="seven rows")
    assert (i[0, :7] >= 0).all() and (i[0, 7:] == -1).all() and (h[0, :7] == 2).all()
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_size_edges(vdb, metric):
    V, Q, offs = fc.mixed_sets_case()  # sets of 0, 1, 16, 0 and 2 sub-queries in one call
    ix = _index(vdb, V, metric)
    for fetch in fc.SIZE_FETCH:
        for k in sorted({1, fetch}):
            for fusion in fc.FUSIONS:
                s, i, f, h = _check(ix, V, Q, offs, k, fetch, fusion, metric, what="mixed sets", device=fetch in (1, 65, 200))
                assert (i[0] == -1).all() and (i[3] == -1).all() and (i[1:3, 0] >= 0).all() and i[4, 0] >= 0
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_many_sets_and_a_set_depends_on_itself_alone(vdb, metric):
    V, Q, offs = fc.many_sets_case()
    ix = _index(vdb, V, metric)
    S = offs.size - 1
    assert S == 70
    for fusion in fc.FUSIONS:
        got = _check(ix, V, Q, offs, 10, 40, fusion, metric, what="70 sets")
        # set 2 (4 sub-queries) alone, and moved to the first, a middle and the last position
        alone = _call(ix, Q[offs[2]:offs[3]], fc.offsets_of([4]), 10, 40, fusion)
        assert alone[0] == 0
        _same(alone[1], [g[2:3] for g in got], "a set alone")
        sizes = np.diff(offs)
        for pos in (0, 35, 69):
            order = [s for s in range(S) if s != 2]
            order.insert(pos, 2)
            Qp = np.concatenate([Q[offs[s]:offs[s + 1]] for s in order])
            code, moved = _call(ix, Qp, fc.offsets_of(sizes[order]), 10, 40, fusion)
            assert code == 0
            _same(moved, [g[order] for g in got], f"set 2 at position {pos}")
    ix.close()


# =============================================================================
# properties
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_precisions_and_force_exact_give_the_same_bytes(vdb, metric):
    Vo, Qo = fc.overlap_case(3, metric)
    Vd, Qd = fc.disjoint_case(2)
    runs = [(Vo, Qo, fc.offsets_of([3]), 50, 64), (Vd, Qd, fc.offsets_of([2]), 200, 200)]
    wants = {(j, fusion): fc.expected(Q, offs, V, k, F, fusion, metric)
             for j, (V, Q, offs, k, F) in enumerate(runs) for fusion in fc.FUSIONS}
    for prec, force in [(p, 0) for p in ("fp32", "bf16x3", "bf16", "i8", "i8x3", "auto")] + [("auto", 1)]:
        for j, (V, Q, offs, k, F) in enumerate(runs):
            ix = _index(vdb, V, metric, precision=prec)
            if force:
                ix.set_param("force_exact", 1)
            for fusion in fc.FUSIONS:
                code, got = _call(ix, Q, offs, k, F, fusion)
                assert code == 0, (prec, force)
                _same(got, wants[(j, fusion)], f"precision {prec} force_exact {force} run {j} {fusion}")
            ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_one_list_under_max_is_the_plain_search(vdb, metric):
    V, Q = fc.corpus(700, 32, seed=1)
    ix = _index(vdb, V, metric)
    mask = np.random.default_rng(2).random(700) < 0.5
    for k, m in ((10, None), (64, None), (1, None), (200, None), (40, mask)):
        words = None if m is None else fc.bitmap_words(m)
        code, got = _call(ix, Q[:4], fc.offsets_of([1, 1, 1, 1]), k, k, "max", mask=words)
        assert code == 0
        s, i, ks = ix.search(Q[:4], k, row_mask=words, with_keys=True)
        _same(got[:3], (s, i, ks), f"one list under MAX against search, k {k}")
        assert (got[3] == 1).all()
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_max_is_the_exact_top_k_of_the_corpus(vdb, metric):
    for V, Qs in (fc.overlap_case(3, metric), fc.overlap_case(5, metric)):
        ix = _index(vdb, V, metric)
        mask = np.random.default_rng(9).random(V.shape[0]) < 0.5
        assert np.unique(np.concatenate([c for c, _ in fc.set_lists(Qs, V, 10, metric)])).size < 10 * len(Qs)
        for k, fetch, m in ((10, 10, None), (10, 40, None), (64, 64, mask), (1, 1, None), (200, 200, None)):
            words = None if m is None else fc.bitmap_words(m)
            code, (s, i, f, h) = _call(ix, Qs, fc.offsets_of([len(Qs)]), k, fetch, "max", mask=words)
            assert code == 0
            rows, vals = fc.brute_force_max(Qs, V, k, metric, m)
            np.testing.assert_array_equal(i[0], rows)
            np.testing.assert_array_equal(_bits(f[0]), _bits(vals))
            np.testing.assert_array_equal(_bits(s[0]), _bits(fc.key_scores(vals, metric)))
        ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_index_offset_moves_the_valid_ids_only(vdb, metric):
    V, Q = fc.corpus(65, 16, seed=2)
    ix = _index(vdb, V, metric)
    off = 2 ** 40
    offs = fc.offsets_of([2, 0, 1])
    for fusion in fc.FUSIONS:
        base = _check(ix, V, Q[:3], offs, 70, 70, fusion, metric)
        moved = _check(ix, V, Q[:3], offs, 70, 70, fusion, metric, index_offset=off)
        assert (base[1] == -1).any() and (base[1] >= 0).any()
        np.testing.assert_array_equal(moved[1], np.where(base[1] >= 0, base[1] + off, -1))
        _same((moved[0], None, moved[2], moved[3]), (base[0], None, base[2], base[3]))
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_optional_outputs(vdb, metric):
    V, Q = fc.corpus(300, 32, seed=2)
    ix = _index(vdb, V, metric)
    offs = fc.offsets_of([3, 2])
    want = fc.expected(Q[:5], offs, V, 10, 20, "rrf", metric)
    for with_fused, with_hits in ((False, False), (True, False), (False, True)):
        code, got = _call(ix, Q[:5], offs, 10, 20, "rrf", with_fused=with_fused, with_hits=with_hits)
        assert code == 0
        assert (got[2] is None) == (not with_fused) and (got[3] is None) == (not with_hits)
        _same(got, want, f"fused {with_fused} hits {with_hits}")
        got = _call_device(ix, Q[:5], offs, 10, 20, "rrf", with_fused=with_fused, with_hits=with_hits)
        _same(got, want, f"fused {with_fused} hits {with_hits} device")
    # the binding returns what was asked for, in order
    s, i = ix.search_fused(Q[:5], offs, 10, 20)
    s2, i2, h = ix.search_fused(Q[:5], offs, 10, 20, with_hits=True)
    s3, i3, f, h3 = ix.search_fused(Q[:5], offs, 10, 20, with_fused=True, with_hits=True)
    _same((s, i, None, None), want)
    _same((s2, i2, None, h), want)
    _same((s3, i3, f, h3), want)
    q, o = vdb.pack_query_sets([Q[:3], Q[3:5]], 32)
    np.testing.assert_array_equal(q, Q[:5])
    np.testing.assert_array_equal(o, offs)
    ix.close()


# =============================================================================
# errors, bad device input, stats, the empty index
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_host_errors_leave_the_stats_untouched(vdb, metric):
    V, Q = fc.corpus(300, 32, seed=2)
    ix = _index(vdb, V, metric)
    Q20 = np.concatenate([Q, Q, Q[:4]])  # 20 sub-queries
    ok = fc.offsets_of([3, 2])
    assert _call(ix, Q[:5], ok, 5, 20)[0] == 0
    before = {s: ix.stat(s) for s in STATS}
    nan, inf = float("nan"), float("inf")
    bad = [dict(k=0, fetch_k=10), dict(k=201, fetch_k=201), dict(k=10, fetch_k=9), dict(k=10, fetch_k=201),
           dict(k=-1, fetch_k=-1), dict(fusion=2), dict(fusion=-1), dict(rrf_c=nan), dict(rrf_c=inf), dict(rrf_c=-1.0),
           dict(mem=7), dict(n_sub=-1), dict(n_sets=-1),
           dict(offs=[0, 3, 2]), dict(offs=[0, 3, 6]), dict(offs=[-1, 3, 5]), dict(offs=[3, 2, 5]),
           dict(Q=Q20, offs=[0, 17, 20]),
           dict(fusion="max", weights=np.ones(5)),
           dict(weights=[1, 1, nan, 1, 1]), dict(weights=[1, 1, 1, inf, 1]), dict(weights=[1, -0.5, 1, 1, 1])]
    for kw in bad:
        a = dict(Q=Q[:5], offs=ok, k=5, fetch_k=20)
        a.update(kw)
        code, got = _call(ix, a.pop("Q"), a.pop("offs"), a.pop("k"), a.pop("fetch_k"), **a)
        assert code == VDB_ERR_INVALID, kw
        assert np.isnan(got[0]).all() and (got[1] == S_IDX).all(), f"outputs written on {kw}"
    # NULL pointers
    sc, idx = np.zeros(10, np.float32), np.zeros(10, np.int64)
    q = np.ascontiguousarray(Q[:5])
    f = ix._lib.vdb_index_search_fused
    c = ctypes.c_double(60.0)
    assert f(ix._h, None, 5, _p(ok), 2, None, 5, 20, 0, c, None, 0, _p(sc), _p(idx), None, None, 0, None) == VDB_ERR_INVALID
    assert f(ix._h, _p(q), 5, None, 2, None, 5, 20, 0, c, None, 0, _p(sc), _p(idx), None, None, 0, None) == VDB_ERR_INVALID
    assert f(ix._h, _p(q), 5, _p(ok), 2, None, 5, 20, 0, c, None, 0, None, _p(idx), None, None, 0, None) == VDB_ERR_INVALID
    assert f(ix._h, _p(q), 5, _p(ok), 2, None, 5, 20, 0, c, None, 0, _p(sc), None, None, None, 0, None) == VDB_ERR_INVALID
    # a NaN / Inf in a host query
    for v in (np.nan, np.inf):
        Qb = Q[:5].copy()
        Qb[4, 3] = v
        assert _call(ix, Qb, ok, 5, 20)[0] == VDB_ERR_NONFINITE
    # the binding raises ValueError with the limit in the message
    with pytest.raises(ValueError, match="200"):
        ix.search_fused(Q[:5], ok, 201, 201)
    with pytest.raises(ValueError, match="fetch_k"):
        ix.search_fused(Q[:5], ok, 10, 5)
    with pytest.raises(ValueError, match="fusion"):
        ix.search_fused(Q[:5], ok, 5, 20, fusion="sum")
    with pytest.raises(ValueError, match="16"):
        ix.search_fused(Q20, [0, 17, 20], 5, 20)
    with pytest.raises(ValueError, match="weight"):
        ix.search_fused(Q[:5], ok, 5, 20, weights=[1, 1, 1])
    with pytest.raises(ValueError, match="weight"):
        ix.search_fused(Q[:5], ok, 5, 20, weights=[1, 1, 1, -1, 1])
    with pytest.raises(ValueError):
        ix.search_fused(Q[:5, :5], ok, 5, 20)
    with pytest.raises(ValueError, match="row_mask"):
        ix.search_fused(Q[:5], ok, 5, 20, row_mask=np.zeros(3, np.uint32))
    assert {s: ix.stat(s) for s in STATS} == before
    assert _call(ix, Q[:5], ok, 5, 20)[0] == 0  # and the index still answers
    # what is no error: rrf_c is ignored for MAX; 16 sub-queries are a set
    assert _call(ix, Q[:5], ok, 5, 20, "max", rrf_c=nan)[0] == 0
    assert _call(ix, Q20, [0, 16, 20], 5, 20)[0] == 0
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_device_memory_bad_input_is_answered_per_set(vdb, metric):
    import torch
    V, Q = fc.corpus(300, 32, seed=2, n_queries=30)
    ix = _index(vdb, V, metric)
    k, F, n_sub = 5, 20, 30
    nan = float("nan")
    # (offsets, weights, the sets that are bad)
    runs = [
        # a set of 17; decreasing; a good set between; past n_sub; lo past n_sub and decreasing
        ([0, 3, 20, 18, 21, 35, 24, 27, 30], None, {1, 2, 4, 5}),
        # a negative offset (clamped, bad); the next sets good
        ([-4, 2, 5], None, {0}),
        # every offset far outside
        ([2 ** 62, -2 ** 62, 2 ** 40], None, {0, 1}),
        # a NaN weight in set 1, a negative one in set 3, an infinite one in set 4; set 5 has 15 lists
        ([0, 3, 6, 9, 12, 15, 30], [1, 1, 1, 1, nan, 1, 1, 1, 1, 1, -0.5, 1, 1, float("inf"), 1] + [1.0] * 15, {1, 3, 4}),
    ]
    for fusion in fc.FUSIONS:
        for offs, w, bad in runs:
            if fusion == "max" and w is not None:  # (MAX takes no weights)
                continue
            offs = np.asarray(offs, np.int64)
            S = offs.size - 1
            before = ix.stat("fused_bad_sets")
            got = _call_device(ix, Q, offs, k, F, fusion, weights=w)
            torch.cuda.synchronize()
            assert ix.stat("fused_bad_sets") - before == len(bad), (fusion, offs.tolist())
            for s in range(S):
                one = [g[s:s + 1] for g in got]
                if s in bad:
                    assert (one[1] == -1).all() and (one[0] == 0).all() and np.isneginf(one[2]).all() and (one[3] == 0).all(), s
                else:
                    o0, o1 = int(offs[s]), int(offs[s + 1])
                    ws = None if w is None else np.asarray(w[o0:o1])
                    want = fc.expected(Q[o0:o1], fc.offsets_of([o1 - o0]), V, k, F, fusion, metric, ws)
                    _same(one, want, f"good set {s} beside bad ones")
    # no HIP error afterwards: the device and the index still answer
    torch.cuda.synchronize()
    _check(ix, V, Q[:3], fc.offsets_of([3]), k, F, "rrf", metric, what="after the bad input")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_stats_no_sets_and_the_empty_index(vdb, metric):
    V, Q = fc.corpus(300, 32, seed=2)
    ix = _index(vdb, V, metric)
    before = {s: ix.stat(s) for s in STATS}
    assert _call(ix, Q[:0], [0], 5, 20)[0] == 0  # n_sets == 0 is OK and counts nothing
    assert {s: ix.stat(s) for s in STATS} == before
    assert _call(ix, Q[:5], fc.offsets_of([3, 0, 2]), 5, 20)[0] == 0
    assert _call(ix, Q[:1], fc.offsets_of([1]), 1, 1, "max")[0] == 0
    code, got = _call(ix, Q[:0], fc.offsets_of([0, 0]), 3, 3)  # sets without any sub-query
    assert code == 0 and (got[1] == -1).all() and (got[3] == 0).all()
    _call_device(ix, Q[:5], fc.offsets_of([3, 2]), 5, 20)
    after = {s: ix.stat(s) for s in STATS}
    assert [after[s] - before[s] for s in STATS] == [4, 11, 4, 8, 0]
    ix.close()
    # an empty index: every slot "no result", counted as a search
    empty = vdb.NativeIndex(32, metric)
    for m in (None, np.zeros(1, np.uint32)):
        for fusion in fc.FUSIONS:
            code, (s, i, f, h) = _call(empty, Q[:5], fc.offsets_of([3, 2]), 7, 20, fusion, mask=m)
            assert code == 0
            assert (s == 0).all() and (i == -1).all() and np.isneginf(f).all() and (h == 0).all()
    s, i, f, h = _call_device(empty, Q[:5], fc.offsets_of([3, 2]), 7, 20)
    assert (s == 0).all() and (i == -1).all() and np.isneginf(f).all() and (h == 0).all()
    assert _call(empty, Q[:5], fc.offsets_of([3, 2]), 7, 20, with_fused=False, with_hits=False)[0] == 0
    assert [empty.stat(s) for s in STATS] == [6, 30, 6, 12, 0]
    empty.close()

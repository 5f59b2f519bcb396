"""Range search (include/vdb.h vdb_index_search_range; csrc/vdb_range.hip).

The contract: count[b] = the exact number of eligible rows whose canonical fp64 key is at or above
kt[b], and the first min(count, cap) of them in ascending row id with their fp32 scores and fp64
keys; slots past that -1 / 0 / -inf; nothing at or past cap written.  Every case compares counts,
indices, keys and scores with the oracle set ``{r : ref_cpu.exact_keys(q, V, metric)[r] >= kt}``
(tests/_range_cases.py; preconditions: tests/test_range_precondition.py) with
``assert_array_equal``.  No tolerance appears anywhere.

Every call goes through ``_call``: the output arrays carry a guard region past [B][cap] filled with
a sentinel, which must be untouched afterwards.

Shapes are the smallest at which the kernels can go wrong: dims that leave pad columns (1, 33,
100), one 256-dim piece and one piece plus 4 dims (256, 260), three and six pieces (768, 1536: the
4- and 8-piece held forms) and rows too long to hold (2100: the any-length form); row counts at
the last-word and last-workgroup edges of the bitmap and its prefix, for the scan (512 rows), for
the emit (8 192 rows per workgroup) and for the prefix kernel's carry loop (131 072 rows per round),
the latter two at 8 dims so that corpus and oracle stay cheap; caps past one trip of the score
kernel's strided loops; batches around the query block the plan picks.
"""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _range_cases as rc  # noqa: E402
from oracle import ref_cpu  # noqa: E402

pytestmark = pytest.mark.gpu

WG_ROWS = 512  # csrc/vdb_range_plan.h kRangeWgRows
GUARD = 257    # guard elements past [B][cap] of every output array
S_IDX, S_CNT = -7, -9
METRICS = rc.METRICS


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def _index(vdb, V, metric, precision=None):
    ix = vdb.NativeIndex(V.shape[1], metric, precision=precision)
    if V.shape[0]:
        ix.add(V)
    assert ix.count() == V.shape[0]
    return ix


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _call(ix, Q, thr, cap, mask=None, index_offset=0, with_keys=True, null_lists=False):
    """The C-ABI call in host memory with guarded outputs -> (rc, counts, idx, scores, keys)."""
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    B = Q.shape[0]
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thr, np.float64), (B,)))
    n = B * max(cap, 0)
    counts = np.full(B + GUARD, S_CNT, np.int64)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    sc = np.full(n + GUARD, np.nan, np.float32)
    ks = np.full(n + GUARD, np.nan, np.float64) if with_keys else None
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    code = ix._lib.vdb_index_search_range(
        ix._h, _p(Q), B, _p(thr), _p(m), 0, cap, _p(counts), None if null_lists else _p(idx),
        None if null_lists else _p(sc), None if null_lists else _p(ks), index_offset, None)
    assert (counts[B:] == S_CNT).all(), "counts guard touched"
    assert (idx[n:] == S_IDX).all(), "indices guard touched"
    assert np.isnan(sc[n:]).all(), "scores guard touched"
    assert ks is None or np.isnan(ks[n:]).all(), "keys guard touched"
    shape = (B, max(cap, 0))
    return (code, counts[:B], idx[:n].reshape(shape), sc[:n].reshape(shape),
            None if ks is None else ks[:n].reshape(shape))


def _check(ix, V, Q, thr, cap, metric, keys=None, mask=None, index_offset=0, what=""):
    """Call and compare with the oracle; returns the counts."""
    Q = np.asarray(Q, np.float32).reshape(-1, V.shape[1])
    keys = rc.oracle_keys(Q, V, metric) if keys is None else keys
    thr = np.broadcast_to(np.asarray(thr, np.float64), (Q.shape[0],))
    ec, ei, es, ek = rc.expected(keys, rc.kt_of(metric, thr), cap, metric, mask, index_offset)
    code, c, i, s, k = _call(ix, Q, thr, cap, None if mask is None else rc.words(mask), index_offset)
    assert code == 0, f"status {code} {what}"
    np.testing.assert_array_equal(c, ec, err_msg=f"counts {what}")
    np.testing.assert_array_equal(i, ei, err_msg=f"indices {what}")
    np.testing.assert_array_equal(k, ek, err_msg=f"keys {what}")
    np.testing.assert_array_equal(s, es, err_msg=f"scores {what}")
    return c


def _spread_thresholds(keys, metric, lo=3, step=7):
    """A different midpoint threshold per query (query b passes lo + step b rows, within N)."""
    n = keys.shape[1]
    return np.array([rc.midpoint_threshold(keys[b], min(lo + step * b, n), metric) for b in range(keys.shape[0])])


# =============================================================================
# shapes
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 33, 100, 256, 260, 768, 1536, 2100])
def test_dims(vdb, dim, metric):
    n = 1100
    V, Q = rc.corpus(n, dim)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:3], V, metric)
    if dim == 1 and metric == "cosine":  # keys are +-1: the thresholds between and beyond them
        thr = np.array([0.0, 1.0, 1.5])
    else:
        thr = _spread_thresholds(keys, metric, lo=5, step=40)
    _check(ix, V, Q[:3], thr, 64, metric, keys, what=f"dim {dim}")
    _check(ix, V, Q[:3], thr, 0, metric, keys, what=f"dim {dim} count only")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, WG_ROWS - 1, WG_ROWS, WG_ROWS + 1])
def test_row_counts(vdb, n, metric):
    V, Q = rc.corpus(n, 100)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:3], V, metric)
    every = -np.inf if metric == "cosine" else np.inf
    thr = np.array([every, rc.midpoint_threshold(keys[1], (n + 1) // 2, metric),
                    rc.midpoint_threshold(keys[2], n - 1, metric)])
    c = _check(ix, V, Q[:3], thr, n + 2, metric, keys, what=f"n {n}")
    assert c.tolist() == [n, (n + 1) // 2, n - 1]
    _check(ix, V, Q[:3], thr, max(n // 2, 1), metric, keys, what=f"n {n} truncated")
    ix.close()


EMIT_ROWS = 8192      # rows per emit workgroup: 32 x csrc/vdb_range_plan.h kRangeEmitWords
PREFIX_ROWS = 131072  # rows per round of the prefix kernel's carry loop: 256 chunks of kRangeWgRows
SCORE_SLOTS = 16384   # slots per trip of the score kernel's strided loops: 4 x kRangeScoreWgs


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [EMIT_ROWS - 1, EMIT_ROWS, EMIT_ROWS + 1, PREFIX_ROWS + 1 + WG_ROWS,
                               2 * PREFIX_ROWS + 3 * WG_ROWS + 7])
def test_row_counts_past_one_emit_workgroup(vdb, n, metric):
    """The edges the small corpora never reach: a second emit workgroup (its chunk lookup and its
    early return once the prefix is at or past cap), a second and third round of the prefix
    kernel's carry loop, and caps past one trip of the score kernel's strided loops.  Query 0
    passes every row (slot p holds row p: hits on both sides of every boundary), query 1 a third
    of the rows spread over all of them, query 2 five rows."""
    V, Q = rc.corpus(n, 8)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:3], V, metric)
    every = -np.inf if metric == "cosine" else np.inf
    third = n // 3
    thr = np.array([every, rc.midpoint_threshold(keys[1], third, metric), rc.midpoint_threshold(keys[2], 5, metric)])
    # caps before, at, inside and after the second emit workgroup (for query 0; query 1 reaches its
    # cap about three times as far into the rows), past one trip of the score loops, around the
    # counts and past N
    caps = {1, 100, EMIT_ROWS - 1, EMIT_ROWS, EMIT_ROWS + 1, EMIT_ROWS + 100, SCORE_SLOTS + 1, third - 1, third,
            third + 1, n - 1, n, n + 3}
    if n > PREFIX_ROWS:
        caps |= {PREFIX_ROWS - 1, PREFIX_ROWS, PREFIX_ROWS + 1, 3 * SCORE_SLOTS + 5}
    for cap in sorted(c for c in caps if c >= 1):
        c = _check(ix, V, Q[:3], thr, cap, metric, keys, what=f"n {n} cap {cap}")
        assert c.tolist() == [n, third, 5]
    assert _check(ix, V, Q[:3], thr, 0, metric, keys, what=f"n {n} count only").tolist() == [n, third, 5]
    # a mask that leaves only rows at and beyond the first emit workgroup's last row
    mask = np.zeros(n, bool)
    mask[EMIT_ROWS - 1:] = True
    mask[::7] = False
    _check(ix, V, Q[:3], thr, 50, metric, keys, mask=mask, what=f"n {n} masked")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [100, 1536])
def test_batch_sizes(vdb, dim, metric):
    blk = rc.query_block(dim)
    n = 700
    sizes = [1, 2, blk - 1, blk, blk + 1, 2 * blk + 3]
    V, Q = rc.corpus(n, dim, n_queries=2 * 64 + 3)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:max(sizes)], V, metric)
    thr = _spread_thresholds(keys, metric, lo=0, step=5)  # neighbouring queries' words differ
    for B in sizes:
        c = _check(ix, V, Q[:B], thr[:B], 40, metric, keys[:B], what=f"dim {dim} B {B}")
        assert c.tolist() == [min(5 * b, n) for b in range(B)]
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_caps(vdb, metric):
    n, count = 1500, 200
    V, Q = rc.corpus(n, 100)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:2], V, metric)
    thr = np.array([rc.midpoint_threshold(keys[0], count, metric), rc.midpoint_threshold(keys[1], 3, metric)])
    for cap in (0, 1, count - 1, count, count + 1, n):
        c = _check(ix, V, Q[:2], thr, cap, metric, keys, what=f"cap {cap}")
        assert c.tolist() == [count, 3]  # exact at every cap
    # count only with NULL list pointers
    code, c, _, _, _ = _call(ix, Q[:2], thr, 0, null_lists=True)
    assert code == 0 and c.tolist() == [count, 3]
    # the midpoint cases around a cap
    cap = 10
    for m in rc.midpoint_ms(n, cap):
        t = rc.midpoint_threshold(keys[0], m, metric)
        c = _check(ix, V, Q[:1], [t], cap, metric, keys[:1], what=f"midpoint m {m}")
        assert c[0] == m
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", rc.DENSITIES)
def test_hit_density(vdb, name, metric):
    for n in (WG_ROWS + 1, 1000):
        V, q, rows, t = rc.density_case(name, n, metric)
        ix = _index(vdb, V, metric)
        c = _check(ix, V, q, [t], n, metric, what=f"{name} n {n}")
        assert c[0] == rows.size
        _check(ix, V, q, [t], 7, metric, what=f"{name} n {n} cap 7")
        ix.close()


# =============================================================================
# equality
# =============================================================================
@pytest.mark.parametrize("dim", [1, 33, 100, 768])
def test_cosine_equality(vdb, dim):
    n = 700
    V, Q = rc.corpus(n, dim)
    ix = _index(vdb, V, "cosine")
    keys = rc.oracle_keys(Q[:1], V, "cosine")
    t_in, t_out = rc.cosine_equality(keys[0], 123)
    c = _check(ix, V, np.repeat(Q[:1], 2, axis=0), [t_in, t_out], n, "cosine", np.repeat(keys, 2, axis=0))
    assert c[0] - c[1] == np.count_nonzero(keys[0] == keys[0, 123]) >= 1
    ix.close()


@pytest.mark.parametrize("dim", [1, 2, 33, 100, 260, 1536])
def test_euclidean_equality(vdb, dim):
    n = 600
    V, q, planted = rc.euclid_equality_case(n, dim)
    ix = _index(vdb, V, "euclidean")
    t_out = np.nextafter(rc.EUCLID_RADIUS, 0.0)
    code, c, i, s, k = _call(ix, np.stack([q, q]), [rc.EUCLID_RADIUS, t_out], n)
    assert code == 0 and c[0] - c[1] == planted.size
    assert set(planted) <= set(i[0, :c[0]]) and not set(planted) & set(i[1, :c[1]])
    at = np.isin(i[0, :c[0]], planted)
    np.testing.assert_array_equal(k[0, :c[0]][at], -rc.EUCLID_SQ)
    np.testing.assert_array_equal(s[0, :c[0]][at], np.float32(rc.EUCLID_RADIUS))
    _check(ix, V, np.stack([q, q]), [rc.EUCLID_RADIUS, t_out], n, "euclidean")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_duplicates(vdb, metric):
    n = 900
    V, Q, groups = rc.duplicates_case(n, 100)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:1], V, metric)
    for g in groups:
        key = keys[0, g[0]]
        t = float(key) if metric == "cosine" else float(np.sqrt(-key)) * (1 + 1e-9)
        code, c, i, s, k = _call(ix, Q[:1], [t], n)
        assert code == 0 and set(g) <= set(i[0, :c[0]])  # equal keys: all of them are in
        _check(ix, V, Q[:1], [t], n, metric, keys)
    ix.close()


# =============================================================================
# mask, offset, precision
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_mask_and_offset(vdb, metric):
    n = 1300
    V, Q = rc.corpus(n, 100)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:3], V, metric)
    thr = _spread_thresholds(keys, metric, lo=150, step=200)
    rng = np.random.default_rng(5)
    single = np.zeros(n, bool)
    single[777] = True
    passing = keys[0] >= rc.kt_of(metric, thr[:1])[0]
    masks = {"random": rng.random(n) < 0.4, "all-zero": np.zeros(n, bool), "single": single, "passing only": passing}
    for name, m in masks.items():
        c = _check(ix, V, Q[:3], thr, 500, metric, keys, mask=m, what=f"mask {name}")
        if name == "all-zero":
            assert (c == 0).all()
        if name == "passing only":
            assert c[0] == np.count_nonzero(passing) == 150
    every = np.array([-np.inf if metric == "cosine" else np.inf])
    c = _check(ix, V, Q[:1], every, n, metric, keys[:1], mask=single, what="single bit, every row passes")
    assert c[0] == 1
    # stray bits at or past the count in the last word are ignored
    w = rc.words(masks["random"])
    w[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32)
    code, c2, i2, _, _ = _call(ix, Q[:3], thr, 500, mask=w)
    ec, ei, _, _ = rc.expected(keys, rc.kt_of(metric, thr), 500, metric, masks["random"])
    np.testing.assert_array_equal(c2, ec)
    np.testing.assert_array_equal(i2, ei)
    _check(ix, V, Q[:3], thr, 500, metric, keys, index_offset=10 ** 12, what="index_offset")
    _check(ix, V, Q[:3], thr, 100, metric, keys, mask=masks["random"], index_offset=4096, what="mask + offset")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_precision_settings_give_identical_bytes(vdb, metric):
    n = 2000
    V, Q = rc.corpus(n, 128)
    keys = rc.oracle_keys(Q[:4], V, metric)
    thr = _spread_thresholds(keys, metric, lo=1, step=90)
    ref = None
    for prec in ("auto", "i8", "bf16x3", "fp32"):
        ix = _index(vdb, V, metric, precision=prec)
        names = [f"searches_{p}" for p in ("fp32", "bf16x3", "bf16", "i8", "i8x3", "i8q")] + ["searches", "queries"]
        before = [ix.stat(s) for s in names]
        _check(ix, V, Q[:4], thr, 300, metric, keys, what=f"precision {prec}")
        got = _call(ix, Q[:4], thr, 300)
        assert [ix.stat(s) for s in names] == before, "a searches_* stat moved"
        assert ix.stat("range_searches") == 2 and ix.stat("range_queries") == 8
        blob = b"".join(a.tobytes() for a in got[1:])
        assert ref is None or blob == ref, f"precision {prec} differs"
        ref = blob
        ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_cross_check_against_search(vdb, metric):
    n = 3000
    V, Q = rc.corpus(n, 64)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:3], V, metric)
    for b, count in enumerate((1, 37, 1024)):
        t = rc.midpoint_threshold(keys[b], count, metric)
        code, c, i, s, k = _call(ix, Q[b], [t], 1024)
        assert code == 0 and c[0] == count
        ri, rs, rk = rc.best_first(c[0], i[0], s[0], k[0])
        ss, si, sk = ix.search(Q[b], count, with_keys=True)
        np.testing.assert_array_equal(ri, si[0])
        np.testing.assert_array_equal(rk, sk[0])
        np.testing.assert_array_equal(rs, ss[0])
    ix.close()


def test_binding(vdb):
    """NativeIndex.search_range: scalar broadcast, cap=None's second call, with and without keys."""
    n = 2500
    V, Q = rc.corpus(n, 48)
    ix = _index(vdb, V, "cosine")
    keys = rc.oracle_keys(Q[:3], V, "cosine")
    for count in (10, 1500):  # within the first call's capacity, and past it
        t = rc.midpoint_threshold(keys[0], count, "cosine")
        c, i, s, k = ix.search_range(Q[:3], t, with_keys=True)
        width = max(int(c.max()), 1024) if c.max() > 1024 else 1024
        ec, ei, es, ek = rc.expected(keys, np.full(3, t), width, "cosine")
        assert c[0] == count and i.shape == (3, width)
        for got, want in ((c, ec), (i, ei), (s, es), (k, ek)):
            np.testing.assert_array_equal(got, want)
        c2, i2, s2 = ix.search_range(Q[:3], [t] * 3, cap=5)
        np.testing.assert_array_equal(c2, ec)
        np.testing.assert_array_equal(i2, ei[:, :5])
    c0, i0, s0 = ix.search_range(Q[0], 0.0, cap=0)
    assert i0.shape == (1, 0) and c0[0] == np.count_nonzero(keys[0] >= 0.0)
    with pytest.raises(ValueError):
        ix.search_range(Q[:3], [0.1, 0.2])
    with pytest.raises(ValueError):
        ix.search_range(Q[:3, :5], 0.1)
    ix.close()


# =============================================================================
# device memory
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_device_memory(vdb, metric):
    import torch
    n, B, cap = 1700, 5, 128
    V, Q = rc.corpus(n, 100)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:B], V, metric)
    thr = _spread_thresholds(keys, metric, lo=2, step=60)
    bad = thr.copy()
    bad[1] = np.nan
    bad[3] = np.nan if metric == "cosine" else -1.0  # a negative radius
    mask = np.random.default_rng(3).random(n) < 0.5
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    for t, m in ((thr, None), (thr, mask), (bad, None)):
        with torch.cuda.stream(st):
            dq = torch.from_numpy(Q[:B].copy()).to(dev)
            dt = torch.from_numpy(t.copy()).to(dev)
            dm = torch.from_numpy(rc.words(m).view(np.int32)).to(dev) if m is not None else None
            dc = torch.full((B + GUARD,), S_CNT, dtype=torch.int64, device=dev)
            di = torch.full((B * cap + GUARD,), S_IDX, dtype=torch.int64, device=dev)
            ds = torch.full((B * cap + GUARD,), float("nan"), dtype=torch.float32, device=dev)
            dk = torch.full((B * cap + GUARD,), float("nan"), dtype=torch.float64, device=dev)
            ix.search_range_device(dq.data_ptr(), B, dt.data_ptr(), cap, dc.data_ptr(), di.data_ptr(), ds.data_ptr(),
                                   dk.data_ptr(), mask_ptr=dm.data_ptr() if dm is not None else 0,
                                   stream=st.cuda_stream)
            dc0 = torch.full((B + GUARD,), S_CNT, dtype=torch.int64, device=dev)
            ix.search_range_device(dq.data_ptr(), B, dt.data_ptr(), 0, dc0.data_ptr(),
                                   mask_ptr=dm.data_ptr() if dm is not None else 0, stream=st.cuda_stream)
        st.synchronize()
        invalid = np.isnan(t) | ((t < 0) if metric == "euclidean" else False)
        kt = rc.kt_of(metric, np.where(invalid, np.nan, t))  # an invalid threshold passes nothing
        ec, ei, es, ek = rc.expected(keys, kt, cap, metric, m)
        c, i, s, k = (x.cpu().numpy() for x in (dc, di, ds, dk))
        np.testing.assert_array_equal(c[:B], ec)
        np.testing.assert_array_equal(dc0.cpu().numpy()[:B], ec)
        np.testing.assert_array_equal(i[:B * cap].reshape(B, cap), ei)
        np.testing.assert_array_equal(s[:B * cap].reshape(B, cap), es)
        np.testing.assert_array_equal(k[:B * cap].reshape(B, cap), ek)
        assert (c[B:] == S_CNT).all() and (i[B * cap:] == S_IDX).all()
        assert np.isnan(s[B * cap:]).all() and np.isnan(k[B * cap:]).all()
        if t is bad:
            assert ec[1] == 0 and ec[3] == 0 and ec[0] > 0 and ec[2] > 0 and ec[4] > 0
    ix.close()


# =============================================================================
# index states
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_empty_index(vdb, metric):
    V, Q = rc.corpus(10, 40)
    ix = vdb.NativeIndex(40, metric)
    for cap in (0, 3):
        code, c, i, s, k = _call(ix, Q[:2], [0.5, 0.5], cap)
        assert code == 0 and (c == 0).all()
        assert (i == -1).all() and (s == 0).all() and np.isneginf(k).all()
    ix.add(V)
    ix.clear()
    code, c, i, s, k = _call(ix, Q[:2], [0.5, 0.5], 3, mask=np.zeros(1, np.uint32))
    assert code == 0 and (c == 0).all() and (i == -1).all()
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_after_mutation(vdb, metric):
    n = 1200
    V, Q = rc.corpus(n, 72)
    V2, _ = rc.corpus(300, 72, seed=9)
    ix = _index(vdb, V, metric)
    cur = V.copy()
    thr = None
    for step in ("remove", "update", "add"):
        if step == "remove":
            gone = np.zeros(n, bool)
            gone[np.random.default_rng(1).choice(n, 173, replace=False)] = True
            ix.remove(rc.words(gone))
            cur = cur[~gone]
        elif step == "update":
            ids = np.array([0, 5, cur.shape[0] - 1, 400], np.int64)
            ix.update(ids, V2[:4])
            cur[ids] = V2[:4]
        else:
            ix.add(V2)
            cur = np.concatenate([cur, V2])
        assert ix.count() == cur.shape[0]
        keys = rc.oracle_keys(Q[:3], cur, metric)
        thr = _spread_thresholds(keys, metric, lo=20, step=100)
        _check(ix, cur, Q[:3], thr, 256, metric, keys, what=f"after {step}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_concurrent_with_searches(vdb, metric):
    n = 2000
    V, Q = rc.corpus(n, 96)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:4], V, metric)
    thr = _spread_thresholds(keys, metric, lo=10, step=50)
    want = rc.expected(keys, rc.kt_of(metric, thr), 200, metric)
    want_s = ref_cpu.exact_search(Q[:4], V, 10, metric)
    errors = []

    def work(t):
        try:
            for _ in range(6):
                if t % 2 == 0:
                    code, c, i, s, k = _call(ix, Q[:4], thr, 200)
                    assert code == 0
                    for got, exp in zip((c, i, s, k), want):
                        np.testing.assert_array_equal(got, exp)
                else:
                    s, i, k = ix.search(Q[:4], 10, with_keys=True)
                    for got, exp in zip((s, i, k), want_s):
                        np.testing.assert_array_equal(got, exp)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    ix.close()


# =============================================================================
# errors
# =============================================================================
def test_errors(vdb):
    from service._vdb import VDB_ERR_INVALID, VDB_ERR_NONFINITE
    n = 300
    V, Q = rc.corpus(n, 24)
    for metric in METRICS:
        ix = _index(vdb, V, metric)
        assert _call(ix, Q[:2], [0.1, 0.2], 4)[0] == 0
        stats = (ix.stat("range_searches"), ix.stat("range_queries"))
        assert stats == (1, 2)
        qn = Q[:2].copy()
        qn[1, 3] = np.nan
        qi = Q[:2].copy()
        qi[0, 0] = np.inf
        assert _call(ix, qn, [0.1, 0.2], 4)[0] == VDB_ERR_NONFINITE
        assert _call(ix, qi, [0.1, 0.2], 4)[0] == VDB_ERR_NONFINITE
        assert _call(ix, Q[:2], [0.1, np.nan], 4)[0] == VDB_ERR_INVALID
        assert _call(ix, Q[:2], [0.1, 0.2], -1)[0] == VDB_ERR_INVALID
        assert _call(ix, Q[:2], [0.1, 0.2], 4, null_lists=True)[0] == VDB_ERR_INVALID
        neg = _call(ix, Q[:2], [0.1, -0.5], 4)
        assert neg[0] == (VDB_ERR_INVALID if metric == "euclidean" else 0)  # a negative similarity is a threshold
        thr = np.array([0.1, 0.2])
        counts = np.zeros(2, np.int64)
        assert ix._lib.vdb_index_search_range(ix._h, _p(np.ascontiguousarray(Q[:2])), 2, _p(thr), None, 7, 0,
                                              _p(counts), None, None, None, 0, None) == VDB_ERR_INVALID  # bad mem
        assert ix._lib.vdb_index_search_range(ix._h, _p(np.ascontiguousarray(Q[:2])), 2, _p(thr), None, 0, 0,
                                              None, None, None, None, 0, None) == VDB_ERR_INVALID  # no counts
        assert ix._lib.vdb_index_search_range(ix._h, _p(np.ascontiguousarray(Q[:2])), 0, _p(thr), None, 0, 0,
                                              None, None, None, None, 0, None) == 0  # no queries
        with pytest.raises(ValueError):
            ix.search_range(Q[:2], [0.1, np.nan])
        with pytest.raises(ValueError):
            ix.search_range(Q[:2], 0.1, cap=-3)
        extra = 1 if metric == "cosine" else 0  # the negative cosine threshold was a valid call
        assert (ix.stat("range_searches"), ix.stat("range_queries")) == (stats[0] + extra, stats[1] + 2 * extra)
        # failed calls wrote nothing
        code, c, i, s, k = _call(ix, qn, [0.1, 0.2], 4)
        assert (c == S_CNT).all() and (i == S_IDX).all() and np.isnan(s).all() and np.isnan(k).all()
        ix.close()

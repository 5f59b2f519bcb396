"""Grouped search (include/vdb.h vdb_index_set_groups / vdb_index_search_groups; csrc/vdb_group.hip).

The contract: slot j of query b holds the best row of the j-th best group -- groups ranked by (best
canonical fp64 key desc, best row asc) over the rows whose group id is >= 0 and whose mask bit is
set -- with its fp32 score, fp64 key and group id; slots past the number of eligible groups hold
-1 / 0 / -inf / -1.  Every case compares all four outputs with the oracle statement of
tests/_group_cases.py (preconditions: tests/test_group_precondition.py) with
``assert_array_equal``; no tolerance appears anywhere.  Every case also asserts that the stat
"group_fallback_queries" moved by exactly ``len(flagged)``: the queries with fewer than k groups
among their best k' eligible rows although more than k' rows are eligible.

Every host call goes through ``_call``: the four output arrays carry a guard region past [B][k]
filled with a sentinel, which must be untouched afterwards.

Shapes are the smallest at which the kernels can go wrong: dims that leave pad columns (1, 33, 100),
one 256-dim piece plus 4 (260), three pieces (768) and rows too long to hold (2100: the any-length
key form of the fallback); row counts around a mask word, a fallback segment (1024 rows) and past
four segments; 70 000 rows of 32 and of 128 dims, the latter through the wide int8 pass.
"""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _group_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 257
S_IDX, S_GRP = -7, -9
METRICS = gc.METRICS
VDB_ERR_INVALID = -1


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def _index(vdb, V, metric, groups=None, precision=None):
    ix = vdb.NativeIndex(V.shape[1], metric, precision=precision)
    if V.shape[0]:
        ix.add(V)
    assert ix.count() == V.shape[0]
    if groups is not None:
        ix.set_groups(groups)
    return ix


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _call(ix, Q, k, mask=None, index_offset=0, with_keys=True, null_groups=False):
    """The C-ABI call in host memory with guarded outputs -> (rc, scores, idx, groups, keys)."""
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    B = Q.shape[0]
    n = B * max(k, 0)
    sc = np.full(n + GUARD, np.nan, np.float32)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    gr = np.full(n + GUARD, S_GRP, np.int32)
    ks = np.full(n + GUARD, np.nan, np.float64) if with_keys else None
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    code = ix._lib.vdb_index_search_groups(ix._h, _p(Q), B, k, _p(m), 0, _p(sc), _p(idx),
                                           None if null_groups else _p(gr), _p(ks), index_offset, None)
    assert np.isnan(sc[n:]).all(), "scores guard touched"
    assert (idx[n:] == S_IDX).all(), "indices guard touched"
    assert (gr[n:] == S_GRP).all(), "groups guard touched"
    assert ks is None or np.isnan(ks[n:]).all(), "keys guard touched"
    shape = (B, max(k, 0))
    return (code, sc[:n].reshape(shape), idx[:n].reshape(shape), gr[:n].reshape(shape),
            None if ks is None else ks[:n].reshape(shape))


def _check(ix, keys, Q, groups, k, metric, knob=0, mask=None, index_offset=0, what=""):
    """Call and compare with the oracle; asserts the fallback count; returns the flagged queries."""
    Q = np.asarray(Q, np.float32).reshape(-1, ix.dim)
    ix.set_param("group_fetch", knob)
    es, ei, eg, ek = gc.expected(keys, groups, k, metric, mask, index_offset)
    fl = gc.flagged(keys, groups, mask, k, gc.fetch_k(knob, k))
    before = ix.stat("group_fallback_queries")
    code, s, i, g, kk = _call(ix, Q, k, None if mask is None else gc.bitmap_words(mask), index_offset)
    assert code == 0, f"status {code} {what}: {ix._lib.vdb_last_error()}"
    moved = ix.stat("group_fallback_queries") - before  # (the stat waits for the queued work)
    np.testing.assert_array_equal(i, ei, err_msg=f"indices {what}")
    np.testing.assert_array_equal(g, eg, err_msg=f"groups {what}")
    np.testing.assert_array_equal(kk, ek, err_msg=f"keys {what}")
    np.testing.assert_array_equal(s, es, err_msg=f"scores {what}")
    assert moved == len(fl), f"{moved} queries took the fallback, {len(fl)} must ({what})"
    return fl


# =============================================================================
# shapes
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 33, 100, 260, 768, 2100])
def test_dims(vdb, dim, metric):
    n = 1100
    V, Q, g = gc.fast_case(n, dim)
    ix = _index(vdb, V, metric, g)
    keys = gc.oracle_keys(Q[:3], V, metric)
    _check(ix, keys, Q[:3], g, 5, metric, what=f"dim {dim}")
    _check(ix, keys, Q[:3], g, 9, metric, knob=32, what=f"dim {dim} k past the groups")  # the fallback
    ix.set_param("group_force_exact", 1)
    code, s, i, gg, kk = _call(ix, Q[:3], 5)
    es, ei, eg, ek = gc.expected(keys, g, 5, metric)
    for got, want in ((s, es), (i, ei), (gg, eg), (kk, ek)):
        np.testing.assert_array_equal(got, want)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 511, 512, 513, 4097])
def test_row_counts(vdb, n, metric):
    V, Q, g = gc.fast_case(n, 100, "modulo")
    ix = _index(vdb, V, metric, g)
    keys = gc.oracle_keys(Q[:3], V, metric)
    G = gc.n_groups(g)
    for k, knob in gc.fast_settings(G):
        _check(ix, keys, Q[:3], g, k, metric, knob=knob, what=f"n {n} k {k} fetch {knob}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [32, 128])
def test_many_rows(vdb, dim, metric):
    """70 000 rows, past the row count from which the inner fetch may take the wide int8 pass.  That
    pass reads rows of four 32-dim groups, so the 128-dim corpus takes it (asserted) and the 32-dim
    one, padded to 64 dims, takes the ordinary int8 pass; k' = 40 and 200."""
    n = 70000
    V, Q, _ = gc.fast_case(n, dim, n_queries=6)
    g = (np.arange(n) % 3000).astype(np.int32)
    ix = _index(vdb, V, metric, g)
    keys = gc.oracle_keys(Q[:6], V, metric)
    before = ix.stat("searches_wide")
    _check(ix, keys, Q[:6], g, 10, metric, knob=40, what="many rows")
    _check(ix, keys, Q[:6], g, 128, metric, knob=200, what="many rows k 128")
    if dim == 128:
        assert ix.stat("searches_wide") > before, "the inner fetch did not take the wide int8 pass"
    ix.close()


# =============================================================================
# group layouts
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", gc.LAYOUTS)
def test_layouts(vdb, name, metric):
    n = 1500
    V, Q, _ = gc.fast_case(n, 64)
    g = gc.layout(name, n)
    ix = _index(vdb, V, metric, g)
    keys = gc.oracle_keys(Q[:4], V, metric)
    G = gc.n_groups(g)
    for k in sorted({1, 2, max(G, 1), G + 1, 128} & set(range(1, 129))):
        _check(ix, keys, Q[:4], g, k, metric, what=f"layout {name} k {k}")
    if name == "all_negative":
        code, s, i, gg, kk = _call(ix, Q[:4], 3)
        assert (i == -1).all() and (gg == -1).all() and (s == 0).all() and np.isneginf(kk).all()
    assert ix.stat("group_rows") == n
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_duplicated_rows(vdb, metric):
    n = 700
    V, Q, g, (a, b), (c, e) = gc.duplicates_case(n, 48)
    ix = _index(vdb, V, metric, g)
    keys = gc.oracle_keys(Q[:2], V, metric)
    for knob in (0, 3):  # k' = 32, and k' = k
        _check(ix, keys, Q[:2], g, 3, metric, knob=knob, what="duplicates")
    code, s, i, gg, kk = _call(ix, Q[:2], 3)
    assert i[0, 0] == a and i[0, 1] == b and kk[0, 0] == kk[0, 1], "equal keys: the lower row's group first"
    assert i[1, 0] == c and e not in i[1], "copies in one group: the lower row, once"
    ix.set_param("group_force_exact", 1)
    code, s2, i2, g2, k2 = _call(ix, Q[:2], 3)
    np.testing.assert_array_equal(i2, i)
    np.testing.assert_array_equal(g2, gg)
    ix.close()


# =============================================================================
# the fallback
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("batch", gc.DOM_BATCHES)
def test_dominant_group(vdb, batch, metric):
    n = 3000
    V, Q, g, hot = gc.dominant_case(n, 40, batch)
    ix = _index(vdb, V, metric, g)
    keys = gc.oracle_keys(Q, V, metric)
    fl = _check(ix, keys, Q, g, gc.DOM_K, metric, knob=gc.DOM_FETCH, what=f"dominant B {batch}")
    assert fl == list(hot)
    assert _check(ix, keys, Q, g, gc.DOM_K, metric, knob=200, what=f"dominant B {batch}, k' 200") == []
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_force_exact_gives_the_same_bytes(vdb, metric):
    n = 4097  # five fallback segments
    V, Q, g = gc.fast_case(n, 100, "random")
    ix = _index(vdb, V, metric, g)
    mask = np.random.default_rng(5).random(n) < 0.6
    for k, m in ((1, None), (4, None), (7, mask), (128, mask)):
        ix.set_param("group_force_exact", 0)
        ref = _call(ix, Q[:4], k, None if m is None else gc.bitmap_words(m))
        before = ix.stat("group_fallback_queries")
        ix.set_param("group_force_exact", 1)
        got = _call(ix, Q[:4], k, None if m is None else gc.bitmap_words(m))
        assert ix.stat("group_fallback_queries") - before == 4
        assert ref[0] == 0 and got[0] == 0
        for x, y in zip(ref[1:], got[1:]):
            assert x.tobytes() == y.tobytes()
    ix.close()


# =============================================================================
# masks, offset, precision, metric
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_masks(vdb, metric):
    n = 1500
    V, Q, _ = gc.fast_case(n, 64)
    rng = np.random.default_rng(11)
    keys = gc.oracle_keys(Q[:4], V, metric)
    few = np.zeros(n, bool)
    few[rng.choice(n, 20, replace=False)] = True  # fewer than k' = 32 eligible: complete without the fallback
    exactly = np.zeros(n, bool)
    exactly[rng.choice(n, 32, replace=False)] = True  # exactly k' eligible
    masks = {"random": rng.random(n) < 0.5, "few": few, "exactly_fetch": exactly, "none": np.zeros(n, bool),
             "last_word": np.arange(n) >= (n // 32) * 32}
    for lname in ("random", "some_negative"):
        g = gc.layout(lname, n)
        ix = _index(vdb, V, metric, g)
        for mname, m in masks.items():
            for k in (3, 9):
                fl = _check(ix, keys, Q[:4], g, k, metric, knob=32, mask=m, what=f"{lname} mask {mname} k {k}")
                if mname in ("few", "exactly_fetch", "none", "last_word"):
                    assert fl == []
        _check(ix, keys, Q[:4], g, 4, metric, mask=masks["random"], index_offset=1 << 40, what="mask + offset")
        _check(ix, keys, Q[:4], g, 4, metric, index_offset=12345, what="offset")
        ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_mask_bits_past_count_are_ignored(vdb, metric):
    """A caller mask whose last word has bits set at and past ``count``: they name no row, so they
    must neither be returned nor counted as eligible.  Exactly k' = 32 real rows are eligible and
    hold fewer than k groups: complete without the fallback, which a count of 36 would flag."""
    n = 1500  # the last word covers rows 1472..1503
    V, Q, g = gc.fast_case(n, 64, "random")
    ix = _index(vdb, V, metric, g)
    keys = gc.oracle_keys(Q[:4], V, metric)
    rng = np.random.default_rng(13)
    for m in (np.ones(n, bool), None):
        if m is None:
            m = np.zeros(n, bool)
            m[rng.choice(n - 40, 30, replace=False)] = True
            m[[n - 2, n - 1]] = True  # 32 eligible rows, two of them in the last word
        words = gc.bitmap_words(m)
        words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # rows 1500..1503
        for k in (3, 9):
            es, ei, eg, ek = gc.expected(keys, g, k, metric, m)
            fl = gc.flagged(keys, g, m, k, 32)
            ix.set_param("group_fetch", 32)
            before = ix.stat("group_fallback_queries")
            code, s, i, gg, kk = _call(ix, Q[:4], k, words)
            assert code == 0
            for got, want in ((i, ei), (gg, eg), (kk, ek), (s, es)):
                np.testing.assert_array_equal(got, want)
            assert ix.stat("group_fallback_queries") - before == len(fl)
            assert m.all() or fl == []
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_fallback_at_the_segment_cap(vdb, metric):
    """270 331 rows: the exact fallback runs its most segments (256, csrc/vdb_group_plan.h
    kGroupMaxSeg), of 1 056 rows each, every one with rows and the last one short; 8 dims keep corpus
    and oracle cheap."""
    n = 256 * 1056 - 5
    V, Q, _ = gc.fast_case(n, 8, n_queries=3)
    g = (np.arange(n) % 41).astype(np.int32)
    g[::97] = -1
    ix = _index(vdb, V, metric, g)
    keys = gc.oracle_keys(Q[:3], V, metric)
    mask = np.random.default_rng(7).random(n) < 0.5
    for k, m in ((5, None), (41, mask), (128, None)):
        # k = 128 > 41 groups: flagged by the select; the others forced
        ix.set_param("group_force_exact", 0 if k == 128 else 1)
        es, ei, eg, ek = gc.expected(keys, g, k, metric, m)
        before = ix.stat("group_fallback_queries")
        code, s, i, gg, kk = _call(ix, Q[:3], k, None if m is None else gc.bitmap_words(m))
        assert code == 0
        for got, want in ((i, ei), (gg, eg), (kk, ek), (s, es)):
            np.testing.assert_array_equal(got, want)
        assert ix.stat("group_fallback_queries") - before == 3
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_precision_settings_give_identical_bytes(vdb, metric):
    n = 2000
    V, Q, g = gc.fast_case(n, 128, "some_negative")
    keys = gc.oracle_keys(Q[:4], V, metric)
    ref = None
    for prec in ("auto", "i8", "i8x3", "i8q", "bf16", "bf16x3", "fp32"):  # service/_vdb.py PRECISION_IDS, all seven
        ix = _index(vdb, V, metric, g, precision=prec)
        _check(ix, keys, Q[:4], g, 5, metric, what=f"precision {prec}")
        _check(ix, keys, Q[:4], g, 8, metric, knob=8, what=f"precision {prec}, fallback")
        got = _call(ix, Q[:4], 5)
        blob = b"".join(a.tobytes() for a in got[1:])
        assert ref is None or blob == ref, f"precision {prec} differs"
        ref = blob
        ix.close()


# =============================================================================
# device memory, concurrency
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_device_memory(vdb, metric):
    import torch
    n, B, k = 3000, 5, gc.DOM_K
    V, Q, g, hot = gc.dominant_case(n, 40, B)
    ix = vdb.NativeIndex(40, metric)
    ix.add(V)
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dg = torch.from_numpy(g.copy()).to(dev)
        ix.set_groups_device(dg.data_ptr(), n, stream=st.cuda_stream)
    ix.set_param("group_fetch", gc.DOM_FETCH)
    mask = np.random.default_rng(3).random(n) < 0.7
    for m in (None, mask):
        host = _call(ix, Q, k, None if m is None else gc.bitmap_words(m))
        assert host[0] == 0
        before = ix.stat("group_fallback_queries")
        with torch.cuda.stream(st):
            dq = torch.from_numpy(Q.copy()).to(dev)
            dm = torch.from_numpy(gc.bitmap_words(m).view(np.int32)).to(dev) if m is not None else None
            ds = torch.full((B * k + GUARD,), float("nan"), dtype=torch.float32, device=dev)
            di = torch.full((B * k + GUARD,), S_IDX, dtype=torch.int64, device=dev)
            dgr = torch.full((B * k + GUARD,), S_GRP, dtype=torch.int32, device=dev)
            dk = torch.full((B * k + GUARD,), float("nan"), dtype=torch.float64, device=dev)
            ix.search_groups_device(dq.data_ptr(), B, k, ds.data_ptr(), di.data_ptr(), dgr.data_ptr(), dk.data_ptr(),
                                    mask_ptr=dm.data_ptr() if dm is not None else 0, stream=st.cuda_stream)
        st.synchronize()
        keys = gc.oracle_keys(Q, V, metric)
        assert ix.stat("group_fallback_queries") - before == len(gc.flagged(keys, g, m, k, gc.DOM_FETCH))
        s, i, gg, kk = (x.cpu().numpy() for x in (ds, di, dgr, dk))
        for got, want in ((s, host[1]), (i, host[2]), (gg, host[3]), (kk, host[4])):
            np.testing.assert_array_equal(got[:B * k].reshape(B, k), want)
        assert np.isnan(s[B * k:]).all() and (i[B * k:] == S_IDX).all()
        assert (gg[B * k:] == S_GRP).all() and np.isnan(kk[B * k:]).all()
        es, ei, eg, ek = gc.expected(keys, g, k, metric, m)
        np.testing.assert_array_equal(host[2], ei)
        np.testing.assert_array_equal(host[3], eg)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_four_threads_agree(vdb, metric):
    n, B = 3000, 8
    V, Q, g, hot = gc.dominant_case(n, 40, B)
    ix = _index(vdb, V, metric, g)
    ix.set_param("group_fetch", gc.DOM_FETCH)
    keys = gc.oracle_keys(Q, V, metric)
    want = gc.expected(keys, g, gc.DOM_K, metric)
    errors = []

    def work(t):
        try:
            for _ in range(5):
                code, s, i, gg, kk = _call(ix, Q, gc.DOM_K)
                assert code == 0
                for got, exp in zip((s, i, gg, kk), want):
                    np.testing.assert_array_equal(got, exp)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert ix.stat("group_fallback_queries") == 20 * len(hot)
    ix.close()


# =============================================================================
# lifecycle, arguments, stats
# =============================================================================
def test_lifecycle(vdb):
    n = 600
    V, Q, g = gc.fast_case(n, 40, "random")
    V2, _ = gc.corpus(50, 40, seed=9)
    ix = _index(vdb, V, "cosine")
    assert ix.stat("group_rows") == 0
    assert _call(ix, Q[:2], 3)[0] == VDB_ERR_INVALID  # before any set_groups
    assert b"group column" in ix._lib.vdb_last_error()
    with pytest.raises(ValueError):
        ix.set_groups(g[:-1])  # a wrong n
    assert ix._lib.vdb_index_set_groups(ix._h, None, 5, 0, None) == VDB_ERR_INVALID
    ix.set_groups(g)
    assert ix.stat("group_rows") == n and ix.stat("group_sets") == 1
    keys = gc.oracle_keys(Q[:2], V, "cosine")
    _check(ix, keys, Q[:2], g, 3, "cosine", what="attached")
    # update keeps the column, and the updated row's new key decides
    cur = V.copy()
    cur[17] = Q[0] * 3.0
    ix.update(np.array([17]), cur[17:18])
    assert ix.stat("group_rows") == n
    keys = gc.oracle_keys(Q[:2], cur, "cosine")
    _check(ix, keys, Q[:2], g, 3, "cosine", what="after update")
    assert _call(ix, Q[:1], 3)[2][0, 0] == 17
    # add, remove and clear drop it
    ix.add(V2)
    assert ix.stat("group_rows") == 0 and _call(ix, Q[:2], 3)[0] == VDB_ERR_INVALID
    g2 = np.concatenate([g, np.full(50, 99, np.int32)])
    ix.set_groups(g2)
    assert _call(ix, Q[:2], 3)[0] == 0
    ix.remove(np.array([3, 4]))
    assert ix.stat("group_rows") == 0 and _call(ix, Q[:2], 3)[0] == VDB_ERR_INVALID
    ix.set_groups(np.delete(g2, [3, 4]))
    assert _call(ix, Q[:2], 3)[0] == 0
    ix.set_groups(None)  # detach
    assert ix.stat("group_rows") == 0 and _call(ix, Q[:2], 3)[0] == VDB_ERR_INVALID
    ix.set_groups(np.delete(g2, [3, 4]))
    ix.clear()
    assert _call(ix, Q[:2], 3)[0] == VDB_ERR_INVALID
    # an empty index with its empty column: every slot "no result"
    ix.set_groups(np.zeros(0, np.int32))
    code, s, i, gg, kk = _call(ix, Q[:2], 3)
    assert code == 0 and (i == -1).all() and (gg == -1).all() and (s == 0).all() and np.isneginf(kk).all()
    assert ix.stat("group_sets") == 5  # (a detach attaches nothing)
    ix.close()


def test_arguments_and_stats(vdb):
    n = 600
    V, Q, g = gc.fast_case(n, 40, "random")
    ix = _index(vdb, V, "euclidean", g)
    for k in (0, 129, -1):
        assert _call(ix, Q[:2], k)[0] == VDB_ERR_INVALID
    # more queries than one launch takes (65 535): refused before anything runs (no buffer is read)
    one = np.zeros(1, np.float32)
    assert ix._lib.vdb_index_search_groups(ix._h, _p(one), 65536, 3, None, 1, _p(one), _p(one), _p(one), None, 0,
                                           None) == VDB_ERR_INVALID
    assert b"65535" in ix._lib.vdb_last_error()
    assert _call(ix, Q[:2], 3, null_groups=True)[0] == VDB_ERR_INVALID
    bad = Q[:2].copy()
    bad[1, 3] = np.nan
    assert _call(ix, bad, 3)[0] != 0 and b"NaN" in ix._lib.vdb_last_error()
    assert ix._lib.vdb_index_search_groups(ix._h, None, 0, 3, None, 0, None, None, None, None, 0, None) == 0
    for name in ("group_searches", "group_queries", "searches", "queries", "group_fallback_queries"):
        assert ix.stat(name) == 0, name  # failed calls count nothing
    with pytest.raises(ValueError):
        ix.set_param("group_fetch", 201)
    with pytest.raises(ValueError):
        ix.set_param("group_force_exact", 2)
    code, s, i, gg = _call(ix, Q[:3], 4, with_keys=False)[:4]
    assert code == 0
    s2, i2, g2, k2 = ix.search_groups(Q[:3], 4, with_keys=True)  # the binding
    np.testing.assert_array_equal(i2, i)
    np.testing.assert_array_equal(g2, gg)
    np.testing.assert_array_equal(s2, s)
    before = ix.stat("group_fallback_queries")
    ix.set_param("group_force_exact", 1)
    ix.search_groups(Q[0], 4)
    assert ix.stat("group_searches") == 3 and ix.stat("group_queries") == 7
    assert ix.stat("searches") == 3 and ix.stat("queries") == 7  # once per call
    assert ix.stat("group_fallback_queries") == before + 1
    ix.close()

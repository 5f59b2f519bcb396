"""The fp32-MFMA form of the range search's scan (csrc/vdb_range_mfma.hip; knob ``range_mfma``).

The contract is the range search's own (tests/test_gpu_search_range.py): every case runs with
``range_mfma = 1``, checks that ``range_mfma_queries`` rose by the batch, and compares counts,
indices, keys and scores with ``_range_cases.expected`` by ``assert_array_equal`` through guarded
outputs.  No tolerance appears anywhere.

Shapes: dims with pad columns, a K tail and many K chunks of 32 (1, 33, 260, 768, 2100); row counts at
the 32-row tile and the 512-row chunk edges; batches with a partly empty 32-query N tile, two tiles
and a second block of 64.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _range_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 257
S_IDX, S_CNT = -7, -9
METRICS = rc.METRICS


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def _index(vdb, V, metric, knob=1):
    ix = vdb.NativeIndex(V.shape[1], metric)
    if V.shape[0]:
        ix.add(V)
    ix.set_param("range_mfma", knob)
    return ix


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _call(ix, Q, thr, cap, mask=None, index_offset=0):
    """The C-ABI call in host memory with guarded outputs -> (counts, idx, scores, keys)."""
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    B = Q.shape[0]
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thr, np.float64), (B,)))
    n = B * cap
    counts = np.full(B + GUARD, S_CNT, np.int64)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    sc = np.full(n + GUARD, np.nan, np.float32)
    ks = np.full(n + GUARD, np.nan, np.float64)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    before = ix.stat("range_mfma_queries")
    code = ix._lib.vdb_index_search_range(ix._h, _p(Q), B, _p(thr), _p(m), 0, cap, _p(counts), _p(idx), _p(sc), _p(ks),
                                          index_offset, None)
    assert code == 0
    assert ix.stat("range_mfma_queries") - before == (B if ix.mfma_expected else 0), "the other form served the call"
    assert (counts[B:] == S_CNT).all() and (idx[n:] == S_IDX).all(), "guard touched"
    assert np.isnan(sc[n:]).all() and np.isnan(ks[n:]).all(), "guard touched"
    return counts[:B], idx[:n].reshape(B, cap), sc[:n].reshape(B, cap), ks[:n].reshape(B, cap)


def _check(ix, V, Q, thr, cap, metric, keys=None, mask=None, index_offset=0, what=""):
    Q = np.asarray(Q, np.float32).reshape(-1, V.shape[1])
    keys = rc.oracle_keys(Q, V, metric) if keys is None else keys
    thr = np.broadcast_to(np.asarray(thr, np.float64), (Q.shape[0],))
    want = rc.expected(keys, rc.kt_of(metric, thr), cap, metric, mask, index_offset)
    ix.mfma_expected = getattr(ix, "mfma_expected", True)
    got = _call(ix, Q, thr, cap, None if mask is None else rc.words(mask), index_offset)
    for g, w, name in zip(got, want, ("counts", "indices", "scores", "keys")):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")
    return got


def _midpoints(keys, metric, lo, step):
    n = keys.shape[1]
    return np.array([rc.midpoint_threshold(keys[b], min(lo + step * b, n), metric) for b in range(keys.shape[0])])


def _dim_thresholds(keys, dim, metric, lo=5, step=40):
    if dim == 1 and metric == "cosine":  # keys are +-1: thresholds between and beyond them, not on them
        return np.resize(np.array([0.0, 0.5, -0.5, 1.5]), keys.shape[0])
    return _midpoints(keys, metric, lo, step)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 33, 260, 768, 2100])
def test_dims_and_fast_path(vdb, dim, metric):
    """Every dim at cap below, at and above the counts and count-only; and the fast path is the
    common path: at most 1 / 50 of the pairs scored took the fp64 path."""
    n, B = 1100, 3
    V, Q = rc.corpus(n, dim)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:B], V, metric)
    thr = _dim_thresholds(keys, dim, metric)
    before = ix.stat("range_mfma_exact_pairs")
    counts = _check(ix, V, Q[:B], thr, 0, metric, keys, what=f"dim {dim} count only")[0]
    exact = ix.stat("range_mfma_exact_pairs") - before
    print(f"dim {dim} {metric}: {exact} of {n * B} pairs took the fp64 path")
    assert exact * 50 <= n * B
    for cap in (int(counts[1]) - 1, int(counts[1]), 64, n + 3):
        _check(ix, V, Q[:B], thr, max(cap, 1), metric, keys, what=f"dim {dim} cap {cap}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [31, 32, 33, 511, 513, 1100])
def test_row_counts(vdb, n, metric):
    V, Q = rc.corpus(n, 100)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:3], V, metric)
    every = -np.inf if metric == "cosine" else np.inf
    thr = np.array([every, rc.midpoint_threshold(keys[1], (n + 1) // 2, metric), rc.midpoint_threshold(keys[2], n - 1, metric)])
    c = _check(ix, V, Q[:3], thr, n + 2, metric, keys, what=f"n {n}")[0]
    assert c.tolist() == [n, (n + 1) // 2, n - 1]
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [100, 2100])
def test_batches_and_same_bytes_as_the_other_form(vdb, dim, metric):
    """Batches 1, 31, 33, 64, 65 (a dim below and above 2 048); knob 2 on the same index gives the
    same bytes and leaves range_mfma_queries still."""
    n = 700
    V, Q = rc.corpus(n, dim, n_queries=65)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q, V, metric)
    thr = _midpoints(keys, metric, 0, 5)
    got = {}
    for B in (1, 31, 33, 64, 65):
        got[B] = _check(ix, V, Q[:B], thr[:B], 40, metric, keys[:B], what=f"dim {dim} B {B}")
        assert got[B][0].tolist() == [min(5 * b, n) for b in range(B)]
    ix.set_param("range_mfma", 2)
    ix.mfma_expected = False
    other = _check(ix, V, Q, thr, 40, metric, keys, what="knob 2")
    assert b"".join(a.tobytes() for a in other) == b"".join(a.tobytes() for a in got[65])
    ix.close()


@pytest.mark.parametrize("case", ["cosine_equality", "euclid_equality", "duplicates_cosine", "duplicates_euclidean"])
def test_soundness_at_the_bound(vdb, case):
    """Bounds that are a row's own key, and the next fp64 beyond: the undecided path must run."""
    n, dim = 700, 100
    if case == "cosine_equality":
        metric = "cosine"
        V, Q = rc.corpus(n, dim)
        keys = rc.oracle_keys(Q[:1], V, metric)
        Qs, thr = np.repeat(Q[:1], 2, axis=0), list(rc.cosine_equality(keys[0], 123))
    elif case == "euclid_equality":
        metric = "euclidean"
        V, q, planted = rc.euclid_equality_case(n, dim)
        Qs, thr = np.stack([q, q]), [rc.EUCLID_RADIUS, np.nextafter(rc.EUCLID_RADIUS, 0.0)]
    else:
        metric = case.split("_")[1]
        V, Q, groups = rc.duplicates_case(n, dim)
        keys = rc.oracle_keys(Q[:1], V, metric)
        ks = [keys[0, g[0]] for g in groups]
        Qs = np.repeat(Q[:1], len(ks), axis=0)
        thr = [float(k) if metric == "cosine" else float(np.sqrt(-k)) * (1 + 1e-9) for k in ks]
    ix = _index(vdb, V, metric)
    before = ix.stat("range_mfma_exact_pairs")
    c = _check(ix, V, Qs, thr, n, metric, what=case)[0]
    assert ix.stat("range_mfma_exact_pairs") > before, "no pair took the fp64 path"
    if case.endswith("equality"):
        assert c[0] - c[1] >= 1
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", ["underflow", "overflow", "coincide", "clamp"])
def test_magnitudes(vdb, case, metric):
    n, dim = 600, 100
    V, Q = rc.corpus(n, dim)
    V, Q = V.copy(), Q[:4].copy()
    if case == "underflow":  # fp32 products underflow: only the absolute term saves the decision
        V, Q = V * np.float32(2.0 ** -70), Q * np.float32(2.0 ** -70)
    elif case == "overflow":  # fp32 sums overflow: NaN and infinity take the fp64 path
        V, Q = V * np.float32(2.0 ** 63), Q * np.float32(2.0 ** 63)
    elif case == "coincide":  # rows equal to a query: the euclidean subtraction cancels
        V[[3, 77, 300, 599]] = Q[0]
        V[[40, 41]] = Q[1]
    else:  # rows and a query with a norm below 1e-8: the cosine clamp
        V[::7] *= np.float32(1e-12)
        Q[2] *= np.float32(1e-12)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q, V, metric)
    thr = _midpoints(keys, metric, 4, 50)
    _check(ix, V, Q, thr, 64, metric, keys, what=case)
    if case == "coincide" and metric == "euclidean":
        c = _check(ix, V, Q[:2], [0.0, 1e-30], n, metric, keys[:2], what="radius 0 and tiny")[0]
        assert c.tolist() == [4, 2]
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_mask_offset_device_memory_and_empty(vdb, metric):
    import torch
    n, B, cap = 1300, 5, 128
    V, Q = rc.corpus(n, 100)
    ix = _index(vdb, V, metric)
    keys = rc.oracle_keys(Q[:B], V, metric)
    thr = _midpoints(keys, metric, 150, 200)
    mask = np.random.default_rng(5).random(n) < 0.4
    mask[64:96] = False    # a whole empty tile
    mask[128:1024] = False  # empty passes and a whole empty workgroup
    mask[1024:] = False
    mask[1290:] = True     # ... but for a ragged last word
    _check(ix, V, Q[:B], thr, 500, metric, keys, mask=mask, what="mask")
    _check(ix, V, Q[:B], thr, 100, metric, keys, mask=mask, index_offset=10 ** 12, what="mask + offset")
    # device memory: a NaN threshold and a negative radius count 0
    bad = thr.copy()
    bad[1] = np.nan
    bad[3] = np.nan if metric == "cosine" else -1.0
    dev = torch.device("cuda")
    dq, dt = torch.from_numpy(Q[:B].copy()).to(dev), torch.from_numpy(bad).to(dev)
    dc = torch.full((B + GUARD,), S_CNT, dtype=torch.int64, device=dev)
    di = torch.full((B * cap + GUARD,), S_IDX, dtype=torch.int64, device=dev)
    ds = torch.full((B * cap + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    dk = torch.full((B * cap + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    before = ix.stat("range_mfma_queries")
    ix.search_range_device(dq.data_ptr(), B, dt.data_ptr(), cap, dc.data_ptr(), di.data_ptr(), ds.data_ptr(), dk.data_ptr())
    torch.cuda.synchronize()
    assert ix.stat("range_mfma_queries") - before == B
    invalid = np.isnan(bad) | ((bad < 0) if metric == "euclidean" else False)
    want = rc.expected(keys, rc.kt_of(metric, np.where(invalid, np.nan, bad)), cap, metric)
    assert want[0][1] == 0 and want[0][3] == 0 and want[0][0] > 0
    c, i, s, k = (x.cpu().numpy() for x in (dc, di, ds, dk))
    for g, w in zip((c, i, s, k), want):
        np.testing.assert_array_equal(g[:w.size].reshape(w.shape), w)
    assert (c[B:] == S_CNT).all() and (i[B * cap:] == S_IDX).all()
    assert np.isnan(s[B * cap:]).all() and np.isnan(k[B * cap:]).all()
    ix.close()
    # an empty index
    ix = _index(vdb, V[:0].reshape(0, 100), metric)
    ix.mfma_expected = True
    c, i, s, k = _call(ix, Q[:2], [0.5, 0.5], 3)
    assert (c == 0).all() and (i == -1).all() and (s == 0).all() and np.isneginf(k).all()
    ix.close()

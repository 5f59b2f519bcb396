"""Case builders and the oracle of tests/test_gpu_search_hybrid_sum.py and
tests/test_gpu_store_hybrid_sum.py (weighted-sum hybrid search, include/vdb.h
vdb_index_search_hybrid_sum), kept apart from the GPU tests so that
tests/test_hybsum_precondition.py can check on the CPU that every case has the property its name
claims.

``expected`` restates the contract literally.  ``kd`` is ``oracle.ref_cpu.exact_keys`` (the canonical
dense key), ``ks`` is ``_sparse_cases.keys_of`` (the sparse contract's loop); a row's value is four
separate numpy float64 operations, ``t1 = w_dense * kd``, ``t2 = w_sparse * ks``, ``u = t1 + t2``,
``c = u + 0.0``; every row whose mask bit is set is a candidate, and they rank by ``lexsort((row,
-c))``.
"""
import functools

import numpy as np

import _fused_cases as fc
import _sparse_cases as sp
from oracle import ref_cpu

METRICS = fc.METRICS
MAX_K = 1024           # csrc/vdb_hybsum_plan.h kHybsumMaxK
MAX_QUERIES = 65535    # csrc/vdb_hybsum_plan.h kHybsumMaxQueries
MAX_WEIGHT = 2.0 ** 64  # csrc/vdb_hybsum_plan.h kHybsumMaxWeight
WEIGHTS = ((1.0, 1.0), (0.3, 0.7), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0), (MAX_WEIGHT, MAX_WEIGHT))
ROWS = sp.ROWS          # under a wave trip, under a chunk, two chunks plus one row, more than four chunks
DIMS = (16, 260, 1100, 2100)  # the 4-piece, 8-piece and any-length key paths; 260: no multiple of 256


def combine(w_dense, kd, w_sparse, ks):
    """csrc/vdb_hybsum_plan.h hybsum_combine in numpy float64: four separate operations."""
    t1 = np.float64(w_dense) * np.asarray(kd, np.float64)
    t2 = np.float64(w_sparse) * np.asarray(ks, np.float64)
    u = t1 + t2
    return u + np.float64(0.0)


def parts_of(V, q, col, qt, qw, metric, xn=None):
    """(kd f64 [n], ks f64 [n]) of every row against one query."""
    V = np.asarray(V, np.float32)
    if V.shape[0] == 0:
        return np.zeros(0), np.zeros(0)
    kd = ref_cpu.exact_keys(np.asarray(q, np.float32), V, metric, fc._norms(V, metric) if xn is None else xn)
    ks, _ = sp.keys_of(col, np.asarray(qt, np.int32), np.asarray(qw, np.float32))
    return kd, ks


def one_list(V, q, col, qt, qw, k, metric, weights, mask=None, xn=None):
    """(rows, c, kd, ks): the first k candidates by (c desc, row asc)."""
    kd, ks = parts_of(V, q, col, qt, qw, metric, xn)
    c = combine(weights[0], kd, weights[1], ks)
    n = np.asarray(V).shape[0]
    rows = np.arange(n) if mask is None else np.nonzero(np.asarray(mask, bool)[:n])[0]
    o = rows[np.lexsort((rows, -c[rows]))][:k]
    return o.astype(np.int64), c[o], kd[o], ks[o]


def expected(V, Q, col, qs, k, metric, weights, mask=None, index_offset=0, bad=()):
    """(scores f32, indices i64, fused f64, dense f64, sparse f64), each [B, k], of the contract.
    ``bad``: the queries answered with "no result" whatever they hold (bad device input)."""
    V = np.asarray(V, np.float32)
    Q = np.asarray(Q, np.float32).reshape(-1, V.shape[1])
    B = len(qs)
    sc = np.zeros((B, k), np.float32)
    idx = np.full((B, k), -1, np.int64)
    fu = np.full((B, k), -np.inf)
    de = np.full((B, k), -np.inf)
    spk = np.full((B, k), -np.inf)
    xn = fc._norms(V, metric)
    for b, (qt, qw) in enumerate(qs):
        if b in bad:
            continue
        rows, c, kd, ks = one_list(V, Q[b], col, qt, qw, k, metric, weights, mask, xn)
        n = rows.size
        idx[b, :n] = rows + index_offset
        fu[b, :n] = c
        de[b, :n] = kd
        spk[b, :n] = ks
        sc[b, :n] = c.astype(np.float32)
    return sc, idx, fu, de, spk


@functools.lru_cache(maxsize=None)
def dense_rows(n, d, seed=0, n_queries=8):
    return fc.corpus(n, d, seed=seed, n_queries=n_queries)


# ---- named cases (their claims: tests/test_hybsum_precondition.py) -----------------------------------
BETWEEN_N = 1300
BETWEEN_SIDE = 250  # rows near the query, and rows with high sparse keys: more than any fetch_k (200)


@functools.lru_cache(maxsize=None)
def between_case():
    """(V, Q [1, 16], col, qs, planted): cosine, weights (1, 1).  250 rows lie near the query and share
    no term with it; 250 rows are nearly orthogonal to it and have high sparse keys; the planted row
    has moderate values of both, so that it is far down both rankings and still has the best sum."""
    rng = np.random.default_rng(20260)
    n, d = BETWEEN_N, sp.DIM
    q = rng.standard_normal(d).astype(np.float32)
    qu = q / np.linalg.norm(q)
    V = rng.standard_normal((n, d)).astype(np.float32)
    where = rng.permutation(n)
    near, high, planted = where[:BETWEEN_SIDE], where[BETWEEN_SIDE:2 * BETWEEN_SIDE], int(where[2 * BETWEEN_SIDE])
    rest = where[2 * BETWEEN_SIDE + 1:]
    V[near] = (q + 0.25 * rng.standard_normal((BETWEEN_SIDE, d))).astype(np.float32)
    orth = rng.standard_normal((BETWEEN_SIDE, d))
    orth -= np.outer(orth @ qu, qu)
    V[high] = (orth + 0.02 * np.outer(rng.standard_normal(BETWEEN_SIDE), qu)).astype(np.float32)
    o = rng.standard_normal(d)
    o -= (o @ qu) * qu
    o /= np.linalg.norm(o)
    V[planted] = (0.6 * qu + 0.8 * o).astype(np.float32)  # cosine about 0.6
    qt = np.arange(10, 18, dtype=np.int32)
    qw = np.ones(8, np.float32)
    rows = [None] * n
    for r in near.tolist():  # no shared term
        rows[r] = ((600 + r % 50,), (1.0,))
    for r in high.tolist():  # keys in [0.9, 1.0]
        a = 0.45 + 0.05 * rng.random()
        rows[r] = ((10, 12, 2000 + r), (a, a, 1.0))
    rows[planted] = ((11, 13), (0.3, 0.3))  # key about 0.6
    for j, r in enumerate(rest.tolist()):  # keys of at most 0.2, or no shared term
        rows[r] = ((14, 700 + r % 90), (0.2 * rng.random(), 1.0)) if j % 2 else ((800 + r % 70,), (1.0,))
    col = sp.Column([(np.asarray(t, np.int32), np.asarray(w, np.float32)) for t, w in rows], 30522)
    V.setflags(write=False)
    Q = q.reshape(1, d)
    Q.setflags(write=False)
    return V, Q, col, [(qt, qw)], planted


@functools.lru_cache(maxsize=None)
def tie_case(n=1300):
    """(V, Q [2, 16], col, qs): every dense row is the same vector, so kd is one value per query, with
    ``_sparse_cases.tie_case``'s integer column: ties in ks are ties in c, and the row-id rule decides
    among the first k."""
    col, qs = sp.tie_case(n)
    rng = np.random.default_rng(20261)
    v = rng.standard_normal(sp.DIM).astype(np.float32)
    V = np.repeat(v[None, :], n, axis=0)
    Q = rng.standard_normal((len(qs), sp.DIM)).astype(np.float32)
    V.setflags(write=False)
    Q.setflags(write=False)
    return V, Q, col, qs


@functools.lru_cache(maxsize=None)
def signed_case(n=513):
    """(V, Q [2, 16], col, qs, copy): euclidean, ``_sparse_cases.signed_case``'s column (sparse weights
    of both signs and zeros).  Row ``copy`` is an exact copy of query 0 (kd = -0.0) and shares no term
    with it (ks = +0.0), so its c is +0.0; most rows have c < 0."""
    col, qs = sp.signed_case(n)
    rng = np.random.default_rng(20262)
    V = (0.3 * rng.standard_normal((n, sp.DIM))).astype(np.float32)
    Q = (0.3 * rng.standard_normal((len(qs), sp.DIM))).astype(np.float32)
    ks, matched = sp.keys_of(col, *qs[0])
    copy = int(np.nonzero(~matched & (ks == 0))[0][7])
    V[copy] = Q[0]
    V.setflags(write=False)
    Q.setflags(write=False)
    return V, Q, col, qs, copy


@functools.lru_cache(maxsize=None)
def short_case(n=300, k=10):
    """(V, Q [5, 16], col, qs, mask, k): k above the eligible rows: a mask of four bits."""
    V, Q = dense_rows(n, sp.DIM, seed=5)
    col = sp.column(n, 30522)
    mask = np.zeros(n, bool)
    mask[[3, 64, 255, 299]] = True
    mask.setflags(write=False)
    return V, Q[:5], col, sp.queries(30522), mask, k

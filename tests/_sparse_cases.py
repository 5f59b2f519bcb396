"""Case builders and the oracle of tests/test_gpu_search_sparse.py and tests/test_gpu_store_hybrid.py
(sparse and hybrid search, include/vdb.h vdb_index_set_sparse / vdb_index_search_sparse /
vdb_index_search_hybrid), kept apart from the GPU tests so that tests/test_sparse_precondition.py
can check on the CPU that every case has the property its name claims.

``expected`` restates the sparse contract with plain loops: ``qd[t]`` is the query's weight as a
float64 (0.0 for a term it does not list); a row's key is ``acc = acc + float64(w_e) * qd[t_e]`` over
its entries in stored order, in numpy float64 scalars (two separate operations); the row matches when
some entry has ``w_e != 0`` and ``qd[t_e] != 0``; the matching rows with their mask bit rank by
``lexsort((row, -key))``.  ``expected_hybrid`` feeds that list and the dense list of
tests/_fused_cases.py (``one_list``) to its literal RRF (``fuse`` / ``rank``).
"""
import functools

import numpy as np

import _fused_cases as fc

METRICS = fc.METRICS
MAX_K = 1024            # csrc/vdb_sparse_plan.h kSparseMaxK
MAX_QUERY_TERMS = 1024  # csrc/vdb_sparse_plan.h kSparseMaxQueryTerms
VOCABS = (5, 30522, 2 ** 31 - 1)
ROW_LENGTHS = (0, 1, 63, 64, 65, 300)
ROWS = (3, 37, 513, 1300)
DIM = 16


class Column:
    """One sparse vector per row in CSR form (what vdb_index_set_sparse takes)."""

    def __init__(self, rows, n_terms):
        self.n_terms = int(n_terms)
        self.rows = [(np.asarray(t, np.int32), np.asarray(w, np.float32)) for t, w in rows]
        self.indptr = np.zeros(len(rows) + 1, np.int64)
        if rows:
            np.cumsum([t.size for t, _ in self.rows], out=self.indptr[1:])
        self.terms = np.concatenate([t for t, _ in self.rows]) if rows else np.zeros(0, np.int32)
        self.weights = np.concatenate([w for _, w in self.rows]) if rows else np.zeros(0, np.float32)
        self.terms = self.terms.astype(np.int32)
        self.weights = self.weights.astype(np.float32)

    @property
    def n(self):
        return len(self.rows)

    @property
    def nnz(self):
        return int(self.indptr[-1])


def pack(vectors):
    """[(terms, weights), ...] -> (indptr i64, terms i32, weights f32)."""
    c = Column(vectors, 1)
    return c.indptr, c.terms, c.weights


def _draw_terms(rng, n, lo_pool, n_terms, exclude=()):
    """n distinct ascending term ids: from lo_pool first (random subset), the rest uniform over the
    vocabulary outside ``exclude``."""
    n = min(n, n_terms - (len(exclude) if len(lo_pool) == 0 else 0))
    chosen = set()
    if len(lo_pool):
        take = min(n, len(lo_pool), 1 + int(rng.integers(0, 12)))
        chosen.update(rng.choice(lo_pool, size=take, replace=False).tolist())
    ex = set(exclude)
    while len(chosen) < n:
        for t in rng.integers(0, n_terms, size=2 * (n - len(chosen)) + 4).tolist():
            if t not in chosen and t not in ex and len(chosen) < n:
                chosen.add(t)
    return np.asarray(sorted(chosen), np.int32)


def _weights(rng, n, kind):
    if kind == "int":      # small positive integers: many rows tie exactly
        return rng.integers(1, 3, size=n).astype(np.float32)
    if kind == "signed":   # integers of both signs and zeros: keys of 0 and below, entries that do not match
        return rng.integers(-2, 3, size=n).astype(np.float32)
    return rng.standard_normal(n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def hot_terms(n_terms, seed=0):
    """The terms the queries draw from and most rows hold some of: 0, n_terms - 1 and up to 30 more."""
    if n_terms <= 32:
        return tuple(range(n_terms))
    rng = np.random.default_rng(977 * seed + n_terms % 1000003)
    return tuple(sorted({0, n_terms - 1, *rng.integers(1, n_terms - 1, size=30).tolist()}))


@functools.lru_cache(maxsize=None)
def column(n, n_terms, kind="float", seed=0):
    """n rows whose lengths cycle through ROW_LENGTHS (capped by the vocabulary); every fifth row is
    cold (it holds no hot term, where the vocabulary has room for that), the others hold some."""
    rng = np.random.default_rng(1000003 * seed + 31 * n + n_terms % 65521 + {"float": 0, "int": 1, "signed": 2}[kind])
    hot = np.asarray(hot_terms(n_terms, seed), np.int64)
    rows = []
    for r in range(n):
        L = min(ROW_LENGTHS[(r + seed) % len(ROW_LENGTHS)], n_terms)
        cold = r % 5 == 4 and n_terms > 4 * len(hot)
        t = _draw_terms(rng, L, np.zeros(0, np.int64) if cold else hot, n_terms, exclude=hot.tolist() if cold else ())
        rows.append((t, _weights(rng, t.size, kind)))
    return Column(rows, n_terms)


def query(n_terms, length, kind="float", seed=0):
    """A query of ``length`` terms (capped by the vocabulary): hot terms first, then random fill."""
    rng = np.random.default_rng(7919 * seed + length + n_terms % 65521)
    hot = np.asarray(hot_terms(n_terms, seed // 100), np.int64)
    length = min(length, n_terms, MAX_QUERY_TERMS)
    if length == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float32)
    chosen = set(rng.choice(hot, size=min(length, len(hot)), replace=False).tolist())
    while len(chosen) < length:
        for t in rng.integers(0, n_terms, size=2 * (length - len(chosen)) + 4).tolist():
            if len(chosen) < length:
                chosen.add(t)
    t = np.asarray(sorted(chosen), np.int32)
    w = _weights(rng, t.size, kind)
    if kind == "float":
        w[w == 0] = 1.0
    return t, w


def queries(n_terms, kind="float", seed=0):
    """The query lengths of the issue, 0, 1 and 1 024, and two of eight terms."""
    return [query(n_terms, L, kind, 100 * seed + j) for j, L in enumerate((8, 0, 1, 1024, 8))]


# ---- the oracle ------------------------------------------------------------------------------------
def row_key(rt, rw, qt, qw):
    """(key, matched) of one row (terms rt, weights rw) against one query: the contract's loop."""
    acc = np.float64(0.0)
    matched = False
    pos = np.searchsorted(qt, rt)
    for e in range(rt.size):
        j = int(pos[e])
        if j >= qt.size or qt[j] != rt[e]:
            continue  # qd = 0.0: adds +-0.0 to a sum that is never -0.0, the same bits
        qd = np.float64(qw[j])
        p = np.float64(rw[e]) * qd
        acc = acc + p
        matched = matched or (rw[e] != 0 and qd != 0)
    return acc, matched


def row_key_all_entries(rt, rw, qt, qw):
    """The contract's first form: every entry adds, with qd = 0.0 for an unlisted term."""
    acc = np.float64(0.0)
    table = {int(t): np.float64(w) for t, w in zip(qt.tolist(), qw.tolist())}
    for e in range(rt.size):
        acc = acc + np.float64(rw[e]) * table.get(int(rt[e]), np.float64(0.0))
    return acc


def keys_of(col, qt, qw):
    """(keys f64 [n], matched bool [n]) of every row against one query."""
    keys = np.zeros(col.n, np.float64)
    matched = np.zeros(col.n, bool)
    if qt.size == 0:
        return keys, matched
    hit = np.isin(col.terms, qt)
    rows_with = np.unique(np.searchsorted(col.indptr, np.nonzero(hit)[0], side="right") - 1)
    for r in rows_with.tolist():
        rt, rw = col.rows[r]
        keys[r], matched[r] = row_key(rt, rw, qt, qw)
    return keys, matched


def one_list(col, qt, qw, k, mask=None):
    """(rows, keys): the first k candidates by (key desc, row asc)."""
    keys, matched = keys_of(col, np.asarray(qt, np.int32), np.asarray(qw, np.float32))
    if mask is not None:
        matched = matched & np.asarray(mask, bool)[:col.n]
    rows = np.nonzero(matched)[0]
    o = rows[np.lexsort((rows, -keys[rows]))][:k]
    return o.astype(np.int64), keys[o]


def expected(col, qs, k, mask=None, index_offset=0):
    """(scores f32 [B, k], indices i64 [B, k], keys f64 [B, k]) of the contract."""
    B = len(qs)
    sc = np.zeros((B, k), np.float32)
    idx = np.full((B, k), -1, np.int64)
    ke = np.full((B, k), -np.inf)
    for b, (qt, qw) in enumerate(qs):
        rows, keys = one_list(col, qt, qw, k, mask)
        n = rows.size
        idx[b, :n] = rows + index_offset
        ke[b, :n] = keys
        sc[b, :n] = keys.astype(np.float32)
    return sc, idx, ke


def expected_hybrid(V, Q, col, qs, k, fetch_k, metric, weights=(1.0, 1.0), rrf_c=fc.RRF_C, mask=None, index_offset=0,
                    sparse_empty=()):
    """(scores, indices, fused, hits) [B, k]: query b's dense list and sparse list fused by RRF.
    ``sparse_empty``: the queries whose sparse list is empty whatever they hold (bad device input)."""
    V = np.asarray(V, np.float32)
    Q = np.asarray(Q, np.float32).reshape(-1, V.shape[1])
    B = len(qs)
    sc = np.zeros((B, k), np.float32)
    idx = np.full((B, k), -1, np.int64)
    fu = np.full((B, k), -np.inf)
    hi = np.zeros((B, k), np.int32)
    xn = fc._norms(V, metric)
    for b in range(B):
        dense = fc.one_list(Q[b], V, fetch_k, metric, mask, xn)
        sparse = (np.zeros(0, np.int64), np.zeros(0)) if b in sparse_empty else one_list(col, qs[b][0], qs[b][1], fetch_k, mask)
        rows, fused, hits = fc.rank(fc.fuse([dense, sparse], "rrf", np.asarray(weights, np.float64), rrf_c))
        n = min(k, rows.size)
        idx[b, :n] = rows[:n] + index_offset
        fu[b, :n] = fused[:n]
        hi[b, :n] = hits[:n]
        sc[b, :n] = fused[:n].astype(np.float32)
    return sc, idx, fu, hi


# ---- named cases (their claims: tests/test_sparse_precondition.py) -----------------------------------
def tie_case(n=1300):
    """Integer weights: many rows share a key exactly, so the row-id rule decides among the first k."""
    col = column(n, 30522, "int", seed=1)
    return col, [query(30522, 8, "int", 100), query(30522, 1, "int", 102)]


def signed_case(n=513):
    """Weights of both signs and zeros: matching rows with a key of 0 and below are ranked, and an
    entry with weight 0 on a listed term does not make its row match."""
    col = column(n, 30522, "signed", seed=2)
    return col, [query(30522, 8, "signed", 200), query(30522, 8, "signed", 204)]


def beyond_case(n=513):
    """k above the number of matching rows: a query of three rare terms, which few rows hold."""
    col = column(n, 30522, "float", seed=3)
    hot = set(hot_terms(30522, 3))
    rare = sorted({int(t) for r in (4, 9, 14) for t in col.rows[r][0][-1:].tolist()} - hot)
    return col, [(np.asarray(rare, np.int32), np.full(len(rare), 1.5, np.float32))]


def zero_key_case():
    """Rows whose products cancel: row 1 matches with key exactly 0, row 2 with a key below 0; row 3
    shares a term whose stored weight is 0 and row 4 shares no term: neither is returned."""
    rows = [((1, 5), (2.0, 1.0)), ((1, 5), (1.0, -1.0)), ((1, 5), (-1.0, -1.0)), ((1, 9), (0.0, 3.0)), ((2, 9), (1.0, 1.0)),
            ((), ())]
    col = Column([(np.asarray(t, np.int32), np.asarray(w, np.float32)) for t, w in rows], 10)
    return col, [(np.asarray([1, 5], np.int32), np.asarray([1.0, 1.0], np.float32))]


def edge_terms_case(n_terms):
    """Terms 0 and n_terms - 1 stored and queried."""
    last = n_terms - 1
    rows = [((0,), (1.0,)), ((0, last), (1.0, 2.0)) if last > 0 else ((0,), (3.0,)), ((last,), (0.5,)), ((), ())]
    col = Column([(np.asarray(t, np.int32), np.asarray(w, np.float32)) for t, w in rows], n_terms)
    qs = [(np.asarray(sorted({0, last}), np.int32), np.ones(len({0, last}), np.float32)),
          (np.asarray([last], np.int32), np.asarray([2.0], np.float32))]
    return col, qs


def dense_rows(n, seed=0, n_queries=8):
    return fc.corpus(n, DIM, seed=seed, n_queries=n_queries)

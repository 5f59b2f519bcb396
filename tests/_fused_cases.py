"""Case builders and the oracle of tests/test_gpu_search_fused.py and tests/test_gpu_store_fused.py
(fused search, include/vdb.h vdb_index_search_fused), kept apart from the GPU tests so that
tests/test_fused_precondition.py can check on the CPU that every case has the property its name
claims.

Every expectation comes from the reference arithmetic alone (``oracle.ref_cpu.exact_keys`` and
``canonical_norm64``).  ``expected`` restates the contract literally: list l of a set is the best
``fetch_k`` eligible rows of its l-th sub-query by ``lexsort((rows, -keys))``; a row's fused value is
built in numpy float64 scalars in the contract's operation order (RRF: ``t = c + float64(p + 1)``,
``u = w / t``, ``acc = acc + u`` for l ascending; MAX: the first holding list's key, then ``k if k >
fused else fused``); the candidates rank by ``lexsort((row, -fused))``.
"""
import functools

import numpy as np

from oracle import ref_cpu

METRICS = ("cosine", "euclidean")
FUSIONS = ("rrf", "max")
MAX_K = 200      # csrc/vdb_fuse_plan.h kFuseMaxK
MAX_FETCH = 200  # csrc/vdb_fuse_plan.h kFuseMaxFetch
MAX_LISTS = 16   # csrc/vdb_fuse_plan.h kFuseMaxLists
RRF_C = 60.0


@functools.lru_cache(maxsize=None)
def corpus(n, d, seed=0, n_queries=8):
    rng = np.random.default_rng(300007 * seed + 43 * n + d)
    V = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((n_queries, d)).astype(np.float32)
    V.setflags(write=False)
    Q.setflags(write=False)
    return V, Q


def bitmap_words(mask_bool, extra_bits=0):
    """bool [N] -> the uint32 row_mask words; ``extra_bits``: that many bits set at and past N (they
    name no row)."""
    m = np.concatenate([np.asarray(mask_bool, bool), np.ones(extra_bits, bool)])
    raw = np.packbits(m, bitorder="little").tobytes().ljust((len(m) + 31) // 32 * 4, b"\0")
    return np.frombuffer(raw, dtype=np.uint32).copy()


def offsets_of(sizes):
    o = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64), out=o[1:])
    return o


def _norms(V, metric):
    return ref_cpu.canonical_norm64(V) if metric == "cosine" and V.shape[0] else None


def one_list(q, V, fetch_k, metric, mask=None, xn=None):
    """(c, kappa): one sub-query's list, row ids by (key desc, row asc), and their keys."""
    if V.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0)
    keys = ref_cpu.exact_keys(q, V, metric, xn)
    rows = np.arange(V.shape[0]) if mask is None else np.nonzero(np.asarray(mask, bool))[0]
    c = rows[np.lexsort((rows, -keys[rows]))][:fetch_k]
    return c.astype(np.int64), keys[c]


def key_scores(keys, metric):
    """The fp32 score a search writes for a key: the similarity, or the root of the squared distance."""
    keys = np.asarray(keys, np.float64)
    return keys.astype(np.float32) if metric == "cosine" else np.sqrt(-keys).astype(np.float32)


def fuse(lists, fusion, weights=None, rrf_c=RRF_C, order=None, dtype=np.float64):
    """{row: (fused, hits)} of the contract for one set's lists [(c, kappa), ...].  ``order``: the
    lists' summation order (default ascending l) and ``dtype`` the arithmetic: the contract is the
    default of both; the precondition test varies them."""
    acc, hits = {}, {}
    c_ = dtype(rrf_c)
    for l in (range(len(lists)) if order is None else order):
        c, kappa = lists[l]
        w = dtype(1.0 if weights is None else weights[l])
        for p, r in enumerate(c.tolist()):
            if fusion == "rrf":
                t = c_ + dtype(p + 1)
                u = w / t
                acc[r] = acc.get(r, dtype(0.0)) + u
            else:
                kv = dtype(kappa[p])
                acc[r] = kv if r not in acc else (kv if kv > acc[r] else acc[r])
            hits[r] = hits.get(r, 0) + 1
    return {r: (acc[r], hits[r]) for r in acc}


def rank(cands):
    """(rows, fused, hits) of {row: (fused, hits)} by (fused desc, row asc)."""
    rows = np.asarray(sorted(cands), np.int64)
    fused = np.asarray([cands[r][0] for r in rows.tolist()], np.float64)
    hits = np.asarray([cands[r][1] for r in rows.tolist()], np.int32)
    o = np.lexsort((rows, -fused))
    return rows[o], fused[o], hits[o]


def set_lists(Qs, V, fetch_k, metric, mask=None, xn=None):
    xn = _norms(V, metric) if xn is None else xn
    return [one_list(q, V, fetch_k, metric, mask, xn) for q in np.asarray(Qs, np.float32).reshape(-1, V.shape[1])]


def expected(Q, offsets, V, k, fetch_k, fusion, metric, weights=None, rrf_c=RRF_C, mask=None, index_offset=0):
    """(scores f32 [S, k], indices i64 [S, k], fused f64 [S, k], hits i32 [S, k]) of the contract for
    the sub-queries Q [n_sub, dim] in sets ``offsets``, rows V and an optional bool mask [N]."""
    V = np.asarray(V, np.float32)
    Q = np.asarray(Q, np.float32).reshape(-1, V.shape[1])
    S = len(offsets) - 1
    sc = np.zeros((S, k), np.float32)
    idx = np.full((S, k), -1, np.int64)
    fu = np.full((S, k), -np.inf)
    hi = np.zeros((S, k), np.int32)
    xn = _norms(V, metric)
    cache = {}
    for s in range(S):
        o0, o1 = int(offsets[s]), int(offsets[s + 1])
        lists = []
        for j in range(o0, o1):
            key = Q[j].tobytes()
            if key not in cache:
                cache[key] = one_list(Q[j], V, fetch_k, metric, mask, xn)
            lists.append(cache[key])
        w = None if weights is None else np.asarray(weights, np.float64)[o0:o1]
        rows, fused, hits = rank(fuse(lists, fusion, w, rrf_c))
        n = min(k, rows.size)
        idx[s, :n] = rows[:n] + index_offset
        fu[s, :n] = fused[:n]
        hi[s, :n] = hits[:n]
        sc[s, :n] = fused[:n].astype(np.float32) if fusion == "rrf" else key_scores(fused[:n], metric)
    return sc, idx, fu, hi


def brute_force_max(Qs, V, k, metric, mask=None):
    """(rows, values): the top k of max_l exact_keys(q_l, V) over all eligible rows of the corpus, by
    (value desc, row asc): what MAX fusion must equal for any fetch_k >= k."""
    xn = _norms(V, metric)
    K = np.stack([ref_cpu.exact_keys(q, V, metric, xn) for q in np.asarray(Qs, np.float32).reshape(-1, V.shape[1])])
    best = K[0].copy()
    for row in K[1:]:
        best = np.where(row > best, row, best)
    rows = np.arange(V.shape[0]) if mask is None else np.nonzero(np.asarray(mask, bool))[0]
    o = rows[np.lexsort((rows, -best[rows]))][:k]
    return o.astype(np.int64), best[o]


# ---- identical: every list of the set is the same ---------------------------------------------------------
def identical_case(m, n=700, d=32):
    """(V, Qset): m copies of one vector."""
    V, Q = corpus(n, d, seed=1)
    return V, np.repeat(Q[:1], m, axis=0)


# ---- disjoint: one planted cluster per sub-query ------------------------------------------------------------
CLUSTER_ROWS = 210  # > MAX_FETCH: a list of 200 stays inside its cluster


@functools.lru_cache(maxsize=None)
def disjoint_case(m, d=32, seed=0):
    """(V, Qset): m clusters of CLUSTER_ROWS rows around far-apart centres at shuffled row ids (then
    random rows up to a multiple of 256 + 37); sub-query l is centre l, so with fetch_k = 200 the lists
    are pairwise disjoint and, under RRF with equal weights, every rank holds m rows that tie."""
    rng = np.random.default_rng(7001 + 13 * m + seed)
    centres = (rng.standard_normal((m, d)) * 4.0).astype(np.float32)
    n_cl = m * CLUSTER_ROWS
    n = (n_cl + 255) // 256 * 256 + 37
    V = (rng.standard_normal((n, d)) * 0.5).astype(np.float32)
    where = rng.permutation(n)[:n_cl].reshape(m, CLUSTER_ROWS)
    for l in range(m):
        V[where[l]] = centres[l] + 0.05 * rng.standard_normal((CLUSTER_ROWS, d)).astype(np.float32)
    V.setflags(write=False)
    centres.setflags(write=False)
    return V, centres


# ---- overlap: random, correlated sub-queries ----------------------------------------------------------------
OVERLAP_N = 2000
OVERLAP_D = 32
OVERLAP_FETCH = 200
# seeds at which the case has a pair of candidates that a float32 or re-ordered sum would rank the
# other way (tests/test_fused_precondition.py holds them to it)
OVERLAP_SEEDS = {(3, "cosine"): 30, (3, "euclidean"): 180, (5, "cosine"): 124, (5, "euclidean"): 422}


@functools.lru_cache(maxsize=None)
def overlap_case(m, metric, seed=None):
    """(V, Qset): m random sub-queries around one random direction, so that their lists overlap at
    different ranks: a row's hits run from 1 to m and its RRF sum has up to m terms."""
    seed = OVERLAP_SEEDS[(m, metric)] if seed is None else seed
    rng = np.random.default_rng(910007 * seed + 17 * m + (0 if metric == "cosine" else 5))
    V = rng.standard_normal((OVERLAP_N, OVERLAP_D)).astype(np.float32)
    base = rng.standard_normal(OVERLAP_D).astype(np.float32)
    Qs = (base + 0.35 * rng.standard_normal((m, OVERLAP_D))).astype(np.float32)
    V.setflags(write=False)
    Qs.setflags(write=False)
    return V, Qs


def order_differs(lists, weights=None, rrf_c=RRF_C):
    """Does the RRF ranking of a set change under float32 arithmetic or a reversed summation order?"""
    want = rank(fuse(lists, "rrf", weights, rrf_c))[0]
    f32 = rank(fuse(lists, "rrf", weights, rrf_c, dtype=np.float32))[0]
    rev = rank(fuse(lists, "rrf", weights, rrf_c, order=range(len(lists) - 1, -1, -1)))[0]
    return bool((want != f32).any() or (want != rev).any())


# ---- weighted ---------------------------------------------------------------------------------------------
WEIGHTS = {3: (0.0, 0.5, 3.0), 5: (3.0, 0.0, 0.5, 1.0, 0.5)}


# ---- sizes ------------------------------------------------------------------------------------------------
SIZE_FETCH = (1, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def many_sets_case(n_sets=70, n=600, d=16, seed=3):
    """(V, Q, offsets): n_sets sets of 0..4 sub-queries (the first three of sizes 0, 1, 4)."""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 4] + rng.integers(0, 5, size=n_sets - 3).tolist()
    V, _ = corpus(n, d, seed=seed)
    base = rng.standard_normal((n_sets, d)).astype(np.float32)
    Q = np.concatenate([base[s] + 0.5 * rng.standard_normal((sizes[s], d)).astype(np.float32) for s in range(n_sets)])
    Q = np.ascontiguousarray(Q, np.float32)
    Q.setflags(write=False)
    return V, Q, offsets_of(sizes)


@functools.lru_cache(maxsize=None)
def mixed_sets_case(n=600, d=16, seed=4):
    """(V, Q, offsets): sets of 0, 1, 16, 0 and 2 sub-queries in one call."""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 16, 0, 2]
    V, _ = corpus(n, d, seed=seed)
    base = rng.standard_normal(d).astype(np.float32)
    Q = (base + 0.6 * rng.standard_normal((sum(sizes), d))).astype(np.float32)
    Q.setflags(write=False)
    return V, Q, offsets_of(sizes)

"""Case builders and the oracle of tests/test_gpu_search_mmr.py and tests/test_gpu_store_mmr.py (MMR
search, include/vdb.h vdb_index_search_mmr), kept apart from the GPU tests so that
tests/test_mmr_precondition.py can check on the CPU that every case has the property its name
claims.

Every expectation comes from the reference arithmetic alone.  ``expected`` restates the contract
literally: the candidate list is the best ``fetch_k`` eligible rows by ``lexsort`` (key desc, row
asc) on ``oracle.ref_cpu.exact_keys``; ``S[i]`` is ``exact_keys(V[c_i], V[c])``; the selection runs
in numpy float64 scalars with separate multiply and subtract, ``np.where(s > pen, s, pen)`` for the
penalty and the first greatest value (the lowest position) as the pick.
"""
import functools

import numpy as np

from oracle import ref_cpu

METRICS = ("cosine", "euclidean")
MAX_K = 200      # csrc/vdb_mmr_plan.h kMmrMaxK
MAX_FETCH = 200  # csrc/vdb_mmr_plan.h kMmrMaxFetch
LAMBDAS = (0.0, 0.25, 0.5, 1.0, float(np.nextafter(1.0, 0.0)))


def query_block(fetch_k):
    """Queries that share one pair scratch (csrc/vdb_mmr_plan.h mmr_query_block)."""
    return max(1, min((64 << 20) // (fetch_k * fetch_k * 8), 32768))


@functools.lru_cache(maxsize=None)
def corpus(n, d, seed=0, n_queries=8):
    rng = np.random.default_rng(200033 * seed + 41 * n + d)
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


def _norms(V, metric):
    return ref_cpu.canonical_norm64(V) if metric == "cosine" and V.shape[0] else None


def candidates(q, V, fetch_k, metric, mask=None, xn=None):
    """(c, rel): the candidate list of one query, row ids by (key desc, row asc), and their keys."""
    if V.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0)
    keys = ref_cpu.exact_keys(q, V, metric, xn)
    rows = np.arange(V.shape[0]) if mask is None else np.nonzero(np.asarray(mask, bool))[0]
    c = rows[np.lexsort((rows, -keys[rows]))][:fetch_k]
    return c.astype(np.int64), keys[c]


def pair_matrix(V, c, metric, xn=None):
    """fp64 [n, n]: S[i][j] = the canonical key of (row c_i taken as the query, row c_j)."""
    Vc = V[c]
    xc = None if xn is None else xn[c]
    if len(c) == 0:
        return np.zeros((0, 0))
    return np.stack([ref_cpu.exact_keys(V[ci], Vc, metric, xc) for ci in c])


def select(rel, S, k, lam):
    """(positions, mmr values) of the contract's greedy selection."""
    n = rel.shape[0]
    m = min(k, n)
    lam = np.float64(lam)
    oml = np.float64(1.0) - lam
    picked = np.zeros(n, bool)
    pen = np.zeros(n)
    pos, val = [], []
    for t in range(m):
        if t == 0:
            pick, v = 0, lam * np.float64(rel[0])
        else:
            a = lam * rel
            b = oml * pen
            vals = a - b
            cand = np.nonzero(~picked)[0]
            pick = int(cand[np.argmax(vals[cand])])  # the first greatest: the lowest position
            v = vals[pick]
        pos.append(pick)
        val.append(v)
        picked[pick] = True
        s = S[:, pick]
        pen = s.copy() if t == 0 else np.where(s > pen, s, pen)
    return np.asarray(pos, np.int64), np.asarray(val, np.float64)


def expected(Q, V, k, fetch_k, lam, metric, mask=None, index_offset=0):
    """(scores f32 [B, k], indices i64 [B, k], keys f64 [B, k], mmr f64 [B, k]) of the contract for
    queries Q, rows V and an optional bool mask [N]."""
    V = np.asarray(V, np.float32)
    Q = np.asarray(Q, np.float32).reshape(-1, V.shape[1])
    B = Q.shape[0]
    sc = np.zeros((B, k), np.float32)
    idx = np.full((B, k), -1, np.int64)
    ks = np.full((B, k), -np.inf)
    mm = np.full((B, k), -np.inf)
    xn = _norms(V, metric)
    for b in range(B):
        c, rel = candidates(Q[b], V, fetch_k, metric, mask, xn)
        if c.size == 0:
            continue
        S = pair_matrix(V, c, metric, xn)
        pos, val = select(rel, S, k, lam)
        m = pos.size
        idx[b, :m] = c[pos] + index_offset
        ks[b, :m] = rel[pos]
        mm[b, :m] = val
        sc[b, :m] = ref_cpu.keys_to_scores(rel[pos], metric)
    return sc, idx, ks, mm


# ---- planted near-copies ---------------------------------------------------------------------------------
PLANT_N = 700
PLANT_COPIES = 12
PLANT_K = 10
PLANT_FETCH = 64
PLANT_DIMS = (33, 100, 260)
PLANT_SEED = 5


@functools.lru_cache(maxsize=None)
def planted_case(d, seed=PLANT_SEED):
    """(V, q, rows): PLANT_N random rows of which the PLANT_COPIES rows ``rows`` are q + 0.01 noise.
    Plain top-10 is ten of the copies; MMR keeps one of them at lambda 0.5 (cosine) / 0 (euclidean)
    (tests/test_mmr_precondition.py pins the seed by exactly that)."""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((PLANT_N, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    rows = np.sort(rng.choice(PLANT_N, size=PLANT_COPIES, replace=False))
    V[rows] = q + 0.01 * rng.standard_normal((PLANT_COPIES, d)).astype(np.float32)
    for x in (V, q, rows):
        x.setflags(write=False)
    return V, q, rows


# ---- ties ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_case(n=700, seed=0):
    """(V, Q) of one dim: under cosine every key and every pair similarity is +1 or -1, so nearly
    every comparison of the selection is a tie that the position rule decides."""
    rng = np.random.default_rng(seed + 7)
    V = (rng.standard_normal((n, 1)) * 3).astype(np.float32)
    V[V == 0] = 1.0
    Q = np.asarray([[2.0], [-0.5]], np.float32)
    V.setflags(write=False)
    Q.setflags(write=False)
    return V, Q


@functools.lru_cache(maxsize=None)
def duplicates_case(n=300, d=100, seed=0, copies=5):
    """(V, Q, groups of equal rows): three vectors each stored ``copies`` times at scattered rows;
    query j is near vector j, so its list opens with ``copies`` equal keys (position = row order)
    whose pair similarities are equal too."""
    V, Q = corpus(n, d, seed + 90, 3)
    V, Q = V.copy(), Q.copy()
    rng = np.random.default_rng(seed + n + d)
    rows = rng.permutation(n)[:3 * copies].reshape(3, copies)
    rows.sort(axis=1)
    for j in range(3):
        V[rows[j]] = V[rows[j, 0]]
        Q[j] = V[rows[j, 0]] + 0.01 * Q[j]
    for x in (V, Q, rows):
        x.setflags(write=False)
    return V, Q, rows

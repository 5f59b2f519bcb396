"""Case builders of tests/test_gpu_search_range.py and tests/test_gpu_store_range.py (range search,
include/vdb.h vdb_index_search_range), kept apart from the GPU tests so that
tests/test_range_precondition.py can check on the CPU that every case has the property its name
claims.

Every expectation comes from the reference arithmetic alone: a row passes query b when
``oracle.ref_cpu.exact_keys(q_b, V, metric)[row] >= kt_b``, with kt from the documented formula
in numpy fp64 (cosine: kt = t; euclidean: kt = -(t * t), one multiply), intersected with the mask;
the hits are listed in ascending row id with ``oracle.ref_cpu.keys_to_scores`` of their keys.
"""
import functools

import numpy as np

from oracle import ref_cpu

METRICS = ("cosine", "euclidean")
WG_ROWS = 512  # rows per workgroup of the scan (csrc/vdb_range_plan.h kRangeWgRows)
MAX_BLOCK = 64  # most queries per block (csrc/vdb_range_plan.h kRangeMaxBlock)
QUERY_BYTES = 128 * 1024  # a block's query bytes (csrc/vdb_range_plan.h kRangeQueryBytes)


def query_block(dim):
    """Queries per block for rows of `dim` dims (csrc/vdb_range_plan.h range_query_block; rows are
    padded to a multiple of 8 dims)."""
    dp = (dim + 7) // 8 * 8
    return max(1, min(MAX_BLOCK, QUERY_BYTES // (dp * 4)))


def kt_of(metric, thresholds):
    """Threshold(s) in score units -> the key bound, by the documented formula in fp64."""
    t = np.asarray(thresholds, dtype=np.float64)
    if metric == "cosine":
        return t.copy()
    return -(t * t)


@functools.lru_cache(maxsize=None)
def corpus(n, d, seed=0, n_queries=8):
    rng = np.random.default_rng(100003 * seed + 31 * n + d)
    V = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((n_queries, d)).astype(np.float32)
    V.setflags(write=False)
    Q.setflags(write=False)
    return V, Q


def oracle_keys(Q, V, metric):
    """fp64 [B, N]: the canonical key of every (query, row) pair."""
    Q = np.asarray(Q, np.float32).reshape(-1, V.shape[1])
    xn = ref_cpu.canonical_norm64(V) if metric == "cosine" else None
    return np.stack([ref_cpu.exact_keys(q, V, metric, xn) for q in Q])


def expected(keys, kt, cap, metric, mask=None, index_offset=0):
    """(counts [B], indices [B, cap], scores [B, cap], keys [B, cap]) of the contract for oracle
    keys [B, N], bounds kt [B] and an optional bool mask [N]."""
    keys = np.asarray(keys, np.float64)
    B, N = keys.shape
    kt = np.broadcast_to(np.asarray(kt, np.float64), (B,))
    counts = np.zeros(B, np.int64)
    idx = np.full((B, cap), -1, np.int64)
    sc = np.zeros((B, cap), np.float32)
    ks = np.full((B, cap), -np.inf)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            hit = keys[b] >= kt[b]
        if mask is not None:
            hit &= np.asarray(mask, bool)
        rows = np.nonzero(hit)[0]
        counts[b] = rows.size
        m = min(rows.size, cap)
        idx[b, :m] = rows[:m] + index_offset
        ks[b, :m] = keys[b, rows[:m]]
        sc[b, :m] = ref_cpu.keys_to_scores(keys[b, rows[:m]], metric)
    return counts, idx, sc, ks


def best_first(counts, idx, sc, ks):
    """One query's hits (a result that fits its cap) ordered as a search orders them: key
    descending, ties to the lower row."""
    n = int(counts)
    order = np.lexsort((idx[:n], -ks[:n]))
    return idx[:n][order], sc[:n][order], ks[:n][order]


def bitmap(mask_bool):
    """bool [N] -> the uint32 row_mask words."""
    return np.packbits(np.asarray(mask_bool, bool), bitorder="little").tobytes().ljust(
        (len(mask_bool) + 31) // 32 * 4, b"\0")


def words(mask_bool):
    return np.frombuffer(bitmap(mask_bool), dtype=np.uint32).copy()


# ---- thresholds ----------------------------------------------------------------------------------
def midpoint_threshold(keys_row, m, metric):
    """A threshold (score units) that exactly the m best rows of one query pass: halfway between
    the m-th and the (m + 1)-th best key (m = 0: above the best; m = N: below the worst)."""
    s = np.sort(np.asarray(keys_row, np.float64))[::-1]
    n = s.size
    upper = s[m - 1] if m > 0 else (s[0] + 1.0 if metric == "cosine" else 0.0)
    lower = s[m] if m < n else s[n - 1] - 1.0
    mid = 0.5 * (upper + lower)
    return float(mid) if metric == "cosine" else float(np.sqrt(-mid))


def midpoint_ms(n, cap):
    """The m of the midpoint cases: {0, 1, cap - 1, cap, cap + 1, N}, those inside [0, N]."""
    return sorted({m for m in (0, 1, cap - 1, cap, cap + 1, n) if 0 <= m <= n})


def cosine_equality(keys_row, row):
    """(t_in, t_out): t_in is the row's oracle key itself, so the row passes; the next fp64 up
    excludes it."""
    t = float(keys_row[row])
    return t, float(np.nextafter(t, np.inf))


# Planted offsets whose squared length is exactly 25 (integer coordinates).
_OFFSETS_25 = ((3, 4), (5, 0), (0, 5), (-3, 4), (4, -3), (-5, 0))
EUCLID_RADIUS = 5.0
EUCLID_SQ = 25.0


@functools.lru_cache(maxsize=None)
def euclid_equality_case(n, d, seed=0):
    """(V, q, planted rows): a standard-normal corpus in which the planted rows and the query are
    integer-valued and every planted row lies at squared distance exactly 25 from the query, so a
    radius of 5.0 includes them and np.nextafter(5.0, 0) excludes them.  d == 1: offsets +-5."""
    rng = np.random.default_rng(7919 * seed + 13 * n + d)
    V = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.integers(-3, 4, size=d).astype(np.float32)
    offs = ((5,), (-5,)) if d == 1 else _OFFSETS_25
    planted = np.sort(rng.choice(n, size=min(len(offs), n), replace=False))
    for r, o in zip(planted, offs):
        V[r] = q
        if d == 1:
            V[r, 0] += o[0]
        else:
            V[r, 0] += o[0]
            V[r, d - 1] += o[1]  # the last dim: beside the pad columns
    V.setflags(write=False)
    q.setflags(write=False)
    return V, q, planted


@functools.lru_cache(maxsize=None)
def duplicates_case(n, d, seed=0):
    """(V, Q, groups): a corpus in which each group of rows holds copies of the group's first row,
    so their keys are equal for every query."""
    V, Q = corpus(n, d, seed + 50)
    V = V.copy()
    rng = np.random.default_rng(seed + n + d)
    groups = []
    for size in (2, 3, 5):
        rows = np.sort(rng.choice(n, size=size, replace=False))
        V[rows] = V[rows[0]]
        groups.append(rows)
    V.setflags(write=False)
    return V, Q, tuple(groups)


# ---- hit densities ---------------------------------------------------------------------------------
DENSITIES = ("all", "none", "first_word", "last_word", "one_per_word")
DENSITY_DIM = 100  # random rows of this many dims are nowhere near a similarity of 0.9


def density_rows(name, n, rng):
    """The rows that should pass for a named hit density."""
    n_words = (n + 31) // 32
    if name == "all":
        return np.arange(n)
    if name == "none":
        return np.zeros(0, np.int64)
    if name == "first_word":
        return np.arange(min(32, n))
    if name == "last_word":
        return np.arange((n_words - 1) * 32, n)
    if name == "one_per_word":
        return np.unique(np.minimum(np.arange(n_words) * 32 + rng.integers(0, 32, size=n_words), n - 1))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def density_case(name, n, metric, seed=0):
    """(V, q, rows, threshold): a standard-normal corpus in which exactly `rows` pass `threshold`
    unmasked: they are the query plus a little noise (similarity near 1, distance near 0), every
    other row is far.  "all": the threshold that passes everything (-inf / +inf radius)."""
    d = DENSITY_DIM
    rng = np.random.default_rng(3 * seed + n + len(name))
    V = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    rows = density_rows(name, n, rng)
    if name == "all":
        t = -np.inf if metric == "cosine" else np.inf
    else:
        V[rows] = q + 0.001 * rng.standard_normal((rows.size, d)).astype(np.float32)
        t = 0.9 if metric == "cosine" else 0.5
    V.setflags(write=False)
    q.setflags(write=False)
    return V, q, rows, float(t)

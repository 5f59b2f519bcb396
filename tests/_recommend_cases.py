"""Case builders and the oracle of tests/test_gpu_search_recommend.py and
tests/test_gpu_store_recommend.py (recommend search, include/vdb.h vdb_index_search_recommend), kept
apart from the GPU tests so that tests/test_recommend_precondition.py can check on the CPU that every
case has the property its name claims.

Every expectation comes from the reference arithmetic alone.  ``build_query`` restates the contract
literally: a python loop over the examples in list order on float64 arrays (``acc = acc + e``, for
cosine ``e = x / max(norm, 1e-8)`` with ``oracle.ref_cpu.canonical_norm64``), ``acc / np.float64(n)``,
``(mp + mp) - mn`` and ``.astype(np.float32)``.  ``expected`` ranks the eligible non-example rows by
``lexsort`` (key desc, row asc) on ``oracle.ref_cpu.exact_keys`` of that vector.
"""
import functools
import os
import sys

import numpy as np

from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _mmr_cases import METRICS, bitmap_words, corpus, planted_case  # noqa: E402,F401

MAX_K = 136        # csrc/vdb_recommend_plan.h kRecMaxK
MAX_EXAMPLES = 64  # csrc/vdb_recommend_plan.h kRecMaxExamples
EPS = np.float64(1e-8)


def norms(V):
    return ref_cpu.canonical_norm64(V) if V.shape[0] else np.zeros(0)


def _mean(V, rows, metric, xn):
    acc = np.zeros(V.shape[1], np.float64)
    for r in rows:
        e = V[r].astype(np.float64)
        if metric == "cosine":
            e = e / max(np.float64(xn[r]), EPS)
        acc = acc + e
    return acc / np.float64(len(rows))


def build_query(V, pos, neg, metric, xn):
    """The built vector of one query, fp32 [dim], or None for a query without a positive."""
    if len(pos) == 0:
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        mp = _mean(V, pos, metric, xn)
        t = mp
        if len(neg):
            mn = _mean(V, neg, metric, xn)
            t = (mp + mp) - mn
        return t.astype(np.float32)


def expected(V, pos_lists, neg_lists, k, metric, mask=None, index_offset=0):
    """(scores f32 [B, k], indices i64 [B, k], keys f64 [B, k], queries f32 [B, dim]) of the contract
    for rows V, one positive and one negative list per query (``neg_lists`` None: none) and an
    optional bool mask [N].  A query without a positive, or whose vector has a non-finite element,
    is all "no result" with a zero vector."""
    V = np.asarray(V, np.float32)
    B = len(pos_lists)
    neg_lists = [[] for _ in range(B)] if neg_lists is None else neg_lists
    sc = np.zeros((B, k), np.float32)
    idx = np.full((B, k), -1, np.int64)
    ks = np.full((B, k), -np.inf)
    qs = np.zeros((B, V.shape[1]), np.float32)
    xn = norms(V)
    elig = np.ones(V.shape[0], bool) if mask is None else np.asarray(mask, bool).copy()
    for b in range(B):
        pos, neg = list(pos_lists[b]), list(neg_lists[b])
        q = build_query(V, pos, neg, metric, xn)
        if q is None or not np.isfinite(q).all():
            continue
        qs[b] = q
        keys = ref_cpu.exact_keys(q, V, metric, xn if metric == "cosine" else None)
        ok = elig.copy()
        ok[sorted(set(pos) | set(neg))] = False
        rows = np.nonzero(ok)[0]
        c = rows[np.lexsort((rows, -keys[rows]))][:k]
        m = c.size
        idx[b, :m] = c + index_offset
        ks[b, :m] = keys[c]
        sc[b, :m] = ref_cpu.keys_to_scores(keys[c], metric)
    return sc, idx, ks, qs


# ---- the shape cases ---------------------------------------------------------------------------------------
EXAMPLE_COUNTS = (1, 2, 3, 5, 17, 63, 64, 64)


@functools.lru_cache(maxsize=None)
def example_lists(n, seed=0, counts=EXAMPLE_COUNTS):
    """(pos, neg): one pair of lists per entry of ``counts`` with that many examples in all, the
    negatives' share cycling through none, one, half and all but one; distinct rows of [0, n) in
    random order."""
    rng = np.random.default_rng(7919 * seed + n)
    pos, neg = [], []
    for j, c in enumerate(counts):
        rows = rng.choice(n, size=c, replace=False).tolist()
        nn = (0, 1, c // 2, c - 1)[j % 4]
        nn = min(nn, c - 1)
        pos.append(tuple(rows[:c - nn]))
        neg.append(tuple(rows[c - nn:]))
    return tuple(pos), tuple(neg)


@functools.lru_cache(maxsize=None)
def full_house(n=700, d=100, seed=3):
    """(V, pos, neg) for k = 136 with 64 examples (k' = 200): the positives are 40 near-copies of one
    direction and the negatives 24 near-copies of the same direction a little shorter, so the examples stand at the
    head of the built query's ranking."""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, d)).astype(np.float32)
    c = rng.standard_normal(d).astype(np.float32)
    rows = rng.choice(n, size=64, replace=False)
    pos, neg = rows[:40], rows[40:]
    V[pos] = c + 0.05 * rng.standard_normal((40, d)).astype(np.float32)
    V[neg] = c * np.float32(0.9) + 0.05 * rng.standard_normal((24, d)).astype(np.float32)
    V.setflags(write=False)
    return V, tuple(int(r) for r in pos), tuple(int(r) for r in neg)


@functools.lru_cache(maxsize=None)
def order_case(n=300, d=100, seed=6):
    """(V, pos, neg): rows scaled by powers of two from 2^-20 to 2^20, so that a sum of them rounds in
    fp64 (fp32 rows of one magnitude sum exactly there, in any order) and the order of the additions
    shows in the bits, for euclidean as for cosine; lists of 17, 33 and 64 examples."""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, d)).astype(np.float32)
    V = V * np.exp2(rng.integers(-20, 21, size=(n, 1))).astype(np.float32)
    rows = rng.permutation(n).tolist()
    pos = (tuple(rows[:17]), tuple(rows[17:50]), tuple(rows[50:90]))
    neg = ((), (), tuple(rows[90:114]))
    V.setflags(write=False)
    return V, pos, neg


@functools.lru_cache(maxsize=None)
def overflow_case():
    """(V [8, 4], pos, neg) euclidean: rows of +-1.2e38, finite as fp32, whose (mp + mp) - mn passes
    fp32's range, beside an ordinary second query."""
    V = np.asarray([[1.2e38, -1.2e38, 1.0, 2.0], [-1.2e38, 1.2e38, 0.5, 1.0], [1.0, 2.0, 3.0, 4.0], [2.0, 1.0, 0.0, -1.0],
                    [0.5, 0.5, 0.5, 0.5], [-1.0, 0.0, 1.0, 2.0], [3.0, 3.0, 1.0, 0.0], [1.1e38, 1.0e38, 0.0, 1.0]], np.float32)
    V.setflags(write=False)
    return V, ((0,), (2, 3)), ((1,), (4,))

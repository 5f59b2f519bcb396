"""Case builders of tests/test_gpu_search_groups.py and tests/test_gpu_store_groups.py (grouped
search, include/vdb.h vdb_index_search_groups), kept apart from the GPU tests so that
tests/test_group_precondition.py can check on the CPU that every case has the property its name
claims.

Every expectation comes from the reference arithmetic alone: the keys are
``oracle.ref_cpu.exact_keys``; a row is eligible when its group id is >= 0 and the mask has it; the
eligible rows are ordered by ``lexsort`` (key desc, row asc), each group's first occurrence is kept,
and the first k of those are the answer.
"""
import functools

import numpy as np

from oracle import ref_cpu

METRICS = ("cosine", "euclidean")
MAX_FETCH = 200  # csrc/vdb_group_plan.h kGroupMaxFetch


def fetch_k(knob, k):
    """Rows the inner search fetches (csrc/vdb_group_plan.h group_fetch_k)."""
    f = knob if knob > 0 else (1 if k == 1 else MAX_FETCH)
    return max(min(f, MAX_FETCH), k)


@functools.lru_cache(maxsize=None)
def corpus(n, d, seed=0, n_queries=8):
    rng = np.random.default_rng(100019 * seed + 37 * n + d)
    V = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((n_queries, d)).astype(np.float32)
    V.setflags(write=False)
    Q.setflags(write=False)
    return V, Q


def oracle_keys(Q, V, metric):
    """fp64 [B, N]: the canonical key of every (query, row) pair."""
    Q = np.asarray(Q, np.float32).reshape(-1, V.shape[1])
    xn = ref_cpu.canonical_norm64(V) if metric == "cosine" else None
    if V.shape[0] == 0:
        return np.zeros((Q.shape[0], 0))
    return np.stack([ref_cpu.exact_keys(q, V, metric, xn) for q in Q])


def _eligible(groups, mask):
    el = np.asarray(groups) >= 0
    if mask is not None:
        el = el & np.asarray(mask, bool)
    return el


def ranked_rows(keys_row, groups, mask=None):
    """One query's eligible rows ordered by (key desc, row asc)."""
    rows = np.nonzero(_eligible(groups, mask))[0]
    return rows[np.lexsort((rows, -np.asarray(keys_row, np.float64)[rows]))]


def expected(keys, groups, k, metric, mask=None, index_offset=0):
    """(scores f32 [B, k], indices i64 [B, k], groups i32 [B, k], keys f64 [B, k]) of the contract
    for oracle keys [B, N], int group ids [N] and an optional bool mask [N]."""
    keys = np.asarray(keys, np.float64)
    groups = np.asarray(groups)
    B = keys.shape[0]
    sc = np.zeros((B, k), np.float32)
    idx = np.full((B, k), -1, np.int64)
    gr = np.full((B, k), -1, np.int32)
    ks = np.full((B, k), -np.inf)
    for b in range(B):
        order = ranked_rows(keys[b], groups, mask)
        _, first = np.unique(groups[order], return_index=True)  # each group's first occurrence
        best = order[np.sort(first)][:k]
        m = best.size
        idx[b, :m] = best + index_offset
        gr[b, :m] = groups[best]
        ks[b, :m] = keys[b, best]
        sc[b, :m] = ref_cpu.keys_to_scores(keys[b, best], metric)
    return sc, idx, gr, ks


def flagged(keys, groups, mask, k, k_fetch):
    """The queries that must take the exact fallback: fewer than k distinct groups among the best
    k_fetch eligible rows, and more than k_fetch eligible rows."""
    keys = np.asarray(keys, np.float64)
    groups = np.asarray(groups)
    out = []
    for b in range(keys.shape[0]):
        order = ranked_rows(keys[b], groups, mask)
        if order.size > k_fetch and np.unique(groups[order[:k_fetch]]).size < k:
            out.append(b)
    return out


def bitmap_words(mask_bool):
    """bool [N] -> the uint32 row_mask words."""
    raw = np.packbits(np.asarray(mask_bool, bool), bitorder="little").tobytes().ljust(
        (len(mask_bool) + 31) // 32 * 4, b"\0")
    return np.frombuffer(raw, dtype=np.uint32).copy()


# ---- group layouts -----------------------------------------------------------------------------------
LAYOUTS = ("one_group", "own_group", "blocks", "modulo", "random", "some_negative", "all_negative", "huge_ids")


def layout(name, n, G=7, seed=0):
    """int32 [n] group ids of a named layout (G = the number of groups where it applies)."""
    rng = np.random.default_rng(seed + 17 * n + len(name))
    r = np.arange(n)
    if name == "one_group":
        g = np.full(n, 5)
    elif name == "own_group":
        g = r[::-1].copy()
    elif name == "blocks":
        g = r * G // max(n, 1)
    elif name == "modulo":
        g = r % G
    elif name == "random":
        g = rng.integers(0, G, size=n)
    elif name == "some_negative":
        g = rng.integers(0, G, size=n)
        g[rng.random(n) < 0.3] = -1
        g[rng.random(n) < 0.1] = -(2 ** 31)
    elif name == "all_negative":
        g = -1 - rng.integers(0, 5, size=n)
    elif name == "huge_ids":
        g = (2 ** 31 - 1) - rng.integers(0, G, size=n)
    else:
        raise KeyError(name)
    return g.astype(np.int32)


def n_groups(groups, mask=None):
    groups = np.asarray(groups)
    return int(np.unique(groups[_eligible(groups, mask)]).size)


# ---- "fast" cases: no query needs the fallback at the fetch the test uses -----------------------------
FAST_G = 7


@functools.lru_cache(maxsize=None)
def fast_case(n, d, layout_name="random", seed=0, n_queries=4):
    """(V, Q, groups): random rows whose groups are spread, so the best k' rows of every query hold
    min(k, G) groups for the (k, k') pairs of fast_settings()."""
    V, Q = corpus(n, d, seed, n_queries)
    g = layout(layout_name, n, FAST_G, seed)
    g.setflags(write=False)
    return V, Q, g


def fast_settings(G):
    """The (k, group_fetch knob) pairs the fast cases run: k = 1, 2, G, G + 1, 128 and knobs k (as
    small as allowed), 32, 200."""
    ks = sorted({1, 2, max(G, 1), G + 1, 128})
    return [(k, knob) for k in ks for knob in sorted({k, 32, 200})]


# ---- duplicated rows -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def duplicates_case(n, d, seed=0):
    """(V, Q, groups, (a, b), (c, e)): rows a < b are copies of one vector in DIFFERENT groups (equal
    keys: the lower row's group ranks first) and rows c < e copies in ONE group (the lower row is
    returned); every other row has a group of its own."""
    V, Q = corpus(n, d, seed + 60, 4)
    V = V.copy()
    rng = np.random.default_rng(seed + n + d)
    a, b, c, e = np.sort(rng.choice(n, size=4, replace=False))
    V[b] = V[a]
    V[e] = V[c]
    g = np.arange(n, dtype=np.int32) + 1000
    g[e] = g[c]
    Q = Q.copy()
    Q[0] = V[a] + 0.01 * Q[0]  # the copies rank at the top of queries 0 and 1
    Q[1] = V[c] + 0.01 * Q[1]
    for x in (V, Q, g):
        x.setflags(write=False)
    return V, Q, g, (int(a), int(b)), (int(c), int(e))


# ---- dominant-group cases ------------------------------------------------------------------------------
DOM_K = 5
DOM_FETCH = 32
DOM_COPIES = 40
DOM_BATCHES = (1, 2, 64, 65, 130)


# Seeds per batch size, chosen on the CPU (tests/test_group_precondition.py) so that no cold query
# happens to lie close enough to a hot one for that query's copies to fill ITS best rows too.
DOM_SEEDS = {64: 1, 130: 5}


@functools.lru_cache(maxsize=None)
def dominant_case(n, d, batch, seed=None):
    """(V, Q, groups, hot): `hot` lists the queries that have DOM_COPIES near-copies of themselves in
    the corpus, all in one group of their own, so that group fills their best DOM_FETCH rows and
    k = DOM_K cannot be met from the fetch; every other query is a random vector.  Each other row
    has one of 50 spread groups.  Batches mix hot and cold queries (every third, from the first)."""
    seed = DOM_SEEDS.get(batch, 0) if seed is None else seed
    rng = np.random.default_rng(7 * seed + n + 3 * d + batch)
    V = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((batch, d)).astype(np.float32)
    g = rng.integers(0, 50, size=n).astype(np.int32)
    hot = list(range(0, batch, 3))[:max(1, min(6, n // (2 * DOM_COPIES)))]
    free = rng.permutation(n)
    for i, b in enumerate(hot):
        rows = np.sort(free[i * DOM_COPIES:(i + 1) * DOM_COPIES])
        V[rows] = Q[b] + 0.01 * rng.standard_normal((DOM_COPIES, d)).astype(np.float32)
        g[rows] = 1000 + i
    for x in (V, Q, g):
        x.setflags(write=False)
    return V, Q, g, tuple(hot)

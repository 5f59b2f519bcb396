"""Case builders and the oracle of tests/test_gpu_search_maxsim.py and tests/test_gpu_store_maxsim.py
(MaxSim search, include/vdb.h vdb_index_search_maxsim), kept apart from the GPU tests so that
tests/test_maxsim_precondition.py can check on the CPU that every case has the property its name
claims.

Every expectation comes from the reference arithmetic alone: the keys are
``oracle.ref_cpu.exact_keys`` (+ 0.0, one fp64 add); a row is eligible when its group id lies in
[0, n_group_slots) and the mask has it; m[t][g] is the maximum over g's eligible rows; a set's sum is
``acc = 0.0; acc = acc + m[t][g]`` for t ascending; the groups with an eligible row are ordered by
``lexsort`` (sum desc, id asc) and the first k are the answer.
"""
import functools

import numpy as np

from oracle import ref_cpu

METRICS = ("cosine", "euclidean")
MAX_K = 128        # csrc/vdb_maxsim_plan.h kMaxsimMaxK
MAX_VECTORS = 64   # ... kMaxsimMaxVectors
MAX_CELLS = 1 << 27  # ... kMaxsimMaxCells
SEG_SLOTS = 1024   # ... kMaxsimSegSlots: slots per segment of the rank kernel
WAVE_ROWS = 128    # csrc/vdb_range_plan.h: 4 words of 32 rows per wave
WG_ROWS = 512      # ... and 4 waves per workgroup

DIMS = (8, 100, 768, 1100, 2100)
ROWS = (3, 37, 513, 1300)


def query_block(d):
    """Sub-queries per scan block (csrc/vdb_range_plan.h range_query_block of the padded length)."""
    dp = (d + 63) // 64 * 64
    return max(1, min(64, (128 * 1024) // (dp * 4)))


def offsets_of(lengths):
    o = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=o[1:])
    return o


@functools.lru_cache(maxsize=None)
def corpus(n, d, seed=0, n_sub=8):
    rng = np.random.default_rng(100003 * seed + 41 * n + d)
    V = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((n_sub, d)).astype(np.float32)
    V.setflags(write=False)
    Q.setflags(write=False)
    return V, Q


@functools.lru_cache(maxsize=None)
def _keys_cached(qb, vb, qshape, vshape, metric):
    Q = np.frombuffer(qb, np.float32).reshape(qshape)
    V = np.frombuffer(vb, np.float32).reshape(vshape)
    if V.shape[0] == 0 or Q.shape[0] == 0:
        return np.zeros((Q.shape[0], V.shape[0]))
    xn = ref_cpu.canonical_norm64(V) if metric == "cosine" else None
    K = np.stack([ref_cpu.exact_keys(q, V, metric, xn) for q in Q])
    K.setflags(write=False)
    return K


def oracle_keys(Q, V, metric):
    """fp64 [n_sub, N]: the canonical key of every (sub-query, row) pair, as exact_keys gives it
    (computed once per (Q, V, metric) and shared)."""
    V = np.ascontiguousarray(V, np.float32)
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, V.shape[1]))
    return _keys_cached(Q.tobytes(), V.tobytes(), Q.shape, V.shape, metric)


def eligible(groups, n_slots, mask=None):
    g = np.asarray(groups).astype(np.int64)
    el = (g >= 0) & (g < n_slots)
    if mask is not None:
        el = el & np.asarray(mask, bool)
    return el


def maxima(keys, groups, n_slots, mask=None):
    """(ids int64 [C] ascending, M fp64 [n_sub, C]): the candidate groups and m[t][g]."""
    keys = np.asarray(keys, np.float64) + 0.0  # -0.0 -> +0.0, one add
    g = np.asarray(groups).astype(np.int64)
    rows = np.nonzero(eligible(g, n_slots, mask))[0]
    ids = np.unique(g[rows])
    M = np.empty((keys.shape[0], ids.size))
    for c, gid in enumerate(ids):
        M[:, c] = keys[:, rows[g[rows] == gid]].max(axis=1)
    return ids, M


def sums_of(M, o0, o1):
    """acc = 0.0, then acc = acc + m[t] for t ascending: one fp64 add per sub-query."""
    acc = np.zeros(M.shape[1])
    for t in range(o0, o1):
        acc = acc + M[t]
    return acc


def expected(Q, offs, V, groups, n_slots, k, metric, mask=None):
    """(scores f32 [S, k], groups i32 [S, k], sums f64 [S, k]) of the contract."""
    offs = np.asarray(offs, np.int64)
    S = offs.size - 1
    sc = np.zeros((S, k), np.float32)
    gr = np.full((S, k), -1, np.int32)
    sm = np.full((S, k), -np.inf)
    if V.shape[0] == 0:
        return sc, gr, sm
    ids, M = maxima(oracle_keys(Q, V, metric), groups, n_slots, mask)
    for s in range(S):
        o0, o1 = int(offs[s]), int(offs[s + 1])
        if o1 <= o0 or ids.size == 0:
            continue
        acc = sums_of(M, o0, o1)
        order = np.lexsort((ids, -acc))[:k]
        n = order.size
        gr[s, :n] = ids[order]
        sm[s, :n] = acc[order]
        sc[s, :n] = acc[order].astype(np.float32)  # round to nearest even
    return sc, gr, sm


def set_sums(Q, offs, V, groups, n_slots, metric, mask=None):
    """Per set: (ids, sums) of all candidates, unranked (the precondition tests look at ties)."""
    ids, M = maxima(oracle_keys(Q, V, metric), groups, n_slots, mask)
    offs = np.asarray(offs, np.int64)
    return ids, [sums_of(M, int(offs[s]), int(offs[s + 1])) for s in range(offs.size - 1)]


def bitmap_words(mask_bool):
    """bool [N] -> the uint32 row_mask words."""
    raw = np.packbits(np.asarray(mask_bool, bool), bitorder="little").tobytes().ljust(
        (len(mask_bool) + 31) // 32 * 4, b"\0")
    return np.frombuffer(raw, dtype=np.uint32).copy()


# ---- group layouts (those of tests/_group_cases.py, rebuilt) ---------------------------------------------
LAYOUTS = ("one_group", "own_group", "blocks", "modulo", "random", "some_negative", "past_slots")
LAYOUT_G = 7
PAST_SLOTS = 5  # "past_slots": the call states this many slots, ids run to LAYOUT_G + 2


def layout(name, n, G=LAYOUT_G, seed=0):
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
    elif name == "past_slots":  # ids 0 .. G + 1, and a few huge ones: those >= PAST_SLOTS are skipped
        g = rng.integers(0, G + 2, size=n)
        g[rng.random(n) < 0.05] = 2 ** 31 - 1
    else:
        raise KeyError(name)
    g = g.astype(np.int32)
    g.setflags(write=False)
    return g


def slots_of(name, groups):
    """The n_group_slots a test states for a layout: one past the greatest id (at least 1), but
    PAST_SLOTS for "past_slots"."""
    if name == "past_slots":
        return PAST_SLOTS
    return max(int(np.asarray(groups).max(initial=-1)) + 1, 1)


SPARSE_SLOTS = 5000  # more than four rank segments of SEG_SLOTS slots


def sparse_layout(n):
    """int32 [n]: distinct ids spread over [0, SPARSE_SLOTS) in no row order (n <= 1300), but every
    seventh row in one larger group."""
    g = layout("own_group", n).astype(np.int64) * 3 + (np.arange(n) % 3 == 0) * 1000
    g[::7] = g[3]
    g = g.astype(np.int32)
    g.setflags(write=False)
    return g


def blocks_runs(n, G=LAYOUT_G):
    """The first row of every run of the "blocks" layout."""
    g = layout("blocks", n, G)
    return np.nonzero(np.diff(g, prepend=-1))[0]


# ---- masks -----------------------------------------------------------------------------------------------
MASKS = ("cut_run", "wave_tail", "drop_group", "nothing")


def mask_of(name, groups, n_slots):
    """bool [N] of a named mask over a layout (and for "drop_group" the id it removes, else None)."""
    g = np.asarray(groups)
    n = g.size
    m = np.ones(n, bool)
    dropped = None
    if name == "cut_run":  # rows out of the middle of a run: the run's rows on both sides stay
        lo, hi = n // 4, n // 4 + max(n // 8, 1)
        m[lo:hi] = False
    elif name == "wave_tail":  # the last rows of the first wave's range (and of the last wave's)
        m[min(WAVE_ROWS, n) - min(40, n // 2):min(WAVE_ROWS, n)] = False
        m[n - max(n // 10, 1):] = False
    elif name == "drop_group":
        ids = np.unique(g[(g >= 0) & (g.astype(np.int64) < n_slots)])
        dropped = int(ids[ids.size // 2])
        m[g == dropped] = False
    elif name == "nothing":
        m[:] = False
    else:
        raise KeyError(name)
    return m, dropped


# ---- sets ------------------------------------------------------------------------------------------------
SET_LENGTHS = (0, 1, 2, 33, 64)


def straddle_sets(d):
    """(n_sub, lengths): one more sub-query than a scan block holds, in sets of which one straddles the
    block boundary and the last starts right at it or behind it."""
    qb = query_block(d)
    n_sub = qb + 1
    a = qb // 2
    return n_sub, [a, n_sub - a]  # the second set runs from a across qb to the end


# ---- duplicated documents: bit-equal sums ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_case(n_docs=9, rows_per_doc=5, d=100, seed=0):
    """(V, Q, groups, (a, b)): documents of rows_per_doc consecutive rows; document b is a copy of
    document a < b with its rows in another order, so every maximum and hence every sum is bit-equal
    and a must come first."""
    rng = np.random.default_rng(7 + seed)
    V = rng.standard_normal((n_docs * rows_per_doc, d)).astype(np.float32)
    Q = rng.standard_normal((6, d)).astype(np.float32)
    a, b = 2, 6
    perm = rng.permutation(rows_per_doc)
    V[b * rows_per_doc:(b + 1) * rows_per_doc] = V[a * rows_per_doc:(a + 1) * rows_per_doc][perm]
    # the pair near the top: the queries lean towards document a's rows
    Q = (V[a * rows_per_doc + np.arange(6) % rows_per_doc] + 0.1 * Q).astype(np.float32)
    g = (np.arange(n_docs * rows_per_doc) // rows_per_doc).astype(np.int32)
    for x in (V, Q, g):
        x.setflags(write=False)
    return V, Q, g, (a, b)


# ---- a query equal to a stored row (euclidean: the key is -0.0) ------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_match_case(n=37, d=8, seed=0):
    """(V, Q, groups, row): Q[0] is V[row]; its euclidean key against that row is -0.0."""
    V, Q = corpus(n, d, seed + 11, 4)
    Q = Q.copy()
    row = 2
    Q[0] = V[row]
    g = layout("modulo", n)
    Q.setflags(write=False)
    return V, Q, g, row

"""Shared cases of the filter-operator tests: seeded fp64 columns and predicates for
vdb_index_filter_mask, its numpy restatement, and the per-row oracles in plain Python (one for a
predicate over column values, one for the condition language over metadata dicts).

The columns hold what the contract names: rows without a value (NaN), +-inf, -0.0 and +0.0, and a
few small values the predicates' bounds are equal to.  The predicates cover 0, 1 and 8 clauses,
every flag combination, bounds equal to stored values, +-inf bounds and lo > hi.
(Preconditions: tests/test_filter_precondition.py.)"""
import math

import numpy as np

LO, HI, NEG = 1, 2, 4  # include/vdb.h VDB_FILTER_LO_INCL / HI_INCL / NEGATE
N_COLS = 3
SIZES = (1, 31, 32, 33, 63, 64, 65, 97, 255, 256, 257, 4099)
PREDS = (1, 3, 256)
INF = math.inf
# every column draws from this pool (NaN = no value); the bounds below are pool values
POOL = np.array([np.nan, -np.inf, np.inf, -0.0, 0.0, 1.0, 2.0, 2.5, 3.0, 5.0, -4.0, np.nan], dtype=np.float64)


def columns(n, seed=0):
    """[N_COLS][n] fp64: each column starts with the pool (rotated per column), then draws from it."""
    rng = np.random.default_rng(1000 + seed)
    cols = np.empty((N_COLS, n), dtype=np.float64)
    for c in range(N_COLS):
        head = np.roll(POOL, c * 5)
        body = POOL[rng.integers(0, POOL.size, size=n)]
        body[:min(n, head.size)] = head[:min(n, head.size)]
        cols[c] = body
    return cols


# (name, clauses): the named predicates; a clause is (slot, lo, hi, flags)
NAMED = [
    ("closed 1..3", [(0, 1.0, 3.0, LO | HI)]),
    ("no clauses", []),
    ("eight clauses", [(0, -4.0, 5.0, LO | HI), (1, -INF, INF, LO | HI), (2, 2.0, 2.0, LO | HI | NEG),
                       (0, 2.5, 2.5, LO | HI | NEG), (1, -INF, 5.0, LO), (2, -INF, INF, 0), (0, 3.0, 1.0, NEG),
                       (1, -4.0, -4.0, LO | HI | NEG)]),
    ("flags 0", [(1, 1.0, 3.0, 0)]),
    ("flags LO", [(1, 1.0, 3.0, LO)]),
    ("flags HI", [(1, 1.0, 3.0, HI)]),
    ("flags LO|HI", [(1, 1.0, 3.0, LO | HI)]),
    ("flags NEG", [(1, 1.0, 3.0, NEG)]),
    ("flags NEG|LO", [(1, 1.0, 3.0, NEG | LO)]),
    ("flags NEG|HI", [(1, 1.0, 3.0, NEG | HI)]),
    ("flags NEG|LO|HI", [(1, 1.0, 3.0, NEG | LO | HI)]),
    ("equals 0 (both zeros)", [(2, 0.0, 0.0, LO | HI)]),
    ("equals -0 (both zeros)", [(2, -0.0, -0.0, LO | HI)]),
    ("not equal 2", [(2, 2.0, 2.0, LO | HI | NEG)]),
    ("exists", [(0, -INF, INF, LO | HI)]),
    ("not exists", [(0, -INF, INF, LO | HI | NEG)]),
    ("finite only", [(0, -INF, INF, 0)]),
    ("equals +inf", [(1, INF, INF, LO | HI)]),
    ("equals -inf", [(1, -INF, -INF, LO | HI)]),
    ("lo > hi: empty", [(0, 3.0, 1.0, LO | HI)]),
    ("lo > hi negated: full", [(0, 3.0, 1.0, LO | HI | NEG)]),
    ("exclusive point: empty", [(2, 2.0, 2.0, 0)]),
    ("two columns", [(0, 0.0, INF, LO | HI), (2, -INF, 2.5, LO)]),
    ("half open below", [(2, -INF, 2.0, HI)]),
]
EMPTY = {"lo > hi: empty", "exclusive point: empty"}
FULL = {"no clauses", "lo > hi negated: full"}


def predicates(P, seed=0):
    """P predicates.  1: one closed interval; 3: no clauses, one clause, eight clauses; more: the
    named ones, then seeded draws over the pool's finite and infinite values and every flag."""
    if P == 1:
        return [list(NAMED[0][1])]
    if P == 3:
        return [list(NAMED[1][1]), list(NAMED[0][1]), list(NAMED[2][1])]
    rng = np.random.default_rng(2000 + seed)
    bounds = [v for v in POOL.tolist() if not math.isnan(v)]
    out = [list(cl) for _, cl in NAMED][:P]
    while len(out) < P:
        nc = int(rng.integers(0, 9)) if len(out) % 7 == 0 else int(rng.integers(1, 4))
        out.append([(int(rng.integers(0, N_COLS)), bounds[int(rng.integers(0, len(bounds)))],
                     bounds[int(rng.integers(0, len(bounds)))], int(rng.integers(0, 8))) for _ in range(nc)])
    return out


def n_words(n):
    return (n + 31) // 32


def words(bits):
    """bool [n] -> uint32 [ceil(n / 32)], the row_mask layout."""
    n = bits.shape[0]
    b = np.zeros(n_words(n) * 32, dtype=bool)
    b[:n] = bits
    return np.packbits(b, bitorder="little").view("<u4").astype(np.uint32)


def unwords(w, n):
    return np.unpackbits(np.ascontiguousarray(w, np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


def clause_bits(v, lo, hi, flags):
    """The clause over a whole column, in numpy: plain IEEE fp64 compares."""
    with np.errstate(invalid="ignore"):
        has = ~(v != v)
        t = has & ((v >= lo) if flags & LO else (v > lo)) & ((v <= hi) if flags & HI else (v < hi))
    return ~t if flags & NEG else t


def restate(cols, preds, base=None):
    """The numpy restatement -> (masks uint32 [P, W], counts int64 [P])."""
    n = cols.shape[1]
    masks = np.zeros((len(preds), n_words(n)), dtype=np.uint32)
    counts = np.zeros(len(preds), dtype=np.int64)
    for p, pred in enumerate(preds):
        bits = np.ones(n, dtype=bool)
        for slot, lo, hi, flags in pred:
            bits &= clause_bits(cols[slot], lo, hi, flags)
        if base is not None:
            bits &= unwords(base[p], n)
        masks[p] = words(bits)
        counts[p] = int(bits.sum())
    return masks, counts


def base_masks(P, n, seed=0):
    rng = np.random.default_rng(3000 + seed)
    return rng.integers(0, 2**32, size=(P, n_words(n)), dtype=np.uint64).astype(np.uint32)


def oracle_row(values, pred):
    """One row (its value per slot) against one predicate, in plain Python."""
    for slot, lo, hi, flags in pred:
        v = values[slot]
        if math.isnan(v):
            t = False
        else:
            t = (v >= lo if flags & LO else v > lo) and (v <= hi if flags & HI else v < hi)
        if (not t) if not flags & NEG else t:
            return False
    return True


def oracle_bits(cols, pred):
    return np.array([oracle_row([float(cols[c][r]) for c in range(cols.shape[0])], pred)
                     for r in range(cols.shape[1])], dtype=bool)


# ---- the condition language over metadata dicts ------------------------------------------------------
_CMP = {"$gt": lambda a, b: a > b, "$gte": lambda a, b: a >= b, "$lt": lambda a, b: a < b, "$lte": lambda a, b: a <= b}


def _is_cond(v):
    return isinstance(v, dict) and len(v) > 0 and all(isinstance(k, str) and k.startswith("$") for k in v)


def _is_num(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and not (isinstance(v, float) and math.isnan(v))


def meta_matches(meta, filt):
    """The per-row oracle of the filter language: plain Python over one metadata dict."""
    m = meta if isinstance(meta, dict) else {}
    for key, want in filt.items():
        if not _is_cond(want):
            if not m.get(key) == want:
                return False
            continue
        for op, x in want.items():
            if op == "$eq":
                ok = m.get(key) == x
            elif op == "$ne":
                ok = not (m.get(key) == x)
            elif op == "$in":
                ok = any(m.get(key) == y for y in x)
            elif op == "$nin":
                ok = not any(m.get(key) == y for y in x)
            elif op == "$exists":
                ok = (key in m) == x
            else:
                ok = key in m and _is_num(m[key]) and _CMP[op](m[key], x)
            if not ok:
                return False
    return True


def meta_bits(metadata, filt, n=None):
    n = len(metadata) if n is None else n
    return np.array([meta_matches(metadata[r] if r < len(metadata) else {}, filt) for r in range(n)], dtype=bool)


def store_metadata(n, seed=0):
    """n metadata dicts with numeric (int and float), string, missing and bool values."""
    rng = np.random.default_rng(4000 + seed)
    out = []
    for r in range(n):
        m = {"id": r, "tenant": f"t{r % 4}"}
        u = r % 10
        if u < 6:
            m["ts"] = int(rng.integers(0, 1000))
        elif u == 6:
            m["ts"] = float(rng.integers(0, 1000)) + 0.5
        elif u == 7:
            m["ts"] = "yesterday"
        elif u == 8:
            m["ts"] = bool(r % 20 == 8)
        # u == 9: no "ts"
        if r % 3:
            m["price"] = float(rng.integers(0, 40)) / 4.0
        if r % 11 == 0:
            m["price"] = float("nan")
        out.append(m)
    return out


STORE_FILTERS = [
    {"ts": {"$gte": 500}},
    {"ts": {"$lt": 250.5}},
    {"ts": {"$gt": 100, "$lte": 900}},
    {"ts": {"$gte": 0, "$lte": 1}},
    {"tenant": "t1", "ts": {"$gte": 300}},
    {"tenant": {"$in": ["t0", "t2"]}, "price": {"$lt": 5}},
    {"price": {"$gte": 2.5, "$lt": 7.25}, "ts": {"$gt": 10}},
    {"ts": {"$ne": "yesterday", "$gt": 50}},
    {"ts": {"$exists": True, "$lt": 800}},
]

"""Case tables of tests/test_gpu_update.py (in-place row update, include/vdb.h vdb_index_update),
kept apart from the GPU tests so that tests/test_update_precondition.py can check their
preconditions on the CPU: that every pattern changes at least one query's answer, and that the
planted effects (a new top 1, a lost self-match) hold wherever their rows are updated.

Every expectation comes from the reference arithmetic alone: ``V2 = V.copy(); V2[rows] = new`` and
``oracle.ref_cpu.exact_search`` over ``V2``.  The data, the queries, the masks and the reduced
settings are those of tests/_remove_cases.py.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _planted as pl  # noqa: E402
import _remove_cases as rc  # noqa: E402
from oracle import ref_cpu  # noqa: E402

N, DIMS, B, K = rc.N, rc.DIMS, rc.B, rc.K
POISON_IDX = rc.POISON_IDX

PATTERNS = ("first", "last", "word", "every_other", "block", "rand1", "rand50", "all", "reversed_ids")
REDUCED = ("first", "block", "rand50", "all")
REDUCED_SETTINGS = rc.REDUCED_SETTINGS
BIG_SCALE = np.float32(50.0)  # the loud updated row: 50x the corpus scale, its int8 copy clips


def pattern_rows(name, count=N):
    """Row ids in the order the call gives them (pairwise distinct)."""
    if name == "all":
        return np.arange(count)
    if name == "reversed_ids":
        return rc.pattern_rows("rand50", count)[::-1].copy()
    return rc.pattern_rows(name, count)


def new_rows(name, D, count=N):
    """The new value of every row of the pattern, in the pattern's order: fresh standard-normal
    draws with five plants -- the new row 0 is Q[2] (that query's new top 1), the new row
    count - 1 is a fresh draw like the rest (Q[1], its old value, loses its self-match), one
    updated row is all zeros, one is 50x the corpus scale, and the first updated row that is
    neither row 0 nor row count - 1 is Q[3] (so a pattern that touches neither end still changes
    an answer)."""
    rows = pattern_rows(name, count)
    _, Q = rc.rows_data(count, D, 100 + D)
    rng = np.random.default_rng(sum(map(ord, name)) + 7 * D + count)
    new = rng.standard_normal((rows.size, D)).astype(np.float32)
    free = np.nonzero((rows != 0) & (rows != count - 1))[0]  # list positions without another plant
    if free.size >= 3:
        new[free[free.size // 3]] = 0.0
        new[free[2 * free.size // 3]] *= BIG_SCALE
        new[free[0]] = Q[3]
    at0 = np.nonzero(rows == 0)[0]
    if at0.size:
        new[at0[0]] = Q[2]
    new.setflags(write=False)
    return new


def zero_and_loud(name, count=N):
    """List positions of the all-zero and the 50x row (None, None where the pattern is too small)."""
    rows = pattern_rows(name, count)
    free = np.nonzero((rows != 0) & (rows != count - 1))[0]
    if free.size < 3:
        return None, None
    return int(free[free.size // 3]), int(free[2 * free.size // 3])


@functools.lru_cache(maxsize=None)
def updated(name, D):
    """V2 [N, D]: the corpus after the pattern's update (read-only)."""
    V, _ = rc.rows_data(N, D, 100 + D)
    V2 = V.copy()
    V2[pattern_rows(name)] = new_rows(name, D)
    V2.setflags(write=False)
    return V2


@functools.lru_cache(maxsize=None)
def base_oracle(D, metric):
    V, Q = rc.rows_data(N, D, 100 + D)
    return ref_cpu.exact_search(Q, V, K, metric), ref_cpu.exact_search(Q, V, K, metric, row_mask=rc.filter_mask(N))


@functools.lru_cache(maxsize=None)
def pattern_oracle(name, D, metric):
    """(V2, unmasked oracle, masked oracle) of one pattern (shared, computed once)."""
    _, Q = rc.rows_data(N, D, 100 + D)
    V2 = updated(name, D)
    return V2, ref_cpu.exact_search(Q, V2, K, metric), ref_cpu.exact_search(Q, V2, K, metric, row_mask=rc.filter_mask(N))


def pattern_cases():
    out = [(D, "cosine", "auto", p) for D in DIMS for p in PATTERNS]
    out += [(D, m, prec, p) for D in DIMS for m, prec in REDUCED_SETTINGS for p in REDUCED]
    return out


def pattern_id(c):
    return f"D{c[0]}-{c[1]}-{c[2]}-{c[3]}"


# ---- chunks ------------------------------------------------------------------------------------
CHUNK = 1000  # update_chunk: rand50's 2 501 rows -> chunks of 1000, 1000 and 501

# ---- past the re-derivation phase --------------------------------------------------------------
# 70 017 rows in one add: mu / sx / dir come from the first 65 536 of them and are final
# (csrc/vdb_api.cpp kDirRows), so an update meets them frozen for good.
BIG_N, BIG_D, DIR_ROWS = rc.BIG_N, rc.BIG_D, 65536


def big_rows():
    rng = np.random.default_rng(170017)
    return rng.permutation(BIG_N)[: BIG_N * 3 // 10]  # unsorted


@functools.lru_cache(maxsize=None)
def big_oracle(metric="cosine"):
    V, Q = rc.rows_data(BIG_N, BIG_D, 7)
    rows = big_rows()
    V2 = V.copy()
    V2[rows] = np.random.default_rng(270017).standard_normal((rows.size, BIG_D)).astype(np.float32)
    V2[rows[0]] = Q[2]
    V2.setflags(write=False)
    return V2, ref_cpu.exact_search(Q, V2, K, metric)


# One chunk of more than COLSUM_LONG_FROM rows: the long form of the list column sums
# (csrc/vdb_update.hip kUpdColsumLongFrom; kUpdColsumRowsLong entries per workgroup, the last partial).
COLSUM_LONG_FROM, COLSUM_ROWS_LONG = 32768, 512


def long_rows():
    return np.random.default_rng(370017).permutation(BIG_N)[: BIG_N // 2]  # 35 008 rows, unsorted


@functools.lru_cache(maxsize=None)
def long_oracle(metric="cosine"):
    V, Q = rc.rows_data(BIG_N, BIG_D, 7)
    rows = long_rows()
    V2 = V.copy()
    V2[rows] = np.random.default_rng(470017).standard_normal((rows.size, BIG_D)).astype(np.float32)
    V2[rows[-1]] = Q[2]
    V2.setflags(write=False)
    return V2, ref_cpu.exact_search(Q, V2, K, metric)


# ---- certification survives (planted-gap data) -------------------------------------------------
def cert_rows(n, d):
    """A random half of the rows (unsorted)."""
    return np.random.default_rng(n + d + 1).permutation(n)[: n // 2]


@functools.lru_cache(maxsize=None)
def cert_updated(n, d, b, k):
    """(rows, V2): the chosen rows take a shuffle of their own old values, so the multiset of rows
    -- the planted gap and every bound with it -- is that of tests/test_planted_precondition.py."""
    V, _, _ = pl.data(n, d, b, k, rc.cert_seed(n, d, b, k))
    rows = cert_rows(n, d)
    V2 = V.copy()
    V2[rows] = V[np.random.default_rng(n + d + 2).permutation(rows)]
    V2.setflags(write=False)
    return rows, V2


@functools.lru_cache(maxsize=None)
def cert_oracle(n, d, b, k, metric):
    _, Q, _ = pl.data(n, d, b, k, rc.cert_seed(n, d, b, k))
    return ref_cpu.exact_search(Q, cert_updated(n, d, b, k)[1], k, metric)

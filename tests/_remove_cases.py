"""Case tables of tests/test_gpu_remove.py (row removal, include/vdb.h vdb_index_remove), kept
apart from the GPU tests so that tests/test_remove_precondition.py can check their preconditions
on the CPU: that each pattern removes what its name says, that the chunked case really has chunks
with no survivor and chunks with no removed row and more bitmap words than one workgroup of the
keep-count scan handles, and that the planted-gap cases still force certification after a remove.

Every expectation comes from the reference arithmetic alone: ``np.delete`` on the rows and
``oracle.ref_cpu.exact_search`` over the result.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _planted as pl  # noqa: E402
from oracle import ref_cpu  # noqa: E402

POISON_IDX = -7  # what every output buffer holds before a call (keys and scores: NaN)

# ---- the pattern cases -----------------------------------------------------------------------
N = 5003          # last bitmap word partial (5003 = 156 * 32 + 11), last 1024-row granule partial
DIMS = (96, 200)  # D = 200: Dp = 256, the pad columns must stay zero
B, K = 16, 10
SCAN_WG_WORDS = 1024  # bitmap words per workgroup of the keep-count scan (csrc/vdb_compact_plan.h kScanWgWords)

PATTERNS = ("first", "last", "word", "granule", "every_other", "block", "rand1", "rand50", "all_but_one",
            "none", "past_count")
REDUCED = ("first", "last", "block", "rand50")
# (metric, precision) of the reduced set; the full list runs under ("cosine", "auto")
REDUCED_SETTINGS = (("euclidean", "auto"), ("cosine", "bf16x3"), ("cosine", "fp32"), ("cosine", "i8x3"),
                    ("euclidean", "i8x3"))


def n_words(count):
    return (count + 31) // 32


def words_of(rows, count, stray_high_bits=False):
    """uint32 remove bitmap over `count` rows with the bits of `rows` set (stray_high_bits: also
    every bit of the last word at or past count, which the library must ignore)."""
    bits = np.zeros(n_words(count) * 32, np.uint8)
    bits[np.asarray(rows, dtype=np.int64)] = 1
    if stray_high_bits:
        bits[count:] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


def pattern_rows(name, count=N):
    """Sorted row ids the pattern removes."""
    rng = np.random.default_rng(sum(map(ord, name)) + count)
    if name == "first":
        return np.array([0])
    if name == "last":
        return np.array([count - 1])
    if name == "word":
        return np.arange(17 * 32, 18 * 32)
    if name == "granule":
        return np.arange(1024, 2048)
    if name == "every_other":
        return np.arange(0, count, 2)
    if name == "block":
        return np.arange(1000, 1500)  # starts at bit 8 of word 31, ends at bit 28 of word 46
    if name == "rand1":
        return np.sort(rng.permutation(count)[: count // 100])
    if name == "rand50":
        return np.sort(rng.permutation(count)[: count // 2])
    if name == "all_but_one":
        return np.delete(np.arange(count), 2501)
    if name in ("none", "past_count"):
        return np.zeros(0, np.int64)
    raise ValueError(name)


def pattern_words(name, count=N):
    return words_of(pattern_rows(name, count), count, stray_high_bits=(name == "past_count"))


@functools.lru_cache(maxsize=None)
def rows_data(count, D, seed):
    """(V [count, D], Q [B, D]) standard normal, read-only; two queries are corpus rows."""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((count, D)).astype(np.float32)
    Q = rng.standard_normal((B, D)).astype(np.float32)
    Q[0] = V[count // 2]
    Q[1] = V[count - 1]
    for a in (V, Q):
        a.setflags(write=False)
    return V, Q


def filter_mask(count):
    """The row_mask of the masked search over `count` rows (new numbering): two rows in three."""
    return (np.arange(count) % 3) != 1


def mask_words(mask):
    bits = np.zeros(n_words(mask.size) * 32, np.uint8)
    bits[: mask.size] = mask
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


@functools.lru_cache(maxsize=None)
def pattern_oracle(name, D, metric):
    """(survivors [M, D], unmasked oracle, masked oracle) of one pattern (shared, computed once)."""
    V, Q = rows_data(N, D, 100 + D)
    S = np.delete(V, pattern_rows(name), axis=0)
    out = (S, ref_cpu.exact_search(Q, S, K, metric), ref_cpu.exact_search(Q, S, K, metric, row_mask=filter_mask(S.shape[0])))
    S.setflags(write=False)
    return out


def pattern_cases():
    out = [(D, "cosine", "auto", p) for D in DIMS for p in PATTERNS]
    out += [(D, m, prec, p) for D in DIMS for m, prec in REDUCED_SETTINGS for p in REDUCED]
    return out


def pattern_id(c):
    return f"D{c[0]}-{c[1]}-{c[2]}-{c[3]}"


# ---- the chunked case --------------------------------------------------------------------------
# 70 017 rows = 2 189 bitmap words: more than the SCAN_WG_WORDS = 1024 words one workgroup of the
# keep-count scan handles (three workgroups, the last partial), so the scan of partials and the
# add-back matter.  remove_chunk = 1000 rows -> 31 words = 992 rows per chunk, 71 chunks.  Row 0 is
# removed, so chunk c covers rows [992 c, 992 (c + 1)); chunk 5 loses every row, chunk 9 none.
BIG_N, BIG_D, BIG_CHUNK = 70017, 96, 1000
BIG_CHUNK_ROWS = BIG_CHUNK // 32 * 32
BIG_ALL_REMOVED, BIG_ALL_KEPT = 5, 9


def big_rows():
    rng = np.random.default_rng(70017)
    gone = rng.random(BIG_N) < 0.30
    gone[0] = True
    gone[BIG_ALL_REMOVED * BIG_CHUNK_ROWS:(BIG_ALL_REMOVED + 1) * BIG_CHUNK_ROWS] = True
    gone[BIG_ALL_KEPT * BIG_CHUNK_ROWS:(BIG_ALL_KEPT + 1) * BIG_CHUNK_ROWS] = False
    return np.nonzero(gone)[0]


@functools.lru_cache(maxsize=None)
def big_oracle(metric="cosine"):
    V, Q = rows_data(BIG_N, BIG_D, 7)
    S = np.delete(V, big_rows(), axis=0)
    S.setflags(write=False)
    return S, ref_cpu.exact_search(Q, S, K, metric)


# ---- certification survives (planted-gap data) -----------------------------------------------------
CERT_SHAPES = (("short", 6000, 96, 16, 10), ("ragged", 6000, 200, 70, 10))
CERT_PRECISIONS = ("i8", "i8x3", "bf16x3", "auto")


def cert_cases():
    return [(name, n, d, b, k, m, p) for name, n, d, b, k in CERT_SHAPES for m in pl.BOTH for p in CERT_PRECISIONS]


def cert_id(c):
    return f"{c[0]}-{c[5]}-{c[6]}"


def cert_seed(n, d, b, k):
    return n + 3 * d + 5 * b + 7 * k  # tests/_planted.py _case: the variant matrix's data sets


def cert_removed(n, d, b, k):
    """A random quarter of the rows that are in no query's planted top k."""
    _, _, pos = pl.data(n, d, b, k, cert_seed(n, d, b, k))
    free = np.setdiff1d(np.arange(n), pos.ravel())
    rng = np.random.default_rng(n + d)
    return np.sort(rng.permutation(free)[: free.size // 4])


@functools.lru_cache(maxsize=None)
def cert_oracle(n, d, b, k, metric):
    """exact_search at k + 1 over the surviving rows: (scores, indices, keys) [B, k] and the gap
    s_k - s_{k+1} [B]."""
    V, Q, _ = pl.data(n, d, b, k, cert_seed(n, d, b, k))
    S = np.delete(V, cert_removed(n, d, b, k), axis=0)
    es, ei, ek = ref_cpu.exact_search(Q, S, k + 1, metric)
    return es[:, :k].copy(), ei[:, :k].copy(), ek[:, :k].copy(), ek[:, k - 1] - ek[:, k]

"""Cases, fp64 references and derived error bounds for the stand-alone operators of
csrc/vdb_ops.hip (vdb_similarity_matrix, vdb_normalize_rows, vdb_topk_scores), shared by
tests/test_gpu_ops_alone.py (the kernels) and tests/test_ops_precondition.py (the cases
themselves, on the CPU).  No GPU and no library here: numpy only.

Bounds.  u = 2^-24 is the fp32 unit roundoff and gamma(n) = n u / (1 - n u).  A sum of D products
carries at most D roundings per term whatever the order of summation and with or without fused
multiply-add, so the bounds below hold for an MFMA accumulation, a butterfly reduction and numpy's
pairwise sum alike.  Every reference is fp64 numpy over the same fp32 inputs.

  dot product   |out - ref| <= gamma(D) A,  A = sum_d |q_d x_d|
  cosine        |out - ref| <= gamma(D) A / (max(|q|, c) max(|x|, c)) + (gamma(D) + 10 u) |ref|
                c = float32(1e-8), the kernel's clamp; 10 u: two square roots, two reciprocals and
                two multiplies at 1 to 2 ulp each (the two sums of squares are the gamma(D))
  euclidean     |out - ref| <= (gamma(D) / 2 + 3 u) ref   (the square root halves the sum's error)
  normalise     |out - ref| <= (gamma(D) / 2 + 3 u) |ref| per element, ref = x_d / max(|x|, c)
  top-k         exact

Non-zero magnitudes stay within [2^-20, 2^20] (nothing under- or overflows in fp32); the one
exception is the row of norm 1e-10 that exercises the clamp.
"""
import numpy as np

U = 2.0 ** -24
C = float(np.float32(1e-8))
METRICS = ("cosine", "euclidean", "dot_product")
TOPK_CHUNK = 16384  # vdb_ops.hip
POISON_IDX = -7
POISON_BITS = 0xDEADBEEF  # as fp32: a finite -6.26e18 no operator can produce from these inputs
TINY_NORM = 1e-10
COSINE_HEADER_ATOL = 1e-4  # include/vdb.h's own promise, asserted where D <= 768


def gamma(n):
    return n * U / (1.0 - n * U)


def ratio(err, bound):
    """Largest err / bound; an error against a zero bound counts as infinite, 0 / 0 as 0."""
    err = np.asarray(err, np.float64)
    bound = np.asarray(bound, np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


# =============================================================================
# A. score matrix
# =============================================================================
# (N, D, B): N around the 128-row tile, D around the 32-dim slab and the k-step of 2, B around the
# 32-query tile (more than one blockIdx.y at 33 and 70); one larger case.
MATRIX_SHAPES = [
    (1, 1, 1), (1, 64, 32), (127, 2, 31), (127, 100, 33), (128, 31, 32), (128, 100, 1), (129, 32, 33),
    (129, 1, 70), (300, 33, 70), (300, 64, 31), (300, 2, 5), (4097, 768, 5),
]


def _clamp_magnitudes(a):
    lo = np.float32(2.0 ** -20)
    small = (np.abs(a) < lo) & (a != 0)
    a[small] = np.where(np.signbit(a[small]), -lo, lo)
    return a


def scaled_normal(rng, n, D, query=False):
    """Normal rows, row r scaled by 2^(r mod 5) (queries: 2^-(b mod 3)): a norm taken from the
    wrong lane or row misses by a factor, not by percent."""
    a = rng.standard_normal((n, D)).astype(np.float32)
    r = np.arange(n)
    scale = np.exp2(-(r % 3)) if query else np.exp2(r % 5)
    return _clamp_magnitudes(a * scale[:, None].astype(np.float32))


def tiny_row(rng, D):
    g = rng.standard_normal(D)
    return (g / np.linalg.norm(g) * TINY_NORM).astype(np.float32)


def matrix_data(N, D, B):
    """(X [N, D], Q [B, D], roles).  roles maps 'zero_row', 'tiny_row', 'equal_row' (with
    'equal_query') and 'zero_query' to their indices where the shape has room for them."""
    rng = np.random.default_rng(1000 * N + 10 * D + B)
    X = scaled_normal(rng, N, D)
    Q = scaled_normal(rng, B, D, query=True)
    roles = {}
    if B >= 2:
        roles["zero_query"] = B - 1
        Q[B - 1] = 0
    if N >= 4:
        roles["zero_row"] = N - 1  # in the ragged last tile
        X[N - 1] = 0
        roles["tiny_row"] = 1
        X[1] = tiny_row(rng, D)
        roles["equal_row"], roles["equal_query"] = N // 2, 0
        X[N // 2] = Q[0]
    elif N == 1 and D == 1:
        roles["equal_row"], roles["equal_query"] = 0, 0
        X[0] = Q[0]
    elif N == 1:
        roles["tiny_row"] = 0
        X[0] = tiny_row(rng, D)
    return X, Q, roles


NEAR_D, NEAR_N = 384, 64


def near_rows(seed=77):
    """Euclidean only: 64 rows and, for each, a query 1e-3 g away from it."""
    rng = np.random.default_rng(seed)
    X = scaled_normal(rng, NEAR_N, NEAR_D)
    g = rng.standard_normal((NEAR_N, NEAR_D))
    Q = (X.astype(np.float64) + 1e-3 * g).astype(np.float32)
    return X, Q


def _norms64(A):
    return np.maximum(np.sqrt((A.astype(np.float64) ** 2).sum(axis=1)), C)


def matrix_reference(X, Q, metric):
    """(ref [B, N], bound [B, N]), both fp64."""
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    D = X.shape[1]
    if metric == "euclidean":
        ref = np.stack([np.sqrt(((X64 - q) ** 2).sum(axis=1)) for q in Q64])
        return ref, (gamma(D) / 2 + 3 * U) * ref
    dot = Q64 @ X64.T
    A = np.abs(Q64) @ np.abs(X64).T
    if metric == "dot_product":
        return dot, gamma(D) * A
    nn = _norms64(Q)[:, None] * _norms64(X)[None, :]
    ref = dot / nn
    return ref, gamma(D) * A / nn + (gamma(D) + 10 * U) * np.abs(ref)


def _sumsq32(A):
    return (A * A).sum(axis=1, dtype=np.float32)


def fp32_matrix(X, Q, metric, wrong=None):
    """A straightforward fp32 numpy restatement of vdb_similarity_matrix ([B, N] fp32), or one of
    the wrong variants the cases must catch:
      'expansion'   euclidean as sqrt(|x|^2 + |q|^2 - 2 q.x)
      'drop_slab'   the last partial 32-dim slab left out
      'neighbour'   cosine with row r's norm taken from row r + 1
      'no_clamp'    cosine without max(., 1e-8)"""
    X = np.asarray(X, np.float32)
    Q = np.asarray(Q, np.float32)
    if wrong == "drop_slab":
        keep = X.shape[1] // 32 * 32
        X, Q = X[:, :keep], Q[:, :keep]
    c = np.float32(1e-8)
    out = np.zeros((Q.shape[0], X.shape[0]), np.float32)
    xs = _sumsq32(X)
    for b, q in enumerate(Q):
        if metric == "euclidean":
            if wrong == "expansion":
                d2 = xs + _sumsq32(q[None])[0] - np.float32(2) * (X * q).sum(axis=1, dtype=np.float32)
                out[b] = np.sqrt(np.maximum(d2, np.float32(0)))
            else:
                df = X - q
                out[b] = np.sqrt((df * df).sum(axis=1, dtype=np.float32))
            continue
        dot = (X * q).sum(axis=1, dtype=np.float32)
        if metric == "dot_product":
            out[b] = dot
            continue
        xn, qn = np.sqrt(xs), np.sqrt(_sumsq32(q[None])[0])
        if wrong == "neighbour":
            xn = np.roll(xn, -1)
        if wrong != "no_clamp":
            xn, qn = np.maximum(xn, c), np.maximum(qn, c)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[b] = dot * (np.float32(1) / xn) * (np.float32(1) / qn)
    return out


# =============================================================================
# B. normalise
# =============================================================================
# (n, D): four rows per workgroup, 64 dims per wave step
NORMALIZE_SHAPES = [(1, 1), (3, 63), (4, 64), (5, 65), (1001, 384), (5, 1), (1001, 63), (4, 384)]


def normalize_data(n, D):
    """(x [n, D], roles): a zero row last and a row of norm 1e-10 (clamped) at index 1 where
    n >= 3; every other row's norm is far above c."""
    rng = np.random.default_rng(500000 + 1000 * n + D)
    x = scaled_normal(rng, n, D)
    roles = {}
    if n >= 3:
        roles["zero_row"] = n - 1
        x[n - 1] = 0
        roles["tiny_row"] = 1
        x[1] = tiny_row(rng, D)
    return x, roles


def normalize_reference(x):
    """(ref [n, D], bound [n, D]) fp64."""
    ref = x.astype(np.float64) / _norms64(x)[:, None]
    return ref, (gamma(x.shape[1]) / 2 + 3 * U) * np.abs(ref)


def fp32_normalize(x, wrong=None):
    x = np.asarray(x, np.float32)
    if wrong == "drop_slab":
        nr = np.sqrt(_sumsq32(x[:, :x.shape[1] // 32 * 32]))
    else:
        nr = np.sqrt(_sumsq32(x))
    if wrong == "neighbour":
        nr = np.roll(nr, -1)
    if wrong != "no_clamp":
        nr = np.maximum(nr, np.float32(1e-8))
    with np.errstate(divide="ignore", invalid="ignore"):
        return x / nr[:, None]


# =============================================================================
# C. top-k
# =============================================================================
TOPK_K = (1, 31, 32, 33, 1000, 1024)
WAVE_EDGE, PASS_EDGE, CHUNK_EDGE = (63, 64), (255, 256), (TOPK_CHUNK - 1, TOPK_CHUNK)
LEVELS = np.array([-1.5, -0.25, 0.5, 2.0], np.float32)
SPECIAL_BEST = 5  # winning infinities in a 'specials' row


def topk_ks(n):
    """Every k of TOPK_K that fits, and k == n where the operator allows it."""
    ks = [k for k in TOPK_K if k <= n]
    if n <= 1024 and n not in ks:
        ks.append(n)
    return ks


def topk_oracle(s, k, largest, ties="lower"):
    """[rows, k] int64.  key = s (largest) or -s, NaN -> -inf; order: key descending, index
    ascending, so a NaN ties with the worst infinity and is ordered against it by index.
    ties='higher' is the wrong rule the cases must tell apart."""
    s = np.asarray(s, np.float32)
    out = np.empty((s.shape[0], k), np.int64)
    n = s.shape[1]
    for b in range(s.shape[0]):
        key = s[b] if largest else -s[b]
        key = np.where(np.isnan(key), np.float32(-np.inf), key)
        if ties == "lower":
            out[b] = np.argsort(-key, kind="stable")[:k]
        else:
            out[b] = n - 1 - np.argsort(-key[::-1], kind="stable")[:k]
    return out


def _tcase(family, rows, n, ks=None, **extra):
    return dict(family=family, rows=rows, n=n, ks=tuple(ks if ks is not None else topk_ks(n)), **extra)


_SIZES = (1, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 2 * TOPK_CHUNK + 1, 40 * TOPK_CHUNK + 5)
_ROWS_A = (7, 3, 1, 7, 3, 1, 7, 3, 7, 1, 7, 3)
_ROWS_B = (3, 7, 7, 1, 7, 3, 1, 7, 1, 3, 3, 1)
PLANT_N = 2 * TOPK_CHUNK + 1
PLANTS = WAVE_EDGE + PASS_EDGE + CHUNK_EDGE + (PLANT_N - 1,)  # the last: alone in the partial chunk

TOPK_CASES = (
    [_tcase("distinct", r, n) for n, r in zip(_SIZES, _ROWS_A)]
    + [_tcase("levels", r, n) for n, r in zip(_SIZES, _ROWS_B)]
    + [_tcase("constant", 3, n) for n in (65, TOPK_CHUNK + 1, 2 * TOPK_CHUNK + 1)]
    + [_tcase("planted", 3, PLANT_N, (1, 6, 7, 31, 32, 33, 1000, 1024))]
    + [_tcase("specials", 3, 300, (21, 25, 26, 31, 32, 33, 300), finite=20),
       _tcase("specials", 7, 2 * TOPK_CHUNK + 1, (501, 505, 506, 1000, 1024), finite=500),
       _tcase("zeros", 3, TOPK_CHUNK + 1),
       _tcase("zeros", 1, 1500)]
    + [_tcase("all_nan", r, n, (n,)) for r, n in ((1, 1), (3, 65), (7, 257), (1, 1024))]
    + [_tcase("all_nan", 3, 2 * TOPK_CHUNK + 1, (1, 1024))]
)


def topk_id(c):
    return f"{c['family']}-n{c['n']}-r{c['rows']}"


def topk_scores(c, largest):
    """The score rows [rows, n] fp32 of a case; each row holds different data."""
    rows, n, fam = c["rows"], c["n"], c["family"]
    rng = np.random.default_rng(7 * n + rows + 13 * len(fam))
    sgn = np.float32(1.0 if largest else -1.0)
    if fam == "distinct":  # a permutation of n distinct quarter-integers per row
        return np.stack([(rng.permutation(n) - n // 2).astype(np.float32) * np.float32(0.25) + np.float32(0.125 * b)
                         for b in range(rows)])
    if fam == "levels":  # four values: the order is decided almost wholly by the index
        return LEVELS[rng.integers(0, 4, (rows, n))]
    if fam == "constant":
        return np.repeat((np.arange(rows, dtype=np.float32) - 1)[:, None] * np.float32(2.5), n, axis=1)
    if fam == "planted":  # equal best values astride a wave, a workgroup pass, a chunk; one in the tail
        s = np.stack([(rng.permutation(n) / np.float32(n)).astype(np.float32) for _ in range(rows)]) - np.float32(0.5)
        s[:, list(PLANTS)] = sgn * np.float32(5.0)
        return s
    if fam == "specials":
        # SPECIAL_BEST winning infinities and c['finite'] finite values; everything else is the
        # losing infinity or NaN, laid out by index: they tie, and any k above finite + 5 cuts
        # into that tie
        kinds = np.array([-sgn * np.inf, np.nan, np.nan, -sgn * np.inf, np.nan, -sgn * np.inf, -sgn * np.inf],
                         np.float32)
        s = np.stack([kinds[(np.arange(n) + b) % 7] for b in range(rows)])
        for b in range(rows):
            at = rng.choice(n, c["finite"] + SPECIAL_BEST, replace=False)
            s[b, at[SPECIAL_BEST:]] = np.round(rng.standard_normal(c["finite"]) * 4).astype(np.float32) / np.float32(4)
            s[b, at[:SPECIAL_BEST]] = sgn * np.float32(np.inf)
        return s
    if fam == "zeros":  # -0.0 and +0.0 compare equal: the lower index wins; a few non-zeros
        s = np.where(rng.random((rows, n)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        for b in range(rows):
            at = rng.choice(n, min(10, n // 8), replace=False)
            s[b, at] = np.where(np.arange(at.size) % 2 == 0, np.float32(1 + b), np.float32(-1 - b))
        return s
    if fam == "all_nan":
        return np.full((rows, n), np.nan, np.float32)
    raise ValueError(fam)

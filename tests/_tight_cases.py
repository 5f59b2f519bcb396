"""Adversarial rows at the certificate's bound, arriving by every ingest route.

The finish (vdb_exact.hip) trusts |approx - (exact - shift)| <= eps for every row; eps is built
from maxima that ingest keeps (the largest row residual R, its directional form M, the plane norms
ZA / XL, xmax, the bf16 residuals).  A maximum that is too SMALL changes no result on ordinary
data, where the realised error is a fraction of eps.  Here the realised error of a few planted
rows is most of eps, by construction, and those rows alone raise the maximum that covers them:

  query   q = c s, s in {+-1}^D: every |q_i| equal, so Cauchy-Schwarz on a residual parallel to s
          is tight; the int8 queries lie on the batch's 8-bit query grid (qh = +-127, ql = 0), so
          the query's own rounding term is ~0.  The batch holds B = 4 such queries and nothing
          else (s_q is per batch): two Hadamard rows and their negatives, mutually orthogonal or
          opposite, so one query's planted rows are nothing to another and q.dir stays small.
  star    per query one row parallel to s, the exact top-1, whose every coordinate lies DELTA of
          a grid step short of the next grid point AWAY from the query: it is under-scored by
          ~DELTA step |q|_1.
  decoys  k rows just below the star (one coordinate lowered by a few steps) whose coordinates
          lie DELTA of a step past the midpoint TOWARDS the query: over-scored by the same
          amount.  The star's approximate rank is k + 1; its exact rank 1.
  FLIP    coordinates of every planted row round the other way, which leaves |r| as it is and
          takes |r.q| down to (D - 2 FLIP) / D of |r||q|: the realised error is ~0.92 eps, not
          0.99, which leaves room for the fp32 terms the models leave out.
  cosine  one more coordinate per planted row restores the unit norm (to < 2e-8, so that the
          fp32 normalisation multiplies by exactly 1).

The "grid" is the pass's: s_x after centring (i8, i8q), s_x / 256 (i8x3: the second plane; the
first plane is exact), the bf16 grid of the scored row (bf16).  mu and s_x depend on the rows the
setup is derived from, which the route decides and which may include the planted rows: a few
fixed-point iterations settle them.

Routes (vdb_api.cpp vdb_index_add: the setup -- mu, s_x, dir -- is derived from the first add's
rows, up to kDirRows = 65536, and again from ALL rows when an add makes count + n >= 2 dir_rows
while dir_rows < kDirRows; vdb_index_update and vdb_index_remove never derive it again):

  R1   one add.                                              setup: all N rows
  R2   5956 bulk rows, then the 44 planted rows.             setup: the 5956 (6000 < 2 x 5956)
  R3   2900 rows, then 3100 with the planted ones.           setup: all N (6000 >= 2 x 2900)
  R4   N = 66100: 65536 bulk rows, then 564 with the planted ones.  setup: the 65536, frozen
  R5   bulk rows at the planted positions; update writes the planted rows.  setup: the rows
       before the update
  R6   R1, then an add with one NaN (rejected: the rollback must keep the maxima)
  R7   R2 with a rejected add between the two adds
  R8   R1 with 500 more bulk rows interleaved, which remove takes out again: the planted rows
       move and their copies are rebuilt.                    setup: the 6500 rows
  R9   created as fp32, all rows added, then set_precision: the copy is built late
  R10  3000 rows of 10 x the scale, clear, then R1.          setup: all N rows of the second life

R1, R3, R6, R9 and R10 end with the same rows and the same setup: one data set ("A", planted rows
at scattered positions past row 2900).  R2 and R7 share "B".
"""
import functools

import numpy as np

from oracle import ref_cpu

import _planted as pl

N, D, K, B = 6000, 64, 10, 4
DELTA = 0.48   # of a grid step; 0.02 from the rounding boundary, >> the fp32 roundings of t (~3e-3 at worst, i8x3)
FLIP = 2       # coordinates per planted row that round the other way: |r.q| = (D - 2 FLIP) / D |r||q|
N_PLANT = B * (K + 1)
N_R4, HEAD_R4 = 66100, 65536
N_EXTRA = 500  # R8
BOTH = ("cosine", "euclidean")
PRECISIONS = ("i8", "i8x3", "i8q", "bf16")
ROUTES = ("R1", "R2", "R3", "R4", "R5", "R6", "R7", "R8", "R9", "R10")
DATASET = {"R1": "A", "R3": "A", "R6": "A", "R9": "A", "R10": "A", "R2": "B", "R7": "B", "R4": "R4", "R5": "R5",
           "R8": "R8"}
# (precision, metric) pairs whose (c) -- a smaller bound changes the outcome -- cannot be reached
# on standard-normal bulk rows (tests/test_tight_precondition.py prints the figures)
LEFT_OUT = (("bf16", "cosine"),)


def _hadamard_row(i):
    j = np.arange(D)
    return np.where(np.array([bin(i & int(x)).count("1") for x in j]) % 2 == 0, 1.0, -1.0)


SIGNS = np.stack([_hadamard_row(21), -_hadamard_row(21), _hadamard_row(42), -_hadamard_row(42)])


def _bulk(n, seed):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)


def _setup_of(S, metric):
    """(mu fp32, s_x fp32) of setup rows S, as _planted.i8_model derives them."""
    f32 = np.float32
    Y, _ = pl._scored_rows(S, metric)
    sums = Y.astype(np.float64).sum(0)
    mu = (sums / len(S)).astype(f32)
    zmax = np.abs((Y - mu).astype(f32)).max()
    return mu, f32(1.25 * zmax / 127)


def _unit_free(y, jf, sign):
    """y (fp32) with coordinate jf set so that |y| = 1 as nearly as fp32 allows."""
    rest = (np.delete(y, jf).astype(np.float64) ** 2).sum()
    assert rest < 1.0, rest
    best = None
    f0 = np.float32(sign * np.sqrt(1.0 - rest))
    for f in (f0, np.nextafter(f0, np.float32(0)), np.nextafter(f0, np.float32(2 * sign))):
        err = abs(np.sqrt(rest + float(f) ** 2) - 1.0)
        if best is None or err < best[0]:
            best = (err, f)
    y = y.copy()
    y[jf] = best[1]
    return y


def _planted_rows(prec, metric, mu, step, n0, coords):
    """The B x (K + 1) planted rows (star first) in the scored space: mu + step * t, t per the
    module docstring.  coords[b, j] = a permutation of the D coordinates: [0] the free one
    (cosine), [1] the lowered one (decoys), [2 : 2 + FLIP] the flipped ones."""
    sub = 256.0 if prec == "i8x3" else 1.0  # grid steps per first-plane step
    n2 = 40.0 if prec == "i8x3" else 0.0
    out = np.empty((B, K + 1, D), np.float32)
    for b in range(B):
        s = SIGNS[b]
        for j in range(K + 1):
            star = j == 0
            frac = np.full(D, DELTA if star else 1.0 - DELTA)
            frac[coords[b, j, 2:2 + FLIP]] = 1.0 - DELTA if star else DELTA
            t = n0 + (n2 + frac) / sub
            if not star:
                # decoy j: 3 ... K + 2 steps lower (the other coordinates lie (D - 1 - 3 FLIP) x
                # (1 - 2 DELTA) = 2.3 steps nearer the query than the star's), distinct keys
                t[coords[b, j, 1]] -= (2 + j) / sub
            y = (mu.astype(np.float64) + float(step) * s * t).astype(np.float32)
            if metric == "cosine":
                jf = coords[b, j, 0]
                y = _unit_free(y, jf, s[jf])
            out[b, j] = y
    return out


def _grid(prec, metric, S):
    """(mu, step, n0) of the pass's grid for planted rows, from the setup rows S."""
    if prec == "bf16":  # the bf16 grid of the row itself: a binade with 2^-7 relative steps
        if metric == "cosine":
            return np.zeros(D, np.float32), 2.0 ** -11, 240.0   # |y_i| ~ 0.117 in [2^-4, 2^-3)
        return np.zeros(D, np.float32), 2.0 ** -6, 200.0        # |x_i| ~ 3.1 in [2, 4)
    mu, sx = _setup_of(S, metric)
    # L2: 60 steps of the ~102 that reach the largest bulk |z| (the planted rows never set s_x);
    # cosine: 63 coordinates of ~0.117 leave the free one ~0.37 of the unit norm
    n0 = 60.0 if metric == "euclidean" else float(np.floor(0.117 / float(sx)))
    return mu, sx, n0


def _queries(prec, metric, step):
    if metric == "cosine":
        return SIGNS.astype(np.float32)
    c = np.float32(6.5) if prec == "bf16" else np.float32(127.0) * np.float32(step)
    return (SIGNS * float(c)).astype(np.float32)


# the adds of each route's (last) life, in rows
ROUTE_ADDS = {"R1": (N,), "R2": (N - N_PLANT, N_PLANT), "R3": (2900, N - 2900), "R4": (HEAD_R4, N_R4 - HEAD_R4),
              "R5": (N,), "R6": (N,), "R7": (N - N_PLANT, N_PLANT), "R8": (N + N_EXTRA,), "R9": (N,), "R10": (N,)}
# ... and the rows of the data set the setup must then come from
SETUP_ROWS = {"A": N, "B": N - N_PLANT, "R4": HEAD_R4, "R5": N, "R8": N + N_EXTRA}


def setup_rule(adds, k_dir_rows=65536):
    """How many leading rows the setup is derived from after `adds` (vdb_api.cpp vdb_index_add:
    the first add's rows, at most kDirRows; then, while dir_rows < kDirRows, all rows again
    whenever count + n >= 2 dir_rows)."""
    count = dir_rows = 0
    for n in adds:
        if count == 0:
            dir_rows = min(n, k_dir_rows)
        if dir_rows < k_dir_rows and count + n >= 2 * dir_rows:
            dir_rows = min(count + n, k_dir_rows)
        count += n
    return dir_rows


def dataset(name, prec, metric):
    """One data set (shared, read-only): dict(W = the rows the model sees, keep = the rows of W
    that are the final rows, V = W[keep], Q, planted [B, K + 1] (rows of V, star first), setup =
    the rows the setup is derived from, pre = R5's rows before the update, extra = R8's rows of W
    to remove).  i8q takes i8's: on the 8-bit query grid the two passes score alike."""
    return _dataset(name, "i8" if prec == "i8q" else prec, metric)


@functools.lru_cache(maxsize=6)
def oracle(name, prec, metric):
    """ref_cpu.exact_search over the final rows, once per data set."""
    d = dataset(name, prec, metric)
    out = ref_cpu.exact_search(d["Q"], d["V"], K, metric)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=6)
def _dataset(name, prec, metric):
    seed = {"A": 11, "B": 12, "R4": 13, "R5": 14, "R8": 15}[name]
    rng = np.random.default_rng(1000 + seed)
    n = {"R4": N_R4, "R8": N + N_EXTRA}.get(name, N)
    W = _bulk(n, seed)
    lo = {"A": 2900, "B": N - N_PLANT, "R4": HEAD_R4}.get(name, 0)
    pos = (lo + rng.permutation(n - lo)[:N_PLANT]).reshape(B, K + 1)
    extra = None
    if name == "R8":
        extra = np.sort(np.setdiff1d(np.arange(n), pos.ravel())[rng.permutation(n - N_PLANT)[:N_EXTRA]])
    # one free coordinate per query (the same for its K + 1 rows: another one would move the
    # free value, and with it the key, by ~2 y_i mu_i, which is many i8x3 steps), the others shuffled per row
    coords = np.empty((B, K + 1, D), np.int64)
    for b in range(B):
        jf = int(rng.integers(D))
        for j in range(K + 1):
            coords[b, j] = np.concatenate([[jf], rng.permutation(np.delete(np.arange(D), jf))])
    pre = W.copy()
    setup_rows = {"A": slice(0, n), "B": slice(0, N - N_PLANT), "R4": slice(0, HEAD_R4), "R5": None,
                  "R8": slice(0, n)}[name]
    for _ in range(8):  # the planted rows depend on (mu, s_x), which may depend on them
        S = pre if setup_rows is None else W[setup_rows]
        mu, step, n0 = _grid(prec, metric, S)
        rows = _planted_rows(prec, metric, mu, step, n0, coords)
        if np.array_equal(W[pos], rows):
            break
        W[pos] = rows
    else:
        raise AssertionError("the setup did not settle")
    keep = np.ones(n, bool)
    if extra is not None:
        keep[extra] = False
    planted = np.cumsum(keep)[pos] - 1  # rows of V
    out = dict(W=W, keep=keep, V=W if extra is None else np.ascontiguousarray(W[keep]), Q=_queries(prec, metric, step),
               planted=planted, setup=S, pre=pre if name == "R5" else None, extra=extra)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def bf16_model(V, Q, metric, setup=None, maxima=None):
    """(approx [N, B], eps [B], shift [B]) of the bf16 pass: the scored row rounded to bf16, the
    query in fp32, the sum in fp64 (the pass's own summation error is inside eps_rel); eps as
    _planted.eps_upper writes it, with the finish's directional form of the corpus term beside the
    Cauchy-Schwarz one (vdb_exact.hip: the smaller of the two) and the maxima over `maxima`."""
    f32 = np.float32
    Y, nr = pl._scored_rows(V, metric)
    S = Y[:min(len(V), 65536)] if setup is None else pl._scored_rows(np.asarray(setup, dtype=f32), metric)[0]
    sel = slice(None) if maxima is None else maxima
    sums = S.astype(np.float64).sum(0)
    dirv = (sums / np.sqrt((sums ** 2).sum())).astype(f32).astype(np.float64)
    Yb = pl._bf16_rne(Y).astype(np.float64)
    res = Y.astype(np.float64) - Yb
    rn = np.sqrt((res ** 2).sum(1))
    qn = np.sqrt((Q.astype(np.float64) ** 2).sum(1))
    q = (Q * (1.0 / np.maximum(qn, 1e-8)).astype(f32)[:, None]).astype(f32) if metric == "cosine" else Q.astype(f32)
    qd = q.astype(np.float64)
    dots = Yb @ qd.T
    xmax = nr[sel].max()
    if metric == "cosine":
        approx = dots
        R = (rn / np.maximum(np.sqrt((Y.astype(np.float64) ** 2).sum(1)), 1e-8))[sel].max()
        shift = np.zeros(len(Q))
    else:
        rinit = (f32(-0.5) * (nr ** 2).astype(f32)).astype(np.float64)
        approx = 2.0 * (dots + rinit[:, None])
        R = rn[sel].max()
        shift = -qn ** 2
    M = np.abs(res @ dirv)[sel].max()
    c = qd @ dirv
    w = np.sqrt(((qd - c[:, None] * dirv) ** 2).sum(1))
    xres, dres = 1.01 * R, 1.01 * M
    bq = np.minimum(xres * (1.0 if metric == "cosine" else qn), (w * xres + np.abs(c) * dres) * (1 + 1e-6) + 1e-6 * xres)
    eps_rel = 1.01 * (2.0 * D * 2.0 ** -23 + 1.1 * 2.0 ** -16 + 8 * 2.0 ** -24)
    if metric == "cosine":
        eps = eps_rel + bq
    else:  # (the finish adds 2.4e-7 max(|a_k|, |acut|): finish_rule does)
        eps = eps_rel * (2.0 * qn * xmax + xmax * xmax) + 2.0 * bq
    return approx, eps, shift


def model(prec, metric, V, Q, setup, maxima=None):
    if prec == "bf16":
        return bf16_model(V, Q, metric, setup=setup, maxima=maxima)
    return pl.i8_model(V, Q, metric, prec, setup=setup, maxima=maxima)


def exact_all(V, Q, metric):
    """The oracle's fp64 keys of every row, [N, B]."""
    xn = ref_cpu.canonical_norm64(V) if metric == "cosine" else None
    return np.stack([ref_cpu.exact_keys(Q[b], V, metric, xn) for b in range(Q.shape[0])], axis=1)


def finish_rule(approx, exact, shift, eps, k, metric="cosine", kp=256, rank_cut=None):
    """The finish's decisions (DESIGN.md §3.2 steps 3-4, §3.8's exact-key certificate and guard 2
    of §3.9; vdb_exact.hip finish_kernel), restated on the CPU.  Per query:
    (certified [B] bool, rerank: list of row arrays, violations: list of row arrays).

    The candidates are the kp best rows by (approx desc, row asc).  acut = max(a_KP, T) is not
    known without the pilot's sample; it is at most the rank_cut-th best approximate score for
    every KP >= rank_cut and every pilot rank >= rank_cut (T is the r-th best of the pilot's slot
    maxima, each a different row's score).  rank_cut defaults to k + 2, which every plan here
    exceeds (KP >= 128; pilot rank >= 2 KP S / N clamped to KP, or no bound at all), so
    `certified` here implies certified on the device, under the same eps or a larger one.
    L2: eps gains the finish's rounding term 2.4e-7 max(|a_k|, |acut|)."""
    rank_cut = k + 2 if rank_cut is None else rank_cut
    nq = approx.shape[1]
    certified = np.zeros(nq, bool)
    rerank, violations = [], []
    for b in range(nq):
        a = approx[:, b]
        order = np.lexsort((np.arange(a.size), -a))
        cand = order[:kp]
        ak, acut = a[order[k - 1]], a[order[rank_cut - 1]]
        e = float(eps[b])
        ec = e + (2.4e-7 * max(abs(ak), abs(acut)) if metric == "euclidean" else 0.0)
        ok = acut + ec < ak - ec
        rr = cand[a[cand] >= ak - 2.001 * ec]
        ex = exact[rr, b] - shift[b]
        if not ok:  # the exact-key certificate: the exact k-th best of the reranked rows beats acut + eps
            ekk = np.sort(exact[rr, b])[::-1][k - 1] if rr.size >= k else -np.inf
            tol = 4e-16 * (abs(ekk) + abs(shift[b]))
            ok = ekk - shift[b] - tol > acut + ec
        fr = 4e-16 * (np.abs(exact[rr, b]) + abs(shift[b]))
        l2 = 2.4e-7 * np.maximum(np.abs(a[rr]), np.abs(ex)) if metric == "euclidean" else 0.0
        bad = ~(np.abs(a[rr] - ex) <= 1.01 * (e + l2) + fr)
        certified[b] = ok
        rerank.append(rr)
        violations.append(rr[bad])
    return certified, rerank, violations


def cases():
    """(route, precision, metric) of every case the GPU test runs."""
    return [(r, p, m) for r in ROUTES for p in PRECISIONS for m in BOTH if (p, m) not in LEFT_OUT]


def case_id(c):
    return "-".join(c)


def rejected_rows(seed=99):
    """An add that must be rejected: 64 rows of 5 x the bulk's scale with one NaN."""
    X = 5.0 * _bulk(64, seed)
    X[37, 5] = np.nan
    return X


def ingest(ix, route, d, precision):
    """Bring index `ix` (created with `precision`; R9: with fp32) to the rows d["V"] by `route`."""
    V = d["V"]

    def rejected():
        count = ix.count()
        try:
            ix.add(rejected_rows())
        except ValueError as e:  # VDB_ERR_NONFINITE
            assert "NaN" in str(e), e
        else:
            raise AssertionError("the add with a NaN was accepted")
        assert ix.count() == count

    if route in ("R1", "R6", "R9"):
        ix.add(V)
        if route == "R6":
            rejected()
        if route == "R9":
            ix.set_precision(precision)
    elif route in ("R2", "R7"):
        ix.add(V[:N - N_PLANT])
        if route == "R7":
            rejected()
        ix.add(V[N - N_PLANT:])
    elif route == "R3":
        ix.add(V[:2900])
        ix.add(V[2900:])
    elif route == "R4":
        ix.add(V[:HEAD_R4])
        ix.add(V[HEAD_R4:])
    elif route == "R5":
        ix.add(d["pre"])
        rows = d["planted"].ravel()
        assert ix.update(rows, V[rows]) == rows.size
    elif route == "R8":
        ix.add(d["W"])
        assert ix.remove(d["extra"]) == N_EXTRA
    elif route == "R10":
        ix.add(10.0 * _bulk(3000, 77))
        ix.clear()
        ix.add(V)
    else:
        raise ValueError(route)
    assert ix.count() == V.shape[0]

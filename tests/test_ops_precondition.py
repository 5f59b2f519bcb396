"""CPU preconditions of tests/test_gpu_ops_alone.py: a green GPU run means what it claims only if
the cases of tests/_ops_cases.py can tell a right operator from a wrong one.  No GPU here.

* a straightforward fp32 numpy restatement of each operator meets every derived bound on every
  case, so the bounds are attainable (a slip in a derivation shows here, not on the GPU);
* the wrong variants miss the bound on the cases meant for them: euclidean by the fp32 expansion
  on the near rows (by more than 100x), the last partial 32-dim slab dropped at D = 33 and 100,
  norms taken from the neighbouring row, the clamp left out on the tiny-norm row;
* the top-k families are what they say: distinct values are distinct, planted ties tie, the
  specials leave fewer than k finite values, and wherever a case has ties at all the answer under
  "ties to the higher index" differs from the oracle's.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _ops_cases as oc  # noqa: E402


def _ratio(out, ref, bound):
    assert np.isfinite(out).all()
    return oc.ratio(np.abs(out.astype(np.float64) - ref), bound)


def test_tables_cover_the_tile_edges():
    N, D, B = (set(s[i] for s in oc.MATRIX_SHAPES) for i in range(3))
    assert {1, 127, 128, 129, 300} <= N and {1, 2, 31, 32, 33, 64, 100} <= D and {1, 31, 32, 33, 70} <= B
    assert (4097, 768, 5) in oc.MATRIX_SHAPES
    assert {1, 3, 4, 5, 1001} <= set(s[0] for s in oc.NORMALIZE_SHAPES)
    assert {1, 63, 64, 65, 384} <= set(s[1] for s in oc.NORMALIZE_SHAPES)
    ns = set(c["n"] for c in oc.TOPK_CASES)
    assert {1, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 2 * 16384 + 1, 40 * 16384 + 5} <= ns
    assert {1, 3, 7} == set(c["rows"] for c in oc.TOPK_CASES)
    assert all(c["rows"] in (1, 3) for c in oc.TOPK_CASES if c["n"] > 4 * oc.TOPK_CHUNK)
    ks = set(k for c in oc.TOPK_CASES for k in c["ks"])
    assert {1, 31, 32, 33, 1000, 1024} <= ks
    assert all(1 <= k <= min(c["n"], 1024) for c in oc.TOPK_CASES for k in c["ks"])
    assert any(c["n"] in c["ks"] for c in oc.TOPK_CASES)


def _magnitudes_ok(a, but_rows=()):
    a = np.delete(a, list(but_rows), axis=0)
    nz = np.abs(a[a != 0])
    return nz.size == 0 or (nz.min() >= 2.0 ** -20 and nz.max() <= 2.0 ** 20)


@pytest.mark.parametrize("N,D,B", oc.MATRIX_SHAPES)
def test_matrix_data_holds_its_planted_rows(N, D, B):
    X, Q, roles = oc.matrix_data(N, D, B)
    assert X.shape == (N, D) and Q.shape == (B, D) and X.dtype == Q.dtype == np.float32
    tiny = [roles["tiny_row"]] if "tiny_row" in roles else []
    assert _magnitudes_ok(X, tiny) and _magnitudes_ok(Q)
    if N >= 4:
        assert {"zero_row", "tiny_row", "equal_row"} <= set(roles)
    if B >= 2:
        assert not Q[roles["zero_query"]].any()
    if "zero_row" in roles:
        assert not X[roles["zero_row"]].any()
    if "tiny_row" in roles:
        nr = np.linalg.norm(X[roles["tiny_row"]].astype(np.float64))
        assert 0.9 * oc.TINY_NORM < nr < 1.1 * oc.TINY_NORM and nr < oc.C / 4
    if "equal_row" in roles:
        assert X[roles["equal_row"]].tobytes() == Q[roles["equal_query"]].tobytes()
    # every other norm is at least 4x above the clamp: kernel and reference take the same branch
    nx = np.linalg.norm(X.astype(np.float64), axis=1)
    assert ((nx == 0) | (nx < oc.C / 4) | (nx > 4 * oc.C)).all()
    # scaled rows: neighbouring norms differ by factors, so a misplaced norm cannot hide
    if N >= 127 and D >= 31:
        r = np.arange(11, 40, 5)  # scale 2, followed by scale 4; none of them a planted row
        assert (nx[r + 1] / nx[r] > 1.2).all()


@pytest.mark.parametrize("metric", oc.METRICS)
@pytest.mark.parametrize("N,D,B", oc.MATRIX_SHAPES)
def test_fp32_restatement_meets_the_matrix_bounds(N, D, B, metric):
    X, Q, roles = oc.matrix_data(N, D, B)
    ref, bound = oc.matrix_reference(X, Q, metric)
    out = oc.fp32_matrix(X, Q, metric)
    assert _ratio(out, ref, bound) <= 1.0
    if metric == "cosine" and D <= 768:
        assert np.abs(out - ref).max() <= oc.COSINE_HEADER_ATOL
    if metric == "euclidean" and "equal_row" in roles:
        assert out[roles["equal_query"], roles["equal_row"]] == 0.0
        assert ref[roles["equal_query"], roles["equal_row"]] == 0.0
    if "zero_query" in roles and metric != "euclidean":
        assert not ref[roles["zero_query"]].any() and not bound[roles["zero_query"]].any()


def test_near_rows_tell_direct_differences_from_the_expansion():
    X, Q = oc.near_rows()
    ref, bound = oc.matrix_reference(X, Q, "euclidean")
    d = np.arange(oc.NEAR_N)
    assert (ref[d, d] < 1e-2 * np.linalg.norm(X.astype(np.float64), axis=1)).all()  # near indeed
    assert _ratio(oc.fp32_matrix(X, Q, "euclidean"), ref, bound) <= 1.0
    wrong = oc.fp32_matrix(X, Q, "euclidean", wrong="expansion")
    assert oc.ratio(np.abs(wrong - ref)[d, d], bound[d, d]) > 100.0


@pytest.mark.parametrize("metric", oc.METRICS)
@pytest.mark.parametrize("shape", [s for s in oc.MATRIX_SHAPES if s[1] in (33, 100)])
def test_a_dropped_partial_slab_misses_the_bound(shape, metric):
    assert {s[1] for s in oc.MATRIX_SHAPES if s[1] in (33, 100)} == {33, 100}
    X, Q, _ = oc.matrix_data(*shape)
    ref, bound = oc.matrix_reference(X, Q, metric)
    assert _ratio(oc.fp32_matrix(X, Q, metric, wrong="drop_slab"), ref, bound) > 100.0


@pytest.mark.parametrize("N,D,B", [s for s in oc.MATRIX_SHAPES if s[0] >= 4])
def test_neighbouring_norms_and_a_missing_clamp_miss_the_bound(N, D, B):
    X, Q, roles = oc.matrix_data(N, D, B)
    ref, bound = oc.matrix_reference(X, Q, "cosine")
    err = np.abs(oc.fp32_matrix(X, Q, "cosine", wrong="neighbour").astype(np.float64) - ref)
    assert oc.ratio(err, bound) > 100.0
    t = roles["tiny_row"]
    out = oc.fp32_matrix(X, Q, "cosine", wrong="no_clamp")[:, t].astype(np.float64)
    live = [b for b in range(B) if b != roles.get("zero_query")]
    assert oc.ratio(np.abs(out - ref[:, t])[live], bound[live, t]) > 100.0


@pytest.mark.parametrize("n,D", oc.NORMALIZE_SHAPES)
def test_normalize_cases(n, D):
    x, roles = oc.normalize_data(n, D)
    tiny = [roles["tiny_row"]] if "tiny_row" in roles else []
    assert _magnitudes_ok(x, tiny)
    nx = np.linalg.norm(x.astype(np.float64), axis=1)
    assert ((nx == 0) | (nx < oc.C / 4) | (nx > 4 * oc.C)).all()
    ref, bound = oc.normalize_reference(x)
    out = oc.fp32_normalize(x)
    assert _ratio(out, ref, bound) <= 1.0
    if n >= 3:
        assert not x[roles["zero_row"]].any() and not out[roles["zero_row"]].any()
        assert 0.9 * oc.TINY_NORM < nx[tiny[0]] < 1.1 * oc.TINY_NORM
        t = tiny[0]
        assert oc.ratio(np.abs(oc.fp32_normalize(x, "no_clamp")[t] - ref[t]), bound[t]) > 100.0
        live = np.arange(n - 1)  # the zero row is 0 / anything
        assert oc.ratio(np.abs(oc.fp32_normalize(x, "neighbour")[live] - ref[live]), bound[live]) > 100.0
    if D >= 32 and D % 32:
        assert _ratio(oc.fp32_normalize(x, "drop_slab"), ref, bound) > 100.0


# ---- top-k ---------------------------------------------------------------------------------
TIED = ("levels", "constant", "planted", "specials", "zeros", "all_nan")


@pytest.mark.parametrize("largest", [True, False], ids=["largest", "smallest"])
@pytest.mark.parametrize("c", oc.TOPK_CASES, ids=[oc.topk_id(c) for c in oc.TOPK_CASES])
def test_topk_families_are_what_they_claim(c, largest):
    s = oc.topk_scores(c, largest)
    rows, n, fam = c["rows"], c["n"], c["family"]
    assert s.shape == (rows, n) and s.dtype == np.float32
    if rows > 1 and fam != "all_nan" and (n >= 63 or fam == "distinct"):
        assert all(s[b].tobytes() != s[0].tobytes() for b in range(1, rows))  # different data per row
    kmax = max(c["ks"])
    want = oc.topk_oracle(s, kmax, largest)
    assert all(sorted(set(w.tolist())) == sorted(w.tolist()) for w in want)  # k distinct indices
    if fam == "distinct":
        assert all(np.unique(s[b]).size == n for b in range(rows))
    if fam == "levels":
        assert set(np.unique(s).tolist()) <= set(oc.LEVELS.tolist())
    if fam == "constant":
        assert (want == np.arange(kmax)).all() and all(np.unique(s[b]).size == 1 for b in range(rows))
    if fam == "planted":
        p = sorted(oc.PLANTS)
        assert {63, 64, 255, 256, oc.TOPK_CHUNK - 1, oc.TOPK_CHUNK} < set(p) and p[-1] // oc.TOPK_CHUNK == n // oc.TOPK_CHUNK
        assert n % oc.TOPK_CHUNK and p[-1] >= n - n % oc.TOPK_CHUNK  # in the last, partial chunk
        for b in range(rows):
            assert np.unique(s[b, p]).size == 1  # they really tie
            rest = np.delete(s[b], p)
            assert (rest < s[b, p[0]]).all() if largest else (rest > s[b, p[0]]).all()
            assert want[b, :len(p)].tolist() == p
    if fam == "specials":
        for b in range(rows):
            assert np.isfinite(s[b]).sum() == c["finite"] < min(c["ks"])
            assert np.isnan(s[b]).any() and np.isposinf(s[b]).any() and np.isneginf(s[b]).any()
            best = np.isposinf(s[b]) if largest else np.isneginf(s[b])
            assert best.sum() == oc.SPECIAL_BEST
            # NaN and the losing infinity interleave by index in the tail of the answer
            tail = want[b, oc.SPECIAL_BEST + c["finite"]:]
            assert (np.diff(tail) > 0).all() and np.isnan(s[b, tail]).any() and np.isinf(s[b, tail]).any()
        assert max(c["ks"]) > c["finite"] + oc.SPECIAL_BEST
    if fam == "zeros":
        z = s == 0
        assert (np.signbit(s) & z).any() and (~np.signbit(s) & z).any() and z.sum() > kmax
    if fam == "all_nan":
        assert np.isnan(s).all() and (want == np.arange(kmax)).all()
    if fam in TIED and n >= 63:
        for k in c["ks"]:
            assert not np.array_equal(oc.topk_oracle(s, k, largest, ties="higher"), want[:, :k]), k

"""The CPU preconditions of tests/test_gpu_bound_tight.py (data: tests/_tight_cases.py; argument:
DESIGN.md §5.4), from the numpy models of the candidate passes and oracle/ref_cpu alone -- never
the library.  For every data set, precision and metric the GPU test runs:

  (a) every planted row's model error is at most 0.95 eps, and each star's at least 0.8 eps: the
      error reaches the bound, and the 5 % left covers the fp32 terms the models leave out
      (tests/test_int8_bounds.py puts them inside 1 %);
  (b) with the sound eps the finish's rule (tc.finish_rule) certifies every query, reranks every
      true top-k row and finds no guard-2 violation -- also with twice that eps (R5 and R8 leave
      maxima of rows that are gone: the device's eps may be larger);
  (c) with eps0 -- the same formula, the planted rows left out of the maxima: an upper bound of
      what a build that missed them would use -- at least one query loses a true top-k row from
      the rerank set while it still certifies, or has a guard-2 violation.

(c) is what gives the GPU test its teeth: it asserts exact results with no fallback, no
inconsistency and no re-pass, so either outcome fails it.  (a) and (b) show that a correct build
passes it.  The pairs of tc.LEFT_OUT are shown NOT to reach (c), with their figures.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # tests/_planted.py, under any pytest import mode
import _planted as pl  # noqa: E402
import _tight_cases as tc  # noqa: E402

DATASETS = ("A", "B", "R4", "R5", "R8")
PAIRS = [(p, m) for p in tc.PRECISIONS for m in tc.BOTH]


def _figures(name, prec, metric):
    """Everything (a)-(c) need, for one data set."""
    d = tc.dataset(name, prec, metric)
    V, Q, P = d["V"], d["Q"], d["planted"]
    approx, eps, shift = tc.model(prec, metric, V, Q, d["setup"])
    bulk = np.ones(len(V), bool)
    bulk[P.ravel()] = False
    if prec == "bf16":
        _, eps0, _ = tc.bf16_model(V, Q, metric, setup=d["setup"], maxima=bulk)
    else:
        _, eps0, _ = pl.i8_model(V, Q, metric, prec, want_approx=False, setup=d["setup"], maxima=bulk)
    exact = tc.exact_all(V, Q, metric)
    return d, approx, eps, eps0, shift, exact, bulk


def _outcome(approx, exact, shift, eps, metric, topk):
    """Per query: (certified, every true top-k row reranked, guard-2 violations)."""
    cert, rerank, viol = tc.finish_rule(approx, exact, shift, eps, tc.K, metric)
    kept = np.array([set(topk[b].tolist()) <= set(rerank[b].tolist()) for b in range(tc.B)])
    return cert, kept, np.array([v.size for v in viol])


@pytest.mark.parametrize("prec,metric", PAIRS, ids=[f"{p}-{m}" for p, m in PAIRS])
@pytest.mark.parametrize("name", DATASETS)  # (the slowest index: a data set is built once per precision and metric)
def test_error_reaches_the_bound_and_only_the_sound_bound_holds(name, prec, metric):
    d, approx, eps, eps0, shift, exact, bulk = _figures(name, prec, metric)
    P = d["planted"]
    es, ei, ek = tc.oracle(name, prec, metric)
    err = np.abs(approx - (exact - shift[None, :]))
    star = np.array([err[P[b, 0], b] / eps[b] for b in range(tc.B)])
    worst = np.array([err[P[b], b].max() / eps[b] for b in range(tc.B)])
    a_star = np.array([approx[P[b, 0], b] for b in range(tc.B)])
    a_k = np.array([np.sort(approx[:, b])[-tc.K] for b in range(tc.B)])
    rank = np.array([(approx[:, b] > a_star[b]).sum() + 1 for b in range(tc.B)])
    margin = np.array([exact[P[b], b].min() - exact[bulk, b].max() for b in range(tc.B)])
    sound = _outcome(approx, exact, shift, eps, metric, ei)
    twice = _outcome(approx, exact, shift, 2.0 * eps, metric, ei)
    small = _outcome(approx, exact, shift, eps0, metric, ei)
    toothed = (small[0] & ~small[1]) | (small[2] > 0)
    l2 = np.array([2.4e-7 * abs(a_k[b]) if metric == "euclidean" else 0.0 for b in range(tc.B)])
    print(f"{name} {prec} {metric}: eps {eps.min():.4g}  star err/eps {star.min():.3f}-{star.max():.3f}  "
          f"planted max {worst.max():.3f}  star's approx rank {rank.min()}-{rank.max()}  "
          f"a_k - a_star {(a_k - a_star).max():.4g}  sound cut {(2.001 * (eps + l2)).min():.4g}  "
          f"cut with eps0 {(2.001 * (eps0 + l2)).max():.4g}  eps0/eps {(eps0 / eps).max():.3f}  "
          f"with eps0: star cut {int((small[0] & ~small[1]).sum())}/{tc.B}, guard-2 rows {int(small[2].sum())}")
    if (prec, metric) in tc.LEFT_OUT:
        # the planted rows do not set the maximum here: nothing a smaller bound would change
        assert not toothed.any() and star.max() < 0.8, (toothed, star)
        return
    # the construction: the star is the exact top-1 and the k + 1 planted rows lead, far above the bulk
    for b in range(tc.B):
        assert ei[b, 0] == P[b, 0]
        assert set(ei[b].tolist()) <= set(P[b].tolist())
    assert (rank == tc.K + 1).all(), rank
    # (4 eps of gap force certification; 8 with the doubled eps of (b))
    assert (margin > 10.0 * eps).all(), (margin, eps)
    # (a)
    assert worst.max() <= 0.95, worst
    assert star.min() >= 0.8, star
    # (b)
    for cert, kept, nviol in (sound, twice):
        assert cert.all() and kept.all() and not nviol.any(), (cert, kept, nviol)
    # (c)
    assert toothed.any(), small


def test_the_setup_rows_of_every_route():
    """Which rows mu, s_x and dir come from, per route, by the rule of vdb_index_add."""
    for route, adds in tc.ROUTE_ADDS.items():
        assert sum(adds) == {"R4": tc.N_R4, "R8": tc.N + tc.N_EXTRA}.get(route, tc.N)
        assert tc.setup_rule(adds) == tc.SETUP_ROWS[tc.DATASET[route]], route
    # the planted rows lie where the route's adds put them
    for name, lo in (("A", 2900), ("B", tc.N - tc.N_PLANT), ("R4", tc.HEAD_R4)):
        assert tc.dataset(name, "i8", "cosine")["planted"].min() >= lo
    d = tc.dataset("R8", "i8", "cosine")
    assert d["V"].shape[0] == tc.N and not np.isin(d["extra"], np.nonzero(~d["keep"])[0], invert=True).any()
    assert d["planted"].max() < tc.N


def test_i8_model_defaults_are_the_explicit_arguments():
    """setup / maxima left out = the first min(N, 65536) rows / every row, bit for bit."""
    rng = np.random.default_rng(8)
    V = rng.standard_normal((700, 48)).astype(np.float32)
    Q = rng.standard_normal((5, 48)).astype(np.float32)
    for metric in tc.BOTH:
        for prec in ("i8", "i8x3"):
            want = pl.i8_model(V, Q, metric, prec)
            got = pl.i8_model(V, Q, metric, prec, setup=V, maxima=np.arange(len(V)))
            for w, g in zip(want, got):
                np.testing.assert_array_equal(w, g)

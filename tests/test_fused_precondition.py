"""The cases of tests/_fused_cases.py have the properties their names claim, checked on the CPU with
the reference arithmetic alone (no GPU): identical lists are identical, disjoint lists are disjoint
and tie rank by rank, the overlap cases hold rows in several lists and a pair of candidates that a
float32 or re-ordered sum would rank the other way, weights change the answer, the short cases are
short, and MAX fusion over the lists is brute force over the whole corpus."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fused_cases as fc  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("metric", fc.METRICS)
@pytest.mark.parametrize("m", [2, 16])
def test_identical_lists_are_equal_and_the_union_is_one_list(m, metric):
    V, Qs = fc.identical_case(m)
    lists = fc.set_lists(Qs, V, 64, metric)
    for c, kappa in lists[1:]:
        np.testing.assert_array_equal(c, lists[0][0])
        np.testing.assert_array_equal(_bits(kappa), _bits(lists[0][1]))
    cands = fc.fuse(lists, "rrf")
    assert len(cands) == 64 and all(h == m for _, h in cands.values())
    rows, fused, hits = fc.rank(cands)
    np.testing.assert_array_equal(rows, lists[0][0])  # the fused order is the list's order
    rows, fused, hits = fc.rank(fc.fuse(lists, "max"))
    np.testing.assert_array_equal(rows, lists[0][0])
    np.testing.assert_array_equal(_bits(fused), _bits(lists[0][1]))


@pytest.mark.parametrize("metric", fc.METRICS)
@pytest.mark.parametrize("m", [2, 16])
def test_disjoint_lists_are_disjoint_and_every_rank_ties(m, metric):
    V, Qs = fc.disjoint_case(m)
    assert fc.CLUSTER_ROWS > fc.MAX_FETCH and V.shape[0] <= 4096
    F = fc.MAX_FETCH
    lists = fc.set_lists(Qs, V, F, metric)
    allrows = np.concatenate([c for c, _ in lists])
    assert allrows.size == m * F == np.unique(allrows).size  # pairwise disjoint: the union is m x fetch_k
    if m == 16:
        assert allrows.size == 3200  # the kernel's largest input
    rows, fused, hits = fc.rank(fc.fuse(lists, "rrf"))
    assert (hits == 1).all()
    vals, counts = np.unique(_bits(fused), return_counts=True)
    assert vals.size == F and (counts == m).all()  # fetch_k groups of m exactly equal values
    # inside a group the row id decides, and the groups' rows are not already in list order
    g = rows.reshape(F, m)
    assert (np.diff(g, axis=1) > 0).all()
    by_list = np.stack([c for c, _ in lists], axis=1)  # [F, m] in list order
    assert (g != by_list).any()


@pytest.mark.parametrize("metric", fc.METRICS)
@pytest.mark.parametrize("m", [3, 5])
def test_overlap_rows_stand_in_several_lists_and_the_sum_order_matters(m, metric):
    V, Qs = fc.overlap_case(m, metric)
    lists = fc.set_lists(Qs, V, fc.OVERLAP_FETCH, metric)
    cands = fc.fuse(lists, "rrf")
    hits = np.asarray([h for _, h in cands.values()])
    assert set(np.unique(hits)) == set(range(1, m + 1))  # hits between 1 and m, every value
    assert (hits >= 2).sum() >= 50
    # a row in several lists stands at different ranks in them
    pos = [{r: p for p, r in enumerate(c.tolist())} for c, _ in lists]
    multi = [r for r, (_, h) in cands.items() if h >= 2]
    assert any(len({p[r] for p in pos if r in p}) > 1 for r in multi)
    # a wrong accumulation would be caught: float32 or a reversed order ranks some pair the other way
    assert fc.order_differs(lists)
    # the weighted form of the case is another answer, and NULL weights are all-ones
    w = fc.WEIGHTS[m]
    assert {0.0, 0.5, 3.0} <= set(w)
    plain = fc.rank(cands)
    weighted = fc.rank(fc.fuse(lists, "rrf", w))
    assert (plain[0][:50] != weighted[0][:50]).any()
    ones = fc.rank(fc.fuse(lists, "rrf", np.ones(m)))
    np.testing.assert_array_equal(plain[0], ones[0])
    np.testing.assert_array_equal(_bits(plain[1]), _bits(ones[1]))
    # a zero weight leaves its list's rows in (hits counts them) with nothing added
    zero = w.index(0.0)
    only = [r for r in lists[zero][0].tolist() if cands[r][1] == 1]
    wc = fc.fuse(lists, "rrf", w)
    assert only and all(wc[r] == (0.0, 1) for r in only)


@pytest.mark.parametrize("metric", fc.METRICS)
def test_short_cases_are_short(metric):
    V, Q = fc.corpus(300, 32, seed=2)
    few = np.zeros(300, bool)
    few[np.random.default_rng(5).choice(300, size=20, replace=False)] = True
    offs = fc.offsets_of([3])
    s, i, f, h = fc.expected(Q[:3], offs, V, 50, 50, "rrf", metric, mask=few)
    assert (i[0, :20] >= 0).all() and few[i[0, :20]].all() and (i[0, 20:] == -1).all()  # k > the union
    assert (h[0, :20] == 3).all() and (h[0, 20:] == 0).all()
    assert (s[0, 20:] == 0).all() and np.isneginf(f[0, 20:]).all()
    s, i, f, h = fc.expected(Q[:3], offs, V, 5, 40, "max", metric, mask=np.zeros(300, bool))
    assert (i == -1).all() and (s == 0).all() and np.isneginf(f).all() and (h == 0).all()
    # a set without a sub-query is all "no result" too
    s, i, f, h = fc.expected(Q[:3], fc.offsets_of([0, 3]), V, 5, 40, "rrf", metric)
    assert (i[0] == -1).all() and (i[1] >= 0).all()


@pytest.mark.parametrize("metric", fc.METRICS)
def test_max_over_the_lists_is_brute_force_over_the_corpus(metric):
    cases = [fc.overlap_case(3, metric), fc.overlap_case(5, metric), fc.identical_case(2), fc.disjoint_case(2)]
    V, Q, offs = fc.mixed_sets_case()
    cases.append((V, Q[1:17]))
    for V, Qs in cases:
        mask = np.random.default_rng(9).random(V.shape[0]) < 0.5
        for k, fetch, m in ((10, 10, None), (10, 40, None), (64, 64, mask), (1, 1, None), (200, 200, None)):
            s, i, f, h = fc.expected(Qs, fc.offsets_of([len(Qs)]), V, k, fetch, "max", metric, mask=m)
            rows, vals = fc.brute_force_max(Qs, V, k, metric, m)
            np.testing.assert_array_equal(i[0, :rows.size], rows)
            np.testing.assert_array_equal(_bits(f[0, :rows.size]), _bits(vals))
    # the lists of the overlap case do overlap: the proof's case of a row ahead in one list only
    V, Qs = fc.overlap_case(3, metric)
    lists = fc.set_lists(Qs, V, 10, metric)
    assert np.unique(np.concatenate([c for c, _ in lists])).size < 30


def test_sizes_cases_have_their_sizes():
    V, Q, offs = fc.many_sets_case()
    sizes = np.diff(offs)
    assert sizes.size == 70 and sizes[:3].tolist() == [0, 1, 4] and sizes.max() <= 4 and offs[-1] == Q.shape[0]
    V, Q, offs = fc.mixed_sets_case()
    assert np.diff(offs).tolist() == [0, 1, 16, 0, 2] and offs[-1] == Q.shape[0]
    assert fc.SIZE_FETCH == (1, 63, 64, 65, 200)
    # one sub-query under MAX with fetch_k == k is the plain list
    V, Q = fc.corpus(300, 32, seed=2)
    for metric in fc.METRICS:
        c, kappa = fc.one_list(Q[0], V, 10, metric, None, fc._norms(V, metric))
        s, i, f, h = fc.expected(Q[:1], fc.offsets_of([1]), V, 10, 10, "max", metric)
        np.testing.assert_array_equal(i[0], c)
        np.testing.assert_array_equal(_bits(f[0]), _bits(kappa))
        assert (h == 1).all()
        np.testing.assert_array_equal(s[0].view(np.uint32), fc.key_scores(kappa, metric).view(np.uint32))

"""CPU preconditions of tests/test_gpu_exact_alone.py: a green GPU run means what
it claims only if each fixture of tests/_exact_cases.py is what its case says.  No GPU here.

* the merge lists are sorted (key desc, id asc) and sentinel padded, hold ids above 2^32, and every
  "short" case has fewer valid entries than k_out -- counted by a restatement of merge_block's
  survivor walk, which also names the branch (register sort, LDS sort, stream) each case reaches;
* the oracle (ref_cpu.exact_search, with its BLAS prefilter) equals a direct computation over all
  rows on every tie-heavy, masked or few-eligible corpus;
* a query meant to be flagged has more rows tied with its best than the largest KP (256), so no
  certificate can pass; a query meant to certify has no tie with its best and a gap of at least
  6 eps below its k-th row (the argument of tests/_planted.py);
* the row-range boundary the tie-block case uses is run_exact's.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _exact_cases as ec  # noqa: E402
import _planted as pl  # noqa: E402
from oracle import ref_cpu  # noqa: E402


def _assert_sorted_padded(K, I):
    G, B, k_in = K.shape
    assert K.dtype == np.float64 and I.dtype == np.int64
    valid = I >= 0
    assert np.isfinite(K[valid]).all()
    assert (K[~valid] == -np.inf).all() and (I[~valid] == -1).all()
    # valid entries first, then only padding
    assert (valid[..., :-1] >= valid[..., 1:]).all()
    a_k, b_k, a_i, b_i = K[..., :-1], K[..., 1:], I[..., :-1], I[..., 1:]
    both = valid[..., 1:]
    assert ((a_k > b_k) | ((a_k == b_k) & (a_i < b_i)))[both].all()
    for b in range(B):  # ids distinct within a query
        ids = I[:, b][valid[:, b]]
        assert np.unique(ids).size == ids.size


MERGE_TABLES = ec.FEW_VALID + ec.LIST_COUNTS + ec.K_SIZES


@pytest.mark.parametrize("c", MERGE_TABLES, ids=[ec.case_id(c) for c in MERGE_TABLES])
def test_merge_lists_are_sorted_padded_and_counted(c):
    K, I = ec.random_lists(c["G"], c["k_in"], c["counts"], c["seed"])
    assert K.shape == (c["G"], 3, c["k_in"])
    _assert_sorted_padded(K, I)
    assert tuple(int(v) for v in (I >= 0).sum(axis=(0, 2))) == c["counts"]
    if max(c["counts"]) >= 8:
        assert (I > 1 << 32).any()
    # the full lists each few-valid case runs after
    if c["name"] == "few":
        Kf, If = ec.random_lists(c["G"], c["k_in"], (c["G"] * c["k_in"],) * 3, c["seed"] + 1)
        _assert_sorted_padded(Kf, If)
        assert (If >= 0).all()


@pytest.mark.parametrize("c", ec.FEW_VALID, ids=[ec.case_id(c) for c in ec.FEW_VALID])
def test_few_valid_cases_reach_their_branch(c):
    K, I = ec.random_lists(c["G"], c["k_in"], c["counts"], c["seed"])
    KP = ec.merge_kp(c["k_in"], c["k_out"])
    n, branch = ec.merge_survivors(K[:, 0], I[:, 0], KP)
    assert n == c["counts"][0]  # T is (-inf, sentinel): G < KP
    assert c["short"] == (n < c["k_out"])
    want = "e1" if n <= 64 else "e2" if n <= 128 else "e4" if n <= 256 else "lds" if n <= 1024 else "stream"
    assert branch == want


def test_few_valid_table_covers_the_unwritten_slots():
    """Each register-sort width E with a KP it does not fill (c <= 64 E < KP), at every list
    count; and every c of the issue's list that a k_out can exceed has a short case."""
    for G in (1, 2, 33):
        seen = set()
        for c in ec.FEW_VALID:
            if c["G"] != G or not c["short"]:
                continue
            n, KP = c["counts"][0], ec.merge_kp(c["k_in"], c["k_out"])
            E = 1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else None
            if E and 64 * E < KP and 64 * E < c["k_out"]:
                seen.add(E)
        assert seen == {1, 2, 4}, (G, seen)
        for n in (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023):
            assert any(c["G"] == G and c["counts"][0] == n and c["short"] for c in ec.FEW_VALID), (G, n)


def test_list_count_cases_reach_their_branch():
    got = {}
    for c in ec.LIST_COUNTS:
        K, I = ec.random_lists(c["G"], c["k_in"], c["counts"], c["seed"])
        n, branch = ec.merge_survivors(K[:, 0], I[:, 0], ec.merge_kp(c["k_in"], c["k_out"]))
        got[(c["G"], c["k_in"])] = (n, branch)
        total = c["counts"][0]
        if c["G"] > ec.MERGE_HEADS:
            assert branch == "stream"
        elif c["G"] >= ec.merge_kp(c["k_in"], c["k_out"]):
            assert n < total or c["G"] == 32  # T is real: it cuts entries off
        else:
            assert n == total  # T = -inf
    assert got[(31, 32)][1] == "lds" and got[(1, 32)][1] == "e1"
    assert got[(512, 32)][1] != "stream" and got[(513, 32)][1] == "stream" and got[(600, 10)][1] == "stream"


def test_tie_fixtures_of_the_merge():
    K, I = ec.all_equal_lists(64, 32)
    _assert_sorted_padded(K, I)
    assert np.unique(K[:, 0]).size == 1
    K, I = ec.all_equal_lists(64, 32, contiguous=True)
    _assert_sorted_padded(K, I)
    assert ec.merge_survivors(K[:, 0], I[:, 0], 32) == (31 * 32 + 1, "lds")
    K, I = ec.all_equal_lists(64, 64, contiguous=True)
    _assert_sorted_padded(K, I)
    assert ec.merge_survivors(K[:, 0], I[:, 0], 64) == (63 * 64 + 1, "stream")  # overflows MERGE_BUF
    K, I = ec.tie_block_lists()
    _assert_sorted_padded(K, I)
    ek, ei = ref_cpu.merge_topk(K, I, 25)
    for b in range(3):
        in_lists = [(K[g, b] == -2.0).sum() for g in range(4)]
        assert in_lists[:3] == [10, 10, 10]  # one block of ties over three lists
        assert (ek[b] == -2.0).sum() == 15 and ek[b, -1] == -2.0  # ... cut by k_out in its middle


@pytest.mark.parametrize("G,k", [(32, 32), (64, 64), (512, 512), (33, 32)])
def test_heads_fixture_is_tight(G, k):
    K, I = ec.heads_are_the_answer(G, k)
    _assert_sorted_padded(K, I)
    for b in range(2):
        assert K[:, b, 0].min() > K[:, b, 1:].max()  # every head beats every deeper entry
        n, _ = ec.merge_survivors(K[:, b], I[:, b], ec.merge_kp(k, k))
        assert n == k  # exactly KP survivors: T is the KP-th best entry itself
    assert np.unique(K[:, 0, 0]).size == G and np.unique(K[:, 1, 0]).size == 1


# ---- the oracle against a direct computation ------------------------------------------------------
def _same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


CUS = 256  # (the fixtures that depend on the CU count are built for the device's at run time)


@pytest.mark.parametrize("metric", ec.BOTH)
def test_oracle_equals_direct_on_masked_and_few_eligible_rows(metric):
    V = ec.rows(ec.FEW_N, ec.FEW_D, 5)
    Q = ec.rows(3, ec.FEW_D, 6)
    for eligible in ec.FEW_ELIGIBLE:
        mask = ec.few_mask(eligible)
        assert int(mask.sum()) == eligible
        _same(ref_cpu.exact_search(Q, V, 300, metric, row_mask=mask), ec.direct_search(Q, V, 300, metric, mask))
    for c in ec.SCAN_CASES:
        if c["mask"] and c["metric"] == metric:
            V, Q, mask, words = ec.scan_data(c, CUS)
            assert words.size >= (V.shape[0] + 31) // 32
            _same(ref_cpu.exact_search(Q, V, c["k"], metric, row_mask=mask), ec.direct_search(Q, V, c["k"], metric, mask))
    for N, k in ec.FEW_UNMASKED:
        V, Q = ec.rows(N, 24, N), ec.rows(3, 24, N + 1)
        _same(ref_cpu.exact_search(Q, V, k, metric), ec.direct_search(Q, V, k, metric))


@pytest.mark.parametrize("metric", ec.BOTH)
def test_oracle_equals_direct_on_walls_of_ties(metric):
    V, Q, rpw = ec.boundary_ties(1500, 24, CUS)
    _same(ref_cpu.exact_search(Q, V, 10, metric), ec.direct_search(Q, V, 10, metric))
    V, Q, pos = ec.spread_copies()
    for k in (10, 40):
        got = ref_cpu.exact_search(Q, V, k, metric)
        _same(got, ec.direct_search(Q, V, k, metric))
        np.testing.assert_array_equal(got[1][0], pos[:k])  # the lowest copies
    V, Q = ec.zero_rows()
    _same(ref_cpu.exact_search(Q, V, 10, metric), ec.direct_search(Q, V, 10, metric))
    if metric == "cosine":
        np.testing.assert_array_equal(ref_cpu.exact_search(Q, V, 10, metric)[1][0], np.arange(10))
    V, Q, mask = ec.host_flagged()
    for m in (None, mask):
        _same(ref_cpu.exact_search(Q, V, 150, metric, row_mask=m), ec.direct_search(Q, V, 150, metric, m))
    V, Q, flagged = ec.gated(64, 40, 40)  # (a small device's corpus: the direct form over all rows)
    for m in (None, ec.gated_mask(V.shape[0])):
        _same(ref_cpu.exact_search(Q[:6], V, 200, metric, row_mask=m), ec.direct_search(Q[:6], V, 200, metric, m))
    V, Q, pos = ec.single_wg()
    _same(ref_cpu.exact_search(Q, V, 10, metric), ec.direct_search(Q, V, 10, metric))


def test_spread_copies_reach_the_stream_path_at_k40_only():
    """2100 copies over 64 ranges of 256 rows, about 33 a range.  At k = 10 (KE = 32) T is the
    32nd range's first copy, so 31 full lists and one entry survive: 993, the LDS sort.  At k = 40
    (KE = 64) 63 ranges' copies do: over MERGE_BUF, the stream path."""
    V, Q, pos = ec.spread_copies()
    n_wg, rpw = ec.row_split(V.shape[0], CUS)
    assert (n_wg, rpw) == (64, 256) == ec.row_split(V.shape[0], 304)
    keys = ref_cpu.exact_keys(Q[0], V, "cosine")
    K, I = ec.scan_lists(keys, n_wg, rpw, 32)
    assert ec.merge_survivors(K, I, 32) == (993, "lds")
    K, I = ec.scan_lists(keys, n_wg, rpw, 64)
    n, branch = ec.merge_survivors(K, I, 64)
    assert n > ec.MERGE_BUF and branch == "stream"


# ---- the certificate must fail / must pass -----------------------------------------------------------
@pytest.mark.parametrize("metric", ec.BOTH)
def test_host_flagged_queries_cannot_certify_and_the_others_must(metric):
    V, Q, mask = ec.host_flagged()
    plain = [b for b in range(ec.HOST_B) if b not in ec.HOST_FLAGGED]
    for m in (None, mask):
        ties = ec.tied_with_best(Q, V, metric, m)
        assert (ties[list(ec.HOST_FLAGGED)] > 256).all(), ties
        assert (ties[plain] == 1).all(), ties
        _, _, ek = ref_cpu.exact_search(Q, V, 257, metric, row_mask=m)
        for prec in ("bf16x3", "i8"):
            eps = pl.eps_upper(V, Q, metric, prec)
            for k in ec.HOST_K:
                gap = ek[:, k - 1] - ek[:, k]
                assert (gap[plain] >= 6.0 * eps[plain]).all(), (prec, k, gap[plain], eps[plain])


@pytest.mark.parametrize("metric", ec.BOTH)
@pytest.mark.parametrize("cus", [64])
def test_gated_queries_cannot_certify_and_the_others_must(metric, cus):
    for B, n_flag in ((40, 40), (16, 1), (16, 4), (16, 5)):
        V, Q, flagged = ec.gated(cus, B, n_flag)
        N = V.shape[0]
        assert N >= 256 * cus + 64 and ec.row_split(N, cus, gated=True)[0] == cus
        assert flagged.size == n_flag
        plain = np.setdiff1d(np.arange(B), flagged)
        for m in (None, ec.gated_mask(N)):
            ties = ec.tied_with_best(Q, V, metric, m)
            assert (ties[flagged] > 256).all(), ties
            assert (ties[plain] == 1).all(), ties
            if plain.size:
                _, _, ek = ref_cpu.exact_search(Q, V, 11, metric, row_mask=m)
                eps = pl.eps_upper(V, Q, metric, "bf16x3")
                assert ((ek[:, 9] - ek[:, 10])[plain] >= 6.0 * eps[plain]).all()
    # the copies of a distinct row lie in every workgroup's range
    V, Q, flagged = ec.gated(cus, 40, 40)
    _, rpw = ec.row_split(V.shape[0], cus, gated=True)
    _, ei, _ = ref_cpu.exact_search(Q[:1], V, ec.COPIES, metric)
    assert np.unique(ei[0] // rpw).size == cus


@pytest.mark.parametrize("metric", ec.BOTH)
def test_single_workgroup_queries_cannot_certify(metric):
    V, Q, pos = ec.single_wg()
    assert ec.row_split(300, 256, gated=True) == (1, 300) == ec.row_split(300, 304)
    assert pos.size == 280 and (ec.tied_with_best(Q, V, metric) == 280).all()


# ---- the row split -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [256, 304])
def test_row_split_is_run_exacts(cus):
    """n_wg = min(2 CUs, max(1, N / 256)), rpw = ceil(N / n_wg), then the ranges actually used."""
    for N in (1, 2, 255, 256, 257, 511, 512, 513, 1500, 5000, 9000, 16384, ec.big_n("issue", cus), ec.big_n("full", cus)):
        n0 = min(2 * cus, max(1, N // 256))
        rpw = (N + n0 - 1) // n0
        n_wg = (N + rpw - 1) // rpw
        assert ec.row_split(N, cus) == (n_wg, rpw)
        assert (n_wg - 1) * rpw < N <= n_wg * rpw
    # the two large cases: fewer than 2 CUs lists (511 on 256 CUs) and all 2 CUs, a short last range in both
    n_wg, rpw = ec.row_split(ec.big_n("issue", cus), cus)
    assert rpw == 257 and n_wg < 2 * cus and ec.big_n("issue", cus) - (n_wg - 1) * rpw < rpw
    if cus == 256:
        assert n_wg == ec.MERGE_HEADS - 1
    n_wg, rpw = ec.row_split(ec.big_n("full", cus), cus)
    assert (n_wg, rpw) == (2 * cus, 257) and ec.big_n("full", cus) - (n_wg - 1) * rpw == 3
    if cus == 256:
        assert n_wg == ec.MERGE_HEADS
    # the tie block straddles the first boundary
    V, Q, rpw = ec.boundary_ties(1500, 24, cus)
    assert rpw == ec.row_split(1500, cus)[1] == 300
    assert (V[rpw - 2:rpw + 3] == V[rpw]).all() and (Q[0] == V[rpw]).all()
    for metric in ec.BOTH:
        _, ei, _ = ref_cpu.exact_search(Q[:1], V, 10, metric)
        np.testing.assert_array_equal(ei[0, :5], np.arange(rpw - 2, rpw + 3))

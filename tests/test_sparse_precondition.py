"""The cases of tests/_sparse_cases.py have the properties their names claim, checked on the CPU
with the oracle alone: ties are ties, a "k beyond the matches" case has fewer than k matching rows, a
case named for a matching row with a key of 0 or below has one, cold rows share no term with the
queries, and the two forms of the key the contract allows give the same bits.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sparse_cases as sp  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_columns_are_valid_and_mix_the_row_lengths():
    for n_terms in sp.VOCABS:
        col = sp.column(1300, n_terms)
        assert col.n == 1300 and col.indptr[0] == 0 and col.indptr[-1] == col.terms.size
        lens = np.diff(col.indptr)
        assert set(lens.tolist()) == {min(L, n_terms) for L in sp.ROW_LENGTHS}
        for t, w in col.rows:
            assert (np.diff(t.astype(np.int64)) > 0).all() and np.isfinite(w).all()
            assert t.size == 0 or (t[0] >= 0 and t[-1] < n_terms)
        assert (col.terms == 0).any() and (col.terms == n_terms - 1).any()
    # the row counts of the issue fall below a wave trip, across one and a workgroup trip, into several chunks
    assert sp.ROWS == (3, 37, 513, 1300) and 37 < 64 < 256 < 513 and 1300 > 4 * 256


def test_queries_have_the_lengths_of_the_issue():
    for n_terms in sp.VOCABS:
        qs = sp.queries(n_terms)
        assert [t.size for t, _ in qs] == [min(L, n_terms) for L in (8, 0, 1, 1024, 8)]
        for t, w in qs:
            assert (np.diff(t.astype(np.int64)) > 0).all() and np.isfinite(w).all() and (w != 0).all()


def test_cold_rows_share_no_term_and_are_never_returned():
    col = sp.column(513, 30522)
    hot = np.asarray(sp.hot_terms(30522))
    cold = [r for r in range(col.n) if r % 5 == 4]
    assert all(not np.isin(col.rows[r][0], hot).any() for r in cold)
    assert any(col.rows[r][0].size for r in cold)
    qt, qw = sp.queries(30522)[0]
    assert np.isin(qt, hot).all()
    keys, matched = sp.keys_of(col, qt, qw)
    assert not matched[cold].any() and matched.sum() > 20
    sc, idx, ke = sp.expected(col, [(qt, qw)], 1024)
    assert not np.isin(idx[0], cold).any() and (idx[0] >= 0).sum() == matched.sum()


def test_ties_are_ties():
    col, qs = sp.tie_case()
    for qt, qw in qs:
        rows, keys = sp.one_list(col, qt, qw, 100)
        assert rows.size == 100
        same = np.diff(keys) == 0
        assert same.sum() >= 30, "few exact ties among the first 100"
        assert (np.diff(rows)[same] > 0).all()  # among equal keys the lower row comes first
        assert (np.diff(keys) <= 0).all()
    # a tie crosses the cut at k = 10: the row-id rule decides who is in
    rows, keys = sp.one_list(col, qs[0][0], qs[0][1], 11)
    assert keys[9] == keys[10]


def test_signed_case_ranks_matching_rows_with_keys_of_zero_and_below():
    col, qs = sp.signed_case()
    seen_neg = seen_zero = seen_unmatched_share = False
    for qt, qw in qs:
        keys, matched = sp.keys_of(col, qt, qw)
        seen_neg |= bool((matched & (keys < 0)).any())
        seen_zero |= bool((matched & (keys == 0)).any())
        shares = np.asarray([np.isin(t, qt).any() for t, _ in col.rows])
        seen_unmatched_share |= bool((shares & ~matched).any())  # only zero products: not a match
        sc, idx, ke = sp.expected(col, [(qt, qw)], 1024)
        n = int(matched.sum())
        assert (idx[0, :n] >= 0).all() and (idx[0, n:] == -1).all() and (ke[0, :n] <= ke[0, 0]).all()
        assert (ke[0, :n] <= 0).any()
    assert seen_neg and seen_zero and seen_unmatched_share


def test_zero_key_case():
    col, qs = sp.zero_key_case()
    sc, idx, ke = sp.expected(col, qs, 5)
    assert idx[0].tolist() == [0, 1, 2, -1, -1]
    assert ke[0, :3].tolist() == [3.0, 0.0, -2.0] and not np.signbit(ke[0, 1])
    assert np.isneginf(ke[0, 3:]).all() and (sc[0, 3:] == 0).all()


def test_beyond_case_has_fewer_matches_than_k():
    col, qs = sp.beyond_case()
    keys, matched = sp.keys_of(col, *qs[0])
    assert 0 < matched.sum() < 10
    sc, idx, ke = sp.expected(col, qs, 10)
    assert (idx[0] == -1).any() and (idx[0] >= 0).any()


def test_edge_terms_case():
    for n_terms in sp.VOCABS:
        col, qs = sp.edge_terms_case(n_terms)
        assert col.terms.max() == n_terms - 1 and col.terms.min() == 0
        sc, idx, ke = sp.expected(col, qs, 4)
        assert idx[0].tolist() == [1, 0, 2, -1] and ke[0, :3].tolist() == [3.0, 1.0, 0.5]
        assert idx[1].tolist() == [1, 2, -1, -1]


def test_both_forms_of_the_key_give_the_same_bits():
    for col, qs in (sp.signed_case(), sp.tie_case(513), (sp.column(513, 5), sp.queries(5)),
                    (sp.column(513, 2 ** 31 - 1), sp.queries(2 ** 31 - 1))):
        for qt, qw in qs:
            for r in range(0, col.n, 7):
                rt, rw = col.rows[r]
                a, _ = sp.row_key(rt, rw, qt, qw)
                b = sp.row_key_all_entries(rt, rw, qt, qw)
                assert _bits(a) == _bits(b) and not (a == 0 and np.signbit(a))


def test_mask_and_offset_in_the_oracle():
    col = sp.column(513, 30522)
    qs = sp.queries(30522)
    mask = np.random.default_rng(4).random(513) < 0.5
    sc, idx, ke = sp.expected(col, qs, 20, mask=mask, index_offset=1000)
    assert mask[idx[idx >= 0] - 1000].all()
    full = sp.expected(col, qs, 1024)
    assert ((full[1] >= 0).sum(axis=1) >= (idx >= 0).sum(axis=1)).all()
    assert (idx[1] == -1).all()  # the query without terms


def test_hybrid_oracle_edges():
    V, Q = sp.dense_rows(513)
    col = sp.column(513, 30522)
    qs = sp.queries(30522)
    # w_sparse == 0: the dense order
    sc, idx, fu, hi = sp.expected_hybrid(V, Q[:5], col, qs, 10, 40, "cosine", weights=(1.0, 0.0))
    for b in range(5):
        dense, _ = sp.fc.one_list(Q[b], V, 10, "cosine")
        assert idx[b].tolist() == dense.tolist()
    # a query without terms equals its dense-only fusion; hits are 1 or 2 elsewhere
    sc, idx, fu, hi = sp.expected_hybrid(V, Q[:5], col, qs, 10, 40, "cosine")
    assert (hi[1] == 1).all() and set(np.unique(hi).tolist()) <= {1, 2} and (hi == 2).any()

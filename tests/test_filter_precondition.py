"""The shared filter cases (tests/_filter_cases.py) do what they claim: the columns hold rows
without a value, +-inf, both zeros and values equal to the predicates' bounds; every predicate
passes some rows and fails some, except those built to be empty or full; negated and plain clauses
differ on the rows without a value; and the store metadata holds numeric, string, missing and bool
values that every store filter splits.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _filter_cases as fc  # noqa: E402


@pytest.mark.parametrize("n", [33, 257, 4099])
def test_columns_hold_what_the_contract_names(n):
    cols = fc.columns(n)
    assert cols.shape == (fc.N_COLS, n) and cols.dtype == np.float64
    for c in cols:
        assert np.isnan(c).any() and not np.isnan(c).all()
        assert (c == np.inf).any() and (c == -np.inf).any()
        zeros = c[c == 0.0]
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any(), "both -0.0 and +0.0"
        for bound in (1.0, 2.0, 2.5, 3.0, 5.0, -4.0):
            assert (c == bound).any(), bound
    assert not np.array_equal(cols[0], cols[1], equal_nan=True)


def test_sizes_cover_the_edges():
    W = [fc.n_words(n) for n in fc.SIZES]
    assert any(w % 2 for w in W) and any(w % 2 == 0 for w in W)
    assert any(n < 64 for n in fc.SIZES) and 64 in fc.SIZES and any(64 < n < 128 for n in fc.SIZES)
    assert any(n % 32 for n in fc.SIZES) and any(n % 32 == 0 for n in fc.SIZES)
    assert any(n > 4 * 256 for n in fc.SIZES), "more than one workgroup"


def test_predicates_cover_the_clause_space():
    assert [len(p) for p in fc.predicates(3)] == [0, 1, 8]
    assert len(fc.predicates(1)) == 1 and len(fc.predicates(256)) == 256
    preds = fc.predicates(256)
    clauses = [cl for p in preds for cl in p]
    assert {cl[3] for cl in clauses} == set(range(8)), "every flag combination"
    assert {len(p) for p in preds} >= {0, 1, 8} and max(len(p) for p in preds) == 8
    assert any(cl[1] == -math.inf for cl in clauses) and any(cl[2] == math.inf for cl in clauses)
    assert any(cl[1] > cl[2] for cl in clauses), "lo > hi"
    assert any(cl[1] == cl[2] for cl in clauses), "equality"
    assert {cl[0] for cl in clauses} == set(range(fc.N_COLS))
    assert not any(math.isnan(cl[1]) or math.isnan(cl[2]) for cl in clauses)


@pytest.mark.parametrize("n", [257, 4099])
def test_named_predicates_split_the_rows_unless_built_not_to(n):
    cols = fc.columns(n)
    for name, pred in fc.NAMED:
        c = int(fc.oracle_bits(cols, pred).sum())
        if name in fc.EMPTY:
            assert c == 0, name
        elif name in fc.FULL:
            assert c == n, name
        else:
            assert 0 < c < n, (name, c)


def test_negated_and_plain_clauses_differ_on_rows_without_a_value():
    cols = fc.columns(257)
    missing = np.isnan(cols[1])
    assert missing.any()
    for f in range(4):
        plain = fc.clause_bits(cols[1], 1.0, 3.0, f)
        neg = fc.clause_bits(cols[1], 1.0, 3.0, f | fc.NEG)
        assert not plain[missing].any() and neg[missing].all()
        np.testing.assert_array_equal(neg, ~plain)


def test_base_masks_are_mixed():
    b = fc.base_masks(3, 257)
    assert b.shape == (3, 9) and b.dtype == np.uint32
    bits = np.array([fc.unwords(w, 257) for w in b])
    assert bits.any(axis=1).all() and not bits.all(axis=1).any()


def test_store_metadata_is_mixed_and_every_filter_splits_it():
    md = fc.store_metadata(300)
    ts = [m.get("ts") for m in md]
    assert any(isinstance(v, int) and not isinstance(v, bool) for v in ts)
    assert any(isinstance(v, float) for v in ts) and any(isinstance(v, str) for v in ts)
    assert any(isinstance(v, bool) for v in ts) and any("ts" not in m for m in md)
    assert any(isinstance(m.get("price"), float) and math.isnan(m["price"]) for m in md)
    for f in fc.STORE_FILTERS:
        c = int(fc.meta_bits(md, f).sum())
        assert 0 < c < len(md), (f, c)
    # a bool is no number: True == 1, yet {"$gte": 0, "$lte": 1} passes no bool row
    hits = np.nonzero(fc.meta_bits(md, {"ts": {"$gte": 0, "$lte": 1}}))[0]
    assert all(not isinstance(md[r]["ts"], bool) for r in hits)
    assert any(md[r].get("ts") is True for r in range(len(md)))

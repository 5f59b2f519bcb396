"""CPU checks that the cases of tests/_group_cases.py have the properties their names claim, for the
oracle alone (no GPU): a "fast" case flags no query at the settings it is run with, a "dominant
group" case flags exactly the queries it says, the duplicated rows rank where the GPU test expects
them, and the oracle statement itself agrees with a naive per-group maximum."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _group_cases as gc  # noqa: E402


@pytest.mark.parametrize("metric", gc.METRICS)
@pytest.mark.parametrize("n,d,name", [(1100, 100, "random"), (513, 100, "modulo"), (4097, 100, "random"),
                                       (2000, 128, "random")])
def test_fast_cases_flag_no_query(n, d, name, metric):
    V, Q, g = gc.fast_case(n, d, name)
    keys = gc.oracle_keys(Q[:4], V, metric)
    G = gc.n_groups(g)
    assert G == gc.FAST_G
    # every k up to the number of groups, at the auto fetch and at the largest
    for k in (1, 2, 5, G):
        for knob in (0, 200):
            assert gc.flagged(keys, g, None, k, gc.fetch_k(knob, k)) == [], (k, knob)
    # ... and a k past the groups is what flags: every query, as soon as more than k' rows are eligible
    assert gc.flagged(keys, g, None, G + 1, gc.fetch_k(32, G + 1)) == [0, 1, 2, 3]


@pytest.mark.parametrize("metric", gc.METRICS)
@pytest.mark.parametrize("batch", gc.DOM_BATCHES)
def test_dominant_cases_flag_exactly_the_hot_queries(batch, metric):
    V, Q, g, hot = gc.dominant_case(3000, 40, batch)
    keys = gc.oracle_keys(Q, V, metric)
    assert len(hot) >= 1 and (batch < 3 or len(hot) < batch)  # mixed, from three queries on
    assert gc.flagged(keys, g, None, gc.DOM_K, gc.DOM_FETCH) == list(hot)
    assert gc.flagged(keys, g, None, gc.DOM_K, 200) == []
    for i, b in enumerate(hot):  # the hot query's best DOM_FETCH rows are its own group's
        top = gc.ranked_rows(keys[b], g)[:gc.DOM_FETCH]
        assert (g[top] == 1000 + i).all()


@pytest.mark.parametrize("metric", gc.METRICS)
def test_device_memory_case(metric):
    mask = np.random.default_rng(3).random(3000) < 0.7  # (the device-memory test's mask)
    V5, Q5, g5, hot5 = gc.dominant_case(3000, 40, 5)
    k5 = gc.oracle_keys(Q5, V5, metric)
    assert gc.flagged(k5, g5, None, gc.DOM_K, gc.DOM_FETCH) == list(hot5)
    assert set(gc.flagged(k5, g5, mask, gc.DOM_K, gc.DOM_FETCH)) <= set(hot5)  # (some copies masked away)


@pytest.mark.parametrize("metric", gc.METRICS)
def test_duplicates_rank_as_claimed(metric):
    V, Q, g, (a, b), (c, e) = gc.duplicates_case(700, 48)
    keys = gc.oracle_keys(Q[:2], V, metric)
    assert a < b and c < e and g[a] != g[b] and g[c] == g[e]
    assert keys[0, a] == keys[0, b] and keys[1, c] == keys[1, e]
    s, i, gg, k = gc.expected(keys, g, 3, metric)
    assert i[0, 0] == a and i[0, 1] == b and i[1, 0] == c and e not in i[1]


@pytest.mark.parametrize("metric", gc.METRICS)
@pytest.mark.parametrize("name", gc.LAYOUTS)
def test_oracle_agrees_with_per_group_maximum(name, metric):
    n = 400
    V, Q, _ = gc.fast_case(n, 24)
    g = gc.layout(name, n)
    mask = np.random.default_rng(1).random(n) < 0.6
    keys = gc.oracle_keys(Q[:2], V, metric)
    for m in (None, mask):
        s, i, gg, k = gc.expected(keys, g, 128, metric, m)
        for b in range(2):
            best = {}
            for r in range(n):
                if g[r] < 0 or (m is not None and not m[r]):
                    continue
                if g[r] not in best or keys[b, r] > keys[b, best[g[r]]]:
                    best[g[r]] = r  # (ascending r: an equal key keeps the lower row)
            want = sorted(best.values(), key=lambda r: (-keys[b, r], r))[:128]
            assert i[b, :len(want)].tolist() == want and (i[b, len(want):] == -1).all()
            assert gg[b, :len(want)].tolist() == [g[r] for r in want] and (gg[b, len(want):] == -1).all()
    if name == "all_negative":
        assert gc.n_groups(g) == 0
    if name == "huge_ids":
        assert g.max() == 2 ** 31 - 1

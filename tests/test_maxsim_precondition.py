"""Every case of tests/_maxsim_cases.py has the property its name claims, checked on the CPU from the
reference arithmetic alone (no GPU, no library): the tie case really has two groups with bit-equal
sums, the -0.0 case really has a key with its sign bit set that changes no order, the straddling
cases really cross the boundaries they name, and apart from the ties a case builds on purpose no two
distinct candidates of any set have equal sums (so an order can only be wrong, never ambiguous)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _maxsim_cases as mc  # noqa: E402

from oracle import ref_cpu  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _no_ties(Q, offs, V, g, n_slots, metric, mask=None, allow=()):
    ids, sums = mc.set_sums(Q, offs, V, g, n_slots, metric, mask)
    for s, acc in enumerate(sums):
        if offs[s + 1] <= offs[s]:
            continue
        u, cnt = np.unique(acc, return_counts=True)
        tied = {tuple(ids[acc == x].tolist()) for x in u[cnt > 1]}
        assert tied <= set(allow), (s, tied)


def test_query_blocks_are_what_the_cases_assume():
    assert [mc.query_block(d) for d in mc.DIMS] == [64, 64, 42, 28, 15]
    for d in (8, 768):
        n_sub, lengths = mc.straddle_sets(d)
        qb = mc.query_block(d)
        assert n_sub == qb + 1 == {8: 65, 768: 43}[d] and sum(lengths) == n_sub
        offs = mc.offsets_of(lengths)
        assert any(offs[s] < qb < offs[s + 1] for s in range(len(lengths))), "no set straddles the block boundary"
        assert max(lengths) <= mc.MAX_VECTORS
    # the piece forms: <= 1024 dims 4 pieces, <= 2048 dims 8, longer any length
    assert [4 if d <= 1024 else 8 if d <= 2048 else 0 for d in mc.DIMS] == [4, 4, 4, 8, 0]
    # the row counts: a partial 4-row trip, a partial word, one row past a workgroup's chunk, several
    # chunks with a ragged tail
    assert mc.ROWS[0] < 4 and mc.ROWS[1] % 32 and mc.ROWS[2] == mc.WG_ROWS + 1
    assert mc.ROWS[3] > 2 * mc.WG_ROWS and mc.ROWS[3] % mc.WG_ROWS % 32


def test_layouts_have_their_shapes():
    n = 1300
    assert np.unique(mc.layout("one_group", n)).tolist() == [5]
    assert np.unique(mc.layout("own_group", n)).size == n
    b = mc.layout("blocks", n)
    assert (np.diff(b) >= 0).all() and np.unique(b).size == mc.LAYOUT_G
    starts = mc.blocks_runs(n)
    run = np.diff(np.append(starts, n))
    assert run.min() > mc.WAVE_ROWS, "a run does not cross a wave's 128 rows"
    # a run crosses a wave boundary and a workgroup boundary in its middle
    assert any(s % mc.WAVE_ROWS and (s // mc.WAVE_ROWS) != ((s + l - 1) // mc.WAVE_ROWS) for s, l in zip(starts, run))
    assert any((s // mc.WG_ROWS) != ((s + l - 1) // mc.WG_ROWS) for s, l in zip(starts, run))
    m = mc.layout("modulo", n)
    assert (m[:-1] != m[1:]).all(), "modulo combines something"
    assert (m[0] == m[mc.WG_ROWS * 2 + 2 * mc.LAYOUT_G - (mc.WG_ROWS * 2) % mc.LAYOUT_G]), "no slot hit from distant chunks"
    sn = mc.layout("some_negative", n)
    assert (sn < 0).any() and (sn >= 0).any() and (sn == -(2 ** 31)).any()
    ps = mc.layout("past_slots", n)
    skipped = int((ps.astype(np.int64) >= mc.PAST_SLOTS).sum())
    assert 0 < skipped < n and (ps == 2 ** 31 - 1).any() and mc.slots_of("past_slots", ps) == mc.PAST_SLOTS
    assert np.unique(ps[mc.eligible(ps, mc.PAST_SLOTS)]).size == mc.PAST_SLOTS
    for name in mc.LAYOUTS:
        for nn in mc.ROWS:
            g = mc.layout(name, nn)
            assert g.dtype == np.int32 and g.size == nn and 1 <= mc.slots_of(name, g)


@pytest.mark.parametrize("name", ["blocks", "random", "some_negative"])
def test_masks_do_what_they_say(name):
    n = 1300
    g = mc.layout(name, n)
    slots = mc.slots_of(name, g)
    cut, _ = mc.mask_of("cut_run", g, slots)
    if name == "blocks":  # rows gone from inside one run, rows of that run left on both sides
        lo, hi = np.nonzero(~cut)[0][[0, -1]]
        assert g[lo - 1] == g[lo] and g[hi] == g[hi + 1]
    tail, _ = mc.mask_of("wave_tail", g, slots)
    assert not tail[mc.WAVE_ROWS - 1] and tail[mc.WAVE_ROWS] and not tail[n - 1] and tail[0]
    drop, gid = mc.mask_of("drop_group", g, slots)
    assert (g == gid).any() and not drop[g == gid].any() and drop[g != gid].all()
    ids, _ = mc.maxima(np.zeros((1, n)), g, slots, drop)
    assert gid not in ids.tolist() and ids.size == np.unique(g[mc.eligible(g, slots)]).size - 1
    none, _ = mc.mask_of("nothing", g, slots)
    assert not none.any() and mc.maxima(np.zeros((1, n)), g, slots, none)[0].size == 0


@pytest.mark.parametrize("metric", mc.METRICS)
def test_tie_case_has_two_groups_with_bit_equal_sums(metric):
    V, Q, g, (a, b) = mc.tie_case()
    assert a < b
    offs = mc.offsets_of([1, 2, 3])
    ids, sums = mc.set_sums(Q, offs, V, g, int(g.max()) + 1, metric)
    for acc in sums:
        assert _bits(acc[ids == a]) == _bits(acc[ids == b])
    sc, gr, sm = mc.expected(Q, offs, V, g, int(g.max()) + 1, 4, metric)
    for s in range(3):
        pa, pb = np.nonzero(gr[s] == a)[0], np.nonzero(gr[s] == b)[0]
        assert pa.size == 1 and pb.size == 1 and pb[0] == pa[0] + 1, "the pair is not adjacent in the top 4, lower id first"
    _no_ties(Q, offs, V, g, int(g.max()) + 1, metric, allow={(a, b)})


def test_exact_match_key_is_minus_zero_and_changes_no_order():
    V, Q, g, row = mc.exact_match_case()
    k = ref_cpu.exact_keys(Q[0], V, "euclidean")
    assert k[row] == 0.0 and np.signbit(k[row]), "the key of the exact match is not -0.0"
    assert np.signbit(ref_cpu.exact_keys(V[2], V, "euclidean")[2])
    assert not np.signbit(k[row] + 0.0)
    slots = mc.slots_of("modulo", g)
    offs = mc.offsets_of([1, 3])
    sc, gr, sm = mc.expected(Q, offs, V, g, slots, slots, "euclidean")
    # the group of the matching row is first for the one-vector set, with sum +0.0
    assert gr[0, 0] == g[row] and _bits(sm[0, :1])[0] == 0
    # -0.0 and +0.0 compare equal: the order is what plain doubles give
    ids, M = mc.maxima(np.stack([ref_cpu.exact_keys(q, V, "euclidean") for q in Q]), g, slots)
    raw = np.stack([ref_cpu.exact_keys(q, V, "euclidean") for q in Q])
    M_raw = np.stack([[raw[t, g == gid].max() for gid in ids] for t in range(Q.shape[0])])
    assert (M == M_raw).all()
    _no_ties(Q, offs, V, g, slots, "euclidean")


@pytest.mark.parametrize("metric", mc.METRICS)
def test_no_unintended_ties_in_the_random_cases(metric):
    """The seeds of the cases tests/test_gpu_search_maxsim.py runs: no two candidates of a set share a
    sum (one_group has one candidate; own_group over duplicates does not occur)."""
    for d, n in ((8, 1300), (100, 513), (768, 37), (1100, 37), (2100, 37), (8, 3), (100, 37)):
        n_sub = 8
        V, Q = mc.corpus(n, d, 0, n_sub)
        offs = mc.offsets_of([1, 2, 5])
        for name in mc.LAYOUTS:
            g = mc.layout(name, n)
            _no_ties(Q, offs, V, g, mc.slots_of(name, g), metric)
    V, Q = mc.corpus(1300, 8, 0, 8)
    g = mc.sparse_layout(1300)
    assert mc.SPARSE_SLOTS > 4 * mc.SEG_SLOTS and 0 <= int(g.min()) and int(g.max()) < mc.SPARSE_SLOTS
    assert np.unique(g).size > 1000 and np.bincount(g).max() > 100 and (np.diff(g.astype(np.int64)) > 0).any()
    _no_ties(Q, mc.offsets_of([3, 0, 5]), V, g, mc.SPARSE_SLOTS, metric)
    V, Q = mc.corpus(513, 8, 2, sum(mc.SET_LENGTHS))
    g = mc.layout("random", 513)
    _no_ties(Q, mc.offsets_of(list(mc.SET_LENGTHS)), V, g, mc.slots_of("random", g), metric)
    for d in (8, 768):
        n_sub, lengths = mc.straddle_sets(d)
        V, Q = mc.corpus(37, d, 1, n_sub)
        g = mc.layout("random", 37)
        _no_ties(Q, mc.offsets_of(lengths), V, g, mc.slots_of("random", g), metric)


def test_oracle_is_the_literal_definition():
    """expected() against a loop written straight from the contract."""
    V, Q = mc.corpus(37, 8, 3, 6)
    g = mc.layout("some_negative", 37)
    offs = mc.offsets_of([0, 1, 3, 2])
    mask = np.ones(37, bool)
    mask[5:11] = False
    for metric in mc.METRICS:
        sc, gr, sm = mc.expected(Q, offs, V, g, 7, 4, metric, mask)
        keys = [ref_cpu.exact_keys(q, V, metric) for q in Q]
        for s in range(4):
            cands = []
            for gid in range(7):
                rows = [r for r in range(37) if g[r] == gid and mask[r]]
                if not rows or offs[s + 1] == offs[s]:
                    continue
                acc = 0.0
                for t in range(offs[s], offs[s + 1]):
                    acc = acc + max(float(keys[t][r]) + 0.0 for r in rows)
                cands.append((-acc, gid))
            cands.sort()
            want_g = [c[1] for c in cands[:4]] + [-1] * (4 - min(4, len(cands)))
            want_s = [-c[0] for c in cands[:4]] + [-np.inf] * (4 - min(4, len(cands)))
            assert gr[s].tolist() == want_g
            assert _bits(sm[s]).tolist() == _bits(np.array(want_s)).tolist()
            assert sc[s].tolist() == [np.float32(x) if np.isfinite(x) else np.float32(0) for x in want_s]

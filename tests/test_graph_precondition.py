"""The CPU preconditions of tests/test_gpu_graph_exact.py: conditions on the data of
tests/_graph_cases.py that the restatements (oracle.ref_cpu.graph_beam_search / graph_add) meet
on their own, never measured against the library.

  * determinism: graph_search_kernel's result depends on the order in which its waves arrive only
    where a visited-table probe chain reaches GS_PROBE = 64 slots.  Every team's visited set of
    every case leaves the table's longest run of occupied slots below 64, so no chain can.
  * exactness: every dot product of every case is representable in fp32, and so is every partial
    sum on the way (the magnitudes stay below 2^24 units), so the kernel's FMA order cannot show.
  * reach: the events that distinguish a right kernel from a nearly right one do occur.
  * teeth: each deliberately wrong variant of the restatement changes the result of some case.
"""
import os
import sys

import numpy as np
import pytest

from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # tests/_graph_cases.py, under any pytest import mode
import _graph_cases as gc  # noqa: E402

NAMES = [c["name"] for c in gc.SEARCH]


@pytest.mark.parametrize("name", NAMES)
def test_no_probe_chain_can_reach_the_limit(name):
    runs = [gc.longest_run(v) for v in gc.restated(name)["trace"]["visited_sets"]]
    print(f"{name}: longest run of occupied visited slots {max(runs)} over {len(runs)} team searches")
    assert max(runs) < ref_cpu.GS_PROBE
    if gc.BY_NAME[name]["graph"] == "hash":
        assert max(runs) >= 2  # a probe really happens


def test_longest_run_model():
    assert gc.longest_run(set()) == 0
    assert gc.longest_run({5}) == 1
    assert gc.longest_run({5, 5 + 16384, 5 + 32768}) == 3  # one slot, two rows walk on
    h = lambda r: (r * 2654435761) & 16383
    a = next(r for r in range(1, 16384) if h(r) == 16383)  # wraps around the table's end
    b = next(r for r in range(16384) if h(r) == 0)
    assert gc.longest_run({a, b, a + 16384}) == 3


@pytest.mark.parametrize("name", NAMES)
def test_every_dot_product_is_exact(name):
    c = gc.BY_NAME[name]
    V, Q, _, _ = gc.inputs(c)
    V64 = gc.rows64(c["N"], c["D"], c["seed"])
    sc = gc.scales(c["N"], c["D"], c["seed"], c["metric"])
    for q in Q:
        _, qn2, dots = ref_cpu.graph_query_scores(V64, q, c["metric"], sc)
        assert np.array_equal(dots.astype(np.float32).astype(np.float64), dots)
        q64 = q.astype(np.float64)
        assert float(qn2) == float(q64 @ q64)
        if c["metric"] == "cosine":  # q_hat = q * 2^-j exactly: |q|^2 is zero or a power of 4
            n2 = float(qn2)
            assert n2 == 0.0 or (np.log2(n2) / 2.0).is_integer()
            unit = 1.0 if n2 == 0.0 else 1.0 / np.sqrt(n2)
        else:
            unit = 1.0
        # partial sums are multiples of `unit` no larger than sum |q_hat_i x_i|: below 2^24 units
        assert (np.abs(V64) @ np.abs(q64)).max() < 2.0 ** 24
        assert float(np.float32(unit)) == unit
    if c["metric"] == "euclidean":
        assert np.array_equal(sc.astype(np.float64), (V64 * V64).sum(1))


def test_the_matrix_reaches_the_events_that_matter():
    seen = dict(shared_neighbour=[], beam_overflow=[], entries_exceed_ef=[], tie_in_top_k=[])
    for name in NAMES:
        r = gc.restated(name)
        for ev in ("shared_neighbour", "beam_overflow", "entries_exceed_ef"):
            if r["trace"].get(ev, 0) > 0:
                seen[ev].append(name)
        for lab, d in zip(r["labels"], r["dist"]):
            d = d[lab >= 0]
            if np.unique(d).size < d.size:
                seen["tie_in_top_k"].append(name)
                break
    for ev, names in seen.items():
        print(f"{ev}: {len(names)} cases, first {names[:3]}")
        assert names, ev


# the cases most likely to tell a variant apart come first: the first that does is reported
_TEETH_ORDER = sorted(NAMES, key=lambda n: (gc.BY_NAME[n]["teams"] > 7, not n.startswith(("d448", "ent256-t5", "r1-"))))


@pytest.mark.parametrize("flaw", ref_cpu.BEAM_FLAWS)
def test_teeth_each_wrong_search_variant_is_told_apart(flaw):
    caught = next((n for n in _TEETH_ORDER if not gc.same_result(gc.restated(n), gc.restated(n, flaw))), None)
    print(f"{flaw}: caught by {caught}")
    assert caught is not None, flaw


def test_the_enter_test_is_only_a_filter():
    """Testing each fresh row against the beam as updated by the rows before it (hnswlib's form)
    instead of the beam as of the start of the iteration cannot be told apart: it never drops a
    row of the best ef of beam + fresh, and the merge takes exactly those.  So the matrix need
    not, and cannot, distinguish the two; a test that is too strict is caught above."""
    for n in NAMES:
        if gc.BY_NAME[n]["teams"] <= 7 and gc.BY_NAME[n]["N"] <= gc.N_BASE:
            assert gc.same_result(gc.restated(n), gc.restated(n, "enter_against_updated_beam")), n


@pytest.mark.parametrize("metric", gc.METRICS)
def test_the_restatement_is_a_search(metric):
    """Sanity, not a pin: with one team the beam search finds what hnswlib's one-at-a-time search
    finds on the same graph (recall@10 against the exact top 10, within 0.05)."""
    rng = np.random.default_rng(61)
    N, D, nq, k, ef = 3000, 32, 20, 10, 64
    V = rng.standard_normal((N, D)).astype(np.float32)
    Q = rng.standard_normal((nq, D)).astype(np.float32)
    V64 = V.astype(np.float64)
    sq = (V64 * V64).sum(1)
    Dm = sq[:, None] + sq[None, :] - 2.0 * (V64 @ V64.T)
    np.fill_diagonal(Dm, np.inf)
    nbr = np.argsort(Dm, axis=1, kind="stable")[:, :16].astype(np.int32)
    ent = gc.spread_entries(N, 64)
    _, ei, _ = ref_cpu.exact_search(Q, V, k, metric)
    sc = ref_cpu._row_scales(V, metric)
    hits_beam = hits_one = 0
    for b in range(nq):
        want = set(ei[b].tolist())
        hits_beam += len(want & set(ref_cpu.graph_beam_search(V64, nbr, ent, Q[b], k, ef, metric, scales=sc)[0].tolist()))
        hits_one += len(want & set(ref_cpu.graph_search(V, nbr, ent, Q[b], k, ef, metric)[0].tolist()))
    r_beam, r_one = hits_beam / (nq * k), hits_one / (nq * k)
    print(f"{metric}: recall@10 beam {r_beam:.3f}, one at a time {r_one:.3f}")
    assert r_beam >= r_one - 0.05


@pytest.mark.parametrize("metric", gc.METRICS)
def test_teeth_each_wrong_insert_variant_is_told_apart(metric):
    X = gc.add_rows(32, 500)
    nbr, _, amb = ref_cpu.graph_build(X[:400], metric, degree=16, knn=16, n_entries=8)
    assert not amb.any()
    want = ref_cpu.graph_add(X, nbr, 400, metric, degree=16, knn=16)
    assert want.shape == (500, 16) and (want[400:, 0] >= 0).all()
    for flaw in ref_cpu.ADD_FLAWS:
        got = ref_cpu.graph_add(X, nbr, 400, metric, degree=16, knn=16, flaw=flaw)
        changed = int((got != want).any(axis=1).sum())
        print(f"{metric} {flaw}: {changed} lists differ")
        assert changed > 0, flaw

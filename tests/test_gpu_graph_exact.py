"""The graph path pinned bit for bit: graph_search_kernel + graph_merge_kernel against
oracle.ref_cpu.graph_beam_search, and vdb_graph_add (pass 1, graph_prune_kernel's sort branch,
the host mirror, capacity growth, graph_scatter_kernel) against oracle.ref_cpu.graph_add.

tests/test_gpu_graph.py judges this path by recall and by distances at rtol 1e-4, which a beam
that drops a list's last slot, a wrong tie rule, a skipped entry rank, an ef off by one, a wrong
statistic or a dropped dimension chunk would all pass.  Here the data (tests/_graph_cases.py)
makes every fp32 score the kernel forms exact or a single rounding, and the CPU preconditions
(tests/test_graph_precondition.py) exclude the one source of non-determinism (a visited-table
probe chain of 64), so labels, distances as fp32 bits, both statistics and every neighbour list
must EQUAL the restatement's.  No tolerance anywhere in this file.
"""
import os
import sys

import numpy as np
import pytest

from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # tests/_graph_cases.py, under any pytest import mode
import _graph_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


@pytest.fixture(scope="module")
def index_of(vdb):
    """One index per (metric, rows) of the search matrix, shared by its cases."""
    made = {}

    def get(metric, N, D, seed):
        key = (metric, N, D, seed)
        if key not in made:
            made[key] = vdb.NativeIndex(D, metric)
            made[key].add(gc.rows(N, D, seed))
        return made[key]

    yield get
    for ix in made.values():
        ix.close()


def _assert_search_equals(g, Q, k, ef, want):
    """One host-memory call: labels, distances (fp32 bits) and the three statistics' increase."""
    before = {s: g.stat(s) for s in ("iterations", "visited", "queries")}
    labels, dist = g.search(Q, k, ef=ef)
    moved = {s: g.stat(s) - before[s] for s in before}
    np.testing.assert_array_equal(labels, want["labels"])
    np.testing.assert_array_equal(dist.view(np.uint32), want["dist"].view(np.uint32))
    assert moved == dict(iterations=want["iterations"], visited=want["visited"], queries=Q.shape[0]), moved
    return labels, dist


@pytest.mark.parametrize("name", [c["name"] for c in gc.SEARCH])
def test_search_equals_the_restated_beam(vdb, index_of, name):
    c = gc.BY_NAME[name]
    V, Q, nbr, ent = gc.inputs(c)
    g = vdb.NativeGraph.from_arrays(index_of(c["metric"], c["N"], c["D"], c["seed"]), nbr, ent)
    g.set_param("teams", c["teams"])
    labels, dist = _assert_search_equals(g, Q, c["k"], c["ef"], gc.restated(name))
    if c["graph"] == "tiny":  # the beam never fills: 4 reachable rows, then -1 / inf
        assert ((labels >= 0).sum(axis=1) == 4).all() and np.isinf(dist[labels < 0]).all()
    g.close()


@pytest.mark.parametrize("metric", gc.METRICS)
def test_search_of_a_built_graph_equals_the_restated_beam(vdb, metric):
    """The same pin on the lists and entries vdb_graph_build itself produces."""
    N, D, k, ef, teams = 1500, 64, 63, 63, 2
    V = gc.rows(N, D, 7)
    Q = gc.queries(metric, D, 9, 7)
    ix = vdb.NativeIndex(D, metric)
    ix.add(V)
    g = vdb.NativeGraph.build(ix, degree=16, knn=16, n_entries=64)
    nbr, ent = g.to_arrays()
    want = gc.beam_batch(V, Q, nbr, ent, k, ef, metric, teams)
    assert max(gc.longest_run(v) for v in want["trace"]["visited_sets"]) < ref_cpu.GS_PROBE
    g.set_param("teams", teams)
    _assert_search_equals(g, Q, k, ef, want)
    g.close()
    ix.close()


@pytest.mark.parametrize("metric", gc.METRICS)
def test_device_memory_call_equals_host_memory_call(vdb, index_of, metric):
    """search_device with teams > 1 (the caller's buffers, the teams' scratch behind them): byte
    for byte what the host-memory call returns, which is pinned above."""
    import torch
    c = gc.BY_NAME[f"ent256-t5-{metric}"]
    V, Q, nbr, ent = gc.inputs(c)
    g = vdb.NativeGraph.from_arrays(index_of(metric, c["N"], c["D"], c["seed"]), nbr, ent)
    g.set_param("teams", c["teams"])
    labels, dist = _assert_search_equals(g, Q, c["k"], c["ef"], gc.restated(c["name"]))
    q = torch.from_numpy(Q).cuda()
    dl = torch.full((Q.shape[0], c["k"]), -7, dtype=torch.int64, device="cuda")
    dd = torch.full((Q.shape[0], c["k"]), -7.0, dtype=torch.float32, device="cuda")
    g.search_device(q.data_ptr(), Q.shape[0], c["k"], c["ef"], dl.data_ptr(), dd.data_ptr(),
                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert dl.cpu().numpy().tobytes() == labels.tobytes()
    assert dd.cpu().numpy().tobytes() == dist.tobytes()
    g.close()


def _extend_and_compare(ix, g, X, n, adds, metric, degree, knn, fill):
    """Each add: the exported array after it == graph_add(the exported array before it), for every
    row, order included; the entry rows stay.  Returns the row count reached."""
    for m in adds:
        before, ent0 = g.to_arrays()
        ix.add(X[n:n + m])
        g.add()
        n += m
        after, ent1 = g.to_arrays()
        want = ref_cpu.graph_add(X[:n], before, n - m, metric, degree=degree, knn=knn, fill=bool(fill))
        diff = np.nonzero((after != want).any(axis=1))[0]
        assert diff.size == 0, f"add of {m} to {n - m}: {diff.size} lists differ, first row {diff[0]}: " \
                               f"{after[diff[0]]} vs {want[diff[0]]}"
        np.testing.assert_array_equal(ent1, ent0)
    return n


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("metric", gc.METRICS)
@pytest.mark.parametrize("case", gc.ADD, ids=[a[0] for a in gc.ADD])
def test_add_equals_the_restated_insert(vdb, case, metric, fill):
    name, D, degree, knn, n0, adds = case
    X = gc.add_rows(D, n0 + sum(adds))
    ix = vdb.NativeIndex(D, metric)
    ix.set_param("graph_fill", fill)
    ix.add(X[:n0])
    if knn is None:  # attached: vdb_graph_add falls back to knn = degree
        g = vdb.NativeGraph.from_arrays(ix, gc.knn_lists(X[:n0], degree), gc.spread_entries(n0, 16))
        knn = degree
    else:
        g = vdb.NativeGraph.build(ix, degree=degree, knn=knn, n_entries=64)
    n = _extend_and_compare(ix, g, X, n0, adds, metric, degree, knn, fill)
    assert g.info()[0] == n
    if name == "r16-grow-then-fit":  # one exact search of the extended graph (the device array, not the mirror)
        nbr, ent = g.to_arrays()
        Q = gc.queries(metric, D, 9, 11)
        want = gc.beam_batch(X, Q, nbr, ent, 63, 63, metric, 2)
        assert max(gc.longest_run(v) for v in want["trace"]["visited_sets"]) < ref_cpu.GS_PROBE
        g.set_param("teams", 2)
        _assert_search_equals(g, Q, 63, 63, want)
    g.close()
    ix.close()


def test_import_refuses_repeated_entry_rows(vdb):
    """graph_search_kernel ranks the entries by counting the better ones, so two copies of a row
    would share a rank and leave a counted beam slot unwritten: vdb_graph_import refuses them.
    Attach only: a graph with repeated entries is never searched."""
    V = gc.rows(8, 8, 7)
    ix = vdb.NativeIndex(8, "euclidean")
    ix.add(V)
    nbr = gc.tiny_graph()
    for ent in ([0, 0], [3, 1, 3], [5, 2, 7, 2, 6]):
        with pytest.raises(ValueError, match="repeated"):
            vdb.NativeGraph.from_arrays(ix, nbr, np.asarray(ent, np.int32))
    vdb.NativeGraph.from_arrays(ix, nbr, np.asarray([3, 1, 0], np.int32)).close()  # distinct rows, any order
    with pytest.raises(ValueError):
        vdb.NativeGraph.from_arrays(ix, nbr, np.asarray([8], np.int32))  # out of range, as before
    ix.close()

"""MaxSim search (include/vdb.h vdb_index_search_maxsim; csrc/vdb_maxsim.hip).

The contract: a row is eligible when its group id lies in [0, n_group_slots) and the mask has it;
m[t][g] is the maximum over g's eligible rows of (canonical fp64 key + 0.0); a set's sum adds its
m[t][g] in sub-query order; the groups with an eligible row rank by (sum desc, id asc); slots past
min(k, candidates) hold 0 / -1 / -inf.  Every case compares all three outputs with the literal
oracle of tests/_maxsim_cases.py (preconditions: tests/test_maxsim_precondition.py) BIT FOR BIT: the
fp64 sums as uint64, the fp32 scores as uint32; no tolerance appears anywhere.

``_check`` runs a case in host memory and in device memory.  Every output carries a guard region past
[n_sets][k] filled with a sentinel, which must be untouched afterwards.

Shapes are the smallest that reach each path: rows of 8 .. 2100 dims (the 4-piece, 8-piece and
any-length forms; at 768 a scan block is 42 sub-queries), 3 .. 1300 rows (a partial 4-row trip, a
partial word, one row past a workgroup's chunk, several chunks), sets of 0 .. 64 vectors, one more
sub-query than a block holds, and more group slots than one rank segment takes.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _maxsim_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 257
S_GRP = -7
METRICS = mc.METRICS
VDB_ERR_INVALID = -1
VDB_ERR_NONFINITE = -4
STATS = ("maxsim_searches", "maxsim_sets", "maxsim_bad_sets", "maxsim_skipped_rows")
STILL = ("searches", "queries", "searches_fp32", "searches_bf16x3", "searches_bf16", "searches_i8", "searches_i8x3",
         "searches_i8q", "searches_q4", "searches_wide", "group_searches", "fused_searches", "range_searches")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    assert _vdb.VDB_ERR_INVALID == VDB_ERR_INVALID and _vdb.VDB_ERR_NONFINITE == VDB_ERR_NONFINITE
    return _vdb


@pytest.fixture(scope="module")
def indexes(vdb):
    """One index per (rows, metric, precision) of the module, built on first use."""
    made = {}

    def get(V, metric, precision=None):
        key = (V.tobytes(), V.shape, metric, precision)
        if key not in made:
            ix = vdb.NativeIndex(V.shape[1], metric, precision=precision)
            if V.shape[0]:
                ix.add(V)
            assert ix.count() == V.shape[0]
            made[key] = ix
        return made[key]

    yield get
    for ix in made.values():
        ix.close()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what=""):
    """The three outputs bit for bit (got / want: (scores, groups, sums); None entries skipped)."""
    for name, g, w in zip(("scores", "groups", "sums"), got, want):
        if g is None or w is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} {what}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{name} {what}")


def _call(ix, Q, offs, n_slots, k, mask=None, with_sums=True, n_sub=None, n_sets=None, mem=0, null=()):
    """The C-ABI call in host memory with guarded outputs -> (rc, (scores, groups, sums))."""
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    offs = np.ascontiguousarray(offs, np.int64)
    n_sub = Q.shape[0] if n_sub is None else n_sub
    S = offs.size - 1 if n_sets is None else n_sets
    n = max(S, 0) * max(k, 0)
    sc = np.full(n + GUARD, np.nan, np.float32)
    gr = np.full(n + GUARD, S_GRP, np.int32)
    sm = np.full(n + GUARD, np.nan, np.float64) if with_sums else None
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    code = ix._lib.vdb_index_search_maxsim(
        ix._h, None if "queries" in null or not Q.size else _p(Q), n_sub, None if "offsets" in null else _p(offs), S,
        n_slots, k, _p(m), mem, None if "scores" in null else _p(sc), None if "groups" in null else _p(gr), _p(sm), None)
    assert np.isnan(sc[n:]).all(), "scores guard touched"
    assert (gr[n:] == S_GRP).all(), "groups guard touched"
    assert sm is None or np.isnan(sm[n:]).all(), "sums guard touched"
    shape = (max(S, 0), max(k, 0))
    return code, (sc[:n].reshape(shape), gr[:n].reshape(shape), None if sm is None else sm[:n].reshape(shape))


def _call_device(ix, Q, offs, n_slots, k, mask=None, with_sums=True, n_sub=None):
    """The same call with every argument in device memory on a side stream -> the three outputs."""
    import torch
    Q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(-1, ix.dim))
    offs = np.ascontiguousarray(offs, np.int64)
    S = offs.size - 1
    n_sub = Q.shape[0] if n_sub is None else n_sub
    n = S * k
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dq = torch.from_numpy(Q.copy()).to(dev) if Q.size else None
        do = torch.from_numpy(offs.copy()).to(dev)
        dm = torch.from_numpy(np.ascontiguousarray(mask, np.uint32).view(np.int32).copy()).to(dev) if mask is not None else None
        ds = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        dg = torch.full((n + GUARD,), S_GRP, dtype=torch.int32, device=dev)
        du = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device=dev)
        ix.search_maxsim_device(dq.data_ptr() if dq is not None else 0, n_sub, do.data_ptr(), S, n_slots, k,
                                ds.data_ptr(), dg.data_ptr(), out_sums_ptr=du.data_ptr() if with_sums else 0,
                                mask_ptr=dm.data_ptr() if dm is not None else 0, stream=st.cuda_stream)
    st.synchronize()
    s, g, u = (x.cpu().numpy() for x in (ds, dg, du))
    assert np.isnan(s[n:]).all() and (g[n:] == S_GRP).all(), "guard touched (device)"
    assert np.isnan(u[n if with_sums else 0:]).all(), "guard touched (device)"
    return s[:n].reshape(S, k), g[:n].reshape(S, k), u[:n].reshape(S, k) if with_sums else None


def _check(ix, V, Q, offs, groups, n_slots, k, metric, mask=None, what="", device=True, want=None):
    """Call in host and in device memory and compare both with the oracle (the column must be
    attached); ``mask``: bool [N].  Returns the host outputs."""
    if want is None:
        want = mc.expected(Q, offs, V, groups, n_slots, k, metric, mask)
    words = None if mask is None else mc.bitmap_words(mask)
    what = f"{what} ({metric}, N {V.shape[0]}, D {V.shape[1]}, slots {n_slots}, k {k})"
    code, got = _call(ix, Q, offs, n_slots, k, words)
    assert code == 0, f"status {code} {what}: {ix._lib.vdb_last_error()}"
    _same(got, want, what + " host")
    if device:
        _same(_call_device(ix, Q, offs, n_slots, k, words), want, what + " device")
    return got


def _candidates(groups, n_slots, mask=None):
    g = np.asarray(groups)
    return int(np.unique(g[mc.eligible(g, n_slots, mask)]).size)


# =============================================================================
# shapes
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", mc.DIMS)
def test_row_lengths_and_counts(vdb, indexes, d, metric):
    """Every piece form at every row count: a partial trip, a partial word, a chunk and a row, several
    chunks; sets of 0, 1, 2 and 5 vectors in one call."""
    offs = mc.offsets_of([1, 0, 2, 5])
    for n in mc.ROWS if d <= 768 else mc.ROWS[:3]:
        V, Q = mc.corpus(n, d, 0, 8)
        ix = indexes(V, metric)
        g = mc.layout("random", n)
        ix.set_groups(g)
        slots = mc.slots_of("random", g)
        got = _check(ix, V, Q, offs, g, slots, slots, metric, what="shapes", device=n in (37, 1300))
        assert (got[1][1] == -1).all() and np.isneginf(got[2][1]).all() and (got[0][1] == 0).all()  # the empty set


@pytest.mark.parametrize("metric", METRICS)
def test_set_lengths_and_independent_sets(vdb, indexes, metric):
    """Sets of 0, 1, 2, 33 and 64 vectors in one call (100 sub-queries: two scan blocks), and every
    set alone gives the rows it gave among its neighbours."""
    n, d = 513, 8
    lengths = list(mc.SET_LENGTHS)
    V, Q = mc.corpus(n, d, 2, sum(lengths))
    ix = indexes(V, metric)
    g = mc.layout("random", n)
    ix.set_groups(g)
    slots = mc.slots_of("random", g)
    offs = mc.offsets_of(lengths)
    together = _check(ix, V, Q, offs, g, slots, 5, metric, what="set lengths")
    for s, m in enumerate(lengths):
        code, alone = _call(ix, Q[offs[s]:offs[s + 1]], mc.offsets_of([m]), slots, 5)
        assert code == 0
        _same(alone, tuple(x[s:s + 1] for x in together), f"set {s} alone")
    # the same sets in another order, with gaps between them
    order = [3, 0, 4, 1, 2]
    Q2 = np.concatenate([Q[offs[s]:offs[s + 1]] for s in order])
    again = _check(ix, V, Q2, mc.offsets_of([lengths[s] for s in order]), g, slots, 5, metric, what="reordered")
    _same(again, tuple(x[order] for x in together), "reordered sets")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [8, 768])
def test_a_set_straddles_two_query_blocks(vdb, indexes, d, metric):
    n_sub, lengths = mc.straddle_sets(d)
    assert n_sub == {8: 65, 768: 43}[d]
    V, Q = mc.corpus(37, d, 1, n_sub)
    ix = indexes(V, metric)
    g = mc.layout("random", 37)
    ix.set_groups(g)
    slots = mc.slots_of("random", g)
    _check(ix, V, Q, mc.offsets_of(lengths), g, slots, slots, metric, what="straddle")


# =============================================================================
# group layouts, masks, k
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", mc.LAYOUTS)
def test_group_layouts(vdb, indexes, name, metric):
    n, d = 1300, 8
    V, Q = mc.corpus(n, d, 0, 8)
    ix = indexes(V, metric)
    g = mc.layout(name, n)
    ix.set_groups(g)
    slots = mc.slots_of(name, g)
    before = {s: ix.stat(s) for s in STATS}
    k = min(max(_candidates(g, slots), 1), 128)
    _check(ix, V, Q, mc.offsets_of([1, 2, 5]), g, slots, k, metric, what=name)
    # two successful calls (host, device), three sets each; the skipped rows counted once per call
    past = int((g.astype(np.int64) >= slots).sum())
    assert (past > 0) == (name == "past_slots")
    assert ix.stat("maxsim_skipped_rows") - before["maxsim_skipped_rows"] == 2 * past
    assert ix.stat("maxsim_searches") - before["maxsim_searches"] == 2
    assert ix.stat("maxsim_sets") - before["maxsim_sets"] == 6
    assert ix.stat("maxsim_bad_sets") == before["maxsim_bad_sets"]


@pytest.mark.parametrize("metric", METRICS)
def test_more_slots_than_one_rank_segment(vdb, indexes, metric):
    """Sparse ids over 5 000 slots: five rank segments per set and the last-workgroup merge, k below,
    at and above a segment's share; twice in a row on one workspace (the counters are left at zero)."""
    n, d = 1300, 8
    V, Q = mc.corpus(n, d, 0, 8)
    ix = indexes(V, metric)
    g = mc.sparse_layout(n)  # one larger group among singletons
    slots = mc.SPARSE_SLOTS
    ix.set_groups(g)
    offs = mc.offsets_of([3, 0, 5])
    for k in (1, 100, 128):
        want = mc.expected(Q, offs, V, g, slots, k, metric)
        first = _check(ix, V, Q, offs, g, slots, k, metric, what="segments", want=want, device=False)
        second = _check(ix, V, Q, offs, g, slots, k, metric, what="segments again", want=want, device=k == 128)
        _same(first, second, "two calls back to back")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("mask_name", mc.MASKS)
@pytest.mark.parametrize("name", ["blocks", "random"])
def test_masks(vdb, indexes, name, mask_name, metric):
    n, d = 1300, 8
    V, Q = mc.corpus(n, d, 0, 8)
    ix = indexes(V, metric)
    g = mc.layout(name, n)
    ix.set_groups(g)
    slots = mc.slots_of(name, g)
    mask, dropped = mc.mask_of(mask_name, g, slots)
    k = slots
    sc, gr, sm = _check(ix, V, Q, mc.offsets_of([1, 2, 5]), g, slots, k, metric, mask=mask, what=f"{name} {mask_name}")
    if dropped is not None:
        assert dropped not in gr.tolist()[0] and (gr[:, -1] == -1).all()
    if mask_name == "nothing":
        assert (gr == -1).all() and np.isneginf(sm).all() and (sc == 0).all()


@pytest.mark.parametrize("metric", METRICS)
def test_k_at_and_around_the_candidates(vdb, indexes, metric):
    n, d = 513, 100
    V, Q = mc.corpus(n, d, 0, 8)
    ix = indexes(V, metric)
    g = mc.layout("some_negative", n)
    ix.set_groups(g)
    slots = mc.slots_of("some_negative", g)
    c = _candidates(g, slots)
    for k in (1, c, c + 1, 128):
        sc, gr, sm = _check(ix, V, Q, mc.offsets_of([2, 5]), g, slots, k, metric, what="k", device=k in (1, 128))
        assert ((gr >= 0).sum(axis=1) == min(k, c)).all()
        assert (gr[:, c:] == -1).all() and np.isneginf(sm[:, c:]).all() and (sc[:, c:] == 0).all()
    # without out_sums
    code, (sc2, gr2, none) = _call(ix, Q, mc.offsets_of([2, 5]), slots, c, with_sums=False)
    assert code == 0 and none is None
    _same((sc2, gr2), mc.expected(Q, mc.offsets_of([2, 5]), V, g, slots, c, metric)[:2], "no sums")
    _same(_call_device(ix, Q, mc.offsets_of([2, 5]), slots, c, with_sums=False)[:2], (sc2, gr2), "no sums, device")


# =============================================================================
# ties, zeros, the grouped search
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_duplicated_documents_put_the_lower_id_first(vdb, indexes, metric):
    V, Q, g, (a, b) = mc.tie_case()
    ix = indexes(V, metric)
    ix.set_groups(g)
    slots = int(g.max()) + 1
    sc, gr, sm = _check(ix, V, Q, mc.offsets_of([1, 2, 3]), g, slots, 4, metric, what="tie")
    for s in range(3):
        pa = gr[s].tolist().index(a)
        assert gr[s, pa + 1] == b and _bits(sm[s])[pa] == _bits(sm[s])[pa + 1]


def test_a_query_equal_to_a_stored_row_sums_plus_zero(vdb, indexes):
    V, Q, g, row = mc.exact_match_case()
    ix = indexes(V, "euclidean")
    ix.set_groups(g)
    slots = mc.slots_of("modulo", g)
    sc, gr, sm = _check(ix, V, Q, mc.offsets_of([1, 3]), g, slots, slots, "euclidean", what="exact match")
    assert gr[0, 0] == g[row] and _bits(sm[0])[0] == 0 and _bits(sc[0])[0] == 0  # +0.0, not -0.0


@pytest.mark.parametrize("metric", METRICS)
def test_one_vector_sets_against_the_grouped_search(vdb, indexes, metric):
    n, d = 513, 100
    V, Q = mc.corpus(n, d, 0, 8)
    ix = indexes(V, metric)
    g = mc.layout("some_negative", n)
    ix.set_groups(g)
    slots = mc.slots_of("some_negative", g)
    k = _candidates(g, slots)
    scores, idx, grp, keys = ix.search_groups(Q, k, with_keys=True)
    code, (sc, gr, sm) = _call(ix, Q, np.arange(Q.shape[0] + 1), slots, k)
    assert code == 0
    np.testing.assert_array_equal(gr, grp)
    np.testing.assert_array_equal(_bits(sm), _bits(keys + 0.0))


# =============================================================================
# precision, memory kinds, stats
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_same_bytes_for_every_precision_and_no_search_stat_moves(vdb, indexes, metric):
    n, d = 1300, 100
    V, Q = mc.corpus(n, d, 0, 8)
    g = mc.layout("random", n)
    slots = mc.slots_of("random", g)
    offs = mc.offsets_of([1, 2, 5])
    want = mc.expected(Q, offs, V, g, slots, slots, metric)
    for precision in ("fp32", "bf16x3", "i8", "auto"):
        ix = indexes(V, metric, precision)
        ix.set_groups(g)
        before = {s: ix.stat(s) for s in STILL}
        _check(ix, V, Q, offs, g, slots, slots, metric, what=precision, want=want)
        assert {s: ix.stat(s) for s in STILL} == before, precision


# =============================================================================
# errors and bad device input
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
def test_errors_before_any_launch(vdb, indexes, metric):
    n, d = 37, 8
    V, Q = mc.corpus(n, d, 0, 8)
    ix = vdb.NativeIndex(d, metric)
    ix.add(V)
    offs = mc.offsets_of([3, 5])
    g = mc.layout("random", n)
    for mem in (0, 1):  # (nothing is read before these are refused, so host pointers do for mem 1)
        stats = {s: ix.stat(s) for s in STATS}
        assert _call(ix, Q, offs, 7, 3, mem=mem)[0] == VDB_ERR_INVALID and b"group column" in ix._lib.vdb_last_error()
        ix.set_groups(g)
        for k in (0, -1, 129):
            assert _call(ix, Q, offs, 7, k, mem=mem)[0] == VDB_ERR_INVALID, k
        for slots in (0, -3, (1 << 27) // 8 + 1, 2 ** 31 - 1):
            assert _call(ix, Q, offs, slots, 3, mem=mem)[0] == VDB_ERR_INVALID, slots
        assert _call(ix, Q, offs, 7, 3, n_sub=-1, mem=mem)[0] == VDB_ERR_INVALID
        assert _call(ix, Q, offs, 7, 3, n_sets=-1, mem=mem)[0] == VDB_ERR_INVALID
        for null in ("queries", "offsets", "scores", "groups"):
            assert _call(ix, Q, offs, 7, 3, mem=mem, null=(null,))[0] == VDB_ERR_INVALID, null
        assert {s: ix.stat(s) for s in STATS} == stats
        ix.set_groups(None)
    assert _call(ix, Q, offs, 7, 3, mem=2)[0] == VDB_ERR_INVALID
    ix.set_groups(g)
    # host memory: the offsets and the queries
    for bad in ([0, 5, 4], [0, 3, 9], [-1, 8], [1, 0, 8]):
        assert _call(ix, Q, np.asarray(bad), 7, 3)[0] == VDB_ERR_INVALID, bad
    Qbig = np.tile(Q, (9, 1))
    assert _call(ix, Qbig, np.asarray([0, 65, 72]), 7, 3)[0] == VDB_ERR_INVALID and b"64" in ix._lib.vdb_last_error()
    assert _call(ix, Qbig, np.asarray([0, 64, 72]), 7, 3)[0] == 0
    for bad in (np.nan, np.inf, -np.inf):
        Qn = Q.copy()
        Qn[5, 3] = bad
        assert _call(ix, Qn, offs, 7, 3)[0] == VDB_ERR_NONFINITE
    assert ix.stat("maxsim_searches") == 1 and ix.stat("maxsim_sets") == 2 and ix.stat("maxsim_bad_sets") == 0
    # the wrapper raises ValueError for them; n_sets == 0 is fine
    with pytest.raises(ValueError):
        ix.search_maxsim([Q[:2]], 7, 0)
    with pytest.raises(ValueError):
        ix.search_maxsim([np.tile(Q, (9, 1))[:65]], 7, 3)
    with pytest.raises(ValueError):
        ix.search_maxsim([Q[:2, :5]], 7, 3)
    assert _call(ix, Q, np.zeros(1, np.int64), 7, 3)[0] == 0
    # add, remove and clear drop the column
    ix.add(V[:1])
    assert _call(ix, Q, offs, 7, 3)[0] == VDB_ERR_INVALID
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_device_memory_bad_sets_are_counted_and_neighbours_unaffected(vdb, indexes, metric):
    n, d = 513, 8
    V, Q = mc.corpus(n, d, 2, 100)
    ix = indexes(V, metric)
    g = mc.layout("random", n)
    ix.set_groups(g)
    slots = mc.slots_of("random", g)
    k = 4
    good = mc.expected(Q, np.asarray([0, 3, 3, 10, 20]), V, g, slots, k, metric)
    # sets: good [0,3) | decreasing | good [3,10)... written as raw offset pairs through one array
    offs = np.asarray([0, 3, 2, 10, 100, 170, 20, 20], np.int64)
    #        set 0 [0,3) ok; 1 [3,2) bad; 2 [2,10) ok; 3 [10,100) too long; 4 [100,170) past n_sub; 5 [170,20) bad; 6 [20,20) empty
    before = ix.stat("maxsim_bad_sets")
    sc, gr, sm = _call_device(ix, Q, offs, slots, k)
    assert ix.stat("maxsim_bad_sets") - before == 4
    _same((sc[0:1], gr[0:1], sm[0:1]), tuple(x[0:1] for x in good), "set 0")
    _same((sc[2:3], gr[2:3], sm[2:3]), mc.expected(Q, np.asarray([2, 10]), V, g, slots, k, metric), "set 2")
    for s in (1, 3, 4, 5, 6):
        assert (gr[s] == -1).all() and np.isneginf(sm[s]).all() and (sc[s] == 0).all(), s
    # negative offsets and ones far outside
    offs = np.asarray([-5, 4, 2 ** 62, -2 ** 62, 8], np.int64)
    sc, gr, sm = _call_device(ix, Q, offs, slots, k)
    assert (gr == -1).all() and ix.stat("maxsim_bad_sets") - before == 8


def test_empty_index_and_call_without_sub_queries(vdb):
    ix = vdb.NativeIndex(8, "cosine")
    ix.set_groups(np.zeros(0, np.int32))
    Q = np.ones((3, 8), np.float32)
    code, (sc, gr, sm) = _call(ix, Q, np.asarray([0, 1, 3]), 4, 5)
    assert code == 0 and (gr == -1).all() and np.isneginf(sm).all() and (sc == 0).all()
    sc, gr, sm = _call_device(ix, Q, np.asarray([0, 1, 3]), 4, 5)
    assert (gr == -1).all() and np.isneginf(sm).all() and (sc == 0).all()
    ix.add(np.eye(8, dtype=np.float32))
    ix.set_groups(np.arange(8) % 4)
    code, (sc, gr, sm) = _call(ix, np.zeros((0, 8), np.float32), np.zeros(4, np.int64), 4, 5)
    assert code == 0 and (gr == -1).all() and np.isneginf(sm).all() and (sc == 0).all()
    assert ix.stat("maxsim_searches") == 3 and ix.stat("maxsim_sets") == 7 and ix.stat("searches") == 0
    ix.close()

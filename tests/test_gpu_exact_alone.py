"""The exact path, the list merge and the top-k operator, each alone at its edges.

Every result is either certified by the finish or comes from the exact path (exact_scan_kernel,
merge_block / merge_lists_kernel, finalize_kernel or the fused tail): the safety net behind every
candidate pass.  These tests drive it directly -- force_exact, k > 200, queries that cannot certify
-- and the merge kernel and the top-k operator with synthetic input, at the sizes where their loops
and branches change (tests/_exact_cases.py; tests/test_exact_precondition.py checks the fixtures
on the CPU).

Every comparison is bit for bit: indices, fp64 keys and fp32 scores against ref_cpu.exact_search,
merges against ref_cpu.merge_topk, top-k indices against a stable argsort.  Every output buffer
holds a poison value before each call (index -7, key and score NaN), so a slot nobody wrote cannot
pass; the "few" cases run right after a call with full lists, so that recycled scratch holds
valid-looking entries.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _exact_cases as ec  # noqa: E402
from oracle import ref_cpu  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


@pytest.fixture(scope="module")
def cus(vdb):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _poisoned(B, k):
    import torch
    return (torch.full((B, k), float("nan"), dtype=torch.float32, device="cuda"),
            torch.full((B, k), ec.POISON_IDX, dtype=torch.int64, device="cuda"),
            torch.full((B, k), float("nan"), dtype=torch.float64, device="cuda"))


def _host(bufs):
    return tuple(b.cpu().numpy() for b in bufs)


def _assert_same(got, want, what=""):
    (s, i, k), (es, ei, ek) = got, want
    np.testing.assert_array_equal(i, ei, err_msg=f"indices {what}")
    np.testing.assert_array_equal(k, ek, err_msg=f"keys {what}")
    np.testing.assert_array_equal(s, es, err_msg=f"scores {what}")


# =============================================================================
# A. the merge kernel alone
# =============================================================================
def _merge(vdb, K, I, k_out, metric):
    import torch
    G, B, k_in = K.shape
    kd, idd = torch.from_numpy(K).cuda(), torch.from_numpy(I).cuda()
    bufs = _poisoned(B, k_out)
    vdb.merge_topk_device(kd.data_ptr(), idd.data_ptr(), G, B, k_in, k_out, metric, bufs[0].data_ptr(),
                          bufs[1].data_ptr(), bufs[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return _host(bufs)


def _check_merge(vdb, K, I, k_out, metric, what=""):
    _assert_same(_merge(vdb, K, I, k_out, metric), ec.merge_expected(K, I, k_out, metric), what)


@pytest.mark.parametrize("c", ec.FEW_VALID, ids=[ec.case_id(c) for c in ec.FEW_VALID])
def test_merge_of_few_valid_entries(vdb, c):
    """Fewer valid entries than KP, right after a merge of the same shape with full lists: the
    first min(c, k_out) slots are the merge and every later one is id -1, key -inf, score 0."""
    metric = ec.BOTH[c["seed"] % 2]
    G, k_in, k_out = c["G"], c["k_in"], c["k_out"]
    Kf, If = ec.random_lists(G, k_in, (G * k_in,) * 3, c["seed"] + 1)
    _check_merge(vdb, Kf, If, k_out, metric, "full lists")
    K, I = ec.random_lists(G, k_in, c["counts"], c["seed"])
    got = _merge(vdb, K, I, k_out, metric)
    _assert_same(got, ec.merge_expected(K, I, k_out, metric))
    for b, n in enumerate(c["counts"]):
        assert (got[1][b, n:] == -1).all() and (got[2][b, n:] == -np.inf).all() and (got[0][b, n:] == 0).all()


@pytest.mark.parametrize("metric", ec.BOTH)
@pytest.mark.parametrize("c", ec.LIST_COUNTS + ec.K_SIZES, ids=[ec.case_id(c) for c in ec.LIST_COUNTS + ec.K_SIZES])
def test_merge_list_counts_and_k(vdb, c, metric):
    K, I = ec.random_lists(c["G"], c["k_in"], c["counts"], c["seed"])
    _check_merge(vdb, K, I, c["k_out"], metric)


@pytest.mark.parametrize("metric", ec.BOTH)
def test_merge_ties(vdb, metric):
    for G, k_in, contiguous in ((64, 32, False), (64, 32, True), (64, 64, True)):
        K, I = ec.all_equal_lists(G, k_in, contiguous)
        got = _merge(vdb, K, I, k_in, metric)
        _assert_same(got, ec.merge_expected(K, I, k_in, metric), f"all equal {G} x {k_in}")
        np.testing.assert_array_equal(got[1][0], np.sort(I[:, 0].ravel())[:k_in])  # the lowest ids
    K, I = ec.tie_block_lists()
    _check_merge(vdb, K, I, 25, metric, "tie block")


@pytest.mark.parametrize("metric", ec.BOTH)
@pytest.mark.parametrize("G,k", [(32, 32), (64, 64), (512, 512), (33, 32)])
def test_merge_when_the_heads_are_the_answer(vdb, metric, G, k):
    """The head threshold at its tightest: exactly KP entries are not worse than T."""
    K, I = ec.heads_are_the_answer(G, k)
    got = _merge(vdb, K, I, k, metric)
    _assert_same(got, ec.merge_expected(K, I, k, metric))
    if G == k:
        for b in range(2):
            np.testing.assert_array_equal(np.sort(got[1][b]), np.sort(I[:, b, 0]))  # the heads, all of them


# =============================================================================
# B. the exact scan
# =============================================================================
def _search(vdb, ix, Q, k, words=None, index_offset=0):
    """A host-memory search into poisoned buffers."""
    q = np.ascontiguousarray(Q, dtype=np.float32)
    B = q.shape[0]
    s = np.full((B, k), np.nan, np.float32)
    i = np.full((B, k), ec.POISON_IDX, np.int64)
    kk = np.full((B, k), np.nan, np.float64)
    if words is not None:
        words = np.ascontiguousarray(words, dtype=np.uint32)
    vdb._check(ix._lib.vdb_index_search(ix._h, q.ctypes.data, B, int(k), words.ctypes.data if words is not None else None,
                                        vdb.MEM_HOST, s.ctypes.data, i.ctypes.data, kk.ctypes.data, int(index_offset),
                                        None))
    return s, i, kk


def _index(vdb, V, metric, force=1, precision="bf16x3"):
    ix = vdb.NativeIndex(V.shape[1], metric, precision=precision)
    if force:
        ix.set_param("force_exact", 1)
    ix.add(V)
    assert ix.count() == V.shape[0]
    return ix


def _exact_search_checked(vdb, ix, V, Q, k, metric, mask=None, words=None, what=""):
    """One search that must take the exact path for every query, against the oracle."""
    before = ix.stat("fallback_queries")
    got = _search(vdb, ix, Q, k, words)
    want = ref_cpu.exact_search(Q, V, k, metric, row_mask=mask)
    _assert_same(got, want, what)
    assert ix.stat("fallback_queries") - before == Q.shape[0], "the exact path did not run for every query"
    assert ix.stat("inconsistent_queries") == 0
    return got, want


@pytest.mark.parametrize("c", ec.SCAN_CASES, ids=[ec.scan_id(c) for c in ec.SCAN_CASES])
def test_exact_scan_every_query(vdb, cus, c):
    V, Q, mask, words = ec.scan_data(c, cus)
    ix = _index(vdb, V, c["metric"], c["force"])
    _exact_search_checked(vdb, ix, V, Q, c["k"], c["metric"], mask, words)
    ix.close()


@pytest.mark.parametrize("metric", ec.BOTH)
@pytest.mark.parametrize("N,k", ec.FEW_UNMASKED)
def test_fewer_rows_than_k(vdb, metric, N, k):
    """A search with full lists (3000 rows), then the same index with N < k rows: the slots past N
    are -1 / 0 / -inf, not what the workspace held."""
    ix = _index(vdb, ec.rows(3000, 24, 3), metric)
    Q = ec.rows(3, 24, N + 1)
    _exact_search_checked(vdb, ix, ec.rows(3000, 24, 3), Q, k, metric, what="full lists")
    ix.clear()
    V = ec.rows(N, 24, N)
    ix.add(V)
    (s, i, kk), _ = _exact_search_checked(vdb, ix, V, Q, k, metric)
    assert (i[:, :N] >= 0).all() and (i[:, N:] == -1).all() and (s[:, N:] == 0).all() and (kk[:, N:] == -np.inf).all()
    ix.close()


@pytest.fixture(scope="module")
def few_index(vdb):
    V, Q = ec.rows(ec.FEW_N, ec.FEW_D, 5), ec.rows(3, ec.FEW_D, 6)
    made = {}

    def get(metric):
        if metric not in made:
            made[metric] = _index(vdb, V, metric)
        return made[metric], V, Q
    yield get
    for ix in made.values():
        ix.close()


@functools.lru_cache(maxsize=None)
def _few_full_oracle(metric):
    V, Q = ec.rows(ec.FEW_N, ec.FEW_D, 5), ec.rows(3, ec.FEW_D, 6)
    return ref_cpu.exact_search(Q, V, 1024, metric)


@pytest.mark.parametrize("metric", ec.BOTH)
@pytest.mark.parametrize("k", ec.FEW_K)
@pytest.mark.parametrize("eligible", ec.FEW_ELIGIBLE)
def test_fewer_eligible_rows_than_k(vdb, few_index, metric, eligible, k):
    """An unmasked search at the same k (full lists in the workspace), then a mask that leaves
    `eligible` of 9000 rows: min(k, eligible) results, the rest -1 / 0 / -inf."""
    ix, V, Q = few_index(metric)
    _assert_same(_search(vdb, ix, Q, k), tuple(a[:, :k] for a in _few_full_oracle(metric)), "full lists")
    mask = ec.few_mask(eligible)
    (s, i, kk), _ = _exact_search_checked(vdb, ix, V, Q, k, metric, mask, ec.mask_words(mask))
    n = min(k, eligible)
    assert (i[:, :n] >= 0).all() and (i[:, n:] == -1).all() and (s[:, n:] == 0).all() and (kk[:, n:] == -np.inf).all()


@pytest.mark.parametrize("metric", ec.BOTH)
def test_ties_across_a_range_boundary(vdb, cus, metric):
    V, Q, rpw = ec.boundary_ties(1500, 24, cus)
    ix = _index(vdb, V, metric)
    (_, i, _), _ = _exact_search_checked(vdb, ix, V, Q, 10, metric)
    np.testing.assert_array_equal(i[0, :5], np.arange(rpw - 2, rpw + 3))
    ix.close()


@pytest.mark.parametrize("metric", ec.BOTH)
@pytest.mark.parametrize("k", [10, 40])
def test_more_tied_rows_than_the_merge_buffer(vdb, metric, k):
    """2100 copies of the query's row over 16384 rows: the answer is the k lowest copies.  (At
    k = 40 more than 1024 entries survive the head threshold: the merge's stream path.)"""
    V, Q, pos = ec.spread_copies()
    ix = _index(vdb, V, metric)
    (_, i, _), _ = _exact_search_checked(vdb, ix, V, Q, k, metric)
    np.testing.assert_array_equal(i[0], pos[:k])
    ix.close()


def test_cosine_zero_rows_and_zero_query(vdb):
    V, Q = ec.zero_rows()
    ix = _index(vdb, V, "cosine")
    (_, i, kk), _ = _exact_search_checked(vdb, ix, V, Q, 10, "cosine")
    np.testing.assert_array_equal(i[0], np.arange(10))  # every key 0: row order
    assert (kk[0] == 0).all()
    ix.close()


@pytest.mark.parametrize("metric", ec.BOTH)
def test_chunked_adds_across_capacity_doublings(vdb, metric):
    V, Q = ec.rows(1401, 24, 61, "normal"), ec.rows(3, 24, 62, "normal")
    ix = vdb.NativeIndex(24, metric, precision="bf16x3")
    ix.set_param("force_exact", 1)
    for a, b in ((0, 700), (700, 1400), (1400, 1401)):
        ix.add(V[a:b])
        assert ix.count() == b
        _exact_search_checked(vdb, ix, V[:b], Q, 10, metric, what=f"{b} rows")
    ix.close()


@pytest.mark.parametrize("metric", ec.BOTH)
def test_index_offset_above_32_bits(vdb, metric):
    off = (1 << 32) + 12345
    V, Q = ec.rows(1500, 24, 63), ec.rows(3, 24, 64)
    ix = _index(vdb, V, metric)
    mask = ec.few_mask(40)[:1500]
    mask[:7] = True
    for m, k in ((None, 10), (mask, 300)):
        before = ix.stat("fallback_queries")
        got = _search(vdb, ix, Q, k, None if m is None else ec.mask_words(m), index_offset=off)
        es, ei, ek = ref_cpu.exact_search(Q, V, k, metric, row_mask=m)
        _assert_same(got, (es, np.where(ei >= 0, ei + off, -1), ek))
        assert ix.stat("fallback_queries") - before == 3
    ix.close()


@pytest.mark.parametrize("metric", ec.BOTH)
def test_two_small_shards_searched_with_a_larger_k(vdb, metric):
    """The shard set's merge (stream-ordered scratch): two shards of 30 rows at k = 100, after the
    same search over two shards of 1500 rows."""
    import torch
    Q = ec.rows(3, 24, 72)
    qd = torch.from_numpy(Q).cuda()
    for N in (3000, 60):
        V = ec.rows(N, 24, 71)
        sh = vdb.NativeShards(24, metric, [0, 0])
        sh.add(V)
        assert sorted(sh.shard_counts()) == [N // 2, N // 2]
        bufs = _poisoned(3, 100)
        torch.cuda.synchronize()
        sh.search_device(qd.data_ptr(), 3, 100, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                         stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = _host(bufs)
        _assert_same(got, ref_cpu.exact_search(Q, V, 100, metric), f"{N} rows")
        sh.close()
    assert (got[1][:, 60:] == -1).all()


# ---- (ii) the flagged subset of a host-memory search-------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_oracle(metric, masked):
    V, Q, mask = ec.host_flagged()
    return ref_cpu.exact_search(Q, V, max(ec.HOST_K), metric, row_mask=mask if masked else None)


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("k", ec.HOST_K)
@pytest.mark.parametrize("precision", ["bf16x3", "i8"])
@pytest.mark.parametrize("metric", ec.BOTH)
def test_flagged_subset_of_a_host_search(vdb, metric, precision, k, masked):
    """Queries 1, 5 and 6 of 9 tie on 320 rows and cannot certify; the other six must (planted
    gaps): run_exact serves a non-contiguous query list, and exactly those three per search."""
    V, Q, mask = ec.host_flagged()
    ix = _index(vdb, V, metric, force=0, precision=precision)
    words = ec.mask_words(mask) if masked else None
    want = tuple(a[:, :k] for a in _host_oracle(metric, masked))
    for rep in range(2):
        before = ix.stat("fallback_queries")
        _assert_same(_search(vdb, ix, Q, k, words), want, f"search {rep}")
        assert ix.stat("fallback_queries") - before == len(ec.HOST_FLAGGED)
    assert ix.stat("inconsistent_queries") == 0
    ix.close()


# ---- (iii) the device-gated fused tail ---------------------------------------------------------------
def _device_searches(ix, Q, k, words=None, n=3):
    """n searches queued back to back on a side stream, one synchronise."""
    import torch
    qd = torch.from_numpy(np.array(Q, dtype=np.float32)).cuda()
    md = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda() if words is not None else None
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(n):
        bufs = _poisoned(Q.shape[0], k)
        torch.cuda.synchronize()  # (the poison fill runs on torch's stream)
        outs.append(bufs)
    for bufs in outs:
        ix.search_device(qd.data_ptr(), Q.shape[0], k, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                         mask_ptr=md.data_ptr() if md is not None else 0, stream=st.cuda_stream)
    torch.cuda.synchronize()
    return [_host(b) for b in outs]


@functools.lru_cache(maxsize=None)
def _gated_oracle(cus, B, n_flag, metric, masked, k=200):
    V, Q, _ = ec.gated(cus, B, n_flag)
    return ref_cpu.exact_search(Q, V, k, metric, row_mask=ec.gated_mask(V.shape[0]) if masked else None)


@functools.lru_cache(maxsize=None)
def _gated_ties(cus, B, metric, masked):
    V, Q, _ = ec.gated(cus, B, B)
    return ec.tied_with_best(Q, V, metric, ec.gated_mask(V.shape[0]) if masked else None)


@pytest.fixture(scope="module")
def gated_index(vdb, cus):
    made = {}

    def get(B, n_flag, metric):
        key = (B, n_flag, metric)
        if key not in made:
            V, Q, flagged = ec.gated(cus, B, n_flag)
            made[key] = _index(vdb, V, metric, force=0)
        return made[key]
    yield get
    for ix in made.values():
        ix.close()


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("k", [10, 100, 200])
@pytest.mark.parametrize("metric", ec.BOTH)
def test_gated_tail_more_flagged_than_slots(vdb, cus, gated_index, metric, k, masked):
    """40 queries, each tied on 320 rows spread over every workgroup's range: all flagged, ten
    rounds over the four gate slots, three searches in flight."""
    B = 40
    V, Q, flagged = ec.gated(cus, B, B)
    mask = ec.gated_mask(V.shape[0]) if masked else None
    assert (_gated_ties(cus, B, metric, masked) > 256).all()
    ix = gated_index(B, B, metric)
    want = tuple(a[:, :k] for a in _gated_oracle(cus, B, B, metric, masked))
    before = ix.stat("fallback_queries")
    for n, got in enumerate(_device_searches(ix, Q, k, ec.mask_words(mask) if masked else None)):
        _assert_same(got, want, f"search {n}")
    assert ix.stat("fallback_queries") - before == 3 * B
    assert ix.stat("inconsistent_queries") == 0


@pytest.mark.parametrize("n_flag", [1, 4, 5])
@pytest.mark.parametrize("metric", ec.BOTH)
def test_gated_tail_flagged_counts_around_the_slots(vdb, cus, gated_index, metric, n_flag):
    B = 16
    V, Q, flagged = ec.gated(cus, B, n_flag)
    ix = gated_index(B, n_flag, metric)
    want = tuple(a[:, :10] for a in _gated_oracle(cus, B, n_flag, metric, False, 10))
    before = ix.stat("fallback_queries")
    for n, got in enumerate(_device_searches(ix, Q, 10)):
        _assert_same(got, want, f"search {n}")
    assert ix.stat("fallback_queries") - before == 3 * n_flag
    assert ix.stat("inconsistent_queries") == 0


@pytest.mark.parametrize("metric", ec.BOTH)
def test_gated_tail_single_workgroup(vdb, metric):
    V, Q, pos = ec.single_wg()
    ix = _index(vdb, V, metric, force=0)
    want = ref_cpu.exact_search(Q, V, 10, metric)
    np.testing.assert_array_equal(want[1], np.tile(pos[:10], (Q.shape[0], 1)))
    for n, got in enumerate(_device_searches(ix, Q, 10)):
        _assert_same(got, want, f"search {n}")
    assert ix.stat("fallback_queries") == 3 * Q.shape[0]
    ix.close()


@pytest.mark.parametrize("metric", ec.BOTH)
def test_device_search_with_fewer_eligible_rows_than_k(vdb, cus, gated_index, metric):
    """A full search at k = 100, then a mask that leaves 50 rows: whichever path answers, the
    results equal the oracle and the tail is -1."""
    B = 16
    V, Q, flagged = ec.gated(cus, B, 4)
    ix = gated_index(B, 4, metric)
    full = ref_cpu.exact_search(Q, V, 100, metric)
    _assert_same(_device_searches(ix, Q, 100, n=1)[0], full, "full lists")
    mask = np.zeros(V.shape[0], bool)
    mask[np.random.default_rng(9).permutation(V.shape[0])[:50]] = True
    want = ref_cpu.exact_search(Q, V, 100, metric, row_mask=mask)
    for n, got in enumerate(_device_searches(ix, Q, 100, ec.mask_words(mask))):
        _assert_same(got, want, f"search {n}")
        assert (got[1][:, :50] >= 0).all() and (got[1][:, 50:] == -1).all()
    assert ix.stat("inconsistent_queries") == 0


# =============================================================================
# C. the top-k operator
# =============================================================================
def _topk_check(vdb, s, ks, largest):
    import torch
    rows_, n = s.shape
    sd = torch.from_numpy(s).cuda()
    ref = ec.topk_reference(s, max(ks), largest)
    for k in ks:
        oi = torch.full((rows_, k), ec.POISON_IDX, dtype=torch.int64, device="cuda")
        ov = torch.full((rows_, k), float("nan"), dtype=torch.float32, device="cuda")
        vdb.topk_scores_device(sd.data_ptr(), rows_, n, k, largest, oi.data_ptr(), ov.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        idx, val = oi.cpu().numpy(), ov.cpu().numpy()
        np.testing.assert_array_equal(idx, ref[:, :k], err_msg=f"k={k}")
        np.testing.assert_array_equal(val.view(np.uint32), np.take_along_axis(s, ref[:, :k], axis=1).view(np.uint32),
                                      err_msg=f"values k={k}")


TOPK_SHAPES = [(r, n) for n in ec.TOPK_N for r in (1, 3) if not (r == 3 and n > 4 * ec.TOPK_CHUNK)]


@pytest.mark.parametrize("largest", [True, False], ids=["largest", "smallest"])
@pytest.mark.parametrize("rows_,n", TOPK_SHAPES)
def test_topk_sizes(vdb, rows_, n, largest):
    _topk_check(vdb, ec.topk_rows(rows_, n, 7 * n + rows_), ec.topk_ks(n), largest)


@pytest.mark.parametrize("largest", [True, False], ids=["largest", "smallest"])
def test_topk_special_values(vdb, largest):
    s, ks = ec.topk_special(largest)
    for b, k in enumerate(ks):
        _topk_check(vdb, np.ascontiguousarray(s[b:b + 1]), [k], largest)
    _topk_check(vdb, s, [33], largest)  # the four rows in one call
    s, k = ec.topk_small_special(largest)
    _topk_check(vdb, s, [k], largest)
    ref = ec.topk_reference(s, k, largest)
    assert ref[0, 0] == 40 and ref[0, -1] == 12  # the winning infinity first, the NaN last

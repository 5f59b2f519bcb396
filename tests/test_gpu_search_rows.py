"""Search over explicit row-id lists (include/vdb.h vdb_index_search_rows; csrc/vdb_subset.hip).

The contract is that of a masked search whose row_mask is exactly the list's set, bit for bit:
every case compares indices, fp64 keys and fp32 scores with BOTH
``oracle.ref_cpu.exact_search(..., row_mask=<the list as a bool mask>)`` and
``NativeIndex.search(..., row_mask=<the list as a bitmap>, with_keys=True)`` on the same index.
No tolerance appears anywhere.

Shapes are the smallest at which the kernel can go wrong: dims that leave pad columns (1, 33,
100), exactly one 256-dim piece and one piece plus 4 dims (256, 260), three pieces (768) and six
(1536: the second trip of exact_key's 4-piece loop, and the 8-piece form of the row-list kernel);
list lengths around k and around the plan's chunk (csrc/vdb_subset_plan.h kSubsetChunk = 64
positions, 16 per wave); one, two and seven workgroups per query.
"""
import functools
import threading

import numpy as np
import pytest

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

CHUNK = 64  # csrc/vdb_subset_plan.h kSubsetChunk
METRICS = ("cosine", "euclidean")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


@functools.lru_cache(maxsize=None)
def _corpus(n, d, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * n + d)
    V = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((80, d)).astype(np.float32)
    V.setflags(write=False)
    Q.setflags(write=False)
    return V, Q


def _index(vdb, V, metric, precision=None):
    ix = vdb.NativeIndex(V.shape[1], metric, precision=precision)
    ix.add(V)
    assert ix.count() == V.shape[0]
    return ix


def _pick(rng, n, length):
    return np.sort(rng.choice(n, size=length, replace=False)).astype(np.int64)


def _same(got, want, what):
    (s, i, k), (es, ei, ek) = got, want
    np.testing.assert_array_equal(i, ei, err_msg=f"indices {what}")
    np.testing.assert_array_equal(k, ek, err_msg=f"keys {what}")
    np.testing.assert_array_equal(s, es, err_msg=f"scores {what}")


def _expect(vdb, ix, V, Q, k, metric, lists, query_list, index_offset=0):
    """(oracle, masked search) results for the queries, list by list."""
    B, n = Q.shape[0], V.shape[0]
    ql = np.arange(B) if query_list is None else np.asarray(query_list)
    ora = (np.zeros((B, k), np.float32), np.full((B, k), -1, np.int64), np.full((B, k), -np.inf))
    msk = tuple(a.copy() for a in ora)
    for li in np.unique(ql):
        members = np.nonzero(ql == li)[0]
        rows = np.asarray(lists[li], np.int64)
        mask = np.zeros(n, bool)
        mask[rows] = True
        es, ei, ek = ref_cpu.exact_search(Q[members], V, k, metric, row_mask=mask)
        ei = np.where(ei >= 0, ei + index_offset, ei)
        for dst, src in zip(ora, (es, ei, ek)):
            dst[members] = src
        ms, mi, mk = ix.search(Q[members], k, row_mask=vdb.rows_to_bitmap(rows, n), with_keys=True,
                               index_offset=index_offset)
        for dst, src in zip(msk, (ms, mi, mk)):
            dst[members] = src
    return ora, msk


def _check(vdb, ix, V, Q, k, metric, lists, query_list=None, index_offset=0, what=""):
    got = ix.search_rows(Q, k, lists, query_list=query_list, with_keys=True, index_offset=index_offset)
    ora, msk = _expect(vdb, ix, V, Q, k, metric, lists, query_list, index_offset)
    _same(got, ora, f"vs oracle {what}")
    _same(got, msk, f"vs masked search {what}")
    s2, i2 = ix.search_rows(Q, k, lists, query_list=query_list, index_offset=index_offset)  # without keys
    np.testing.assert_array_equal(i2, got[1])
    np.testing.assert_array_equal(s2, got[0])
    return got


# =============================================================================
# shapes
# =============================================================================
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 33, 100, 256, 260, 768, 1536])
def test_dims(vdb, dim, metric):
    n = 2000
    V, Q = _corpus(n, dim)
    ix = _index(vdb, V, metric)
    rng = np.random.default_rng(dim)
    lists = [_pick(rng, n, m) for m in (CHUNK - 1, CHUNK, CHUNK + 1, 300)]
    _check(vdb, ix, V, Q[:4], 10, metric, lists, what=f"dim {dim}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_list_lengths(vdb, metric):
    n, k = 3000, 10
    V, Q = _corpus(n, 100)
    ix = _index(vdb, V, metric)
    rng = np.random.default_rng(1)
    lengths = [0, 1, k - 1, k, k + 1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, n]
    lists = [_pick(rng, n, m) for m in lengths]
    lists += [np.array([0, n - 1]), np.array([n - 1]), np.array([0]), np.concatenate([[0], _pick(rng, n - 2, 70) + 1, [n - 1]])]
    got = _check(vdb, ix, V, Q[:len(lists)], k, metric, lists)
    assert (got[1][0] == -1).all() and (got[0][0] == 0).all() and np.isneginf(got[2][0]).all()  # the empty list
    assert (got[1][1][1:] == -1).all() and got[1][1][0] == lists[1][0]
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1, 10, 32, 33, 200, 201, 1024])
def test_k(vdb, k, metric):
    n = 2500
    V, Q = _corpus(n, 64)
    ix = _index(vdb, V, metric)
    rng = np.random.default_rng(k)
    # every list shorter than k (pads), lists around k, and one of every row
    lists = [_pick(rng, n, m) for m in sorted({1, max(k - 1, 1), k, min(k + 1, n), min(k + 300, n), n})]
    _check(vdb, ix, V, Q[:len(lists)], k, metric, lists, what=f"k {k}")
    short = [_pick(rng, n, m) for m in (1, 3)]  # k larger than every list
    got = _check(vdb, ix, V, Q[:2], max(k, 5), metric, short, what=f"k {k} > every list")
    assert (got[1][:, 3:] == -1).all()
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_subset_wgs_identical(vdb, metric):
    n, k = 4000, 40
    V, Q = _corpus(n, 100)
    ix = _index(vdb, V, metric)
    rng = np.random.default_rng(2)
    lists = [_pick(rng, n, m) for m in (1, 70, 1000, n, 0, 3 * CHUNK)]  # 7 segments > the chunks of most
    ref = None
    for wgs in (1, 2, 7, 0):
        ix.set_param("subset_wgs", wgs)
        got = _check(vdb, ix, V, Q[:len(lists)], k, metric, lists, what=f"subset_wgs {wgs}") if ref is None else \
            ix.search_rows(Q[:len(lists)], k, lists, with_keys=True)
        if ref is None:
            ref = got
        _same(got, ref, f"subset_wgs {wgs} vs 1")
    with pytest.raises(ValueError):
        ix.set_param("subset_wgs", -1)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_ties_go_to_the_lower_row(vdb, metric):
    n, k = 4000, 50
    V0, Q0 = _corpus(n, 100)
    V = V0.copy()
    dups = np.arange(37, n, n // 40)[:40]  # 40 copies of one row, ~100 rows apart
    V[dups] = V[dups[0]]
    ix = _index(vdb, V, metric)
    ix.set_param("subset_wgs", 7)
    rng = np.random.default_rng(3)
    rows = np.union1d(dups, _pick(rng, n, 900))  # the copies land in different chunks and segments
    pos = np.searchsorted(rows, dups)
    assert len(set((pos // CHUNK) % 7)) > 1 and len(set(pos // CHUNK)) > 4
    Q = np.stack([V[dups[0]], Q0[0]])
    got = _check(vdb, ix, V, Q, k, metric, [rows], query_list=[0, 0])
    np.testing.assert_array_equal(got[1][0][:40], dups)  # ascending ids ...
    assert len(set(got[2][0][:40].tolist())) == 1         # ... of equal keys
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("B", [1, 4, 65])
def test_batches_and_query_lists(vdb, B, metric):
    n, k = 3000, 10
    V, Q = _corpus(n, 100)
    ix = _index(vdb, V, metric)
    rng = np.random.default_rng(B)
    lengths = [int(x) for x in rng.choice([0, 1, 5, 63, 64, 65, 200, 1500], size=B)]
    if B > 1:
        lengths[1] = 0
    lists = [_pick(rng, n, m) for m in lengths]
    _check(vdb, ix, V, Q[:B], k, metric, lists, what="distinct lists")
    # shared lists: several queries per list, a list used by no query
    few = [_pick(rng, n, m) for m in (300, 64, 0, 7)]
    ql = rng.integers(0, 3, size=B)  # list 3 unused
    _check(vdb, ix, V, Q[:B], k, metric, few, query_list=ql, what="shared lists")
    perm = rng.permutation(B)
    _check(vdb, ix, V, Q[:B], k, metric, lists, query_list=perm, what="permutation")
    ix.close()


def test_index_offset(vdb):
    n = 2000
    V, Q = _corpus(n, 33)
    ix = _index(vdb, V, "cosine")
    rng = np.random.default_rng(4)
    lists = [_pick(rng, n, m) for m in (3, 200)]
    for wgs in (1, 3):
        ix.set_param("subset_wgs", wgs)
        got = _check(vdb, ix, V, Q[:2], 10, "cosine", lists, index_offset=1 << 40)
        assert got[1][0][0] >= 1 << 40 and (got[1][0][3:] == -1).all()
    ix.close()


def test_every_precision_same_output_and_no_candidate_pass(vdb):
    n, k = 3000, 10
    V, Q = _corpus(n, 256)
    rng = np.random.default_rng(5)
    lists = [_pick(rng, n, m) for m in (1, 100, 1000)]
    ref = None
    names = ["searches_fp32", "searches_bf16x3", "searches_bf16", "searches_i8", "searches_i8x3", "searches_i8q",
             "searches", "queries", "fallback_queries"]
    for prec in ("auto", "i8", "bf16x3", "fp32"):
        ix = _index(vdb, V, "cosine", precision=prec)
        before = [ix.stat(s) for s in names]
        got = ix.search_rows(Q[:3], k, lists, with_keys=True)
        assert [ix.stat(s) for s in names] == before, prec
        if ref is None:
            ref = _check(vdb, ix, V, Q[:3], k, "cosine", lists)
        _same(got, ref, f"precision {prec}")
        ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_after_mutations(vdb, metric):
    n, k = 3000, 10
    V0, Q = _corpus(n, 100)
    V = V0.copy()
    ix = _index(vdb, V, metric)
    rng = np.random.default_rng(6)
    lists = [_pick(rng, 2000, m) for m in (5, 64, 700)]  # ids below every later count
    _check(vdb, ix, V, Q[:3], k, metric, lists, what="before")
    gone = _pick(rng, n, 400)
    assert ix.remove(gone) == 400
    V = np.delete(V, gone, axis=0)
    _check(vdb, ix, V, Q[:3], k, metric, lists, what="after a remove that renumbers")
    upd = np.concatenate([lists[0][:3], lists[2][::50]])
    upd = np.unique(upd)
    new = np.random.default_rng(7).standard_normal((upd.size, 100)).astype(np.float32)
    ix.update(upd, new)
    V[upd] = new
    _check(vdb, ix, V, Q[:3], k, metric, lists, what="after an update of listed rows")
    more = np.random.default_rng(8).standard_normal((500, 100)).astype(np.float32)
    ix.add(more)
    V = np.concatenate([V, more])
    lists2 = lists + [np.arange(V.shape[0] - 100, V.shape[0])]
    _check(vdb, ix, V, Q[:4], k, metric, lists2, what="after an add")
    ix.close()


# =============================================================================
# device memory
# =============================================================================
def _device_call(ix, torch, Q, k, offs, rows, ql, stream):
    B = Q.shape[0]
    dev = torch.device("cuda:0")
    with torch.cuda.stream(stream):
        q = torch.from_numpy(np.array(Q, np.float32)).to(dev)
        o = torch.from_numpy(np.ascontiguousarray(offs, np.int64)).to(dev)
        r = torch.from_numpy(np.ascontiguousarray(rows, np.int64)).to(dev) if len(rows) else None
        l = torch.from_numpy(np.ascontiguousarray(ql, np.int32)).to(dev) if ql is not None else None
        s = torch.full((B, k), float("nan"), dtype=torch.float32, device=dev)
        i = torch.full((B, k), -7, dtype=torch.int64, device=dev)
        kk = torch.full((B, k), float("nan"), dtype=torch.float64, device=dev)
        ix.search_rows_device(q.data_ptr(), B, k, o.data_ptr(), len(offs) - 1, r.data_ptr() if r is not None else 0,
                              len(rows), s.data_ptr(), i.data_ptr(), kk.data_ptr(),
                              query_list_ptr=l.data_ptr() if l is not None else 0, stream=stream.cuda_stream)
    stream.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), kk.cpu().numpy()


@pytest.mark.parametrize("metric", METRICS)
def test_device_memory_form(vdb, metric):
    import torch
    n, k = 3000, 10
    V, Q = _corpus(n, 100)
    ix = _index(vdb, V, metric)
    rng = np.random.default_rng(9)
    lists = [_pick(rng, n, m) for m in (0, 5, 64, 65, 900)]
    offs, rows = vdb.pack_row_lists(lists)
    st = torch.cuda.Stream()
    for wgs in (1, 3):
        ix.set_param("subset_wgs", wgs)
        host = ix.search_rows(Q[:5], k, lists, with_keys=True)
        before = ix.stat("subset_bad_ids")
        _same(_device_call(ix, torch, Q[:5], k, offs, rows, None, st), host, "device vs host, identity map")
        ql = np.array([4, 4, 1, 0, 2, 3, 4], np.int32)
        host = ix.search_rows(Q[:7], k, lists, query_list=ql, with_keys=True)
        _same(_device_call(ix, torch, Q[:7], k, offs, rows, ql, st), host, "device vs host, query_list")
        assert ix.stat("subset_bad_ids") == before
        # handled, not trapped: one id >= count, one negative, one repeated
        good = lists[4]
        bad = np.concatenate([good[:7], [-3], good[7:100], [good[99]], good[100:], [n + 5]])
        boffs = np.array([0, bad.size], np.int64)
        want = ix.search_rows(Q[:1], k, [good], with_keys=True)
        _same(_device_call(ix, torch, Q[:1], k, boffs, bad, None, st), want, "list with three bad ids")
        assert ix.stat("subset_bad_ids") == before + 3
        # a query_list entry out of range: an all -1 row, the others untouched by it
        ql = np.array([1, 99, -1, 4], np.int32)
        s, i, kk = _device_call(ix, torch, Q[:4], k, offs, rows, ql, st)
        want = ix.search_rows(Q[[0, 3]], k, lists, query_list=[1, 4], with_keys=True)
        _same((s[[0, 3]], i[[0, 3]], kk[[0, 3]]), want, "rows beside a bad query_list entry")
        assert (i[1:3] == -1).all() and (s[1:3] == 0).all() and np.isneginf(kk[1:3]).all()
        # offsets past n_ids are clamped: the list ends where the ids end
        s, i, kk = _device_call(ix, torch, Q[:1], k, np.array([offs[4], rows.size + 1000]), rows, None, st)
        _same((s, i, kk), ix.search_rows(Q[:1], k, [lists[4]], with_keys=True), "clamped offset")
    ix.close()


# =============================================================================
# host-memory validation
# =============================================================================
def test_host_errors_leave_the_index_usable(vdb):
    n, k = 2000, 5
    V, Q = _corpus(n, 33)
    ix = _index(vdb, V, "cosine")
    rng = np.random.default_rng(10)
    lists = [_pick(rng, n, 50), _pick(rng, n, 3)]
    offs, rows = vdb.pack_row_lists(lists)
    q2 = np.ascontiguousarray(Q[:2])
    want = _check(vdb, ix, V, q2, k, "cosine", lists)
    stats = lambda: tuple(ix.stat(s) for s in ("subset_searches", "subset_queries", "subset_rows", "subset_bad_ids"))
    base = stats()

    def bad(fn):
        before = stats()
        with pytest.raises(ValueError):
            fn()
        assert stats() == before  # only successful calls count
        _same(ix.search_rows(q2, k, lists, with_keys=True), want, "the call after an error")

    bad(lambda: ix.search_rows_csr(q2, k, np.array([0, 53, 50]), rows))            # descending offsets
    bad(lambda: ix.search_rows_csr(q2, k, np.array([0, 50, 54]), rows))            # an offset beyond n_ids
    bad(lambda: ix.search_rows_csr(q2, k, np.array([-1, 50, 53]), rows))           # a negative offset
    bad(lambda: ix.search_rows(q2, k, [lists[0], np.array([5, n])]))               # id out of range
    bad(lambda: ix.search_rows(q2, k, [lists[0], np.array([-1, 5])]))
    bad(lambda: ix.search_rows(q2, k, [lists[0], np.array([5, 9, 7])]))            # unsorted
    bad(lambda: ix.search_rows(q2, k, [lists[0], np.array([5, 5])]))               # repeated
    bad(lambda: ix.search_rows(q2, k, lists, query_list=[0, 2]))                   # bad query_list
    bad(lambda: ix.search_rows(q2, k, lists, query_list=[-1, 0]))
    bad(lambda: ix.search_rows(q2, k, lists[:1]))                                  # no query_list, 1 list, 2 queries
    qn = q2.copy()
    qn[1, 3] = np.nan
    bad(lambda: ix.search_rows(qn, k, lists))                                      # NaN in a query
    bad(lambda: ix.search_rows(q2, 0, lists))
    bad(lambda: ix.search_rows(q2, 1025, lists))
    after = stats()
    # 13 good calls of 2 queries and 53 ids each, one after every error
    assert after[0] - base[0] == 13 and after[1] - base[1] == 26 and after[2] - base[2] == 13 * 53
    assert after[3] == base[3]
    s, i = ix.search_rows(np.zeros((0, 33), np.float32), k, [])                    # no queries: fine
    assert s.shape == (0, k) and i.shape == (0, k)
    ix.close()


def test_empty_index(vdb):
    ix = vdb.NativeIndex(16, "cosine")
    s, i, kk = ix.search_rows(np.ones((2, 16), np.float32), 3, [[], []], with_keys=True)
    assert (i == -1).all() and (s == 0).all() and np.isneginf(kk).all()
    with pytest.raises(ValueError):
        ix.search_rows(np.ones((1, 16), np.float32), 3, [[0]])
    ix.close()


# =============================================================================
# concurrency
# =============================================================================
def test_concurrent_row_searches_beside_ordinary_searches(vdb):
    n, k = 3000, 10
    V, Q = _corpus(n, 100)
    ix = _index(vdb, V, "cosine")
    rng = np.random.default_rng(11)
    jobs = []
    for t in range(4):
        lists = [_pick(rng, n, m) for m in (1 + t, 64, 500 + 100 * t)]
        q = np.ascontiguousarray(Q[3 * t:3 * t + 3])
        jobs.append((q, lists, _expect(vdb, ix, V, q, k, "cosine", lists, None)[0]))
    plain_q = np.ascontiguousarray(Q[20:28])
    plain = ref_cpu.exact_search(plain_q, V, k, "cosine")
    errors = []

    def rows_worker(q, lists, want):
        try:
            for _ in range(20):
                _same(ix.search_rows(q, k, lists, with_keys=True), want, "concurrent search_rows")
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    def plain_worker():
        try:
            for _ in range(20):
                _same(ix.search(plain_q, k, with_keys=True), plain, "concurrent search")
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=rows_worker, args=j) for j in jobs] + [threading.Thread(target=plain_worker)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[0]
    ix.close()

"""Binary codes and the exact Hamming search (include/vdb.h vdb_index_set_codes,
vdb_index_search_hamming; csrc/vdb_hamming.hip).

The contract: d(b, r) = popcount(q_b XOR x_r); the rows whose mask bit is set rank by (d asc, row
asc); slots past min(k, candidates) hold -1 / -1.  Distances are integers, so every comparison is exact
equality with the inline numpy oracle below.  ``_check`` runs a case in host memory and in device
memory; every output carries a guard region past [n_queries][k] that must be untouched.

The sweep: 1, 63, 65, 513 and 1 300 rows (below a wave, across a tile, across a workgroup trip,
several tiles per segment) by codes of 1, 8, 9, 128, 136 and 1 024 bytes (below a word, a whole word,
a ragged word, one full register pass, a ragged second pass, the maximum); inside each, 1, 2 and 7
workgroups per query block, k of 1, 10 and 1 024 and 1, QB and QB + 1 queries, with a half-set mask
that has stray bits at and past count.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 257
S_DIST = -7
S_IDX = -9
DIM = 8
QB = {1: 16, 10: 16, 1024: 1}  # csrc/vdb_hamming_plan.h ham_qb
STATS = ("searches", "queries", "hamming_searches", "hamming_queries", "code_sets", "searches_fp32", "searches_bf16")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def distances(Q, X):
    return np.unpackbits(Q[:, None, :] ^ X[None, :, :], axis=2).sum(2).astype(np.int64)


def oracle(Q, X, k, mask=None, index_offset=0, d=None):
    n = X.shape[0]
    d = distances(Q, X) if d is None else d.copy()
    rows = np.arange(n)
    if mask is not None:
        d[:, ((mask[rows >> 5] >> (rows & 31).astype(np.uint32)) & 1) == 0] = 1 << 40
    dist = np.full((Q.shape[0], k), -1, np.int32)
    idx = np.full((Q.shape[0], k), -1, np.int64)
    for b in range(Q.shape[0]):
        order = np.lexsort((rows, d[b]))[:k]
        order = order[d[b, order] < (1 << 40)]
        dist[b, :order.size] = d[b, order]
        idx[b, :order.size] = order + index_offset
    return dist, idx


def _index(vdb, X, metric="cosine", precision=None):
    ix = vdb.NativeIndex(DIM, metric, precision=precision)
    if X.shape[0]:
        ix.add(np.random.default_rng(1).random((X.shape[0], DIM), dtype=np.float32))
    ix.set_codes(X)
    return ix


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _call(ix, Q, k, mask=None, index_offset=0, mem=0, n_queries=None, null=()):
    """The raw host-memory call with guarded outputs -> (rc, dist, idx)."""
    B = Q.shape[0] if n_queries is None else n_queries
    n = max(B, 0) * max(k, 0)
    dist = np.full(n + GUARD, S_DIST, np.int32)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    q = np.ascontiguousarray(Q)
    rc = ix._lib.vdb_index_search_hamming(ix._h, None if "q" in null else _p(q), B, k, _p(m), mem,
                                          None if "d" in null else _p(dist), None if "i" in null else _p(idx),
                                          index_offset, None)
    assert (dist[n:] == S_DIST).all() and (idx[n:] == S_IDX).all(), "guard touched"
    shape = (max(B, 0), max(k, 0))
    return rc, dist[:n].reshape(shape), idx[:n].reshape(shape)


def _call_device(ix, Q, k, mask=None, index_offset=0):
    import torch
    B, n = Q.shape[0], Q.shape[0] * k
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dq = torch.from_numpy(np.ascontiguousarray(Q)).to("cuda")
        dm = torch.from_numpy(np.ascontiguousarray(mask, np.uint32).view(np.int32).copy()).to("cuda") if mask is not None else None
        dd = torch.full((n + GUARD,), S_DIST, dtype=torch.int32, device="cuda")
        di = torch.full((n + GUARD,), S_IDX, dtype=torch.int64, device="cuda")
        ix.search_hamming_device(dq.data_ptr(), B, k, dd.data_ptr(), di.data_ptr(),
                                 mask_ptr=dm.data_ptr() if dm is not None else 0, index_offset=index_offset,
                                 stream=st.cuda_stream)
    st.synchronize()
    dist, idx = dd.cpu().numpy(), di.cpu().numpy()
    assert (dist[n:] == S_DIST).all() and (idx[n:] == S_IDX).all(), "device guard touched"
    return dist[:n].reshape(B, k), idx[:n].reshape(B, k)


def _check(ix, Q, X, k, mask=None, index_offset=0, what="", d=None):
    want = oracle(Q, X, k, mask, index_offset, d)
    rc, dist, idx = _call(ix, Q, k, mask, index_offset)
    assert rc == 0, what
    np.testing.assert_array_equal(dist, want[0], err_msg=f"host distances {what}")
    np.testing.assert_array_equal(idx, want[1], err_msg=f"host indices {what}")
    dist, idx = _call_device(ix, Q, k, mask, index_offset)
    np.testing.assert_array_equal(dist, want[0], err_msg=f"device distances {what}")
    np.testing.assert_array_equal(idx, want[1], err_msg=f"device indices {what}")


def _half_mask(n, rng):
    m = rng.integers(0, 2**32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    m[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32) if n % 32 else np.uint32(0)  # stray bits at and past count
    return m


@pytest.mark.parametrize("n_bytes", [1, 8, 9, 128, 136, 1024])
@pytest.mark.parametrize("rows", [1, 63, 65, 513, 1300])
def test_sweep(vdb, rows, n_bytes):
    rng = np.random.default_rng(rows * 4099 + n_bytes)
    X = rng.integers(0, 256, (rows, n_bytes), dtype=np.uint8)
    Qall = rng.integers(0, 256, (17, n_bytes), dtype=np.uint8)
    Qall[1] = X[rows // 2]  # an exact hit
    if n_bytes >= 8:  # close codes, so that ties and near-ties reach the head of the lists
        X[::3] = Qall[0]
        X[::3, 0] ^= rng.integers(0, 4, X[::3].shape[0], dtype=np.uint8)
    mask = _half_mask(rows, rng)
    ix = _index(vdb, X)
    assert ix.stat("code_rows") == rows and ix.stat("code_bytes") == n_bytes
    D = distances(Qall, X)  # once, shared by the cases below
    for wgs in (1, 2, 7):
        ix.set_param("hamming_wgs", wgs)
        for k in (1, 10, 1024):
            for nq in (1, QB[k], QB[k] + 1):
                _check(ix, Qall[:nq], X, k, mask if (wgs + nq) % 2 else None, what=f"wgs {wgs} k {k} nq {nq}",
                       d=D[:nq])
    ix.close()


def test_identical_codes_rank_by_row(vdb):
    X = np.tile(np.arange(16, dtype=np.uint8), (1300, 1))
    ix = _index(vdb, X)
    ix.set_param("hamming_wgs", 3)
    for Q in (X[:1], X[:1] ^ np.uint8(0x55)):
        for k in (10, 1024):
            rc, dist, idx = _call(ix, Q, k)
            assert rc == 0
            np.testing.assert_array_equal(idx[0], np.arange(k))
            assert (dist[0] == (0 if Q[0, 0] == 0 else 64)).all()
            _check(ix, Q, X, k)
    ix.close()


def test_one_byte_codes_tie_across_slot_k(vdb):
    rng = np.random.default_rng(5)
    X = rng.integers(0, 256, (1300, 1), dtype=np.uint8)
    Q = rng.integers(0, 256, (17, 1), dtype=np.uint8)
    ix = _index(vdb, X)
    for wgs in (0, 2):
        ix.set_param("hamming_wgs", wgs)
        for k in (1, 10, 100, 1024):
            _check(ix, Q, X, k, what=f"wgs {wgs} k {k}")
    ix.close()


def test_empty_mask_offset_and_empty_index(vdb):
    rng = np.random.default_rng(6)
    X = rng.integers(0, 256, (513, 16), dtype=np.uint8)
    Q = rng.integers(0, 256, (3, 16), dtype=np.uint8)
    ix = _index(vdb, X)
    _check(ix, Q, X, 10, mask=np.zeros(17, np.uint32), what="no bit set")
    _check(ix, Q, X, 10, index_offset=1 << 40, what="index_offset")
    _check(ix, Q, X, 10, mask=_half_mask(513, rng), index_offset=-5, what="mask and offset")
    assert _call(ix, Q, 10, n_queries=0)[0] == 0
    ix.close()
    empty = _index(vdb, X[:0])
    _check(empty, Q, X[:0], 10, what="empty index")
    empty.close()


def test_errors_move_no_stat(vdb):
    rng = np.random.default_rng(7)
    X = rng.integers(0, 256, (65, 8), dtype=np.uint8)
    Q = X[:2].copy()
    ix = vdb.NativeIndex(DIM, "cosine")
    ix.add(rng.random((65, DIM), dtype=np.float32))
    before = {s: ix.stat(s) for s in STATS}
    for mem in (0, 1):
        assert _call(ix, Q, 10, mem=mem)[0] == vdb.VDB_ERR_INVALID  # no column attached
    for bad in (X[:64], X[:, :0], np.zeros((65, 1025), np.uint8)):
        with pytest.raises(ValueError):
            ix.set_codes(bad)
    assert {s: ix.stat(s) for s in STATS} == before
    ix.set_codes(X)
    before = {s: ix.stat(s) for s in STATS}
    for mem in (0, 1):
        for kw in (dict(k=0), dict(k=1025), dict(k=10, n_queries=-1), dict(k=1, n_queries=65536),
                   dict(k=10, null=("q",)), dict(k=10, null=("d",)), dict(k=10, null=("i",))):
            rc, dist, idx = _call(ix, Q, mem=mem, **kw)
            assert rc == vdb.VDB_ERR_INVALID, kw
            assert (dist == S_DIST).all() and (idx == S_IDX).all()
    assert _call(ix, Q, 10, mem=2)[0] == vdb.VDB_ERR_INVALID
    assert {s: ix.stat(s) for s in STATS} == before
    _check(ix, Q, X, 10)
    assert ix.stat("hamming_searches") == before["hamming_searches"] + 2
    assert ix.stat("hamming_queries") == before["hamming_queries"] + 4
    assert ix.stat("searches") == before["searches"] and ix.stat("queries") == before["queries"]
    ix.close()


def test_column_lifetime(vdb):
    rng = np.random.default_rng(8)
    X = rng.integers(0, 256, (70, 8), dtype=np.uint8)
    V = rng.random((65, DIM), dtype=np.float32)
    ix = vdb.NativeIndex(DIM, "cosine")
    ix.add(V)
    ix.set_codes(X[:65])
    bytes_with = ix.stat("device_bytes")
    ix.update(np.array([3, 40]), V[:2])
    assert ix.stat("code_rows") == 65  # an update keeps the column
    _check(ix, X[:2], X[:65], 5)
    for change in (lambda: ix.add(V[:1]), lambda: ix.remove(np.array([0])), ix.clear):
        change()
        assert ix.stat("code_rows") == 0 and ix.stat("code_bytes") == 0
        assert _call(ix, X[:1], 5)[0] == vdb.VDB_ERR_INVALID
        ix.set_codes(X[:ix.count()])
        assert ix.stat("code_rows") == ix.count()
    assert ix.stat("code_sets") == 4
    ix.set_codes(None)
    assert ix.stat("code_rows") == 0 and ix.stat("device_bytes") <= bytes_with
    ix.close()
    bare = vdb.NativeIndex(DIM, "cosine")
    bare.add(V)
    assert bytes_with - bare.stat("device_bytes") == 2 * 1 * 64 * 8  # two tiles of one word
    bare.close()


def test_same_result_for_every_metric_and_precision(vdb):
    rng = np.random.default_rng(9)
    X = rng.integers(0, 256, (513, 9), dtype=np.uint8)
    Q = rng.integers(0, 256, (3, 9), dtype=np.uint8)
    for metric, precision in (("cosine", "fp32"), ("euclidean", "bf16"), ("euclidean", "fp32")):
        ix = _index(vdb, X, metric, precision)
        _check(ix, Q, X, 10, mask=_half_mask(513, rng), what=f"{metric} {precision}")
        ix.close()

"""The integer-MFMA form of the exact Hamming search (include/vdb.h vdb_index_search_hamming, knob
"hamming_mfma"; csrc/vdb_hamming_mfma.hip).

The same contract as the popcount form: d(b, r) = popcount(q_b XOR x_r), candidates rank by (d asc,
row asc), slots past min(k, candidates) hold -1 / -1.  Every comparison is exact equality with the
inline numpy oracle, in host memory and in device memory with a guard region past [n_queries][k].
Every case forces the form (knob = 1) and asserts that "hamming_mfma_queries" rose by the batch, so a
fall-back to the popcount kernel cannot pass.

Shapes: rows below / across a 32-row sub-tile, a whole tile, across a tile and several chunks; code
bytes inside and across a 32-bit piece, a whole and a ragged word, an odd word count (the missing
pair word), 136 and the maximum; batches of a partly empty query tile, a full one, a second tile and
a second block; k of 1, 10, the form's largest and more than the rows; 1, 2 and 7 workgroups per block.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 257
S_DIST, S_IDX = -7, -9
DIM = 8
QB, MAX_K, MIN_Q = 64, 64, 64  # csrc/vdb_hamming_plan.h kHamMfmaQB, kHamMfmaMaxK, kHamMfmaMinQueries


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def oracle(Q, X, k, mask=None, index_offset=0):
    rows = np.arange(X.shape[0])
    dist = np.full((Q.shape[0], k), -1, np.int32)
    idx = np.full((Q.shape[0], k), -1, np.int64)
    for b in range(Q.shape[0]):
        d = np.unpackbits(X ^ Q[b][None, :], axis=1).sum(1).astype(np.int64)
        if mask is not None:
            d[((mask[rows >> 5] >> (rows & 31).astype(np.uint32)) & 1) == 0] = 1 << 40
        order = np.lexsort((rows, d))[:k]
        order = order[d[order] < (1 << 40)]
        dist[b, :order.size] = d[order]
        idx[b, :order.size] = order + index_offset
    return dist, idx


def _index(vdb, X, knob=1):
    ix = vdb.NativeIndex(DIM, "cosine")
    ix.add(np.random.default_rng(1).random((X.shape[0], DIM), dtype=np.float32))
    ix.set_codes(X)
    ix.set_param("hamming_mfma", knob)
    return ix


def _host(ix, Q, k, mask, index_offset):
    n = Q.shape[0] * k
    dist = np.full(n + GUARD, S_DIST, np.int32)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    q = np.ascontiguousarray(Q)
    rc = ix._lib.vdb_index_search_hamming(ix._h, ctypes.c_void_p(q.ctypes.data), Q.shape[0], k,
                                          None if m is None else ctypes.c_void_p(m.ctypes.data), 0,
                                          ctypes.c_void_p(dist.ctypes.data), ctypes.c_void_p(idx.ctypes.data), index_offset, None)
    assert rc == 0
    return dist, idx


def _device(ix, Q, k, mask, index_offset):
    import torch
    n = Q.shape[0] * k
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dq = torch.from_numpy(np.ascontiguousarray(Q)).to("cuda")
        dm = torch.from_numpy(np.ascontiguousarray(mask, np.uint32).view(np.int32).copy()).to("cuda") if mask is not None else None
        dd = torch.full((n + GUARD,), S_DIST, dtype=torch.int32, device="cuda")
        di = torch.full((n + GUARD,), S_IDX, dtype=torch.int64, device="cuda")
        ix.search_hamming_device(dq.data_ptr(), Q.shape[0], k, dd.data_ptr(), di.data_ptr(),
                                 mask_ptr=dm.data_ptr() if dm is not None else 0, index_offset=index_offset,
                                 stream=st.cuda_stream)
    st.synchronize()
    return dd.cpu().numpy(), di.cpu().numpy()


def _check(ix, Q, X, k, mask=None, index_offset=0, what="", mfma=True):
    """Both memory kinds against the oracle; the new form's stat rises by the batch (or not at all)."""
    want = oracle(Q, X, k, mask, index_offset)
    n = Q.shape[0] * k
    for kind, call in (("host", _host), ("device", _device)):
        before = ix.stat("hamming_mfma_queries"), ix.stat("hamming_mfma_searches"), ix.stat("hamming_queries")
        dist, idx = call(ix, Q, k, mask, index_offset)
        assert (dist[n:] == S_DIST).all() and (idx[n:] == S_IDX).all(), f"{kind} guard touched {what}"
        np.testing.assert_array_equal(dist[:n].reshape(-1, k), want[0], err_msg=f"{kind} distances {what}")
        np.testing.assert_array_equal(idx[:n].reshape(-1, k), want[1], err_msg=f"{kind} indices {what}")
        assert ix.stat("hamming_mfma_queries") == before[0] + (Q.shape[0] if mfma else 0), f"{kind} form {what}"
        assert ix.stat("hamming_mfma_searches") == before[1] + (1 if mfma else 0)
        assert ix.stat("hamming_queries") == before[2] + Q.shape[0]


def _half_mask(n, rng):
    m = rng.integers(0, 2**32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    m[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32) if n % 32 else np.uint32(0)  # stray bits at and past count
    return m


def _codes(rows, n_bytes, nq, rng):
    X = rng.integers(0, 256, (rows, n_bytes), dtype=np.uint8)
    Q = rng.integers(0, 256, (nq, n_bytes), dtype=np.uint8)
    Q[nq // 2] = X[rows // 2]  # an exact hit
    if n_bytes >= 8:  # close codes, so that ties and near-ties reach the head of the lists
        X[::3] = Q[0]
        X[::3, 0] ^= rng.integers(0, 4, X[::3].shape[0], dtype=np.uint8)
    return X, Q


@pytest.mark.parametrize("n_bytes", [1, 3, 4, 5, 8, 9, 24, 136, 1024])
@pytest.mark.parametrize("rows", [1, 31, 33, 64, 65, 1300])
def test_rows_by_bytes(vdb, rows, n_bytes):
    rng = np.random.default_rng(rows * 4099 + n_bytes)
    X, Q = _codes(rows, n_bytes, 33, rng)
    ix = _index(vdb, X)
    ix.set_param("hamming_wgs", 2)
    _check(ix, Q, X, 10)
    ix.close()


@pytest.mark.parametrize("rows,n_bytes", [(33, 5), (65, 9), (1300, 136)])
def test_batch_k_segments_mask(vdb, rows, n_bytes):
    rng = np.random.default_rng(rows + n_bytes)
    X, Qall = _codes(rows, n_bytes, QB + 1, rng)
    mask = _half_mask(rows, rng)
    ix = _index(vdb, X)
    for nq in (1, 31, 32, 33, QB + 1):
        ix.set_param("hamming_wgs", 2)
        _check(ix, Qall[:nq], X, 10, mask if nq % 2 else None, what=f"nq {nq}")
    for k in (1, MAX_K):  # (at 33 rows MAX_K is more than the rows: -1 / -1 behind them)
        _check(ix, Qall[:33], X, k, what=f"k {k}")
    for wgs in (1, 7):
        ix.set_param("hamming_wgs", wgs)
        for m in (None, mask):
            _check(ix, Qall[:33], X, 10, m, what=f"wgs {wgs} mask {m is not None}")
    _check(ix, Qall[:33], X, 10, mask, index_offset=(1 << 40) + 3, what="index_offset")
    ix.close()


def test_mask_rules_out_whole_tiles(vdb):
    rng = np.random.default_rng(3)
    X, Q = _codes(1300, 24, 33, rng)
    mask = np.full(41, 0xFFFFFFFF, np.uint32)
    mask[2:4] = 0    # tile 1
    mask[5] = 0      # one sub-tile of tile 2
    mask[8:16] = 0   # a whole chunk
    ix = _index(vdb, X)
    for wgs in (1, 2):
        ix.set_param("hamming_wgs", wgs)
        _check(ix, Q, X, 10, mask, what=f"wgs {wgs}")
    _check(ix, Q, X, 10, np.zeros(41, np.uint32), what="no bit set")
    ix.close()


def test_ties_and_extremes(vdb):
    rng = np.random.default_rng(5)
    # one-byte codes: nine distances, ties decide nearly every slot
    X = rng.integers(0, 256, (1300, 1), dtype=np.uint8)
    Q = rng.integers(0, 256, (QB + 1, 1), dtype=np.uint8)
    ix = _index(vdb, X)
    for wgs, k in ((0, 10), (2, 1), (2, MAX_K)):
        ix.set_param("hamming_wgs", wgs)
        _check(ix, Q, X, k, what=f"one byte wgs {wgs} k {k}")
    ix.close()
    # the largest |dot|: all-ones rows against an all-zeros query and the reverse, at 1 024 bytes
    for xv, qv in ((0xFF, 0), (0, 0xFF)):
        X = np.full((65, 1024), xv, np.uint8)
        X[7, :3] = 0x5A
        Q = np.full((2, 1024), qv, np.uint8)
        Q[1, 1000:] = 0x0F
        ix = _index(vdb, X)
        _check(ix, Q, X, 10, what=f"extremes {xv:#x}")
        ix.close()
    # every row nearer than all before it: each offer passes its threshold, trip after trip
    X = np.zeros((1300, 168), np.uint8)
    for r in range(1300):
        X[r] = np.packbits(np.arange(1344) < 1300 - r)
    ix = _index(vdb, X)
    ix.set_param("hamming_wgs", 1)
    _check(ix, np.zeros((QB, 168), np.uint8), X, 10, what="descending distances")
    ix.close()


def test_ineligible_calls_take_the_popcount_form(vdb):
    rng = np.random.default_rng(6)
    X, Q = _codes(200, 16, MIN_Q, rng)
    ix = _index(vdb, X, knob=1)
    _check(ix, Q[:33], X, MAX_K + 1, what="k past the form's", mfma=False)
    ix.set_param("hamming_mfma", 2)
    _check(ix, Q[:64], X, 10, what="knob 2", mfma=False)
    ix.set_param("hamming_mfma", 0)
    _check(ix, Q[:MIN_Q], X, 10, what="auto at the threshold")
    _check(ix, Q[:MIN_Q - 1], X, 10, what="auto below the threshold", mfma=False)
    for bad in (3, -1):
        with pytest.raises(ValueError):
            ix.set_param("hamming_mfma", bad)
    ix.close()

"""Asymmetric code search (include/vdb.h vdb_index_search_code_dot; csrc/vdb_code_dot.hip, the bit-plane
form, and csrc/vdb_code_dot_mfma.hip, the int8-MFMA form).

Contract: s(b, r) = sum_j q[b][j] * bit_j(code r), candidates rank by (s desc, row asc), slots past
min(k, candidates) hold INT32_MIN / -1.  Every comparison is exact equality with the inline numpy
oracle, in host memory and in device memory with a guard region past [n_queries][k].  Every case forces
a form with the knob "code_dot_mfma" and asserts that form's stat rose by the batch (or stayed), so a
fall-back cannot pass.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 257
S_SCORE, S_IDX = -7, -9
DIM = 8
NONE = np.iinfo(np.int32).min
# csrc/vdb_code_dot_plan.h: kHamMfmaQB, kHamMfmaMaxK, kCdMfmaMinQueries, kCdMfmaChunkBytes
QB, MAX_K, MIN_Q, CHUNK_BYTES = 64, 64, 16, 176
PLANE, MFMA = 2, 1  # knob values
FORMS = [pytest.param(PLANE, id="plane"), pytest.param(MFMA, id="mfma")]


def plane_qb(k, n_bytes):
    """cd_qb of the plan header: the plane form's query block."""
    ke = max(32, 1 << (k - 1).bit_length())
    cap = 1 << (max(2 * ke, ke + 64) - 1).bit_length()
    words = (n_bytes + 7) // 8
    ws = (words + 15) // 16 * 16
    qb = 8
    while qb > 1 and 2 * (qb * 8 * ws * 8 + max(4 * qb * cap * 8, max(cap, 1024) * 8) + 64) > 160 * 1024:
        qb //= 2
    return qb


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def oracle(Q, X, k, mask=None, index_offset=0):
    rows = np.arange(X.shape[0])
    bits = np.unpackbits(X, axis=1, bitorder="little").astype(np.float64)
    S = (bits @ Q.astype(np.float64).T).astype(np.int64).T  # exact: |s| <= 2^20
    assert (S == np.rint(S)).all()
    ok = np.ones(X.shape[0], bool) if mask is None else ((mask[rows >> 5] >> (rows & 31).astype(np.uint32)) & 1) == 1
    score = np.full((Q.shape[0], k), NONE, np.int32)
    idx = np.full((Q.shape[0], k), -1, np.int64)
    for b in range(Q.shape[0]):
        cand = rows[ok]
        order = cand[np.lexsort((cand, -S[b][cand]))][:k]
        score[b, :order.size] = S[b][order]
        idx[b, :order.size] = order + index_offset
    return score, idx


def _index(vdb, X, knob):
    ix = vdb.NativeIndex(DIM, "cosine")
    ix.add(np.random.default_rng(1).random((X.shape[0], DIM), dtype=np.float32))
    ix.set_codes(X)
    ix.set_param("code_dot_mfma", knob)
    return ix


def _host(ix, Q, k, mask, index_offset):
    n = Q.shape[0] * k
    score = np.full(n + GUARD, S_SCORE, np.int32)
    idx = np.full(n + GUARD, S_IDX, np.int64)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    q = np.ascontiguousarray(Q)
    rc = ix._lib.vdb_index_search_code_dot(ix._h, ctypes.c_void_p(q.ctypes.data), Q.shape[0], k,
                                           None if m is None else ctypes.c_void_p(m.ctypes.data), 0,
                                           ctypes.c_void_p(score.ctypes.data), ctypes.c_void_p(idx.ctypes.data), index_offset, None)
    assert rc == 0
    return score, idx


def _device(ix, Q, k, mask, index_offset, shift=0):
    import torch
    n = Q.shape[0] * k
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        # (shift = 1: a query pointer that is not 8-byte aligned)
        dq = torch.from_numpy(np.concatenate([np.zeros(shift, np.int8), Q.reshape(-1)])).to("cuda")
        dm = torch.from_numpy(np.ascontiguousarray(mask, np.uint32).view(np.int32).copy()).to("cuda") if mask is not None else None
        ds = torch.full((n + GUARD,), S_SCORE, dtype=torch.int32, device="cuda")
        di = torch.full((n + GUARD,), S_IDX, dtype=torch.int64, device="cuda")
        ix.search_code_dot_device(dq.data_ptr() + shift, Q.shape[0], k, ds.data_ptr(), di.data_ptr(),
                                  mask_ptr=dm.data_ptr() if dm is not None else 0, index_offset=index_offset,
                                  stream=st.cuda_stream)
    st.synchronize()
    return ds.cpu().numpy(), di.cpu().numpy()


def _unaligned(ix, Q, k, mask, index_offset):
    return _device(ix, Q, k, mask, index_offset, shift=1)


def _check(ix, Q, X, k, mask=None, index_offset=0, what="", mfma=True, calls=(_host, _device)):
    """Both memory kinds against the oracle; the MFMA form's stat rises by the batch (or not at all)."""
    want = oracle(Q, X, k, mask, index_offset)
    n = Q.shape[0] * k
    names = ("code_dot_mfma_queries", "code_dot_mfma_searches", "code_dot_queries", "code_dot_searches", "hamming_queries")
    for call in calls:
        before = [ix.stat(s) for s in names]
        score, idx = call(ix, Q, k, mask, index_offset)
        kind = call.__name__
        assert (score[n:] == S_SCORE).all() and (idx[n:] == S_IDX).all(), f"{kind} guard touched {what}"
        np.testing.assert_array_equal(idx[:n].reshape(-1, k), want[1], err_msg=f"{kind} indices {what}")
        np.testing.assert_array_equal(score[:n].reshape(-1, k), want[0], err_msg=f"{kind} scores {what}")
        B = Q.shape[0]
        assert [ix.stat(s) for s in names] == [before[0] + (B if mfma else 0), before[1] + (1 if mfma else 0),
                                               before[2] + B, before[3] + 1, before[4]], f"{kind} form {what}"


def _half_mask(n, rng):
    m = rng.integers(0, 2**32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    m[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32) if n % 32 else np.uint32(0)  # stray bits at and past count
    return m


def _data(rows, n_bytes, nq, rng, lo=-128, hi=127):
    X = rng.integers(0, 256, (rows, n_bytes), dtype=np.uint8)
    Q = rng.integers(lo, hi + 1, (nq, 8 * n_bytes)).astype(np.int8)
    X[::3] = X[0]  # equal codes: ties at the head of every list
    return X, Q


def _batch(form, k, n_bytes):
    return 33 if form == MFMA else plane_qb(k, n_bytes) + 1


@pytest.mark.parametrize("n_bytes", [1, 3, 8, 9, 24, 136, CHUNK_BYTES, CHUNK_BYTES + 1, 1024])
@pytest.mark.parametrize("rows", [1, 31, 33, 64, 65, 1300])
@pytest.mark.parametrize("form", FORMS)
def test_rows_by_bytes(vdb, form, rows, n_bytes):
    rng = np.random.default_rng(rows * 4099 + n_bytes)
    X, Q = _data(rows, n_bytes, _batch(form, 10, n_bytes), rng)
    ix = _index(vdb, X, form)
    ix.set_param("hamming_wgs", 2)
    _check(ix, Q, X, 10, mfma=form == MFMA)
    ix.close()


@pytest.mark.parametrize("rows,n_bytes", [(33, 3), (65, 9), (1300, 136), (1300, CHUNK_BYTES + 1)])
@pytest.mark.parametrize("form", FORMS)
def test_batch_k_segments_mask(vdb, form, rows, n_bytes):
    rng = np.random.default_rng(rows + n_bytes)
    X, Qall = _data(rows, n_bytes, QB + 1, rng)
    mask = _half_mask(rows, rng)
    on = form == MFMA
    ix = _index(vdb, X, form)
    ix.set_param("hamming_wgs", 2)
    for nq in (1, 31, 33, QB + 1) if on else (1, plane_qb(10, n_bytes) + 1):
        _check(ix, Qall[:nq], X, 10, mask if nq % 2 else None, what=f"nq {nq}", mfma=on)
    for k in (1, MAX_K):  # (at 33 rows MAX_K is more than the rows: "no result" behind them)
        _check(ix, Qall[:_batch(form, k, n_bytes)], X, k, what=f"k {k}", mfma=on)
    _check(ix, Qall[:3], X, MAX_K + 1, what="k past the MFMA form's", mfma=False)
    if not on:
        _check(ix, Qall[:2], X, 1024, mask, what="k 1024", mfma=False)
    for wgs in (1, 7):
        ix.set_param("hamming_wgs", wgs)
        for m in (None, mask):
            _check(ix, Qall[:_batch(form, 10, n_bytes)], X, 10, m, what=f"wgs {wgs} mask {m is not None}", mfma=on)
    _check(ix, Qall[:5], X, 10, mask, index_offset=(1 << 40) + 3, what="index_offset", mfma=on)
    ix.close()


@pytest.mark.parametrize("form", FORMS)
def test_mask_rules_out_whole_tiles(vdb, form):
    rng = np.random.default_rng(3)
    X, Q = _data(1300, 24, 33, rng)
    mask = np.full(41, 0xFFFFFFFF, np.uint32)
    mask[2:4] = 0    # tile 1
    mask[5] = 0      # one sub-tile of tile 2
    mask[8:16] = 0   # a whole chunk
    ix = _index(vdb, X, form)
    for wgs in (1, 2):
        ix.set_param("hamming_wgs", wgs)
        _check(ix, Q, X, 10, mask, what=f"wgs {wgs}", mfma=form == MFMA)
    _check(ix, Q, X, 10, np.zeros(41, np.uint32), what="no bit set", mfma=form == MFMA)
    ix.close()


@pytest.mark.parametrize("form", FORMS)
def test_query_value_ranges(vdb, form):
    """Plane counts of 4 and 1, and a block whose plane count its widest query sets; an unaligned pointer."""
    rng = np.random.default_rng(4)
    n_bytes, on = 24, form == MFMA
    nq = 2 * plane_qb(10, n_bytes)
    X, Q4 = _data(1300, n_bytes, nq, rng, -8, 7)
    Q4[0, :3] = (-8, 7, 0)
    Q1 = rng.integers(-1, 1, (nq, 8 * n_bytes)).astype(np.int8)
    mixed = Q4.copy()
    mixed[1] = rng.integers(-128, 128, 8 * n_bytes)
    mixed[1, 5] = -128  # the block of queries 0 and 1: an int4 query beside one that needs 8 planes
    ix = _index(vdb, X, form)
    ix.set_param("hamming_wgs", 2)
    for name, Q in (("int4", Q4), ("0 / -1", Q1), ("mixed", mixed)):
        _check(ix, Q, X, 10, what=name, mfma=on, calls=(_host, _device, _unaligned))
    ix.close()


@pytest.mark.parametrize("form", FORMS)
def test_ties_extremes_and_refills(vdb, form):
    rng = np.random.default_rng(5)
    on = form == MFMA
    # one-byte codes, queries in {-1, 0, 1}: the row order decides nearly every slot
    X = rng.integers(0, 256, (1300, 1), dtype=np.uint8)
    Q = rng.integers(-1, 2, (QB + 1, 8)).astype(np.int8)
    ix = _index(vdb, X, form)
    for wgs, k in ((0, 10), (2, 1), (2, MAX_K)):
        ix.set_param("hamming_wgs", wgs)
        _check(ix, Q, X, k, what=f"one byte wgs {wgs} k {k}", mfma=on)
    ix.close()
    # the largest |s|: all-ones rows at 1 024 bytes against all -128 and all 127, one row perturbed
    X = np.full((65, 1024), 0xFF, np.uint8)
    X[7, :3] = 0x5A
    Q = np.stack([np.full(8192, -128, np.int8), np.full(8192, 127, np.int8)])
    ix = _index(vdb, X, form)
    _check(ix, Q, X, 10, what="extremes", mfma=on)
    assert oracle(Q, X, 1)[0].ravel().tolist() == [-128 * 8192 + 128 * 12, 127 * 8192]
    ix.close()
    # every row beats all before it, on one workgroup: each offer passes its threshold, trip after trip
    X = np.stack([np.packbits(np.arange(1344) <= r) for r in range(1300)])
    ix = _index(vdb, X, form)
    ix.set_param("hamming_wgs", 1)
    _check(ix, np.ones((QB if on else 9, 1344), np.int8), X, 10, what="ascending scores", mfma=on)
    ix.close()


def test_knob_and_auto_threshold(vdb):
    rng = np.random.default_rng(6)
    X, Q = _data(200, 16, MIN_Q, rng)
    ix = _index(vdb, X, 0)
    _check(ix, Q[:MIN_Q], X, 10, what="auto at the threshold")
    _check(ix, Q[:MIN_Q - 1], X, 10, what="auto below the threshold", mfma=False)
    for knob, on in ((2, False), (1, True), (0, False)):
        ix.set_param("code_dot_mfma", knob)
        _check(ix, Q[:5], X, 10, what=f"knob {knob}", mfma=on)
    for bad in (3, -1):
        with pytest.raises(ValueError):
            ix.set_param("code_dot_mfma", bad)
    ix.close()

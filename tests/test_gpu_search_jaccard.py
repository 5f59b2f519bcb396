"""Jaccard / Tanimoto search over the code column (include/vdb.h vdb_index_search_jaccard;
csrc/vdb_jaccard.hip, the popcount form, and csrc/vdb_jaccard_mfma.hip, the int8-MFMA form).

Contract: i = popcount(q AND x), u = popcount(q OR x); candidates rank by (i / u descending as an exact
rational, u == 0 counting as 1, row ascending); slots past min(k, candidates) hold -1 / -1 / -1.  All
three outputs are compared for equality with an integer-only oracle, in host and in device memory, for
each form forced by the knob "jaccard_mfma", whose stats must rise by the batch (or stay): a fall-back
cannot pass.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
POP, MFMA = 2, 1  # knob values
FORMS = [pytest.param(POP, id="popcount"), pytest.param(MFMA, id="mfma")]
NEW = ("jaccard_queries", "jaccard_searches", "jaccard_mfma_queries", "jaccard_mfma_searches")
STILL = ("hamming_queries", "hamming_searches", "code_dot_queries", "searches", "queries")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def oracle(Q, X, k, mask=None, off=0):
    qb, xb = (np.unpackbits(a, axis=1).astype(np.int64) for a in (Q, X))
    I = qb @ xb.T
    U = qb.sum(1)[:, None] + xb.sum(1)[None, :] - I
    rows = np.arange(X.shape[0])
    cand = rows if mask is None else rows[((mask[rows >> 5] >> (rows & 31).astype(np.uint32)) & 1) == 1]
    out = np.full((3, Q.shape[0], k), -1, np.int64)
    for b in range(Q.shape[0]):
        best = sorted(cand, key=lambda r: (-(Fraction(int(I[b, r]), int(U[b, r])) if U[b, r] else 1), r))[:k]
        out[:, b, :len(best)] = I[b, best], U[b, best], np.asarray(best, np.int64) + off
    return out[0].astype(np.int32), out[1].astype(np.int32), out[2]


def _index(vdb, X, knob, wgs=2):
    ix = vdb.NativeIndex(8, "cosine")
    ix.add(np.random.default_rng(1).random((X.shape[0], 8), dtype=np.float32))
    ix.set_codes(X)
    ix.set_param("jaccard_mfma", knob)
    ix.set_param("hamming_wgs", wgs)
    return ix


def _device(ix, Q, k, mask, off):
    import torch
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dq = torch.from_numpy(Q.copy()).to("cuda")
        dm = torch.from_numpy(mask.view(np.int32).copy()).to("cuda") if mask is not None else None
        dn, du = (torch.full((Q.shape[0], k), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        di = torch.full((Q.shape[0], k), -7, dtype=torch.int64, device="cuda")
        ix.search_jaccard_device(dq.data_ptr(), Q.shape[0], k, dn.data_ptr(), du.data_ptr(), di.data_ptr(),
                                 mask_ptr=dm.data_ptr() if dm is not None else 0, index_offset=off, stream=st.cuda_stream)
    st.synchronize()
    return dn.cpu().numpy(), du.cpu().numpy(), di.cpu().numpy()


def _check(ix, Q, X, k, mask=None, off=0, mfma=False, what=""):
    want = oracle(Q, X, k, mask, off)
    B = Q.shape[0]
    for kind in ("host", "device"):
        before = [ix.stat(s) for s in NEW + STILL]
        got = ix.search_jaccard(Q, k, mask=mask, index_offset=off) if kind == "host" else _device(ix, Q, k, mask, off)
        for name, g, w in zip(("indices", "inter", "union"), (got[2], got[0], got[1]), (want[2], want[0], want[1])):
            np.testing.assert_array_equal(g, w, err_msg=f"{kind} {name} {what}")
        moved = [B, 1, B if mfma else 0, 1 if mfma else 0] + [0] * len(STILL)
        assert [ix.stat(s) for s in NEW + STILL] == [a + m for a, m in zip(before, moved)], f"{kind} stats {what}"


def _data(rows, n_bytes, nq, rng):
    """Few distinct small popcounts over a pool of 16 bit positions spread over the width: dense ties
    (1/2 = 2/4 = 3/6); every fifth row dense; all-zero rows and an all-zero query."""
    bits = 8 * n_bytes
    pool = rng.choice(bits, min(bits, 16), replace=False)

    def draw(n):
        B = np.zeros((n, bits), np.uint8)
        for r in range(n):
            B[r, rng.choice(pool, min(pool.size, int(rng.choice([1, 2, 3, 4, 6]))), replace=False)] = 1
        A = np.packbits(B, axis=1)
        A[::5] = rng.integers(0, 256, A[::5].shape, dtype=np.uint8)
        return A
    X, Q = draw(rows), draw(nq)
    X[3::11] = 0
    X[rows // 2] = 0
    Q[-1] = 0
    return X, Q


@pytest.mark.parametrize("n_bytes", [1, 7, 9, 24, 129, 177, 1024])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("form", FORMS)
def test_rows_by_bytes(vdb, form, rows, n_bytes):
    X, Q = _data(rows, n_bytes, 17, np.random.default_rng(rows * 4099 + n_bytes))
    ix = _index(vdb, X, form)
    _check(ix, Q, X, 10, mfma=form == MFMA)
    ix.close()


@pytest.mark.parametrize("k", [1, 10, 64, 65, 1024])
@pytest.mark.parametrize("nq", [1, 17, 64, 65])
@pytest.mark.parametrize("form", FORMS)
def test_batch_by_k(vdb, form, nq, k):
    """k 65 and 1024 are past the MFMA form: its stats stay even with the knob at 1.  Knob 0 (auto) takes
    the MFMA form from 64 queries (kJacMfmaMinQueries), so it differs from the forced form in one half
    of the cases: it runs there too."""
    X, Q = _data(257, 24, nq, np.random.default_rng(nq * 131 + k))
    ix = _index(vdb, X, form)
    _check(ix, Q, X, k, mfma=form == MFMA and k <= 64)
    if (form == MFMA) != (nq >= 64):
        ix.set_param("jaccard_mfma", 0)
        _check(ix, Q, X, k, mfma=nq >= 64 and k <= 64, what="auto")
    ix.close()


@pytest.mark.parametrize("form", FORMS)
def test_near_collision_needs_an_exact_key(vdb, form):
    """8190/8191 < 8191/8192, and float32(8190)/float32(8191) == float32(8191)/float32(8192): a form that
    ranks in fp32 ties the two and returns row 0 first."""
    rng = np.random.default_rng(7)
    bits = np.ones((6, 8192), np.uint8)
    bits[2:] = rng.integers(0, 2, (4, 8192))
    bits[0, :2] = 0                       # row 0: the query minus one bit; row 1: all ones
    q = np.ones((1, 8192), np.uint8)
    q[0, 0] = 0                           # 8 191 ones
    X, Q = np.packbits(bits, axis=1), np.packbits(q, axis=1)
    ix = _index(vdb, X, form, wgs=0)
    inter, union, idx = ix.search_jaccard(Q, 2)
    assert (inter.tolist(), union.tolist(), idx.tolist()) == ([[8191, 8190]], [[8192, 8191]], [[1, 0]])
    assert ix.search_jaccard(Q, 1)[2].tolist() == [[1]]
    _check(ix, Q, X, 2, mfma=form == MFMA)
    ix.close()


@pytest.mark.parametrize("form", FORMS)
def test_jaccard_is_not_hamming(vdb, form):
    X = np.array([[0x01, 0x00], [0xFF, 0x00], [0xF0, 0xFF]], np.uint8)  # against 0x0F: 1/4 at distance 3, 4/8 at distance 4
    Q = np.array([[0x0F, 0x00]], np.uint8)
    ix = _index(vdb, X, form)
    assert ix.search_hamming(Q, 1)[1].tolist() == [[0]]
    assert [a.tolist() for a in ix.search_jaccard(Q, 3)] == [[[4, 1, 0]], [[8, 4, 16]], [[1, 0, 2]]]
    ix.close()


@pytest.mark.parametrize("form", FORMS)
def test_mask_offset_sentinels(vdb, form):
    rng = np.random.default_rng(9)
    X, Q = _data(257, 9, 17, rng)
    mask = rng.integers(0, 2**32, 9, dtype=np.uint64).astype(np.uint32)
    mask[2:4] = 0                  # tile 1
    mask[5] = 0                    # one 32-row sub-tile of tile 2
    mask[8] = 0xFFFFFFFF           # the last word: one row, stray bits past count
    on = form == MFMA
    ix = _index(vdb, X, form)
    for wgs in (1, 2):
        ix.set_param("hamming_wgs", wgs)
        _check(ix, Q, X, 10, mask, off=(1 << 40) + 3, mfma=on, what=f"wgs {wgs}")
    _check(ix, Q, X, 64, np.where(np.arange(9) == 6, mask, 0).astype(np.uint32), mfma=on, what="fewer candidates than k")
    _check(ix, Q, X, 10, np.zeros(9, np.uint32), mfma=on, what="no bit set")
    ix.close()


def test_errors_move_no_stat(vdb):
    X, Q = _data(65, 9, 3, np.random.default_rng(11))
    bare = vdb.NativeIndex(8, "cosine")
    bare.add(np.zeros((65, 8), np.float32))
    with pytest.raises(ValueError):
        bare.search_jaccard(Q, 5)      # no column
    bare.close()
    empty = vdb.NativeIndex(8, "cosine")
    empty.set_codes(np.zeros((0, 9), np.uint8))
    assert all((a == -1).all() and a.shape == (3, 5) for a in empty.search_jaccard(Q, 5))  # no rows: no result
    empty.close()
    ix = _index(vdb, X, 0)
    out = [np.zeros(30, np.int32), np.zeros(30, np.int32), np.zeros(30, np.int64)]
    p = [ctypes.c_void_p(a.ctypes.data) for a in out]
    qp = ctypes.c_void_p(Q.ctypes.data)
    call = lambda k, mem, a, b, c: ix._lib.vdb_index_search_jaccard(ix._h, qp, 3, k, None, mem, a, b, c, 0, None)
    before = [ix.stat(s) for s in NEW]
    for bad in ((0, 0, *p), (1025, 0, *p), (5, 7, *p), (5, 0, None, p[1], p[2]), (5, 0, p[0], None, p[2]), (5, 0, p[0], p[1], None)):
        assert call(*bad) != 0, bad[:2]
    for knob in (3, -1):
        with pytest.raises(ValueError):
            ix.set_param("jaccard_mfma", knob)
    assert [ix.stat(s) for s in NEW] == before
    assert ix._lib.vdb_index_search_jaccard(ix._h, None, 0, 5, None, 0, None, None, None, 0, None) == 0  # an empty batch
    assert call(5, 0, *p) == 0 and [ix.stat(s) for s in NEW] == [before[0] + 3, before[1] + 1, before[2], before[3]]
    ix.close()

"""Jaccard range search (include/vdb.h vdb_index_search_jaccard_range; csrc/vdb_jaccard_range.hip).

With i = popcount(q AND x) and u = popcount(q OR x) (tested as 1 / 1 when u == 0), row r passes query b
when its mask bit is set, r < count and i * den >= num * u; out_counts is the exact number of passing
rows, the first min(count, cap) of them come in ascending row id with the raw i and u, later slots hold
-1 / -1 / -1 and nothing at or past cap is written.  Every comparison is exact equality with the inline
numpy oracle (unpackbits, int64 cross-multiplication), in host memory and in device memory with a guard
region past [n_queries][cap] and past out_counts.  Every case forces one of the two scans by the knob
"jaccard_range_mfma" and asserts that "jaccard_range_mfma_queries" rose by the batch (or, for the
popcount scan, not at all), so a fall-back cannot pass.

Shapes: rows 1, 33, 65, 513, 1 100 (a word, a tile, a chunk and two chunks crossed); code bytes 1, 3, 24
(an odd word count), 136 (a second register pass) and 1 024; batches 1, 5, 16, 64 and 70.  Each batch
mixes planted thresholds: a row at 2/4 against 1/2 and one at 2/5 (its cross-product misses by one); a row
at 3/6 against 2^17 / 2^18; num = 0; num = den with a planted copy of the query; an all-zero query at 1/1
with a planted empty row; at 1 024 bytes an all-ones query and row at 2^18 / 2^18 (the product is 2^31);
fractions around the random codes' similarity behind them.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 67
S_CNT, S_IDX, S_INT, S_UNI = -5, -9, -7, -3
DIM = 8
FORMS = [pytest.param(2, id="popcount"), pytest.param(1, id="mfma")]
STATS = ("jaccard_range_mfma_queries", "jaccard_range_mfma_searches", "jaccard_range_queries", "jaccard_range_searches",
         "jaccard_queries", "hamming_range_queries", "hamming_queries", "searches", "queries")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def oracle(Q, X, num, den, cap, mask=None, index_offset=0):
    rows = np.arange(X.shape[0])
    ok = np.ones(X.shape[0], bool) if mask is None else ((mask[rows >> 5] >> (rows & 31).astype(np.uint32)) & 1) == 1
    B = Q.shape[0]
    counts = np.zeros(B, np.int64)
    idx = np.full((B, cap), -1, np.int64)
    inter = np.full((B, cap), -1, np.int32)
    union = np.full((B, cap), -1, np.int32)
    Xb = np.unpackbits(X, axis=1)
    for b in range(B):
        n, d = int(num[b]), int(den[b])
        if not (1 <= d <= 1 << 18 and 0 <= n <= d):
            continue  # a device-memory call's bad threshold: nothing passes
        qb = np.unpackbits(Q[b])[None, :]
        i = (Xb & qb).sum(1).astype(np.int64)
        u = (Xb | qb).sum(1).astype(np.int64)
        it, ut = np.where(u == 0, 1, i), np.where(u == 0, 1, u)
        hit = rows[ok & (it * d >= n * ut)]  # ascending rows
        f = min(hit.size, cap)
        counts[b] = hit.size
        idx[b, :f], inter[b, :f], union[b, :f] = hit[:f] + index_offset, i[hit[:f]], u[hit[:f]]
    return counts, idx, inter, union


def _host(ix, Q, num, den, cap, mask, index_offset):
    B = Q.shape[0]
    bufs = [np.full(B + GUARD, S_CNT, np.int64), np.full(B * cap + GUARD, S_IDX, np.int64),
            np.full(B * cap + GUARD, S_INT, np.int32), np.full(B * cap + GUARD, S_UNI, np.int32)]
    args = [np.ascontiguousarray(Q), np.ascontiguousarray(num, np.int32), np.ascontiguousarray(den, np.int32)]
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = ix._lib.vdb_index_search_jaccard_range(ix._h, p(args[0]), B, p(args[1]), p(args[2]), None if m is None else p(m), 0, cap,
                                                *[p(b) for b in bufs], index_offset, None)
    assert rc == 0
    return bufs


def _device(ix, Q, num, den, cap, mask, index_offset):
    import torch
    B = Q.shape[0]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dq = torch.from_numpy(np.ascontiguousarray(Q)).to("cuda")
        dn = torch.from_numpy(np.ascontiguousarray(num, np.int32)).to("cuda")
        dd = torch.from_numpy(np.ascontiguousarray(den, np.int32)).to("cuda")
        dm = torch.from_numpy(np.ascontiguousarray(mask, np.uint32).view(np.int32).copy()).to("cuda") if mask is not None else None
        out = [torch.full((B + GUARD,), S_CNT, dtype=torch.int64, device="cuda"),
               torch.full((B * cap + GUARD,), S_IDX, dtype=torch.int64, device="cuda"),
               torch.full((B * cap + GUARD,), S_INT, dtype=torch.int32, device="cuda"),
               torch.full((B * cap + GUARD,), S_UNI, dtype=torch.int32, device="cuda")]
        ix.search_jaccard_range_device(dq.data_ptr(), B, dn.data_ptr(), dd.data_ptr(), cap, *[o.data_ptr() for o in out],
                                       mask_ptr=dm.data_ptr() if dm is not None else 0, index_offset=index_offset,
                                       stream=st.cuda_stream)
    st.synchronize()
    return [o.cpu().numpy() for o in out]


def _check(ix, Q, X, thr, cap, mask=None, index_offset=0, what="", mfma=True, kinds=(_host, _device)):
    """The memory kinds against the oracle; the MFMA scan's stats rise by the batch (or not at all)."""
    num, den = thr
    want = oracle(Q, X, num, den, cap, mask, index_offset)
    B = Q.shape[0]
    for call in kinds:
        before = [ix.stat(s) for s in STATS]
        got = call(ix, Q, num, den, cap, mask, index_offset)
        tag = f"{call.__name__} {what} cap {cap}"
        for g, sentinel, n in zip(got, (S_CNT, S_IDX, S_INT, S_UNI), (B, B * cap, B * cap, B * cap)):
            assert (g[n:] == sentinel).all(), f"guard {tag}"
        np.testing.assert_array_equal(got[0][:B], want[0], err_msg=f"counts {tag}")
        for g, w, name in zip(got[1:], want[1:], ("indices", "intersections", "unions")):
            np.testing.assert_array_equal(g[:B * cap].reshape(B, cap), w, err_msg=f"{name} {tag}")
        moved = [B if mfma else 0, 1 if mfma else 0, B, 1, 0, 0, 0, 0, 0]
        assert [ix.stat(s) for s in STATS] == [b + m for b, m in zip(before, moved)], f"stats {tag}"
    return want[0]


def _bits(n_bytes, *ones):
    b = np.zeros(8 * n_bytes, np.uint8)
    b[list(ones)] = 1
    return np.packbits(b)


def _case(rows, n_bytes, nq, seed):
    """Codes, queries and thresholds (num, den) with the planted rows of the module docstring."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (rows, n_bytes), dtype=np.uint8)
    Q = rng.integers(0, 256, (nq, n_bytes), dtype=np.uint8)
    num = np.array([2 + b % 3 for b in range(nq)], np.int32)  # 2/9, 3/9, 4/9: around 1/3, random codes' similarity
    den = np.full(nq, 9, np.int32)
    plant = {}
    Q[0], num[0], den[0] = _bits(n_bytes, 0, 1, 2), 1, 2
    plant[rows // 3] = _bits(n_bytes, 0, 1, 3, 4)   # 2 / 5 against 1 / 2: 2 * 2 < 1 * 5 by one
    if nq > 1:
        Q[1], num[1], den[1] = _bits(n_bytes, 0, 1, 2, 3), 1 << 17, 1 << 18
        plant[rows // 2] = _bits(n_bytes, 0, 1, 2, 4, 5)  # 3 / 6 against 2^17 / 2^18
    if nq > 2:
        num[2], den[2] = 0, 7                       # every eligible row
    if nq > 3:
        num[3], den[3] = 5, 5                       # only copies of the query
        plant[rows // 4] = Q[3].copy()
    if nq > 4:
        Q[4], num[4], den[4] = 0, 1, 1              # an all-zero query: only empty rows
        plant[rows // 5] = np.zeros(n_bytes, np.uint8)
    if nq > 5 and n_bytes == 1024:
        Q[5], num[5], den[5] = 255, 1 << 18, 1 << 18  # 8 192 * 2^18 = 2^31 on both sides
        plant[rows // 6] = np.full(n_bytes, 255, np.uint8)
    if rows >= 12:  # (fewer rows: the planted positions would collide)
        for r, code in plant.items():
            X[r] = code
    X[rows - 1] = _bits(n_bytes, 0, 1, 3)           # 2 / 4 against 1 / 2: passes, in the last row
    return X, Q, (num, den)


def _index(vdb, X, knob):
    ix = vdb.NativeIndex(DIM, "cosine")
    if X.shape[0]:
        ix.add(np.random.default_rng(1).random((X.shape[0], DIM), dtype=np.float32))
    ix.set_codes(X)
    ix.set_param("jaccard_range_mfma", knob)
    return ix


@pytest.mark.parametrize("knob", FORMS)
@pytest.mark.parametrize("rows,n_bytes,nq", [(1, 3, 1), (33, 1, 5), (65, 24, 16), (513, 136, 5), (1100, 3, 70), (130, 1024, 16),
                                             (200, 24, 64)])
def test_rows_bytes_batches(vdb, knob, rows, n_bytes, nq):
    X, Q, thr = _case(rows, n_bytes, nq, rows * 4099 + n_bytes * 17 + nq)
    ix = _index(vdb, X, knob)
    counts = _check(ix, Q, X, thr, 0, mfma=knob == 1, kinds=(_device,))
    assert counts[0] >= 1 and (nq < 3 or counts[2] == rows) and (nq < 5 or (counts[3] >= 1 and counts[4] >= 1))
    assert nq < 6 or n_bytes != 1024 or counts[5] == 1
    _check(ix, Q, X, thr, int(counts.max()), mfma=knob == 1)  # exactly the count for one query, more for others
    ix.close()


@pytest.mark.parametrize("knob", FORMS)
def test_caps_mask_offset(vdb, knob):
    rows, nq = 513, 7
    X, Q, thr = _case(rows, 9, nq, 77)
    rng = np.random.default_rng(rows)
    mask = rng.integers(0, 2**32, (rows + 31) // 32, dtype=np.uint64).astype(np.uint32)
    mask[-1] |= np.uint32((0xFFFFFFFF << (rows % 32)) & 0xFFFFFFFF)  # stray bits at and past count
    ix = _index(vdb, X, knob)
    counts = _check(ix, Q, X, thr, 0, mask, what="masked", mfma=knob == 1)
    assert 1 < counts.max() < rows
    for cap in (1, int(counts.max()) // 2, int(counts.max()) + 3):  # below the count and above it
        _check(ix, Q, X, thr, cap, mask, index_offset=(1 << 40) + 3, what="masked, offset", mfma=knob == 1)
    _check(ix, Q, X, thr, 3, np.zeros_like(mask), what="no bit set", mfma=knob == 1)
    ix.close()


@pytest.mark.parametrize("knob", FORMS)
def test_device_bad_thresholds_and_empty_index(vdb, knob):
    X, Q, (num, den) = _case(200, 9, 6, 11)
    ix = _index(vdb, X, knob)
    num[1], den[1] = 1, 0      # den == 0
    num[3], den[3] = 6, 5      # num > den
    num[5], den[5] = -1, 9     # negative num
    got = _check(ix, Q, X, (num, den), 6, what="bad thresholds", mfma=knob == 1, kinds=(_device,))
    assert got[1] == 0 and got[3] == 0 and got[5] == 0 and got[2] == 200 and got[0] >= 1
    with pytest.raises(ValueError, match="threshold"):
        ix.search_jaccard_range(Q, num, den, cap=6)
    ix.close()
    ix = _index(vdb, np.zeros((0, 9), np.uint8), knob)
    for cap in (0, 4):
        _check(ix, Q[:3], np.zeros((0, 9), np.uint8), (np.array([0, 1, 1]), np.array([1, 2, 1])), cap, what="empty index",
               mfma=knob == 1)
    ix.close()


def test_errors_move_no_stat(vdb):
    X, Q, (num, den) = _case(200, 9, 5, 13)
    bare = vdb.NativeIndex(DIM, "cosine")
    with pytest.raises(ValueError, match="column"):
        bare.search_jaccard_range(Q, num, den, cap=1)
    bare.close()
    ix = _index(vdb, X, 0)
    before = [ix.stat(s) for s in STATS]
    cnt, idx, inter, union = np.zeros(5, np.int64), np.zeros(5, np.int64), np.zeros(5, np.int32), np.zeros(5, np.int32)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    bad_den, bad_num = den.copy(), num.copy()
    bad_den[2], bad_num[4] = (1 << 18) + 1, -1
    good = dict(q=Q, B=5, n=num, d=den, mem=0, cap=1, c=cnt, i=idx, it=inter, un=union)
    for bad in (dict(B=-1), dict(B=65536), dict(cap=-1), dict(cap=(1 << 36) // 5 + 1), dict(q=None), dict(n=None), dict(d=None),
                dict(c=None), dict(i=None), dict(it=None), dict(un=None), dict(mem=2), dict(d=bad_den), dict(n=bad_num),
                dict(d=np.zeros(5, np.int32)), dict(n=den + 1)):
        a = dict(good, **bad)
        rc = ix._lib.vdb_index_search_jaccard_range(ix._h, p(a["q"]), a["B"], p(a["n"]), p(a["d"]), None, a["mem"], a["cap"],
                                                    p(a["c"]), p(a["i"]), p(a["it"]), p(a["un"]), 0, None)
        assert rc == vdb.VDB_ERR_INVALID, bad
    assert [ix.stat(s) for s in STATS] == before
    counts, idx, inter, union = ix.search_jaccard_range(Q[:0], num[:0], den[:0], cap=4)
    assert counts.size == 0 and idx.shape == (0, 4) and [ix.stat(s) for s in STATS] == before
    for v in (3, -1):
        with pytest.raises(ValueError):
            ix.set_param("jaccard_range_mfma", v)
    # auto: the MFMA scan from 64 queries (csrc/vdb_jaccard_range_plan.h kJacRangeMfmaMinQueries)
    X64, Q64, thr64 = _case(200, 9, 64, 17)
    ix.set_codes(X64)
    _check(ix, Q64, X64, thr64, 2, what="auto at the threshold", mfma=True, kinds=(_host,))
    _check(ix, Q64[:63], X64, (thr64[0][:63], thr64[1][:63]), 2, what="auto below the threshold", mfma=False, kinds=(_host,))
    ix.set_codes(X)
    # cap=None: a count-only call, then one with the largest count
    got = ix.search_jaccard_range(Q, num, den)
    want = oracle(Q, X, num, den, 200)
    assert got[1].shape == (5, 200) and all((g == w).all() for g, w in zip(got, want))
    ix.close()

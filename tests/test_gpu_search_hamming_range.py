"""Hamming range search (include/vdb.h vdb_index_search_hamming_range; csrc/vdb_hamming_range.hip).

Row r passes query b when its mask bit is set, r < count and popcount(q_b XOR x_r) <= radii[b];
out_counts is the exact number of passing rows, the first min(count, cap) of them come in ascending
row id with their distances, later slots hold -1 / -1 and nothing at or past cap is written.  Every
comparison is exact equality with the inline numpy oracle, in host memory and in device memory with
a guard region past [n_queries][cap] and past out_counts.  Every case forces one of the two scans by
the knob "hamming_range_mfma" and asserts that "hamming_range_mfma_queries" rose by the batch (or,
for the popcount scan, not at all), so a fall-back cannot pass.

Shapes: rows below and across a 32-row word, a 64-row tile and a 512-row chunk (at 1 and 31 the last
tile's second word lies past n_words); code bytes of a ragged and a whole word, an odd word count
(the MFMA scan's missing pair word), 136 (a second register pass) and the maximum; batches of a
partly empty query tile, a full popcount block, a full MFMA block and a second ragged one.  Each
batch mixes the radii: a planted row at exactly r and another at r + 1, 0 with a planted duplicate,
8 n_bytes (everything), more than that, and half the bits.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 67
S_CNT, S_IDX, S_DIST = -5, -9, -7
DIM = 8
FORMS = [pytest.param(2, id="popcount"), pytest.param(1, id="mfma")]


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def oracle(Q, X, radii, cap, mask=None, index_offset=0):
    rows = np.arange(X.shape[0])
    ok = np.ones(X.shape[0], bool) if mask is None else ((mask[rows >> 5] >> (rows & 31).astype(np.uint32)) & 1) == 1
    counts = np.zeros(Q.shape[0], np.int64)
    idx = np.full((Q.shape[0], cap), -1, np.int64)
    dist = np.full((Q.shape[0], cap), -1, np.int32)
    for b in range(Q.shape[0]):
        d = np.unpackbits(X ^ Q[b][None, :], axis=1).sum(1).astype(np.int64) if X.shape[0] else np.zeros(0, np.int64)
        hit = rows[ok & (d <= radii[b])]  # ascending rows
        counts[b] = hit.size
        idx[b, :min(hit.size, cap)] = hit[:cap] + index_offset
        dist[b, :min(hit.size, cap)] = d[hit[:cap]]
    return counts, idx, dist


def _host(ix, Q, radii, cap, mask, index_offset):
    B = Q.shape[0]
    bufs = [np.full(B + GUARD, S_CNT, np.int64), np.full(B * cap + GUARD, S_IDX, np.int64), np.full(B * cap + GUARD, S_DIST, np.int32)]
    q, r = np.ascontiguousarray(Q), np.ascontiguousarray(radii, np.int32)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    rc = ix._lib.vdb_index_search_hamming_range(
        ix._h, ctypes.c_void_p(q.ctypes.data), B, ctypes.c_void_p(r.ctypes.data), None if m is None else ctypes.c_void_p(m.ctypes.data),
        0, cap, *[ctypes.c_void_p(b.ctypes.data) for b in bufs], index_offset, None)
    assert rc == 0
    return bufs


def _device(ix, Q, radii, cap, mask, index_offset):
    import torch
    B = Q.shape[0]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dq = torch.from_numpy(np.ascontiguousarray(Q)).to("cuda")
        dr = torch.from_numpy(np.ascontiguousarray(radii, np.int32)).to("cuda")
        dm = torch.from_numpy(np.ascontiguousarray(mask, np.uint32).view(np.int32).copy()).to("cuda") if mask is not None else None
        dc = torch.full((B + GUARD,), S_CNT, dtype=torch.int64, device="cuda")
        di = torch.full((B * cap + GUARD,), S_IDX, dtype=torch.int64, device="cuda")
        dd = torch.full((B * cap + GUARD,), S_DIST, dtype=torch.int32, device="cuda")
        ix.search_hamming_range_device(dq.data_ptr(), B, dr.data_ptr(), cap, dc.data_ptr(), di.data_ptr(), dd.data_ptr(),
                                       mask_ptr=dm.data_ptr() if dm is not None else 0, index_offset=index_offset,
                                       stream=st.cuda_stream)
    st.synchronize()
    return dc.cpu().numpy(), di.cpu().numpy(), dd.cpu().numpy()


def _check(ix, Q, X, radii, cap, mask=None, index_offset=0, what="", mfma=True, kinds=(_host, _device)):
    """Both memory kinds against the oracle; the MFMA scan's stat rises by the batch (or not at all)."""
    want = oracle(Q, X, radii, cap, mask, index_offset)
    B = Q.shape[0]
    for call in kinds:
        names = ("hamming_range_mfma_queries", "hamming_range_mfma_searches", "hamming_range_queries", "hamming_queries", "searches")
        before = [ix.stat(s) for s in names]
        cnt, idx, dist = call(ix, Q, radii, cap, mask, index_offset)
        tag = f"{call.__name__} {what} cap {cap}"
        assert (cnt[B:] == S_CNT).all() and (idx[B * cap:] == S_IDX).all() and (dist[B * cap:] == S_DIST).all(), f"guard {tag}"
        np.testing.assert_array_equal(cnt[:B], want[0], err_msg=f"counts {tag}")
        np.testing.assert_array_equal(idx[:B * cap].reshape(B, cap), want[1], err_msg=f"indices {tag}")
        np.testing.assert_array_equal(dist[:B * cap].reshape(B, cap), want[2], err_msg=f"distances {tag}")
        assert [ix.stat(s) for s in names] == [before[0] + (B if mfma else 0), before[1] + (1 if mfma else 0),
                                                before[2] + B, before[3], before[4]], f"stats {tag}"
    return want[0]


def _flip(code, n):
    bits = np.unpackbits(code)
    bits[:n] ^= 1
    return np.packbits(bits)


def _case(rows, n_bytes, nq, seed):
    """Codes, queries and mixed radii with the planted rows of the module docstring."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (rows, n_bytes), dtype=np.uint8)
    Q = rng.integers(0, 256, (nq, n_bytes), dtype=np.uint8)
    r = min(5, 8 * n_bytes - 1)
    radii = np.array([r, 0, 8 * n_bytes, 8 * n_bytes + 9, 4 * n_bytes][:nq] + [4 * n_bytes - (b % 7) for b in range(5, nq)], np.int32)
    X[rows - 1] = _flip(Q[0], r)          # exactly at the radius, in the last row: passes
    if rows >= 3:
        X[rows // 3] = _flip(Q[0], r + 1)  # one bit past it: does not
        if nq > 1:
            X[rows // 2] = Q[1]            # a duplicate, radius 0
    return X, Q, radii


def _index(vdb, X, knob):
    ix = vdb.NativeIndex(DIM, "cosine")
    if X.shape[0]:
        ix.add(np.random.default_rng(1).random((X.shape[0], DIM), dtype=np.float32))
    ix.set_codes(X)
    ix.set_param("hamming_range_mfma", knob)
    return ix


def _half_mask(n, rng):
    m = rng.integers(0, 2**32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    if n % 32:
        m[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # stray bits at and past count
    return m


@pytest.mark.parametrize("knob", FORMS)
@pytest.mark.parametrize("rows,n_bytes,nq", [(r, 9, 5) for r in (1, 31, 33, 64, 65, 511, 513, 1100)] +
                         [(130, nb, 5) for nb in (1, 3, 8, 24, 136, 1024)] + [(200, 9, nq) for nq in (1, 16, 17, 64, 65, 130)])
def test_rows_bytes_batches(vdb, knob, rows, n_bytes, nq):
    X, Q, radii = _case(rows, n_bytes, nq, rows * 4099 + n_bytes * 17 + nq)
    ix = _index(vdb, X, knob)
    counts = _check(ix, Q, X, radii, 0, mfma=knob == 1, kinds=(_device,))
    assert counts[0] >= 1 and (nq < 3 or counts[2] == rows)  # the planted row at the radius passes; 8 n_bytes: every row
    _check(ix, Q, X, radii, int(counts.max()), mfma=knob == 1)           # exactly the count for one query, more for others
    ix.close()


@pytest.mark.parametrize("knob", FORMS)
@pytest.mark.parametrize("rows,n_bytes,nq", [(200, 9, 5), (513, 9, 65)])
def test_caps_mask_offset(vdb, knob, rows, n_bytes, nq):
    X, Q, radii = _case(rows, n_bytes, nq, rows + nq)
    mask = _half_mask(rows, np.random.default_rng(rows))
    ix = _index(vdb, X, knob)
    counts = _check(ix, Q, X, radii, 0, mask, what="masked", mfma=knob == 1)
    assert 1 < counts.max() < rows
    for cap in (1, int(counts.max()) // 2, int(counts.max()), int(counts.max()) + 3):  # less, exact, more
        _check(ix, Q, X, radii, cap, mask, index_offset=(1 << 40) + 3, what="masked, offset", mfma=knob == 1)
    _check(ix, Q, X, radii, rows + 1, what="unmasked", mfma=knob == 1)
    _check(ix, Q, X, radii, 3, np.zeros_like(mask), what="no bit set", mfma=knob == 1)
    ix.close()


@pytest.mark.parametrize("knob", FORMS)
def test_empty_index_no_queries_and_negative_radius(vdb, knob):
    ix = _index(vdb, np.zeros((0, 9), np.uint8), knob)
    Q = np.random.default_rng(2).integers(0, 256, (3, 9), dtype=np.uint8)
    for cap in (0, 4):
        _check(ix, Q, np.zeros((0, 9), np.uint8), np.array([0, 5, 99], np.int32), cap, what="empty index", mfma=knob == 1)
    ix.close()
    X, Q, radii = _case(200, 9, 5, 11)
    ix = _index(vdb, X, knob)
    before = ix.stat("hamming_range_searches")
    counts, idx, dist = ix.search_hamming_range(Q[:0], radii[:0], cap=4)
    assert counts.size == 0 and idx.shape == (0, 4) and ix.stat("hamming_range_searches") == before
    radii[2] = -1  # a device-memory call: that query counts 0, all its slots -1
    got = _check(ix, Q, X, radii, 6, what="negative radius", mfma=knob == 1, kinds=(_device,))
    assert got[2] == 0 and got[3] == 200
    with pytest.raises(ValueError, match="radi"):
        ix.search_hamming_range(Q, radii, cap=6)
    # cap=None: a count-only call, then one with the largest count
    radii[2] = 8 * 9
    counts, idx, dist = ix.search_hamming_range(Q, radii)
    want = oracle(Q, X, radii, 200)
    assert idx.shape == (5, 200) and (counts == want[0]).all() and (idx == want[1]).all() and (dist == want[2]).all()
    ix.close()


def test_errors_and_choice_of_scan(vdb):
    X, Q, radii = _case(200, 9, 64, 13)
    bare = vdb.NativeIndex(DIM, "cosine")
    with pytest.raises(ValueError, match="column"):
        bare.search_hamming_range(Q, radii, cap=1)
    bare.close()
    ix = _index(vdb, X, 0)
    names = ("hamming_range_searches", "hamming_range_queries", "hamming_range_mfma_searches")
    before = [ix.stat(s) for s in names]
    cnt, idx, dist = np.zeros(64, np.int64), np.zeros(64, np.int64), np.zeros(64, np.int32)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    good = dict(q=Q, B=64, r=radii, mem=0, cap=1, c=cnt, i=idx, d=dist)
    for bad in (dict(B=-1), dict(B=65536), dict(cap=-1), dict(cap=(1 << 36) // 64 + 1), dict(q=None), dict(r=None), dict(c=None),
                dict(i=None), dict(d=None), dict(mem=2)):
        a = dict(good, **bad)
        rc = ix._lib.vdb_index_search_hamming_range(ix._h, p(a["q"]), a["B"], p(a["r"]), None, a["mem"], a["cap"], p(a["c"]),
                                                    p(a["i"]), p(a["d"]), 0, None)
        assert rc == vdb.VDB_ERR_INVALID, bad
    assert [ix.stat(s) for s in names] == before
    # auto: the MFMA scan from 64 queries (csrc/vdb_hamming_range_plan.h kHamRangeMfmaMinQueries)
    _check(ix, Q, X, radii, 2, what="auto at the threshold", mfma=True, kinds=(_host,))
    _check(ix, Q[:63], X, radii[:63], 2, what="auto below the threshold", mfma=False, kinds=(_host,))
    for v in (3, -1):
        with pytest.raises(ValueError):
            ix.set_param("hamming_range_mfma", v)
    ix.close()

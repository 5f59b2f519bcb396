"""The stand-alone operators of csrc/vdb_ops.hip, each alone through the C-ABI on device buffers:
vdb_similarity_matrix (sim_gemm_kernel, l2_matrix_kernel), vdb_normalize_rows and vdb_topk_scores
(topk_chunk_kernel, the fp32 list merge, topk_write_kernel).  These kernels hand every score to the
caller with no certificate or exact fallback behind them, so a wrong tile tail or lane-to-row map is
simply a wrong answer.

Every comparison is against fp64 numpy over the same fp32 inputs, within the error bounds derived in
tests/_ops_cases.py (no flat tolerance; the one exception is the header's own 1e-4 for cosine at
D <= 768); top-k is exact.  tests/test_ops_precondition.py shows on the CPU that the cases meet
those bounds with a plain fp32 restatement and catch the wrong variants they are meant for.

Buffer discipline: inputs live at the front of a larger allocation whose tail is NaN (a read past
N rows or B queries that reaches an output shows as NaN); outputs are the front of an allocation
filled with a poison pattern: every entry must be overwritten, and the poison behind it must be
untouched bit for bit.  Each case prints its largest error / bound ratio.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _ops_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu

PAD_ROWS = 160   # more than one 128-row tile of NaN behind the corpus; > 32 behind the queries
OUT_TAIL = 4096  # poisoned floats behind every output


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _front(a, pad_rows=PAD_ROWS):
    """Device buffer holding a's rows followed by pad_rows rows of NaN."""
    import torch
    buf = torch.full((a.shape[0] + pad_rows, a.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
    buf[:a.shape[0]] = torch.from_numpy(a).cuda()
    return buf


def _poison(count):
    import torch
    return torch.full((count + OUT_TAIL,), oc.POISON_BITS - (1 << 32), dtype=torch.int32, device="cuda")


def _take(buf, count, shape):
    """Host copy of the first count floats; asserts all were written and the tail was not."""
    import torch
    torch.cuda.synchronize()
    bits = buf.cpu().numpy().view(np.uint32)
    assert (bits[count:] == oc.POISON_BITS).all(), "wrote past the end of the output"
    assert (bits[:count] != oc.POISON_BITS).all(), "left output entries unwritten"
    return bits[:count].view(np.float32).reshape(shape).copy()


def _matrix(vdb, X, Q, metric):
    xb, qb = _front(X), _front(Q)
    out = _poison(Q.shape[0] * X.shape[0])
    vdb.similarity_matrix_device(xb.data_ptr(), X.shape[0], X.shape[1], qb.data_ptr(), Q.shape[0], metric,
                                 out.data_ptr(), _stream())
    got = _take(out, Q.shape[0] * X.shape[0], (Q.shape[0], X.shape[0]))
    assert np.isfinite(got).all(), "a NaN from behind the inputs reached the output"
    return got


# =============================================================================
# A. score matrix
# =============================================================================
@pytest.mark.parametrize("metric", oc.METRICS)
@pytest.mark.parametrize("N,D,B", oc.MATRIX_SHAPES)
def test_score_matrix(vdb, N, D, B, metric):
    X, Q, roles = oc.matrix_data(N, D, B)
    got = _matrix(vdb, X, Q, metric)
    ref, bound = oc.matrix_reference(X, Q, metric)
    err = np.abs(got.astype(np.float64) - ref)
    r = oc.ratio(err, bound)
    print(f"\nRATIO matrix {metric} N={N} D={D} B={B}: {r:.3f}")
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), f"error / bound = {r:.3f}, worst at (query, row) = {worst}"
    if metric == "cosine" and D <= 768:
        assert err.max() <= oc.COSINE_HEADER_ATOL
    if metric == "euclidean" and "equal_row" in roles:
        assert got[roles["equal_query"], roles["equal_row"]] == 0.0


def test_euclidean_near_rows_by_direct_differences(vdb):
    X, Q = oc.near_rows()
    got = _matrix(vdb, X, Q, "euclidean")
    ref, bound = oc.matrix_reference(X, Q, "euclidean")
    err = np.abs(got.astype(np.float64) - ref)
    d = np.arange(oc.NEAR_N)
    print(f"\nRATIO matrix euclidean near rows D={oc.NEAR_D}: {oc.ratio(err[d, d], bound[d, d]):.3f} "
          f"(all pairs {oc.ratio(err, bound):.3f})")
    assert (err <= bound).all()


# =============================================================================
# B. normalise
# =============================================================================
@pytest.mark.parametrize("n,D", oc.NORMALIZE_SHAPES)
def test_normalize_rows(vdb, n, D):
    import torch
    x, roles = oc.normalize_data(n, D)
    xb = _front(x)
    out = _poison(n * D)
    vdb.normalize_rows_device(xb.data_ptr(), n, D, out.data_ptr(), _stream())
    got = _take(out, n * D, (n, D))
    assert np.isfinite(got).all()
    ref, bound = oc.normalize_reference(x)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"\nRATIO normalize n={n} D={D}: {oc.ratio(err, bound):.3f}")
    assert (err <= bound).all(), f"error / bound = {oc.ratio(err, bound):.3f}"
    if "zero_row" in roles:
        assert not got[roles["zero_row"]].any()
    # in == out: the same bytes as out of place, and the NaN rows behind stay as they were
    vdb.normalize_rows_device(xb.data_ptr(), n, D, xb.data_ptr(), _stream())
    torch.cuda.synchronize()
    inplace = xb.cpu().numpy()
    assert inplace[:n].tobytes() == got.tobytes()
    assert np.isnan(inplace[n:]).all()


# =============================================================================
# C. top-k
# =============================================================================
def _topk(vdb, sd, rows, n, k, largest, with_values):
    import torch
    oi = torch.full((rows * k + 64,), oc.POISON_IDX, dtype=torch.int64, device="cuda")
    ov = torch.full((rows * k + 64,), float("nan"), dtype=torch.float32, device="cuda")
    vdb.topk_scores_device(sd.data_ptr(), rows, n, k, largest, oi.data_ptr(), ov.data_ptr() if with_values else 0,
                           _stream())
    torch.cuda.synchronize()
    idx, val = oi.cpu().numpy(), ov.cpu().numpy()
    assert (idx[rows * k:] == oc.POISON_IDX).all() and np.isnan(val[rows * k:]).all(), "wrote past the end"
    if not with_values:
        assert np.isnan(val).all(), "out_values was NULL"
    return idx[:rows * k].reshape(rows, k), val[:rows * k].reshape(rows, k)


@pytest.mark.parametrize("largest", [True, False], ids=["largest", "smallest"])
@pytest.mark.parametrize("c", oc.TOPK_CASES, ids=[oc.topk_id(c) for c in oc.TOPK_CASES])
def test_topk_scores(vdb, c, largest):
    import torch
    s = oc.topk_scores(c, largest)
    rows, n = s.shape
    want = oc.topk_oracle(s, max(c["ks"]), largest)
    want_val = np.take_along_axis(s, want, axis=1)
    sd = _front(s, pad_rows=1)
    for k in c["ks"]:
        for with_values in (True, False):
            idx, val = _topk(vdb, sd, rows, n, k, largest, with_values)
            what = f"k={k} values={with_values}"
            assert (idx >= 0).all() and (idx < n).all(), what
            np.testing.assert_array_equal(idx, want[:, :k], err_msg=what)
            if with_values:  # the raw scores, NaN and the sign of zero included
                np.testing.assert_array_equal(val.view(np.uint32), want_val[:, :k].view(np.uint32), err_msg=what)
                np.testing.assert_array_equal(val, want_val[:, :k])  # (equal_nan: numpy's default)
    if c["family"] in ("constant", "all_nan"):
        assert (want == np.arange(max(c["ks"]))).all()


# =============================================================================
# D. argument checks (host side: nothing is launched)
# =============================================================================
def test_argument_checks(vdb):
    import torch
    lib = vdb.load_library()
    x = torch.ones((4, 8), dtype=torch.float32, device="cuda")
    out = _poison(64)
    oi = torch.full((64,), oc.POISON_IDX, dtype=torch.int64, device="cuda")
    P = ctypes.c_void_p
    xp, op, ip = x.data_ptr(), out.data_ptr(), oi.data_ptr()
    INV, UNS = vdb.VDB_ERR_INVALID, vdb.VDB_ERR_UNSUPPORTED

    def sim(c=xp, n=4, d=8, q=xp, b=4, m=0, o=op):
        return lib.vdb_similarity_matrix(P(c or None), n, d, P(q or None), b, m, P(o or None), None)

    def norm(i=xp, n=4, d=8, o=op):
        return lib.vdb_normalize_rows(P(i or None), n, d, P(o or None), None)

    def topk(s=xp, rows=4, n=8, k=3, o=ip):
        return lib.vdb_topk_scores(P(s or None), rows, n, k, 1, P(o or None), None, None)

    assert sim(c=0) == INV and sim(q=0) == INV and sim(o=0) == INV
    assert sim(n=-1) == INV and sim(d=0) == INV and sim(b=0) == INV
    assert sim(m=3) == UNS and sim(m=-1) == UNS
    assert sim(n=0) == vdb.VDB_OK  # an empty corpus: nothing to write
    assert norm(i=0) == INV and norm(o=0) == INV and norm(n=-1) == INV and norm(d=0) == INV
    assert topk(s=0) == INV and topk(o=0) == INV
    assert topk(rows=0) == INV and topk(rows=-1) == INV and topk(n=0) == INV and topk(n=-1) == INV
    assert topk(k=0) == INV and topk(k=-1) == INV and topk(k=9) == INV       # k > n
    big = torch.zeros(2048, dtype=torch.float32, device="cuda")
    assert lib.vdb_topk_scores(P(big.data_ptr()), 1, 2048, 1025, 1, P(ip), None, None) == INV  # k > 1024
    torch.cuda.synchronize()
    # none of the refused calls, nor the empty one, wrote anything
    assert (out.cpu().numpy().view(np.uint32) == oc.POISON_BITS).all()
    assert (oi.cpu().numpy() == oc.POISON_IDX).all()

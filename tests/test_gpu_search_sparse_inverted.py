"""The inverted (term-major) sparse kernel (csrc/vdb_sparse_inv.hip) behind vdb_index_search_sparse and
the sparse list of vdb_index_search_hybrid, chosen by the knob "sparse_inverted" (1 = whenever postings
exist, 2 = never, 0 = by the row count).

It must give the row-major kernel's result in every byte, so every case compares every output with
the literal oracle of tests/_sparse_cases.py BIT FOR BIT, in host and in device memory, through the
call helpers of tests/test_gpu_search_sparse.py (guard regions included).  No tolerance appears anywhere.

Shapes: rows around a wave's quarter of a row block and around a block for both block sizes (8192
rows, and 4096 at k = 1024: quarters of 2048 and 1024), three blocks and a few rows; 1, 2 and 7
workgroups per query, so that a workgroup loops over blocks and the merge tail runs.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_search_sparse as ts  # noqa: E402

sp, fc = ts.sp, ts.fc
vdb = ts.vdb
pytestmark = pytest.mark.gpu

INV = ("sparse_inverted_searches", "sparse_inverted_queries")
STATS = ts.STATS + INV
MAX_TERMS = 1 << 22  # csrc/vdb_sparse_inv_plan.h kSparseInvMaxTerms


def _index(vdb, n, col, knob=1, built=1, **kw):
    ix, V, Q = ts._index(vdb, n, col=col, **kw)
    ix.set_param("sparse_inverted", knob)
    assert ix.stat("sparse_inverted_built") == built
    return ix, V, Q


def _moved(ix, before):
    return {s: ix.stat(s) - before[s] for s in STATS if ix.stat(s) != before[s]}


@pytest.mark.parametrize("n", (1, 65, 2047, 2049, 4095, 4097, 8193, 3 * 8192 + 5))
def test_block_and_wave_boundaries(vdb, n):
    base = sp.column(n, 30522)
    # term 0 in every row (its postings cross every block), term 1 in none, the other entries as the case has them
    col = sp.Column([(np.r_[0, t[t > 1]], np.r_[1.5, w[t > 1]]) for t, w in base.rows], 30522)
    none = np.ones(1, np.int32)
    q = sp.queries(30522)
    qs = [q[3], q[1], (none, np.ones(1, np.float32)), (np.zeros(1, np.int32), np.full(1, 2.0, np.float32)), q[0]]
    assert qs[0][0].size == 1024 and qs[1][0].size == 0 and not (col.terms == 1).any()
    ix, V, Q = _index(vdb, n, col)
    full = sp.expected(col, qs, 1024)
    assert (full[1][2] == -1).all() and (full[1][3][:min(n, 1024)] >= 0).all()
    for wgs in (1, 2, 7):
        ix.set_param("sparse_wgs", wgs)
        for k in (1, 10, 1024):
            before = {s: ix.stat(s) for s in STATS}
            ts._check(ix, col, qs, k, what=f"n {n} wgs {wgs}", want=tuple(x[:, :k] for x in full))
            assert _moved(ix, before) == {"sparse_searches": 2, "sparse_queries": 10, INV[0]: 2, INV[1]: 10}
    ix.close()


@pytest.mark.parametrize("case", ("ties", "signed", "zero_key", "beyond", "edge_5", "edge_30522", "mask_and_offset"))
def test_edge_cases_through_the_inverted_kernel(vdb, case):
    if case == "mask_and_offset":
        col, qs = sp.column(300, 30522), sp.queries(30522)
    else:
        col, qs = {"ties": sp.tie_case, "signed": sp.signed_case, "zero_key": sp.zero_key_case, "beyond": sp.beyond_case,
                   "edge_5": lambda: sp.edge_terms_case(5), "edge_30522": lambda: sp.edge_terms_case(30522)}[case]()
    ix, V, Q = _index(vdb, col.n, col)
    before = ix.stat(INV[0])
    for wgs in (1, 7):
        ix.set_param("sparse_wgs", wgs)
        if case == "mask_and_offset":
            half = np.random.default_rng(6).random(300) < 0.5
            ts._check(ix, col, qs, 10, mask=np.zeros(300, bool), what="no eligible row")
            ts._check(ix, col, qs, 400, mask=half, words=fc.bitmap_words(half, extra_bits=52), what="mask bits past count")
            ts._check(ix, col, qs, 400, index_offset=2 ** 40, what="offset 2^40")
        else:
            for k in (1, 10, 11, 1024):
                ts._check(ix, col, qs, k, what=f"{case} wgs {wgs}")
    assert ix.stat(INV[0]) > before
    ix.close()


@pytest.mark.parametrize("metric", ts.METRICS)
def test_same_bytes_whatever_the_kernel(vdb, metric):
    col, qs = sp.column(513, 30522), sp.queries(30522)
    mask = np.random.default_rng(3).random(513) < 0.5
    want, want_m = sp.expected(col, qs, 50), sp.expected(col, qs, 50, mask)
    for prec in ("auto", "fp32"):
        ix, V, Q = _index(vdb, 513, col, metric=metric, precision=prec)
        got = {}
        for knob in (1, 2):
            ix.set_param("sparse_inverted", knob)
            before = {s: ix.stat(s) for s in STATS}
            got[knob] = (ts._check(ix, col, qs, 50, what=f"{metric} {prec} knob {knob}", want=want),
                         ts._check(ix, col, qs, 50, mask=mask, what=f"{metric} {prec} knob {knob} masked", want=want_m))
            inv = {INV[0]: 4, INV[1]: 20} if knob == 1 else {}
            assert _moved(ix, before) == {"sparse_searches": 4, "sparse_queries": 20, **inv}
        for a, b in zip(got[1], got[2]):
            ts._same(a, b, "knob 1 against knob 2")
        ix.close()


def test_hybrid_takes_its_sparse_list_from_the_inverted_kernel(vdb):
    n = 1300
    col, qs = sp.tie_case(n)
    ix, V, Q = _index(vdb, n, col)
    ix.set_param("sparse_wgs", 2)
    mask = np.random.default_rng(12).random(n) < 0.5
    want = sp.expected_hybrid(V, Q[:2], col, qs, 50, 200, "cosine", (1.0, 2.0), mask=mask, index_offset=2 ** 40)
    before = {s: ix.stat(s) for s in STATS}
    words = fc.bitmap_words(mask)
    code, got = ts._call_hybrid(ix, Q[:2], qs, 50, 200, (1.0, 2.0), mask=words, index_offset=2 ** 40)
    assert code == 0
    ts._same(got, want, "hybrid host")
    ts._same(ts._call_hybrid_device(ix, Q[:2], qs, 50, 200, (1.0, 2.0), mask=words, index_offset=2 ** 40), want, "hybrid device")
    moved = _moved(ix, before)  # the sparse list came from the inverted kernel; hybrid calls count no sparse search
    assert "sparse_searches" not in moved and "sparse_bad_queries" not in moved, moved
    assert [moved[x] for x in ("hybrid_searches", "hybrid_queries") + INV] == [2, 4, 2, 4], moved
    ix.close()


def test_device_memory_garbage_is_answered_per_query(vdb):
    import torch
    col, qs = sp.column(513, 30522), sp.queries(30522)
    ix, V, Q = _index(vdb, 513, col)
    csr, nnz, bad, good = ts._garbage(qs, 30522)
    for wgs in (1, 2):
        ix.set_param("sparse_wgs", wgs)
        before = {s: ix.stat(s) for s in ("sparse_bad_queries",) + INV}
        s, i, k = ts._call_device(ix, None, 10, csr=csr, q_nnz=nnz)
        torch.cuda.synchronize()
        assert [ix.stat(x) - before[x] for x in before] == [len(bad), 1, 11]
        for b in range(11):
            one = (s[b:b + 1], i[b:b + 1], k[b:b + 1])
            if b in bad:
                assert (one[1] == -1).all() and (one[0] == 0).all() and np.isneginf(one[2]).all(), b
            else:
                ts._same(one, sp.expected(col, [good[b]], 10), f"good query {b} beside bad ones")
    ts._check(ix, col, qs, 10, what="after the bad input")
    ix.close()


def test_lifetime_and_choice(vdb):
    col, other, qs = sp.column(37, 30522), sp.column(37, 30522, seed=5), sp.queries(30522)
    want = sp.expected(col, qs, 10)
    ix, V, Q = ts._index(vdb, 37, col=col)
    assert ix.stat("sparse_inverted_built") == 1

    def served(inverted, what, c=col, w=want):
        before = {s: ix.stat(s) for s in INV}
        ts._check(ix, c, qs, 10, want=w, what=what, device=False)
        assert [ix.stat(s) - before[s] for s in INV] == ([1, 5] if inverted else [0, 0]), what

    served(False, "auto, a small index: the row-major kernel")
    for bad in (-1, 3):
        assert ix._lib.vdb_index_set_param(ix._h, b"sparse_inverted", bad) == ts.VDB_ERR_INVALID
    ix.set_param("sparse_inverted", 1)
    served(True, "knob 1")
    ix.update(np.asarray([3, 5], np.int64), V[:2] * 2)
    assert ix.stat("sparse_inverted_built") == 1
    served(True, "after an update")
    f = ix._lib.vdb_index_set_sparse
    for name, ip, t, w, nt, err in ts._bad_columns(other):
        ip, t, w = (np.ascontiguousarray(x) for x in (ip, t, w))
        assert f(ix._h, ts._p(ip), ts._p(t), ts._p(w), ip.size - 1, t.size, nt, 0, None) == err, name
        assert ix.stat("sparse_inverted_built") == 1, name
    served(True, "after refused columns")
    # the postings are counted in device_bytes; knob 2 at attach time builds none
    with_postings = ix.stat("device_bytes")
    ix.set_param("sparse_inverted", 2)
    served(False, "knob 2")
    ix.set_sparse(other.indptr, other.terms, other.weights, other.n_terms)
    assert ix.stat("sparse_inverted_built") == 0
    assert with_postings - ix.stat("device_bytes") == 8 * (col.n_terms + 1) + 8 * col.nnz
    ix.set_param("sparse_inverted", 1)
    served(False, "knob 1 without postings", other, sp.expected(other, qs, 10))
    # a vocabulary above the cap builds none either
    big = sp.column(37, 2 ** 31 - 1)
    assert big.n_terms > MAX_TERMS
    ix.set_sparse(big.indptr, big.terms, big.weights, big.n_terms)
    assert ix.stat("sparse_inverted_built") == 0
    served(False, "a vocabulary above the cap", big, sp.expected(big, qs, 10))
    # add, remove and clear drop the postings with the column
    ix.set_sparse(col.indptr, col.terms, col.weights, col.n_terms)
    assert ix.stat("sparse_inverted_built") == 1
    ix.add(V[:1])
    assert ix.stat("sparse_inverted_built") == 0 and ts._call(ix, qs, 10)[0] == ts.VDB_ERR_INVALID
    bits = np.zeros(38, bool)
    bits[37] = True
    ix.remove(fc.bitmap_words(bits))
    ix.set_sparse(col.indptr, col.terms, col.weights, col.n_terms)
    served(True, "re-attached after add and remove")
    ix.remove(fc.bitmap_words(bits[:37] | (np.arange(37) == 36)))
    assert ix.stat("sparse_inverted_built") == 0
    ix.clear()
    assert ix.stat("sparse_inverted_built") == 0
    ix.close()

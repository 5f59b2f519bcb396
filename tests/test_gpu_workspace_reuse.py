"""One workspace serving calls of different layouts, one after another.

The main search lays its workspace out per call (csrc/vdb_search_plan.h search_layout), and the
row-list, range and grouped searches lay theirs out in the same buffer through the same lease.  A
wrong total or a wrong offset shows when a workspace sized and carved for one call is reused for a
call of another shape: a sequence of calls on one index from one thread, so one workspace serves
them all.  Every result is compared with the oracle (oracle/ref_cpu.py): indices and fp64 keys bit
for bit.  Default knobs only.
"""
import os
import sys

import numpy as np
import pytest

from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(__file__))
import _group_cases as gc  # noqa: E402
import _range_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

N, D, METRIC = 1000, 24, "cosine"
# (B, k, masked): a single query, more than one query super tile, a masked small batch, k past the
# candidate pass's limit (the exact path), and the single query again
SEQUENCE = [(1, 1, False), (130, 100, False), (3, 10, True), (130, 201, False), (1, 1, False)]


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


@pytest.fixture(scope="module")
def small():
    """(V, Q, mask, keys): the corpus of cases (a) and (c), 130 queries, a 35 % mask and the
    oracle's key of every (query, row) pair."""
    rng = np.random.default_rng(20261020)
    V = rng.standard_normal((N, D)).astype(np.float32)
    Q = rng.standard_normal((130, D)).astype(np.float32)
    Q[0] = V[N - 1]
    mask = rng.random(N) < 0.35
    keys = gc.oracle_keys(Q, V, METRIC)
    for a in (V, Q, mask, keys):
        a.setflags(write=False)
    return V, Q, mask, keys


@pytest.fixture(scope="module")
def small_oracle(small):
    V, Q, mask, _ = small
    return {(B, k, m): ref_cpu.exact_search(Q[:B], V, k, METRIC, row_mask=mask if m else None)
            for B, k, m in set(SEQUENCE)}


def _same(got, want, what):
    (s, i, kk), (es, ei, ek) = got, want
    np.testing.assert_array_equal(i, ei, err_msg=f"indices, {what}")
    valid = ei >= 0
    np.testing.assert_array_equal(kk[valid], ek[valid], err_msg=f"keys, {what}")
    np.testing.assert_array_equal(s[valid], es[valid], err_msg=f"scores, {what}")


def test_shape_sequence_host_then_device(vdb, small, small_oracle):
    import torch
    V, Q, mask, _ = small
    words = gc.bitmap_words(mask)
    ix = vdb.NativeIndex(D, METRIC)  # auto precision
    ix.add(V)
    for step, (B, k, m) in enumerate(SEQUENCE):
        got = ix.search(Q[:B], k, row_mask=words if m else None, with_keys=True)
        _same(got, small_oracle[(B, k, m)], f"host call {step}: B {B} k {k}")
    st = torch.cuda.current_stream().cuda_stream
    md = torch.from_numpy(words.view(np.int32)).cuda()
    outs = []
    for B, k, m in SEQUENCE:  # queued back to back on the current stream
        qd = torch.from_numpy(Q[:B].copy()).cuda()
        sd = torch.empty((B, k), dtype=torch.float32, device="cuda")
        idd = torch.empty((B, k), dtype=torch.int64, device="cuda")
        kd = torch.empty((B, k), dtype=torch.float64, device="cuda")
        ix.search_device(qd.data_ptr(), B, k, sd.data_ptr(), idd.data_ptr(), kd.data_ptr(),
                         mask_ptr=md.data_ptr() if m else 0, stream=st)
        outs.append((qd, sd, idd, kd))
    torch.cuda.synchronize()
    for step, ((B, k, m), (_, sd, idd, kd)) in enumerate(zip(SEQUENCE, outs)):
        _same((sd.cpu().numpy(), idd.cpu().numpy(), kd.cpu().numpy()), small_oracle[(B, k, m)],
              f"device call {step}: B {B} k {k}")
    assert ix.stat("searches") == 2 * len(SEQUENCE)
    assert ix.stat("inconsistent_queries") == 0
    ix.close()


def test_wide_long_layout_between_two_ordinary_ones(vdb):
    """66 000 rows (just past the wide pass's row threshold) of 512 dims, I8: batches of 2, 200 and 2
    all take the long-row wide pass (16 groups: every batch size up to 256), whose layout has
    segment counts and per-segment candidate lists instead of the 64-query pass's."""
    rng = np.random.default_rng(66)
    n, d, k = 66_000, 512, 10
    V = rng.random((n, d), dtype=np.float32)
    Q = rng.random((200, d), dtype=np.float32)
    Q[0] = V[n - 1]
    want = ref_cpu.exact_search(Q, V, k, METRIC)  # once: the batches of 2 are its first rows
    ix = vdb.NativeIndex(d, METRIC, precision="i8")
    ix.add(V)
    for step, B in enumerate((2, 200, 2)):
        _same(ix.search(Q[:B], k, with_keys=True), tuple(a[:B] for a in want), f"call {step}: B {B}")
    assert ix.stat("searches_wide") == 3
    assert ix.stat("inconsistent_queries") == 0
    ix.close()


def test_four_entry_points_share_one_pool(vdb, small):
    V, Q, mask, keys = small
    words = gc.bitmap_words(mask)
    groups = gc.layout("random", N)
    rng = np.random.default_rng(7)
    lists = [np.sort(rng.choice(N, size=m, replace=False)).astype(np.int64) for m in (1, 40, 700)]
    cap = 16
    thr = np.array([rc.midpoint_threshold(keys[b], (5, 16, 17, 60)[b % 4], METRIC) for b in range(Q.shape[0])])
    ix = vdb.NativeIndex(D, METRIC)
    ix.add(V)
    ix.set_groups(groups)

    def plain(B):
        _same(ix.search(Q[:B], 10, row_mask=words, with_keys=True),
              ref_cpu.exact_search(Q[:B], V, 10, METRIC, row_mask=mask), f"search B {B}")

    def rows(B):
        ql = np.arange(B) % len(lists)
        s, i, kk = ix.search_rows(Q[:B], 10, lists, query_list=ql, with_keys=True)
        for li, members in ((li, np.nonzero(ql == li)[0]) for li in range(len(lists))):
            if members.size:
                m = np.zeros(N, bool)
                m[lists[li]] = True
                _same((s[members], i[members], kk[members]), ref_cpu.exact_search(Q[members], V, 10, METRIC, row_mask=m),
                      f"search_rows B {B} list {li}")

    def rng_(B):
        c, i, s, kk = ix.search_range(Q[:B], thr[:B], cap=cap, row_mask=words, with_keys=True)
        ec, ei, es, ek = rc.expected(keys[:B], rc.kt_of(METRIC, thr[:B]), cap, METRIC, mask=mask)
        np.testing.assert_array_equal(c, ec, err_msg=f"range counts B {B}")
        _same((s, i, kk), (es, ei, ek), f"search_range B {B}")

    def grouped(B):
        s, i, g, kk = ix.search_groups(Q[:B], 5, row_mask=words, with_keys=True)
        es, ei, eg, ek = gc.expected(keys[:B], groups, 5, METRIC, mask=mask)
        np.testing.assert_array_equal(g, eg, err_msg=f"groups B {B}")
        _same((s, i, kk), (es, ei, ek), f"search_groups B {B}")

    for call, B in ((plain, 2), (rows, 130), (rng_, 2), (grouped, 130), (plain, 130), (rows, 2), (rng_, 130), (grouped, 2)):
        call(B)
    # (a grouped search counts once in "searches" too: its inner fetch is a search)
    assert ix.stat("searches") == 2 + 2
    assert ix.stat("subset_searches") == 2
    assert ix.stat("range_searches") == 2
    assert ix.stat("group_searches") == 2
    assert ix.stat("inconsistent_queries") == 0
    ix.close()

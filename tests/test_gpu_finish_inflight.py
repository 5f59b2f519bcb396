"""The finish kernel's load schedule (vdb_exact.hip finish_kernel): the per-query scalars, the
query row and the rounding residual are requested at the top of the kernel, the refinement's and
the exact keys' row loads run a batch ahead of the reduction, and a segment's first four entry
slots are read with its count.  None of that may change a result or request a row that was not
validated, so the shapes here are the smallest at which the schedule can go wrong:

  * fewer candidates than a batch, than k, or none (tiny corpora, masks that leave 0, 1 and k - 1
    eligible rows), batches of 1, 3 and 64;
  * every form and switch: the 4-, 8- and 16-wave forms, the refinement on and off, one and two
    workgroups per query, both metrics;
  * planted-gap data (tests/_planted.py) on which every query MUST certify unaided, with its CPU
    precondition repeated here as tests/test_planted_precondition.py does for the matrix;
  * one index searched again and again on three streams, as the benchmark does.

Results are compared bit for bit with oracle/ref_cpu.exact_search (indices, fp64 keys, scores).
"""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # tests/_planted.py, under any pytest import mode
import _planted as pl  # noqa: E402

gpu = pytest.mark.gpu
K = 10


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def _words(mask):
    n = mask.size
    bits = np.zeros(((n + 31) // 32) * 32, bool)
    bits[:n] = mask
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _random(N, D, B, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((N, D)).astype(np.float32)
    Q = rng.standard_normal((B, D)).astype(np.float32)
    Q[0] = V[N // 2]  # an exact duplicate of a row
    for a in (V, Q):
        a.setflags(write=False)
    return V, Q


@functools.lru_cache(maxsize=None)
def _expected(N, D, B, seed, metric, eligible):
    """The oracle's answer, once per data set, metric and mask (eligible: None = every row, else
    the number of eligible rows, the first ones of a fixed permutation)."""
    V, Q = _random(N, D, B, seed)
    mask = None
    if eligible is not None:
        mask = np.zeros(N, bool)
        mask[np.random.default_rng(seed + 1).permutation(N)[:eligible]] = True
        mask.setflags(write=False)
    out = ref_cpu.exact_search(Q, V, K, metric, row_mask=mask)
    for a in out:
        a.setflags(write=False)
    return mask, out


def _check(ix, Q, mask, want, what):
    s, i, kk = ix.search(Q, K, row_mask=_words(mask) if mask is not None else None, with_keys=True)
    es, ei, ek = (a[:Q.shape[0]] for a in want)
    np.testing.assert_array_equal(i, ei, err_msg=f"indices, {what}")
    valid = ei >= 0
    np.testing.assert_array_equal(kk[valid], ek[valid], err_msg=f"keys, {what}")
    np.testing.assert_array_equal(s[valid], es[valid], err_msg=f"scores, {what}")
    assert ix.stat("inconsistent_queries") == 0, what


# ---- fewer candidates than a batch, than k, or none ------------------------------------------------

@gpu
@pytest.mark.parametrize("small", [0, 1])
@pytest.mark.parametrize("D", [768, 96])
@pytest.mark.parametrize("N", [1, 7, 33, 300])
def test_few_candidates(vdb, N, D, small):
    """Cosine I8 through the wide pass: lists of fewer entries than a refinement or exact-key batch
    (m < NB), than k (no cut, no refinement: the prefetched rows are masked off) and of none."""
    seed = 1000 + N + D
    ix = vdb.NativeIndex(D, "cosine", precision="i8")
    ix.set_param("scan_wide", 1)
    ix.set_param("finish_small", small)
    ix.set_param("i8_refine", 1)
    V, Q = _random(N, D, 64, seed)
    ix.add(V)
    searches = 0
    for eligible in (None, 0, 1, K - 1):
        if eligible is not None and eligible > N:
            continue
        mask, want = _expected(N, D, 64, seed, "cosine", eligible)
        for B in (1, 3, 64):
            before = {n: ix.stat(n) for n in ("fallback_queries", "overflow_queries")}
            _check(ix, Q[:B], mask, want, f"N {N} D {D} B {B} eligible {eligible} small {small}")
            searches += 1
            # every search went through the int8 wide pass, so the finish kernel saw its lists
            assert ix.stat("searches") == searches
            assert ix.stat("searches_i8") == searches and ix.stat("searches_wide") == searches
            # A corpus of fewer than 256 row tiles gets no pilot bound, so the lists hold every
            # eligible row, and no segment holds more than one 32-row tile.  With at most KP = 256
            # entries the finish then needs no certificate (fewer than k: it writes what there is):
            # nothing may overflow or go to the exact path.  Only the unmasked 300 rows, more than
            # KP, need the certificate; their count is printed.
            fell = ix.stat("fallback_queries") - before["fallback_queries"]
            over = ix.stat("overflow_queries") - before["overflow_queries"]
            print(f"N {N} D {D} B {B} eligible {eligible} small {small}: fallbacks {fell} overflow {over}")
            assert over == 0
            if N <= 256 or eligible is not None:
                assert fell == 0
    ix.close()


# ---- every form and switch -------------------------------------------------------------------------

def _forms():
    out = []
    for small in (0, 1):  # the 16- and the 4-wave form
        for refine in (0, 1):
            for split in (1, 2):
                out.append((5000, 768, "cosine", small, refine, split))
                if refine:  # forced on at 96 dims it also covers L2
                    out.append((4000, 96, "cosine", small, refine, split))
                    out.append((4000, 96, "euclidean", small, refine, split))
        out.append((4000, 96, "euclidean", small, 0, 1))
    for metric in ("cosine", "euclidean"):  # the 8-wave form
        for refine in (0, 1):
            for split in (1, 2):
                out.append((4000, 1090, metric, 0, refine, split))
    out.append((8000, 768, "euclidean", 0, 1, 1))
    # rows past the 8-wave form's LDS copy of the residual (2048 dims): the refinement reads it from
    # memory, three 1024-dim chunks a row, and the exact keys take the generic loop
    for metric in ("cosine", "euclidean"):
        out.append((3000, 2100, metric, 0, 1, 1))
    return out


@gpu
@pytest.mark.parametrize("N,D,metric,small,refine,split", _forms())
def test_every_form_and_switch(vdb, N, D, metric, small, refine, split):
    seed = 2000 + N + D
    V, Q = _random(N, D, 64, seed)
    ix = vdb.NativeIndex(D, metric, precision="i8")
    ix.set_param("finish_small", small)
    ix.set_param("i8_refine", refine)
    ix.set_param("finish_split", split)
    ix.add(V)
    mask, want = _expected(N, D, 64, seed, metric, None)
    _check(ix, Q, mask, want, f"{metric} D {D} small {small} refine {refine} split {split}")
    mask, want = _expected(N, D, 64, seed, metric, N // 3)
    _check(ix, Q[:5], mask, want, f"{metric} D {D} small {small} refine {refine} split {split}, masked")
    assert ix.stat("searches_i8") == 2
    ix.close()


# ---- the planted-gap bar ---------------------------------------------------------------------------

def _planted_cases():
    out = []
    for B in (1, 3, 31, 64, 127):
        for fs in (0, 1):
            out.append(pl._case("fin_long", 8000, 768, B, K, "cosine", "i8",
                                {"scan_wide": 1, "pilot_rank": 11, "finish_small": fs}, wide=1))
    for metric in pl.BOTH:
        for B in (3, 127, 129):
            out.append(pl._case("fin_short", 6000, 96, B, K, metric, "i8"))
    return out


PLANTED = _planted_cases()


def _planted_datasets():
    seen = {}
    for c in PLANTED:
        seen.setdefault((c["N"], c["D"], c["B"], c["k"], c["seed"], c["metric"]), c)
    return list(seen)


@pytest.mark.parametrize("key", _planted_datasets(), ids=lambda k: f"N{k[0]}-D{k[1]}-B{k[2]}-{k[5]}")
def test_planted_precondition(key):
    """On the CPU, against the reference arithmetic alone: the planted rows are the exact top k, the
    smallest gap is at least 6 eps_upper, and no query has more than 3 planted rows in one of the
    wide pass's 256 segments (so a segment's first four slots hold them all)."""
    N, D, B, k, seed, metric = key
    assert seed == N + 3 * D + 5 * B + 7 * k
    V, Q, pos = pl.data(N, D, B, k, seed)
    es, ei, ek, gap = pl.oracle(N, D, B, k, seed, metric)
    np.testing.assert_array_equal(np.sort(ei, axis=1), np.sort(pos, axis=1))
    ratio = float((gap / pl.eps_upper(V, Q, metric, "i8")).min())
    worst = pl.max_planted_in_segment(pos, 256)
    print(f"N {N} D {D} B {B} {metric}: min gap / eps = {ratio:.1f}, at most {worst} planted rows in a segment")
    assert ratio >= 6.0, ratio
    assert worst <= 3, worst


def _assert_unaided(ix):
    st = {n: ix.stat(n) for n in ("fallback_queries", "overflow_queries", "inconsistent_queries", "repass_queries")}
    assert all(v == 0 for v in st.values()), st


@gpu
@pytest.mark.parametrize("c", PLANTED, ids=[pl.case_id(c) for c in PLANTED])
def test_planted_rows_certify_unaided(vdb, c):
    V, Q, _ = pl.data(c["N"], c["D"], c["B"], c["k"], c["seed"])
    es, ei, ek, _ = pl.oracle(c["N"], c["D"], c["B"], c["k"], c["seed"], c["metric"])
    ix = vdb.NativeIndex(c["D"], c["metric"], precision=c["precision"])
    for name, value in c["params"].items():
        ix.set_param(name, value)
    ix.add(V)
    s, i, kk = ix.search(Q, c["k"], with_keys=True)
    np.testing.assert_array_equal(i, ei)
    np.testing.assert_array_equal(kk, ek)
    np.testing.assert_array_equal(s, es)
    _assert_unaided(ix)
    assert ix.stat("searches_i8") == 1 and ix.stat("searches_wide") == c["wide"]
    ix.close()


# ---- reuse of a workspace --------------------------------------------------------------------------

@gpu
def test_twelve_searches_on_three_streams(vdb):
    """The benchmark's loop: one index, device-memory searches queued round-robin on three streams
    (a batch's finish then runs beside the next batch's scan, in its 4-wave form).  Every output
    equals the first, and the first the oracle's."""
    import torch
    N, D, B = 20_000, 768, 64
    V, Q = _random(N, D, B, 3000)
    _, (es, ei, ek) = _expected(N, D, B, 3000, "cosine", None)
    ix = vdb.NativeIndex(D, "cosine", precision="i8")
    ix.set_param("scan_wide", 1)
    ix.add(V)
    qd = torch.from_numpy(np.array(Q)).cuda()
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(2)]
    outs = [(torch.empty((B, K), dtype=torch.float32, device="cuda"),
             torch.empty((B, K), dtype=torch.int64, device="cuda"),
             torch.empty((B, K), dtype=torch.float64, device="cuda")) for _ in range(12)]
    torch.cuda.synchronize()
    for n, (sd, idd, kd) in enumerate(outs):
        ix.search_device(qd.data_ptr(), B, K, sd.data_ptr(), idd.data_ptr(), kd.data_ptr(),
                         stream=streams[n % 3].cuda_stream)
    torch.cuda.synchronize()
    got = [(sd.cpu().numpy(), idd.cpu().numpy(), kd.cpu().numpy()) for sd, idd, kd in outs]
    np.testing.assert_array_equal(got[0][1], ei)
    np.testing.assert_array_equal(got[0][2], ek)
    np.testing.assert_array_equal(got[0][0], es)
    for n, (s, i, kk) in enumerate(got[1:], 1):
        np.testing.assert_array_equal(i, got[0][1], err_msg=f"indices, search {n}")
        np.testing.assert_array_equal(kk, got[0][2], err_msg=f"keys, search {n}")
        np.testing.assert_array_equal(s, got[0][0], err_msg=f"scores, search {n}")
    assert ix.stat("searches") == 12
    assert ix.stat("inconsistent_queries") == 0
    ix.close()

#!/usr/bin/env python3
"""What vdb_index_search_sparse and vdb_index_search_hybrid cost: on 1M rows of about
64 sparse entries each (and 128-dim cosine dense rows for the hybrid call), vocabularies of 30 522 and
250 002 terms, batches of 1 and 64 queries of 32 terms, k = 10 (hybrid: fetch_k = 40), the time per
call of
  1. ``search_sparse`` (host memory, complete on return),
  2. ``search_hybrid``,
each the median of repeated calls after warm-up with their range, and for the sparse call the CSR
bytes the kernel reads per second (every row's offsets and (term, weight) pairs, once per query)
against the HBM figure DESIGN.md uses.  One JSON line per measurement.

``--inverted`` measures the two kernels behind ``search_sparse`` against each other instead (DESIGN.md
§21.1): at 10^4, 10^5 and 10^6 rows, both vocabularies, batches of 1 and 64 and queries of 32 and
1 024 terms, the knob "sparse_inverted" at 2 (the row-major kernel, the baseline) and at 1 (the
inverted kernel) alternating in one process; every argument in device memory, device events around a
window of back-to-back calls after warm-up, the median of ``--windows`` windows with their range; the
two results must be equal in every byte.  Beside each, the host-memory call's wall time as above, and
per column the ``set_sparse`` time without and with the postings build.

Run it under a time limit of its own (``timeout -k 10 600 python tools/sparse_bench.py``).

  python tools/sparse_bench.py [--rows 1000000] [--entries 64] [--reps 15] [--out FILE]
  python tools/sparse_bench.py --inverted [--inverted-rows 10000 100000 1000000] [--windows 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

DIM, METRIC = 128, "cosine"
K, FETCH, QUERY_TERMS = 10, 40, 32
HBM_GBPS = 8000.0  # the peak DESIGN.md measures bandwidth against


def _stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(1e3 * ts[len(ts) // 2], 4), "min_ms": round(1e3 * ts[0], 4),
            "max_ms": round(1e3 * ts[-1], 4), "runs": len(ts)}


def _timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return _stats(ts)


def column(rows, entries, n_terms, rng):
    """About ``entries`` terms per row, Zipf-like over the vocabulary, ascending within a row."""
    # `entries` power-law draws per row, sorted within the row, repeats dropped
    t = np.minimum((n_terms * rng.random((rows, entries), dtype=np.float32) ** 3).astype(np.int32), n_terms - 1)
    t.sort(axis=1)
    keep = np.ones(t.shape, bool)
    keep[:, 1:] = t[:, 1:] != t[:, :-1]
    indptr = np.zeros(rows + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    terms = t[keep].astype(np.int32)
    weights = (0.1 + rng.random(terms.size)).astype(np.float32)
    return indptr, terms, weights


def queries(B, n_terms, rng, length=QUERY_TERMS):
    ts, ws = [], []
    for _ in range(B):
        t = np.unique(np.minimum((n_terms * rng.random(length) ** 3).astype(np.int64), n_terms - 1)).astype(np.int32)
        ts.append(t)
        ws.append((0.1 + rng.random(t.size)).astype(np.float32))
    indptr = np.zeros(B + 1, np.int64)
    np.cumsum([t.size for t in ts], out=indptr[1:])
    return indptr, np.concatenate(ts), np.concatenate(ws)


def inverted(args, emit):
    import torch
    from service import _vdb
    rng = np.random.default_rng(0)
    for rows in args.inverted_rows:
        ix = _vdb.NativeIndex(DIM, METRIC)
        ix.add(rng.standard_normal((rows, DIM)).astype(np.float32))
        for n_terms in (30522, 250002):
            indptr, terms, weights = column(rows, args.entries, n_terms, rng)
            for knob in (2, 0):  # without and with the postings build
                ix.set_param("sparse_inverted", knob)
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    ix.set_sparse(indptr, terms, weights, n_terms)
                    ts.append(time.perf_counter() - t0)
                emit({"what": "set_sparse", "postings": ix.stat("sparse_inverted_built"), "n_terms": n_terms, "rows": rows,
                      "nnz": int(terms.size), "ms": round(1e3 * sorted(ts)[1], 2), "device_bytes": ix.stat("device_bytes")})
            for length in (32, 1024):
                for B in (1, 64):
                    qi, qt, qw = queries(B, n_terms, rng, length)
                    dqi, dqt, dqw = (torch.from_numpy(x).to("cuda") for x in (qi, qt, qw))
                    ds = torch.empty((B, K), dtype=torch.float32, device="cuda")
                    di = torch.empty((B, K), dtype=torch.int64, device="cuda")
                    dk = torch.empty((B, K), dtype=torch.float64, device="cuda")
                    st = torch.cuda.current_stream().cuda_stream

                    def call():
                        ix.search_sparse_device(dqi.data_ptr(), dqt.data_ptr(), dqw.data_ptr(), B, int(qt.size), K,
                                                ds.data_ptr(), di.data_ptr(), out_keys_ptr=dk.data_ptr(), stream=st)

                    base = None
                    for knob in (2, 1):
                        ix.set_param("sparse_inverted", knob)
                        before = ix.stat("sparse_inverted_queries")
                        for _ in range(3):
                            call()
                        torch.cuda.synchronize()
                        assert ix.stat("sparse_inverted_queries") - before == (3 * B if knob == 1 else 0), "not the kernel asked for"
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(); call(); e1.record(); torch.cuda.synchronize()
                        per = max(int(100.0 / max(e0.elapsed_time(e1), 1e-3)), 5)  # calls per window: about 0.1 s
                        ws = []
                        for _ in range(args.windows):
                            e0.record()
                            for _ in range(per):
                                call()
                            e1.record()
                            torch.cuda.synchronize()
                            ws.append(e0.elapsed_time(e1) / per)
                        ws.sort()
                        host = _timed(lambda: ix.search_sparse(qi, qt, qw, K), 5, warm=1)
                        rec = {"what": "search_sparse", "kernel": "rows" if knob == 2 else "inverted", "rows": rows,
                               "n_terms": n_terms, "query_terms": length, "B": B, "k": K, "mem": "device",
                               "median_ms": round(ws[len(ws) // 2], 4), "min_ms": round(ws[0], 4), "max_ms": round(ws[-1], 4),
                               "windows": len(ws), "calls_per_window": per, "host_call_median_ms": host["median_ms"]}
                        got = tuple(x.cpu().numpy().copy() for x in (ds, di, dk))
                        if knob == 2:
                            base = got
                        else:
                            rec["equal_to_rows"] = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, base))
                        emit(rec)
        ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inverted", action="store_true", help="the two kernels against each other (DESIGN.md §21.1)")
    ap.add_argument("--inverted-rows", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--entries", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from service import _vdb
    rng = np.random.default_rng(0)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    if args.inverted:
        inverted(args, emit)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    V = rng.standard_normal((args.rows, DIM)).astype(np.float32)
    ix = _vdb.NativeIndex(DIM, METRIC)
    ix.add(V)
    for n_terms in (30522, 250002):
        indptr, terms, weights = column(args.rows, args.entries, n_terms, rng)
        t0 = time.perf_counter()
        ix.set_sparse(indptr, terms, weights, n_terms)
        emit({"what": "set_sparse", "n_terms": n_terms, "rows": args.rows, "nnz": int(terms.size),
              "ms": round(1e3 * (time.perf_counter() - t0), 2)})
        csr_bytes = terms.size * 8 + (args.rows + 1) * 8
        for B in (1, 64):
            qi, qt, qw = queries(B, n_terms, rng)
            Q = rng.standard_normal((B, DIM)).astype(np.float32)
            s = _timed(lambda: ix.search_sparse(qi, qt, qw, K), args.reps)
            s.update({"what": "search_sparse", "n_terms": n_terms, "B": B, "k": K, "rows": args.rows,
                      "csr_gb_per_s": round(B * csr_bytes / (s["median_ms"] * 1e-3) / 1e9, 1),
                      "of_hbm": round(B * csr_bytes / (s["median_ms"] * 1e-3) / 1e9 / HBM_GBPS, 4)})
            emit(s)
            h = _timed(lambda: ix.search_hybrid(Q, qi, qt, qw, K, FETCH), args.reps)
            h.update({"what": "search_hybrid", "n_terms": n_terms, "B": B, "k": K, "fetch_k": FETCH, "rows": args.rows})
            emit(h)
            d = _timed(lambda: ix.search(Q, FETCH), args.reps)
            d.update({"what": "search (the hybrid call's dense list alone)", "B": B, "k": FETCH, "rows": args.rows})
            emit(d)
    ix.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

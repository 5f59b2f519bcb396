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

Run it under a time limit of its own (``timeout -k 10 600 python tools/sparse_bench.py``).

  python tools/sparse_bench.py [--rows 1000000] [--entries 64] [--reps 15] [--out FILE]
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


def queries(B, n_terms, rng):
    ts, ws = [], []
    for _ in range(B):
        t = np.unique(np.minimum((n_terms * rng.random(QUERY_TERMS) ** 3).astype(np.int64), n_terms - 1)).astype(np.int32)
        ts.append(t)
        ws.append((0.1 + rng.random(t.size)).astype(np.float32))
    indptr = np.zeros(B + 1, np.int64)
    np.cumsum([t.size for t in ts], out=indptr[1:])
    return indptr, np.concatenate(ts), np.concatenate(ws)


def main():
    ap = argparse.ArgumentParser()
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

#!/usr/bin/env python3
"""What vdb_index_search_hybrid_sum costs: on 1M cosine rows of 768 dims with the
sparse column of tools/sparse_bench.py (about 60 entries a row, 30 522 terms), queries of 32 terms, k =
10, host-memory calls (complete on return), for batches of 1, 8 and 64 queries the time per call of
  1. ``search_hybrid_sum``,
  2. ``search_sparse`` (the same read of the column),
  3. ``search(k)`` under ``force_exact`` (the same read of the fp32 rows),
  4. ``search_hybrid`` (RRF of two fetched lists, fetch_k = 40),
all in one process on one device, each the median of repeated calls after warm-up with their range; and
for the weighted-sum call the bytes its kernel reads per second (the fp32 rows plus every row's offsets
and (term, weight) pairs, once per query) against the HBM figure DESIGN.md uses.  One JSON line per
measurement.  Reads nothing outside the repository.

Run it under a time limit of its own (``timeout -k 10 900 python tools/hybrid_sum_bench.py``).

  python tools/hybrid_sum_bench.py [--rows 1000000] [--dim 768] [--entries 64] [--reps 9] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from sparse_bench import HBM_GBPS, _stats, column, queries  # noqa: E402

METRIC = "cosine"
K, FETCH, N_TERMS = 10, 40, 30522
BATCHES = (1, 8, 64)
WARMUPS = 3


def _timed(fn, reps):
    for _ in range(WARMUPS):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return _stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--entries", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error("--reps must be at least 9")
    from service import _vdb
    rng = np.random.default_rng(0)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    V = rng.standard_normal((args.rows, args.dim), dtype=np.float32)
    ix = _vdb.NativeIndex(args.dim, METRIC)
    ix.add(V)
    del V
    indptr, terms, weights = column(args.rows, args.entries, N_TERMS, rng)
    ix.set_sparse(indptr, terms, weights, N_TERMS)
    csr_bytes = terms.size * 8 + (args.rows + 1) * 8
    row_bytes = args.rows * ((args.dim + 7) // 8 * 8) * 4  # the fp32 rows, padded to whole groups of 8 dims
    emit({"what": "corpus", "rows": args.rows, "dim": args.dim, "nnz": int(terms.size),
          "entries_per_row": round(terms.size / args.rows, 1), "row_bytes": row_bytes, "csr_bytes": csr_bytes})
    for B in BATCHES:
        qi, qt, qw = queries(B, N_TERMS, rng)
        Q = rng.standard_normal((B, args.dim)).astype(np.float32)
        common = {"B": B, "k": K, "rows": args.rows, "dim": args.dim}
        h = _timed(lambda: ix.search_hybrid_sum(Q, qi, qt, qw, K, (0.5, 0.5)), args.reps)
        gbps = B * (row_bytes + csr_bytes) / (h["median_ms"] * 1e-3) / 1e9
        h.update({"what": "search_hybrid_sum", "read_gb_per_s": round(gbps, 1), "of_hbm": round(gbps / HBM_GBPS, 4), **common})
        emit(h)
        p = _timed(lambda: ix.search_hybrid_sum(Q, qi, qt, qw, K, (0.5, 0.5), with_fused=True, with_parts=True), args.reps)
        p.update({"what": "search_hybrid_sum with out_fused, out_dense, out_sparse", **common})
        emit(p)
        # the same call for queries without terms: no lane walks a row, what is left is the dense half
        ei, et, ew = np.zeros(B + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
        e = _timed(lambda: ix.search_hybrid_sum(Q, ei, et, ew, K, (0.5, 0.5)), args.reps)
        e.update({"what": "search_hybrid_sum, queries without terms",
                  "rows_gb_per_s": round(B * row_bytes / (e["median_ms"] * 1e-3) / 1e9, 1), **common})
        emit(e)
        s = _timed(lambda: ix.search_sparse(qi, qt, qw, K), args.reps)
        s.update({"what": "search_sparse", "csr_gb_per_s": round(B * csr_bytes / (s["median_ms"] * 1e-3) / 1e9, 1), **common})
        emit(s)
        ix.set_param("force_exact", 1)
        d = _timed(lambda: ix.search(Q, K), args.reps)
        ix.set_param("force_exact", 0)
        d.update({"what": "search under force_exact", "rows_gb_per_s": round(B * row_bytes / (d["median_ms"] * 1e-3) / 1e9, 1),
                  **common})
        emit(d)
        r = _timed(lambda: ix.search_hybrid(Q, qi, qt, qw, K, FETCH), args.reps)
        r.update({"what": "search_hybrid (RRF)", "fetch_k": FETCH, **common})
        emit(r)
        emit({"what": "hybrid_sum against sparse + forced exact", "B": B,
              "ratio": round(h["median_ms"] / (s["median_ms"] + d["median_ms"]), 3)})
    ix.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What vdb_index_search_range costs with each form of its scan: 1M x 768 cosine and
1M x 128 euclidean, standard-normal rows, batches of 1, 8, 64 and 256 queries in host memory, with
thresholds found by bisection over count-only calls so that every query has exactly 10 or 1 000 hits,
count-only (cap 0) and with lists (cap = the hits).  Each configuration runs with the knob
"range_mfma" at 2 (the fp64 scan, the baseline) and at 1 (the fp32-MFMA scan), the two alternating
window by window; the time per call is a host clock around a window of blocking host-memory calls
(each ends in its download), after a warm-up call of each form, and the line carries the median of the
windows with their range.  The two forms' outputs must be equal in every byte.  Each line also gives
the share of pairs the MFMA form rescored in fp64 (stat "range_mfma_exact_pairs") and the corpus
bytes read per second if the fp32 copy is read once per block of 64 queries.  One JSON line per
configuration; the last line names the smallest batch from which the MFMA form is not slower at
either shape.

Run it under a time limit of its own (``timeout -k 10 900 python tools/range_bench.py``).

  python tools/range_bench.py [--reps 5] [--out FILE] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SHAPES = ((1_000_000, 768, "cosine"), (1_000_000, 128, "euclidean"))
BATCHES = (1, 8, 64, 256)
HITS = (10, 1000)
WINDOW_S = 0.25  # least time of a timed window


def bisect_thresholds(ix, Q, hits, metric):
    """Per-query thresholds at which the count-only call returns exactly `hits` for every query."""
    B = Q.shape[0]
    lo = np.full(B, -1.0 if metric == "cosine" else 0.0)
    hi = np.full(B, 1.0 if metric == "cosine" else 4.0 * np.sqrt(Q.shape[1]))
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        c = ix.search_range(Q, mid, cap=0)[0]
        if (c == hits).all():
            return mid
        more = c > hits  # too many rows pass: cosine raises the threshold, euclidean shrinks the radius
        if metric == "cosine":
            lo, hi = np.where(more, mid, lo), np.where(c < hits, mid, hi)
        else:
            hi, lo = np.where(more, mid, hi), np.where(c < hits, mid, lo)
    raise RuntimeError("bisection did not reach the stated hits")


def window(ix, Q, thr, cap, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        ix.search_range(Q, thr, cap=cap)
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="20 000 rows: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    from service import _vdb
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    not_slower = {}
    for n, dim, metric in SHAPES:
        if args.small:
            n = 20_000
        rng = np.random.default_rng(dim)
        V = rng.standard_normal((n, dim), dtype=np.float32)
        Qall = rng.standard_normal((max(BATCHES), dim), dtype=np.float32)
        ix = _vdb.NativeIndex(dim, metric)
        for s in range(0, n, 100_000):
            ix.add(V[s:s + 100_000])
        del V
        for B in BATCHES:
            Q = Qall[:B]
            for hits in HITS:
                ix.set_param("range_mfma", 2)
                thr = bisect_thresholds(ix, Q, hits, metric)
                for cap in (0, hits):
                    res, times = {}, {1: [], 2: []}
                    for knob in (2, 1):  # warm-up, and the outputs to compare
                        ix.set_param("range_mfma", knob)
                        res[knob] = b"".join(np.ascontiguousarray(a).tobytes() for a in ix.search_range(Q, thr, cap=cap))
                    same = res[1] == res[2]
                    e0, q0 = ix.stat("range_mfma_exact_pairs"), ix.stat("range_mfma_queries")
                    calls = {}
                    for knob in (2, 1):
                        ix.set_param("range_mfma", knob)
                        calls[knob] = max(2, int(np.ceil(WINDOW_S / max(window(ix, Q, thr, cap, 1), 1e-5))))
                    for _ in range(args.reps):
                        for knob in (2, 1):
                            ix.set_param("range_mfma", knob)
                            times[knob].append(window(ix, Q, thr, cap, calls[knob]))
                    pairs = (ix.stat("range_mfma_queries") - q0) * n
                    share = (ix.stat("range_mfma_exact_pairs") - e0) / max(pairs, 1)
                    med = {k: float(np.median(v)) for k, v in times.items()}
                    blocks = -(-B // 64)
                    emit({"rows": n, "dim": dim, "metric": metric, "batch": B, "hits": hits, "cap": cap, "same_bytes": same,
                          "fp64_ms": round(med[2] * 1e3, 3), "fp64_ms_range": [round(min(times[2]) * 1e3, 3), round(max(times[2]) * 1e3, 3)],
                          "mfma_ms": round(med[1] * 1e3, 3), "mfma_ms_range": [round(min(times[1]) * 1e3, 3), round(max(times[1]) * 1e3, 3)],
                          "speedup": round(med[2] / med[1], 2), "mfma_exact_pair_share": share,
                          "mfma_corpus_gbps": round(blocks * n * ((dim + 63) // 64 * 64) * 4 / med[1] / 1e9, 1),
                          "calls_per_window": calls})
                    assert same, "the two forms differ"
                    not_slower.setdefault(B, True)
                    not_slower[B] &= med[1] <= med[2]
        ix.close()
    ok = [B for B in BATCHES if all(not_slower.get(b, False) for b in BATCHES if b >= B)]
    emit({"auto_min_queries": min(ok) if ok else None, "not_slower_by_batch": {str(k): v for k, v in not_slower.items()}})


if __name__ == "__main__":
    main()

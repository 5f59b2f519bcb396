#!/usr/bin/env python3
"""Range search against the only alternative the library had, same index, same rows.

For each shape (1 M x 768 cosine, 1 M x 128 L2; a fresh index each), B = 1 and B = 64, and 0, 10,
1 000 and 100 000 hits per query: ``NativeIndex.search_range`` with cap = the largest count, and
the same call with cap = 0 (scan and prefix alone), host memory, median of 20 calls after 5
warm-ups with the range reported.  The thresholds are found on the device data, per query, by
bisection over count-only calls.  Beside each figure: ``search(k = min(hits, 1024))``, the only
read the library had before (it answers a different question once the hits exceed 1 024: the best
1 024, not all of them); phase 1's bytes per second against the size of the fp32 copy (one read
per query block); and the share of the call spent after phase 1, (full - count-only) / full, host
timed, so it includes the download of the lists.

Run without arguments: each shape runs as a child process under its own ``timeout -k 10``, and
nothing more is started after one fails.  Prints one JSON line per measurement and a table.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (os.path.join(ROOT, "mlx-vector-db_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"c2": (1_000_000, 768, "cosine"), "l2": (1_000_000, 128, "euclidean")}
HITS = (0, 10, 1_000, 100_000)
BATCHES = (1, 64)
QUERY_BYTES, MAX_BLOCK = 128 * 1024, 64  # csrc/vdb_range_plan.h


def _time(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def _thresholds(ix, Q, hits, metric, np):
    """Per-query thresholds that `hits` rows pass (as near as the keys allow), by bisection on the
    key bound over count-only calls."""
    B = Q.shape[0]
    if hits == 0:
        return np.full(B, 2.0 if metric == "cosine" else 0.0)
    to_t = (lambda kt: kt) if metric == "cosine" else (lambda kt: np.sqrt(-kt))
    lo = np.full(B, -1.0) if metric == "cosine" else np.full(B, -1e7)  # passes every row
    hi = np.full(B, 1.0) if metric == "cosine" else np.zeros(B)       # passes (next to) none
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        c = ix.search_range(Q, to_t(mid), cap=0)[0]
        more = c > hits
        lo = np.where(more, mid, lo)
        hi = np.where(more, hi, mid)
        if (c == hits).all():
            return to_t(mid)
    return to_t(hi)


def run_shape(name, reps, warm, rows_override=None):
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime per process)
    from service import _vdb

    n, d, metric = SHAPES[name]
    if rows_override:
        n = rows_override
    rng = np.random.default_rng(23)
    ix = _vdb.NativeIndex(d, metric)
    ix.reserve(n)
    for s in range(0, n, 250_000):
        ix.add(rng.standard_normal((min(250_000, n - s), d), dtype=np.float32))
    Qall = rng.standard_normal((64, d), dtype=np.float32)
    dp = (d + 7) // 8 * 8
    copy_bytes = n * dp * 4
    block = max(1, min(MAX_BLOCK, QUERY_BYTES // (dp * 4)))
    out = []
    for B in BATCHES:
        Q = Qall[:B]
        passes = (B + block - 1) // block
        for hits in HITS:
            if hits > n:
                continue
            thr = _thresholds(ix, Q, hits, metric, np)
            counts = ix.search_range(Q, thr, cap=0)[0]
            cap = max(int(counts.max()), 1)
            got = ix.search_range(Q, thr, cap=cap, with_keys=True)
            assert np.array_equal(got[0], counts)
            k = max(1, min(hits, 1024))
            ss, si, sk = ix.search(Q, k, with_keys=True)
            for b in range(B):  # the two reads agree on the rows they share
                c = int(counts[b])
                order = np.lexsort((got[1][b, :c], -got[3][b, :c]))[:k]
                m = min(c, k)
                assert np.array_equal(got[1][b, :c][order][:m], si[b, :m]), (name, B, hits, b)
            r = reps if B * cap <= 1_000_000 else max(5, reps // 4)  # (the 100+ MB result copies)
            tf = _time(lambda: ix.search_range(Q, thr, cap=cap, with_keys=True), r, warm)
            tc = _time(lambda: ix.search_range(Q, thr, cap=0), r, warm)
            ts = _time(lambda: ix.search(Q, k, with_keys=True), r, warm)
            rec = {"shape": name, "rows": n, "dim": d, "metric": metric, "B": B, "hits": hits,
                   "count_min_max": [int(counts.min()), int(counts.max())], "cap": cap,
                   "range_ms": round(tf[0], 4), "range_min_max": [round(tf[1], 4), round(tf[2], 4)],
                   "count_only_ms": round(tc[0], 4), "count_only_min_max": [round(tc[1], 4), round(tc[2], 4)],
                   "search_k": k, "search_ms": round(ts[0], 4), "search_min_max": [round(ts[1], 4), round(ts[2], 4)],
                   "phase1_gb_per_s": round(passes * copy_bytes / (tc[0] * 1e-3) / 1e9, 1),
                   "after_phase1_share": round(max(0.0, 1.0 - tc[0] / tf[0]), 3), "reps": r}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    ix.close()
    print(f"{'shape':6}{'B':>4}{'hits':>9}{'range ms':>11}{'count ms':>11}{'search ms':>11}{'k':>6}{'GB/s':>9}{'after p1':>10}")
    for r in out:
        print(f"{r['shape']:6}{r['B']:>4}{r['hits']:>9}{r['range_ms']:>11.3f}{r['count_only_ms']:>11.3f}"
              f"{r['search_ms']:>11.3f}{r['search_k']:>6}{r['phase1_gb_per_s']:>9.1f}{r['after_phase1_share']:>10.1%}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=0, help="fewer rows than the shape's (a quick look)")
    ap.add_argument("--step-timeout", type=int, default=420)
    a = ap.parse_args()
    if a.shape:
        run_shape(a.shape, a.reps, a.warmup, a.rows or None)
        return 0
    for name in SHAPES:  # one GPU step per shape, each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--shape", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--rows", str(a.rows)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"{name}: exit {rc}; nothing more is run", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

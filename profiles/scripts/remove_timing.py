#!/usr/bin/env python3
"""Time row removal on the device against the host round trip (DESIGN.md "Deleting rows").

    python profiles/scripts/remove_timing.py [--rows 1000000] [--dim 768] [--reps 5] [--host-reps 3]

At C2's corpus (1M x 768 cosine, precision auto), for a random 1 % and a random 50 % of the rows:

  * device path: ``NativeIndex.remove(bitmap)`` (include/vdb.h vdb_index_remove), median of
    ``--reps`` runs, a fresh index each time (the add is not timed);
  * host round trip, the only route without it: ``get_vectors`` -> ``np.delete`` -> ``clear`` ->
    ``add``, same process, same data, median of ``--host-reps``.

After each timed run a B = 64, k = 10 search must return the same rows whichever route removed
them.  Prints one JSON line with the times and an estimate of the bytes the device path moves.
Run each invocation under a time limit of its own (``timeout 600 python ...``).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (os.path.join(ROOT, "mlx-vector-db_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def moved_bytes(N, Dp, rows, split_copy=False):
    """Estimate of the device path's traffic for removing sorted `rows` of N (csrc/vdb_api.cpp
    vdb_index_remove): gather + place (4 passes over the moved rows), rebuild of their int8
    copy (read 4 B, write 2 + 1 B per element; + 4 B for an existing split copy), column sums
    (2 B per element of every kept row), zeroing of the tail (4 + 2 + 1 B per element)."""
    kept = N - rows.size
    first = int(rows[0]) // 32 * 32
    moved = kept - first
    row_b = Dp * 4 + 20
    gather = 4 * moved * row_b
    rebuild = moved * Dp * (4 + 2 + 1 + (4 if split_copy else 0))
    colsum = kept * Dp * 2
    tail = (N - kept) * Dp * (4 + 2 + 1 + (4 if split_copy else 0))
    return {"gather_place": gather, "rebuild": rebuild, "column_sums": colsum, "tail_zero": tail,
            "total": gather + rebuild + colsum + tail}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--metric", default="cosine")
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    from service import _vdb
    N, D = a.rows, a.dim
    Dp = (D + 63) // 64 * 64
    rng = np.random.default_rng(0)
    V = rng.random((N, D), dtype=np.float32)
    Q = rng.random((64, D), dtype=np.float32)
    out = {"rows": N, "dim": D, "metric": a.metric, "precision": "auto", "fractions": {}}
    for name, frac in (("1pct", 0.01), ("50pct", 0.50)):
        rows = np.sort(rng.permutation(N)[: int(N * frac)])
        mask = _vdb.rows_to_bitmap(rows, N)
        dev_ms, host_ms, host_parts = [], [], []
        want = None
        for rep in range(a.reps):
            ix = _vdb.NativeIndex(D, a.metric)
            ix.add(V)
            ix.search(Q, 10)  # warm: workspaces, kernels loaded
            t0 = time.perf_counter()
            n = ix.remove(mask)
            dev_ms.append((time.perf_counter() - t0) * 1e3)
            assert n == rows.size and ix.count() == N - rows.size
            got = ix.search(Q, 10)[1]
            want = got if want is None else want
            assert np.array_equal(got, want)
            ix.close()
        for rep in range(a.host_reps):
            ix = _vdb.NativeIndex(D, a.metric)
            ix.add(V)
            ix.search(Q, 10)
            t0 = time.perf_counter()
            X = ix.get_vectors()
            t1 = time.perf_counter()
            X = np.delete(X, rows, axis=0)
            t2 = time.perf_counter()
            ix.clear()
            ix.add(X)
            t3 = time.perf_counter()
            host_ms.append((t3 - t0) * 1e3)
            host_parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
            assert np.array_equal(ix.search(Q, 10)[1], want), "the two routes disagree"
            ix.close()
        best = min(range(len(host_ms)), key=lambda i: host_ms[i])
        out["fractions"][name] = {
            "removed": int(rows.size),
            "device_ms_median": round(statistics.median(dev_ms), 3),
            "device_ms_all": [round(x, 3) for x in dev_ms],
            "host_round_trip_ms_median": round(statistics.median(host_ms), 1),
            "host_round_trip_ms_all": [round(x, 1) for x in host_ms],
            "host_best_parts_ms": {"get_vectors": round(host_parts[best][0], 1), "np_delete": round(host_parts[best][1], 1),
                                   "clear_add": round(host_parts[best][2], 1)},
            "speedup": round(statistics.median(host_ms) / statistics.median(dev_ms), 1),
            "device_bytes": moved_bytes(N, Dp, rows),
        }
        b = out["fractions"][name]["device_bytes"]["total"]
        out["fractions"][name]["device_effective_TBps"] = round(b / (statistics.median(dev_ms) * 1e-3) / 1e12, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What vdb_index_search_hamming costs: on 1M rows of 1 024 bits and on 10M rows of
256 bits, batches of 1, 16, 64, 256 and 1 024 queries, k = 10, every argument in device memory, each
with the knob "hamming_mfma" at 2 (the popcount kernel, the baseline) and at 1 (the integer-MFMA
kernel), the two alternating per batch size, the time per batch
(device events around a window of back-to-back calls, after warm-up; the median of several windows
with their range), the code bytes the batch reads per second if the column is read once per block of
queries (ceil(B / QB) times; QB = 16 for the popcount kernel, 64 for the MFMA one) against the HBM figure DESIGN.md uses, and the XOR + popcount word
operations per second.  Beside each line, the same search restated in numpy on the CPU with at most
16 threads (XOR, a 16-bit popcount table, argpartition per slice of the rows, then a lexsort), one
run (batches up to 64); its result must equal the popcount kernel's, and the MFMA kernel's result
must equal the popcount kernel's at every batch size.  One JSON line per measurement.

Whether the search is bound by the code read or by the popcount and top-k work shows in the lines
themselves: a read-bound search takes the same time for 1 and for 16 queries (one block, one read),
a compute-bound one 16 times as long.

Run it under a time limit of its own (``timeout -k 10 900 python tools/hamming_bench.py``).

  python tools/hamming_bench.py [--reps 7] [--out FILE] [--small] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

DIM, K = 8, 10
QB = {2: 16, 1: 64}  # knob -> queries per column read (csrc/vdb_hamming_plan.h ham_qb(10), ham_mfma_qb(10))
CPU_MAX_B = 64
HBM_GBPS = 8000.0  # the peak DESIGN.md measures bandwidth against
CPU_THREADS = min(16, os.cpu_count() or 1)
POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.uint8)


def cpu_search(Q, X, k):
    """(distances, rows) [B, k] by (distance asc, row asc), rows cut into CPU_THREADS slices."""
    n = X.shape[0]
    X16 = X.view(np.uint16)
    bounds = np.linspace(0, n, CPU_THREADS + 1).astype(np.int64)

    def part(args):
        q16, lo, hi = args
        d = POP16[X16[lo:hi] ^ q16].sum(axis=1, dtype=np.int32)
        kk = min(k, hi - lo)
        # every row at or below the kk-th smallest distance, so that ties at the cut keep their lowest rows
        cut = np.partition(d, kk - 1)[kk - 1]
        rows = np.nonzero(d <= cut)[0]
        return d[rows], rows + lo

    dist = np.empty((Q.shape[0], k), np.int32)
    idx = np.empty((Q.shape[0], k), np.int64)
    with ThreadPoolExecutor(CPU_THREADS) as pool:
        for b in range(Q.shape[0]):
            q16 = Q[b].view(np.uint16)
            parts = list(pool.map(part, [(q16, bounds[i], bounds[i + 1]) for i in range(CPU_THREADS) if bounds[i] < bounds[i + 1]]))
            d = np.concatenate([p[0] for p in parts])
            r = np.concatenate([p[1] for p in parts])
            order = np.lexsort((r, d))[:k]
            dist[b], idx[b] = d[order], r[order]
    return dist, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1/100 of the rows (a rehearsal of the script, not a measurement)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement")
    args = ap.parse_args()
    import torch
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    rng = np.random.default_rng(0)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for rows, n_bytes in ((1_000_000, 128), (10_000_000, 32)):
        if args.small:
            rows //= 100
        X = rng.integers(0, 256, (rows, n_bytes), dtype=np.uint8)
        ix = _vdb.NativeIndex(DIM, "cosine", precision="fp32")
        for lo in range(0, rows, 1_000_000):
            ix.add(rng.random((min(1_000_000, rows - lo), DIM), dtype=np.float32))
        t0 = time.perf_counter()
        ix.set_codes(X)
        emit({"what": "set_codes", "rows": rows, "n_bytes": n_bytes, "ms": round(1e3 * (time.perf_counter() - t0), 2)})
        code_bytes = rows * n_bytes
        for B in (1, 16, 64, 256, 1024):
            Q = rng.integers(0, 256, (B, n_bytes), dtype=np.uint8)
            Q[0] = X[rows // 3]
            Q[0, 0] ^= 1
            dq = torch.from_numpy(Q).to("cuda")
            dd = torch.empty((B, K), dtype=torch.int32, device="cuda")
            di = torch.empty((B, K), dtype=torch.int64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream

            def call():
                ix.search_hamming_device(dq.data_ptr(), B, K, dd.data_ptr(), di.data_ptr(), stream=st)

            base = None  # the popcount kernel's result
            for knob in (2, 1):
                ix.set_param("hamming_mfma", knob)
                before = ix.stat("hamming_mfma_queries")
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
                assert ix.stat("hamming_mfma_queries") - before == (3 * B if knob == 1 else 0), "not the form asked for"
                # calls per window: enough for about 0.2 s, sized from one timed call
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(); e1.record(); torch.cuda.synchronize()
                per = max(int(200.0 / max(e0.elapsed_time(e1), 1e-3)), 5)
                ts = []
                for _ in range(args.reps):
                    e0.record()
                    for _ in range(per):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) / per)
                ts.sort()
                med = ts[len(ts) // 2]
                reads = -(-B // QB[knob])
                word_ops = B * rows * ((n_bytes + 7) // 8)
                rec = {"what": "search_hamming", "form": "popcount" if knob == 2 else "mfma", "rows": rows, "bits": 8 * n_bytes,
                       "B": B, "k": K, "mem": "device",
                       "median_ms": round(med, 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "windows": len(ts),
                       "calls_per_window": per, "ms_per_query": round(med / B, 4), "column_reads": reads,
                       "code_gb_per_s": round(reads * code_bytes / (med * 1e-3) / 1e9, 1),
                       "of_hbm": round(reads * code_bytes / (med * 1e-3) / 1e9 / HBM_GBPS, 4),
                       "gword_ops_per_s": round(word_ops / (med * 1e-3) / 1e9, 1)}
                got = dd.cpu().numpy().copy(), di.cpu().numpy().copy()
                if knob == 2:
                    base = got
                    if B <= CPU_MAX_B and not args.no_cpu:
                        t0 = time.perf_counter()
                        cd, ci = cpu_search(Q, X, K)
                        rec.update({"cpu_numpy_ms": round(1e3 * (time.perf_counter() - t0), 1), "cpu_threads": CPU_THREADS})
                        rec["equal_to_cpu"] = bool(np.array_equal(got[0], cd) and np.array_equal(got[1], ci))
                else:
                    rec["equal_to_popcount"] = bool(np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]))
                emit(rec)
        ix.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

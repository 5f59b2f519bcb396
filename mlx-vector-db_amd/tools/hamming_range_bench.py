#!/usr/bin/env python3
"""What vdb_index_search_hamming_range costs, and from which batch size its MFMA scan
beats its popcount scan: on 1M rows of 1 024 bits and on 10M rows of 256 bits, batches of 1, 16, 64,
256 and 1 024 queries, every argument in device memory, once count-only (cap = 0) and once with the
radius at which a random code expects about 100 rows (cap = 256), each with the knob
"hamming_range_mfma" at 2 (the popcount scan) and at 1 (the MFMA scan).  The two forms alternate
window by window; a window is a run of back-to-back calls between two device events, sized to about
0.2 s after warm-up, and the line gives the median of the windows with their range.  Beside the time:
the code bytes read per second if the column is read once per block of queries (16 for the popcount
scan, 64 for the MFMA one) against the HBM figure DESIGN.md uses.  The MFMA scan's counts, ids and
distances must equal the popcount scan's at every point.  One JSON line per measurement, and at the end
one line per shape and mode with the smallest batch from which the MFMA scan is the faster at every
larger batch measured.

Run it under a time limit of its own (``timeout -k 10 900 python tools/hamming_range_bench.py``).

  python tools/hamming_range_bench.py [--reps 7] [--out FILE] [--small]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

DIM, CAP = 8, 256
QB = {2: 16, 1: 64}  # knob -> queries per column read (csrc/vdb_hamming_range_plan.h)
FORM = {2: "popcount", 1: "mfma"}
BATCHES = (1, 16, 64, 256, 1024)
HBM_GBPS = 8000.0  # the peak DESIGN.md measures bandwidth against


def radius_for(rows, bits, hits):
    """The smallest radius within which a uniformly random code expects at least ``hits`` of ``rows`` rows."""
    total, acc = 1 << bits, 0
    for r in range(bits + 1):
        acc += math.comb(bits, r)
        if acc * rows >= hits * total:
            return r
    return bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1/100 of the rows (a rehearsal of the script, not a measurement)")
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
        ix.set_codes(X)
        code_bytes = rows * n_bytes
        radius = radius_for(rows, 8 * n_bytes, 100)
        for mode, cap in (("count", 0), ("hits", CAP)):
            wins = {}
            for B in BATCHES:
                Q = rng.integers(0, 256, (B, n_bytes), dtype=np.uint8)
                dq = torch.from_numpy(Q).to("cuda")
                dr = torch.full((B,), radius, dtype=torch.int32, device="cuda")
                dc = torch.empty((B,), dtype=torch.int64, device="cuda")
                di = torch.empty((B, max(cap, 1)), dtype=torch.int64, device="cuda")
                dd = torch.empty((B, max(cap, 1)), dtype=torch.int32, device="cuda")
                st = torch.cuda.current_stream().cuda_stream

                def call():
                    ix.search_hamming_range_device(dq.data_ptr(), B, dr.data_ptr(), cap, dc.data_ptr(), di.data_ptr(),
                                                   dd.data_ptr(), stream=st)

                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                per, got, ts = {}, {}, {2: [], 1: []}
                for knob in (2, 1):  # warm-up, the form check, the result and the window size
                    ix.set_param("hamming_range_mfma", knob)
                    before = ix.stat("hamming_range_mfma_queries")
                    for _ in range(3):
                        call()
                    torch.cuda.synchronize()
                    assert ix.stat("hamming_range_mfma_queries") - before == (3 * B if knob == 1 else 0), "not the form asked for"
                    got[knob] = [t.cpu().numpy().copy() for t in ((dc, di, dd) if cap else (dc,))]
                    e0.record(); call(); e1.record(); torch.cuda.synchronize()
                    per[knob] = max(int(200.0 / max(e0.elapsed_time(e1), 1e-3)), 5)
                for _ in range(args.reps):  # the forms alternate window by window
                    for knob in (2, 1):
                        ix.set_param("hamming_range_mfma", knob)
                        e0.record()
                        for _ in range(per[knob]):
                            call()
                        e1.record()
                        torch.cuda.synchronize()
                        ts[knob].append(e0.elapsed_time(e1) / per[knob])
                equal = all(np.array_equal(a, b) for a, b in zip(got[2], got[1]))
                med = {}
                for knob in (2, 1):
                    t = sorted(ts[knob])
                    med[knob] = t[len(t) // 2]
                    reads = -(-B // QB[knob])
                    emit({"what": "search_hamming_range", "form": FORM[knob], "mode": mode, "rows": rows, "bits": 8 * n_bytes,
                          "B": B, "radius": radius, "cap": cap, "mem": "device", "mean_count": round(float(got[knob][0].mean()), 1),
                          "median_ms": round(med[knob], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                          "windows": len(t), "calls_per_window": per[knob], "ms_per_query": round(med[knob] / B, 5),
                          "column_reads": reads, "code_gb_per_s": round(reads * code_bytes / (med[knob] * 1e-3) / 1e9, 1),
                          "of_hbm": round(reads * code_bytes / (med[knob] * 1e-3) / 1e9 / HBM_GBPS, 4),
                          "equal_to_popcount": equal if knob == 1 else None})
                wins[B] = med[1] < med[2]
            first = None
            for B in reversed(BATCHES):  # the smallest batch from which the MFMA scan wins at every larger one
                if not wins[B]:
                    break
                first = B
            emit({"what": "threshold", "mode": mode, "rows": rows, "bits": 8 * n_bytes, "mfma_wins_from": first})
        ix.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What vdb_index_search_jaccard_range costs, and from which batch size its MFMA scan
beats its popcount scan: on 1M rows of 1 024 bits, 1M rows of 2 048 bits and 10M rows of 256 bits,
batches of 1, 16, 64, 256 and 1 024 queries, every argument in device memory, once count-only (cap = 0)
and once with the threshold num / 8 192 at which random codes give about 100 rows per query (found by
bisection with count-only calls; cap = 256), each with the knob "jaccard_range_mfma" at 2 (the popcount
scan) and at 1 (the MFMA scan).  For orientation the same batch goes through
vdb_index_search_hamming_range (its own choice of scan, the radius that expects about 100 rows), which
reads the same bytes.  The forms alternate window by window; a window is a run of back-to-back calls
between two device events, sized to about 0.2 s after warm-up, and the line gives the median of the
windows with their range.  Beside the time: the code bytes read per second if the column is read once
per block of queries (16 for the popcount scan, 64 for the MFMA one) against the HBM figure DESIGN.md
uses.  The MFMA scan's counts, ids, intersections and unions must equal the popcount scan's at every
point.  One JSON line per measurement, and at the end of a shape and mode one line with the smallest
batch from which the MFMA scan is the faster at every larger batch measured.

Run it under a time limit of its own (``timeout -k 10 900 python tools/jaccard_range_bench.py``).

  python tools/jaccard_range_bench.py [--reps 5] [--out FILE] [--small] [--shapes 0,1,2]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from tools.hamming_range_bench import radius_for  # noqa: E402

DIM, CAP, DEN = 8, 256, 8192
QB = {2: 16, 1: 64}  # knob -> queries per column read (csrc/vdb_jaccard_range_plan.h)
FORM = {2: "popcount", 1: "mfma", 0: "hamming_range"}
BATCHES = (1, 16, 64, 256, 1024)
SHAPES = ((1_000_000, 128), (1_000_000, 256), (10_000_000, 32))
HBM_GBPS = 8000.0  # the peak DESIGN.md measures bandwidth against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1/100 of the rows (a rehearsal of the script, not a measurement)")
    ap.add_argument("--shapes", default="0,1,2", help="which of the three shapes to run")
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
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for rows, n_bytes in [SHAPES[int(s)] for s in args.shapes.split(",")]:
        if args.small:
            rows //= 100
        X = rng.integers(0, 256, (rows, n_bytes), dtype=np.uint8)
        ix = _vdb.NativeIndex(DIM, "cosine", precision="fp32")
        for lo in range(0, rows, 1_000_000):
            ix.add(rng.random((min(1_000_000, rows - lo), DIM), dtype=np.float32))
        ix.set_codes(X)
        code_bytes = rows * n_bytes
        radius = radius_for(rows, 8 * n_bytes, 100)
        st = torch.cuda.current_stream().cuda_stream

        # the largest num / 8 192 that still gives 16 random queries about 100 rows each
        Q16 = torch.from_numpy(rng.integers(0, 256, (16, n_bytes), dtype=np.uint8)).to("cuda")
        c16 = torch.empty((16,), dtype=torch.int64, device="cuda")
        d16 = torch.full((16,), DEN, dtype=torch.int32, device="cuda")
        lo, hi = 0, DEN
        while lo < hi:  # counts fall as num rises: the last num with a mean count >= 100
            mid = (lo + hi + 1) // 2
            n16 = torch.full((16,), mid, dtype=torch.int32, device="cuda")
            ix.search_jaccard_range_device(Q16.data_ptr(), 16, n16.data_ptr(), d16.data_ptr(), 0, c16.data_ptr(), stream=st)
            torch.cuda.synchronize()
            lo, hi = (mid, hi) if float(c16.double().mean()) >= 100 else (lo, mid - 1)
        num_hits = lo

        for mode, cap in (("count", 0), ("hits", CAP)):
            wins = {}
            for B in BATCHES:
                Q = rng.integers(0, 256, (B, n_bytes), dtype=np.uint8)
                dq = torch.from_numpy(Q).to("cuda")
                dn = torch.full((B,), num_hits, dtype=torch.int32, device="cuda")
                dd = torch.full((B,), DEN, dtype=torch.int32, device="cuda")
                dr = torch.full((B,), radius, dtype=torch.int32, device="cuda")
                dc = torch.empty((B,), dtype=torch.int64, device="cuda")
                di = torch.empty((B, max(cap, 1)), dtype=torch.int64, device="cuda")
                d1 = torch.empty((B, max(cap, 1)), dtype=torch.int32, device="cuda")
                d2 = torch.empty((B, max(cap, 1)), dtype=torch.int32, device="cuda")

                def call(knob):
                    if knob == 0:
                        ix.search_hamming_range_device(dq.data_ptr(), B, dr.data_ptr(), cap, dc.data_ptr(), di.data_ptr(),
                                                       d1.data_ptr(), stream=st)
                    else:
                        ix.search_jaccard_range_device(dq.data_ptr(), B, dn.data_ptr(), dd.data_ptr(), cap, dc.data_ptr(),
                                                       di.data_ptr(), d1.data_ptr(), d2.data_ptr(), stream=st)

                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                per, got, ts = {}, {}, {2: [], 1: [], 0: []}
                for knob in (2, 1, 0):  # warm-up, the form check, the result and the window size
                    if knob:
                        ix.set_param("jaccard_range_mfma", knob)
                    before = ix.stat("jaccard_range_mfma_queries")
                    for _ in range(3):
                        call(knob)
                    torch.cuda.synchronize()
                    assert ix.stat("jaccard_range_mfma_queries") - before == (3 * B if knob == 1 else 0), "not the form asked for"
                    got[knob] = [t.cpu().numpy().copy() for t in ((dc, di, d1, d2) if cap else (dc,))]
                    e0.record(); call(knob); e1.record(); torch.cuda.synchronize()
                    per[knob] = max(int(200.0 / max(e0.elapsed_time(e1), 1e-3)), 5)
                for _ in range(args.reps):  # the forms alternate window by window
                    for knob in (2, 1, 0):
                        if knob:
                            ix.set_param("jaccard_range_mfma", knob)
                        e0.record()
                        for _ in range(per[knob]):
                            call(knob)
                        e1.record()
                        torch.cuda.synchronize()
                        ts[knob].append(e0.elapsed_time(e1) / per[knob])
                equal = all(np.array_equal(a, b) for a, b in zip(got[2], got[1]))
                med = {}
                for knob in (2, 1, 0):
                    t = sorted(ts[knob])
                    med[knob] = t[len(t) // 2]
                    rec = {"what": "search_" + ("hamming_range" if knob == 0 else "jaccard_range"), "form": FORM[knob], "mode": mode,
                           "rows": rows, "bits": 8 * n_bytes, "B": B, "cap": cap, "mem": "device",
                           "mean_count": round(float(got[knob][0].mean()), 1), "median_ms": round(med[knob], 4),
                           "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4), "windows": len(t), "calls_per_window": per[knob],
                           "ms_per_query": round(med[knob] / B, 5)}
                    if knob:
                        reads = -(-B // QB[knob])
                        rec.update({"threshold": [num_hits, DEN], "column_reads": reads,
                                    "code_gb_per_s": round(reads * code_bytes / (med[knob] * 1e-3) / 1e9, 1),
                                    "of_hbm": round(reads * code_bytes / (med[knob] * 1e-3) / 1e9 / HBM_GBPS, 4),
                                    "equal_to_popcount": equal if knob == 1 else None})
                    else:
                        rec["radius"] = radius
                    emit(rec)
                wins[B] = med[1] < med[2]
            first = None
            for B in reversed(BATCHES):  # the smallest batch from which the MFMA scan wins at every larger one
                if not wins[B]:
                    break
                first = B
            emit({"what": "threshold", "mode": mode, "rows": rows, "bits": 8 * n_bytes, "mfma_wins_from": first})
        ix.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What vdb_index_search_jaccard costs, and from which batch size its int8-MFMA form
beats its popcount form: on 1M rows of 1 024 bits, 1M rows of 2 048 bits and 10M rows of 256 bits,
batches of 1, 16, 64 and 1 024 queries at k = 10, every argument in device memory, each with the knob
"jaccard_mfma" at 2 (popcount) and at 1 (MFMA).  Codes and queries are sparse, as fingerprints are:
about one bit in eight set.  The two forms alternate window by window; a window is a run of back-to-back
calls between two device events, sized to about 0.2 s after warm-up, and the line gives the median of
the windows with their range.  The MFMA form's three outputs must equal the popcount form's at every
point.  One JSON line per measurement, and at the end one line per shape with the smallest batch from
which the MFMA form is the faster at every larger batch measured.

Run it under a time limit of its own (``timeout -k 10 900 python tools/jaccard_bench.py``).

  python tools/jaccard_bench.py [--reps 7] [--out FILE] [--small]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

DIM, K = 8, 10
FORM = {2: "popcount", 1: "mfma"}
BATCHES = (1, 16, 64, 1024)
SHAPES = ((1_000_000, 128), (1_000_000, 256), (10_000_000, 32))


def sparse_codes(rng, rows, n_bytes):
    a = rng.integers(0, 256, (rows, n_bytes), dtype=np.uint8)
    a &= rng.integers(0, 256, (rows, n_bytes), dtype=np.uint8)
    a &= rng.integers(0, 256, (rows, n_bytes), dtype=np.uint8)
    return a


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

    for rows, n_bytes in SHAPES:
        if args.small:
            rows //= 100
        ix = _vdb.NativeIndex(DIM, "cosine", precision="fp32")
        for r0 in range(0, rows, 1_000_000):
            ix.add(rng.random((min(1_000_000, rows - r0), DIM), dtype=np.float32))
        ix.set_codes(sparse_codes(rng, rows, n_bytes))
        wins = {}
        for B in BATCHES:
            dq = torch.from_numpy(sparse_codes(rng, B, n_bytes)).to("cuda")
            dn = torch.empty((B, K), dtype=torch.int32, device="cuda")
            du = torch.empty((B, K), dtype=torch.int32, device="cuda")
            di = torch.empty((B, K), dtype=torch.int64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream

            def call():
                ix.search_jaccard_device(dq.data_ptr(), B, K, dn.data_ptr(), du.data_ptr(), di.data_ptr(), stream=st)

            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            per, got, ts = {}, {}, {2: [], 1: []}
            for knob in (2, 1):  # warm-up, the form check, the result and the window size
                ix.set_param("jaccard_mfma", knob)
                before = ix.stat("jaccard_mfma_queries")
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
                assert ix.stat("jaccard_mfma_queries") - before == (3 * B if knob == 1 else 0), "not the form asked for"
                got[knob] = [t.cpu().numpy().copy() for t in (dn, du, di)]
                e0.record(); call(); e1.record(); torch.cuda.synchronize()
                per[knob] = max(int(200.0 / max(e0.elapsed_time(e1), 1e-3)), 5)
            for _ in range(args.reps):  # the forms alternate window by window
                for knob in (2, 1):
                    ix.set_param("jaccard_mfma", knob)
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
                emit({"what": "search_jaccard", "form": FORM[knob], "rows": rows, "bits": 8 * n_bytes, "B": B, "k": K,
                      "mem": "device", "median_ms": round(med[knob], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                      "windows": len(t), "calls_per_window": per[knob], "ms_per_query": round(med[knob] / B, 5),
                      "equal_to_popcount": equal if knob == 1 else None})
            wins[B] = med[1] < med[2]
        first = None
        for B in reversed(BATCHES):  # the smallest batch from which the MFMA form wins at every larger one
            if not wins[B]:
                break
            first = B
        emit({"what": "threshold", "rows": rows, "bits": 8 * n_bytes, "mfma_wins_from": first})
        ix.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

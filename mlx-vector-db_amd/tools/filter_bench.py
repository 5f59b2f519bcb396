#!/usr/bin/env python3
"""What vdb_index_filter_mask costs: on indexes of 1M and 10M rows (dim 8: the rows
themselves are never read) with three fp64 columns attached, for P = 1 and 64 predicates of 1 and 3
clauses each, every predicate with its own bounds, the time per call of
  1. ``filter_mask`` in host memory (complete on return: the masks and counts come down),
  2. ``filter_mask_device`` in device memory, timed with device events around the call on one stream,
  3. a numpy restatement of the same predicates on the host, ``np.packbits`` included: what building
     the same masks without the device call costs on the same box,
each the median of repeated calls after warm-up with their range; and for the device-memory call
the bytes the kernel reads and writes (each used column once, the masks once) over its time, against
the HBM figure DESIGN.md uses.  One JSON line per measurement.  Reads nothing outside the
repository.

Run it under a time limit of its own (``timeout -k 10 600 python tools/filter_bench.py``).

  python tools/filter_bench.py [--rows 1000000,10000000] [--reps 9] [--out FILE]
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

from sparse_bench import HBM_GBPS, _stats  # noqa: E402

DIM, N_COLS = 8, 3
PREDS = (1, 64)
CLAUSES = (1, 3)
WARMUPS = 3
LO, HI = 1, 2


def _timed(fn, reps):
    for _ in range(WARMUPS):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return _stats(ts)


def predicates(P, n_clauses, rng):
    """P predicates of n_clauses clauses, one per column, each with bounds of its own."""
    out = []
    for _ in range(P):
        pred = []
        for c in range(n_clauses):
            lo = float(rng.uniform(0.0, 0.5))
            pred.append((c, lo, lo + float(rng.uniform(0.2, 0.5)), LO | HI))
        out.append(pred)
    return out


def numpy_masks(cols, preds):
    """The host restatement: compares, ANDs and packbits (little bit order, the row_mask layout)."""
    n = cols.shape[1]
    W = (n + 31) // 32
    masks = np.zeros((len(preds), W), np.uint32)
    counts = np.zeros(len(preds), np.int64)
    for p, pred in enumerate(preds):
        bits = np.ones(n, bool)
        for slot, lo, hi, _ in pred:
            v = cols[slot]
            bits &= (v >= lo) & (v <= hi)
        packed = np.packbits(bits, bitorder="little")
        masks[p].view(np.uint8)[:packed.size] = packed
        counts[p] = int(bits.sum())
    return masks, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error("--reps must be at least 9")
    import torch
    from service import _vdb
    rng = np.random.default_rng(0)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for rows in [int(r) for r in args.rows.split(",")]:
        ix = _vdb.NativeIndex(DIM, "cosine")
        step = 1_000_000
        for s in range(0, rows, step):
            ix.add(rng.standard_normal((min(step, rows - s), DIM), dtype=np.float32))
        cols = rng.random((N_COLS, rows))
        cols[:, ::17] = np.nan  # rows without a value
        for c in range(N_COLS):
            ix.set_column(c, cols[c])
        W = (rows + 31) // 32
        emit({"what": "corpus", "rows": rows, "columns": N_COLS, "column_bytes": rows * 8, "mask_words": W})
        for P in PREDS:
            for nc in CLAUSES:
                preds = predicates(P, nc, rng)
                common = {"rows": rows, "P": P, "clauses": nc}
                want_m, want_c = numpy_masks(cols, preds)
                got_m, got_c = ix.filter_mask(preds)
                assert np.array_equal(got_m, want_m) and np.array_equal(got_c, want_c), "device and numpy disagree"
                h = _timed(lambda: ix.filter_mask(preds), args.reps)
                h.update({"what": "filter_mask, host memory", **common})
                emit(h)
                clauses, offs = _vdb.pack_predicates(preds)
                out = torch.empty(P * W, dtype=torch.int32, device="cuda")
                cnt = torch.empty(P, dtype=torch.int64, device="cuda")
                stream = torch.cuda.Stream()
                ts = []
                for it in range(WARMUPS + args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record()
                        ix.filter_mask_device(clauses, offs, 0, out.data_ptr(), cnt.data_ptr(), stream=stream.cuda_stream)
                        e1.record()
                    e1.synchronize()
                    if it >= WARMUPS:
                        ts.append(e0.elapsed_time(e1) * 1e-3)
                d = _stats(ts)
                moved = nc * rows * 8 + P * W * 4
                gbps = moved / (d["median_ms"] * 1e-3) / 1e9
                d.update({"what": "filter_mask, device memory (events)", "bytes": moved, "gb_per_s": round(gbps, 1),
                          "of_hbm": round(gbps / HBM_GBPS, 4), **common})
                emit(d)
                assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(P, W), want_m)
                reps_np = args.reps if rows * P <= 64_000_000 else 3  # (the largest restatement takes seconds)
                ts = []
                for _ in range(reps_np):
                    t0 = time.perf_counter()
                    numpy_masks(cols, preds)
                    ts.append(time.perf_counter() - t0)
                npy = _stats(ts)
                npy.update({"what": "numpy restatement with packbits, host", **common})
                emit(npy)
        ix.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

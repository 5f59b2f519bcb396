#!/usr/bin/env python3
"""What vdb_index_encode_codes and vdb_index_encode cost: standard-normal rows and
projections, every argument in device memory.

  encode_codes   1M x 768 -> 1 024 bits, 10M x 128 -> 256 bits, and 1M x 768 sign bits.  The call
                 returns when the column is attached, so a call is timed on the host clock around it
                 (allocation of its scratch, kernels, tiling, synchronisation): the median of several
                 calls with their range, knob "encode_mfma" at 0 and (once: it is slow) at 2, the share
                 of pairs that paid fp64 (the stat "encode_exact_pairs") beside the derived estimate
                 0.8 * 2.02 (D + 8) 2^-24 sqrt(D), the useful flop rate against the fp32-MFMA peak and,
                 for the sign kernel, the row bytes per second against HBM.
  encode         1, 64 and 1 024 queries of 768 dims -> 1 024 bits: device events around windows of
                 back-to-back calls, the median of several windows with their range.
  the other route  what the library offered before: numpy ``X @ P.T > t`` over the host copy of the
                 rows (with the BLAS threads the environment gives: the line records their number),
                 ``packbits``, ``set_codes`` from host memory, timed once.  That route
                 decides in fp32 and is not exact near the threshold: the differing bits are counted.

Run it under a time limit of its own (``timeout -k 10 900 python tools/encode_bench.py``).

  python tools/encode_bench.py [--reps 5] [--out FILE] [--small] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

MFMA_TFLOPS = 157.3  # fp32 matrix peak: 256 CUs x 256 flop per cycle x 2.4 GHz
HBM_GBPS = 8000.0    # the peak DESIGN.md measures bandwidth against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1/100 of the rows (a rehearsal of the script, not a measurement)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy route")
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

    def timed_codes(ix, dp, bits, reps):
        ts, share = [], 0.0
        for _ in range(reps):
            e0 = ix.stat("encode_exact_pairs")
            t0 = time.perf_counter()
            ix.encode_codes_device(dp.data_ptr() if dp is not None else 0, 0, bits)
            ts.append(1e3 * (time.perf_counter() - t0))
            share = (ix.stat("encode_exact_pairs") - e0) / (ix.count() * bits)
        ts.sort()
        return ts, share

    for rows, dim, bits in ((1_000_000, 768, 1024), (10_000_000, 128, 256)):
        if args.small:
            rows //= 100
        X = rng.standard_normal((rows, dim), dtype=np.float32)
        P = rng.standard_normal((bits, dim), dtype=np.float32)
        ix = _vdb.NativeIndex(dim, "cosine")
        for lo in range(0, rows, 1_000_000):
            ix.add(X[lo:lo + 1_000_000])
        dp = torch.from_numpy(P).to("cuda")
        torch.cuda.synchronize()
        flop = 2.0 * rows * dim * bits
        est = 0.8 * 2.02 * (dim + 8) * 2.0 ** -24 * dim ** 0.5
        for knob, reps in ((0, args.reps), (2, 1)):
            ix.set_param("encode_mfma", knob)
            if knob == 0:
                timed_codes(ix, dp, bits, 1)  # warm-up
            ts, share = timed_codes(ix, dp, bits, reps)
            med = ts[len(ts) // 2]
            emit({"what": "encode_codes", "rows": rows, "dim": dim, "bits": bits, "knob": knob, "median_ms": round(med, 2),
                  "min_ms": round(ts[0], 2), "max_ms": round(ts[-1], 2), "calls": len(ts), "fp64_share": round(share, 6),
                  "fp64_share_derived": round(est, 6), "useful_tflops": round(flop / (med * 1e-3) / 1e12, 2),
                  "of_mfma_peak": round(flop / (med * 1e-3) / 1e12 / MFMA_TFLOPS, 4)})
        ix.set_param("encode_mfma", 0)
        if not args.no_cpu:  # the route the library offered before (fp32 decisions: not exact near the threshold)
            ix.encode_codes_device(dp.data_ptr(), 0, bits)
            q = np.arange(0, rows, max(1, rows // 64))[:64]
            probe = ix.encode(X[q], P)
            t0 = time.perf_counter()
            H = ix.get_vectors(0, rows)
            C = np.empty((rows, bits // 8), np.uint8)
            for lo in range(0, rows, 100_000):
                C[lo:lo + 100_000] = np.packbits(H[lo:lo + 100_000] @ P.T > 0, axis=1, bitorder="little")
            ix.set_codes(C)
            ms = 1e3 * (time.perf_counter() - t0)
            emit({"what": "numpy_route", "rows": rows, "dim": dim, "bits": bits, "ms": round(ms, 1),
                  "blas_threads": blas_threads(),
                  "bits_differing_in_64_rows": int(np.unpackbits(C[q] ^ probe).sum())})
            del H, C
        if dim == 768:
            ts, _ = timed_codes(ix, None, dim, 1)
            ts, _ = timed_codes(ix, None, dim, args.reps)
            med = ts[len(ts) // 2]
            gbs = rows * ix_row_bytes(dim) / (med * 1e-3) / 1e9
            emit({"what": "encode_codes_sign", "rows": rows, "dim": dim, "median_ms": round(med, 2), "min_ms": round(ts[0], 2),
                  "max_ms": round(ts[-1], 2), "calls": len(ts), "row_gb_per_s": round(gbs, 1), "of_hbm": round(gbs / HBM_GBPS, 4)})
            st = torch.cuda.current_stream().cuda_stream
            for B in (1, 64, 1024):
                dq = torch.from_numpy(rng.standard_normal((B, dim), dtype=np.float32)).to("cuda")
                out = torch.empty((B, bits // 8), dtype=torch.uint8, device="cuda")

                def call():
                    ix.encode_device(dq.data_ptr(), B, dp.data_ptr(), 0, bits, out.data_ptr(), stream=st)

                for _ in range(3):
                    call()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ts = []
                for _ in range(args.reps):
                    e0.record()
                    for _ in range(50):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) / 50)
                ts.sort()
                emit({"what": "encode", "B": B, "dim": dim, "bits": bits, "median_ms": round(ts[len(ts) // 2], 4),
                      "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "windows": len(ts), "calls_per_window": 50})
        ix.close()
        del X
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def blas_threads():
    """The threads numpy's BLAS runs the numpy route's products with: what threadpoolctl reports, else what
    the environment asks for; the script sets neither."""
    try:
        from threadpoolctl import threadpool_info
        n = [p["num_threads"] for p in threadpool_info() if p.get("user_api") == "blas"]
        if n:
            return max(n)
    except ImportError:
        pass
    env = os.environ.get("OPENBLAS_NUM_THREADS") or os.environ.get("MKL_NUM_THREADS") or os.environ.get("OMP_NUM_THREADS")
    return f"env {env}" if env else "not controlled"


def ix_row_bytes(dim):
    """Bytes of a stored row: the dim padded to a multiple of 64, fp32."""
    return (dim + 63) // 64 * 64 * 4


if __name__ == "__main__":
    main()

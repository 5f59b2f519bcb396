#!/usr/bin/env python3
"""What vdb_index_search_fused costs: on 1M x 768 cosine rows, 64 sets of 4
sub-queries, k = 10, fetch_k = 40, the time of
  1. ``search_fused`` (host memory, complete on return), RRF and MAX,
  2. the inner ``search(fetch_k)`` of the 256 vectors alone,
  3. the host alternative a user has without the call: that batch search, the lists pulled to the
     host, de-duplicated in a dict that adds the reciprocal ranks, and sorted,
each the median of repeated calls after warm-up with their range, one JSON line per measurement.

Every GPU step is a child process of its own under ``timeout -k 10``; the first that fails ends the
run.  ``--profile`` adds one run of the fused calls under ``rocprofv3 --kernel-trace`` (a run of its
own: tracing slows the host) and reports the fuse kernel's own time per call.

  python tools/fused_bench.py [--rows 1000000] [--reps 25] [--out DIR] [--profile]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

DIM, METRIC = 768, "cosine"
SETS, PER_SET, K, FETCH, RRF_C = 64, 4, 10, 40, 60.0


def _stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(1e3 * ts[len(ts) // 2], 4), "min_ms": round(1e3 * ts[0], 4),
            "max_ms": round(1e3 * ts[-1], 4), "runs": len(ts)}


def _timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return _stats(ts)


def _dict_rrf(idx, offs, k, c):
    """The usual host fusion: reciprocal ranks added per row id in a dict, then sorted."""
    out = []
    for s in range(len(offs) - 1):
        acc = {}
        for l in range(offs[s], offs[s + 1]):
            for p, r in enumerate(idx[l].tolist()):
                if r >= 0:
                    acc[r] = acc.get(r, 0.0) + 1.0 / (c + p + 1)
        out.append(sorted(acc.items(), key=lambda kv: (-kv[1], kv[0]))[:k])
    return out


def child(args):
    import numpy as np
    from service import _vdb
    ix = _vdb.NativeIndex(DIM, METRIC)
    rng = np.random.default_rng(4321)
    for r0 in range(0, args.rows, 100000):
        ix.add(rng.standard_normal((min(100000, args.rows - r0), DIM)).astype(np.float32))
    base_q = rng.standard_normal((SETS, 1, DIM)).astype(np.float32)
    Q = (base_q + 0.5 * rng.standard_normal((SETS, PER_SET, DIM)).astype(np.float32)).reshape(-1, DIM)
    offs = np.arange(0, SETS * PER_SET + 1, PER_SET, dtype=np.int64)
    base = {"dim": DIM, "metric": METRIC, "rows": args.rows, "sets": SETS, "per_set": PER_SET, "k": K, "fetch_k": FETCH}

    def fused_rrf():
        return ix.search_fused(Q, offs, K, FETCH, "rrf", rrf_c=RRF_C)

    def fused_max():
        return ix.search_fused(Q, offs, K, FETCH, "max")

    def inner():
        return ix.search(Q, FETCH)

    def host():
        _, idx = ix.search(Q, FETCH)
        return _dict_rrf(idx, offs.tolist(), K, RRF_C)

    if args.profile_child:
        for _ in range(3 + args.reps):
            fused_rrf()
        ix.close()
        return 0
    for what, fn in (("search_fused_rrf", fused_rrf), ("search_fused_max", fused_max), ("search_fetch_k", inner),
                     ("host_alternative", host)):
        print(json.dumps(dict(base, what=what, **_timed(fn, args.reps))), flush=True)
    # the two reads rank the same rows (the dict's sums are the same fp64 operations)
    got = fused_rrf()[1]
    want = host()
    assert all(got[s].tolist() == [r for r, _ in want[s]] for s in range(SETS))
    ix.close()
    return 0


def _fuse_kernel_time(outdir):
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        if not rows:
            continue
        cols = {c.lower(): c for c in rows[0]}
        name_c, start_c, end_c = cols.get("kernel_name"), cols.get("start_timestamp"), cols.get("end_timestamp")
        if not (name_c and start_c and end_c):
            continue
        d = sorted(int(r[end_c]) - int(r[start_c]) for r in rows if "fuse_kernel" in r[name_c])
        if d:
            return {"launches": len(d), "median_us": round(d[len(d) // 2] / 1e3, 2), "min_us": round(d[0] / 1e3, 2),
                    "max_us": round(d[-1] / 1e3, 2)}
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default="bench_out/fused")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--limit", type=int, default=420, help="seconds per GPU step")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--profile-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child or args.profile_child:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    own = [sys.executable, os.path.abspath(__file__), "--rows", str(args.rows), "--reps", str(args.reps)]
    steps = [["timeout", "-k", "10", str(args.limit)] + own + ["--child"]]
    prof_dir = os.path.join(args.out, "prof")
    if args.profile:
        steps.append(["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv",
                      "-d", prof_dir, "--"] + own + ["--profile-child"])
    for n, cmd in enumerate(steps):
        r = subprocess.run(cmd, stdout=subprocess.PIPE if n == 0 else subprocess.DEVNULL, text=True)
        if n == 0:
            sys.stdout.write(r.stdout)
            with open(os.path.join(args.out, "fused.jsonl"), "w") as f:
                f.write(r.stdout)
        if r.returncode != 0:
            print(f"step failed with status {r.returncode}: {' '.join(cmd)}", file=sys.stderr)
            return r.returncode
    if args.profile:
        got = _fuse_kernel_time(prof_dir)
        if got is None:
            print(f"no fuse kernel found in a trace under {prof_dir}", file=sys.stderr)
            return 1
        print(json.dumps(dict({"what": "fuse_kernel", "sets": SETS, "per_set": PER_SET, "k": K, "fetch_k": FETCH}, **got)),
              flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

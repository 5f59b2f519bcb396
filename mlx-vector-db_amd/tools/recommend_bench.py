#!/usr/bin/env python3
"""What vdb_index_search_recommend costs: per corpus (1M x 768 cosine, 1M x 128 L2),
batch (1, 64) and examples per query (4, 64; a quarter of them negatives), k = 10, the time of
  1. ``search_recommend`` (host memory, complete on return),
  2. the inner ``search(k + examples)`` alone on the same built queries,
  3. the host alternative a user has without the call: one ``get_vectors`` per example, the means
     in numpy, ``search(k + examples)`` and the examples dropped from the answer,
each the median of repeated calls with their range, one JSON line per measurement.

Every GPU step is a child process of its own under ``timeout -k 10``; the first that fails ends the
run.  ``--profile`` adds, per corpus, one run of the B = 64 calls under ``rocprofv3 --kernel-trace``
(a run of its own: tracing slows the host) and reports the share of the call's kernel time
spent in the build kernel, the select kernel and the inner search.

  python tools/recommend_bench.py [--rows 1000000] [--reps 15] [--out DIR] [--profile]
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

CORPORA = ((768, "cosine"), (128, "euclidean"))
BATCHES = (1, 64)
EXAMPLES = (4, 64)
K = 10


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


def _build(dim, metric, rows):
    import numpy as np
    from service import _vdb
    ix = _vdb.NativeIndex(dim, metric)
    rng = np.random.default_rng(1234 + dim)
    for r0 in range(0, rows, 100000):
        ix.add(rng.standard_normal((min(100000, rows - r0), dim)).astype(np.float32))
    return ix, rng


def child(args):
    import numpy as np
    ix, rng = _build(args.dim, args.metric, args.rows)
    base = {"dim": args.dim, "metric": args.metric, "rows": args.rows, "k": K}
    for B in (BATCHES if not args.profile_child else (64,)):
        for E in EXAMPLES:
            ids = [rng.choice(args.rows, size=E, replace=False) for _ in range(B)]
            pos = [r[:E - E // 4] for r in ids]
            neg = [r[E - E // 4:] for r in ids]

            def rec():
                return ix.search_recommend(pos, neg, K)

            built = ix.search_recommend(pos, neg, K, with_queries=True)[2]

            def inner():
                return ix.search(built, K + E)

            def mean_of(rows):
                X = np.concatenate([ix.get_vectors(int(r), 1) for r in rows])
                if args.metric == "cosine":
                    X = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-8)
                return X.mean(axis=0)

            def host():
                Q = np.stack([2.0 * mean_of(p) - mean_of(g) for p, g in zip(pos, neg)]).astype(np.float32)
                scores, idx = ix.search(Q, K + E)
                return [idx[b][~np.isin(idx[b], ids[b])][:K] for b in range(B)]

            if args.profile_child:
                for _ in range(3 + args.reps):
                    rec()
                continue
            for what, fn, reps in (("search_recommend", rec, args.reps), ("search_k_plus_examples", inner, args.reps),
                                   ("host_alternative", host, max(3, args.reps // 3))):
                print(json.dumps(dict(base, what=what, B=B, examples=E, **_timed(fn, reps))), flush=True)
            # do the two reads agree on the best row?  (the host's fp32 means differ in their last bits)
            print(json.dumps(dict(base, what="first_row_agrees", B=B, examples=E,
                                  value=bool(int(rec()[1][0, 0]) == int(host()[0][0])))), flush=True)
    ix.close()


def _kernel_shares(outdir, calls_per_case):
    """Per example count: the kernel time of one call and its shares (build kernel, select kernel, the
    inner search), from rocprofv3's kernel trace.  A call ends with its select kernel, so call c is
    the dispatches after select c - 1 up to select c; the first call of the run (which follows the
    ingest) is left out.  (Each case's ``with_queries`` call is one more call in front of its run.)"""
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        if not rows:
            continue
        cols = {c.lower(): c for c in rows[0]}
        name_c, start_c, end_c = cols.get("kernel_name"), cols.get("start_timestamp"), cols.get("end_timestamp")
        if not (name_c and start_c and end_c):
            continue
        rows.sort(key=lambda r: int(r[start_c]))
        out, call, cur = [], 0, {"build": 0, "select": 0, "search": 0}
        sums = [dict(build=0, select=0, search=0, calls=0) for _ in EXAMPLES]
        for r in rows:
            name, dur = r[name_c], int(r[end_c]) - int(r[start_c])
            key = "build" if "recommend_build_kernel" in name else "select" if "recommend_select_kernel" in name \
                else "search"
            cur[key] += dur
            if key == "select":
                case = call // calls_per_case
                if call > 0 and case < len(EXAMPLES):
                    for k2 in ("build", "select", "search"):
                        sums[case][k2] += cur[k2]
                    sums[case]["calls"] += 1
                call += 1
                cur = {"build": 0, "select": 0, "search": 0}
        for E, s in zip(EXAMPLES, sums):
            tot = s["build"] + s["select"] + s["search"]
            if not s["calls"] or not tot:
                continue
            out.append({"examples": E, "calls": s["calls"],
                        "kernel_us_per_call": round(tot / s["calls"] / 1e3, 2),
                        "build_us_per_call": round(s["build"] / s["calls"] / 1e3, 2),
                        "select_us_per_call": round(s["select"] / s["calls"] / 1e3, 2),
                        "inner_search_us_per_call": round(s["search"] / s["calls"] / 1e3, 2),
                        "share_build": round(s["build"] / tot, 4), "share_select": round(s["select"] / tot, 4),
                        "share_inner_search": round(s["search"] / tot, 4)})
        return out, path
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="bench_out/recommend")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--limit", type=int, default=420, help="seconds per GPU step")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--profile-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dim", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--metric", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child or args.profile_child:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    for dim, metric in CORPORA:
        own = [sys.executable, os.path.abspath(__file__), "--rows", str(args.rows), "--reps", str(args.reps),
               "--dim", str(dim), "--metric", metric]
        steps = [["timeout", "-k", "10", str(args.limit)] + own + ["--child"]]
        prof_dir = os.path.join(args.out, f"prof_{dim}_{metric}")
        if args.profile:
            steps.append(["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace",
                          "--output-format", "csv", "-d", prof_dir, "--"] + own + ["--profile-child"])
        for n, cmd in enumerate(steps):
            r = subprocess.run(cmd, stdout=subprocess.PIPE if n == 0 else subprocess.DEVNULL, text=True)
            if n == 0:
                sys.stdout.write(r.stdout)
                with open(os.path.join(args.out, f"recommend_{dim}_{metric}.jsonl"), "w") as f:
                    f.write(r.stdout)
            if r.returncode != 0:
                print(f"step failed with status {r.returncode}: {' '.join(cmd)}", file=sys.stderr)
                return r.returncode
        if args.profile:
            got = _kernel_shares(prof_dir, 4 + args.reps)  # (+ 1: the with_queries call of each case)
            if got is None:
                print(f"no kernel trace found under {prof_dir}", file=sys.stderr)
                return 1
            for row in got[0]:
                print(json.dumps(dict({"dim": dim, "metric": metric, "what": "kernel_time_shares", "B": 64}, **row)),
                      flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

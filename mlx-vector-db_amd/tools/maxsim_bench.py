#!/usr/bin/env python3
"""What vdb_index_search_maxsim costs: on 1M x 768 cosine rows and 1M x 128
euclidean rows, for one set of 1, 8, 32 and 64 query vectors, k = 10, the time of
  1. ``search_maxsim`` (host memory, complete on return) with documents of 16 consecutive rows (a
     wave folds each document's rows and issues one atomic per (document, query vector)) and with
     the same number of documents dealt ``row % documents`` (no two neighbouring rows share a
     document: one atomic per (row, query vector), which shows what the run combining buys),
  2. ``search_range(cap = 0)`` over the same query vectors: the same read of the rows and the same
     key arithmetic with no atomics and no table,
  3. the host alternative a user has without the call: the vectors x rows score matrix in numpy
     (fp32 matmul over normalised rows / expanded squared distances), the per-document maxima and
     their sums (sets of 8 and 64 only, three runs: it takes seconds),
each the median of repeated calls after warm-up with their range, one JSON line per measurement, and
for every maxsim line the ratio of its median to the range scan's.  The maxsim groups are compared
with the host alternative's (the same documents first; the host's fp32 scores can order near-ties
differently, so the overlap of the two top-k sets is reported, not asserted).

Every GPU step is a child process of its own under ``timeout -k 10``; the first that fails ends the
run.

  python tools/maxsim_bench.py [--rows 1000000] [--reps 15] [--out DIR] [--shape 768|128|both]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SHAPES = {"768": (768, "cosine"), "128": (128, "euclidean")}
PER_DOC, K = 16, 10
SET_SIZES = (1, 8, 32, 64)
HOST_SETS = (8, 64)


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


def child(args):
    import numpy as np
    from service import _vdb
    dim, metric = SHAPES[args.child]
    rows = args.rows // PER_DOC * PER_DOC
    docs = rows // PER_DOC
    ix = _vdb.NativeIndex(dim, metric)
    rng = np.random.default_rng(4321)
    V = np.empty((rows, dim), np.float32)
    for r0 in range(0, rows, 100000):
        V[r0:r0 + 100000] = rng.standard_normal((min(100000, rows - r0), dim)).astype(np.float32)
        ix.add(V[r0:r0 + 100000])
    Qall = rng.standard_normal((max(SET_SIZES), dim)).astype(np.float32)
    layouts = {"consecutive16": (np.arange(rows) // PER_DOC).astype(np.int32),
               "modulo": (np.arange(rows) % docs).astype(np.int32)}
    base = {"dim": dim, "metric": metric, "rows": rows, "documents": docs, "k": K}
    if metric == "cosine":
        Vn = V / np.maximum(np.linalg.norm(V, axis=1, keepdims=True), 1e-8)
        vsq = None
    else:
        Vn, vsq = V, (V.astype(np.float32) ** 2).sum(axis=1)

    def host_alt(Q, layout):
        if metric == "cosine":
            S = (Q / np.maximum(np.linalg.norm(Q, axis=1, keepdims=True), 1e-8)) @ Vn.T
        else:
            S = -(vsq[None, :] - 2.0 * (Q @ Vn.T) + (Q ** 2).sum(axis=1)[:, None])
        M = S.reshape(Q.shape[0], docs, PER_DOC).max(axis=2) if layout == "consecutive16" else \
            S.reshape(Q.shape[0], PER_DOC, docs).max(axis=1)
        total = M.astype(np.float64).sum(axis=0)
        top = np.argpartition(-total, K)[:K]
        return top[np.lexsort((top, -total[top]))]

    range_ms = {}
    for m in SET_SIZES:
        Q = Qall[:m]
        thr = np.full(m, 2.0 if metric == "cosine" else 0.0)  # nothing passes: the scan alone
        st = _timed(lambda: ix.search_range(Q, thr, cap=0), args.reps)
        range_ms[m] = st["median_ms"]
        print(json.dumps(dict(base, what="search_range_cap0", vectors=m, **st)), flush=True)
    for name, col in layouts.items():
        ix.set_groups(col)
        for m in SET_SIZES:
            Q = Qall[:m]
            offs = np.asarray([0, m], np.int64)
            st = _timed(lambda: ix.search_maxsim((Q, offs), docs, K), args.reps)
            print(json.dumps(dict(base, what="search_maxsim", layout=name, vectors=m,
                                  ratio_to_range=round(st["median_ms"] / range_ms[m], 3), **st)), flush=True)
            if m in HOST_SETS:
                hs = _timed(lambda: host_alt(Q, name), 3, warm=1)
                got = ix.search_maxsim((Q, offs), docs, K)[1][0]
                want = host_alt(Q, name)
                print(json.dumps(dict(base, what="host_alternative", layout=name, vectors=m,
                                      top_k_overlap=int(np.intersect1d(got, want).size),
                                      same_first=bool(got[0] == want[0]), **hs)), flush=True)
    assert ix.stat("maxsim_skipped_rows") == 0 and ix.stat("maxsim_bad_sets") == 0
    ix.close()
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="bench_out/maxsim")
    ap.add_argument("--shape", default="both", choices=["768", "128", "both"])
    ap.add_argument("--limit", type=int, default=420, help="seconds per GPU step")
    ap.add_argument("--child", default=None, choices=list(SHAPES), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    shapes = list(SHAPES) if args.shape == "both" else [args.shape]
    with open(os.path.join(args.out, "maxsim.jsonl"), "w") as f:
        for shape in shapes:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--rows",
                   str(args.rows), "--reps", str(args.reps), "--child", shape]
            with subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True) as p:
                for line in p.stdout:  # each measurement as it is made
                    sys.stdout.write(line)
                    sys.stdout.flush()
                    f.write(line)
                    f.flush()
            if p.returncode != 0:
                print(f"step failed with status {p.returncode}: {' '.join(cmd)}", file=sys.stderr)
                return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

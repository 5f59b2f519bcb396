#!/usr/bin/env python3
"""Row-list search against the masked search, same index, same rows.

For each shape (1 M x 768 cosine, 1 M x 128 L2; a fresh index each) and each eligible fraction
(0.01 %, 0.1 %, 1 %, 5 %, 25 % of the rows, drawn at random): B = 1 and B = 64 with one shared
list, and B = 64 with 64 distinct lists.  ``NativeIndex.search_rows`` is timed against
``NativeIndex.search`` with the list's bitmap as row_mask (for distinct lists: one masked search
per query, which is what a batch of differently filtered queries costs without row lists), host
memory, median of 20 calls after 5 warm-ups with the range reported, and the two are asserted to
return identical indices and keys.  The crossover per batch form is interpolated (log-log) between
the first two fractions between which the row-list search stops being the faster one.

Run without arguments: each shape runs as a child process under its own ``timeout -k 10``, and
nothing more is started after one fails.  Prints one JSON line per measurement and a table.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (os.path.join(ROOT, "mlx-vector-db_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"c2": (1_000_000, 768, "cosine"), "l2": (1_000_000, 128, "euclidean")}
FRACTIONS = (0.0001, 0.001, 0.01, 0.05, 0.25)
K = 10


def _time(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def run_shape(name, reps, warm, rows_override=None):
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime per process)
    from service import _vdb

    n, d, metric = SHAPES[name]
    if rows_override:
        n = rows_override
    rng = np.random.default_rng(17)
    ix = _vdb.NativeIndex(d, metric)
    ix.reserve(n)
    for s in range(0, n, 250_000):
        ix.add(rng.standard_normal((min(250_000, n - s), d), dtype=np.float32))
    Q = rng.standard_normal((64, d), dtype=np.float32)
    out = []
    for frac in FRACTIONS:
        m = max(1, int(round(frac * n)))
        lists = [np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64) for _ in range(64)]
        masks = [_vdb.rows_to_bitmap(l, n) for l in lists]
        forms = {
            "B1": (Q[:1], [lists[0]], None, lambda: [ix.search(Q[:1], K, row_mask=masks[0], with_keys=True)]),
            "B64_shared": (Q, [lists[0]], np.zeros(64, np.int32),
                           lambda: [ix.search(Q, K, row_mask=masks[0], with_keys=True)]),
            "B64_distinct": (Q, lists, None,
                             lambda: [ix.search(Q[b:b + 1], K, row_mask=masks[b], with_keys=True) for b in range(64)]),
        }
        for form, (q, ls, ql, masked) in forms.items():
            offs, rows = _vdb.pack_row_lists(ls)
            sub = lambda: ix.search_rows_csr(q, K, offs, rows, ql, with_keys=True)  # noqa: E731
            got = sub()
            want = masked()
            wi = np.concatenate([w[1] for w in want])
            wk = np.concatenate([w[2] for w in want])
            assert np.array_equal(got[1], wi) and np.array_equal(got[2], wk), (name, frac, form)
            r = reps if m * len(ls) <= 4_000_000 else max(5, reps // 4)  # (the 128 MB argument copies)
            ts = _time(sub, r, warm)
            tm = _time(masked, r, warm)
            rec = {"shape": name, "rows": n, "dim": d, "metric": metric, "fraction": frac, "ids_per_list": m,
                   "form": form, "subset_ms": round(ts[0], 4), "subset_min_max": [round(ts[1], 4), round(ts[2], 4)],
                   "masked_ms": round(tm[0], 4), "masked_min_max": [round(tm[1], 4), round(tm[2], 4)], "reps": r}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    ix.close()
    for form in ("B1", "B64_shared", "B64_distinct"):
        recs = [r for r in out if r["form"] == form]
        cross = None
        for a, b in zip(recs, recs[1:]):
            ra, rb = a["subset_ms"] / a["masked_ms"], b["subset_ms"] / b["masked_ms"]
            if ra <= 1.0 < rb:  # log-log interpolation of the ratio to 1
                t = math.log(1.0 / ra) / math.log(rb / ra)
                cross = math.exp(math.log(a["fraction"]) + t * (math.log(b["fraction"]) - math.log(a["fraction"])))
                break  # the first crossing: the fraction up to which the row-list search never loses
        if cross is None:
            cross = 0.0 if recs[0]["subset_ms"] > recs[0]["masked_ms"] else recs[-1]["fraction"]
        print(json.dumps({"shape": name, "form": form, "crossover_fraction": round(cross, 6)}), flush=True)
    print(f"{'shape':6}{'form':14}{'fraction':>10}{'ids':>9}{'rows ms':>10}{'masked ms':>11}")
    for r in out:
        print(f"{r['shape']:6}{r['form']:14}{r['fraction']:>10.4%}{r['ids_per_list']:>9}{r['subset_ms']:>10.3f}"
              f"{r['masked_ms']:>11.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=0, help="fewer rows than the shape's (a quick look)")
    ap.add_argument("--step-timeout", type=int, default=420)
    a = ap.parse_args()
    if a.shape:
        run_shape(a.shape, a.reps, a.warmup, a.rows or None)
        return 0
    for name in SHAPES:  # one GPU step per shape, each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--shape", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--rows", str(a.rows)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"{name}: exit {rc}; nothing more is run", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

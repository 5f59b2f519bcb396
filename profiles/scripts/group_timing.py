#!/usr/bin/env python3
"""Grouped search against the only alternative the library had, same index, same rows.

For each shape (1 M x 768 cosine, 1 M x 128 L2), group columns of 1, 8 and 64 rows per group --
assigned at random over a standard-normal corpus ("random"), or as clustered documents, where the
chunks of a group are the group's centre plus noise and the queries are noisy copies of centres
("clustered": a fresh index per group size) -- and B = 1 and 64, k = 10, host memory, median of 20
calls after 5 warm-ups with the range reported:

  * ``NativeIndex.search_groups`` at the auto ``group_fetch`` (k' = 200) and at k' = 40 (the rule the
    call started from, min(200, max(32, 4 k))), with the queries that took the exact fallback per batch;
  * the alternative without the call: ``search(k')`` at the same k' plus a host de-duplication of
    the fetched rows' groups, and the number of queries for which it returned fewer than k groups;
  * the same call with ``group_force_exact`` = 1.

Run without arguments: each shape runs as a child process under its own ``timeout -k 10``, and
nothing more is started after one fails.  Prints one JSON line per measurement and a table.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (os.path.join(ROOT, "mlx-vector-db_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"c2": (1_000_000, 768, "cosine"), "l2": (1_000_000, 128, "euclidean")}
GROUP_ROWS = (1, 8, 64)
BATCHES = (1, 64)
K = 10
NOISE = 0.3  # a chunk = its document's centre + NOISE * N(0, 1)


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


def _fetch_k(knob, k):  # csrc/vdb_group_plan.h group_fetch_k
    return max(min(knob if knob > 0 else (1 if k == 1 else 200), 200), k)


def _dedup(idx, groups, k, np):
    """The host side of the alternative: the fetched rows' groups, first occurrences, the first k."""
    out = []
    for row in idx:
        g = groups[row[row >= 0]]
        _, first = np.unique(g, return_index=True)
        out.append(np.sort(first)[:k])
    return out


def _build(vdb, np, n, d, metric, rng, layout, per):
    """(index, groups, queries) of one (layout, rows per group) setting."""
    n_groups = max(1, n // per)
    ix = vdb.NativeIndex(d, metric)
    ix.reserve(n)
    if layout == "random":
        groups = rng.integers(0, n_groups, size=n).astype(np.int32)
        for s in range(0, n, 250_000):
            ix.add(rng.standard_normal((min(250_000, n - s), d), dtype=np.float32))
        Q = rng.standard_normal((64, d), dtype=np.float32)
    else:
        groups = (np.arange(n) // per).astype(np.int32)
        centres = rng.standard_normal((n_groups, d), dtype=np.float32)
        for s in range(0, n, 250_000):
            m = min(250_000, n - s)
            ix.add(centres[groups[s:s + m]] + NOISE * rng.standard_normal((m, d), dtype=np.float32))
        Q = centres[rng.choice(n_groups, size=64, replace=n_groups < 64)] + \
            NOISE * rng.standard_normal((64, d), dtype=np.float32)
    ix.set_groups(groups)
    return ix, groups, np.ascontiguousarray(Q, dtype=np.float32)


def _measure(ix, groups, Q, name, layout, per, knob, reps, warm, np, out):
    kf = _fetch_k(knob, K)
    ix.set_param("group_fetch", knob)
    for B in BATCHES:
        q = Q[:B]
        ix.set_param("group_force_exact", 0)
        fb0 = ix.stat("group_fallback_queries")
        got = ix.search_groups(q, K, with_keys=True)
        fallback = ix.stat("group_fallback_queries") - fb0
        tg = _time(lambda: ix.search_groups(q, K, with_keys=True), reps, warm)
        alt = lambda: _dedup(ix.search(q, kf, with_keys=True)[1], groups, K, np)  # noqa: E731
        short = sum(1 for f in alt() if f.size < K)
        ta = _time(alt, reps, warm)
        ts = _time(lambda: ix.search(q, kf, with_keys=True), reps, warm)
        ix.set_param("group_force_exact", 1)
        ex = ix.search_groups(q, K, with_keys=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ex)), (name, layout, per, B)
        te = _time(lambda: ix.search_groups(q, K, with_keys=True), max(3, reps // 4), 1)
        rec = {"shape": name, "layout": layout, "rows_per_group": per, "B": B, "k": K, "fetch": kf,
               "groups_ms": round(tg[0], 4), "groups_min_max": [round(tg[1], 4), round(tg[2], 4)],
               "fallback_queries": int(fallback),
               "search_dedup_ms": round(ta[0], 4), "search_dedup_min_max": [round(ta[1], 4), round(ta[2], 4)],
               "search_ms": round(ts[0], 4), "alt_short_queries": int(short),
               "over_inner_search_ms": round(tg[0] - ts[0], 4),
               "force_exact_ms": round(te[0], 4), "reps": reps}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    ix.set_param("group_force_exact", 0)


def run_shape(name, reps, warm, rows_override=None):
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime per process)
    from service import _vdb

    n, d, metric = SHAPES[name]
    if rows_override:
        n = rows_override
    rng = np.random.default_rng(29)
    out = []
    # random assignment: one corpus, three columns
    ix, groups, Q = _build(_vdb, np, n, d, metric, rng, "random", 1)
    for per in GROUP_ROWS:
        groups = rng.integers(0, max(1, n // per), size=n).astype(np.int32)
        ix.set_groups(groups)
        for knob in (0, 40):
            _measure(ix, groups, Q, name, "random", per, knob, reps, warm, np, out)
    ix.close()
    for per in GROUP_ROWS[1:]:  # (one row per group is the same either way)
        ix, groups, Q = _build(_vdb, np, n, d, metric, rng, "clustered", per)
        for knob in (0, 40):
            _measure(ix, groups, Q, name, "clustered", per, knob, reps, warm, np, out)
        ix.close()
    print(f"{'shape':6}{'layout':>10}{'/grp':>6}{'B':>4}{'k_f':>5}{'groups ms':>11}{'fallback':>9}{'search+dedup':>14}"
          f"{'short':>7}{'search ms':>11}{'exact ms':>10}")
    for r in out:
        print(f"{r['shape']:6}{r['layout']:>10}{r['rows_per_group']:>6}{r['B']:>4}{r['fetch']:>5}{r['groups_ms']:>11.3f}"
              f"{r['fallback_queries']:>9}{r['search_dedup_ms']:>14.3f}{r['alt_short_queries']:>7}{r['search_ms']:>11.3f}"
              f"{r['force_exact_ms']:>10.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=0, help="fewer rows than the shape's (a quick look)")
    ap.add_argument("--step-timeout", type=int, default=540)
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

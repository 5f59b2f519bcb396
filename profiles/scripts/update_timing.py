#!/usr/bin/env python3
"""Time in-place row update on the device against remove + add (DESIGN.md "Updating rows").

    python profiles/scripts/update_timing.py [--rows 1000000] [--dim 768] [--reps 5]

At C2's corpus (1M x 768 cosine, precision auto), for a random 1 % and a random 50 % of the rows,
with the new rows in host memory and in device memory:

  * update: ``NativeIndex.update(rows, new)`` / ``update_device`` (include/vdb.h
    vdb_index_update), median of ``--reps`` runs, a fresh index each time (the add is not timed);
  * what a user does without it: ``remove`` of those rows followed by ``add`` of the new ones
    (host memory: a host bitmap and host rows; device memory: both on the device), same process,
    same data, median of ``--reps``.

After each timed run a B = 64, k = 10 search must return the same row CONTENTS whichever route
changed the rows (remove + add renumbers them, so ids differ).  Prints one JSON line with the times
and an estimate of the bytes an update moves.  Run each invocation under a time limit of its own
(``timeout 600 python ...``).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (os.path.join(ROOT, "mlx-vector-db_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

STAGING_BYTES = 256 << 20  # csrc/vdb_api.cpp vdb_index_update: one staging chunk


def moved_bytes(n, D, Dp, host, split_copy=False):
    """Estimate of an update's traffic for n rows (csrc/vdb_api.cpp vdb_index_update): the
    transfer (host memory; twice when the rows exceed one staging chunk), the validation read, the
    old int8 bytes read for the column sums, pack (read D, write Dp + 20 B), quantisation (read 4,
    write 2 + 1 B per element), the new int8 bytes read, the residual along dir (read 4 B per
    element), and 4 + 4 B per element for an existing split copy."""
    src = n * (D * 4 + 8)
    chunks = -(-n * D * 4 // STAGING_BYTES)
    transfer = src * (2 if chunks > 1 else 1) if host else 0
    validate = src
    colsum = 2 * n * Dp * 2
    pack = n * (D * 4 + Dp * 4 + 20)
    quant = n * Dp * (4 + 2 + 1)
    resid = n * Dp * 4
    split = n * Dp * 8 if split_copy else 0
    dev = validate + colsum + pack + quant + resid + split
    return {"transfer": transfer, "device": dev, "total": transfer + dev}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--metric", default="cosine")
    a = ap.parse_args()
    import torch  # (one HIP runtime per process: torch's)
    from service import _vdb
    N, D = a.rows, a.dim
    Dp = (D + 63) // 64 * 64
    rng = np.random.default_rng(0)
    V = rng.random((N, D), dtype=np.float32)
    Q = rng.random((64, D), dtype=np.float32)
    out = {"rows": N, "dim": D, "metric": a.metric, "precision": "auto", "cases": {}}

    def fresh():
        ix = _vdb.NativeIndex(D, a.metric)
        ix.add(V)
        ix.search(Q, 10)  # warm: workspaces, kernels loaded
        return ix

    for name, frac in (("1pct", 0.01), ("50pct", 0.50)):
        rows = rng.permutation(N)[: int(N * frac)].astype(np.int64)
        new = rng.random((rows.size, D), dtype=np.float32)
        Q[0] = new[0]  # one query's top 1 is an updated row
        mask = _vdb.rows_to_bitmap(rows, N)
        V2 = V.copy()
        V2[rows] = new
        # remove + add: the survivors in order, then the new rows in the order given
        S_ids = np.concatenate([np.delete(np.arange(N), rows), rows])  # new position -> old row id
        rows_d = torch.from_numpy(rows).cuda()
        new_d = torch.from_numpy(new).cuda()
        mask_d = torch.from_numpy(mask.view(np.int32)).cuda()
        torch.cuda.synchronize()
        want = None
        for mem in ("host", "device"):
            upd_ms, ra_ms, ra_parts = [], [], []
            for rep in range(a.reps):
                ix = fresh()
                t0 = time.perf_counter()
                if mem == "host":
                    n = ix.update(rows, new)
                else:
                    n = ix.update_device(rows_d.data_ptr(), new_d.data_ptr(), rows.size)
                upd_ms.append((time.perf_counter() - t0) * 1e3)
                assert n == rows.size and ix.count() == N
                s, i = ix.search(Q, 10)
                got = (s, V2[i])  # scores and row contents
                want = got if want is None else want
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                assert i[0, 0] == rows[0]
                ix.close()
            for rep in range(a.reps):
                ix = fresh()
                t0 = time.perf_counter()
                if mem == "host":
                    n = ix.remove(mask)
                    t1 = time.perf_counter()
                    ix.add(new)
                else:
                    n = ix.remove_device(mask_d.data_ptr())
                    t1 = time.perf_counter()
                    ix.add_device(new_d.data_ptr(), rows.size)
                t2 = time.perf_counter()
                ra_ms.append((t2 - t0) * 1e3)
                ra_parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
                assert n == rows.size and ix.count() == N
                s, i = ix.search(Q, 10)
                assert np.array_equal(s, want[0]) and np.array_equal(V2[S_ids[i]], want[1]), "the two routes disagree"
                ix.close()
            mid = sorted(range(len(ra_ms)), key=lambda j: ra_ms[j])[len(ra_ms) // 2]
            b = moved_bytes(rows.size, D, Dp, mem == "host")
            out["cases"][f"{name}_{mem}"] = {
                "updated": int(rows.size),
                "update_ms_median": round(statistics.median(upd_ms), 3),
                "update_ms_all": [round(x, 3) for x in upd_ms],
                "remove_add_ms_median": round(statistics.median(ra_ms), 3),
                "remove_add_ms_all": [round(x, 3) for x in ra_ms],
                "remove_add_median_parts_ms": {"remove": round(ra_parts[mid][0], 3), "add": round(ra_parts[mid][1], 3)},
                "speedup": round(statistics.median(ra_ms) / statistics.median(upd_ms), 2),
                "update_bytes": b,
                "update_effective_GBps": round(b["total"] / (statistics.median(upd_ms) * 1e-3) / 1e9, 1),
            }
        del rows_d, new_d, mask_d
    print(json.dumps(out))


if __name__ == "__main__":
    main()

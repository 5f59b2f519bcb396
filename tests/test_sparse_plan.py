"""The host arithmetic of vdb_index_set_sparse, vdb_index_search_sparse and vdb_index_search_hybrid
(csrc/vdb_sparse_plan.h: the deal of rows to segments and lanes, the clamp of a device call's offsets
and what makes a query bad, the term search, the key of a row, the scratch layouts and the validation
of the column and of the queries) swept on the CPU under AddressSanitizer + UBSan against naive loops:
the stand-alone program tools/sparse_plan_check.cpp, built and run by ``make sparse-plan-check`` in a
child process (nothing is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_sparse_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "sparse-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "-ffp-contract=off" in r.stdout
    assert "sparse plan ok" in r.stdout

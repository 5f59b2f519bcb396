"""The host arithmetic of the inverted sparse search (csrc/vdb_sparse_inv_plan.h: when postings are
built and serve, the row-block size and its LDS layout, the deal of row blocks to segments and waves,
the lower bound by row, and the walk of the postings against sparse_row_key bit for bit) swept on the
CPU under AddressSanitizer + UBSan against naive loops: the stand-alone program
tools/sparse_inv_plan_check.cpp, built and run by ``make sparse-inv-plan-check`` in a child process
(nothing is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_sparse_inv_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "sparse-inv-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "-ffp-contract=off" in r.stdout
    assert "sparse inverted plan ok" in r.stdout

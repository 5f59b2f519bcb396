"""The host arithmetic of vdb_index_search_rows (csrc/vdb_subset_plan.h: workgroups per query, the
walk of a list's chunks by segments and waves, offset clamping, id eligibility, the scratch layout
and the validation of the CSR arguments) swept on the CPU under AddressSanitizer + UBSan against a
naive reference: the stand-alone program tools/subset_plan_check.cpp, built and run by
``make subset-plan-check`` in a child process (nothing is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_subset_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "subset-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "subset plan ok" in r.stdout

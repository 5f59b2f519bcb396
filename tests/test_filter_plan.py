"""The host arithmetic of vdb_index_set_column / vdb_index_filter_mask (csrc/vdb_filter_plan.h: the
clause test the kernel shares, the validation with its causes, the mask width, the deal of word
pairs to waves and workgroups, the last-word rule and the staging and scratch layouts) swept on the
CPU under AddressSanitizer + UBSan against naive loops: the stand-alone program
tools/filter_plan_check.cpp, built and run by ``make filter-plan-check`` in a child process (nothing
is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_filter_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "filter-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "filter plan ok" in r.stdout

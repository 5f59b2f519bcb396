"""The host arithmetic of vdb_index_search_groups (csrc/vdb_group_plan.h: the fetch rule, the
first-occurrence / complete decision the select kernel shares, the deal of rows to the exact
fallback's segments, the scratch layout and the validation) swept on the CPU under
AddressSanitizer + UBSan against naive loops: the stand-alone program tools/group_plan_check.cpp,
built and run by ``make group-plan-check`` in a child process (nothing is loaded into this one).
No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_group_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "group-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "group plan ok" in r.stdout

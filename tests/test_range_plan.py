"""The host arithmetic of vdb_index_search_range (csrc/vdb_range_plan.h: the query-block size, the
deal of bitmap words to workgroups and waves, the prefix and the emit's slot positions, the scratch
layout, the threshold-to-key conversion and the validation) swept on the CPU under
AddressSanitizer + UBSan against naive loops: the stand-alone program tools/range_plan_check.cpp,
built and run by ``make range-plan-check`` in a child process (nothing is loaded into this one).
No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_range_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "range-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "range plan ok" in r.stdout

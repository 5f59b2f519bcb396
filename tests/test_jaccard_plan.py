"""The host arithmetic of vdb_index_search_jaccard (csrc/vdb_jaccard_plan.h: the exact keys of a ratio
with their order and injectivity over Farey neighbours near 8 192 and the u == 0 case, the threshold
test, both forms' block sizes and LDS layouts, the scratch, the validation causes and the choice of
form) swept on the CPU under AddressSanitizer + UBSan against integer arithmetic: the stand-alone program
tools/jaccard_plan_check.cpp, built and run by ``make jaccard-plan-check`` in a child process (nothing is
loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_jaccard_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "jaccard-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout
    assert "jaccard plan ok" in r.stdout

"""The host arithmetic of vdb_index_search_jaccard_range (csrc/vdb_jaccard_range_plan.h: the threshold
test against 128-bit cross-multiplication, what makes a threshold bad, the block size and LDS layouts of
the two scans, the scratch layout, the validation causes and the choice of scan) swept on the CPU under
AddressSanitizer + UBSan against naive loops: the stand-alone program
tools/jaccard_range_plan_check.cpp, built and run by ``make jaccard-range-plan-check`` in a child
process (nothing is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_jaccard_range_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "jaccard-range-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout
    assert "jaccard range plan ok" in r.stdout

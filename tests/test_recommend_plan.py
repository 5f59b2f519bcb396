"""The host arithmetic of vdb_index_search_recommend (csrc/vdb_recommend_plan.h: the validation, the
clamp of a device call's offsets, the list state, the per-element step of the built query with its
rounding, the membership test and the compaction rule the select kernel shares, the fetch size and
the scratch layout) swept on the CPU under AddressSanitizer + UBSan against naive restatements: the
stand-alone program tools/recommend_plan_check.cpp, built and run by ``make recommend-plan-check`` in
a child process (nothing is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_recommend_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "recommend-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "recommend plan ok" in r.stdout

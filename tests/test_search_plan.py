"""The host arithmetic of the main search (csrc/vdb_search_plan.h: KP and its margins, the choice
of candidate pass and its launch geometry, the pilot's sample and rank, the workspace layout and
the exact path's plan) swept on the CPU under AddressSanitizer + UBSan, with the benchmark's own
shapes pinned: the stand-alone program tools/search_plan_check.cpp, built and run by
``make search-plan-check`` in a child process (nothing is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_search_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "search-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "search plan ok" in r.stdout

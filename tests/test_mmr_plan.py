"""The host arithmetic of vdb_index_search_mmr (csrc/vdb_mmr_plan.h: the query-block size, the deal
of position pairs to workgroups and waves, the scratch layout, the validation and the selection step
the select kernel shares) swept on the CPU under AddressSanitizer + UBSan against naive loops: the
stand-alone program tools/mmr_plan_check.cpp, built and run by ``make mmr-plan-check`` in a child
process (nothing is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_mmr_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "mmr-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "mmr plan ok" in r.stdout

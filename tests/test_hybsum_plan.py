"""The host arithmetic of vdb_index_search_hybrid_sum (csrc/vdb_hybsum_plan.h: the deal of rows to
segments, lanes and the batches of the dense keys, the workgroups per query, the scratch layout, the
validation causes and the combination of a row's two keys, -0.0 and both zero weights included) swept
on the CPU under AddressSanitizer + UBSan against naive loops: the stand-alone program
tools/hybsum_plan_check.cpp, built and run by ``make hybsum-plan-check`` in a child process (nothing is
loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_hybsum_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "hybsum-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "-ffp-contract=off" in r.stdout
    assert "hybsum plan ok" in r.stdout

"""The host arithmetic of vdb_index_search_code_dot (csrc/vdb_code_dot_plan.h: both forms' block sizes
and LDS layouts at every width, the plane count rule and the plane sum, the piece mapping of the MFMA
query operand, the K chunking, the key encoding, the validation causes and the choice of form) swept on
the CPU under AddressSanitizer + UBSan against naive loops: the stand-alone program
tools/code_dot_plan_check.cpp, built and run by ``make code-dot-plan-check`` in a child process (nothing
is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_code_dot_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "code-dot-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout
    assert "code dot plan ok" in r.stdout

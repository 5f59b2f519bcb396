"""The host arithmetic of vdb_index_encode_codes and vdb_index_encode (csrc/vdb_encode_plan.h: the
decision of a (vector, bit) pair against the canonical fp64 sum, the scratch, the bit / byte / word
addressing with the pad bits, the GEMM's layout and the validation causes) swept on the CPU under
AddressSanitizer + UBSan: the stand-alone program tools/encode_plan_check.cpp, built and run by
``make encode-plan-check`` in a child process (nothing is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_encode_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "encode-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout
    assert "encode plan ok" in r.stdout

"""The host arithmetic of vdb_index_search_fused (csrc/vdb_fuse_plan.h: the validation, the clamp of
a device call's offsets, the packed sort words, the sort length with the workgroup size and LDS, the
scratch layout and the fusion of one set the kernel shares) swept on the CPU under AddressSanitizer +
UBSan against naive loops: the stand-alone program tools/fuse_plan_check.cpp, built and run by ``make
fuse-plan-check`` in a child process (nothing is loaded into this one).  No GPU."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_fuse_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mlx-vector-db_amd"), "fuse-plan-check",
                        f"OBJ_DIR={tmp_path}"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "-ffp-contract=off" in r.stdout
    assert "fuse plan ok" in r.stdout

"""The host arithmetic of vdb_index_search_maxsim (csrc/vdb_maxsim_plan.h: the validation, the table
size check, the order-preserving encoding, the clamp of a device call's offsets, the deal of slots to
the rank kernel's segments, the scratch layout and the ranking of one set the kernels share) swept on
the CPU under AddressSanitizer + UBSan against naive loops: the stand-alone program
tools/maxsim_plan_check.cpp, built and run by ``make maxsim-plan-check`` in a child process (nothing
is loaded into this one).  Also: the header declares the call, the wrapper binds it and the Makefile
builds its kernels.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PKG = os.path.join(ROOT, "mlx-vector-db_amd")


def test_maxsim_plan_check_runs_clean_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", PKG, "maxsim-plan-check", f"OBJ_DIR={tmp_path}"], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "-fsanitize=address,undefined" in r.stdout and "-ffp-contract=off" in r.stdout
    assert "maxsim plan ok" in r.stdout


def test_header_declares_and_wrapper_binds_the_call():
    with open(os.path.join(ROOT, "include", "vdb.h")) as f:
        header = f.read()
    m = re.search(r"int32_t\s+vdb_index_search_maxsim\s*\(([^;]*)\)\s*;", header)
    assert m, "include/vdb.h does not declare vdb_index_search_maxsim"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 13 and args[5].endswith("n_group_slots") and args[-1] == "void* stream", args
    for stat in ("maxsim_searches", "maxsim_sets", "maxsim_bad_sets", "maxsim_skipped_rows"):
        assert f'"{stat}"' in header, stat
    with open(os.path.join(PKG, "service", "_vdb.py")) as f:
        wrapper = f.read()
    assert '"vdb_index_search_maxsim"' in wrapper.split("EXPORTED_SYMBOLS", 1)[1].split(")", 1)[0]
    sig = re.search(r'"vdb_index_search_maxsim":\s*\(c_i32,\s*\[([^\]]*)\]', wrapper)
    assert sig and len([a for a in sig.group(1).split(",") if a.strip()]) == 13
    assert "def search_maxsim(" in wrapper and "def search_maxsim_device(" in wrapper
    with open(os.path.join(PKG, "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^KERNELS\s*=.*\bvdb_maxsim\b", mk, re.M) and "vdb_maxsim_plan.h" in mk

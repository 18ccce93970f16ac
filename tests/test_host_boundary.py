"""Host-compiled check of the CSV boundary kernels (csrc/tpx_rt.hip.h):
tests/host_boundary_test.cpp replays tpx_csv_chunk_stats and tpx_csv_emit_rows
with their 64 lanes and four trips emulated, through the per-lane functions the
kernels themselves call, and compares the chunk counts and the row offsets with
a byte-serial state machine: seam and field-width cases, ranged emission, and
a fuzz over quote and newline densities from 0 to 1 with quotes on and off.
Built plain and under ASan+UBSan, as tests/test_host_cellindex.py does."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_boundary_test.cpp")


def test_boundary_kernels_match_byte_walk(tmp_path):
    exe = os.path.join(str(tmp_path), "host_boundary_test")
    subprocess.check_call(["g++", "-O2", "-Wall", "-o", exe, SRC])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert out.strip().endswith("OK"), out


def test_boundary_kernels_under_sanitizers(tmp_path):
    exe = os.path.join(str(tmp_path), "host_boundary_asan")
    subprocess.check_call(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-o", exe, SRC])
    out = subprocess.check_output([exe], timeout=600).decode()
    assert out.strip().endswith("OK"), out

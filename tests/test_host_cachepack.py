"""Host-compiled check of the per-lane pieces of the cache() pack kernels
(csrc/tpx_cache.hip.h): tests/host_cachepack_test.cpp emulates the 64 lanes of
a string-gather batch around tpx_cp_owner and compares the destination with a
row-by-row copy, canaries on both sides; tpx_cp_move is checked for every
descriptor kind. Built plain and under ASan+UBSan, as
tests/test_host_cellindex.py does."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_cachepack_test.cpp")


def test_pack_lane_logic_matches_row_copy(tmp_path):
    exe = os.path.join(str(tmp_path), "host_cachepack_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe,
                           SRC])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert out.strip().endswith("OK"), out


def test_pack_lane_logic_under_sanitizers(tmp_path):
    exe = os.path.join(str(tmp_path), "host_cachepack_asan")
    subprocess.check_call(
        ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-o", exe, SRC])
    out = subprocess.check_output([exe], timeout=600).decode()
    assert out.strip().endswith("OK"), out

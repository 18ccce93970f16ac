"""Host-compiled check of the wave-cooperative cell index (csrc/tpx_ci.hip.h):
tests/host_cellindex_test.cpp emulates the 64 lanes of the index builder and
compares every row read back through tpx_ci_row / tpx_ci_cell with
tpx_csv_next_cell — adversarial fuzz (a row may decline, an accepted row must
match exactly), structured rows (clean rows must all be accepted; odd rows
must decline or match) and list overflow with a canary behind the region.
Built plain and under ASan+UBSan, as tests/test_host_rt.py does."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_cellindex_test.cpp")


def test_cell_index_matches_byte_walk(tmp_path):
    exe = os.path.join(str(tmp_path), "host_cellindex_test")
    subprocess.check_call(["g++", "-O2", "-Wall", "-o", exe, SRC])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert out.strip().endswith("OK"), out


def test_cell_index_under_sanitizers(tmp_path):
    exe = os.path.join(str(tmp_path), "host_cellindex_asan")
    subprocess.check_call(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-o", exe, SRC])
    out = subprocess.check_output([exe], timeout=600).decode()
    assert out.strip().endswith("OK"), out

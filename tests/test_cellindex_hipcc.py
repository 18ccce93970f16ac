"""The stages that take the wave-cooperative cell index — the Zillow bench stage
and both stages of tests/cellindex_pipelines.py — compile for gfx950 through
tpx_stage_compile (compile only, no module load), and tpx_stage_main's LDS
stays within 40 960 B: 160 KiB per CU / 4 blocks, the condition for the
occupancy the fused-window kernel has without the index."""
import ctypes
import os
import re
import subprocess

import pytest

from tests import cellindex_pipelines as CP
from tuplex_amd import codegen

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "tuplex_amd", "libtpx_gpu.so")
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
LDS_LIMIT = 40960


def _compile_only(src, desc):
    assert os.path.exists(LIB), "libtpx_gpu.so not built"
    lib = ctypes.CDLL(LIB)
    lib.tpx_stage_compile.restype = ctypes.c_void_p
    lib.tpx_stage_compile.argtypes = [ctypes.c_char_p] * 3 + [ctypes.c_int64]
    lib.tpx_last_error.restype = ctypes.c_char_p
    lib.tpx_stage_free.argtypes = [ctypes.c_void_p]
    cache = os.path.join(ROOT, "tuplex_amd", ".kernel_cache")
    os.makedirs(cache, exist_ok=True)
    h = lib.tpx_stage_compile(src.encode(), desc.encode(), cache.encode(), 1)
    assert h, "hipRTC compile failed:\n%s" % lib.tpx_last_error().decode()[:4000]
    lib.tpx_stage_free(h)
    return cache


def _main_lds(cache, src):
    """.group_segment_fixed_size of tpx_stage_main in the cached code object
    of `src` (tpx_stage_compile names it by FNV-1a hash and byte length)."""
    raw = src.encode()
    h = 1469598103934665603
    for c in raw:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    path = os.path.join(cache, "tpx_%016x_%d_g2.hsaco" % (h, len(raw)))
    assert os.path.exists(path), "no cached code object at %s" % path
    notes = subprocess.check_output([READELF, "--notes", path]).decode()
    # one metadata map per kernel, keys in alphabetical order
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+)\s*\n"
                         r"(?:(?!\.group_segment_fixed_size).*\n)*?"
                         r"\s*\.name:\s*(\S+)", notes):
        if m.group(2) == "tpx_stage_main":
            return int(m.group(1))
    raise AssertionError("tpx_stage_main not found in %s" % path)


def _bench_stage():
    import bench
    old = os.environ.get("TPX_CELL_INDEX")
    os.environ["TPX_CELL_INDEX"] = "1"
    try:
        return bench.build_stage()
    finally:
        if old is None:
            os.environ.pop("TPX_CELL_INDEX", None)
        else:
            os.environ["TPX_CELL_INDEX"] = old


def _stages():
    yield ("zillow",) + tuple(_bench_stage())
    for sink in ("csv", "mem"):
        _sp, src, desc = CP.generate(sink, "index")
        yield ("cellindex-" + sink, src, desc)


@pytest.mark.parametrize("which", ["zillow", "cellindex-csv", "cellindex-mem"])
def test_index_stage_compiles_within_the_lds_limit(which):
    name, src, desc = next(s for s in _stages() if s[0] == which)
    assert "tpx_ci_stage(" in src and "static_assert(64 * " in src
    assert 1 <= codegen.StageCodegen.CI_MAX_COLS == 14
    cache = _compile_only(src, desc)
    lds = _main_lds(cache, src)
    print("%s: tpx_stage_main LDS %d B" % (name, lds))
    assert lds <= LDS_LIMIT, (name, lds)

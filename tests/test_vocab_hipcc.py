"""One stage with all four vocabulary additions — truthiness on Option[i64] /
Option[str] / f64, a two-field format, capwords and a four-string `in` — over a
6-column row, compiled for gfx950 through tpx_stage_compile (compile only, no
module load), with the csv source and sink and with the mem source and sink."""
import ctypes
import os

import pytest

from tests import vocab_pipelines as V
from tuplex_amd import codegen, plan

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "tuplex_amd", "libtpx_gpu.so")


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


def _stage():
    types = V.all_four_types()
    assert len(types) == 6
    sp = plan.build_stage(types, V.ALL_FOUR_COLS, [("map", V.all_four)])
    assert sp.compilable, sp.why_not_compilable
    ops = {n["op"] for n in _walk(sp.ops[0].tir)}
    assert {"truthy", "format", "capwords", "streq"} <= ops
    return sp


def _walk(node):
    from tuplex_amd.udf import tir
    return list(tir.walk(node))


@pytest.mark.parametrize("source,sink", [("mem", "mem"), ("csv", "csv")])
def test_all_four_stage_compiles_for_gfx950(source, sink):
    sp = _stage()
    kw = {}
    if source == "csv":
        kw["csv_info"] = {"null_values": [""], "delimiter": ","}
    src, desc = codegen.generate_stage(sp, source=source, sink=sink, **kw)
    assert "tpx_format(" in src and "tpx_capwords(" in src
    _compile_only(src, desc)

"""CPU checks of the device cache() pack: the sequential model
(tests/cache_models.py) pinned against pyarrow / numpy building the same
columns from the kept python rows; the runtime header with the pack kernels
cross-compiles for gfx950 under the harness's hipRTC options; libtpx_gpu.so
exports the new entry points and they fail cleanly without a table or a loaded
stage; and the eligibility predicate sends every excluded case to the host
cache with its reason, without opening the GPU."""
import ctypes
import os
import random

import numpy as np
import pytest

import tuplex_amd
from tests import cache_models as CM
from tuplex_amd import engine
from tuplex_amd import ttypes as T

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), "tuplex_amd", "libtpx_gpu.so")

KINDS = [("bool", False), ("i64", True), ("str", False), ("str", True),
         ("f64", False)]


def _rows(n, seed):
    rng = random.Random(seed)
    lens = [0, 1, 7, 8, 9, 63, 64, 65]
    rows = []
    for i in range(n):
        s = "".join(chr(33 + (i * 7 + j) % 90) for j in range(lens[i % 8]))
        if i == 5:
            s = "x" * 700
        rows.append((rng.random() < 0.5,
                     None if i % 5 == 2 else rng.randrange(-2 ** 62, 2 ** 62),
                     s,
                     None if i % 3 == 1 else s[::-1],
                     rng.uniform(-1e9, 1e9)))
    return rows


def _reference(rows, keep, row0):
    """The same columns from the kept rows, by pyarrow and numpy."""
    pa = pytest.importorskip("pyarrow")
    kept = [r for r, k in zip(rows, keep) if k]
    out = []
    for k, (kind, opt) in enumerate(KINDS):
        vals = [r[k] for r in kept]
        d = {}
        if opt:
            d["mask"] = np.array([v is None for v in vals],
                                 dtype=np.uint8).tobytes()
        if kind == "str":
            arr = pa.array(["" if v is None else v for v in vals],
                           type=pa.large_string())
            bufs = arr.buffers()
            d["offsets"] = np.frombuffer(
                bufs[1], dtype=np.int64, count=len(vals) + 1).tolist()
            d["data"] = bufs[2].to_pybytes()[:d["offsets"][-1]] \
                if bufs[2] is not None else b""
        elif kind == "bool":
            d["values"] = np.array(vals, dtype=np.uint8).tobytes()
        elif kind == "f64":
            d["values"] = np.array(vals, dtype=np.float64).tobytes()
        else:
            d["values"] = [v for v in vals]  # nulls: any bits, compared below
        out.append(d)
    keys = [row0 + i for i, k in enumerate(keep) if k]
    return keys, out


@pytest.mark.parametrize("n", [1, 64, 65, 200])
@pytest.mark.parametrize("pattern", ["all", "none", "alt", "first", "last"])
def test_model_matches_arrow_and_numpy(n, pattern):
    rows = _rows(n, seed=n)
    keep = {"all": [1] * n, "none": [0] * n,
            "alt": [i & 1 for i in range(n)],
            "first": [1] + [0] * (n - 1),
            "last": [0] * (n - 1) + [1]}[pattern]
    cols, regions = CM.slots_from_rows(rows, KINDS)
    keys, packed = CM.pack(keep, 1000, cols, CM.Memory(regions))
    want_keys, want = _reference(rows, keep, 1000)
    assert keys == want_keys
    for (kind, opt), got, ref in zip(KINDS, packed, want):
        if opt:
            assert got["mask"] == ref["mask"]
        if kind == "str":
            assert got["offsets"] == ref["offsets"]
            assert got["data"] == ref["data"]
        elif kind == "i64":
            vals = np.frombuffer(got["values"], dtype=np.int64).tolist()
            assert len(vals) == len(ref["values"])
            for g, r in zip(vals, ref["values"]):
                assert r is None or g == r
        else:
            assert got["values"] == ref["values"]


def test_runtime_header_with_pack_kernels_cross_compiles():
    from tests import hipkern
    src = hipkern.source()
    assert 'extern "C" __global__ void tpx_cache_pack_fixed(' in src
    assert 'extern "C" __global__ void tpx_cache_gather_str(' in src
    code = hipkern.compile_code()
    assert b"tpx_cache_pack_fixed" in code and b"tpx_cache_gather_str" in code


def _lib():
    assert os.path.exists(LIB), "libtpx_gpu.so not built"
    lib = ctypes.CDLL(LIB)
    lib.tpx_version.restype = ctypes.c_int64
    for name in ("tpx_table_rows", "tpx_table_bytes", "tpx_table_slots",
                 "tpx_table_download", "tpx_xfer_stats",
                 "tpx_stage_cache_csv", "tpx_stage_cache_csv_dev"):
        getattr(lib, name).restype = ctypes.c_int64
    lib.tpx_table_free.restype = None
    lib.tpx_table_rows.argtypes = [ctypes.c_void_p]
    lib.tpx_table_bytes.argtypes = [ctypes.c_void_p]
    lib.tpx_table_free.argtypes = [ctypes.c_void_p]
    lib.tpx_table_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_int64]
    lib.tpx_table_download.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int64]
    lib.tpx_xfer_stats.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    return lib


def test_library_exports_table_and_xfer_symbols():
    lib = _lib()
    assert lib.tpx_version() >> 16 == 1 and lib.tpx_version() & 0xFFFF >= 1
    h, d = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.tpx_xfer_stats(ctypes.byref(h), ctypes.byref(d)) == 0
    assert h.value >= 0 and d.value >= 0
    assert lib.tpx_xfer_stats(None, None) == 0


def test_table_calls_without_a_table_fail_cleanly():
    lib = _lib()
    assert lib.tpx_table_rows(None) == -1
    assert lib.tpx_table_bytes(None) == -1
    slots = (ctypes.c_void_p * 6)()
    assert lib.tpx_table_slots(None, slots, None, 6) == -1
    assert lib.tpx_table_download(None, slots, 6) == -1
    lib.tpx_table_free(None)


def test_cache_execute_on_an_unloaded_stage_is_an_error():
    """Compile only (no module load — as on a machine with no GPU): the
    cache execute reports an error and hands out no table."""
    from tuplex_amd import codegen, plan
    sp = plan.build_stage([T.I64, T.STR], ["a", "s"], [("filter", _a_gt_1)])
    assert sp.compilable, sp.why_not_compilable
    src, desc = codegen.generate_stage(
        sp, source="csv", sink="mem",
        csv_info={"null_values": [""], "delimiter": ",", "text_mode": False})
    glib = engine.GpuLib.get()
    stage = glib.compile_stage(src, desc, compile_only=True)
    res = engine.TpxResult()
    tab = ctypes.c_void_p(1234)
    data = (ctypes.c_uint8 * 8)(*b"1,a\n2,b\n")
    rc = glib.lib.tpx_stage_cache_csv(stage, data, 8, 0, ctypes.byref(res),
                                      ctypes.byref(tab))
    assert rc == -1 and not tab.value
    assert "not loaded" in glib.err()
    tab = ctypes.c_void_p(1234)
    rc = glib.lib.tpx_stage_cache_csv_dev(stage, 0, 8, 0, ctypes.byref(res),
                                          ctypes.byref(tab))
    assert rc == -1 and not tab.value


def _a_gt_1(x):
    return x["a"] > 1


def _poison_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the eligibility predicate opened the GPU library")
    monkeypatch.setattr(engine.GpuLib, "get", classmethod(boom))


def test_eligibility_reasons(monkeypatch, tmp_path):
    _poison_gpu(monkeypatch)
    p = os.path.join(str(tmp_path), "in.csv")
    with open(p, "w") as f:
        f.write("a,b\n1,2\n")
    ctx = tuplex_amd.Context()
    opts = ctx.options_obj
    csv = ctx.csv(p)
    flt = ("filter", lambda x: x["a"] > 0)
    assert engine.cache_eligibility(opts, csv._source, [flt]) == \
        ("device", None)
    assert engine.cache_eligibility(
        opts, csv._source, [flt], [T.I64, T.opt(T.STR), T.BOOL, T.F64]) == \
        ("device", None)
    assert engine.cache_eligibility(
        opts, ctx.text(p)._source, [flt]) == ("device", None)
    # parallelize source
    assert engine.cache_eligibility(
        opts, ctx.parallelize([1, 2])._source, [flt]) == \
        ("host", "parallelize source")
    # trailing aggregate / unique
    agg = ("aggregate", lambda a, b: a + b, lambda a, x: a + x["a"], 0)
    assert engine.cache_eligibility(opts, csv._source, [flt, agg]) == \
        ("host", "trailing aggregate or unique")
    assert engine.cache_eligibility(opts, csv._source, [("unique",)]) == \
        ("host", "trailing aggregate or unique")
    # nested output type
    assert engine.cache_eligibility(
        opts, csv._source, [flt], [T.I64, T.tup([T.I64, T.STR])]) == \
        ("host", "nested output type")
    # duplicate-key join
    join = ("join", [(1, "x"), (1, "y")], ["k", "v"], "a", "k", "inner",
            "", "", "", "")
    assert engine.cache_eligibility(opts, csv._source, [join]) == \
        ("host", "duplicate-key join")
    # in-process device fan-out
    fan = tuplex_amd.Context({"tuplex.gpu.devices": 2}).options_obj
    assert engine.cache_eligibility(fan, csv._source, [flt]) == \
        ("host", "multi-device fan-out")
    # option off
    off = tuplex_amd.Context({"tuplex.gpu.deviceCache": False}).options_obj
    assert engine.cache_eligibility(off, csv._source, [flt]) == \
        ("host", "tuplex.gpu.deviceCache is off")


def test_host_cache_reports_where_and_why():
    """cache() of a parallelize source (interpreter stage, CPU-runnable)
    keeps today's host cache and says so."""
    ctx = tuplex_amd.Context()
    ds = ctx.parallelize([3, 1, 2]).map(lambda x: sorted([x, x])[0]).cache()
    m = ds._last_outcome.metrics
    assert m["cache"] == "host" and m["cache_reason"] == "parallelize source"
    assert ds.collect() == [3, 1, 2]


def test_decode_table_roundtrip():
    """The lazy host copy decodes the slot layout the pack writes."""
    rows = _rows(70, seed=3)
    keep = [1] * 70
    cols, regions = CM.slots_from_rows(rows, KINDS)
    _keys, packed = CM.pack(keep, 0, cols, CM.Memory(regions))
    bufs = []
    for (kind, opt), d in zip(KINDS, packed):
        if kind == "str":
            bufs.append(np.array(d["offsets"], dtype=np.int64).view(np.uint8))
            bufs.append(np.frombuffer(d["data"], dtype=np.uint8))
        else:
            bufs.append(np.frombuffer(d["values"], dtype=np.uint8))
            bufs.append(None)
        bufs.append(np.frombuffer(d["mask"], dtype=np.uint8) if opt else None)
    types = [T.opt(b) if o else b for (b, o) in KINDS]
    assert engine.decode_table(bufs, types, 70) == rows

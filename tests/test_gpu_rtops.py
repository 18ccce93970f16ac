"""Device slice of the scalar-runtime differential test. The host harness
(test_host_rtops.py) proves the C of csrc/tpx_rt.hip.h; the device build can
still differ in fmod/floor, __int128 shifts, unaligned 8-byte loads from
LDS-staged rows and -ffp-contract. A handful of small pipelines through the
public API carry each helper family's hardest vectors (tests/rtops_cases.py)
onto the GPU; results and exception counts must equal the oracle's, floats by
bit pattern (any NaN equals any NaN)."""
import math
import os
import time

import pytest

import tuplex_amd
from oracle import pyoracle
from oracle import pyoracle_csv
from tests import rtops_cases as RC
from tests import rtops_pipelines as P

pytestmark = pytest.mark.gpu


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return RC.same_float(a, b)
    if isinstance(a, tuple) and isinstance(b, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def _assert_rows(got, want):
    assert len(got) == len(want), (len(got), len(want))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want))
           if not _same(g, w)]
    assert not bad, "%d rows differ, first: %r" % (len(bad), bad[:5])


def _run_mem(name):
    _n, rows, cols, fn = [m for m in P.MEM if m[0] == name][0]
    data = rows()
    ctx = tuplex_amd.Context()
    t = time.time()
    ds = ctx.parallelize(data, columns=cols).map(fn)
    got = ds.collect()
    print("%s: %d rows, %.2fs" % (name, len(data), time.time() - t))
    assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason
    ref = pyoracle.run_pipeline(data, [("map", fn)], columns=cols)
    _assert_rows(got, ref["output"])
    assert ds.exception_counts == ref["exception_counts"]
    return data, got


def test_float_floordiv_mod():
    data = P.fdiv_rows()
    # the pairs where floor(a/b) is NOT a // b must be on board
    assert P.n_divergent(data) >= 100
    assert sum(1 for a, b in data
               if b != 0.0 and math.isfinite(a) and math.isfinite(b)
               and RC.dbits(RC.old_mod(a, b)) != RC.dbits(a % b)) >= 100
    _run_mem("rt_fdiv")


def test_float_parse():
    data, got = _run_mem("rt_float")
    strings = set(s for s, _ in data)
    for must in ("1e4294967297", "-.", "1e-", " 1 ", "InFiNiTy", "infi",
                 "123456789012345678e308"):
        assert must in strings, must
    assert len(got) > 2000


def test_int_parse():
    data, _ = _run_mem("rt_int")
    strings = set(s for s, _ in data)
    for must in ("-", "99999999999999999999", "9223372036854775808",
                 "-9223372036854775809", "12x", ""):
        assert must in strings, must


def test_parse_rejects_replay_in_cpython():
    """Strings the compiled-path parsers reject but CPython accepts ('+5',
    '1_0', '-inf'): the device raises, the row is replayed by the
    interpreter, and CPython's value comes out."""
    ctx = tuplex_amd.Context()
    for strings, fn, py in ((P.float_strings()[1], P.u_float, float),
                            (P.int_strings()[1], P.u_int, int)):
        assert strings
        data = [(s, k) for k, s in enumerate(strings)]
        ds = ctx.parallelize(data, columns=["s", "k"]).map(fn)
        got = ds.collect()
        assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason
        _assert_rows(got, [(py(s), k) for s, k in data])
        assert ds.exception_counts == {}


def test_int_format_and_divmod():
    data, got = _run_mem("rt_ifmt")
    assert (RC.I64_MIN, -1) in data  # 2^63: the row is replayed as a big int
    assert any(g[2] == 1 << 63 for g in got)


def test_int_of_float():
    data, _ = _run_mem("rt_int_f64")
    assert any(v == 2.0 ** 63 for v, _ in data)
    assert any(v == -2.0 ** 63 for v, _ in data)


def test_string_ops():
    data, _ = _run_mem("rt_str")
    assert {len(s) for s, _ in data} >= set(range(73))


def test_split_index():
    _run_mem("rt_split")


def test_center_and_repeat():
    data, _ = _run_mem("rt_center")
    assert max(r for _, _, r in data) == 64  # no larger repeat on the device


def test_string_ops_csv_source(tmp_path):
    """The string family once more through the csv source: the cells sit at
    arbitrary offsets of the LDS-staged row."""
    data = P.str_csv_bytes()
    p = os.path.join(str(tmp_path), "s.csv")
    with open(p, "wb") as f:
        f.write(data)
    ctx = tuplex_amd.Context()
    t = time.time()
    ds = ctx.csv(p).map(P.u_str)
    got = ds.collect()
    print("rt_str_csv: %.2fs" % (time.time() - t))
    assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason
    ref = pyoracle_csv.run_csv_pipeline(data, [("map", P.u_str)])
    assert len(ref["output"]) > 1900
    _assert_rows(got, ref["output"])
    assert ds.exception_counts == ref["exception_counts"]


def test_f64_tocsv(tmp_path):
    """%f on the device: sixth-decimal ties, -0.0 and values either side of
    the accept limit, byte-for-byte the oracle's format_csv_row."""
    data = P.f64_csv_bytes()
    p = os.path.join(str(tmp_path), "f.csv")
    outp = os.path.join(str(tmp_path), "out.csv")
    with open(p, "wb") as f:
        f.write(data)
    ref = pyoracle_csv.run_csv_pipeline(data, [("map", P.u_f64)], sink="csv")
    vals = [v for _, v in ref["output"]]
    # the cells parse to what they are meant to be
    ties = [v for v in vals if math.isfinite(v) and abs(v) < 1e6
            and (abs(v) * 128) % 2 == 1]
    assert len(ties) >= 700
    fits = pyoracle_csv._f64_fits_device
    assert any(fits(v) and abs(v) > 9.2e12 for v in vals)
    assert any(not fits(v) and math.isfinite(v) and abs(v) < 9.3e12
               for v in vals)
    assert any(v == 0.0 and math.copysign(1.0, v) < 0 for v in vals)
    want = b"".join(pyoracle_csv.format_csv_row(list(r))
                    for r in ref["output"])
    assert ref["csv_text"].endswith(want)
    ctx = tuplex_amd.Context()
    t = time.time()
    ds = ctx.csv(p).map(P.u_f64)
    ds.tocsv(outp)
    print("rt_f64_csv: %.2fs" % (time.time() - t))
    assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason
    got = open(outp, "rb").read()
    assert got == ref["csv_text"]
    assert ds.exception_counts == ref["exception_counts"]

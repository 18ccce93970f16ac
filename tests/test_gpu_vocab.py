"""Device tests of the UDF-vocabulary additions (truthiness, constant `in`,
str.format / multi-directive %, string.capwords): small pipelines through the
public API; rows and exception counts must equal the oracle's, every run must
have stayed on the GPU. Row counts are 64k +- 1, so the last wave is partial."""
import math
import os
import time

import pytest

import tuplex_amd
from oracle import pyoracle
from oracle import pyoracle_csv
from tests import vocab_pipelines as V
from tests.pipelines import apply_ops, csv_used_cols

pytestmark = pytest.mark.gpu


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return (math.isnan(a) and math.isnan(b)) or (
            a == b and math.copysign(1.0, a) == math.copysign(1.0, b))
    if isinstance(a, tuple) and isinstance(b, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def _assert_rows(got, want):
    assert len(got) == len(want), (len(got), len(want))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want))
           if not _same(g, w)]
    assert not bad, "%d rows differ, first: %r" % (len(bad), bad[:5])


def _run_mem(name):
    _n, rows, cols, fn = [m for m in V.MEM if m[0] == name][0]
    data = rows()
    assert len(data) % 64 in (1, 63)
    ctx = tuplex_amd.Context()
    t = time.time()
    ds = ctx.parallelize(data, columns=cols).map(fn)
    got = ds.collect()
    print("%s: %d rows, %.2fs" % (name, len(data), time.time() - t))
    assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason
    ref = pyoracle.run_pipeline(data, [("map", fn)], columns=cols)
    _assert_rows(got, ref["output"])
    assert ds.exception_counts == ref["exception_counts"]
    return data, got, ds.exception_counts


# ---- truthiness ---------------------------------------------------------------------

def test_truthy_option_f64():
    data, got, excs = _run_mem("t_int_or_zero")
    # nan is true: int(nan) raises in CPython and on the device alike
    assert excs == {"ValueError": sum(1 for v in data
                                      if v is not None and math.isnan(v))}
    assert 0 in got and 1 in got


def test_truthy_guards_the_unwrap():
    """10 // x if x else -1: x == 0 and x is None both give -1, nothing
    raised — the unwrap in the branch not taken stays silent."""
    data, got, excs = _run_mem("t_guarded_div")
    assert excs == {}
    assert len(got) == len(data)
    for x, g in zip(data, got):
        if x is None or x == 0:
            assert g == -1


def test_truthy_option_str():
    data, got, excs = _run_mem("t_str_upper")
    assert excs == {}
    assert got.count("<empty>") == sum(1 for s in data if not s)


def test_truthy_f64_signed_zero_and_nan():
    data, got, excs = _run_mem("t_f64_flag")
    assert excs == {}
    assert sum(got) == sum(1 for v in data if v != 0.0)  # nan counts, -0.0 not


def test_not_returns_bool():
    _data, got, excs = _run_mem("t_not")
    assert excs == {} and set(got) == {True, False}


def test_and_or_not_over_mixed_types():
    _data, got, excs = _run_mem("t_bool_ops")
    assert excs == {} and set(got) == {"a only", "s or f", "none"}


# ---- format / % ---------------------------------------------------------------------

def test_format_ints():
    data, got, excs = _run_mem("f_ints")
    assert excs == {}
    ints = {i for i, _ in data}
    assert {0, V.I64_MAX, V.I64_MIN, 10 ** 18, -(10 ** 18 - 1)} <= ints


def test_format_strings_roll_the_heap_chunk():
    """Every row's four outputs total more than one 256-byte chunk of the
    thread's string heap; the 300-byte value takes the unchunked path."""
    data, got, excs = _run_mem("f_strs")
    assert excs == {}
    assert all(sum(len(c) for c in row) > 256 for row in got)
    assert any(len(s) == 300 for s, _ in data)


def test_format_non_ascii_with_width_replays():
    data, got, excs = _run_mem("f_strs_non_ascii")
    assert excs == {}
    assert any(not s.isascii() for s, _ in data)


def test_format_non_ascii_without_width_copies_bytes():
    _run_mem("f_plain_non_ascii")


def test_format_null_argument_replays_to_cpythons_text():
    """A null argument raises TYPEERROR on the device; the replay gives what
    CPython gives: the text None for an empty spec, a TypeError for '{:03}'."""
    data, got, excs = _run_mem("f_opt")
    assert excs == {}
    assert got.count("None/None") == data.count(None)
    data, got, excs = _run_mem("f_opt_spec")
    assert excs == {"TypeError": data.count(None)}
    assert len(got) == len(data) - data.count(None)


# ---- capwords / membership ----------------------------------------------------------

def test_capwords():
    data, got, excs = _run_mem("c_cap")
    assert excs == {}  # the non-ASCII rows come back from the replay
    assert any(not s.isascii() for s, _ in data)
    assert max(len(s) for s, _ in data) == 3000


def test_membership_str_and_int_with_null_subject():
    data, got, excs = _run_mem("m_in")
    assert excs == {}
    for (s, n), g in zip(data, got):
        if s is None:
            assert g[0] is False and g[1] is True
        if n is None:
            assert g[2] is False and g[3] is True


# ---- flights-shaped csv -------------------------------------------------------------

def _flights_file(tmp_path):
    data = V.make_flights_vocab_csv(V.FLIGHTS_ROWS)
    p = os.path.join(str(tmp_path), "flights_vocab.csv")
    with open(p, "wb") as f:
        f.write(data)
    return data, p


def test_flights_shapes_csv_collect(tmp_path):
    data, p = _flights_file(tmp_path)
    ops = V.flights_vocab_ops()
    ctx = tuplex_amd.Context()
    t = time.time()
    ds = apply_ops(ctx.csv(p), ops)
    got = ds.collect()
    print("flights_vocab collect: %.2fs" % (time.time() - t))
    assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason
    ref = pyoracle_csv.run_csv_pipeline(data, ops,
                                        used_cols=csv_used_cols(data, ops))
    assert len(ref["output"]) > 1500
    assert sum(ref["exception_counts"].values()) > 5   # the malformed rows
    _assert_rows(got, ref["output"])
    assert ds.exception_counts == ref["exception_counts"]
    assert {r[3] for r in got} >= {"diverted", "None", "carrier", "other"}


def test_flights_shapes_tocsv(tmp_path):
    data, p = _flights_file(tmp_path)
    ops = V.flights_vocab_ops()
    outp = os.path.join(str(tmp_path), "out.csv")
    ref = pyoracle_csv.run_csv_pipeline(data, ops, sink="csv",
                                        used_cols=csv_used_cols(data, ops))
    # capwords of a cell with a comma / a quote, and the ", " literal of the
    # label: all of them must come out quoted
    assert b'"Washington, Dc"' in ref["csv_text"]
    assert b'"The ""windy"" City"' in ref["csv_text"]
    assert b'"jetBlue airways, ' in ref["csv_text"]
    ctx = tuplex_amd.Context()
    t = time.time()
    ds = apply_ops(ctx.csv(p), ops)
    ds.tocsv(outp)
    print("flights_vocab tocsv: %.2fs" % (time.time() - t))
    assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason
    with open(outp, "rb") as f:
        got = f.read()
    assert got == ref["csv_text"]
    assert ds.exception_counts == ref["exception_counts"]

"""Front-end checks of the UDF-vocabulary additions: truthiness in condition
positions, constant-sequence membership, str.format / multi-directive %, and
string.capwords — what compiles (and to which type), what stays uncompiled,
which stages carry tpx_fmt.hip.h, column lineage, and that the oracle agrees
with plain CPython on every UDF of tests/vocab_pipelines.py over its rows."""
import math
import string

import pytest

from oracle import pyoracle
from tests import vocab_pipelines as V
from tuplex_amd import codegen, plan
from tuplex_amd import ttypes as T
from tuplex_amd.udf import tir
from tuplex_amd.udf.compile import UDFCompileError, compile_udf

O = T.opt
FMT_MARK = "tpx_format(TpxHeap& h"     # text of tpx_fmt.hip.h itself
CAP_MARK = "tpx_capwords(TpxHeap& h"


def _ops(node):
    return [n["op"] for n in tir.walk(node)]


# ---- the shapes that used to be rejected -------------------------------------------

def s_chain(row):
    if row["diverted"]:
        return "diverted"
    else:
        if row["ccode"]:
            return "cancelled " + row["ccode"]
        else:
            return "None"


def s_defunct(row):
    if row["d"]:
        return int(row["y"]) < int(row["d"])
    return True


def s_elif(x):
    if not x:
        return None
    elif x in ("10001", "10002"):
        return "nyc"
    return x


SHAPES = [
    ("int_if_optf64", lambda x: int(x) if x else 0, [O(T.F64)], None, T.I64,
     "truthy"),
    ("chain", s_chain, [T.F64, O(T.STR)], ["diverted", "ccode"], T.STR,
     "truthy"),
    ("defunct", s_defunct, [O(T.I64), T.I64], ["d", "y"], T.BOOL, "truthy"),
    ("format_time", lambda x: "{:02}:{:02}".format(int(x / 100), x % 100),
     [T.I64], None, T.STR, "format"),
    ("format_opt", lambda x: "{:02}:{:02}".format(x // 100, x % 100),
     [O(T.I64)], None, T.STR, "format"),
    ("percent_two", lambda a, b: "%02d:%02d" % (a, b), [T.I64, T.I64], None,
     T.STR, "format"),
    ("percent_width", lambda x: "%5d" % x, [T.I64], None, T.STR, "format"),
    ("capwords", lambda x: string.capwords(x) if x else None, [O(T.STR)], None,
     O(T.STR), "capwords"),
    ("in_list", lambda x: x in ["AIR", "AIR REG"], [T.STR], None, T.BOOL,
     "streq"),
    ("in_tuple_opt", lambda x: x in ("AIR", "AIR REG"), [O(T.STR)], None,
     T.BOOL, "opteq"),
    ("not_in_ints", lambda x: x not in [1, 2, 3], [T.I64], None, T.BOOL, "eq"),
    ("not_opt", lambda x: not x, [O(T.I64)], None, T.BOOL, "truthy"),
    ("guarded_div", lambda x: 10 // x if x else -1, [O(T.I64)], None, T.I64,
     "truthy"),
    ("null_typed", lambda x: 1 if x else 0, [T.NULL], None, T.I64, "const"),
    ("elif_not", s_elif, [O(T.STR)], None, O(T.STR), "truthy"),
    ("and_or", lambda a, b: 1 if a and not b or b == "x" else 0,
     [O(T.I64), T.STR], None, T.I64, "truthy"),
    ("format_bool", lambda x: "{} {}".format(x, x > 1), [T.I64], None, T.STR,
     "format"),
]


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_compiles(case):
    _name, fn, types, cols, want_t, want_op = case
    node = compile_udf(fn, types, cols)
    assert node["t"] == want_t
    assert want_op in _ops(node)


def test_format_over_option_row_gives_option_str():
    node = compile_udf(
        lambda x: "{:02}:{:02}".format(x // 100, x % 100) if x else None,
        [O(T.I64)], None)
    assert node["t"] == O(T.STR)
    assert "format" in _ops(node) and "unwrap" in _ops(node)


def test_null_option_is_false_without_unwrap():
    node = compile_udf(lambda x: 1 if x else 0, [O(T.STR)], None)
    assert "truthy" in _ops(node) and "unwrap" not in _ops(node)


def test_membership_is_an_or_chain_of_existing_nodes():
    node = compile_udf(lambda x: x in ["a", "b", "c", "d"], [T.STR], None)
    assert sorted(set(_ops(node))) == ["const", "input", "or", "streq"]
    assert _ops(node).count("streq") == 4


def test_format_descriptors_are_in_v():
    a = compile_udf(lambda x: "{:3}".format(x), [T.I64], None)
    b = compile_udf(lambda x: "{:4}".format(x), [T.I64], None)
    assert a["op"] == b["op"] == "format" and a["v"] != b["v"]
    spa = plan.build_stage([T.I64], None, [("map", lambda x: "{:3}".format(x))])
    spb = plan.build_stage([T.I64], None, [("map", lambda x: "{:4}".format(x))])
    assert spa.signature() != spb.signature()


# ---- what stays uncompiled ----------------------------------------------------------

GLOBAL_LIST = ["a", "b"]

REJECTED = [
    ("value_or", lambda a, b: a or b, [T.I64, T.I64]),
    ("value_and", lambda a, b: a and b, [T.STR, T.STR]),
    ("in_empty", lambda x: x in [], [T.STR]),
    ("in_mixed", lambda x: x in ["a", 1], [T.STR]),
    ("in_nonconst", lambda x, y: x in ["a", y], [T.STR, T.STR]),
    ("in_none", lambda x: x in ["a", None], [T.STR]),
    ("in_33", lambda x: x in [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14,
                              15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26,
                              27, 28, 29, 30, 31, 32], [T.I64]),
    ("in_name", lambda x: x in GLOBAL_LIST, [T.STR]),
    ("fmt_f64", lambda x: "{}".format(x), [T.F64]),
    ("fmt_conv_r", lambda x: "{!r}".format(x), [T.STR]),
    ("fmt_conv_s", lambda x: "{!s}".format(x), [T.I64]),
    ("fmt_keyword", lambda x: "{v}".format(v=x), [T.I64]),
    ("fmt_attr", lambda x: "{0.real}".format(x), [T.I64]),
    ("fmt_nested", lambda x: "{:{}}".format(x, 5), [T.I64]),
    ("fmt_comma", lambda x: "{:,}".format(x), [T.I64]),
    ("fmt_underscore", lambda x: "{:_}".format(x), [T.I64]),
    ("fmt_sign", lambda x: "{:+}".format(x), [T.I64]),
    ("fmt_hash", lambda x: "{:#x}".format(x), [T.I64]),
    ("fmt_center", lambda x: "{:^9}".format(x), [T.STR]),
    ("fmt_eq_align", lambda x: "{:=9}".format(x), [T.I64]),
    ("fmt_str_zero_width", lambda x: "{:05}".format(x), [T.STR]),
    ("fmt_str_zero_right", lambda x: "{:>05}".format(x), [T.STR]),
    ("fmt_str_zero_left", lambda x: "{:<05}".format(x), [T.STR]),
    ("fmt_str_zero_s", lambda x: "{:05s}".format(x), [T.STR]),
    ("fmt_surplus_arg", lambda x: "{}".format(x, x), [T.I64]),
    ("pct_zero_s", lambda x: "%05s|%d" % (x, 1), [T.STR]),
    ("pct_minus_zero_s", lambda x: "%-05s|" % x, [T.STR]),
    ("pct_bool_width_s", lambda x: "%5s|" % (x > 1), [T.I64]),
    ("fmt_mixed_numbering", lambda a, b: "{}{1}".format(a, b), [T.I64, T.I64]),
    ("fmt_width_256", lambda x: "{:256}".format(x), [T.I64]),
    ("fmt_bool_spec", lambda x: "{:5}".format(x > 1), [T.I64]),
    ("fmt_int_s", lambda x: "{:s}".format(x), [T.I64]),
    ("fmt_str_d", lambda x: "{:d}".format(x), [T.STR]),
    ("fmt_missing_arg", lambda x: "{}{}".format(x), [T.I64]),
    ("fmt_var_template", lambda x, y: x.format(y), [T.STR, T.I64]),
    ("pct_float", lambda x: "%5.2f|%d" % (x, 1), [T.F64]),
    ("pct_hex", lambda x: "%x %d" % (x, x), [T.I64]),
    ("pct_d_of_str", lambda x: "%d %d" % (x, 1), [T.STR]),
    ("pct_too_few", lambda x: "%d %d" % x, [T.I64]),
    ("pct_too_many", lambda x: "%d %d" % (x, x, x), [T.I64]),
    ("pct_width_256", lambda x: "%256d" % x, [T.I64]),
    ("capwords_sep", lambda x: string.capwords(x, "-"), [T.STR]),
    ("capwords_int", lambda x: string.capwords(x), [T.I64]),
    ("string_other", lambda x: string.ascii_lowercase, [T.STR]),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_rejected_form_raises(case):
    _name, fn, types = case
    with pytest.raises(UDFCompileError):
        compile_udf(fn, types, None)


def test_shadowed_string_module_is_not_the_module():
    def f(string):
        return string.capwords(string)
    with pytest.raises(UDFCompileError):
        compile_udf(f, [T.STR], None)


# ---- today's single-directive nodes stay -------------------------------------------

def test_single_directive_percent_keeps_its_nodes():
    n = compile_udf(lambda x: "%05d" % x, [T.I64], None)
    assert n["op"] == "fmt_int" and n["w"] == 5
    n = compile_udf(lambda x: "%d" % x, [T.I64], None)
    assert n["op"] == "fmt_int" and n["w"] == 0
    n = compile_udf(lambda x: "%s" % x, [T.I64], None)
    assert n["op"] == "to_str"


# ---- the header travels only with stages that need it ------------------------------

def _source(fn, types, cols=None, **kw):
    sp = plan.build_stage(types, cols, [("map", fn)])
    assert sp.compilable, sp.why_not_compilable
    return codegen.generate_stage(sp, **kw)[0]


def old_pct(x):
    return "%05d" % x


def old_upper(x):
    return x.upper() + "!"


def new_truthy(x):
    return 1 if x else 0


def new_member(x):
    return x in ["a", "b"]


def test_stage_without_new_ops_has_no_fmt_header():
    for fn, types in ((old_pct, [T.I64]), (old_upper, [T.STR]),
                      (new_truthy, [O(T.STR)]), (new_member, [T.STR])):
        src = _source(fn, types)
        assert FMT_MARK not in src and CAP_MARK not in src
        assert "TpxFmtArg" not in src


def many_sites(x):
    return ("{}-{}".format(x["a"], x["b"]), "%d/%d" % (x["a"], x["b"]),
            "{:>8}".format(x["s"]), string.capwords(x["s"]),
            string.capwords(x["s"] + " x"), "{}-{}".format(x["b"], x["a"]))


def test_stage_with_new_ops_has_the_header_once():
    src = _source(many_sites, [T.I64, T.I64, T.STR], ["a", "b", "s"])
    assert src.count(FMT_MARK) == 1 and src.count(CAP_MARK) == 1
    assert src.count("tpx_format(heap") == 4
    assert src.count("tpx_capwords(heap") == 2
    # "{}-{}" twice: one embedded template
    assert src.count("__device__ const int fmt_prog") == 3
    only_cap = _source(lambda x: string.capwords(x), [T.STR])
    assert only_cap.count(CAP_MARK) == 1


# ---- lineage ------------------------------------------------------------------------

def fmt_col2(x):
    return "{:>6}|".format(x["c"])


def cap_col1_if_col3(x):
    return string.capwords(x["b"]) if x["d"] else ""


def keep_kl(x):
    return x["c"] in ["k", "l"]


def test_pushdown_sees_the_new_nodes_arguments():
    cols = ["a", "b", "c", "d"]
    sp = plan.build_stage([T.I64, T.STR, T.STR, O(T.I64)], cols,
                          [("map", fmt_col2)])
    assert sp.compilable, sp.why_not_compilable
    assert sorted(sp.used_source_cols) == [2]
    sp = plan.build_stage([T.I64, T.STR, T.STR, O(T.I64)], cols,
                          [("map", cap_col1_if_col3)])
    assert sorted(sp.used_source_cols) == [1, 3]
    sp = plan.build_stage([T.I64, T.STR, T.STR, O(T.I64)], cols,
                          [("filter", keep_kl)])
    assert sorted(sp.used_source_cols) == [0, 1, 2, 3]  # filter keeps the row


# ---- quote-freedom lattice ----------------------------------------------------------

def _qfree(fn, types, cols=None):
    sp = plan.build_stage(types, cols, [("map", fn)])
    assert sp.compilable, sp.why_not_compilable
    cg = codegen.StageCodegen(sp, source="csv", sink="csv",
                              csv_info={"null_values": [""]})
    return cg._thread_qfree()


def test_qfree_knows_the_new_ops():
    assert _qfree(lambda x: "{:05}|{}".format(x, x > 1), [T.I64]) == [True]
    assert _qfree(lambda x: "{}, {}".format(x, x), [T.I64]) == [False]
    assert _qfree(lambda a, b: "{}:{:>9}".format(a, b), [T.STR, T.STR]) == \
        [frozenset([0, 1])]
    assert _qfree(lambda a, b: "%s;%d" % (a, b), [T.STR, T.I64]) == \
        [frozenset([0])]
    assert _qfree(lambda a, b: '%s"%d' % (a, b), [T.STR, T.I64]) == [False]
    assert _qfree(lambda x: string.capwords(x), [T.STR]) == [frozenset([0])]
    assert _qfree(lambda x: string.capwords(x + ","), [T.STR]) == [False]


# ---- the oracle agrees with plain CPython on the vectors ----------------------------

def _same(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return (math.isnan(a) and math.isnan(b)) or (
            a == b and math.copysign(1.0, a) == math.copysign(1.0, b))
    if isinstance(a, tuple) and isinstance(b, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("name", [m[0] for m in V.MEM])
def test_oracle_agrees_with_cpython(name):
    _n, rows, cols, fn = [m for m in V.MEM if m[0] == name][0]
    data = rows()
    assert len(data) % 64 in (1, 63)  # 64k +- 1: a partial last wave
    want, excs = [], {}
    for r in data:
        try:
            want.append(fn(dict(zip(cols, r))) if cols else fn(r))
        except Exception as e:  # noqa: BLE001 — counted like the engine does
            excs[type(e).__name__] = excs.get(type(e).__name__, 0) + 1
    ref = pyoracle.run_pipeline(data, [("map", fn)], columns=cols)
    assert len(ref["output"]) == len(want)
    assert all(_same(g, w) for g, w in zip(ref["output"], want))
    assert ref["exception_counts"] == excs


def test_vectors_hold_the_values_the_tests_are_about():
    f = V.opt_f64_rows()
    assert None in f and any(v is not None and math.isnan(v) for v in f)
    assert any(v == 0.0 and math.copysign(1.0, v) < 0 for v in f if v is not None)
    i = V.opt_i64_rows()
    assert 0 in i and None in i
    assert V.t_guarded_div(0) == -1 and V.t_guarded_div(None) == -1
    s = V.opt_str_rows()
    assert "" in s and None in s
    assert any(sv is None for sv, _ in V.member_rows())
    # one thread's format outputs exceed a string-heap chunk (256 B) per row
    a, b, c, d = V.f_strs({"s": "x", "k": 1})
    assert len(c) > 241 and len(a) + len(b) + len(c) + len(d) > 256
    assert max(len(sv) for sv, _ in V.str_rows()) == 300

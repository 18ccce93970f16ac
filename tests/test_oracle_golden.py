"""Pin the oracle against golden vectors transcribed from the reference's own tests.

Each case in tests/golden/reference_goldens.json cites the reference test whose
literal assertions it transcribes; here the matching pipeline is reconstructed and run
through the oracle. If these pass, the oracle restates the reference's observable
semantics for this vocabulary and becomes the parity anchor for the GPU engine.
"""
import json
import os

import pytest

from oracle import pyoracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "reference_goldens.json")))["cases"]


def _tuplify(v):
    if isinstance(v, list):
        return tuple(_tuplify(x) for x in v)
    return v


def _load(name):
    c = GOLDEN[name]
    data = [_tuplify(x) for x in c["input"]]
    return c, data


def _run(name, ops, with_resolve=None):
    c, data = _load(name)
    cols = c.get("columns")
    r = pyoracle.run_pipeline(data, ops, columns=cols)
    expect = c["expect_output"]
    if expect == "same_as_input":
        expect = data
    else:
        expect = [_tuplify(x) for x in expect]
    assert r["output"] == expect, (name, r["output"], expect)
    assert r["exception_counts"] == c["expect_ecounts"], (name, r["exception_counts"])
    if with_resolve is not None:
        r2 = pyoracle.run_pipeline(data, ops + with_resolve, columns=cols)
        expect2 = [_tuplify(x) for x in c["after_resolve_output"]]
        assert r2["output"] == expect2, (name, r2["output"], expect2)
        assert r2["exception_counts"] == c["after_resolve_ecounts"]


def test_exceptions_map():
    _run("exceptions_test_map", [("map", lambda x: 1 // x)],
         [("resolve", ZeroDivisionError, lambda x: -1)])


def test_exceptions_filter():
    _run("exceptions_test_filter", [("filter", lambda x: (1 // x) < 5)],
         [("resolve", ZeroDivisionError, lambda x: True)])


def test_exceptions_mapColumn():
    _run("exceptions_test_mapColumn", [("mapColumn", "int", lambda x: 1 // x)],
         [("resolve", ZeroDivisionError, lambda x: -1)])


def test_exceptions_withColumn_replace():
    _run("exceptions_test_withColumn_replace",
         [("withColumn", "str", lambda x, y, z: str(1 // x) + y)],
         [("resolve", ZeroDivisionError, lambda x, y, z: "NULL")])


def test_strings_strconv_option():
    _run("strings_test_strconv_option", [("map", lambda x: str(x))])


def test_aggregates_count():
    _run("aggregates_test_simple_count",
         [("aggregate", lambda a, b: a + b, lambda a, x: a + 1, 0)])


def test_aggregates_sum():
    _run("aggregates_test_simple_sum",
         [("aggregate", lambda a, b: a + b, lambda a, x: a + x, 0)])


def test_parallelize_tuple_option_I():
    _run("parallelize_tuple_option_I", [])


def test_parallelize_tuple_option_II():
    _run("parallelize_tuple_option_II", [])


def test_baseline_config1_plumbing():
    _run("baseline_config1_plumbing", [("map", lambda x: (x, x * x))])


def test_strings_swapcase():
    _run("strings_swapcase", [("map", lambda x: x.swapcase())])


def test_strings_startswith():
    _run("strings_startswith", [("map", lambda s, p: s.startswith(p))])


# ---- parse-function restatements pinned by construction -------------------------

def test_fast_atoi64_quirks():
    """StringUtils.cc:22 semantics incl. quirks: '-' parses to 0; no '+' allowed;
    empty fails; trailing junk fails."""
    assert pyoracle.fast_atoi64("123") == (True, 123)
    assert pyoracle.fast_atoi64("-42") == (True, -42)
    assert pyoracle.fast_atoi64("-") == (True, 0)
    assert pyoracle.fast_atoi64("+5")[0] is False
    assert pyoracle.fast_atoi64("")[0] is False
    assert pyoracle.fast_atoi64("12x")[0] is False
    assert pyoracle.fast_atoi64("007") == (True, 7)


def test_fast_atod_quirks():
    ok, v = pyoracle.fast_atod("3.25")
    assert ok and v == 3.25
    ok, v = pyoracle.fast_atod("-1e3")
    assert ok and v == -1000.0
    ok, v = pyoracle.fast_atod(".")
    assert ok and v == 0.0  # StringUtils.cc:71 quirk: '.' parses to 0.0
    assert pyoracle.fast_atod("1.2.3")[0] is False
    ok, v = pyoracle.fast_atod("nan")
    assert ok and v != v
    ok, v = pyoracle.fast_atod("inf")
    assert ok and v == float("inf")


def test_fast_atod_exponent_wraps_like_unsigned_int():
    """StringUtils.cc:114-130 accumulates the exponent in an `unsigned int`:
    it wraps mod 2^32 per digit before the clamp at 308. Expectations recorded
    from the reference function (double bit patterns)."""
    import struct
    recorded = {"1e4294967295": 0x7fe1ccf385ebc8a3,  # clamps to 1e308's product
                "1e4294967296": 0x3ff0000000000000,  # wraps to e0 -> 1.0
                "1e4294967297": 0x4024000000000000,  # wraps to e1 -> 10.0
                "1e-4294967297": 0x3fb999999999999a}
    for s, bits in recorded.items():
        ok, v = pyoracle.fast_atod(s)
        assert ok, s
        assert struct.unpack("<Q", struct.pack("<d", v))[0] == bits, (s, v)


def test_ref_int_matches_python_on_normal():
    for s in ["0", "42", "-7", "  13  ", "1560"]:
        assert pyoracle.ref_int(s) == int(s)


def test_sum_by_key_golden():
    """tuplex/python/tests/test_aggregates.py:40 test_sum_by_key literal
    expectations (sorted compare — by-key order is parity-unpinned)."""
    data = [(0, 10.0), (1, 20.0), (0, -4.5)]
    r = pyoracle.run_pipeline(
        data, [("aggregateByKey", lambda a, b: a + b,
                lambda a, x: a + x["volume"], 0.0, ["id"])],
        columns=["id", "volume"])
    res = sorted(r["output"])
    assert len(res) == 2
    assert res[0][0] == 0 and res[1][0] == 1
    assert abs(res[0][1] - 5.5) < 1e-9 and abs(res[1][1] - 20.0) < 1e-9


def test_zillow_udfs_vs_cpython():
    """The reference pins zillow-UDF results by comparing the compiled path against a
    per-row CPython map (test/wrappers/WrapperTest.cc:468 extractPriceExample). Same
    methodology: oracle fast path == CPython on normal-case synthetic rows."""
    def extractPrice(x):
        price = x["price"]
        if x["offer"] == "sold":
            val = x["facts and features"]
            s = val[val.find("Price/sqft:") + len("Price/sqft:") + 1:]
            r = s[s.find("$") + 1:s.find(", ") - 1]
            price_per_sqft = int(r)
            price = price_per_sqft * x["sqft"]
        elif x["offer"] == "rent":
            max_idx = price.rfind("/")
            price = int(price[1:max_idx].replace(",", ""))
        else:
            price = int(price[1:].replace(",", ""))
        return price

    rows = [
        ("$489,000", "sale", "3 bds , 1 ba , 1,560 sqft", 1560),
        ("$3,700/mo", "rent", "2 bds , 1 ba , 920 sqft", 920),
        ("$250,000", "sold", "Price/sqft: $161, 3 bds", 1550),
    ]
    cols = ["price", "offer", "facts and features", "sqft"]
    r = pyoracle.run_pipeline(list(rows), [("map", extractPrice)], columns=cols)
    expect = [extractPrice(dict(zip(cols, row))) for row in rows]
    assert r["output"] == expect
    assert r["exception_counts"] == {}


def test_filter_squares():
    _run("filter_squares", [("map", lambda x: x * x),
                            ("filter", lambda x: x > 10)])


def test_filter_bool_or_cubes():
    _run("filter_bool_or_cubes",
         [("filter", lambda x: x == 2 or x == 3 or x == 5),
          ("map", lambda x: x * x * x)])


def test_filter_chained_compare():
    _run("filter_chained_compare", [("filter", lambda x: 2 < x <= 4)])


def test_filter_all_empty():
    _run("filter_all_empty", [("filter", lambda x: x > 10)])


def test_arith_add_float():
    _run("arith_add_float", [("map", lambda x: x + 10.7)])


def test_arith_unary_neg():
    _run("arith_unary_neg", [("map", lambda x: -x)])


def test_arith_idiv_pos():
    _run("arith_idiv_pos", [("map", lambda x: x // 7)])


def test_arith_idiv_negdiv():
    _run("arith_idiv_negdiv", [("map", lambda x: x // -6)])


def test_strings_concat():
    _run("strings_concat", [("map", lambda a, b: a + b)])


def test_strings_dup_str_int():
    _run("strings_dup_str_int", [("map", lambda a, b: a * b)])


def test_strings_dup_int_str():
    _run("strings_dup_int_str", [("map", lambda a, b: a * b)])


def test_strings_center3():
    _run("strings_center3", [("map", lambda x: x.center(3))])


def test_strings_center4_fill():
    _run("strings_center4_fill", [("map", lambda x, y: x.center(4, y))])


def test_nulls_eq_none_mixed():
    _run("nulls_eq_none_mixed", [("map", lambda x: x == None)])  # noqa: E711


def test_nulls_ne_none_mixed():
    _run("nulls_ne_none_mixed", [("map", lambda x: x != None)])  # noqa: E711


def test_is_bool_false():
    _run("is_bool_false", [("map", lambda x: x is False)])


def test_is_none_opt_bool():
    _run("is_none_opt_bool", [("map", lambda x: x is not None)])

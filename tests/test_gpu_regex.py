"""GPU parity of compiled re.search/re.match/re.fullmatch UDFs (device regex VM,
csrc/tpx_re.hip.h) with the oracle running the same Python UDFs. Every test
asserts the stage ran on the GPU: before this feature any `re.` UDF sent the
whole stage to the interpreter. Stage sources are precompiled by build()
(tests/regex_pipelines.py precompile)."""
import os

import pytest

import tuplex_amd
from oracle import pyoracle, pyoracle_csv
from tests import regex_pipelines as RP
from tests.pipelines import apply_ops

pytestmark = pytest.mark.gpu


def _gpu(ds):
    assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason


@pytest.fixture(scope="module")
def log_lines():
    return RP.make_log_lines(5000, seed=11, bad_frac=0.02, nonascii=3)


@pytest.fixture(scope="module")
def log_file(tmp_path_factory, log_lines):
    data = RP.log_text_bytes(log_lines)
    p = os.path.join(str(tmp_path_factory.mktemp("relog")), "access.log")
    with open(p, "wb") as f:
        f.write(data)
    return p, data


@pytest.fixture(scope="module")
def log_ref(log_file):
    return pyoracle_csv.run_text_pipeline(log_file[1], RP.regex_ops())


def test_text_source_nine_group_collect(log_file, log_ref):
    path, _data = log_file
    ctx = tuplex_amd.Context()
    ds = apply_ops(ctx.text(path), RP.regex_ops())
    got = ds.collect()
    _gpu(ds)
    assert got == log_ref["output"]
    assert ds.exception_counts == log_ref["exception_counts"]
    # the filter dropped the malformed lines, kept the rest
    assert 4700 < len(got) < 5000


def test_text_source_nine_group_tocsv(tmp_path, log_file, log_ref):
    path, _data = log_file
    outp = os.path.join(str(tmp_path), "out.csv")
    ctx = tuplex_amd.Context()
    ds = apply_ops(ctx.text(path), RP.regex_ops())
    ds.tocsv(outp)
    _gpu(ds)
    want = [pyoracle_csv.format_csv_row(["column%d" % i for i in range(9)])]
    want += [pyoracle_csv.format_csv_row(list(r)) for r in log_ref["output"]]
    assert open(outp, "rb").read() == b"".join(want)


def test_split_regex_with_column_chain(log_lines):
    ctx = tuplex_amd.Context()
    ops = RP.split_regex_ops()
    ds = apply_ops(ctx.parallelize(log_lines, columns=["logline"]), ops)
    got = ds.collect()
    _gpu(ds)
    ref = pyoracle.run_pipeline(log_lines, ops, columns=["logline"])
    assert got == ref["output"]
    assert ds.exception_counts == ref["exception_counts"]
    assert len(got) > 4700


@pytest.fixture(scope="module")
def sem_rows():
    return RP.sem_strings()


@pytest.mark.parametrize("fn", RP.SEM_UDFS, ids=lambda f: f.__name__)
def test_semantics_table(fn, sem_rows):
    ctx = tuplex_amd.Context()
    ds = ctx.parallelize(sem_rows).map(fn)
    got = ds.collect()
    _gpu(ds)
    ref = pyoracle.run_pipeline(sem_rows, [("map", fn)])
    assert got == ref["output"]
    assert ds.exception_counts == ref["exception_counts"]
    assert len(got) == len(sem_rows) >= 200


def test_budget_divert_is_silent():
    """(a+)+b on 'a'*12..16 exhausts the VM's step budget: those rows take the
    silent host replay (CPython answers them in milliseconds) and no count
    shows up."""
    rows = RP.budget_rows()
    ctx = tuplex_amd.Context()
    ds = ctx.parallelize(rows).map(RP.nested_plus)
    got = ds.collect()
    _gpu(ds)
    assert got == [RP.nested_plus(r) for r in rows]
    ref = pyoracle.run_pipeline(rows, [("map", RP.nested_plus)])
    assert got == ref["output"]
    assert ds.exception_counts == ref["exception_counts"] == {}


def test_unguarded_group_typeerror():
    rows = RP.digit_rows()
    ctx = tuplex_amd.Context()
    ops = [("map", RP.unguarded_digits)]
    ds = apply_ops(ctx.parallelize(rows), ops)
    got = ds.collect()
    _gpu(ds)
    ref = pyoracle.run_pipeline(rows, ops)
    assert got == ref["output"]
    assert ds.exception_counts == ref["exception_counts"]
    assert ds.exception_counts.get("TypeError", 0) > 20

    ops = ops + [("resolve", TypeError, RP.empty_resolver)]
    ds = apply_ops(ctx.parallelize(rows), ops)
    got = ds.collect()
    _gpu(ds)
    ref = pyoracle.run_pipeline(rows, ops)
    assert got == ref["output"]
    assert ds.exception_counts == ref["exception_counts"] == {}
    assert len(got) == len(rows) and "" in got


@pytest.fixture(scope="module")
def long_rows():
    return RP.long_rows()


@pytest.mark.parametrize("fn", [RP.long_anchored, RP.long_search],
                         ids=lambda f: f.__name__)
def test_long_rows_beyond_lds_span(fn, long_rows):
    ctx = tuplex_amd.Context()
    ds = ctx.parallelize(long_rows).map(fn)
    got = ds.collect()
    _gpu(ds)
    ref = pyoracle.run_pipeline(long_rows, [("map", fn)])
    assert got == ref["output"]
    assert ds.exception_counts == ref["exception_counts"]
    assert len(got) == 300

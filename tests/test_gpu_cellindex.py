"""The wave-cooperative cell index end to end: GpuLib.compile_stage +
tpx_stage_execute_csv (flags 0) on the stages of tests/cellindex_pipelines.py.

For every input the build with the index (TPX_CELL_INDEX=1) and the build
without (TPX_CELL_INDEX=0) must agree byte for byte on the output (csv text or
serialized rows), the row offsets, the row indices and the exception records,
for the csv sink (index overlaid on the wave's output window) and for the mem
sink (index region of its own). Each build must also agree with
oracle/pyoracle_csv.

The oracle replays on the host every row the device diverts. The inputs are
built so that no diverted row yields an output row: wrong column counts fail
on the host too, and the escaped / junk / UTF-8 rows carry a qty the filter
drops. The device's exception rows are then the oracle's exceptions plus the
known cleanly diverted rows.

Through this entry point the first batch of an input starts at byte 0, so the
span start that is not 16-aligned (bytes of the previous row masked out of the
index) is exercised by the second and later batches; test_span_starts checks
that the inputs really have such batches.
"""
import functools

import pytest

from oracle import pyoracle_csv
from tests import cellindex_pipelines as CP

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle(case, sink):
    body = CP.case_body(case)
    if not body.endswith(b"\n"):
        # tpx_stage_execute_csv's boundary scan makes a row of every
        # even-parity newline; the reader (csvio) appends the missing final
        # newline before it calls. Given the raw bytes the entry point sees
        # the terminated rows only, with or without the index.
        body = body[:body.rfind(b"\n") + 1]
    ref = pyoracle_csv.run_csv_pipeline(
        CP.HEADER + body,
        CP.ops("csv" if sink == "csv" else "mem"), header=True, sink=sink,
        delimiter=",", type_hints=CP.TYPE_HINTS)
    if sink == "csv":
        head, body = ref["csv_text"].split(b"\n", 1)
        assert head == b"name,qty,price,note"
        return body, ref["exception_counts"]
    return ref["output"], ref["exception_counts"]


@functools.lru_cache(maxsize=None)
def _run(case, sink, build):
    return CP.execute(CP.case_body(case), sink=sink, build=build)


def _check(case, sink, diverted_clean=0):
    want, exc_counts = _oracle(case, "csv" if sink == "csv" else "collect")
    got = _run(case, sink, "index")
    ref = _run(case, sink, "walk")
    for k in ("data", "offsets", "indices", "excs"):
        assert got[k] == ref[k], k
    for out in (got, ref):
        if sink == "csv":
            assert out["data"] == want
            offs = out["offsets"]
            assert offs[0] == 0 and offs[-1] == len(want)
        else:
            assert [tuple(r) for r in out["rows"]] == \
                [tuple(r) for r in want]
        assert len(out["excs"]) == sum(exc_counts.values()) + diverted_clean
        assert out["indices"] == sorted(out["indices"])
    return got


def test_builds_differ_only_where_the_index_applies():
    for sink in ("csv", "mem"):
        _sp, src_i, desc_i = CP.generate(sink, "index")
        _sp, src_w, desc_w = CP.generate(sink, "walk")
        assert "tpx_ci_stage(" in src_i and "tpx_ci_row(" in src_i
        assert "tpx_ci_" not in src_w
        assert desc_i == desc_w
    # fused window: the index overlays the output window
    assert "wave_ci = wave_out" in CP.generate("csv", "index")[1]
    assert "wave_ci = wave_out" not in CP.generate("mem", "index")[1]
    # one column above the limit, and a '|' delimiter: source unchanged
    assert CP.generate_wide("index")[1:] == CP.generate_wide("walk")[1:]
    assert CP.generate_pipe("index")[1:] == CP.generate_pipe("walk")[1:]
    assert "tpx_ci_" not in CP.generate_wide("index")[1]


def test_span_starts():
    """Batches 1.. of the multi-batch inputs start off a 16-byte boundary."""
    for case in ("n65", "n129", "crlf"):
        rows = CP.CASES[case]()
        assert sum(len(r) for r in rows[:64]) % 16 != 0, case


@pytest.mark.parametrize("sink", ["csv", "mem"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_row_counts(n, sink):
    got = _check("n%d" % n, sink)
    want = [i for i in range(n) if (i * 37) % 700 < CP.KEEP_BELOW]
    assert got["indices"] == want


@pytest.mark.parametrize("sink", ["csv", "mem"])
def test_crlf(sink):
    got = _check("crlf", sink)
    assert b"\r" not in got["data"] or sink == "mem"


@pytest.mark.parametrize("sink", ["csv", "mem"])
def test_no_trailing_newline(sink):
    """The input's last row has no newline: the wave's span then ends inside
    the buffer without a terminator (the index's virtual entry is covered on
    the host, tests/host_cellindex_test.cpp); both builds must still agree on
    every terminated row."""
    got = _check("no_final_newline", sink)
    assert got["indices"][-1] == 68          # (68 * 37) % 700 == 416: kept


@pytest.mark.parametrize("sink", ["csv", "mem"])
def test_unstaged_batch_between_staged_ones(sink):
    got = _check("long_between", sink)
    assert set(range(64, 128)) <= set(got["indices"])


def test_embedded_newlines_and_commas_survive():
    got = _check("n129", "csv")
    assert b'"TWO\nLINES 2"' in got["data"]
    assert b'"A,B\n,C3"' in got["data"]
    assert b'"has, comma 3"' in got["data"]


@pytest.mark.parametrize("sink", ["csv", "mem"])
@pytest.mark.parametrize("kind", CP.ODD_KINDS)
def test_odd_rows(kind, sink):
    """The odd row alone in a batch, in lane 0 and in lane 63."""
    at = [31, 64, 191]
    clean = 3 if kind in ("esc", "junk", "utf8") else 0
    got = _check("odd_" + kind, sink, diverted_clean=clean)
    rows = CP.CASES["odd_" + kind]()
    if kind in CP.DIVERTED:
        assert [e[0] for e in got["excs"]] == at
        assert [e[3] for e in got["excs"]] == [rows[i] for i in at]
        assert not set(got["indices"]) & set(at)
    else:
        assert got["excs"] == []
        assert set(at) <= set(got["indices"])


def test_empty_input():
    for sink in ("csv", "mem"):
        a = CP.execute(b"", sink=sink, build="index")
        b = CP.execute(b"", sink=sink, build="walk")
        assert a == b and a["indices"] == [] and a["excs"] == []

"""Cold paths out of line (TPX_OUTLINE=1, the default) against the same
stages with everything inline (TPX_OUTLINE=0), end to end through
GpuLib.compile_stage + tpx_stage_execute_csv (flags 0).

Every input of tests/outline_pipelines.py puts a path that moved out of
tpx_stage_main next to the hot path in one launch: an unstaged batch between
staged ones, rows the cell index declines among rows it accepts and a batch
whose entry list overflows, a wave whose text exceeds the output window and
rows with cells to quote, a row that raises in the UDF chain and an f64 cell
that does not parse. For each, both builds must give the text (or rows), the
row order and the exception set of oracle/pyoracle_csv, and agree with each
other byte for byte, exception payloads included.

As in test_gpu_cellindex.py the oracle replays diverted rows on the host, and
the inputs are built so that a diverted row that replays cleanly is dropped
by the filter: the device's exception rows are the oracle's exceptions plus
those known rows.
"""
import functools

import pytest

from oracle import pyoracle_csv
from tests import cellindex_pipelines as CP
from tests import fused_pipelines as FP
from tests import outline_pipelines as OP

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ci_oracle(case, sink):
    ref = pyoracle_csv.run_csv_pipeline(
        CP.HEADER + b"".join(OP.CI_CASES[case]()),
        CP.ops("csv" if sink == "csv" else "mem"), header=True,
        sink="csv" if sink == "csv" else "collect",
        delimiter=",", type_hints=CP.TYPE_HINTS)
    if sink == "csv":
        head, body = ref["csv_text"].split(b"\n", 1)
        assert head == b"name,qty,price,note"
        return body, ref["exception_counts"]
    return ref["output"], ref["exception_counts"]


@functools.lru_cache(maxsize=None)
def _fs_oracle(case):
    ref = pyoracle_csv.run_csv_pipeline(
        FP.HEADER + b"".join(OP.FS_CASES[case]()), FP.ops(), header=True,
        sink="csv", delimiter=",", type_hints=FP.TYPE_HINTS)
    head, body = ref["csv_text"].split(b"\n", 1)
    assert head == b"label,city,n,note"
    return body, ref["exception_counts"]


@functools.lru_cache(maxsize=None)
def _ci_run(case, sink, level):
    return OP.ci_execute(case, sink, level)


@functools.lru_cache(maxsize=None)
def _fs_run(case, level):
    return OP.fs_execute(case, level)


def _ci_check(case, sink, level, diverted_clean=0):
    want, exc_counts = _ci_oracle(case, sink)
    got = _ci_run(case, sink, level)
    if sink == "csv":
        assert got["data"] == want
        assert got["offsets"][0] == 0 and got["offsets"][-1] == len(want)
    else:
        assert [tuple(r) for r in got["rows"]] == [tuple(r) for r in want]
    assert len(got["excs"]) == sum(exc_counts.values()) + diverted_clean
    assert got["indices"] == sorted(got["indices"])
    other = _ci_run(case, sink, "0" if level == "1" else "1")
    for k in ("data", "offsets", "indices", "excs"):
        assert got[k] == other[k], k
    return got


def _fs_check(case, level):
    want, exc_counts = _fs_oracle(case)
    got = _fs_run(case, level)
    assert got["text"] == want
    offs = got["offsets"]
    assert offs[0] == 0 and offs[-1] == len(want)
    assert [want[a:b] for a, b in zip(offs, offs[1:])] == \
        want.splitlines(keepends=True)
    assert len(got["excs"]) == sum(exc_counts.values())
    assert got["indices"] == sorted(got["indices"])
    other = _fs_run(case, "0" if level == "1" else "1")
    for k in ("text", "offsets", "indices", "excs"):
        assert got[k] == other[k], k
    return got


def test_builds_differ():
    for gen in (lambda: CP.generate("csv", "index")[1:],
                lambda: CP.generate("mem", "index")[1:],
                lambda: FP.generate("fused")):
        with OP.outline("1"):
            src1, desc1 = gen()
        with OP.outline("0"):
            src0, desc0 = gen()
        assert desc1 == desc0
        # ahead of the runtime header, whose own default is 0
        assert src1.split("\n")[1] == "#define TPX_OUTLINE 1"
        assert not src0.split("\n")[1].startswith("#define TPX_OUTLINE")
        assert "tpx_batch_unstaged(" in src1
        assert "tpx_batch_unstaged(" not in src0
        assert "tpx_walk_row<" in src1.split("struct Out {")[1]
        assert "tpx_walk_row<" not in src0.split("struct Out {")[1]
        # the accepted row builds no walk state
        main1 = src1[src1.index('extern "C" __global__', src1.index("struct Out {")):]
        assert "tpx_mw_init(" not in main1 and "tpx_mwalk S" not in main1


@pytest.mark.parametrize("level", OP.LEVELS)
@pytest.mark.parametrize("sink", ["csv", "mem"])
def test_unstaged_batch_between_staged_ones(sink, level):
    got = _ci_check("unstaged", sink, level)
    assert set(range(64, 128)) <= set(got["indices"])
    assert got["excs"] == []


@pytest.mark.parametrize("level", OP.LEVELS)
def test_unstaged_batch_fused_stage(level):
    got = _fs_check("unstaged", level)
    assert set(range(64, 130)) <= set(got["indices"])


@pytest.mark.parametrize("level", OP.LEVELS)
@pytest.mark.parametrize("sink", ["csv", "mem"])
def test_declined_rows_among_accepted_ones(sink, level):
    # esc x2, junk, utf8 replay cleanly on the host and the filter drops them
    got = _ci_check("declined", sink, level, diverted_clean=4)
    rows = OP.ci_declined()
    diverted = [5, 17, 29, 35, 41, 63] + [i for i in range(64, 128)
                                          if i % 16 == 3]
    assert [e[0] for e in got["excs"]] == diverted
    assert [e[3] for e in got["excs"]] == [rows[i] for i in diverted]
    # stray quotes and a bare CR are ordinary cells; the walked batch keeps
    # its well-formed rows
    assert {11, 23, 128, 129} <= set(got["indices"])
    keep1 = [i for i in range(64, 128)
             if i % 16 != 3 and (i * 37) % 700 < CP.KEEP_BELOW]
    assert keep1 and set(keep1) <= set(got["indices"])


@pytest.mark.parametrize("level", OP.LEVELS)
@pytest.mark.parametrize("sink", ["csv", "mem"])
def test_wave_above_the_output_window(sink, level):
    got = _ci_check("direct", sink, level)
    assert got["indices"] == list(range(130))
    if sink == "csv":
        assert got["data"].count(b'"w, ') == len(range(72, 128, 9))


@pytest.mark.parametrize("level", OP.LEVELS)
def test_wave_above_the_output_window_fused_stage(level):
    got = _fs_check("direct_quoting", level)
    assert got["indices"] == list(range(130))
    assert got["text"].count(b'""') > 0        # labels with a doubled quote


@pytest.mark.parametrize("level", OP.LEVELS)
@pytest.mark.parametrize("sink", ["csv", "mem"])
def test_few_cells_to_quote(sink, level):
    got = _ci_check("quoting", sink, level, diverted_clean=1)
    assert [e[0] for e in got["excs"]] == [77]
    if sink == "csv":
        assert got["data"].count(b'"SMITH, J') == 10


@pytest.mark.parametrize("level", OP.LEVELS)
@pytest.mark.parametrize("sink", ["csv", "mem"])
def test_f64_cell_that_does_not_parse(sink, level):
    got = _ci_check("badf64", sink, level)
    rows = OP.ci_badf64()
    assert [e[0] for e in got["excs"]] == [7, 64, 129]
    assert [e[3] for e in got["excs"]] == [rows[i] for i in (7, 64, 129)]
    assert len(got["indices"]) == 127


@pytest.mark.parametrize("level", OP.LEVELS)
def test_row_that_raises_in_the_udf_chain(level):
    got = _fs_check("raises", level)
    assert [e[0] for e in got["excs"]] == [9, 64, 129]
    assert len(got["indices"]) == 127

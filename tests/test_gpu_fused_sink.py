"""The fused csv sink end to end: GpuLib.compile_stage + tpx_stage_execute_csv
(flags 0) on the stage of tests/fused_pipelines.py.

Two references for every input, and the direct-format variant of the fused
build (TPX_FUSED_WINDOW=0) must agree with the default one everywhere. The
expected text and the exception counts
come from oracle/pyoracle_csv.run_csv_pipeline. Separately, the
TPX_FUSED_SINK=0 build of the same stage (columnar slots + tpx_stage_write) on
the same input must give the same bytes, row offsets, row indices and
exception records.

The oracle replays on the host every row the device diverts, so its text also
holds diverted rows that replay cleanly. The inputs here are built so that no
diverted row yields an output row: wrong column counts fail on the host too,
and the non-ASCII rows are dropped by the filter. The device's exception rows
are then the oracle's exceptions plus the known non-ASCII rows.
"""
import functools
import json
import os
import subprocess
import sys

import pytest

from oracle import pyoracle_csv
from tests import fused_pipelines as FP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _oracle(case):
    ref = pyoracle_csv.run_csv_pipeline(
        FP.HEADER + FP.case_body(case), FP.ops(), header=True, sink="csv",
        delimiter=",", type_hints=FP.TYPE_HINTS)
    head, body = ref["csv_text"].split(b"\n", 1)
    assert head == b"label,city,n,note"
    return body, ref["exception_counts"]


@functools.lru_cache(maxsize=None)
def _run(case, build):
    return FP.execute(FP.case_body(case), build=build)


def _check(case, diverted_clean=0):
    want, exc_counts = _oracle(case)
    got = _run(case, "fused")
    assert got["text"] == want
    assert len(got["excs"]) == sum(exc_counts.values()) + diverted_clean
    # offsets delimit the rows of the text, in input order
    offs = got["offsets"]
    assert offs[0] == 0 and offs[-1] == len(want)
    assert [want[a:b] for a, b in zip(offs, offs[1:])] == \
        want.splitlines(keepends=True)
    assert got["indices"] == sorted(got["indices"])
    for other in ("twopass", "direct"):
        ref = _run(case, other)
        for k in ("text", "offsets", "indices", "excs"):
            assert got[k] == ref[k], (other, k)
    return got


def test_builds_differ():
    src_f, desc_f = FP.generate("fused")
    src_d, desc_d = FP.generate("direct")
    src_t, desc_t = FP.generate("twopass")
    assert "fusedcsv=1" in desc_f and "fusedcsv" not in desc_t
    assert desc_d == desc_f
    assert "tpx_stage_write(" not in src_f and "tpx_stage_write(" in src_t
    assert "tpx_wave_commit_csv(_K" in src_f
    assert "tpx_wave_commit_csv(_K" not in src_t
    assert "wave_out" in src_f and "wave_out" not in src_d


@pytest.mark.parametrize("pattern", ["all", "none", "alt"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_row_counts(n, pattern):
    got = _check("n%d_%s" % (n, pattern))
    kept = {"all": n, "none": 0, "alt": (n + 1) // 2}[pattern]
    assert len(got["indices"]) == kept
    if pattern == "alt":
        assert got["indices"] == list(range(0, n, 2))


def test_long_rows_take_the_global_body():
    got = _check("long_and_short")
    assert got["indices"][:64] == list(range(64))
    assert len(got["indices"]) > 64


def test_cells_that_need_quoting():
    got = _check("quoting")
    assert b'"has, comma 0"' in got["text"]
    assert b' ""cITY0"""' in got["text"]          # fs_label's own quotes
    assert b'"Smith, J' in got["text"]


def test_wave_text_above_the_window():
    got = _check("big_wave")
    offs = got["offsets"]
    assert offs[128] - offs[64] > FP.TEXT_WINDOW


def test_malformed_rows_inside_batches():
    rows, bad = FP.rows_malformed()
    got = _check("malformed", diverted_clean=2)
    assert [e[0] for e in got["excs"]] == bad
    assert [e[3] for e in got["excs"]] == [rows[i] for i in bad]
    assert not set(got["indices"]) & set(bad)


def test_empty_input():
    for build in FP.BUILDS:
        out = FP.execute(b"", build=build)
        assert out == {"text": b"", "offsets": [0], "indices": [], "excs": []}


def test_second_execute_gives_the_same_bytes():
    body = FP.case_body("quoting")
    first = FP.execute(body)
    second = FP.execute(body)
    assert first == second == _run("quoting", "fused")


def test_text_scratch_overflow_is_retried():
    """A 64-byte first-attempt text scratch: every wave overflows, the host
    grows the scratch to the cursors' high-water mark and redoes the attempt.
    The capacity override is read once per process, so this runs a child."""
    env = dict(os.environ, TPX_TEXT_CAP0="64")
    env.pop("TPX_FUSED_SINK", None)
    env.pop("TPX_FUSED_WINDOW", None)
    p = subprocess.run([sys.executable, "-m", "tests.fused_pipelines",
                        "big_wave"], cwd=ROOT, env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode("utf-8", "replace")[-2000:]
    got = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert got == FP.digest(_run("big_wave", "fused"))
    assert got["bytes"] > 64

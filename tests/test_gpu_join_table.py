"""Device join tables on the GPU.

Kernel level (tests/hipkern_join.py): the build kernel is launched alone over
the key vectors of tests/join_table_cases.py, then a tiny probe kernel over
hit and miss keys. Every build key must probe to its own row and every absent
key to -1; the table holds exactly n occupied slots; each key is reachable
from its home slot without crossing an empty one; canaries stay intact. Slot
placement under collisions depends on the order of the atomics and is not
asserted.

End to end: joins whose build side lives in a tpx_jtable against the python
oracles, all by exact equality (values are copied, never recomputed)."""
import json
import os
import subprocess
import sys

import pytest

import tuplex_amd
from oracle import pyoracle, pyoracle_csv
from tests import join_table_cases as C
from tests import join_table_pipelines as JP
from tests.pipelines import apply_ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- kernel level ----------------------------------------------------------------

def _check_table(keys, absent, is_str):
    from tests import hipkern_join as HJ
    n = len(keys)
    tsize = C.table_size(n)
    tab = HJ.BuiltTable(keys, tsize, is_str)
    rows, tags = tab.slot_rows()
    assert len(rows) == tsize
    occupied = [s for s in range(tsize) if rows[s] != -1]
    assert len(occupied) == n
    assert sorted(rows[s] for s in occupied) == list(range(n))
    for s in occupied:
        k = keys[rows[s]]
        if is_str:
            h = C.hash_bytes(k.encode("utf-8"))
            assert tags[s] == h >> 32
        else:
            h = C.hash_i64(k)
            assert tags[s] == k
        # reachable from home without crossing an empty slot
        p = h & (tsize - 1)
        steps = 0
        while p != s:
            assert rows[p] != -1, (k, h & (tsize - 1), s)
            p = (p + 1) & (tsize - 1)
            steps += 1
            assert steps < tsize
    queries = list(keys) + list(absent)
    want = list(range(n)) + [-1] * len(absent)
    assert tab.probe(queries) == want
    return rows


@pytest.mark.parametrize("n", C.SIZES)
def test_build_and_probe_i64(n):
    keys, absent = C.i64_case(n)
    assert absent
    _check_table(keys, absent, False)


@pytest.mark.parametrize("n", C.SIZES)
def test_build_and_probe_str(n):
    keys, absent = C.str_case(n)
    assert absent
    _check_table(keys, absent, True)


def test_colliding_home_sets_wrap():
    """12 keys whose home is the last slot: the run wraps to slot 0."""
    for n in (63, 256):
        ts = C.table_size(n)
        for is_str, case in ((False, C.i64_case), (True, C.str_case)):
            keys, absent = case(n)
            rows = _check_table(keys, absent, is_str)
            assert rows[ts - 1] != -1 and rows[0] != -1


# ---- end to end ------------------------------------------------------------------

def _ctx(mode=None):
    return tuplex_amd.Context({"tuplex.gpu.joinTable": mode} if mode else None)


@pytest.mark.parametrize("how", ["inner", "left"])
def test_device_table_mem_parity(how):
    left = JP.left_rows()
    ops = [JP.jop(JP.build_side(), how)]
    ds = apply_ops(_ctx("device").parallelize(left, columns=JP.LCOLS), ops)
    got = ds.collect()
    o = ds._last_outcome
    assert o.mode == "gpu", o.fallback_reason
    assert o.metrics["join_table"] == "device"
    assert o.metrics["join_table_bytes"] > 0
    assert o.metrics["join_build_ms"] >= 0.0
    ref = pyoracle.run_pipeline(left, ops, columns=JP.LCOLS)
    assert got == ref["output"]
    assert ds.exception_counts == ref["exception_counts"]
    hits = [r for r in got if r[2:] != (None, None, None, None)]
    assert 0 < len(hits) < len(left)
    # the handle lives with the DataSet: a second action reuses the table
    from tuplex_amd.jointab import BuildRows
    rrows = ds._ops[0][1]
    assert isinstance(rrows, BuildRows) and len(rrows._jtables) == 1
    tab = next(iter(rrows._jtables.values()))
    assert ds.collect() == got
    assert next(iter(rrows._jtables.values())) is tab


def test_embedded_metric_under_default_options():
    left = JP.left_rows(500)
    ops = [JP.jop(JP.small_build(), rcols=JP.BIG_RCOLS)]
    ds = apply_ops(_ctx().parallelize(left, columns=JP.LCOLS), ops)
    got = ds.collect()
    assert ds._last_outcome.mode == "gpu"
    assert ds._last_outcome.metrics["join_table"] == "embedded"
    assert got == pyoracle.run_pipeline(left, ops, columns=JP.LCOLS)["output"]


def test_device_table_csv_string_key_tocsv(tmp_path):
    data = JP.csv_bytes()
    p = os.path.join(str(tmp_path), "in.csv")
    with open(p, "wb") as f:
        f.write(data)
    outp = os.path.join(str(tmp_path), "out.csv")
    ops = JP.csv_ops(JP.dim_rows())
    ds = apply_ops(_ctx("device").csv(p), ops)
    ds.tocsv(outp)
    o = ds._last_outcome
    assert o.mode == "gpu", o.fallback_reason
    assert o.metrics["join_table"] == "device"
    ref = pyoracle_csv.run_csv_pipeline(data, ops, sink="csv")
    with open(outp, "rb") as f:
        got = f.read()
    assert got == ref["csv_text"]
    assert got.count(b"\n") > 100
    assert ds.exception_counts == ref["exception_counts"]


def test_device_table_csv_left_join_collect(tmp_path):
    data = JP.csv_bytes()
    p = os.path.join(str(tmp_path), "in.csv")
    with open(p, "wb") as f:
        f.write(data)
    ops = JP.csv_left_ops(JP.dim_rows())
    ds = apply_ops(_ctx("device").csv(p), ops)
    got = ds.collect()
    o = ds._last_outcome
    assert o.mode == "gpu", o.fallback_reason
    assert o.metrics["join_table"] == "device"
    ref = pyoracle_csv.run_csv_pipeline(data, ops)
    assert got == ref["output"]
    assert ds.exception_counts == ref["exception_counts"]
    # cache() of such a stage keeps the host cache, and says why
    dc = apply_ops(_ctx("device").csv(p), ops).cache()
    m = dc._last_outcome.metrics
    assert m["cache"] == "host"
    assert "device join table" in m["cache_reason"]
    assert dc.collect() == ref["output"]


def test_default_options_above_the_embedded_limit():
    build, left = JP.big_build(), JP.big_left()
    assert len(build) == 65537
    ops = [JP.jop(build, rcols=JP.BIG_RCOLS)]
    ds = apply_ops(_ctx().parallelize(left, columns=JP.LCOLS), ops)
    got = ds.collect()
    o = ds._last_outcome
    assert o.mode == "gpu", o.fallback_reason
    assert o.metrics["join_table"] == "device"
    ref = pyoracle.run_pipeline(left, ops, columns=JP.LCOLS)
    assert got == ref["output"]
    assert 0 < len(got) < len(left)
    assert ds.exception_counts == ref["exception_counts"]


def test_one_stage_handle_two_tables():
    from tuplex_amd.engine import GpuLib
    left = JP.big_left()[:4000]
    ctx = _ctx("device")
    results, sizes = [], []
    for seed in (1, 2):
        build = [(i * 3 * seed - 600, "n%d-%d" % (seed, i))
                 for i in range(700)]
        ops = [JP.jop(build, rcols=JP.BIG_RCOLS)]
        ds = apply_ops(ctx.parallelize(left, columns=JP.LCOLS), ops)
        got = ds.collect()
        assert ds._last_outcome.mode == "gpu"
        assert ds._last_outcome.metrics["join_table"] == "device"
        assert got == pyoracle.run_pipeline(left, ops,
                                            columns=JP.LCOLS)["output"]
        assert got
        results.append(got)
        sizes.append(len(GpuLib.get()._stage_cache))
    assert results[0] != results[1]
    assert sizes[0] == sizes[1]  # the second run compiled no stage


def test_table_byte_cap_takes_the_interpreter_path():
    env = dict(os.environ, TPX_TABLE_MAX_BYTES="300")
    r = subprocess.run([sys.executable, "-m", "tests.join_table_pipelines",
                        "cap"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       check=True, timeout=300)
    res = json.loads(r.stdout.decode().strip().split("\n")[-1])
    assert res["cap"] == "300"
    assert res["mode"] == "fallback"
    assert "join table allocation" in res["reason"]
    left = JP.left_rows()
    ops = [JP.jop(JP.build_side(), "left")]
    ref = pyoracle.run_pipeline(left, ops, columns=JP.LCOLS)
    assert [tuple(x) for x in res["rows"]] == ref["output"]
    assert res["exc"] == ref["exception_counts"]

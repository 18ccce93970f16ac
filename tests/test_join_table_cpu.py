"""Device join tables, the parts that need no GPU: where plan.build_stage
puts a join's build side under tuplex.gpu.joinTable = auto / embedded /
device, what the generated source of a device join depends on (the schema,
never the contents), that default options leave existing join stages' sources
alone, and that ineligible joins keep the reasons they give today."""
import numpy as np

from tests import join_table_pipelines as JP
from tests.test_join import _jop
from tuplex_amd import codegen, jointab, plan
from tuplex_amd import ttypes as T
from tuplex_amd.options import Options

LT = [T.I64, T.STR]
LC = ["key", "val"]
RC = ["k", "name"]


def _rows(n, seed=1):
    return [(i * 7 + seed, "n%d" % (i * seed)) for i in range(n)]


def test_large_build_side_compiles_under_auto_only():
    big = _rows(70000)
    sp = plan.build_stage(LT, LC, [JP.jop(big, rcols=RC)])
    assert sp.compilable, sp.why_not_compilable
    assert [op.join_dev["index"] for op in sp.device_joins] == [0]
    spa = plan.build_stage(LT, LC, [JP.jop(big, rcols=RC)], join_table="auto")
    assert spa.compilable and len(spa.device_joins) == 1
    spe = plan.build_stage(LT, LC, [JP.jop(big, rcols=RC)],
                           join_table="embedded")
    assert not spe.compilable
    assert "too large" in spe.why_not_compilable
    assert not spe.device_joins


def test_device_source_depends_on_schema_only_and_compiles():
    srcs = []
    for n, seed in ((3, 1), (300, 5)):
        sp = plan.build_stage(LT, LC, [JP.jop(_rows(n, seed), rcols=RC)],
                              join_table="device")
        assert sp.compilable, sp.why_not_compilable
        srcs.append(codegen.generate_stage(sp, source="mem", sink="mem"))
    assert srcs[0] == srcs[1]
    src, desc = srcs[0]
    assert "__device__ TpxJoinTab tpx_jt[1];" in src
    assert "tpx_join_probe_i64(tpx_jt[0]" in src
    assert "n299" not in src and "jt1_key" not in src
    from tuplex_amd.engine import GpuLib
    glib = GpuLib.get()
    st = glib.lib.tpx_stage_compile(src.encode(), desc.encode(), b"", 1)
    assert st, glib.err()
    glib.lib.tpx_stage_free(st)
    # a column that can be null is part of the schema
    rows = _rows(3)
    rows[1] = (rows[1][0], None)
    spn = plan.build_stage(LT, LC, [JP.jop(rows, rcols=RC)],
                           join_table="device")
    assert codegen.generate_stage(spn)[0] != src


def test_default_options_leave_existing_join_sources_alone():
    header_mark = codegen.join_header().split("\n")[0]
    sp = plan.build_stage(LT, LC, [_jop()])
    src, _ = codegen.generate_stage(sp, source="mem", sink="mem")
    right = [("BOS", "Boston"), ("NYC", "New York")]
    op = ("join", right, ["code", "city"], "ap", "code", "inner",
          "", "", "", "")
    sps = plan.build_stage([T.STR, T.I64], ["ap", "n"], [op])
    srcs, _ = codegen.generate_stage(sps, source="mem", sink="mem")
    for s, p in ((src, sp), (srcs, sps)):
        assert not p.device_joins
        assert "tpx_jt" not in s and "TpxJoinTab" not in s
        assert header_mark not in s and "tpx_join_probe" not in s
    assert plan.join_table_mode(Options()) == "auto"
    # embedded and auto agree byte for byte below the limit
    spe = plan.build_stage(LT, LC, [_jop()], join_table="embedded")
    assert codegen.generate_stage(spe)[0] == src


def test_ineligible_joins_keep_their_reasons():
    def post(x):
        return (x[0], x[2])

    dup = [(1, "a"), (1, "b"), (2, "c")]
    for mode in plan.JOIN_TABLE_MODES:
        spm = plan.build_stage(LT, LC, [JP.jop(dup, rcols=RC), ("map", post)],
                               join_table=mode)
        assert not spm.compilable
        assert "duplicate" in spm.why_not_compilable
        # terminal 1:N joins stay on the embedded table
        spt = plan.build_stage(LT, LC, [JP.jop(dup, rcols=RC)],
                               join_table=mode)
        assert spt.compilable and not spt.device_joins
        assert getattr(spt.ops[-1], "join_dup", False)
        fk = [(1.5, "a"), (2.5, "b")]
        spf = plan.build_stage([T.F64, T.STR], LC, [JP.jop(fk, rcols=RC)],
                               join_table=mode)
        assert not spf.compilable
        assert "join key type" in spf.why_not_compilable
    # the in-process multi-device pool keeps the embedded table, with the
    # embedded table's reason above its limit
    for v in ("device", "auto"):
        o = Options({"tuplex.gpu.devices": 2, "tuplex.gpu.joinTable": v})
        assert plan.join_table_mode(o) == "embedded"
    spd = plan.build_stage(LT, LC, [JP.jop(_rows(70000), rcols=RC)],
                           join_table=plan.join_table_mode(o))
    assert not spd.compilable and "too large" in spd.why_not_compilable
    assert plan.join_table_mode(
        Options({"tuplex.gpu.joinTable": "device"})) == "device"


def test_pack_columns_layout():
    rows = JP.build_side(9)
    sp = plan.build_stage([T.opt(T.I64), T.STR], LC, [JP.jop(rows)],
                          join_table="device")
    jd = sp.device_joins[0].join_dev
    assert not jd["key_str"]
    assert jd["cols"] == [(1, "i64", True), (2, "f64", True),
                          (3, "bool", True), (4, "str", True)]
    slots = jointab.pack_columns(rows, len(JP.RCOLS), 0, jd)
    assert len(slots) == 15
    assert slots[0].dtype == np.int64 and slots[0].tolist() == \
        [r[0] for r in rows]
    assert slots[1] is None and slots[2] is None
    for j, dt in ((1, np.int64), (2, np.float64), (3, np.uint8)):
        vals, mask = slots[3 * j], slots[3 * j + 2]
        assert vals.dtype == dt and mask.dtype == np.uint8
        for i, r in enumerate(rows):
            assert bool(mask[i]) == (r[j] is None)
            if r[j] is not None:
                assert vals[i].tobytes() == np.array(r[j], dtype=dt).tobytes()
    offs, data, mask = slots[12], slots[13], slots[14]
    assert offs.dtype == np.int64 and len(offs) == len(rows) + 1
    for i, r in enumerate(rows):
        cell = data[offs[i]:offs[i + 1]].tobytes().decode()
        assert cell == ("" if r[4] is None else r[4])
        assert bool(mask[i]) == (r[4] is None)


def test_test_stages_generate():
    """The stages the GPU tests run all lower to device joins (and the csv
    one takes the fused csv sink)."""
    st = JP.stages()
    assert all("tpx_jt[0]" in src for src, _ in st[:-1])
    assert "tpx_jt" not in st[-1][0]
    assert "fusedcsv=1" in st[2][1]
    assert "tpx_join_probe_str" in st[2][0]

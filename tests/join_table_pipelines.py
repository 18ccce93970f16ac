"""Pipelines of the device join table tests (tests/test_gpu_join_table.py,
tests/test_join_table_cpu.py), at module level so that the build step can
precompile exactly the stages the GPU tests run.

`python -m tests.join_table_pipelines cap` is the fresh child process of the
TPX_TABLE_MAX_BYTES test: the cap is read once per process."""
import json
import os
import random
import sys

N_LEFT = 3000
N_BUILD = 257
BIG_BUILD = 65537
BIG_LEFT = 20000
LCOLS = ["key", "val"]
RCOLS = ["k", "fi", "ff", "fb", "fs"]


def build_side(n=N_BUILD, seed=1):
    """n rows (k i64 unique | fi i64? | ff f64? | fb bool? | fs str?)."""
    rng = random.Random(seed)
    keys = [0, -1, 7] + rng.sample(range(-5000, 5000), n + 3)
    keys = list(dict.fromkeys(keys))[:n]
    strs = ["", "x", "Zürich", "日本", "a,b", 'q"t', "long " * 20]
    floats = [0.0, -0.0, 1.5, -2.25e-300, 1.7976931348623157e308, 1e-5, 3.0]
    rows = []
    for i, k in enumerate(keys):
        rows.append((k,
                     None if i % 5 == 1 else rng.randint(-10 ** 12, 10 ** 12),
                     None if i % 7 == 2 else rng.choice(floats) * (seed + i % 3),
                     None if i % 4 == 3 else bool((i + seed) & 1),
                     None if i % 6 == 4 else rng.choice(strs) + str(i * seed)))
    return rows


def left_rows(n=N_LEFT, seed=2):
    """(key Option[i64], val str): 40 % None keys, about half of the rest
    hit build_side()."""
    rng = random.Random(seed)
    return [(None if rng.random() < 0.4 else rng.randint(-6000, 6000),
             "v%d" % i) for i in range(n)]


def jop(rrows, how="inner", rcols=None, lk="key", rk="k"):
    return ("join", rrows, rcols or RCOLS, lk, rk, how, "", "", "", "")


# ---- csv source, string key, csv sink ------------------------------------------

CODES = ["BOS", "JFK", "LAX", "ORD", "SEA", "SFO", "Zürich", "日本"]
DIM_COLS = ["code", "city", "rank", "hub"]


def dim_rows(seed=1):
    codes = CODES + ["K%03d" % i for i in range(N_BUILD - len(CODES))]
    return [(c, None if i % 5 == 2 else "City-%s-%d" % (c, i * seed),
             i * 10 - 7 * seed, bool((i + seed) & 1))
            for i, c in enumerate(codes)]


def csv_bytes(n=N_LEFT, seed=3):
    rng = random.Random(seed)
    codes = CODES + ["K%03d" % i for i in range(0, N_BUILD - len(CODES), 3)] \
        + ["XXX", "K", "BO"]
    lines = [b"ap,delay"]
    for _ in range(n):
        lines.append(b"%s,%d" % (rng.choice(codes).encode(),
                                 rng.randint(-10, 500)))
    return b"\n".join(lines) + b"\n"


def late(x):
    return x["delay"] > 60


def ranked(x):
    return x["rank"] % 3 != 0


def csv_ops(dim):
    return [("filter", late),
            ("join", dim, DIM_COLS, "ap", "code", "inner", "", "", "", ""),
            ("filter", ranked),
            ("selectColumns", ["ap", "city", "delay", "hub"])]


def csv_left_ops(dim):
    return [("join", dim, DIM_COLS, "ap", "code", "left", "", "", "", ""),
            ("selectColumns", ["delay", "city", "rank", "ap"])]


# ---- above the embedded table's limit --------------------------------------------

def big_build():
    return [(i * 3 - 50000, "name-%d" % i) for i in range(BIG_BUILD)]


def big_left():
    rng = random.Random(5)
    return [(rng.randint(-60000, 160000), "v%d" % i) for i in range(BIG_LEFT)]


BIG_RCOLS = ["k", "name"]


# ---- precompile -------------------------------------------------------------------

def mem_stage(data, columns, ops, join_table):
    """(src, desc) of the stage engine.run_collect builds for a parallelize
    source under default thresholds."""
    from tuplex_amd import codegen, plan
    from tuplex_amd import ttypes as T
    from tuplex_amd.options import Options
    maj = T.infer_majority_type(
        data, optional_threshold=Options().optional_threshold)
    types = list(T.tuple_params(T.row_type_of(maj)))
    sp = plan.build_stage(types, columns, ops, join_table=join_table)
    assert sp.compilable, sp.why_not_compilable
    assert bool(sp.device_joins) == (join_table == "device")
    return codegen.generate_stage(sp, source="mem", sink="mem")


def csv_stage(data, ops, join_table, sink):
    """(src, desc) of the stage csvio.run_csv builds for csv bytes `data`."""
    from tuplex_amd import codegen, csvio, plan
    from tuplex_amd.options import Options
    sample = data[:256 << 10]
    sample = sample[:sample.rfind(b"\n") + 1]
    delim = csvio.sniff_delimiter(sample)
    _hh, names, types = csvio.sniff(sample, [""],
                                    Options().normalcase_threshold, None,
                                    None, delim)
    sp = plan.build_stage(types, names, ops, join_table=join_table)
    assert sp.compilable, sp.why_not_compilable
    assert sp.device_joins
    return codegen.generate_stage(
        sp, source="csv", sink=sink,
        csv_info={"null_values": [""], "delimiter": delim.decode(),
                  "text_mode": False})


def small_build():
    """A build side the embedded table takes under default options."""
    return [(i * 5 - 300, "s%d" % i) for i in range(300)]


def stages():
    """The device join stages of the GPU tests, then the embedded one."""
    left = left_rows()
    out = []
    for how in ("inner", "left"):
        out.append(mem_stage(left, LCOLS, [jop(build_side(), how)], "device"))
    data = csv_bytes()
    out.append(csv_stage(data, csv_ops(dim_rows()), "device", "csv"))
    out.append(csv_stage(data, csv_left_ops(dim_rows()), "device", "mem"))
    small = [(1, "a"), (2, "b"), (3, "c")]
    out.append(mem_stage(big_left()[:100], LCOLS,
                         [jop(small, rcols=BIG_RCOLS)], "device"))
    out.append(mem_stage(left_rows(500), LCOLS,
                         [jop(small_build(), rcols=BIG_RCOLS)], "auto"))
    return out


def precompile(verbose=False):
    from tests import pipelines
    from tuplex_amd import engine
    glib = engine.GpuLib.get()
    n = 0
    for src, desc in stages():
        pipelines._stage_compile(glib, src, desc)
        n += 1
    if verbose:
        print("precompiled %d device join table test stages" % n)
    return n


# ---- child process of the byte-cap test -------------------------------------------

def _cap_child():
    import tuplex_amd
    from tests.pipelines import apply_ops
    left = left_rows()
    ops = [jop(build_side(), "left")]
    ctx = tuplex_amd.Context({"tuplex.gpu.joinTable": "device"})
    ds = apply_ops(ctx.parallelize(left, columns=LCOLS), ops)
    got = ds.collect()
    o = ds._last_outcome
    print(json.dumps({"mode": o.mode, "reason": o.fallback_reason,
                      "rows": got, "exc": ds.exception_counts,
                      "cap": os.environ.get("TPX_TABLE_MAX_BYTES")}))


if __name__ == "__main__":
    if sys.argv[1:] == ["cap"]:
        _cap_child()
    else:
        sys.exit("usage: python -m tests.join_table_pipelines cap")

"""The csv input and pipelines of tests/test_gpu_device_cache.py, and their
precompile(): every stage those tests run — stage 1 over the csv source, the
uncached pipelines, and the second stages over the columnar cache — is
hipRTC-compiled (compile only, no GPU needed) into the in-tree code-object
cache by build(), so the suite never compiles on the GPU machine.

Every UDF sits on a line that is a whole statement: the UDF compiler reads a
lambda's source line on its own. Every post-cache shape reads the column the
cached stage adds ("q")."""
import os
import typing

HINTS = {"note": typing.Optional[str]}
N_DIRTY = 3000


def write_csv(path, n, dirty=True):
    """two ints, a float, a bool-like column, two ~40-byte strings (some
    quoted, with commas), an Option-str column with empty cells; with `dirty`
    a few rows that stage 1 diverts and the interpreter resolves ('+5', a
    non-ASCII cell), a few that stay exceptions ('notanint') and a few zero
    divisors."""
    with open(path, "w", encoding="utf-8") as f:
        f.write("a,b,amount,flag,s1,s2,note\n")
        for i in range(n):
            a, b = str(i), str(i % 7 + 1)
            s1 = "%d Evergreen Terrace, block %04d of the ward" % (i, i % 97)
            s2 = "unit %05d on the north side of the river" % (i * 3)
            if dirty:
                if i % 501 == 7:
                    a = "+5"
                elif i % 503 == 11:
                    s2 = "café %d at the corner of the old square" % i
                elif i % 701 == 13:
                    a = "notanint"
                elif i % 997 == 17:
                    b = "0"
            if i % 3 == 0:
                s1 = '"%s"' % s1
            else:
                s1 = s1.replace(",", ";")
            note = "" if i % 4 == 0 else "n%d" % (i % 13)
            f.write("%s,%s,%s,%s,%s,%s,%s\n" % (
                a, b, repr(i * 0.25), "true" if i % 3 else "false", s1, s2,
                note))


def stage1(ctx, path):
    ds = ctx.csv(path, type_hints=HINTS)
    ds = ds.filter(lambda x: x["a"] % 11 != 3)
    ds = ds.withColumn("q", lambda x: 100 // x["b"])
    return ds


def clean_source(ctx, path):
    return ctx.csv(path, type_hints=HINTS)


def f_filter(ds):
    return ds.filter(lambda x: x["a"] % 3 == 0)


def f_map_filter(ds):
    ds = ds.map(lambda x: (x["a"] * 2, x["s1"], x["note"], x["flag"], x["q"]))
    ds = ds.filter(lambda t: t[0] % 4 == 0)
    return ds


def add(a, b):
    return a + b


def acc_a(a, x):
    return a + x["a"]


def acc_aq(a, x):
    return a + x["a"] + x["q"]


def acc_q(a, x):
    return a + x["q"]


def f_sum(ds):
    return ds.aggregate(add, acc_aq, 0)


def f_sum_by_key(ds):
    return ds.aggregateByKey(add, acc_q, 0, ["b"])


def f_raises(ds):
    return ds.map(lambda x: (x["a"], x["q"], 100 // (x["a"] % 5)))


def f_resolve(ds):
    return ds.resolve(ZeroDivisionError, lambda x: -1)


def f_ident(ds):
    return ds


def f_clean_sum(ds):
    ds = ds.filter(lambda x: x["a"] % 3 == 0)
    return ds.aggregate(add, acc_a, 0)


POSTS = [f_filter, f_map_filter, f_sum, f_sum_by_key, f_raises, f_resolve,
         f_ident]


def _csv_plan(ctx, ds):
    """(stage plan, csv_info) of a csv-source dataset, sniffed as run_csv
    sniffs it."""
    from tuplex_amd import csvio, plan
    src = ds._source
    with open(src.pattern, "rb") as f:
        sample = f.read(256 << 10)
    sample = sample[:sample.rfind(b"\n") + 1]
    delim = csvio.sniff_delimiter(sample)
    _hh, names, types = csvio.sniff(
        sample, src.null_values, ctx.options_obj.normalcase_threshold,
        src.header, src.columns, delim)
    types = csvio.apply_type_hints(types, names, src.type_hints)
    sp = plan.build_stage(types, names, ds._ops)
    assert sp.compilable, sp.why_not_compilable
    return sp, {"null_values": src.null_values, "delimiter": delim.decode(),
                "text_mode": False}


def _strip_lead(ops):
    lead = 0
    while lead < len(ops) and ops[lead][0] in ("resolve", "ignore"):
        lead += 1
    return list(ops[lead:])


def precompile(verbose=False):
    import tempfile
    import tuplex_amd
    from tests import pipelines
    from tuplex_amd import codegen, engine, plan
    from tuplex_amd.dataset import DataSet
    glib = engine.GpuLib.get()
    ctx = tuplex_amd.Context()
    n = 0
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "in.csv")
        write_csv(p, N_DIRTY)
        pc = os.path.join(d, "clean.csv")
        write_csv(pc, 2000, dirty=False)
        cached_from = []  # (stage-1 plan, second-stage builders)
        for base, posts in ((stage1(ctx, p), POSTS),
                            (clean_source(ctx, pc), [f_clean_sum])):
            chains = [base] + [post(base) for post in posts
                               if post is not f_ident]
            for k, ds in enumerate(chains):
                sp, info = _csv_plan(ctx, ds)
                src, desc = codegen.generate_stage(sp, source="csv",
                                                   sink="mem", csv_info=info)
                pipelines._stage_compile(glib, src, desc)
                n += 1
                if k == 0:
                    cached_from.append((sp, posts))
        for sp1, posts in cached_from:
            for post in posts:
                ops2 = _strip_lead(post(DataSet(ctx, None, []))._ops)
                if not ops2:
                    continue
                sp2 = plan.build_stage(list(sp1.gpu_output_types),
                                       sp1.output_columns, ops2)
                assert sp2.compilable, sp2.why_not_compilable
                src, desc = codegen.generate_stage(sp2, source="col",
                                                   sink="mem")
                pipelines._stage_compile(glib, src, desc)
                n += 1
    if verbose:
        print("precompiled %d device-cache test stages" % n)
    return n

"""Pipelines of the device slice of the scalar-runtime differential test
(test_gpu_rtops.py): one UDF per helper family, rows drawn from the host
harness's edge lists (rtops_cases.py). Kept apart from the test so the build's
precompile step can warm exactly these stage kernels."""
import math
import random

from oracle import pyoracle
from tests import rtops_cases as RC

SEED = 20241108


# ---- UDFs ---------------------------------------------------------------------------

def u_fdiv(x):
    return (x["a"] // x["b"], x["a"] % x["b"], x["a"] / x["b"])


def u_float(x):
    return (float(x["s"]), x["k"])


def u_int(x):
    return (int(x["s"]), x["k"])


def u_ifmt(x):
    return (str(x["i"]), "%05d" % x["i"], x["i"] // x["d"], x["i"] % x["d"])


def u_int_f64(x):
    return (int(x["f"]), x["k"])


def u_str(x):
    s = x["s"]
    n = x["nd"]
    return (s.find(n), s.rfind(n), n in s, s.replace(n, "c"),
            s.replace(n, ""), s.replace(n, "xyz"), s.startswith(n),
            s.endswith(n))


def u_split(x):
    return (x["s"].split(x["nd"])[x["i"]], x["k"])


def u_center(x):
    return (x["s"].center(x["w"], "*"), x["s"].center(x["w"]),
            x["s"] * x["r"])


def u_f64(x):
    return (x["k"], x["v"])


# ---- rows ---------------------------------------------------------------------------

def _fill(rows, n, rng):
    """Repeat the edge rows (shuffled) up to n rows: the edge list is never cut."""
    out = list(rows)
    while len(out) < n:
        out.append(rows[rng.randrange(len(rows))])
    return out


def fdiv_rows():
    rng = random.Random(SEED)
    pairs, n_div, n_mod = RC.decimal_pairs(rng, 120000, 1200)
    pairs = pairs[:n_div][:400] + pairs[n_div:n_div + n_mod][:400] + \
        pairs[n_div + n_mod:]
    special = [(a, b) for a in RC.FLOAT_SPECIAL for b in RC.FLOAT_SPECIAL]
    return special + pairs


def n_divergent(rows):
    return sum(1 for a, b in rows
               if b != 0.0 and math.isfinite(a) and math.isfinite(b)
               and math.isfinite(a / b) and math.floor(a / b) != a // b)


def _parse_strings(edge, fast, slow):
    """(agreed, replayed): strings where the compiled-path parser's verdict
    stands (it accepts, or CPython rejects too), and those it rejects but
    CPython accepts — the engine replays these rows in the interpreter."""
    agreed, replayed = [], []
    for s in edge:
        try:
            fast(s)
        except ValueError:
            try:
                slow(s)
            except ValueError:
                agreed.append(s)
            else:
                replayed.append(s)
        else:
            agreed.append(s)
    return agreed, replayed


def float_strings():
    rng = random.Random(SEED + 1)
    edge = RC.FLOAT_EDGE + RC.NANINF + RC.ws_wrapped(RC.FLOAT_EDGE[:40]) + \
        RC.long_mantissas(rng, 1500)
    edge = [s for s in dict.fromkeys(edge)]
    return _parse_strings(edge, pyoracle.ref_float, float)


def int_strings():
    rng = random.Random(SEED + 2)
    edge = RC.INT_EDGE + RC.ws_wrapped(RC.INT_EDGE)
    for _ in range(1200):
        edge.append(rng.choice(["", "-", "-", " "]) + "".join(
            rng.choice("0123456789") for _ in range(rng.choice(
                [1, 5, 17, 18, 19, 20, 21, 25]))))
    edge = [s for s in dict.fromkeys(edge)]
    return _parse_strings(edge, pyoracle.ref_int, int)


def keyed(strings, n):
    rng = random.Random(SEED + 3)
    return [(s, k) for k, s in enumerate(_fill(strings, n, rng))]


def ifmt_rows():
    rows = [(v, d) for v in RC.INT_FMT for d in (1, -1, 2, -2, 7, -7)]
    rows += [(a, b) for a, b in RC.I64_DIV]
    rng = random.Random(SEED + 9)
    while len(rows) < 2000:
        rows.append((rng.randint(RC.I64_MIN, RC.I64_MAX) >> rng.randrange(64),
                     rng.choice([1, -1, 2, -2, 3, 10, -10, 0, 1000003])))
    return rows


def int_f64_rows():
    rng = random.Random(SEED + 4)
    vals = list(RC.INT_F64)
    for _ in range(2000 - len(vals)):
        vals.append(rng.uniform(-1, 1) * 10.0 ** rng.randint(0, 19))
    return [(v, k) for k, v in enumerate(vals)]


def str_rows(min_len=0, n=3000):
    """(haystack, needle) at haystack lengths min_len..72, small alphabet."""
    rng = random.Random(SEED + 5)
    rows = [p for p in RC.OVERLAP if len(p[0]) >= min_len and
            len(p[1]) >= min_len]
    for ln in range(max(min_len, 0), 73):
        for v in range(max(1, (n - len(RC.OVERLAP)) // 73)):
            s = "".join(rng.choice("ab") for _ in range(ln))
            r = v % 6
            if r == 0:
                nd = s
            elif r == 1:
                nd = s + rng.choice("ab")
            elif r == 2 and s:
                a = rng.randrange(len(s))
                nd = s[a:a + rng.randint(1, 6)]
            else:
                nd = rng.choice(RC.NEEDLES)
            if len(nd) < min_len:
                nd = "a"
            rows.append((s, nd))
    return rows


def split_rows():
    rows = []
    k = 0
    for s, nd in str_rows(n=700):
        parts = len(s.split(nd)) if nd else 1
        for ix in sorted({-parts - 1, -parts, -1, 0, parts - 1, parts}):
            rows.append((s, nd, ix, k))
            k += 1
    return rows[:4000]


def center_rows():
    rng = random.Random(SEED + 6)
    rows = []
    for ln in range(73):
        s = "".join(rng.choice("abc") for _ in range(ln))
        for w in (ln - 1, ln, ln + 1, ln + 2, ln + 3, ln + 4):
            rows.append((s, w, (-1, 0, 1, 2, 3, 1)[w % 6]))
    for ln in (0, 1, 2, 7, 8, 9, 33, 72):  # the largest repeat, a few rows only
        rows.append((("abcdefgh" * 9)[:ln], ln + 1, 64))
    return _fill(rows, 2000, rng)


def str_csv_bytes():
    """The string family through the csv source: a short and a long leading
    column put the cells at arbitrary offsets of the staged row."""
    lines = [b"pre,s,nd,post"]
    for i, (s, nd) in enumerate(str_rows(min_len=1, n=2000)):
        pre = "p" * (1 + (i * 7) % 23) if i % 2 else "p"
        lines.append(("%s,%s,%s,%d" % (pre, s, nd, i)).encode())
    return b"\n".join(lines) + b"\n"


def f64_csv_bytes():
    """An f64 column whose cells parse EXACTLY (integer mantissa over a power
    of ten <= 10^22: one correctly-rounded division): sixth-decimal ties,
    signed zero, both sides of the %f accept limit, nan/inf."""
    cells = ["0.0", "-0.0", "0", "5e-7", "15e-7", "25e-7", "-5e-7", "1e-7",
             "4e-7", "6e-7", "1.5", "-2.25", "123456789.125", "nan", "inf",
             "-1e300", "1e13", "2e13",
             "922337203685477e-2", "-922337203685477e-2",   # largest 2-decimal
             "922337203685478e-2", "-922337203685478e-2",   # just past 2^63e-6
             "9223372036854.5", "9223372036855.0", "9.2e12", "9.3e12"]
    for k in range(1, 800, 2):  # (2k+1)/128 == (2k+1)*78125e-7: exact ties
        cells.append("%de-7" % (k * 78125))
        cells.append("-%de-7" % (k * 78125))
    rng = random.Random(SEED + 8)
    while len(cells) < 2000:
        cells.append("%de-%d" % (rng.randint(-10**15, 10**15),
                                 rng.randint(0, 12)))
    lines = [b"k,v"] + [("%d,%s" % (i, c)).encode()
                        for i, c in enumerate(cells)]
    return b"\n".join(lines) + b"\n"


MEM = [
    ("rt_fdiv", fdiv_rows, ["a", "b"], u_fdiv),
    ("rt_float", lambda: keyed(float_strings()[0], 3000), ["s", "k"], u_float),
    ("rt_int", lambda: keyed(int_strings()[0], 2500), ["s", "k"], u_int),
    ("rt_ifmt", ifmt_rows, ["i", "d"], u_ifmt),
    ("rt_int_f64", int_f64_rows, ["f", "k"], u_int_f64),
    ("rt_str", str_rows, ["s", "nd"], u_str),
    ("rt_split", split_rows, ["s", "nd", "i", "k"], u_split),
    ("rt_center", center_rows, ["s", "w", "r"], u_center),
]
CSV = [
    ("rt_str_csv", str_csv_bytes, u_str, ("mem",)),
    ("rt_f64_csv", f64_csv_bytes, u_f64, ("csv",)),
]


def precompile(glib, stage_compile):
    """Compile-only pass over the exact stage sources the GPU tests run."""
    from tuplex_amd import codegen, csvio, plan
    from tuplex_amd import ttypes as T
    from tuplex_amd.options import Options
    opts = Options()
    n = 0
    for _name, rows, cols, fn in MEM:
        maj = T.infer_majority_type(rows(),
                                    optional_threshold=opts.optional_threshold)
        sp = plan.build_stage(list(T.tuple_params(T.row_type_of(maj))), cols,
                              [("map", fn)])
        assert sp.compilable, (_name, sp.why_not_compilable)
        src, desc = codegen.generate_stage(sp, source="mem", sink="mem")
        stage_compile(glib, src, desc)
        n += 1
    for _name, mk, fn, sinks in CSV:
        data = mk()
        _h, names, col_types = csvio.sniff(data[:1 << 20], [""], 0.9, None,
                                           None, b",")
        sp = plan.build_stage(col_types, names, [("map", fn)])
        assert sp.compilable, (_name, sp.why_not_compilable)
        for sink in sinks:
            src, desc = codegen.generate_stage(
                sp, source="csv", sink=sink,
                csv_info={"null_values": [""], "delimiter": ","})
            stage_compile(glib, src, desc)
            n += 1
    return n

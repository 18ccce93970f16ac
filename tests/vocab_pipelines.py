"""UDFs, rows and the build hook for the UDF-vocabulary tests (truthiness,
constant `in`, str.format / multi-directive %, string.capwords): the CPU compile
checks (test_vocab_compile.py, test_vocab_hipcc.py) and the device tests
(test_gpu_vocab.py) share them, and precompile() warms exactly the stage
kernels the device tests run."""
import random
import string

SEED = 20260311

I64_MAX = (1 << 63) - 1
I64_MIN = -(1 << 63)


# ---- edge values (also the host harness's vectors, test_host_fmt.py) ----------

def edge_ints():
    vals = [0, 1, -1, 9, -9, 10, -10]
    for k in range(1, 19):
        for v in (10 ** k, 10 ** k - 1):
            vals += [v, -v]
    vals += [I64_MAX, I64_MIN]
    return list(dict.fromkeys(vals))


def edge_strings():
    alpha = "abcdefghijklmnopqrstuvwxyz0123456789 -_"
    rng = random.Random(SEED)
    out = ["".join(rng.choice(alpha) for _ in range(n)) for n in range(18)]
    out.append("".join(rng.choice(alpha) for _ in range(300)))
    return out


NON_ASCII = ["café", "über alles", "naïve  words", "東京"]

SPLIT_WS = "\t\n\x0b\x0c\r\x1c\x1d\x1e\x1f "


def capwords_strings():
    out = ["", " ", "a", "a b", " a", "a ", "a  b", "  lead and trail  ",
           "mIxEd cAsE wOrDs", "x y z", "1st place", "-dash -Dash", "(paren) [b]",
           "ALL UPPER", "all lower", "new york, ny", 'say "hi" town',
           "tab\tsep", "nl\nsep", "a\x1cb\x1dc\x1ed\x1fe", SPLIT_WS,
           "o'neil mc-donald", "q" * 40 + " " + "R" * 40]
    for c in SPLIT_WS:
        out += [c, "a" + c + "b", c * 3, "a" + c * 2 + "b" + c, c + "word"]
    rng = random.Random(SEED + 1)
    out.append(" ".join("".join(rng.choice("abcXYZ9-") for _ in range(
        rng.randint(1, 9))) for _ in range(600))[:3000])
    return out


# ---- truthiness ---------------------------------------------------------------------

def t_int_or_zero(x):
    return int(x) if x else 0


def t_guarded_div(x):
    return 10 // x if x else -1


def t_str_upper(x):
    if x:
        return x.upper()
    return "<empty>"


def t_f64_flag(x):
    if x:
        return 1
    return 0


def t_not(x):
    return not x


def t_bool_ops(x):
    if x["a"] and not x["s"]:
        return "a only"
    elif x["s"] or x["f"]:
        return "s or f"
    return "none"


def _opt_rows(values, n, seed):
    """`values` and None (about 45 %: the column types as Option) up to n rows."""
    rng = random.Random(seed)
    out = []
    for v in values:
        out += [v, None]
    while len(out) < n:
        out.append(None if rng.random() < 0.45 else rng.choice(values))
    return out


def opt_f64_rows():
    return _opt_rows([0.0, -0.0, float("nan"), 1.5, -2.75, 1e10, 0.25, 7.0],
                     64 * 9 + 1, SEED + 2)


def opt_i64_rows():
    return _opt_rows([0, 1, -1, 3, -3, 10, 11, I64_MAX, I64_MIN], 64 * 9 - 1,
                     SEED + 3)


def opt_str_rows():
    return _opt_rows(["", "a", " ", "word", "Two Words", "0"], 64 * 7 + 1,
                     SEED + 4)


def f64_rows():
    rng = random.Random(SEED + 5)
    vals = [0.0, -0.0, float("nan"), float("inf"), 5e-324, -1.0, 2.5]
    return [rng.choice(vals) for _ in range(64 * 8 - 1)]


def bool_ops_rows():
    a, s, f = opt_i64_rows(), opt_str_rows(), f64_rows()
    n = min(len(a), len(s), len(f))
    return [(a[i], s[(i * 7) % len(s)], f[(i * 3) % len(f)]) for i in range(n)]


# ---- format / % ---------------------------------------------------------------------

def f_ints(x):
    i = x["i"]
    return ("{}|{:5}|{:05}|{:022d}|{:d}".format(i, i, i, i, i),
            "%d:%7d:%022d:%s:%-6s|%%" % (i, i, i, i, i),
            "{1}{0:3}{1}".format(i, x["b"]),
            "%s %d" % (x["b"], x["b"]))


def f_strs(x):
    s = x["s"]
    return ("[{:>20}][{:<20}][{:7}][{}]".format(s, s, s, s),
            "%12s|%-12s|%s|%3s" % (s, s, s, s),
            "{:120}{:>121}{{{}}}".format(s, s, x["k"]),
            "{0}{0}".format(s))


def f_plain(x):
    return ("<{}>".format(x["s"]), "%s=%s" % (x["s"], x["k"]))


def f_opt(x):
    return "{}/{}".format(x, x)


def f_opt_spec(x):
    return "{:03}/{}".format(x, x)


def int_rows():
    rng = random.Random(SEED + 6)
    rows = [(v, i % 3 == 0) for i, v in enumerate(edge_ints())]
    while len(rows) < 64 * 5 + 1:
        rows.append((rng.randint(I64_MIN, I64_MAX) >> rng.randrange(64),
                     rng.random() < 0.5))
    return rows


def str_rows():
    rng = random.Random(SEED + 7)
    base = edge_strings()
    rows = [(s, k) for k, s in enumerate(base)]
    while len(rows) < 64 * 4 - 1:
        rows.append((base[rng.randrange(len(base) - 1)], len(rows)))
    return rows


def non_ascii_rows():
    rows = [(s, k) for k, s in enumerate(NON_ASCII + edge_strings()[:8])]
    return rows * 5 + rows[:5]  # 65 rows


# ---- capwords -----------------------------------------------------------------------

def c_cap(x):
    return (string.capwords(x["s"]), x["k"])


def cap_rows():
    rng = random.Random(SEED + 8)
    base = capwords_strings() + NON_ASCII
    rows = list(base)
    while len(rows) < 64 * 5 - 1:
        rows.append(base[rng.randrange(len(base) - 5)])  # the long one once
    return [(s, k) for k, s in enumerate(rows)]


# ---- membership ---------------------------------------------------------------------

MODES = ["AIR", "AIR REG", "RAIL", "TRUCK", "MAIL", "SHIP", "air", "AIR "]


def m_in(x):
    return (x["s"] in ["AIR", "AIR REG", "RAIL", "TRUCK"],
            x["s"] not in ("AIR", "MAIL"),
            x["n"] in [1, 5, 11, -3],
            x["n"] not in (0, 3))


def member_rows():
    s = _opt_rows(MODES, 64 * 6 + 1, SEED + 9)
    n = _opt_rows([0, 1, 2, 3, 5, 11, -3, 12], 64 * 6 + 1, SEED + 10)
    return list(zip(s, n))


# ---- one stage with all four additions (test_vocab_hipcc.py) ------------------------

def all_four(x):
    tag = "{:04}-{}".format(x["n"], x["code"]) if x["n"] else "none"
    name = string.capwords(x["name"]) if x["name"] else "?"
    return (tag, name, 1 if x["f"] else 0,
            x["mode"] in ["AIR", "AIR REG", "RAIL", "TRUCK"], x["k"])


ALL_FOUR_COLS = ["n", "name", "f", "k", "code", "mode"]


def all_four_types():
    from tuplex_amd import ttypes as T
    return [T.opt(T.I64), T.opt(T.STR), T.F64, T.I64, T.STR, T.STR]


# ---- flights-shaped csv -------------------------------------------------------------

FL_COLS = ["carrier_name", "crs_dep_time", "dep_delay", "cancellation_code",
           "diverted", "origin_city", "year", "defunct_year"]

_CARRIERS = ["delta air lines inc.", "SOUTHWEST AIRLINES CO.",
             "Pan American World Airways (1)", "jetBlue airways",
             "trans world airways llc"]
_CITIES = ["new york", "SAN FRANCISCO", "st. louis", "fort  worth",
           " salt lake city ", "o'hare field", "washington, dc",
           'the "windy" city', "x"]


def fl_dep_time(x):
    return "{:02}:{:02}".format(int(x["crs_dep_time"] / 100),
                                x["crs_dep_time"] % 100)


def fl_delay(x):
    return int(x) if x else 0


def fl_status(row):
    if row["diverted"]:
        return "diverted"
    else:
        if row["cancellation_code"]:
            c = row["cancellation_code"]
            if c == "A":
                return "carrier"
            elif c == "B":
                return "weather"
            elif c == "C":
                return "national air system"
            elif c == "D":
                return "security"
            return "other"
        else:
            return "None"


def fl_city(x):
    return string.capwords(x) if x else None


def fl_still_flying(row):
    if row["defunct_year"]:
        return int(row["year"]) < int(row["defunct_year"])
    return True


def fl_label(x):
    return "%s, %4d" % (x["carrier_name"], x["year"])


def fl_out(x):
    return (x["label"], x["dep_time"], x["dep_delay"], x["status"],
            x["origin_city"], x["year"])


def flights_vocab_ops():
    return [
        ("withColumn", "dep_time", fl_dep_time),
        ("mapColumn", "dep_delay", fl_delay),
        ("withColumn", "status", fl_status),
        ("mapColumn", "origin_city", fl_city),
        ("filter", fl_still_flying),
        ("withColumn", "label", fl_label),
        ("map", fl_out),
    ]


def make_flights_vocab_csv(n, seed=SEED + 11, bad_frac=0.01):
    rng = random.Random(seed)
    lines = [",".join(FL_COLS)]

    def q(s):
        if any(c in s for c in ',"'):
            return '"' + s.replace('"', '""') + '"'
        return s

    for _ in range(n):
        year = rng.randint(1987, 2020)
        cells = [
            q(rng.choice(_CARRIERS)),
            str(rng.randint(0, 23) * 100 + rng.randint(0, 59)),
            "" if rng.random() < 0.2 else "%.1f" % rng.choice(
                [0.0, -4.0, 12.0, 75.5, 240.0]),
            rng.choice(["", "", "", "A", "B", "C", "D", "E"]),
            rng.choice(["0.0", "0.0", "0.0", "1.0"]),
            q(rng.choice(_CITIES)),
            str(year),
            "" if rng.random() < 0.6 else str(rng.randint(1990, 2015)),
        ]
        if rng.random() < bad_frac:
            if rng.random() < 0.5:
                cells = cells[:rng.randint(2, 7)]
            else:
                cells[1] = "late"
        lines.append(",".join(cells))
    return ("\n".join(lines) + "\n").encode()


# ---- build hook ---------------------------------------------------------------------

MEM = [
    ("t_int_or_zero", opt_f64_rows, None, t_int_or_zero),
    ("t_guarded_div", opt_i64_rows, None, t_guarded_div),
    ("t_str_upper", opt_str_rows, None, t_str_upper),
    ("t_f64_flag", f64_rows, None, t_f64_flag),
    ("t_not", opt_i64_rows, None, t_not),
    ("t_bool_ops", bool_ops_rows, ["a", "s", "f"], t_bool_ops),
    ("f_ints", int_rows, ["i", "b"], f_ints),
    ("f_strs", str_rows, ["s", "k"], f_strs),
    ("f_strs_non_ascii", non_ascii_rows, ["s", "k"], f_strs),
    ("f_plain_non_ascii", non_ascii_rows, ["s", "k"], f_plain),
    ("f_opt", opt_i64_rows, None, f_opt),
    ("f_opt_spec", opt_i64_rows, None, f_opt_spec),
    ("c_cap", cap_rows, ["s", "k"], c_cap),
    ("m_in", member_rows, ["s", "n"], m_in),
]

FLIGHTS_ROWS = 64 * 40 + 1


def mem_stage(name):
    """(rows, columns, fn, StageProgram) of a MEM entry, typed like the engine
    types a parallelize() of those rows."""
    from tuplex_amd import plan
    from tuplex_amd import ttypes as T
    from tuplex_amd.options import Options
    _n, rows, cols, fn = [m for m in MEM if m[0] == name][0]
    data = rows()
    maj = T.infer_majority_type(
        data, optional_threshold=Options().optional_threshold)
    sp = plan.build_stage(list(T.tuple_params(T.row_type_of(maj))), cols,
                          [("map", fn)])
    return data, cols, fn, sp


def flights_stage():
    from tuplex_amd import csvio, plan
    data = make_flights_vocab_csv(FLIGHTS_ROWS)
    _h, names, col_types = csvio.sniff(data[:1 << 20], [""], 0.9, None, None,
                                       b",")
    return data, plan.build_stage(col_types, names, flights_vocab_ops())


def generate_sources():
    """(name, source, desc) of every stage the device tests run."""
    from tuplex_amd import codegen
    out = []
    seen = set()
    for name, _rows, _cols, _fn in MEM:
        _d, _c, _f, sp = mem_stage(name)
        assert sp.compilable, (name, sp.why_not_compilable)
        src, desc = codegen.generate_stage(sp, source="mem", sink="mem")
        if src not in seen:
            seen.add(src)
            out.append((name, src, desc))
    _data, sp = flights_stage()
    assert sp.compilable, sp.why_not_compilable
    for sink in ("mem", "csv"):
        src, desc = codegen.generate_stage(
            sp, source="csv", sink=sink,
            csv_info={"null_values": [""], "delimiter": ","})
        out.append(("flights_vocab_" + sink, src, desc))
    return out


def precompile(verbose=False):
    from tests import pipelines
    from tuplex_amd import engine
    glib = engine.GpuLib.get()
    n = 0
    for name, src, desc in generate_sources():
        pipelines._stage_compile(glib, src, desc)
        n += 1
        if verbose:
            print("precompiled vocab:", name)
    return n

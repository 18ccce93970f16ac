"""TEST INFRASTRUCTURE: UDFs, data makers and the build-time precompile hook of
the regex pipelines (the default `--pipeline_type regex` form of the logs
workload: one nine-group Common-Log pattern, or nine withColumn UDFs with one
pattern each). Dict-literal map returns are written as tuples: the oracle's
map drops column names.

precompile() generates the exact stage sources tests/test_gpu_regex.py runs, so
a fresh checkout never cold-compiles during the suite and the CPU-only build
cross-compiles the regex VM for gfx950.
"""
import random
import re


# ---- the ten logs UDFs --------------------------------------------------------

def ParseWithRegex(logline):
    match = re.search(r'^(\S+) (\S+) (\S+) \[([\w:/]+\s[+\-]\d{4})\] "(\S+) (\S+)\s*(\S*)\s*" (\d{3}) (\S+)', logline)
    if match:
        return (match[1], match[2], match[3], match[4], match[5], match[6],
                match[7], int(match[8]),
                0 if match[9] == '-' else int(match[9]))
    else:
        return ('', '', '', '', '', '', '', -1, -1)


def endpoint_nonempty(x):
    return len(x[5]) > 0


def extract_ip(x):
    match = re.search(r"(^\S+) ", x['logline'])
    if match:
        return match[1]
    else:
        return ''


def extract_client_id(x):
    match = re.search(r"^\S+ (\S+) ", x['logline'])
    if match:
        return match[1]
    else:
        return ''


def extract_user_id(x):
    match = re.search(r"^\S+ \S+ (\S+) ", x['logline'])
    if match:
        return match[1]
    else:
        return ''


def extract_date(x):
    match = re.search(r"^.*\[([\w:/]+\s[+\-]\d{4})\]", x['logline'])
    if match:
        return match[1]
    else:
        return ''


def extract_method(x):
    match = re.search(r'^.*"(\S+) \S+\s*\S*\s*"', x['logline'])
    if match:
        return match[1]
    else:
        return ''


def extract_endpoint(x):
    match = re.search(r'^.*"\S+ (\S+)\s*\S*\s*"', x['logline'])
    if match:
        return match[1]
    else:
        return ''


def extract_protocol(x):
    match = re.search(r'^.*"\S+ \S+\s*(\S*)\s*"', x['logline'])
    if match:
        return match[1]
    else:
        return ''


def extract_response_code(x):
    match = re.search(r'^.*" (\d{3}) ', x['logline'])
    if match:
        return int(match[1])
    else:
        return -1


def extract_content_size(x):
    match = re.search(r'^.*" \d{3} (\S+)', x['logline'])
    if match:
        return 0 if match[1] == '-' else int(match[1])
    else:
        return -1


def endpoint_col_nonempty(x):
    return len(x['endpoint']) > 0


SPLIT_UDFS = [
    ("ip", extract_ip), ("client_id", extract_client_id),
    ("user_id", extract_user_id), ("date", extract_date),
    ("method", extract_method), ("endpoint", extract_endpoint),
    ("protocol", extract_protocol),
    ("response_code", extract_response_code),
    ("content_size", extract_content_size),
]

LOG_UDFS = [ParseWithRegex] + [f for _, f in SPLIT_UDFS]


def regex_ops():
    return [("map", ParseWithRegex), ("filter", endpoint_nonempty)]


def split_regex_ops():
    return [("withColumn", c, f) for c, f in SPLIT_UDFS] + \
        [("filter", endpoint_col_nonempty)]


def ParseWithStripTuple(x):
    """The find/slice parser of the logs workload, returning a tuple."""
    y = x
    i = y.find(" ")
    ip = y[:i]
    y = y[i + 1:]
    i = y.find(" ")
    client_id = y[:i]
    y = y[i + 1:]
    i = y.find(" ")
    user_id = y[:i]
    y = y[i + 1:]
    i = y.find("]")
    date = y[:i][1:]
    y = y[i + 2:]
    y = y[y.find('"') + 1:]
    method = ""
    endpoint = ""
    protocol = ""
    failed = False
    if y.find(" ") < y.rfind('"'):
        i = y.find(" ")
        method = y[:i]
        y = y[i + 1:]
        i = y.find(" ")
        endpoint = y[:i]
        y = y[i + 1:]
        i = y.rfind('"')
        protocol = y[:i]
        protocol = protocol[protocol.rfind(" ") + 1:]
        y = y[i + 2:]
    else:
        failed = True
        i = y.rfind('"')
        y = y[i + 2:]
    i = y.find(" ")
    response_code = y[:i]
    content_size = y[i + 1:]
    if not failed:
        return (ip, client_id, user_id, date, method, endpoint, protocol,
                int(response_code),
                0 if content_size == '-' else int(content_size))
    else:
        return ("", "", "", "", "", "", "", -1, -1)


# ---- data ---------------------------------------------------------------------

_MONTHS = ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep",
           "Oct", "Nov", "Dec"]


def _good_line(rng):
    ip = "%d.%d.%d.%d" % (rng.randint(1, 255), rng.randint(0, 255),
                          rng.randint(0, 255), rng.randint(0, 255))
    user = rng.choice(["-", "-", "alice", "bob_7", "svc.web"])
    date = "%02d/%s/%d:%02d:%02d:%02d %s%04d" % (
        rng.randint(1, 28), rng.choice(_MONTHS), rng.randint(1995, 2020),
        rng.randint(0, 23), rng.randint(0, 59), rng.randint(0, 59),
        rng.choice("+-"), rng.choice([0, 100, 400, 530, 800]))
    method = rng.choice(["GET", "GET", "POST", "HEAD", "PUT"])
    depth = rng.randint(1, 5)
    url = "".join("/" + rng.choice(["~user", "img", "a-b", "page%d" %
                                    rng.randint(0, 9999), "x.html", "q?k=v"])
                  for _ in range(depth))
    proto = rng.choice(["HTTP/1.0", "HTTP/1.1", "HTTP/1.1", ""])
    code = rng.choice([200, 200, 200, 301, 304, 404, 500])
    size = rng.choice(["-", str(rng.randint(0, 2000000))])
    req = "%s %s %s" % (method, url, proto) if proto else \
        "%s %s" % (method, url)
    return '%s - %s [%s] "%s" %d %s' % (ip, user, date, req, code, size)


def make_log_lines(n=5000, seed=11, bad_frac=0.02, nonascii=3):
    """Common-Log lines; ~bad_frac malformed (missing quote, short line,
    empty protocol with trailing blank, junk) and a few non-ASCII lines."""
    rng = random.Random(seed)
    lines = []
    for _ in range(n):
        good = _good_line(rng)
        if rng.random() < bad_frac:
            kind = rng.randint(0, 3)
            if kind == 0:
                good = good.replace('"', '', 1)       # missing quote
            elif kind == 1:
                good = " ".join(good.split(" ")[:3])  # short line
            elif kind == 2:
                good = good.replace(' HTTP/1.1"', ' "')  # empty protocol
            else:
                good = "garbage " + good[::-1]
        lines.append(good)
    for k in range(nonascii):
        i = (k + 1) * n // (nonascii + 1)
        lines[i] = lines[i].replace("/", "/caf\u00e9/", 1)
    return lines


def well_formed_lines(n=4900, seed=11):
    rng = random.Random(seed)
    return [_good_line(rng) for _ in range(n)]


def log_text_bytes(lines):
    return ("\n".join(lines) + "\n").encode("utf-8")


# ---- semantics table ----------------------------------------------------------

def sem_optional(x):
    m = re.search(r'(a)?b', x)
    if m:
        return (m[1], m[0])
    return (None, '')


def sem_alt_order(x):
    m = re.search(r'(ab|a|abc)(c?)', x)
    if m:
        return (m[1], m[2])
    return ('', '')


def sem_lazy_greedy(x):
    m = re.search(r'<(.+?)>.*<(.+)>', x)
    if m:
        return (m[1], m[2])
    return ('', '')


def sem_dollar(x):
    m = re.search(r'(\w+)$', x)
    return m[1] if m else ''


def sem_fullmatch(x):
    m = re.fullmatch(r'a+', x)
    return 1 if m else 0


def sem_endz(x):
    m = re.search(r'a\Z', x)
    return m is not None


def sem_space(x):
    m = re.search(r'(\S+)\s+(\S+)', x)
    if m:
        return (m.group(1), m.group(2))
    return ('', '')


def sem_bounds(x):
    m = re.search(r'(\d{2,4})(\d*)', x)
    if m:
        return (m[1], m[2])
    return ('', '')


def sem_wordb(x):
    m = re.search(r'\b(cat)\b', x)
    return 0 if m is None else 1


def sem_match_vs_search(x):
    a = re.match(r'[0-9]+', x)
    b = re.search(r'[0-9]+', x)
    return (a.group() if a else '', b.group() if b else '')


def sem_alt_group(x):
    m = re.match(r'(?:(x+)|(y+))-(\d+|z)', x)
    if m:
        return (m[1], m[2], m[3])
    return (None, None, '')


def sem_not_none(x):
    m = re.search(r'[^,;]{3}(?:;|,)', x)
    return m.group() if m is not None else 'none'


SEM_UDFS = [sem_optional, sem_alt_order, sem_lazy_greedy, sem_dollar,
            sem_fullmatch, sem_endz, sem_space, sem_bounds, sem_wordb,
            sem_match_vs_search, sem_alt_group, sem_not_none]


def sem_strings(n=200, seed=23):
    fixed = ["", "b", "ab", "aab", "abc", "abcc", "a", "aa", "aaa", "a\n",
             "aa\n", "a\n\n", "\na", "word\n", "two words\n", "x\x1cy",
             "x \x1f\ty z", "\x1c", "  lead", "<a><b>", "<a>x<b>y<c>",
             "<>", "<a>", "1", "12", "123", "12345", "1234567", "x12y",
             "cat", "a cat b", "concat", "cat!", "cats", " cat", "xx-12",
             "yyy-z", "x-", "xy-1", "-1", "abc;", "a,b;c,", "ab;", ",,,,",
             "abc,def;", "9 lives", "no digits", "7", "\n", " "]
    rng = random.Random(seed)
    alpha = "ab c<>x1;,\n-ytz9"
    out = list(fixed)
    while len(out) < n:
        out.append("".join(rng.choice(alpha)
                           for _ in range(rng.randint(0, 14))))
    return out


# ---- budget divert / unguarded group -----------------------------------------

def nested_plus(x):
    m = re.search(r'(a+)+b', x)
    return m[1] if m else 'no'


def budget_rows():
    rows = []
    for k in range(12, 17):
        rows.append("a" * k)
        rows.append("a" * (k - 10) + "b")
        rows.append("xyz")
    return rows


def unguarded_digits(x):
    return re.search(r'(\d+)', x)[1]


def empty_resolver(x):
    return ''


def digit_rows(n=400, seed=5):
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        if rng.random() < 0.25:
            rows.append("".join(rng.choice("abc xyz") for _ in range(8)))
        else:
            rows.append("id=%d;" % rng.randint(0, 10 ** 6))
    return rows


# ---- long rows ----------------------------------------------------------------

def long_anchored(x):
    m = re.match(r'([a-h]+)[ ,x]', x)
    return m[1] if m else ''


def long_search(x):
    m = re.search(r'x,([a-h]{3,}) ', x)
    if m:
        return (m[1], len(m[0]))
    return ('', -1)


def long_rows():
    from tests.extra_data import make_long_rows
    return make_long_rows(300, seed=9)


# ---- build hook -----------------------------------------------------------------

def stage_specs():
    """(name, input_types, columns, ops, source, sink, csv_info) of every regex
    stage the GPU tests run."""
    from tuplex_amd import ttypes as T
    text = {"null_values": [], "delimiter": ",", "text_mode": True}
    specs = [
        ("regex_text_mem", [T.STR], None, regex_ops(), "csv", "mem", text),
        ("regex_text_csv", [T.STR], None, regex_ops(), "csv", "csv", text),
        ("split_regex", [T.STR], ["logline"], split_regex_ops(), "mem", "mem",
         None),
        ("budget", [T.STR], None, [("map", nested_plus)], "mem", "mem", None),
        ("unguarded", [T.STR], None, [("map", unguarded_digits)], "mem",
         "mem", None),
        ("unguarded_resolve", [T.STR], None,
         [("map", unguarded_digits), ("resolve", TypeError, empty_resolver)],
         "mem", "mem", None),
        ("long_anchored", [T.STR], None, [("map", long_anchored)], "mem",
         "mem", None),
        ("long_search", [T.STR], None, [("map", long_search)], "mem", "mem",
         None),
        ("probe_regex", [T.STR], None, [("map", ParseWithRegex)], "csv",
         "mem", text),
        ("probe_strip", [T.STR], None, [("map", ParseWithStripTuple)], "csv",
         "mem", text),
    ]
    for f in SEM_UDFS:
        specs.append(("sem_" + f.__name__, [T.STR], None, [("map", f)],
                      "mem", "mem", None))
    return specs


def generate_sources():
    from tuplex_amd import codegen, plan
    out = []
    for name, in_types, cols, ops, source, sink, info in stage_specs():
        sp = plan.build_stage(in_types, cols, ops)
        assert sp.compilable, (name, sp.why_not_compilable)
        kw = {"csv_info": dict(info)} if info else {}
        src, desc = codegen.generate_stage(sp, source=source, sink=sink, **kw)
        out.append((name, src, desc))
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
            print("precompiled regex:", name)
    return n

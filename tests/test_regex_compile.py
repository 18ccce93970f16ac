"""CPU checks of the regex front end: re.search/re.match/re.fullmatch UDFs compile
to TIR (udf/compile.py, udf/relower.py), the TIR evaluates like CPython, what is
outside the subset is rejected (never compiled approximately), and codegen emits
one VM call per call site in stages that hipRTC-compiles for gfx950."""
import json
import os
import re

import pytest

from tests import regex_pipelines as RP
from tests import tir_eval
from tuplex_amd import codegen, plan
from tuplex_amd import ttypes as T
from tuplex_amd.udf import tir
from tuplex_amd.udf.compile import UDFCompileError, compile_udf

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- thin evaluator: regex ops here (CPython re), the rest in tir_eval --------

def ev(node, row):
    memo = {}

    def rec(n):
        key = id(n)
        if key in memo:
            return memo[key]
        op = n["op"]
        if op == "re_exec":
            mode, pattern = n["v"]
            v = getattr(re, mode)(pattern, rec(n["args"][0]))
        elif op == "re_matched":
            v = rec(n["args"][0]) is not None
        elif op == "re_group":
            m = rec(n["args"][0])
            v = m[n["w"]] if n["v"] == "item" else m.group(n["w"])
        else:
            v = tir_eval._ev(n, row, rec)
        memo[key] = v
        return v

    return rec(node)


def _outcome(fn, *args):
    try:
        return ("ok", fn(*args))
    except Exception as e:  # noqa: BLE001 - the class is what is compared
        return ("exc", type(e).__name__)


# ---- the reference's constant-pattern UDFs -------------------------------------

def ref_v1(x):
    return re.search(r'(.*)l.*', x)[1]


def ref_v2(x):
    match = re.search(r'(.*)l(.*)', x)
    return (match[1], match[2])


def ref_v3(x):
    return re.search(r'(.*)l[^0-9]*' + r'([0-9]*)', x)[2]


def ref_v4(x):
    p1 = r'(.*)l([^0-9]*)'
    p2 = r'([0-9]*)'
    match = re.search(p1 + p2, x)
    return (match[1], match[2], match[3])


REF_UDFS = {f.__name__: f for f in (ref_v1, ref_v2, ref_v3, ref_v4)}


# ---- accepts --------------------------------------------------------------------

def test_accepts_parse_with_regex():
    node = compile_udf(RP.ParseWithRegex, [T.STR], None)
    assert node["op"] == "mktuple"
    assert [e["t"] for e in node["args"]] == [T.STR] * 7 + [T.I64, T.I64]
    execs = [n for n in tir.walk(node) if n["op"] == "re_exec"]
    assert len(execs) == 1 and execs[0]["prog"].ngroups == 9


@pytest.mark.parametrize("col,fn", RP.SPLIT_UDFS, ids=[c for c, _ in RP.SPLIT_UDFS])
def test_accepts_split_regex_udfs(col, fn):
    node = compile_udf(fn, [T.STR], ["logline"])
    want = T.I64 if col in ("response_code", "content_size") else T.STR
    assert node["t"] == want


@pytest.mark.parametrize("name", sorted(REF_UDFS))
def test_accepts_reference_constant_patterns(name):
    node = compile_udf(REF_UDFS[name], [T.STR], None)
    assert not any(n["t"] == tir.MATCH for n in
                   (node["args"] if node["op"] == "mktuple" else [node]))


@pytest.mark.parametrize("fn", RP.SEM_UDFS + [RP.nested_plus,
                                              RP.unguarded_digits,
                                              RP.long_anchored, RP.long_search],
                         ids=lambda f: f.__name__)
def test_accepts_test_pipeline_udfs(fn):
    compile_udf(fn, [T.STR], None)


def test_stage_compilable_on_gpu_path():
    """Before this feature every `re.` UDF made the whole stage fall back."""
    sp = plan.build_stage([T.STR], None, RP.regex_ops())
    assert sp.compilable, sp.why_not_compilable
    sp = plan.build_stage([T.STR], ["logline"], RP.split_regex_ops())
    assert sp.compilable, sp.why_not_compilable


# ---- group types ----------------------------------------------------------------

def g_opt_q(x):
    return re.search(r'(a)?b', x)[1]


def g_opt_star(x):
    return re.search(r'(?:(a)c)*b', x)[1]


def g_opt_brace0(x):
    return re.search(r'(?:(a)c){0,2}b', x)[1]


def g_opt_alt(x):
    return re.search(r'(?:(a+)|(b+))c', x)[2]


def g_mandatory(x):
    return re.search(r'(a*)b', x)[1]


def g_mandatory_plus(x):
    return re.search(r'(a+)+b', x)[1]


def g_nested(x):
    m = re.search(r'((a)|b)(c)', x)
    return (m[1], m[2], m[3], m[0], m.group(), m.group(3))


def test_group_types():
    assert compile_udf(g_opt_q, [T.STR], None)["t"] == T.opt(T.STR)
    assert compile_udf(g_opt_star, [T.STR], None)["t"] == T.opt(T.STR)
    assert compile_udf(g_opt_brace0, [T.STR], None)["t"] == T.opt(T.STR)
    assert compile_udf(g_opt_alt, [T.STR], None)["t"] == T.opt(T.STR)
    assert compile_udf(g_mandatory, [T.STR], None)["t"] == T.STR
    assert compile_udf(g_mandatory_plus, [T.STR], None)["t"] == T.STR
    node = compile_udf(g_nested, [T.STR], None)
    assert [e["t"] for e in node["args"]] == \
        [T.STR, T.opt(T.STR), T.STR, T.STR, T.STR, T.STR]


def opt_subject(x):
    return re.search(r'a', x) is None


def test_optional_subject_unwraps():
    node = compile_udf(opt_subject, [T.opt(T.STR)], None)
    assert any(n["op"] == "unwrap" for n in tir.walk(node))
    with pytest.raises(TypeError):
        ev(node, (None,))
    assert ev(node, ("xyz",)) is True


# ---- rejections -----------------------------------------------------------------

_PAT = ""


def pat_udf(x):
    m = re.search(_PAT, x)
    return m[0] if m else ''


REJECTED_PATTERNS = [
    ("backreference", r'(a)\1'),
    ("named_backreference", r'(?P<q>a)(?P=q)'),
    ("lookahead", r'a(?=b)'),
    ("negative_lookahead", r'a(?!b)'),
    ("lookbehind", r'(?<=a)b'),
    ("negative_lookbehind", r'(?<!a)b'),
    ("inline_flag_global", r'(?i)abc'),
    ("inline_flag_scoped", r'(?i:a)bc'),
    ("inline_flag_ascii", r'(?a)\w'),
    ("group_conditional", r'(a)?(?(1)b|c)'),
    ("atomic_group", r'(?>a+)b'),
    ("possessive_repeat", r'a*+b'),
    ("repeat_of_emptyable_group", r'(a*)*b'),
    ("optional_emptyable_group", r'(?:a?|b*)?c'),
    ("capture_in_lazy_group_repeat", r'(a|bc)+?d'),
    ("non_ascii_literal", 'café'),
    ("invalid_pattern", r'(a'),
]


@pytest.mark.parametrize("pattern", [p for _, p in REJECTED_PATTERNS],
                         ids=[n for n, _ in REJECTED_PATTERNS])
def test_rejected_patterns(pattern):
    global _PAT
    _PAT = pattern
    try:
        with pytest.raises(UDFCompileError):
            compile_udf(pat_udf, [T.STR], None)
    finally:
        _PAT = ""


def test_accepted_pattern_through_global():
    global _PAT
    _PAT = r'(\d+)-(\d+)'
    try:
        node = compile_udf(pat_udf, [T.STR], None)
    finally:
        _PAT = ""
    assert ev(node, ("tel 12-345",)) == "12-345"


def rej_flags_arg(x):
    m = re.search(r'a', x, re.IGNORECASE)
    return m is None


def rej_flags_kw(x):
    m = re.search(r'a', x, flags=0)
    return m is None


def rej_one_arg(x):
    return re.search(r'a') is None


def rej_returns_match(x):
    return re.search(r'a', x)


def rej_match_in_tuple(x):
    return (re.search(r'a', x), 1)


def rej_match_in_branch(x):
    m = re.search(r'a', x)
    if len(x) > 2:
        return m
    return None


def rej_compare_match(x):
    return re.search(r'a', x) == 1


def rej_compare_two_matches(x):
    return re.search(r'a', x) is re.search(r'b', x)


def rej_match_as_argument(x):
    return str(re.search(r'a', x))


def rej_group_too_large(x):
    return re.search(r'(a)(b)', x)[3]


def rej_group_negative(x):
    return re.search(r'(a)(b)', x)[-1]


def rej_group_dynamic(x):
    return re.search(r'(a)(b)', x)[len(x)]


def rej_group_method_too_large(x):
    return re.search(r'(a)', x).group(2)


def rej_other_match_method(x):
    return re.search(r'(a)', x).start()


def rej_pattern_from_column(x, y):
    return re.search(x, y)[1]


def rej_re_sub(x):
    return re.sub(r'a', 'b', x)


def rej_non_str_subject(x):
    return re.search(r'1', x) is None


def rej_match_value_in_boolop(x):
    return re.search(r'a', x) and True


REJECTED_UDFS = [rej_flags_arg, rej_flags_kw, rej_one_arg, rej_returns_match,
                 rej_match_in_tuple, rej_match_in_branch, rej_compare_match,
                 rej_compare_two_matches, rej_match_as_argument,
                 rej_group_too_large, rej_group_negative, rej_group_dynamic,
                 rej_group_method_too_large, rej_other_match_method,
                 rej_re_sub, rej_match_value_in_boolop]


@pytest.mark.parametrize("fn", REJECTED_UDFS, ids=lambda f: f.__name__)
def test_rejected_udfs(fn):
    with pytest.raises(UDFCompileError):
        compile_udf(fn, [T.STR], None)


def test_rejected_pattern_from_column_and_int_subject():
    with pytest.raises(UDFCompileError):
        compile_udf(rej_pattern_from_column, [T.STR, T.STR], None)
    with pytest.raises(UDFCompileError):
        compile_udf(rej_non_str_subject, [T.I64], None)


def shadowed_re(x):
    re = x  # noqa: F841 - a local named `re` is not the module
    return re.search("a", x) is None


def test_re_must_be_the_module():
    with pytest.raises(UDFCompileError):
        compile_udf(shadowed_re, [T.STR], None)


def test_rejected_stage_falls_back_as_before():
    sp = plan.build_stage([T.STR], None, [("map", rej_re_sub)])
    assert not sp.compilable and "re.sub" in sp.why_not_compilable


# ---- TIR evaluation == CPython ----------------------------------------------------

@pytest.fixture(scope="module")
def log_lines():
    return RP.make_log_lines(1500, seed=11, bad_frac=0.05, nonascii=3)


def test_tir_matches_cpython_parse_with_regex(log_lines):
    node = compile_udf(RP.ParseWithRegex, [T.STR], None)
    n_fail = 0
    for line in log_lines:
        want = RP.ParseWithRegex(line)
        assert ev(node, (line,)) == want, line
        n_fail += want[0] == ''
    assert 0 < n_fail < len(log_lines) // 4


@pytest.mark.parametrize("col,fn", RP.SPLIT_UDFS, ids=[c for c, _ in RP.SPLIT_UDFS])
def test_tir_matches_cpython_split_regex(col, fn, log_lines):
    node = compile_udf(fn, [T.STR], ["logline"])
    for line in log_lines:
        assert _outcome(ev, node, (line,)) == _outcome(fn, {"logline": line}), \
            line


@pytest.mark.parametrize("fn", RP.SEM_UDFS + [RP.nested_plus, g_nested,
                                              g_opt_star, g_opt_alt],
                         ids=lambda f: f.__name__)
def test_tir_matches_cpython_semantics_table(fn):
    node = compile_udf(fn, [T.STR], None)
    rows = RP.sem_strings() + ["aab", "ac", "acacb", "xxxc", "bc", "abc"]
    for s in rows:
        assert _outcome(ev, node, (s,)) == _outcome(fn, s), (fn.__name__, s)


def unguarded_method(x):
    return re.search(r'(\d+)', x).group(1)


def test_unguarded_group_raises_like_cpython(log_lines):
    rows = RP.digit_rows()
    for fn, exc in ((RP.unguarded_digits, "TypeError"),
                    (unguarded_method, "AttributeError")):
        node = compile_udf(fn, [T.STR], None)
        got = [_outcome(ev, node, (s,)) for s in rows]
        assert got == [_outcome(fn, s) for s in rows]
        assert 20 < sum(g == ("exc", exc) for g in got) < len(rows)
    # malformed log lines through an unguarded nine-group parse
    def unguarded_parse(x):
        return re.search(r'^(\S+) (\S+) (\S+) \[', x)[3]
    node = compile_udf(unguarded_parse, [T.STR], None)
    got = [_outcome(ev, node, (s,)) for s in log_lines]
    assert got == [_outcome(unguarded_parse, s) for s in log_lines]
    assert ("exc", "TypeError") in got


# ---- golden vectors from the reference's own test ----------------------------------

def _goldens():
    with open(os.path.join(HERE, "golden", "regex_goldens.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _goldens(), ids=lambda c: c["udf"])
def test_reference_goldens(case):
    fn = REF_UDFS[case["udf"]]
    assert case["cite"].startswith("UseCaseFunctionsTest.cc:")
    node = compile_udf(fn, [T.STR], None)
    pattern = "".join(case["pattern_parts"])
    execs = [n for n in tir.walk(node) if n["op"] == "re_exec"]
    assert [n["v"] for n in execs] == [("search", pattern)]
    assert sorted(n["w"] for n in tir.walk(node) if n["op"] == "re_group") == \
        case["groups"]
    for s, want in zip(case["inputs"], case["expected"]):
        want = tuple(want) if isinstance(want, list) else want
        assert ev(node, (s,)) == want
        assert fn(s) == want


# ---- codegen ----------------------------------------------------------------------

def _generated_part(src):
    """The stage source after the runtime + regex headers."""
    head = codegen.regex_header()
    assert src.count(head) == 1
    return src.split(head)[1]


def test_one_vm_call_for_nine_groups():
    sp = plan.build_stage([T.STR], None, RP.regex_ops())
    src, _ = codegen.generate_stage(sp, source="mem", sink="mem")
    body = _generated_part(src)
    assert body.count("tpx_re_exec(") == 1
    assert body.count("tpx_re_group(") == 9
    assert body.count("__device__ const int re_prog") == 1


def test_one_vm_call_per_split_regex_operator():
    sp = plan.build_stage([T.STR], ["logline"], RP.split_regex_ops())
    src, _ = codegen.generate_stage(sp, source="mem", sink="mem")
    assert _generated_part(src).count("tpx_re_exec(") == 9


def test_same_search_twice_is_one_call():
    def twice(x):
        a = re.search(r'(\d+)', x)
        b = re.search(r'(\d+)', x)
        if a and b:
            return a[1] + b[0]
        return ''
    sp = plan.build_stage([T.STR], None, [("map", twice)])
    assert sp.compilable, sp.why_not_compilable
    src, _ = codegen.generate_stage(sp, source="mem", sink="mem")
    assert _generated_part(src).count("tpx_re_exec(") == 1


def test_stage_without_regex_has_no_regex_text():
    from tests.pipelines import PIPELINES
    name, data, columns, ops = PIPELINES[0]
    maj = T.infer_majority_type(data, optional_threshold=0.7)
    sp = plan.build_stage(list(T.tuple_params(T.row_type_of(maj))), columns,
                          ops)
    assert sp.compilable
    src, _ = codegen.generate_stage(sp, source="mem", sink="mem")
    assert "tpx_re_" not in src and "TPX_RE_" not in src


def test_group_keeps_subject_quote_freedom():
    """csv source -> csv sink: a group is a view into its subject cell, so it
    needs the RFC-4180 quote scan only when that cell did (like slice)."""
    def first_word(x):
        m = re.search(r'(\w+)', x['a'])
        return m[1] if m else ''
    sp = plan.build_stage([T.STR, T.I64], ["a", "b"],
                          [("withColumn", "w", first_word)])
    assert sp.compilable, sp.why_not_compilable
    cg = codegen.StageCodegen(sp, "csv", "csv", {"null_values": [""]})
    assert cg._thread_qfree() == [frozenset([0]), True, frozenset([0])]


def test_udf_chain_with_re_global_pickles():
    import cloudpickle
    fn = cloudpickle.loads(cloudpickle.dumps(RP.extract_ip))
    assert fn({"logline": "1.2.3.4 - -"}) == "1.2.3.4"
    lam = cloudpickle.loads(cloudpickle.dumps(
        lambda x: re.search(r'(\d+)', x)[1]))
    assert lam("ab12") == "12"


@pytest.mark.parametrize("spec", RP.stage_specs(), ids=lambda s: s[0])
def test_regex_stages_hiprtc_compile(spec):
    from tests.test_codegen_compile import _lib, _numbered
    name, in_types, cols, ops, source, sink, info = spec
    sp = plan.build_stage(in_types, cols, ops)
    assert sp.compilable, sp.why_not_compilable
    kw = {"csv_info": dict(info)} if info else {}
    src, desc = codegen.generate_stage(sp, source=source, sink=sink, **kw)
    lib = _lib()
    cache = os.path.join(os.path.dirname(HERE), "tuplex_amd", ".kernel_cache")
    os.makedirs(cache, exist_ok=True)
    h = lib.tpx_stage_compile(src.encode(), desc.encode(), cache.encode(), 1)
    if not h:
        raise AssertionError("hipRTC compile failed:\n%s\n--- source ---\n%s"
                             % (lib.tpx_last_error().decode()[:4000],
                                _numbered(src)))
    lib.tpx_stage_free(h)

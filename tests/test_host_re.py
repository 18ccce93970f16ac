"""Host-compiled parity of the device regex VM (csrc/tpx_re.hip.h) with CPython:
tests/host_re_test.cpp runs lowered programs over subjects on the host and
prints every group span, the step count, the peak stack depth and the divert
flag. 20k fuzzed (pattern, subject) cases must give CPython's spans unless the
VM diverts (at most 1 %); the well-formed log fixture must never divert and
must stay within a quarter of the step/stack limits. The same program is run
a second time under ASan+UBSan (a plain executable, nothing loaded into
Python)."""
import os
import random
import re
import subprocess

import pytest

from tests import regex_pipelines as RP
from tuplex_amd.udf import relower

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "tuplex_amd", "csrc", "tpx_re.hip.h")

N_PATTERNS = 2000
SUBJECTS_PER_PATTERN = 10
SEED = 20240607
ALPHABET = 'ab1 "\n\x1c_-'


def _limits():
    text = open(HEADER).read()
    out = {}
    for name in ("TPX_RE_STACK", "TPX_RE_BUDGET_A", "TPX_RE_BUDGET_B"):
        out[name] = int(re.search(r"#define %s (\d+)" % name, text).group(1))
    return out


# ---- random patterns from a grammar inside the supported subset ---------------

_ATOMS = ["a", "b", "1", " ", '"', "_", "-", ".", r"\d", r"\D", r"\s", r"\S",
          r"\w", r"\W", "[ab]", "[^a]", r"[\d_]", r"[^\s1]", "[a-b1-9]",
          r"\n", r'[^"]', r"[\w-]"]
_QUANTS = ["", "", "", "*", "+", "?", "*?", "+?", "??", "{2}", "{1,3}",
           "{0,2}", "{2,}", "{1,2}?"]
_ANCHORS = ["^", "$", r"\A", r"\Z", r"\b", r"\B"]


def _gen_seq(rng, depth, n_items):
    parts = []
    for _ in range(n_items):
        r = rng.random()
        if r < 0.62 or depth >= 2:
            parts.append(rng.choice(_ATOMS) + rng.choice(_QUANTS))
        elif r < 0.72:
            parts.append(rng.choice(_ANCHORS))
        elif r < 0.90:
            inner = _gen_seq(rng, depth + 1, rng.randint(1, 3))
            opener = rng.choice(["(", "(", "(?:"])
            parts.append(opener + inner + ")" + rng.choice(_QUANTS))
        else:
            alts = [_gen_seq(rng, depth + 1, rng.randint(1, 2))
                    for _ in range(rng.randint(2, 3))]
            opener = rng.choice(["(", "(?:"])
            parts.append(opener + "|".join(alts) + ")" + rng.choice(_QUANTS))
    return "".join(parts)


def gen_cases(n_patterns=N_PATTERNS, per=SUBJECTS_PER_PATTERN, seed=SEED):
    """[(pattern, mode, program, [subjects])] — patterns the lowering rejects
    (e.g. a repeated group that can match empty) are regenerated."""
    rng = random.Random(seed)
    cases = []
    while len(cases) < n_patterns:
        pat = _gen_seq(rng, 0, rng.randint(1, 4))
        mode = rng.choice(["search", "search", "match", "fullmatch"])
        try:
            re.compile(pat)
            prog = relower.lower(pat, mode)
        except (re.error, relower.ReLowerError):
            continue
        subjects = []
        for _ in range(per):
            ln = rng.choice([0, 1, 2, 3, 5, 8, 13, 21])
            subjects.append("".join(rng.choice(ALPHABET) for _ in range(ln)))
        cases.append((pat, mode, prog, subjects))
    return cases


# ---- driver ---------------------------------------------------------------------

def _build(tmp_path, name, flags):
    exe = os.path.join(str(tmp_path), name)
    subprocess.check_call(["g++"] + flags + ["-o", exe,
                                             os.path.join(HERE, "host_re_test.cpp")])
    return exe


def _run(exe, cases):
    lines = []
    for _pat, _mode, prog, subjects in cases:
        lines.append("P %d %s" % (len(prog.words),
                                  " ".join(map(str, prog.words))))
        for s in subjects:
            lines.append("S " + (s.encode("utf-8").hex() or "-"))
    out = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(),
                         stdout=subprocess.PIPE, check=True,
                         timeout=600).stdout.decode().split("\n")
    assert out[-2] == "OK", out[-5:]
    return [tuple(map(int, ln.split())) for ln in out[:-2]]


def _expected(pat, mode, prog, s):
    m = getattr(re, mode)(pat, s)
    if m is None:
        return None
    spans = []
    for k in range(prog.ngroups + 1):
        spans.extend(m.span(k))
    return tuple(spans)


def _check_fuzz(exe):
    cases = gen_cases()
    res = _run(exe, cases)
    assert len(res) == N_PATTERNS * SUBJECTS_PER_PATTERN >= 20000
    i = 0
    diverts = 0
    bad = []
    for pat, mode, prog, subjects in cases:
        for s in subjects:
            r = res[i]
            i += 1
            if r[0]:
                diverts += 1
                continue
            want = _expected(pat, mode, prog, s)
            got = tuple(r[4:]) if r[1] else None
            if got != want:
                bad.append((pat, mode, s, got, want))
    assert not bad, bad[:10]
    print("fuzz: %d cases, %d diverts" % (len(res), diverts))
    assert diverts <= len(res) // 100, diverts


def _log_cases():
    lines = RP.well_formed_lines()
    pats = []
    for fn in RP.LOG_UDFS:
        consts = [c for c in fn.__code__.co_consts if isinstance(c, str)
                  and ("\\S" in c or "\\d" in c)]
        assert len(consts) == 1, fn
        pats.append(consts[0])
    return [(p, "search", relower.lower(p, "search"), lines) for p in pats]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("host_re"), "host_re_test",
                  ["-O2", "-Wall"])


def test_fuzz_spans_match_cpython(exe):
    _check_fuzz(exe)


def test_log_fixture_no_divert_within_quarter_of_limits(exe):
    lim = _limits()
    cases = _log_cases()
    assert len(cases) == 10
    res = _run(exe, cases)
    i = 0
    max_steps = (0, 0)
    max_depth = 0
    worst_ratio = 0.0
    for pat, mode, prog, lines in cases:
        for s in lines:
            r = res[i]
            i += 1
            assert r[0] == 0, ("diverted", pat, s)
            assert r[1] == 1, ("well-formed line must match", pat, s)
            assert tuple(r[4:]) == _expected(pat, mode, prog, s), (pat, s)
            budget = lim["TPX_RE_BUDGET_A"] + lim["TPX_RE_BUDGET_B"] * len(s)
            assert 4 * r[2] <= budget, (pat, s, r[2], budget)
            assert 4 * r[3] <= lim["TPX_RE_STACK"], (pat, s, r[3])
            if r[2] > max_steps[0]:
                max_steps = (r[2], len(s))
            max_depth = max(max_depth, r[3])
            worst_ratio = max(worst_ratio, r[2] / budget)
    print("log fixture: max steps %d (on a %d-byte line), worst steps/budget "
          "%.3f, max stack depth %d" % (max_steps[0], max_steps[1],
                                        worst_ratio, max_depth))


def test_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "host_re_asan",
                 ["-O1", "-g", "-fsanitize=address,undefined",
                  "-fno-sanitize-recover=all"])
    _check_fuzz(exe)
    res = _run(exe, _log_cases()[:2])
    assert all(r[0] == 0 and r[1] == 1 for r in res)

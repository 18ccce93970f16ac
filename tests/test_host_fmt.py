"""Differential test of csrc/tpx_fmt.hip.h on the host: tests/host_fmt_test.cpp
is a stand-alone program, built plain and with ASan+UBSan and run as its own
process. This side generates the vectors — templates go through the same
udf/fmtspec.py parser and encoder the code generator uses — computes the
expected text with CPython's own str.format / % / string.capwords, and diffs."""
import os
import string
import subprocess

import pytest

from tests import vocab_pipelines as V
from tuplex_amd.udf import fmtspec

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_fmt_test.cpp")

EC_NCV = 7
EC_MEMORYERROR = 114
CHUNK = 256       # TPX_HEAP_CHUNK: smaller allocations take a whole chunk
BIG = 8192


def _hex(b):
    return b.hex() if b else "-"


# ---- requests -----------------------------------------------------------------------

def _kind(a):
    return "s" if isinstance(a, (str, bytes)) else "i"


def raw_fmt_request(template, raw, align=0):
    """One str field over raw bytes that need not be UTF-8 (a lone 0x80): with
    a width it diverts, without one the bytes are copied as they are."""
    items = fmtspec.parse_format(template, ["s"])
    words, blob = fmtspec.encode(items)
    (field,) = [it for it in items if it[0] == "str"]
    want = template.format(raw.decode("latin-1")).encode("latin-1")
    line = " ".join(["F", str(BIG), str(align), str(len(items)),
                     ",".join(map(str, words)), _hex(blob), "1", "S",
                     _hex(raw)])
    diverts = field[3] > 0 and any(c >= 0x80 for c in raw)
    return line, (EC_NCV if diverts else 0, want)


def fmt_request(template, args, percent, cap=BIG, align=0):
    """(request line, expected answer fields) of one template application."""
    parse = fmtspec.parse_percent if percent else fmtspec.parse_format
    items = parse(template, [_kind(a) for a in args])
    words, blob = fmtspec.encode(items)
    if percent:
        want = template % tuple(args)
    else:
        want = template.format(*args)
    parts = ["F", str(cap), str(align), str(len(items)),
             ",".join(map(str, words)), _hex(blob), str(len(args))]
    for a in args:
        if isinstance(a, str):
            parts += ["S", _hex(a.encode("utf-8"))]
        else:
            parts += ["I", str(a)]
    diverts = any(it[0] == "str" and it[3] > 0
                  and not args[it[1]].isascii() for it in items)
    return " ".join(parts), (EC_NCV if diverts else 0,
                             want.encode("utf-8"))


def cap_request(s, cap=BIG, align=0):
    b = s.encode("utf-8")
    diverts = any(c >= 0x80 for c in b)
    return ("C %d %d %s" % (cap, align, _hex(b)),
            (EC_NCV if diverts else 0, string.capwords(s).encode("utf-8")))


def int_vectors():
    out = []
    for v in V.edge_ints():
        for w in list(range(23)) + [255]:
            ws = str(w) if w else ""
            out.append(fmt_request("{:%s}" % ws, [v], False))
            out.append(fmt_request("{:0%s}" % ws, [v], False))
            out.append(fmt_request("{:0%sd}" % ws, [v], False))
            out.append(fmt_request("%" + ws + "d", [v], True))
            out.append(fmt_request("%0" + ws + "d", [v], True))
            out.append(fmt_request("%" + ws + "s", [v], True))
            if w:
                out.append(fmt_request("%-" + ws + "s|", [v], True))
    return out


def str_vectors():
    out = []
    for s in V.edge_strings():
        n = len(s)
        for align in range(8):
            # below, equal to and above the length, within the width cap
            for w in sorted(x for x in {0, max(n - 1, 0), n, n + 1, n + 9, 255}
                            if x <= fmtspec.MAX_WIDTH):
                ws = str(w) if w else ""
                out.append(fmt_request("{:%s}" % ws, [s], False, align=align))
                out.append(fmt_request("{:<%s}" % ws, [s], False, align=align))
                out.append(fmt_request("{:>%ss}" % ws, [s], False, align=align))
                out.append(fmt_request("%" + ws + "s", [s], True, align=align))
                if w:
                    out.append(fmt_request("%-" + ws + "s", [s], True,
                                           align=align))
    # "\u0080.." holds the byte 0x80 itself (C2 80), the lowest that counts
    # as non-ASCII; 0x7f is the highest that does not
    for s in V.NON_ASCII + ["\u0080", "ab\u0080", "\u0080cd ef", "\x7f\x7f"]:
        for align in (0, 3):
            out.append(fmt_request("{}", [s], False, align=align))
            out.append(fmt_request("<%s>", [s], True, align=align))
            out.append(fmt_request("{:4}", [s], False, align=align))
            out.append(fmt_request("{:>40}", [s], False, align=align))
            out.append(fmt_request("%-9s", [s], True, align=align))
    # the boundary itself: a lone 0x80 byte (0x7f on the other side) in the
    # first, middle and last position, at the lengths where tpx_ascii changes
    # from its byte loop to 8-byte words
    for n in (1, 3, 8, 9, 17, 40):
        for pos in sorted({0, n // 2, n - 1}):
            for b in (0x80, 0x7f):
                raw = bytes([b if i == pos else 0x61 for i in range(n)])
                for align in (0, 5):
                    out.append(raw_fmt_request("[{:>45}]", raw, align=align))
                    out.append(raw_fmt_request("[{}]", raw, align=align))
    return out


def template_vectors():
    s = V.edge_strings()
    out = [
        fmt_request("{}{}{}", ["a", 5, "c"], False),                # fields only
        fmt_request("%s%d%s", ["", -1, s[17]], True),
        fmt_request("{{}}", [], False),                 # literals only
        fmt_request("a{{b}}c}}{{", [], False),
        fmt_request("100%% sure", [], True),
        fmt_request("{}-{:02}:{:>4}|{:<4}|{}{:5}{}{:03}",            # 8 fields
                    [1, 2, "ab", "cd", s[9], -7, s[18], -5], False),
        fmt_request("%d-%02d:%4s|%-4s|%s%5d%s%03d",
                    [1, 2, "ab", "cd", s[9], -7, s[18], -5], True),
        fmt_request("{1}{0}{1}", ["x", "yy"], False),               # reordered
        fmt_request("{1:>5}{0:04}{1}", [-12, s[11]], False),
        fmt_request("{0}, {0}; {0:3}", [42], False),
    ]
    for align in range(8):  # a long literal blob at every source alignment
        out.append(fmt_request("literal that is longer than sixteen bytes {} "
                               "and goes on after the field", [s[13]], False,
                               align=align))
    return out


def capwords_vectors():
    out = []
    for s in V.capwords_strings():
        for align in (0, 1, 5):
            out.append(cap_request(s, align=align))
    for pos in ("first", "middle", "last"):
        base = "plain words here"
        # U+0080 encodes to C2 80: the byte 0x80 itself, the lowest that
        # diverts; U+00E9 to C3 A9
        for hi in ("\u0080", "\u00e9"):
            s = {"first": hi + base, "middle": base[:6] + hi + base[6:],
                 "last": base + hi}[pos]
            assert s.encode("utf-8").count(b"\x80") == (hi == "\u0080")
            out.append(cap_request(s))
        # a lone 0x80 byte (not UTF-8: only the divert is checked), and 0x7f,
        # which is an ordinary character
        n = len(base)
        at = {"first": 0, "middle": n // 2, "last": n - 1}[pos]
        raw = bytearray(base.encode())
        raw[at] = 0x80
        out.append(("C %d 0 %s" % (BIG, bytes(raw).hex()), (EC_NCV, b"")))
        raw[at] = 0x7f
        out.append(cap_request(bytes(raw).decode("ascii")))
    assert any(len(r[1][1]) >= 2900 for r in out)  # the 3000-byte input
    return out


def heap_vectors():
    """Capacity one byte short of the output: MEMORYERROR, nothing written.
    Exactly enough: the result. (An output of at most CHUNK bytes takes a
    whole chunk.)"""
    out = []
    s = V.edge_strings()
    cases = [("{:>40}|{}", [s[12], 123456], False),
             ("%s and %s", [s[18], s[18]], True),       # 600+ bytes: no chunk
             ("{:255}{:255}", [s[3], -1], False)]
    for template, args, percent in cases:
        _line, (_ec, want) = fmt_request(template, args, percent)
        n = len(want)
        short, (_e, _w) = fmt_request(template, args, percent, cap=n - 1)
        out.append((short, (EC_MEMORYERROR, b"")))
        if n <= CHUNK:
            chunk_short, _ = fmt_request(template, args, percent,
                                         cap=CHUNK - 1)
            out.append((chunk_short, (EC_MEMORYERROR, b"")))
        out.append(fmt_request(template, args, percent, cap=max(n, CHUNK)))
    for text in ("some words to capitalise", "w " * 400):
        n = len(string.capwords(text))
        out.append((cap_request(text, cap=n - 1)[0], (EC_MEMORYERROR, b"")))
        out.append(cap_request(text, cap=max(n, CHUNK)))
    return out


FAMILIES = [("ints", int_vectors), ("strings", str_vectors),
            ("templates", template_vectors), ("capwords", capwords_vectors),
            ("heap", heap_vectors)]


# ---- build + run --------------------------------------------------------------------

@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("host_fmt"))
    plain = os.path.join(d, "host_fmt_test")
    san = os.path.join(d, "host_fmt_asan")
    subprocess.check_call(["g++", "-O2", "-Wall", "-o", plain, SRC])
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", san, SRC])
    return {"plain": plain, "sanitized": san}


def _run(exe, vectors, tmp_path):
    req = os.path.join(str(tmp_path), "requests.txt")
    with open(req, "w") as f:
        for line, _want in vectors:
            f.write(line + "\n")
    p = subprocess.run([exe, req], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    lines = p.stdout.decode().splitlines()
    assert lines[-1] == "DONE" and len(lines) == len(vectors) + 1
    bad = []
    for (line, (ec, want)), got in zip(vectors, lines):
        g_ec, g_hex, _used, clean = got.split()
        g = b"" if g_hex == "-" else bytes.fromhex(g_hex)
        if int(g_ec) != ec or (ec == 0 and g != want) or clean != "1":
            bad.append((line[:200], ec, want[:80], got[:200]))
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(vectors),
                                                    bad[:3])


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("family", [f[0] for f in FAMILIES])
def test_builders_match_cpython(exes, build, family, tmp_path):
    vectors = dict(FAMILIES)[family]()
    assert vectors
    _run(exes[build], vectors, tmp_path)


def test_vectors_cover_the_edges():
    ints = V.edge_ints()
    for v in (0, 9, -9, 10, -10, 10 ** 18, -(10 ** 18), 10 ** 18 - 1,
              V.I64_MAX, V.I64_MIN):
        assert v in ints
    assert sorted({len(s) for s in V.edge_strings()}) == list(range(18)) + [300]
    ncv = [w for _l, w in str_vectors() if w[0] == EC_NCV]
    assert ncv and any(w[0] == 0 and not w[1].isascii()
                       for _l, w in str_vectors())
    # the boundary byte 0x80 with and without a width, 0x7f with a width
    assert any(b"\x80" in w[1] and w[0] == EC_NCV for _l, w in str_vectors())
    assert any(b"\x80" in w[1] and w[0] == 0 for _l, w in str_vectors())
    assert any(b"\x7f" in w[1] and w[0] == 0 and len(w[1]) > 2
               for _l, w in str_vectors())
    cap80 = [w for l, w in capwords_vectors() if l.split()[3] != "-"
             and max(bytes.fromhex(l.split()[3])) == 0x80]
    assert len(cap80) == 3 and all(w[0] == EC_NCV for w in cap80)
    lone = [w for l, w in str_vectors() if l.split()[-1] != "-"
            and max(bytes.fromhex(l.split()[-1])) == 0x80]
    assert {w[0] for w in lone} == {0, EC_NCV}
    caps = V.capwords_strings()
    for c in V.SPLIT_WS:
        assert c in caps and c * 3 in caps
    assert len(V.SPLIT_WS) == 10

"""Differential test of the scalar device runtime (csrc/tpx_rt.hip.h) on the
host: tests/host_rtops_test.cpp runs every helper the generated kernels call —
SWAR byte scans, string ops, int()/float() parsers, str(int)/%0Nd, the %f and
CSV cell writers, the Python-semantics arithmetic — on cases generated here,
and the results must equal CPython's (or the oracle's restatement of the
reference, for the parsers and the CSV walk). Subjects sit at all 8 alignments
in an arena padded with the needle byte; outputs go through a real TpxHeap with
canaries. The driver is built twice, plain -O2 and ASan+UBSan; both are plain
executables fed over stdin."""
import math
import os
import random
import subprocess

import pytest

from oracle import pyoracle
from oracle import pyoracle_csv
from tests import rtops_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_rtops_test.cpp")

HEAP_MAX = 8192
CHUNK = 256
EC = {IndexError: 111, MemoryError: 114, OverflowError: 118, TypeError: 129,
      ValueError: 135, ZeroDivisionError: 136}
EC_NULL, EC_I64PARSE, EC_F64PARSE, EC_BOOLPARSE = 50, 52, 53, 54
SPECIALS = [0x22, 0x2C, 0x0D, 0x0A, 0x7C]
ALL_OPS = """memchr memchr_hi memchr2 memrchr memchr_hi_spec ascii
csv_needs_quote csv_cell_len csv_cell_write memcpy find rfind contains
startswith endswith streq strcmp getitem slice center strmul lower upper
swapcase capitalize_ix strip concat replace splitget int_drop atoi atod
int_str float_str cell_i64 cell_f64 cell_bool floordiv_i64 mod_i64 truediv
floordiv_f64 mod_f64 int_f64 i64_digits i64_write str_i64 fmt0d f64_csv
csv_row""".split()
FLOAT_RESULT = {"atod", "cell_f64", "float_str", "truediv", "floordiv_f64",
                "mod_f64"}


def hx(b):
    if isinstance(b, str):
        b = b.encode("latin-1")
    return b.hex() if b else "-"


def fx(v):
    return "%016x" % RC.dbits(v)


def fexp(v):
    return "NAN" if v != v else fx(v)


def alloc_ok(n, cap):
    """tpx_alloc on a fresh heap: both of its paths."""
    if n <= 0:
        return True
    return n <= cap if n > CHUNK else CHUNK <= cap


class Cases:
    def __init__(self):
        self.lines = []
        self.expect = []
        self.rand = []
        self._k = 0

    def add(self, op, args, expect, pad=0x61, shift=None, cap=HEAP_MAX,
            alloc=None, rand=False):
        """alloc: bytes the op allocates when it gets that far (None: none)."""
        if shift is None:
            shift = self._k % 8
            self._k += 1
        if alloc is not None and not alloc_ok(alloc, cap):
            expect = "E%d" % EC[MemoryError]
        self.lines.append("%s %d %d %d %s" % (op, shift, pad, cap,
                                              " ".join(args)))
        self.expect.append(str(expect))
        self.rand.append(rand)

    def add_caps(self, op, args, expect, alloc, **kw):
        """An allocating op: a full-size heap, and heaps too small for the
        chunk path (cap 64) and for the direct path (cap 300)."""
        for cap in (HEAP_MAX, 64, 300):
            self.add(op, args, expect, cap=cap, alloc=alloc, **kw)


def py(fn):
    """Evaluate a CPython expression -> result or 'E<ec>'."""
    try:
        return fn()
    except tuple(EC) as e:
        return "E%d" % EC[type(e)]


# ---- byte scans ---------------------------------------------------------------------

def _filler_set(needles):
    s = {0x00, 0x7F, 0x80, 0xFF, 0x61} | set(SPECIALS)
    for c in needles:
        s |= {(c - 1) & 0xFF, (c + 1) & 0xFF, c ^ 0x80}
    return sorted(s - set(needles))


def _subject(rng, n, hits, needle, mode, fill, first, last):
    """n bytes without the needle, then the needle at `hits`. Modes: 0 random
    filler, 1 one filler byte, 2 plain ASCII, 3 ASCII up to the decisive hit and
    high/special bytes after it (a result computed from more than the bytes
    before the hit comes out wrong), 4 ASCII with one high byte."""
    plain = [b for b in b"axyz0 ." if b != needle]
    if mode == 0:
        s = [rng.choice(fill) for _ in range(n)]
    elif mode == 1:
        s = [fill[rng.randrange(len(fill))]] * n
    else:
        s = [rng.choice(plain) for _ in range(n)]
        if mode == 3:
            for i in range(n):
                if (first is not None and i > first) or \
                        (last is not None and i < last):
                    s[i] = rng.choice(fill)
        elif mode == 4 and n:
            s[rng.randrange(n)] = rng.choice(
                [b for b in (0x80, 0xFF, 0xC3) if b != needle])
    for h in hits:
        s[h] = needle
    return bytes(s)


def _hits(rng, n, pos, k, forward):
    """The decisive hit at pos, plus k-1 more on the side that must be ignored
    (two and three hits per string: first-vs-last)."""
    if pos is None:
        return []
    hits = [pos]
    lo, hi = (pos + 1, n - 1) if forward else (0, pos - 1)
    for _ in range(k - 1):
        if lo <= hi:
            hits.append(rng.randint(lo, hi))
    return hits


def spec_truth(s, needle, chk):
    """The hi/spec contract in tpx_rt.hip.h, as a byte loop: hi = a byte >=
    0x80 among those scanned (up to and including the hit; all, without a
    hit); spec = '"', CR (and ',' when chk) strictly before the hit."""
    hit = s.find(bytes([needle]))
    scanned = s if hit < 0 else s[:hit + 1]
    before = s if hit < 0 else s[:hit]
    hi = int(any(b >= 0x80 for b in scanned))
    sp = {0x22, 0x0D} | ({0x2C} if chk else set())
    return hit, hi, int(any(b in sp for b in before))


def gen_scans(C, rng):
    needles = [0x2C, 0x22, 0x7C, 0x0A, 0x61, 0x00, 0xFF, 0x80, 0x0D]
    k = 0
    for n in range(73):
        for shift in range(8):
            for pos in [None] + list(range(n)):
                for mode in (3, (0, 1, 2, 4)[k % 4]):
                    k += 1
                    nd = needles[k % len(needles)]
                    nhits = (1, 1, 2, 3)[(k // 3) % 4]
                    kw = dict(pad=nd, shift=shift)
                    fill = _filler_set([nd])
                    fwd = _subject(rng, n, _hits(rng, n, pos, nhits, True), nd,
                                   mode, fill, pos, None)
                    C.add("memchr", [hx(fwd), str(nd)],
                          fwd.find(bytes([nd])), **kw)
                    for chk in (0, 1):
                        hit, hi, sp = spec_truth(fwd, nd, chk)
                        if chk == 0:
                            C.add("memchr_hi", [hx(fwd), str(nd)],
                                  "%d %d" % (hit, hi), **kw)
                        C.add("memchr_hi_spec", [hx(fwd), str(nd), str(chk)],
                              "%d %d %d" % (hit, hi, sp), **kw)
                    bwd = _subject(rng, n, _hits(rng, n, pos, nhits, False),
                                   nd, mode, fill, None, pos)
                    C.add("memrchr", [hx(bwd), str(nd)],
                          bwd.rfind(bytes([nd])), **kw)
                    # two needles: either may be the first
                    n2 = needles[(k + 1 + k // 7 % 7) % len(needles)]
                    if n2 == nd:
                        n2 = 0x3B
                    fill2 = _filler_set([nd, n2])
                    s2 = bytearray(_subject(
                        rng, n, _hits(rng, n, pos, nhits, True), nd, mode,
                        [b for b in fill2], pos, None))
                    for i in range(len(s2)):
                        if s2[i] == n2:
                            s2[i] = 0x78
                    if pos is not None and pos + 1 < n and k % 2:
                        s2[rng.randint(pos + 1, n - 1)] = n2
                    if pos is not None and k % 5 == 0:
                        s2[pos] = n2
                    s2 = bytes(s2)
                    e = [i for i in (s2.find(bytes([nd])),
                                     s2.find(bytes([n2]))) if i >= 0]
                    C.add("memchr2", [hx(s2), str(nd), str(n2)],
                          min(e) if e else -1, pad=nd, shift=shift)
                    # needle-less scans: the "hit" is a high / special byte
                    hb = (0x80, 0xFF, 0xC3)[k % 3]
                    a = bytearray(rng.choice(b"axyz0 .\x00\x7f") for _ in range(n))
                    if pos is not None:
                        a[pos] = hb
                    C.add("ascii", [hx(bytes(a))], int(pos is None), pad=hb,
                          shift=shift)
                    sb = SPECIALS[k % 4]  # '"' ',' CR LF
                    qfill = [0x21, 0x23, 0x2B, 0x2D, 0x0C, 0x0E, 0x09, 0x0B,
                             0xA2, 0xAC, 0x8D, 0x8A, 0x00, 0x7F, 0x80, 0xFF,
                             0x61, 0x7C]
                    q = bytearray(rng.choice(qfill) for _ in range(n))
                    if mode == 2:
                        q = bytearray(rng.choice(b"axyz0 .") for _ in range(n))
                    for h in _hits(rng, n, pos, nhits, True):
                        q[h] = sb if h == pos else SPECIALS[rng.randrange(4)]
                    q = bytes(q)
                    nq = q.count(b'"')
                    need = int(any(b in q for b in b',"\n\r'))
                    C.add("csv_needs_quote", [hx(q)], "%d %d" % (need, nq),
                          pad=sb, shift=shift)
                    C.add("csv_cell_len", [hx(q)],
                          len(q) + nq + 2 if need else len(q), pad=sb,
                          shift=shift)
                    if all(b < 0x80 for b in q):
                        cell = pyoracle_csv.format_cell(q.decode("ascii"))
                    else:
                        cell = (b'"' + q.replace(b'"', b'""') + b'"') if need \
                            else q
                    C.add("csv_cell_write", [hx(q)], hx(cell), pad=sb,
                          shift=shift, alloc=len(cell))
    # memcpy: every length x source alignment x destination alignment
    for n in range(73):
        for shift in range(8):
            for doff in range(8):
                s = bytes(rng.randrange(256) for _ in range(n))
                C.add("memcpy", [hx(s), str(doff)], hx(s), pad=0xEE,
                      shift=shift, alloc=n + 8)
    for cap in (64, 300):
        for n in (0, 10, 300):
            s = bytes(rng.randrange(1, 128) for _ in range(n))
            C.add("memcpy", [hx(s), "3"], hx(s), cap=cap, alloc=n + 8)
            subj = s + b","
            cell = b'"' + subj.replace(b'"', b'""') + b'"'
            C.add("csv_cell_write", [hx(subj)], hx(cell), cap=cap,
                  alloc=len(cell))


# ---- string ops ---------------------------------------------------------------------

def _idx_set(n):
    return sorted({-n - 1, -n, -1, 0, n - 1, n, n + 1, 1 << 62, -(1 << 62)})


def gen_strings(C, rng, n_rand):
    pairs = list(RC.OVERLAP)
    hay = RC.small_strings(rng, n_rand)
    for i, s in enumerate(hay):
        r = i % 6
        if r == 0:
            nd = s                                    # needle == haystack
        elif r == 1:
            nd = s + rng.choice("ab")                 # longer than the haystack
        elif r == 2 and s:
            a = rng.randrange(len(s))
            nd = s[a:a + rng.randint(1, 6)]           # a real substring
        else:
            nd = rng.choice(RC.NEEDLES)
        pairs.append((s, nd))
    for i, (s, nd) in enumerate(pairs):
        rand = i >= len(RC.OVERLAP)
        pad = ord(nd[0]) if nd else 0x61
        kw = dict(pad=pad, rand=rand)
        a = [hx(s), hx(nd)]
        C.add("find", a, s.find(nd), **kw)
        C.add("rfind", a, s.rfind(nd), **kw)
        C.add("contains", a, int(nd in s), **kw)
        C.add("startswith", a, int(s.startswith(nd)), **kw)
        C.add("endswith", a, int(s.endswith(nd)), **kw)
        C.add("streq", a, int(s == nd), **kw)
        C.add("strcmp", a, (s > nd) - (s < nd), **kw)
        C.add("concat", a, hx(s + nd), alloc=len(s) + len(nd),
              cap=(HEAP_MAX, 64, 300)[i % 3], **kw)
        # replace to an empty, a shorter and a longer string
        for rep in ("", "c", nd + "cc"):
            out = s.replace(nd, rep)
            if nd == "":
                al = len(out)
            elif nd in s:
                al = len(out)
            else:
                al = None
            C.add("replace", [hx(s), hx(nd), hx(rep)], hx(out), alloc=al,
                  cap=(HEAP_MAX, HEAP_MAX, 64, 300)[(i + len(rep)) % 4], **kw)
        # split()[i]: -parts-1 .. parts, and the empty separator
        if i < 400 or i % 8 == 0:
            parts = len(s.split(nd)) if nd else 1
            for ix in range(-parts - 1, parts + 1):
                C.add("splitget", [hx(s), hx(nd), str(ix)],
                      py(lambda: hx(s.split(nd)[ix])), **kw)

    for s in ("", "a", "ab", "abcde", "abcdefgh", "abcdefghijklmnopq"):
        n = len(s)
        for i in _idx_set(n):
            C.add("getitem", [hx(s), str(i)], py(lambda: hx(s[i])))
        for lo in _idx_set(n):
            for hi in _idx_set(n):
                for hl in (0, 1):
                    for hh in (0, 1):
                        want = s[(lo if hl else None):(hi if hh else None)]
                        C.add("slice", [hx(s), str(lo), str(hl), str(hi),
                                        str(hh)], hx(want))
    # center: all four parities of (len, width), the left-bias quirk, fills of
    # length 0 and 2
    for n in range(0, 7):
        s = "xyzuvw"[:n]
        for w in list(range(-1, 12)) + [320]:
            for fill in ("*", " ", "", "ab"):
                want = py(lambda: hx(s.center(w, fill)))
                C.add_caps("center", [hx(s), str(w), hx(fill)], want,
                           alloc=w if (len(fill) == 1 and n < w) else None,
                           pad=0x2A)
    # s * k
    for n in range(73):
        s = "".join(rng.choice("abc") for _ in range(n))
        for k in (-1, 0, 1, 2, 64):
            C.add("strmul", [hx(s), str(k)], hx(s * k),
                  alloc=n * k if (n and k > 0) else None, pad=ord("a"))
        if n % 9 == 1:
            for k in (-1, 0, 1, 2, 5, 64):
                C.add_caps("strmul", [hx(s), str(k)], hx(s * k),
                           alloc=n * k if (n and k > 0) else None)
        if n:
            # host only: products that overflow i64 or exceed the heap must set
            # an error code, allocate nothing and write nothing
            q = (1 << 62) // n
            for k in (q - 1, q, q + 1, 2 * q, 2 * q + 1, 4 * q + 1, (1 << 63) // n,
                      (1 << 63) // n + 1, RC.I64_MAX, (1 << 64) // n + 1,
                      HEAP_MAX // n + 1, 1 << 32, (1 << 61) + 1):
                if 0 < k <= RC.I64_MAX and n * k > HEAP_MAX:
                    for cap in (HEAP_MAX, 300):
                        C.add("strmul", [hx(s), str(k)], "E114", cap=cap)
    # case ops / strip
    subj = RC.small_strings(rng, max(60, n_rand // 10),
                            alphabet="abzAZ@[`{ m09\t") + \
        ["", "a", "A", "z", "Z", "@[`{", "x" * 310, "Ab" * 155]
    for i, s in enumerate(subj):
        rand = i < len(subj) - 8
        for op, fn in (("lower", str.lower), ("upper", str.upper),
                       ("swapcase", str.swapcase)):
            C.add_caps(op, [hx(s)], hx(fn(s)), alloc=len(s), rand=rand)
        C.add_caps("capitalize_ix", [hx(s)],
                   py(lambda: hx(s[0].upper() + s[1:].lower())),
                   alloc=len(s) if s else None, rand=rand)
    for i, core in enumerate(["", "a", "a b", "ab" * 20, "\x1c", "\x85"]):
        for l in ("", " ", RC.WS, "\t\n"):
            for r in ("", " ", RC.WS, "\x0b\x0c\r"):
                s = l + core + r
                C.add("strip", [hx(s)], hx(s.strip(RC.WS)), pad=0x20)
    # int(s.replace(ch, '')): 30..33 bytes cross the stack-buffer cutoff
    for ln in list(range(0, 8)) + [29, 30, 31, 32, 33, 34, 40]:
        for v in range(12):
            digs = [rng.choice("0123456789") for _ in range(ln)]
            ncomma = (0, 1, 3, ln // 2, ln)[v % 5]
            for _ in range(min(ncomma, ln)):
                digs[rng.randrange(ln)] = ","
            if v == 7 and ln:
                digs[0] = "-"
            if v == 9 and ln:
                digs[rng.randrange(ln)] = "x"
            if v == 11 and ln > 2:
                digs[0] = " "
                digs[-1] = "\n"
            s = "".join(digs)
            cnt = s.count(",")
            al = (len(s) - cnt) if (len(s) > 31 and cnt) else None
            want = py(lambda: pyoracle.ref_int(s.replace(",", "")))
            for cap in (HEAP_MAX, 64, 300):
                C.add("int_drop", [hx(s), hx(",")], want, pad=0x2C, cap=cap,
                      alloc=al)


# ---- parsers ------------------------------------------------------------------------

def _atoi_expect(s):
    ok, v = pyoracle.fast_atoi64(s)
    return "0 %d" % v if ok else str(EC_NULL if s == "" else EC_I64PARSE)


def _atod_expect(s):
    ok, v = pyoracle.fast_atod(s)
    return "0 %s" % fexp(v) if ok else str(EC_NULL if s == "" else EC_F64PARSE)


def gen_parsers(C, rng, n_rand):
    ints = RC.INT_EDGE + RC.ws_wrapped(RC.INT_EDGE)
    floats = (RC.FLOAT_EDGE + RC.NANINF + RC.INT_EDGE +
              RC.ws_wrapped(RC.FLOAT_EDGE[:40] + RC.NANINF[:30]))
    rnd = RC.long_mantissas(rng, n_rand)
    rints = []
    for _ in range(n_rand // 4):
        rints.append(rng.choice(["", "-", "-", "+"]) + "".join(
            rng.choice("0123456789") for _ in range(rng.choice(
                [1, 5, 17, 18, 19, 20, 21, 25]))))
    bools = ["true", "True", "TRUE", "t", "T", "yes", "YES", "y", "1", "false",
             "False", "f", "no", "No", "n", "0", "", "tru", "truee", "2", "on",
             "ye", "falsee", " true ", "\tno\n", "tr ue", "yess", "nn", "00"]

    def one(s, rand, shift):
        kw = dict(pad=0x30, rand=rand, shift=shift)
        t = s.strip(RC.WS)
        C.add("atoi", [hx(s)], _atoi_expect(s), **kw)
        C.add("atod", [hx(s)], _atod_expect(s), **kw)
        C.add("cell_i64", [hx(s)], _atoi_expect(t), **kw)
        C.add("cell_f64", [hx(s)], _atod_expect(t), **kw)
        C.add("int_str", [hx(s)], py(lambda: pyoracle.ref_int(s)), **kw)
        C.add("float_str", [hx(s)], py(lambda: fexp(pyoracle.ref_float(s))),
              **kw)

    seen = set()
    for s in ints + floats:
        if s in seen:
            continue
        seen.add(s)
        for shift in range(8):  # every alignment
            one(s, False, shift)
    for i, s in enumerate(rnd + rints):
        one(s, True, i % 8)
    for s in bools + RC.ws_wrapped(bools[:12]) + RC.INT_EDGE[:6]:
        b = pyoracle_csv._try_bool(s)
        for _ in range(8):
            C.add("cell_bool", [hx(s)],
                  str(EC_BOOLPARSE) if b is None else "0 %d" % b, pad=0x74)


# ---- arithmetic ---------------------------------------------------------------------

def _i64(v):
    return v if RC.I64_MIN <= v <= RC.I64_MAX else "E%d" % EC[OverflowError]


def gen_arith(C, rng, n_cand, n_plain, counts):
    pairs, n_div, n_mod = RC.decimal_pairs(rng, n_cand, n_plain)
    counts["floordiv_divergent"] = n_div
    counts["mod_divergent"] = n_mod
    special = [(a, b) for a in RC.FLOAT_SPECIAL for b in RC.FLOAT_SPECIAL]
    for _ in range(300):  # |a| < |b| with mixed signs
        b = rng.choice([-1, 1]) * rng.uniform(1, 1e6)
        a = rng.choice([-1, 1]) * rng.uniform(0, abs(b))
        special.append((a, b))
    for i, (a, b) in enumerate(special + pairs):
        rand = i >= len(special) + n_div + n_mod
        args = [fx(a), fx(b)]
        C.add("floordiv_f64", args, py(lambda: fexp(a // b)), rand=rand)
        C.add("mod_f64", args, py(lambda: fexp(a % b)), rand=rand)
        if i % 4 == 0 or not rand:
            C.add("truediv", args, py(lambda: fexp(a / b)), rand=rand)
    for x in RC.INT_F64:
        C.add("int_f64", [fx(x)], py(lambda: _i64(int(x))))
    ipairs = list(RC.I64_DIV)
    for _ in range(2000):
        ipairs.append((rng.randint(RC.I64_MIN, RC.I64_MAX) >> rng.randrange(64),
                       rng.randint(RC.I64_MIN, RC.I64_MAX) >> rng.randrange(64)))
    for i, (a, b) in enumerate(ipairs):
        rand = i >= len(RC.I64_DIV)
        C.add("floordiv_i64", [str(a), str(b)], py(lambda: _i64(a // b)),
              rand=rand)
        C.add("mod_i64", [str(a), str(b)], py(lambda: _i64(a % b)), rand=rand)


# ---- formatting ---------------------------------------------------------------------

def gen_format(C, rng, n_doubles):
    for v in RC.INT_FMT:
        s = str(v)
        C.add("i64_digits", [str(v)], len(s))
        C.add("i64_write", [str(v)], hx(s), alloc=len(s))
        C.add_caps("str_i64", [str(v)], hx(s), alloc=len(s))
        for w in range(23):
            t = "%0*d" % (w, v)
            C.add("fmt0d", [str(w), str(v)], hx(t), alloc=len(t))
    for v in (0, -7, 42, RC.I64_MIN):
        for w in (0, 5, 300, 320):
            t = "%0*d" % (w, v)
            C.add_caps("fmt0d", [str(w), str(v)], hx(t), alloc=len(t))
    fits = pyoracle_csv._f64_fits_device
    edges = RC.fmt_edges(fits)
    assert any(fits(v) for v in edges[-50:]) and \
        any(not fits(v) and math.isfinite(v) for v in edges[-50:])
    for i, v in enumerate(edges + RC.fmt_mix(rng, n_doubles)):
        # the oracle's range predicate, anchored on CPython's own digits
        assert fits(v) == (math.isfinite(v) and
                           int(("%f" % abs(v)).replace(".", "")) < 1 << 63), v
        if fits(v):
            t = "%f" % v
            want = "0 %d %s" % (len(t), hx(t))
        else:
            want = "7"
        C.add("f64_csv", [fx(v)], want, rand=i >= len(edges))


# ---- the CSV byte walk --------------------------------------------------------------

ROW_ALPHA = b'ab,"\r\n x9\xc3\x00-#\x0e|}'


def gen_rows(C, rng, n_rows):
    """The row generator of host_rt_test.cpp, on this side, so the C walk and
    the oracle's split_cells see the same bytes."""
    fixed = [b"", b",", b",,", b'"', b'""', b'"a"', b'"a",b', b'"a"x,b',
             b'"a""b",c', b'a"b,c', b'"abc', b'a,"b,c",d', b'\xc3\xa9,x',
             b'"\xc3",x', b'a|b|"c|d"|e', b'a\rb,c', b'"a","b"', b'"a",',
             b',"a"', b'"a""', b'"a"""', b'""""']
    for i in range(len(fixed) * 8 + n_rows):
        if i < len(fixed) * 8:
            row = fixed[i // 8]
        else:
            n = rng.randrange(300)
            row = bytearray()
            for _ in range(n):
                if rng.randrange(100) < 80:
                    c = ROW_ALPHA[rng.randrange(len(ROW_ALPHA))]
                else:
                    c = 0x61 + rng.randrange(26)
                if c == 0x0A and rng.random() < 0.5:
                    c = 0x71
                row.append(c)
            row = bytes(row)
        row = row.rstrip(b"\r\n")  # the loader strips the row terminator
        delim = b"|" if i % 8 == 7 else b","
        cells, flags = pyoracle_csv.split_cells(row, delim)
        hi = int(any(b >= 0x80 for b in row))
        C.add("csv_row", [hx(row), str(delim[0])],
              "%d %d %d %s" % (hi, flags & 6, len(cells),
                               " ".join(hx(c) for c in cells)),
              pad=delim[0], rand=i >= len(fixed) * 8)


# ---- driver -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    rng = random.Random(20241107)
    C = Cases()
    counts = {}
    gen_scans(C, rng)
    gen_strings(C, rng, 3000)
    gen_parsers(C, rng, 12000)
    gen_arith(C, rng, 400000, 20000, counts)
    gen_format(C, rng, 200000)
    gen_rows(C, rng, 20000)
    return C, counts


def _build(tmp_path, name, flags):
    exe = os.path.join(str(tmp_path), name)
    # -ffp-contract=off like the device build (tpx_abi.cpp): the per-digit
    # float() accumulation must not fuse
    subprocess.check_call(["g++"] + flags + ["-ffp-contract=off", "-o", exe, SRC])
    return exe


def _norm(op, line):
    """Any NaN equals any NaN: fold a NaN bit pattern to 'NAN'."""
    if op in FLOAT_RESULT:
        t = line.rsplit(" ", 1)
        if len(t[-1]) == 16:
            try:
                v = RC.from_bits(int(t[-1], 16))
            except ValueError:
                return line
            if v != v:
                t[-1] = "NAN"
                return " ".join(t)
    return line


def _run_and_check(exe, C, keep, timeout):
    idx = [i for i in range(len(C.lines)) if keep(i)]
    inp = "\n".join(C.lines[i] for i in idx) + "\n"
    p = subprocess.run([exe], input=inp.encode(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:].decode(),
                               p.stderr[-4000:].decode())
    out = p.stdout.decode().split("\n")
    assert out[-2] == "OK" and len(out) == len(idx) + 2, out[-5:]
    print("cases per op:")
    print(p.stderr.decode())
    per_op = dict(ln.split() for ln in p.stderr.decode().strip().split("\n"))
    for op in ALL_OPS:
        assert int(per_op.get(op, 0)) > 0, "no case ran for %s" % op
    bad = []
    for j, i in enumerate(idx):
        op = C.lines[i].split(" ", 1)[0]
        if _norm(op, out[j]) != C.expect[i]:
            bad.append((C.lines[i], "got " + out[j], "want " + C.expect[i]))
    by_op = {}
    for b in bad:
        by_op.setdefault(b[0].split(" ", 1)[0], []).append(b)
    assert not bad, "%d wrong; first per op: %r" % (
        len(bad), {k: v[:3] for k, v in by_op.items()})
    return len(idx)


def test_divergent_pair_floors(cases):
    """The float // and % vectors cannot quietly lose their teeth: at least
    500 pairs where floor(a/b) != a//b, and 500 where fmod's zero sign differs
    from CPython's %."""
    _C, counts = cases
    print(counts)
    assert counts["floordiv_divergent"] >= 500, counts
    assert counts["mod_divergent"] >= 500, counts


def test_runtime_matches_cpython(cases, tmp_path):
    C, _ = cases
    exe = _build(tmp_path, "host_rtops", ["-O2", "-Wall"])
    n = _run_and_check(exe, C, lambda i: True, 600)
    n_f64 = sum(1 for ln in C.lines if ln.startswith("f64_csv "))
    assert n_f64 >= 200000, n_f64
    print("checked %d cases" % n)


def test_runtime_under_sanitizers(cases, tmp_path):
    """Same cases under ASan+UBSan: every op and every edge list stays, only
    the random volume shrinks (one random case in 8)."""
    C, _ = cases
    exe = _build(tmp_path, "host_rtops_san",
                 ["-O1", "-g", "-fsanitize=address,undefined",
                  "-fno-sanitize-recover=all"])
    n = _run_and_check(exe, C, lambda i: not C.rand[i] or i % 8 == 0, 900)
    print("checked %d cases under sanitizers" % n)

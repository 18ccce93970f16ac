"""Edge lists shared by the host differential harness (test_host_rtops.py) and
its device slice (test_gpu_rtops.py): the hardest vectors of every scalar
runtime helper family. Pure data + tiny generators; imports nothing from the
engine."""
import math
import struct

WS = " \t\n\r\x0b\x0c"
I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1


def dbits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def same_float(a, b):
    """Bit-pattern equality; any NaN equals any NaN."""
    if a != a or b != b:
        return a != a and b != b
    return dbits(a) == dbits(b)


# ---- int()/float() strings --------------------------------------------------------

INT_EDGE = ["", "-", "+", "+5", "5", "-5", "007", "-0", "12x", "x12", "1 2",
            "--1", "-+1", "1-", "0x10", "1_0", "1.0", "1e3"]
# 18-, 19- and 20-digit integers either side of +-2^63 (wrap mod 2^64)
for _v in (10**17, 10**18 - 1, 10**18, I64_MAX - 1, I64_MAX, I64_MAX + 1,
           I64_MAX + 2, 9999999999999999999, 10**19, (1 << 64) - 1, 1 << 64,
           (1 << 64) + 1, 99999999999999999999, 18446744073709551615 + 7):
    INT_EDGE += [str(_v), "-" + str(_v)]

FLOAT_EDGE = ["", "-", "+", "+5", ".", "-.", "+.", "1.", ".5", "-.5", "1e",
              "1e-", "1e+", "e5", ".e5", "1.e5", " 1 ", "1 2", "1..2", "1.2.3",
              "1e5.", "1e5e5", "0", "-0", "-0.0", "0.0", "+0.0", "1e-0",
              "3.25", "-1e3", "1E3", "1E+3", "1x", "x", "0x10", "1_0",
              "123456789.123456789", "0.1", "0.2", "0.3", "1.15", "2.675",
              "179769313486231570000000000000000000000", "4.9e-324",
              "2.2250738585072014e-308", "1.7976931348623157e308"]
EXPONENTS = [0, 7, 8, 49, 50, 307, 308, 309, 400, 4294967295, 4294967296,
             4294967297]
for _e in EXPONENTS:
    for _m in ("1", "1.5", "9.99", "0.001", "123456789012345678"):
        FLOAT_EDGE += ["%se%d" % (_m, _e), "%se-%d" % (_m, _e),
                       "-%sE+%d" % (_m, _e)]


def _casemixes(word):
    out = []
    for mask in range(1 << len(word)):
        out.append("".join(c.upper() if (mask >> i) & 1 else c
                           for i, c in enumerate(word)))
    return out


NANINF = _casemixes("nan") + _casemixes("inf") + _casemixes("infinity")
for _w in ("n", "na", "i", "in", "infi", "infin", "infinit", "nanx", "infx",
           "infinityx", "nann", "infinf", "naninf"):
    NANINF.append(_w)
for _w in ("nan", "inf", "infinity", "NaN", "Inf", "INFINITY"):
    NANINF += ["+" + _w, "-" + _w]


def long_mantissas(rng, n):
    """17..25 significant digits in the integer and/or the fraction part: the
    per-digit roundings of fast_atod must match the oracle's."""
    out = []
    for _ in range(n):
        ip = "".join(rng.choice("0123456789")
                     for _ in range(rng.choice([0, 1, 3, 17, 18, 19, 20, 21,
                                                22, 23, 24, 25])))
        fp = "".join(rng.choice("0123456789")
                     for _ in range(rng.choice([0, 1, 2, 6, 17, 18, 19, 20,
                                                21, 22, 23, 24, 25])))
        s = rng.choice(["", "", "-", "+"]) + ip
        if fp or rng.random() < 0.2:
            s += "." + fp
        r = rng.random()
        if r < 0.3:
            s += rng.choice("eE") + rng.choice(["", "-", "+"]) + \
                str(rng.choice(EXPONENTS[:9] + [1, 2, 15, 22, 100]))
        out.append(s)
    return out


def ws_wrapped(strings):
    """Every python whitespace byte at both ends, plus interior whitespace."""
    out = []
    for k, s in enumerate(strings):
        w = WS[k % len(WS)]
        out += [w + s, s + w, w + s + w, WS + s + WS]
        if len(s) >= 2:
            out.append(s[:1] + w + s[1:])
    return out


# ---- floats -----------------------------------------------------------------------

def old_mod(a, b):
    r = math.fmod(a, b)
    if r != 0.0 and ((r < 0.0) != (b < 0.0)):
        r += b
    return r


def decimal_pairs(rng, n_candidates, n_keep_plain):
    """One- and two-decimal (a, b) pairs. Returns (pairs, n_div, n_mod): every
    candidate where floor(a/b) != a//b or where fmod's zero sign differs from
    CPython's % is kept, plus n_keep_plain ordinary ones."""
    div, mod, plain = [], [], []
    for i in range(n_candidates):
        # every 4th pair is whole/half/quarter-valued: exact zero remainders
        if i % 4 == 0:
            a = rng.randint(-400, 400) / rng.choice([1, 2, 4])
            b = rng.randint(-40, 40) / rng.choice([1, 2, 4])
        else:
            a = rng.randint(-10000, 10000) / rng.choice([10, 100])
            b = rng.randint(-1000, 1000) / rng.choice([10, 100])
        if b == 0.0:
            continue
        if math.floor(a / b) != a // b:
            div.append((a, b))
        elif dbits(old_mod(a, b)) != dbits(a % b):
            mod.append((a, b))
        else:
            plain.append((a, b))
    rng.shuffle(plain)
    return div + mod + plain[:n_keep_plain], len(div), len(mod)


FLOAT_SPECIAL = [0.0, -0.0, math.inf, -math.inf, math.nan, 5e-324, -5e-324,
                 2.2250738585072014e-308, -2.2250738585072009e-308, 1.0, -1.0,
                 0.5, -0.5, 3.0, -3.0, 0.1, -0.1, 1e308, -1e308, 1e-300,
                 29.0, 0.2, 48.0, 0.4, -52.0, -5.2, -4.0, 2.0, 7.5, -2.5]


def _neighbours(x, k=2):
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo = math.nextafter(lo, -math.inf)
        hi = math.nextafter(hi, math.inf)
        out += [lo, hi]
    return out


INT_F64 = []
for _x in (2.0**63, -2.0**63, 2.0**62, -2.0**62, 2.0**53, -2.0**53, 1.0, -1.0,
           0.0, 1e18, -1e18):
    INT_F64 += _neighbours(_x)
INT_F64 += [-0.0, 0.5, -0.5, 0.999, -0.999, 1e19, -1e19, 1e300, math.inf,
            -math.inf, math.nan, 5e-324, 123456.789, -123456.789]


# ---- ints -------------------------------------------------------------------------

INT_FMT = [0, 1, -1, I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1]
for _k in range(19):
    for _d in (-1, 0, 1):
        _v = 10**_k + _d
        INT_FMT += [_v, -_v]
INT_FMT = sorted(set(v for v in INT_FMT if I64_MIN <= v <= I64_MAX))

I64_DIV = [(a, b) for a in range(-3, 4) for b in range(-3, 4)]
for _a in (I64_MIN, I64_MIN + 1, I64_MIN + 2, I64_MAX, I64_MAX - 1, 7, -7):
    for _b in (1, -1, 2, -2, 0, 3, -3, I64_MAX, I64_MIN):
        I64_DIV.append((_a, _b))
        I64_DIV.append((_b, _a))


# ---- %f doubles -------------------------------------------------------------------

def fmt_mix(rng, n):
    """The value mix of test_f64fmt_cpu.py."""
    out = []
    for _ in range(n):
        c = rng.random()
        if c < 0.3:
            v = rng.uniform(-1e13, 1e13)
        elif c < 0.6:
            v = rng.uniform(-1000, 1000)
        elif c < 0.8:
            v = rng.uniform(-1e-5, 1e-5)
        else:
            v = from_bits(rng.getrandbits(64))
        out.append(v)
    return out


def fmt_edges(fits):
    """Sixth-decimal ties, signed zero, both sides of the accept limit
    (2^63 * 10^-6), subnormals, nan, inf. `fits` is the oracle's range
    predicate; the limit is located with it, not assumed."""
    out = [0.0, -0.0, 5e-7, 1.5e-6, 2.5e-6, -5e-7, -1.5e-6, -2.5e-6, 5e-324,
           -5e-324, 2.2250738585072014e-308, 1e-7, 9.2e12, 1.9e13, 1e300,
           123456789.123456789, math.nan, math.inf, -math.inf, 0.9999995,
           0.99999949999, 999999.9999995, 1e-6, 4.9999999e-7, 5.0000001e-7]
    for k in range(1, 400, 2):  # (2k+1)/128: exact ties at the 6th decimal
        out += [k / 128.0, -k / 128.0, 1000.0 + k / 128.0,
                k / 128.0 + 4194304.0]
    for k in range(1, 64, 2):   # ties at larger magnitude (fewer fraction bits)
        out += [k / 128.0 + 2.0**36, -(k / 128.0 + 2.0**40)]
    x = 9223372036854.0
    assert fits(x)
    while fits(x):
        x = math.nextafter(x, math.inf)
    lim = x  # smallest rejected
    for v in _neighbours(lim, 12):
        out += [v, -v]
    return out


# ---- strings ----------------------------------------------------------------------

def small_strings(rng, n, alphabet="ab", maxlen=72):
    out = []
    for _ in range(n):
        ln = rng.choice([0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40,
                         63, 64, 65, 71, 72, rng.randint(0, maxlen)])
        out.append("".join(rng.choice(alphabet) for _ in range(ln)))
    return out


NEEDLES = ["", "a", "b", "ab", "ba", "aa", "aab", "aba", "bb", "abab", "aaaa",
           "c", "ac"]
OVERLAP = [("aaab", "aab"), ("aaaaa", "aa"), ("", ""), ("", "a"), ("a", ""),
           ("a", "a"), ("ab", "abc"), ("abc", "abc"), ("abab", "ab"),
           ("aaaa", "a"), ("baaab", "aa"), ("ab" * 36, "ba"),
           ("a" * 72, "a" * 8), ("a" * 71 + "b", "ab")]

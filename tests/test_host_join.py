"""Host-compiled check of the device join table (csrc/tpx_join.hip.h):
tests/host_join_test.cpp builds slot tables sequentially with the header's
own insert functions and answers probes with its probe functions. Every build
key must probe to its own row and every absent key to -1, over the key
vectors of tests/join_table_cases.py (special int64 values, wrapping
colliding-home sets, prefixes, long and multibyte strings). The same program
is run a second time under ASan+UBSan (a plain executable, nothing loaded
into Python)."""
import os
import subprocess

import pytest

from tests import join_table_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, name, flags):
    exe = os.path.join(str(tmp_path), name)
    subprocess.check_call(["g++"] + flags + [
        "-o", exe, os.path.join(HERE, "host_join_test.cpp")])
    return exe


def _hex(s):
    b = s.encode("utf-8")
    return b.hex() if b else "-"


def _check_all(exe):
    lines, expect = [], []
    for n in C.SIZES:
        keys, absent = C.i64_case(n)
        rows = {k: i for i, k in enumerate(keys)}
        assert len(rows) == n
        lines.append("I %d %s" % (n, " ".join(map(str, keys))))
        expect.append(("B", C.table_size(n), n, 0))
        for k in keys + absent:
            lines.append("p %d" % k)
            expect.append(rows.get(k, -1))
        skeys, sabsent = C.str_case(n)
        srows = {k: i for i, k in enumerate(skeys)}
        assert len(srows) == n
        lines.append("S %d %s" % (n, " ".join(map(_hex, skeys))))
        expect.append(("B", C.table_size(n), n, 0))
        for k in skeys + sabsent:
            lines.append("q %s" % _hex(k))
            expect.append(srows.get(k, -1))
    out = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(),
                         stdout=subprocess.PIPE, check=True,
                         timeout=120).stdout.decode().split("\n")
    assert out[-2] == "OK", out[-5:]
    got = []
    for ln in out[:-2]:
        f = ln.split()
        got.append(("B",) + tuple(map(int, f[1:])) if f[0] == "B"
                   else int(f[0]))
    assert len(got) == len(expect)
    bad = [(ln, g, e) for ln, g, e in zip(lines, got, expect) if g != e]
    assert not bad, bad[:5]
    return len(got)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("host_join"), "host_join_test",
                  ["-O2", "-Wall"])


def test_probe_results_match_dict(exe):
    assert _check_all(exe) > 4000


def test_case_vectors_hold_what_they_promise():
    for n in C.SIZES:
        if n < 17:
            continue
        ts = C.table_size(n)
        keys, absent = C.i64_case(n)
        for k in (0, -1, C.INT64_MIN, C.INT64_MAX, C.POISON_I64):
            assert k in keys
        assert sum(C.hash_i64(k) & (ts - 1) == ts - 1 for k in keys) >= 12
        assert absent and not set(absent) & set(keys)
        skeys, sabsent = C.str_case(n)
        for s in ("", "a", "ab", "abc", "abd", "x" * 299 + "y", "日本"):
            assert s in skeys
        assert sum(C.hash_bytes(s.encode()) & (ts - 1) == ts - 1
                   for s in skeys) >= 12
        assert sabsent and not set(sabsent) & set(skeys)


def test_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "host_join_asan",
                 ["-O1", "-g", "-fsanitize=address,undefined",
                  "-fno-sanitize-recover=all"])
    _check_all(exe)

"""CPU checks behind the kernel-level GPU tests (tests/test_gpu_kernels.py):

- the source the launch harness compiles (tests/hipkern.py) still compiles for
  gfx950 with the product's hipRTC options and holds every fixed kernel;
- the plain models of tests/kern_models.py agree with independent references
  on the very inputs the GPU tests use.
"""
import math
import os

import numpy as np
import pytest

from oracle import pyoracle_csv
from tests import hipkern
from tests import kern_models as M
from tuplex_amd import codegen


def test_harness_source_compiles_for_gfx950():
    if not os.path.exists(hipkern.LIB):
        pytest.skip("libtpx_gpu.so not built")
    assert hipkern.HIPRTC_OPTS == [b"--offload-arch=gfx950", b"-O3",
                                   b"-std=c++17", b"-ffp-contract=off"]
    code = hipkern.compile_code()
    assert code[:4] == b"\x7fELF" or b"\x7fELF" in code[:4096]
    for name in hipkern.KERNELS:
        assert name.encode() in code, name


def test_harness_options_match_the_product():
    """The harness must compile with compile_hiprtc's option list."""
    src = open(os.path.join(os.path.dirname(hipkern.LIB), "csrc",
                            "tpx_abi.cpp")).read()
    body = src[src.index("static bool compile_hiprtc"):]
    body = body[:body.index("hiprtcCompileProgram")]
    for o in hipkern.HIPRTC_OPTS:
        assert ('"%s"' % o.decode()) in body, o
    assert body.count('"-') == len(hipkern.HIPRTC_OPTS)


# ---- rows -------------------------------------------------------------------

CASES = M.csv_cases() + [("ranged", M.ranged_emit_input(), False)]


def test_case_list_covers_the_edges():
    by = {n: d for n, d, _ in CASES}
    assert sorted(len(by["cut%d" % s]) for s in
                  (1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 12289)) == \
        [1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 12289]
    assert 40000 < len(by["random40k"]) < 42000
    assert len(by["random_exact_8192"]) == 8192
    for pos in (63, 64, 4095, 4096):
        assert by["quote_at_%d" % pos][pos] == 0x22
        assert by["close_at_%d" % pos][pos] == 0x22
    for pos in (63, 4095):
        assert by["escpair_at_%d" % pos][pos:pos + 2] == b'""'
    d = by["quoted_nl_at_4095"]
    assert d[4095] == 0x0A and 4096 not in M.row_ends(d)
    assert by["nl_at_63"][63] == 0x0A and 64 in M.row_ends(by["nl_at_63"])
    assert 4096 in M.row_ends(by["nl_at_4095"])
    assert 0 in M.rows_per_chunk(by["long_row"])
    assert by["all_quotes_chunk"][4096:8192] == b'"' * 4096
    assert b"\r\n" in by["crlf"]
    assert not by["no_trailing_newline"].endswith(b"\n")


def test_ranged_input_has_the_required_geometry():
    d = M.ranged_emit_input()
    assert len(d) >= 10 * M.CHUNK and len(d) < 48 * 1024
    ends = M.row_ends(d)
    lens = [b - a for a, b in zip([0] + ends, ends)]
    assert max(lens) > M.CHUNK and min(lens) < 10
    assert any(e % M.CHUNK == 0 for e in ends)       # newline on byte 4095
    rc = M.rows_per_chunk(d)
    assert 0 in rc
    # some chunk's last valid newline is followed by quoted newlines
    last = {}
    for e in ends:
        last[(e - 1) // M.CHUNK] = e
    assert any(b"\n" in d[e:(c + 1) * M.CHUNK] for c, e in last.items())


@pytest.mark.parametrize("name,data,valid", CASES, ids=[c[0] for c in CASES])
def test_row_model_matches_split_rows(name, data, valid):
    rows = pyoracle_csv.split_rows(data)
    ends, pos = [], 0
    for r in rows:
        pos += len(r)
        ends.append(pos)
    if rows and not (rows[-1].endswith(b"\n") and
                     ends == M.row_ends(data)):
        ends.pop()      # split_rows also returns a trailing incomplete row
    assert M.row_ends(data) == ends
    # text mode: every newline
    assert M.row_ends(data, 0) == [i + 1 for i, b in enumerate(data)
                                   if b == 0x0A]
    assert sum(M.rows_per_chunk(data)) == len(ends)


@pytest.mark.parametrize("name,data,valid", CASES, ids=[c[0] for c in CASES])
def test_chunk_stats_compose_to_rows(name, data, valid):
    """Chunk stats + a host scan of q select exactly the rows per chunk."""
    for quotes_on in (1, 0):
        q, c0, c1 = M.chunk_stats(data, quotes_on)
        assert sum(q) == (data.count(b'"') if quotes_on else 0)
        assert sum(c0) + sum(c1) == data.count(b"\n")
        qs, _ = M.exscan(q)
        rc = [b if s & 1 else a for s, a, b in zip(qs, c0, c1)]
        assert rc == M.rows_per_chunk(data, quotes_on)


# ---- scan / reduce -------------------------------------------------------------

def test_exscan_model():
    assert M.exscan([]) == ([], 0)
    assert M.exscan([5]) == ([0], 5)
    v = [3, -1, 4, 1, -5]
    assert M.exscan(v) == ([0, 3, 2, 6, 7], 2)
    big = [2 ** 62, 2 ** 62, 2 ** 62, 7]
    out, tot = M.exscan(big)
    assert out == [0, 2 ** 62, -2 ** 63, -2 ** 62] and tot == -2 ** 62 + 7
    rng = np.random.default_rng(1)
    a = rng.integers(-2 ** 40, 2 ** 40, 5000)
    out, tot = M.exscan(a)
    ref = np.concatenate([[0], np.cumsum(a)[:-1]])
    assert out == ref.tolist() and tot == int(a.sum())
    out2, tot2 = M.exscan_array(a)
    assert out2.tolist() == out and tot2 == tot
    w = np.array(big, dtype=np.int64)
    out2, tot2 = M.exscan_array(w)
    assert (out2.tolist(), tot2) == M.exscan(big)


def test_sum_i64_wraps():
    assert M.sum_i64([2 ** 63 - 1, 1], [1, 1]) == -2 ** 63
    assert M.sum_i64([2 ** 63 - 1, 1], [1, 0]) == 2 ** 63 - 1
    assert M.sum_i64([-2 ** 63, -1], [1, 1]) == 2 ** 63 - 1


def test_reduce_grid():
    assert [M.reduce_grid(n) for n in (1, 2048, 2049, 262145, 2097152,
                                       2097153)] == [1, 1, 2, 129, 1024, 1024]


@pytest.mark.parametrize("n", M.REDUCE_SIZES)
@pytest.mark.parametrize("kind", ["random", "cancel"])
def test_order_model_within_fsum_bound(n, kind):
    vals = M.f64_values(kind, n, seed=n)
    for mk in ("all1", "random", "all0"):
        keep = M.keep_mask(mk, n, seed=n)
        got = M.reduce_f64_order(vals, keep, M.reduce_grid(n))
        ref, bound = M.fsum_bound(vals, keep)
        assert abs(got - ref) <= bound, (n, kind, mk, got, ref, bound)


def test_order_model_small_by_hand():
    # 1 block: thread t holds item t; the tree adds slot t+128 to t, ...
    vals = np.zeros(256)
    vals[0], vals[128], vals[1] = 1e16, 1.0, -1e16
    keep = np.ones(256, np.uint8)
    # (1e16 + 1.0) rounds to 1e16; then + (-1e16 + 0) -> 0.0
    assert M.reduce_f64_order(vals, keep, 1) == 0.0
    # slots 0 and 2 meet at o == 2 and cancel; slot 1 joins at o == 1
    vals = np.zeros(256)
    vals[0], vals[2], vals[1] = 1e16, -1e16, 1.0
    assert M.reduce_f64_order(vals, keep, 1) == 1.0
    # two rounds of one block: thread 0 sums items 0 and 256 first
    vals = np.zeros(300)
    vals[0], vals[256], vals[1] = 1e16, 1.0, -1e16
    assert M.reduce_f64_order(vals, np.ones(300, np.uint8), 1) == 0.0
    # special values and the mask
    v = np.array([1.0, np.nan, 2.0])
    assert M.reduce_f64_order(v, [1, 0, 1], 1) == 3.0
    assert math.isnan(M.reduce_f64_order(v, [1, 1, 1], 1))
    v = np.array([np.inf, 1.0, -np.inf])
    assert math.isnan(M.reduce_f64_order(v, [1, 1, 1], 1))
    assert M.reduce_f64_order(v, [1, 1, 0], 1) == np.inf


# ---- hashes ---------------------------------------------------------------------

def test_hash_replicas_recorded_values():
    # murmur3 fmix64, and FNV-1a with the header's own offset basis
    # 1469598103934665603 (not the standard 64-bit basis)
    assert M.hash_i64(0) == 0
    assert M.hash_i64(1) == 0xb456bcfc34c2cb2c
    assert M.hash_i64(-1) == M.hash_i64(M.M64) == 0x64b5720b4b825f21
    assert M.hash_i64(-2 ** 63) == 0x8f780810af31a493
    assert M.jhash_bytes(b"") == 1469598103934665603 == 0x14650fb0739d0383
    assert M.jhash_bytes(b"a") == 0x44bd8ad473cd9906
    assert M.jhash_bytes(b"foobar") == 0x88fad7c0a8ff07f2
    for s in (b"", b"x", b"hello world", bytes(range(256))):
        assert M.jhash_bytes(s) == codegen.StageCodegen._jhash_bytes(s)
    # fmix64 is a bijection: inverting it returns the key
    def unmix(x):
        inv1 = pow(0xff51afd7ed558ccd, -1, 1 << 64)
        inv2 = pow(0xc4ceb9fe1a85ec53, -1, 1 << 64)
        x ^= x >> 33
        x = (x * inv2) & M.M64
        x ^= x >> 33
        x = (x * inv1) & M.M64
        x ^= x >> 33
        return x
    for k in (1, 2, 12345, 2 ** 63 - 1, 2 ** 64 - 1):
        assert unmix(M.hash_i64(k)) == k


def test_collision_search():
    ks = M.colliding_i64_keys(15, 15, 6)
    assert len(set(ks)) == 6 and all(M.hash_i64(k) & 15 == 15 for k in ks)
    ss = M.colliding_str_keys(63, 0, 5)
    assert len(set(ss)) == 5 and all(M.jhash_bytes(s) & 63 == 0 for s in ss)


def test_group_sum():
    g = M.group_sum([1, 2, 1, -1], [10, 20, 30, 40], [1, 1, 1, 0])
    assert g == {1: [2, 40], 2: [1, 20]}
    g = M.group_sum([7, 7], [2 ** 63 - 1, 1], [1, 1], wrap=True)
    assert g == {7: [2, -2 ** 63]}

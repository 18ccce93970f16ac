"""Kernel-level differential tests of the fixed cooperative kernels of
tpx_rt.hip.h: CSV boundary scan, exclusive scan, aggregate reduce and hash
aggregation, launched directly (tests/hipkern.py) and compared with the plain
models of tests/kern_models.py.

Every launch uses arguments the product could pass: block 256, power-of-two
tables, buffers of the product's sizes. Output buffers are poisoned first and
carry a canary zone, which launch() checks.
"""
import functools
import math
import random

import numpy as np
import pytest

from tests import hipkern as H
from tests import kern_models as M

pytestmark = pytest.mark.gpu

I64 = np.int64
POISON = H.POISON_I64


def _i64s(buf, count=None, offset=0):
    return H.download(buf, I64, count, offset)


# =============================================================================
# CSV boundary scan
# =============================================================================

CSV_CASES = M.csv_cases()
# bytes after the input's end, inside the slack the product allocates (size +
# 80): a kernel that reads past `size` counts them
SLACK = b'"\n' * 40


def _nchunks(size):
    return (size + M.CHUNK - 1) // M.CHUNK


def _grid_w(nch):
    return min((nch + 3) // 4, 8192)     # csv_boundary_and_core


@functools.lru_cache(maxsize=None)
def _csv_dev(name):
    data = dict((n, d) for n, d, _ in CSV_CASES)[name]
    return data, H.upload(data + SLACK)


# Base alignment: every caller hands these kernels the start of an arena block
# or of a tpx_dev_alloc allocation (256-byte aligned), never an interior
# pointer, so the set runs at an aligned base only.
@pytest.mark.parametrize("quotes_on", [1, 0], ids=["quotes", "text"])
@pytest.mark.parametrize("name", [c[0] for c in CSV_CASES])
def test_csv_stats_select_emit(name, quotes_on):
    data, d_data = _csv_dev(name)
    size, nch = len(data), _nchunks(len(data))
    mq, m0, m1 = M.chunk_stats(data, quotes_on)
    mrc = M.rows_per_chunk(data, quotes_on)
    ends = M.row_ends(data, quotes_on)
    qscan, _ = M.exscan(mq)
    base, nrows = M.exscan(mrc)
    assert nrows == len(ends)
    d_qs = H.upload(np.array(qscan, I64))
    d_base = H.upload(np.array(base, I64))
    for grid in sorted({_grid_w(nch), 1, 2}):
        q, c0, c1 = H.alloc(nch * 8), H.alloc(nch * 8), H.alloc(nch * 8)
        H.launch("tpx_csv_chunk_stats", grid, 256,
                 [d_data, H.i64(size), H.i64(nch), q, c0, c1,
                  H.i32(quotes_on)])
        assert _i64s(q).tolist() == mq, ("q", grid)
        assert _i64s(c0).tolist() == m0, ("c0", grid)
        assert _i64s(c1).tolist() == m1, ("c1", grid)
        # select on the device's own counts, after a host scan of q
        rc = H.alloc(nch * 8)
        H.launch("tpx_csv_select_counts",
                 min((nch + 255) // 256, 8192) if grid != 2 else 2, 256,
                 [d_qs, c0, c1, rc, H.i64(nch)])
        assert _i64s(rc).tolist() == mrc, ("rc", grid)
        if nrows == 0:
            continue        # the product returns an empty result before emit
        offs = H.alloc((nrows + 1) * 8)
        H.launch("tpx_csv_emit_rows", grid, 256,
                 [d_data, H.i64(size), H.i64(nch), d_qs, d_base, offs,
                  H.i32(quotes_on), H.i64(0), H.i64(nrows)])
        assert _i64s(offs).tolist() == [0] + ends, ("row_offs", grid)


def test_csv_emit_ranged():
    """One ranged call writes all of row_offs[lo..hi] — what the main kernel
    for rows [lo, hi) reads — and nothing but correct values elsewhere.

    Before the skip test of tpx_csv_emit_rows became `base[c + 1] < row_lo`
    this failed for every lo that is a chunk's base: row_offs[lo] was left to
    the previous range's call, which runs on another stream."""
    data = M.ranged_emit_input()
    size, nch = len(data), _nchunks(len(data))
    assert nch >= 10
    mq, _, _ = M.chunk_stats(data)
    ends = M.row_ends(data)
    model = np.array([0] + ends, I64)
    qscan, _ = M.exscan(mq)
    base, nrows = M.exscan(M.rows_per_chunk(data))
    d_data = H.upload(data + SLACK)
    d_qs = H.upload(np.array(qscan, I64))
    d_base = H.upload(np.array(base, I64))
    offs = H.alloc((nrows + 1) * 8)
    edges = {0, 1, nrows - 1, nrows}
    for b in base:
        edges.update((b - 1, b, b + 1))
    edges = sorted(e for e in edges if 0 <= e <= nrows)
    idx = np.arange(nrows + 1)
    bad = []
    for lo in edges:
        for hi in edges:
            if hi <= lo:
                continue
            offs.fill(H.POISON)
            H.launch("tpx_csv_emit_rows", _grid_w(nch), 256,
                     [d_data, H.i64(size), H.i64(nch), d_qs, d_base, offs,
                      H.i32(1), H.i64(lo), H.i64(hi)])
            got = _i64s(offs)
            inside = (idx >= lo) & (idx <= hi)
            wrong_in = idx[inside & (got != model)]
            wrong_out = idx[~inside & (got != model) & (got != POISON)]
            if wrong_in.size or wrong_out.size:
                bad.append((lo, hi, wrong_in[:4].tolist(),
                            wrong_out[:4].tolist()))
    assert not bad, ("%d of the ranges wrong; (lo, hi, missing entries, "
                     "stray entries): %s" % (len(bad), bad[:6]))


# =============================================================================
# exclusive scan
# =============================================================================

SCAN_BLOCK = 2048
SCAN_KINDS = ["zeros", "ones", "mask01", "random40", "wrap"]
_NMAX = max(M.SCAN_SIZES)


@functools.lru_cache(maxsize=1)      # tests run kind by kind: 64 MB at a time
def _scan_input(kind):
    """(values, model scan) at the largest size; a smaller n uses the prefix,
    whose exclusive scan is the prefix of this one."""
    rng = np.random.default_rng(5)
    if kind == "zeros":
        v = np.zeros(_NMAX, I64)
    elif kind == "ones":
        v = np.ones(_NMAX, I64)
    elif kind == "mask01":
        v = (rng.random(_NMAX) < 0.5).astype(I64)
    elif kind == "random40":
        v = rng.integers(-2 ** 40, 2 ** 40, _NMAX, dtype=I64)
    else:   # partial sums pass 2^63 after a few items, again and again
        v = rng.integers(2 ** 61, 2 ** 62, _NMAX, dtype=I64)
    out, _ = M.exscan_array(v)
    return v, out


def _dev_scan(d_in, d_out, n):
    """tpx_scan_block / tpx_scan_add composed as dev_scan (tpx_abi.cpp)."""
    nblocks = (n + SCAN_BLOCK - 1) // SCAN_BLOCK
    sums = H.alloc(nblocks * 8)
    H.launch("tpx_scan_block", nblocks, 256, [d_in, d_out, sums, H.i64(n)])
    if nblocks > 1:
        sums_scan = H.alloc(nblocks * 8)
        _dev_scan(sums, sums_scan, nblocks)
        H.launch("tpx_scan_add", nblocks, 256, [d_out, sums_scan, H.i64(n)])


@pytest.mark.parametrize("n", M.SCAN_SIZES)
@pytest.mark.parametrize("kind", SCAN_KINDS)
def test_scan(kind, n):
    v, model = _scan_input(kind)
    extra = 64                       # out[n..] must keep its poison
    d_in = H.upload(v[:n])
    d_out = H.alloc((n + extra) * 8)
    _dev_scan(d_in, d_out, n)
    got = _i64s(d_out)
    assert np.array_equal(got[:n], model[:n]), \
        np.nonzero(got[:n] != model[:n])[0][:8]
    assert (got[n:] == POISON).all()
    # totals: this scan as `a`, a short one as `b`
    total = M.s64(int(model[n - 1]) + int(v[n - 1]))
    sv = np.array([5, -2, 9], I64)
    d_sin, d_sout = H.upload(sv), H.alloc(3 * 8)
    _dev_scan(d_sin, d_sout, 3)
    slot = H.alloc(16)
    H.launch("tpx_pair_total", 1, 256,
             [d_in, d_out, H.i64(n), d_sin, d_sout, H.i64(3), slot])
    assert _i64s(slot).tolist() == [total, 12]
    H.launch("tpx_pair_total", 1, 256,
             [d_sin, d_sout, H.i64(3), d_in, d_out, H.i64(n), slot.fill(H.POISON)])
    assert _i64s(slot).tolist() == [12, total]


def test_pair_total_empty_sides():
    sv = np.array([5, -2, 9], I64)
    d_in, d_out = H.upload(sv), H.alloc(3 * 8)
    _dev_scan(d_in, d_out, 3)
    assert _i64s(d_out).tolist() == [0, 5, 3]
    for na, nb, want in ((0, 3, [0, 12]), (3, 0, [12, 0]), (0, 0, [0, 0]),
                         (2, 1, [3, 5])):
        slot = H.alloc(16)
        H.launch("tpx_pair_total", 1, 256,
                 [d_in, d_out, H.i64(na), d_in, d_out, H.i64(nb), slot])
        assert _i64s(slot).tolist() == want, (na, nb)


# =============================================================================
# aggregate reduce
# =============================================================================

def _reduce(kind, vals, keep):
    """The product's two launches (run_core) -> the 8 result bytes."""
    n = len(vals)
    nb = M.reduce_grid(n)
    d_vals, d_keep = H.upload(vals), H.upload(keep)
    partials, out = H.alloc(nb * 8), H.alloc(8)
    H.launch("tpx_reduce_%s" % kind, nb, 256,
             [d_vals, d_keep, H.i64(n), partials])
    H.launch("tpx_reduce_%s_final" % kind, 1, 256, [partials, H.i64(nb), out])
    return H.download(out, np.float64 if kind == "f64" else I64)[0]


@pytest.mark.parametrize("mask", ["all0", "all1", "random"])
@pytest.mark.parametrize("n", M.REDUCE_SIZES)
def test_reduce_i64(n, mask):
    rng = np.random.default_rng(n)
    keep = M.keep_mask(mask, n, seed=n)
    for vals in (rng.integers(-2 ** 40, 2 ** 40, n, dtype=I64),
                 rng.integers(2 ** 61, 2 ** 62, n, dtype=I64)):   # wraps
        got = int(_reduce("i64", vals, keep))
        want = M.s64(sum(vals[keep.astype(bool)].tolist()))
        assert got == want


def _bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("mask", ["all0", "all1", "random"])
@pytest.mark.parametrize("n", M.REDUCE_SIZES)
def test_reduce_f64(n, mask):
    keep = M.keep_mask(mask, n, seed=n)
    for kind in ("random", "cancel"):
        vals = M.f64_values(kind, n, seed=n)
        got = float(_reduce("f64", vals, keep))
        order = M.reduce_f64_order(vals, keep, M.reduce_grid(n))
        ref, bound = M.fsum_bound(vals, keep)
        print("n=%d %s %s: device %r order %r fsum %r bound %r"
              % (n, mask, kind, got, order, ref, bound))
        assert _bits(got) == _bits(order), (kind, got, order)
        assert abs(got - ref) <= bound, (kind, got, ref, bound)


@pytest.mark.parametrize("n", [257, 262145])
def test_reduce_f64_special_values(n):
    base = M.f64_values("random", n, seed=3)
    ones = np.ones(n, np.uint8)
    mid = n // 2

    def run(edits, masked=()):
        v = base.copy()
        for i, x in edits:
            v[i] = x
        keep = ones.copy()
        for i in masked:
            keep[i] = 0
        got = float(_reduce("f64", v, keep))
        want = M.reduce_f64_order(v, keep, M.reduce_grid(n))
        return got, want

    got, want = run([(mid, np.inf)])
    assert got == np.inf and want == np.inf
    got, want = run([(mid, -np.inf)])
    assert got == -np.inf and want == -np.inf
    got, want = run([(0, np.inf), (n - 1, -np.inf)])
    assert math.isnan(got) and math.isnan(want)
    got, want = run([(mid, np.nan)])
    assert math.isnan(got) and math.isnan(want)
    # a masked-out nan (or inf) must not reach the sum
    got, want = run([(mid, np.nan), (1, np.inf)], masked=(mid, 1))
    assert math.isfinite(got) and _bits(got) == _bits(want)


# =============================================================================
# hash aggregation, i64 keys
# =============================================================================

TSIZES = [16, 64, 1024]
IMIN, IMAX = -2 ** 63, 2 ** 63 - 1


def _fill_grid(n):
    return max(1, min((n + 255) // 256, 2048))      # run_core


def _run_hash_i64(keys, vals, keep, tsize, f64=False, grid=None):
    """Fill + emit as run_core does (tables memset 0xFF / 0, state zeroed).
    Checks the table invariants; returns (overflow, {key: value} or None)."""
    n = len(keys)
    vt = np.float64 if f64 else I64
    d_keys = H.upload(np.array(keys, I64))
    d_vals = H.upload(np.array(vals, vt))
    d_keep = H.upload(np.array(keep, np.uint8))
    tkeys = H.alloc(tsize * 8, fill=0xFF)
    tvals = H.alloc(tsize * 8, fill=0)
    used, ovf = H.alloc(8, fill=0), H.alloc(8, fill=0)
    scnt, sval, oidx = H.alloc(8, fill=0), H.alloc(8, fill=0), H.alloc(8, fill=0)
    H.launch("tpx_hashagg_%s" % ("f64" if f64 else "i64"),
             grid or _fill_grid(n), 256,
             [d_keys, d_vals, d_keep, H.i64(n), tkeys, tvals, H.u64(tsize - 1),
              used, ovf, scnt, sval])
    tk = _i64s(tkeys)
    nused = int(H.download(used, np.uint64)[0])
    overflow = int(H.download(ovf, np.int32, 1)[0])
    filled = tk[tk != -1]
    assert nused == filled.size, "used != non-empty slots"
    assert len(set(filled.tolist())) == filled.size, "a key holds two slots"
    kept = {k for k, m in zip(keys, keep) if m}
    assert set(filled.tolist()) <= kept - {-1}
    assert int(H.download(scnt, np.uint64)[0]) == \
        sum(1 for k, m in zip(keys, keep) if m and k == -1)
    assert overflow in (0, 1)
    if overflow:
        return 1, None
    assert set(filled.tolist()) == kept - {-1}
    out = H.alloc(8 + (nused + 1) * 16 + 16)
    H.launch("tpx_hashagg_emit", min((tsize + 255) // 256, 4096), 256,
             [tkeys, tvals, H.i64(tsize), scnt, sval, out, oidx])
    nout = int(H.download(oidx, np.uint64)[0])
    assert nout == len(kept)
    rows = _i64s(out, nout * 2, offset=8).reshape(nout, 2)
    ks = rows[:, 0].tolist()
    assert len(set(ks)) == nout, "a key emitted twice"
    vs = rows[:, 1].copy().view(vt).tolist()
    return 0, dict(zip(ks, vs))


def _hash_cases(tsize):
    """[(name, keys, keep, grid or None, overflow expected)]"""
    rng = random.Random(tsize)
    mask = tsize - 1
    cases = []

    def add(name, keys, keep=None, grid=None, ovf=0):
        cases.append((name, keys, keep or [1] * len(keys), grid, ovf))

    one = M.colliding_i64_keys(mask, 3, 6)
    add("one_slot", [rng.choice(one) for _ in range(500)] + one)
    last = M.colliding_i64_keys(mask, mask, 5)
    add("wrap_to_0", [rng.choice(last) for _ in range(500)] + last)
    add("minus1_alone", [-1] * 300)
    mixed = [-1, 0, IMIN, IMAX, 1, -2, 77]
    keys = [rng.choice(mixed) for _ in range(3000)] + mixed
    add("special_mixed", keys, [rng.randint(0, 3) > 0 for _ in keys[:-7]] +
        [1] * 7)
    add("zero_only", [0] * 257)
    add("all_masked", [rng.randint(-5, 5) for _ in range(1000)], [0] * 1000)
    add("stride_tail", [rng.randint(0, tsize // 4) for _ in range(1000)],
        grid=2)
    add("one_key_100000", [424242] * 100000)
    add("half_full", [rng.randint(IMIN, IMAX) for _ in range(tsize // 2)] * 3)
    add("more_than_slots", list(range(100, 100 + tsize + 8)) * 2 + [-1], ovf=1)
    return cases


@pytest.mark.parametrize("tsize", TSIZES)
def test_hashagg_i64_keys(tsize):
    rng = random.Random(99 + tsize)
    for name, keys, keep, grid, want_ovf in _hash_cases(tsize):
        n = len(keys)
        # i64 values, sums exact mod 2^64 (the large ones wrap)
        vals = [rng.choice((rng.randint(-1000, 1000), rng.randint(2 ** 61, 2 ** 62)))
                for _ in range(n)]
        ovf, got = _run_hash_i64(keys, vals, keep, tsize, grid=grid)
        assert ovf == want_ovf, name
        if not ovf:
            want = {k: e[1] for k, e in
                    M.group_sum(keys, vals, keep, wrap=True).items()}
            assert got == want, name
        # f64 values: integer-valued, |sum| < 2^53 -> any atomic order is exact
        fvals = [float(rng.randint(-2 ** 20, 2 ** 20)) for _ in range(n)]
        ovf, got = _run_hash_i64(keys, fvals, keep, tsize, f64=True, grid=grid)
        assert ovf == want_ovf, name
        if not ovf:
            want = {k: e[1] for k, e in M.group_sum(keys, fvals, keep).items()}
            assert {k: _bits(v) for k, v in got.items()} == \
                {k: _bits(v) for k, v in want.items()}, name


def test_hashagg_wraps_past_the_last_slot():
    """Keys that all hash to the last slot fill slot tsize-1, then 0, 1, ..."""
    for tsize in TSIZES:
        last = M.colliding_i64_keys(tsize - 1, tsize - 1, 4)
        d_keys = H.upload(np.array(last, I64))
        d_vals = H.upload(np.arange(1, 5, dtype=I64))
        d_keep = H.upload(np.ones(4, np.uint8))
        tkeys, tvals = H.alloc(tsize * 8, fill=0xFF), H.alloc(tsize * 8, fill=0)
        st = [H.alloc(8, fill=0) for _ in range(4)]
        H.launch("tpx_hashagg_i64", 1, 256,
                 [d_keys, d_vals, d_keep, H.i64(4), tkeys, tvals,
                  H.u64(tsize - 1)] + st)
        tk = _i64s(tkeys)
        assert sorted(np.nonzero(tk != -1)[0].tolist()) == \
            [0, 1, 2, tsize - 1]
        tv = _i64s(tvals)
        assert {int(k): int(v) for k, v in zip(tk, tv) if k != -1} == \
            dict(zip(last, range(1, 5)))


def test_hashagg_f64_random_within_fsum_bound():
    rng = np.random.default_rng(8)
    n, tsize = 20000, 64
    keys = rng.integers(-1, 20, n).tolist()
    vals = (rng.standard_normal(n) * 1e3).tolist()
    keep = (rng.random(n) < 0.8).astype(np.uint8).tolist()
    ovf, got = _run_hash_i64(keys, vals, keep, tsize, f64=True)
    assert ovf == 0
    assert set(got) == {k for k, m in zip(keys, keep) if m}
    for k, v in got.items():
        sel = [1 if (kk == k and m) else 0 for kk, m in zip(keys, keep)]
        ref, bound = M.fsum_bound(vals, sel)
        assert abs(v - ref) <= bound, (k, v, ref, bound)


# =============================================================================
# hash aggregation, string keys
# =============================================================================

def _run_hash_str(strings, row_keys, vals, keep, tsize, f64=False, copies=3,
                  seed=False):
    """strings: the distinct keys; row_keys[i] indexes into it. Every string is
    stored `copies` times in the key buffer and rows point at any of them.

    seed=True first launches the fill kernel over one row per distinct string
    (value 0), so no two threads race to claim a slot for the same string and
    the table is deterministic: exactly one slot per string. The second launch
    then only probes, over colliding slots and by content.
    Returns (overflow, used, merged {bytes: value} or None)."""
    rng = random.Random(len(row_keys) * 31 + tsize)
    pool = bytearray(b"\xEE" * 8)            # no key lives at offset 0
    where = []
    for _ in range(copies):
        for s in strings:
            where.append(len(pool))
            pool += s + b"\xEE"
    d_pool = H.upload(bytes(pool))
    vt = np.float64 if f64 else I64
    tkeys = H.alloc(tsize * 8, fill=0)
    tlens = H.alloc(tsize * 4, fill=0)
    tvals = H.alloc(tsize * 8, fill=0)
    used, ovf, oidx = (H.alloc(8, fill=0) for _ in range(3))

    def fill(rkeys, rvals, rkeep):
        n = len(rkeys)
        offs = [where[rng.randrange(copies) * len(strings) + k] for k in rkeys]
        d_kptr = H.upload(np.array([d_pool.ptr + o for o in offs], np.uint64))
        d_klen = H.upload(np.array([len(strings[k]) for k in rkeys], np.int32))
        d_vals = H.upload(np.array(rvals, vt))
        d_keep = H.upload(np.array(rkeep, np.uint8))
        H.launch("tpx_hashagg_str_%s" % ("f64" if f64 else "i64"),
                 _fill_grid(n), 256,
                 [d_kptr, d_klen, d_vals, d_keep, H.i64(n), tkeys, tlens,
                  tvals, H.u64(tsize - 1), used, ovf])

    if seed:
        ns = len(strings)
        fill(list(range(ns)), [0] * ns, [1] * ns)
    fill(row_keys, vals, keep)
    nused = int(H.download(used, np.uint64)[0])
    overflow = int(H.download(ovf, np.int32, 1)[0])
    tk = H.download(tkeys, np.uint64)
    tl = H.download(tlens, np.int32)
    assert nused == int((tk != 0).sum()), "used != claimed slots"
    assert ((tk != 0) == (tl != 0)).all(), "a claimed slot without a length"
    assert overflow in (0, 1)
    if overflow:
        return 1, nused, None
    out3 = H.alloc((nused + 1) * 24 + 16)
    H.launch("tpx_hashagg_str_emit", min((tsize + 255) // 256, 4096), 256,
             [tkeys, tlens, tvals, H.i64(tsize), out3, oidx])
    nout = int(H.download(oidx, np.uint64)[0])
    assert nout == nused
    tri = _i64s(out3, nout * 3).reshape(nout, 3)
    merged = {}
    for p, ln, vb in tri.tolist():
        o = p - d_pool.ptr
        assert 8 <= o and o + ln <= len(pool)
        key = bytes(pool[o:o + ln])
        v = np.array([vb], I64).view(vt)[0].item()
        merged[key] = merged.get(key, 0) + v     # the engine's host merge
    if not f64:
        merged = {k: M.s64(v) for k, v in merged.items()}
    return 0, nused, merged


def _hash_str_regrowing(strings, row_keys, vals, keep, tsize, f64):
    """One launch per table, as run_core: rows of one string race for its
    slot, the losers may claim further slots, and a small table can fill up
    with such duplicates and report overflow. The host then regrows (x8, at
    most three times), which this follows."""
    for attempt in range(4):
        ovf, used, got = _run_hash_str(strings, row_keys, vals, keep, tsize,
                                       f64=f64)
        if not ovf and used * 2 <= tsize:
            return got
        tsize *= 8
    raise AssertionError("still overflowing at %d slots" % (tsize // 8))


def _str_cases(tsize):
    long_a = b"L" * 299
    sets = {
        "lengths": [b"", b"a", b"abcdefg", b"abcdefgh", b"abcdefghi",
                    bytes(range(1, 256)) + b"x" * 45],
        "last_byte": [b"abcdefgX", b"abcdefgY", b"abcdefgZ", long_a + b"1",
                      long_a + b"2", b"q1", b"q2"],
        "prefixes": [b"", b"a", b"ab", b"abc", b"abcd", b"abcdefgh",
                     b"abcdefghi", long_a, long_a + b"L"],
        "collide": M.colliding_str_keys(tsize - 1, tsize - 1, 5) +
        M.colliding_str_keys(tsize - 1, 7, 4, prefix=b"z"),
    }
    assert len(sets["lengths"][-1]) == 300
    return sets


@pytest.mark.parametrize("tsize", TSIZES)
def test_hashagg_str_keys(tsize):
    rng = random.Random(5 + tsize)
    for name, strings in _str_cases(tsize).items():
        assert len(set(strings)) == len(strings) <= tsize
        ns, n = len(strings), 4000
        row_keys = [rng.randrange(ns) for _ in range(n)]
        keep = [rng.randint(0, 4) > 0 for _ in range(n)]
        skeys = [strings[k] for k in row_keys]
        ivals = [rng.choice((rng.randint(-1000, 1000),
                             rng.randint(2 ** 61, 2 ** 62))) for _ in range(n)]
        fvals = [float(rng.randint(-2 ** 20, 2 ** 20)) for _ in range(n)]
        for f64, vals in ((False, ivals), (True, fvals)):
            want = {k: e[1] for k, e in
                    M.group_sum(skeys, vals, keep, wrap=not f64).items()}
            # as the product launches it (racing claims, host regrow)
            got = _hash_str_regrowing(strings, row_keys, vals, keep, tsize,
                                      f64)
            assert _same_map(got, want, f64), name
            # seeded: one slot per string at exactly this table size
            ovf, used, got = _run_hash_str(strings, row_keys, vals, keep,
                                           tsize, f64=f64, seed=True)
            assert (ovf, used) == (0, ns), name
            want_seeded = {s: 0 for s in strings}
            want_seeded.update(want)
            assert _same_map(got, want_seeded, f64), name


def _same_map(got, want, f64):
    if not f64:
        return got == want
    return {k: _bits(v) for k, v in got.items()} == \
        {k: _bits(v) for k, v in want.items()}


@pytest.mark.parametrize("tsize", TSIZES)
def test_hashagg_str_overflow_and_masked(tsize):
    strings = [b"key%d" % i for i in range(tsize + 8)]
    row_keys = list(range(len(strings))) * 2
    n = len(row_keys)
    ovf, used, _ = _run_hash_str(strings, row_keys, [1] * n, [1] * n, tsize,
                                 copies=2)
    assert (ovf, used) == (1, tsize)      # more distinct keys than slots
    ovf, used, got = _run_hash_str(strings, row_keys, [1] * n, [0] * n, tsize,
                                   copies=2)
    assert (ovf, used, got) == (0, 0, {})

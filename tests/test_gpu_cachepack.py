"""Kernel-level test of the cache() pack (csrc/tpx_cache.hip.h):
tpx_cache_pack_fixed and tpx_cache_gather_str, driven in the executor's order
by tests/hipkern_cache.py, against the sequential model of
tests/cache_models.py — byte for byte, into poisoned outputs with a canary zone
behind every buffer.

Row counts sit on the wave (64) and TPX_SCAN_BLOCK (2048) edges; the columns
are a bool, an Option-i64, a str and an Option-str column together; string
lengths cycle through 0, 1, 7, 8, 9, 63, 64, 65 with one 700-byte cell per 257
rows; sources lie at every alignment 0..7, scattered over two buffers; null
rows carry garbage in their value, pointer and length slots. Slots are built
and uploaded once per row count and shared by the keep patterns."""
import numpy as np
import pytest

from tests import cache_models as CM

pytestmark = pytest.mark.gpu

KINDS = [("bool", False), ("i64", True), ("str", False), ("str", True)]
LENS = [0, 1, 7, 8, 9, 63, 64, 65]
COUNTS = [1, 63, 64, 65, 2047, 2048, 2049]
PATTERNS = ["all", "none", "alternating", "first", "last", "one_per_batch"]

_shared = {}


def _rows(n):
    rows = []
    for i in range(n):
        ln = 700 if i % 257 == 8 else LENS[(i + i // 8) % 8]
        s = bytes(33 + (i * 5 + j * 3) % 94 for j in range(ln)).decode()
        rows.append((i % 3 != 0,
                     None if i % 5 == 2 else (i - 1000) * 0x10000000001,
                     s,
                     None if i % 4 == 1 else s[::-1]))
    return rows


def _setup(n):
    """(device slots, model columns, model memory) for n rows; built once."""
    if n not in _shared:
        from tests import hipkern, hipkern_cache
        rows = _rows(n)
        _c0, regs0 = CM.slots_from_rows(rows, KINDS, base_addrs=(0x1000, 0x2000))
        srcs = [hipkern.upload(regs0[0][1]), hipkern.upload(regs0[1][1])]
        assert srcs[0].ptr % 8 == 0 and srcs[1].ptr % 8 == 0
        cols, regs = CM.slots_from_rows(rows, KINDS,
                                        base_addrs=(srcs[0].ptr, srcs[1].ptr))
        assert [r[1] for r in regs] == [r[1] for r in regs0]
        aligns = {a % 8 for c in cols if c.kind == "str"
                  for a, z in zip(c.slot0, c.slot2 or [0] * n) if not z}
        assert n < 64 or aligns == set(range(8))
        _shared[n] = (hipkern_cache.DeviceCols(cols), cols, CM.Memory(regs),
                      srcs)
    return _shared[n][:3]


def _keep(n, pattern):
    k = np.zeros(n, dtype=np.uint8)
    if pattern == "all":
        k[:] = 1
    elif pattern == "alternating":
        k[1::2] = 1
        k[0] = n == 1
    elif pattern == "first":
        k[0] = 1
    elif pattern == "last":
        k[n - 1] = 1
    elif pattern == "one_per_batch":
        for b in range(0, n, 64):
            k[min(b + (b // 64 * 7) % 64, n - 1)] = 1
    return k


def _compare(got, want):
    gk, gp = got
    wk, wp = want
    assert gk == wk
    for k, (g, w) in enumerate(zip(gp, wp)):
        assert sorted(g) == sorted(w), k
        for key in w:
            assert g[key] == w[key], "column %d %s differs" % (k, key)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", COUNTS)
def test_pack_matches_model(n, pattern):
    from tests import hipkern_cache
    dcols, cols, mem = _setup(n)
    keep = _keep(n, pattern)
    want = CM.pack(keep.tolist(), 5000, cols, mem)
    _compare(hipkern_cache.pack(dcols, keep, 5000), want)


def test_all_dropped_is_an_empty_partition():
    """m = 0: offsets [0], nothing else written anywhere (every output is
    zero bytes long with its canary right behind it)."""
    from tests import hipkern_cache
    dcols, cols, mem = _setup(2049)
    keys, packed = hipkern_cache.pack(dcols, np.zeros(2049, np.uint8), 7)
    assert keys == []
    assert packed[2] == {"offsets": [0], "data": b""}
    assert packed[3] == {"offsets": [0], "data": b"", "mask": b""}
    assert packed[0] == {"values": b""}
    assert packed[1] == {"values": b"", "mask": b""}


@pytest.mark.parametrize("pattern", ["all", "alternating"])
def test_grid_stride_with_a_single_block(pattern):
    """One block per launch: threads and waves loop over many rows/batches."""
    from tests import hipkern_cache
    dcols, cols, mem = _setup(2049)
    keep = _keep(2049, pattern)
    want = CM.pack(keep.tolist(), 0, cols, mem)
    _compare(hipkern_cache.pack(dcols, keep, 0, one_block=True), want)

"""Kernel-level differential tests of the fused pair scan of tpx_rt.hip.h
(tpx_pair_scan_block / tpx_pair_scan_sums / tpx_pair_scan_add), launched
directly (tests/hipkern.py) exactly as run_core (csrc/tpx_abi.cpp) composes
them, against kern_models.exscan_array on each array separately.

sums and offs are allocated at exactly nblocks pairs, so the canary zone
behind each shows a write past the last pair; both are poisoned first, so a
pair left unwritten shows too.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import hipkern as H
from tests import kern_models as M

pytestmark = pytest.mark.gpu

I64 = np.int64
POISON = H.POISON_I64
SCAN_BLOCK = 2048
PAIR_KERNELS = ["tpx_pair_scan_block", "tpx_pair_scan_sums",
                "tpx_pair_scan_add"]

# 2048*256+1 is the first size with more than 256 block sums (second tile of
# tpx_pair_scan_sums, carry from the first); 2048*513+7 needs three tiles
SIZES = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4096,
         2048 * 256 - 1, 2048 * 256, 2048 * 256 + 1, 2048 * 513 + 7]
NMAX = max(SIZES)
A_KINDS = ["zeros", "ones", "mask01", "fanout5"]
B_KINDS = ["r300", "near2p31"]


def _kernels():
    """Add the pair-scan kernels to the harness's table of function handles,
    resolved from the module it has already loaded."""
    fns = H._module()
    hip = H._libs()[0]
    mod = H._module_cache[0]
    for name in PAIR_KERNELS:
        if name not in fns:
            f = ctypes.c_void_p()
            H._check(hip.hipModuleGetFunction(ctypes.byref(f), mod,
                                              name.encode()),
                     "hipModuleGetFunction(%s)" % name)
            fns[name] = f


@functools.lru_cache(maxsize=None)
def _input(kind):
    """(values, model exclusive scan) at the largest size; a smaller n uses
    the prefix, whose exclusive scan is the prefix of this one."""
    rng = np.random.default_rng(11 + len(kind))
    if kind == "zeros":
        v = np.zeros(NMAX, I64)
    elif kind == "ones":
        v = np.ones(NMAX, I64)
    elif kind == "mask01":
        v = (rng.random(NMAX) < 0.5).astype(I64)
    elif kind == "fanout5":           # join fan-out counts
        v = rng.integers(0, 6, NMAX, dtype=I64)
    elif kind == "r300":              # row sizes
        v = rng.integers(0, 301, NMAX, dtype=I64)
    else:   # totals pass 2^32 after two items: shows a 32-bit truncation
        v = rng.integers(2 ** 31 - 300, 2 ** 31 + 300, NMAX, dtype=I64)
    out, _ = M.exscan_array(v)
    return v, out


def _i64s(buf, count=None, offset=0):
    return H.download(buf, I64, count, offset)


def _pair_scan(d_a, d_b, d_ao, d_bo, n):
    """The three launches as run_core composes them -> (sums, offs, slot)."""
    _kernels()
    nblocks = (n + SCAN_BLOCK - 1) // SCAN_BLOCK
    sums = H.alloc(nblocks * 16)
    offs = H.alloc(nblocks * 16)
    slot = H.alloc(16)
    H.launch("tpx_pair_scan_block", nblocks, 256,
             [d_a, d_b, d_ao, d_bo, sums, H.i64(n)])
    H.launch("tpx_pair_scan_sums", 1, 256, [sums, H.i64(nblocks), offs, slot])
    if nblocks > 1:
        H.launch("tpx_pair_scan_add", nblocks, 256,
                 [d_ao, d_bo, offs, H.i64(n)])
    return sums, offs, slot


def _block_totals(v, n):
    nblocks = (n + SCAN_BLOCK - 1) // SCAN_BLOCK
    pad = np.zeros(nblocks * SCAN_BLOCK, I64)
    pad[:n] = v[:n]
    return pad.reshape(nblocks, SCAN_BLOCK).sum(axis=1, dtype=I64)


def _check_case(akind, bkind, n):
    a, a_model = _input(akind)
    b, b_model = _input(bkind)
    extra = 64                       # out[n..] must keep its poison
    d_a, d_b = H.upload(a[:n]), H.upload(b[:n])
    d_ao, d_bo = H.alloc((n + extra) * 8), H.alloc((n + extra) * 8)
    sums, offs, slot = _pair_scan(d_a, d_b, d_ao, d_bo, n)
    for got, model in ((_i64s(d_ao), a_model), (_i64s(d_bo), b_model)):
        assert np.array_equal(got[:n], model[:n]), \
            np.nonzero(got[:n] != model[:n])[0][:8]
        assert (got[n:] == POISON).all()
    total_a = M.s64(int(a_model[n - 1]) + int(a[n - 1]))
    total_b = M.s64(int(b_model[n - 1]) + int(b[n - 1]))
    assert _i64s(slot).tolist() == [total_a, total_b]
    # every one of the nblocks pairs written, with the block totals and their
    # exclusive scans (no sum here comes near 2^63, so numpy's sums are exact)
    ta, tb = _block_totals(a, n), _block_totals(b, n)
    got_sums = _i64s(sums).reshape(-1, 2)
    assert np.array_equal(got_sums[:, 0], ta)
    assert np.array_equal(got_sums[:, 1], tb)
    got_offs = _i64s(offs).reshape(-1, 2)
    assert np.array_equal(got_offs[:, 0], np.cumsum(ta) - ta)
    assert np.array_equal(got_offs[:, 1], np.cumsum(tb) - tb)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("akind", A_KINDS)
def test_pair_scan(akind, n):
    _check_case(akind, "r300", n)


@pytest.mark.parametrize("n", SIZES)
def test_pair_scan_totals_past_32_bits(n):
    _check_case("fanout5", "near2p31", n)


def test_pair_scan_sums_empty():
    """No blocks at all: nothing but the two zero totals is written."""
    _kernels()
    sums, offs, slot = H.alloc(0), H.alloc(0), H.alloc(16)
    H.launch("tpx_pair_scan_sums", 1, 256, [sums, H.i64(0), offs, slot])
    assert _i64s(slot).tolist() == [0, 0]

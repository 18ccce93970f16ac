"""Direct launches of the cache() pack kernels of csrc/tpx_cache.hip.h, on top
of tests/hipkern.py: the module hipkern compiled (the runtime header, which
ends with the pack kernels) is asked for the two extra functions, and
hipkern.launch then runs them like any other fixed kernel — synchronise, raise
on a HIP error, check the canary behind every buffer.

pack() drives the kernels in the executor's order (pack_table in
csrc/tpx_abi.cpp): tpx_cache_pack_fixed, one exclusive scan of the kept
lengths per string column over m+1 entries, tpx_cache_gather_str.
"""
import ctypes

import numpy as np

from tests import hipkern

KERNELS = ["tpx_cache_pack_fixed", "tpx_cache_gather_str"]
SCAN_BLOCK = 2048  # TPX_SCAN_BLOCK
KIND = {"i64": 0, "f64": 0, "bool": 1}  # TPX_CP_VAL8 / TPX_CP_BOOL
CP_MASK, CP_LEN = 2, 3


def _ensure():
    fns = hipkern._module()
    if KERNELS[0] not in fns:
        hip = hipkern._libs()[0]
        mod = hipkern._module_cache[0]
        for name in KERNELS:
            f = ctypes.c_void_p()
            hipkern._check(hip.hipModuleGetFunction(ctypes.byref(f), mod,
                                                    name.encode()),
                           "hipModuleGetFunction(%s)" % name)
            fns[name] = f
    return fns


def exscan(buf_in, count):
    """Exclusive scan of `count` int64 of buf_in, as dev_scan does it."""
    out = hipkern.alloc(count * 8)
    nblocks = (count + SCAN_BLOCK - 1) // SCAN_BLOCK
    sums = hipkern.alloc(nblocks * 8)
    hipkern.launch("tpx_scan_block", nblocks, 256,
                   [buf_in, out, sums, hipkern.i64(count)])
    if nblocks > 1:
        assert nblocks <= SCAN_BLOCK
        sums_scan = hipkern.alloc(nblocks * 8)
        spare = hipkern.alloc(8)
        hipkern.launch("tpx_scan_block", 1, 256,
                       [sums, sums_scan, spare, hipkern.i64(nblocks)])
        hipkern.launch("tpx_scan_add", nblocks, 256,
                       [out, sums_scan, hipkern.i64(count)])
    return out


class DeviceCols:
    """Sparse slots of cache_models.Col columns, uploaded once."""

    def __init__(self, cols):
        self.cols = cols
        self.slots = []
        for c in cols:
            s0 = hipkern.upload(np.array(c.slot0, dtype=np.uint64))
            s1 = hipkern.upload(np.array(c.slot1, dtype=np.int32)) \
                if c.slot1 is not None else None
            s2 = hipkern.upload(np.array(c.slot2, dtype=np.uint8)) \
                if c.slot2 is not None else None
            self.slots.append((s0, s1, s2))


def pack(dcols, keep, row0, one_block=False):
    """Run the pack on the device; returns (rowkeys, packed) shaped like
    cache_models.pack. one_block: a single block per launch, so every thread
    and wave walks its grid-stride loop many times."""
    _ensure()
    n = len(keep)
    keep = np.asarray(keep, dtype=np.uint8)
    m = int(keep.sum())
    rank = np.concatenate(([0], np.cumsum(keep, dtype=np.int64)[:-1])) \
        .astype(np.int64)
    d_keep, d_rank = hipkern.upload(keep), hipkern.upload(rank)
    outs, descs, klens = [], [], []
    for c, (s0, s1, s2) in zip(dcols.cols, dcols.slots):
        o = {}
        if c.kind == "str":
            kl = hipkern.alloc((m + 1) * 8, fill=0)
            klens.append(kl)
            descs.append((s1.ptr, kl.ptr, s2.ptr if s2 else 0, CP_LEN))
        else:
            o["values"] = hipkern.alloc(m * (1 if c.kind == "bool" else 8))
            descs.append((s0.ptr, o["values"].ptr, 0, KIND[c.kind]))
            klens.append(None)
        if c.opt:
            o["mask"] = hipkern.alloc(m)
            descs.append((s2.ptr, o["mask"].ptr, 0, CP_MASK))
        outs.append(o)
    d_desc = hipkern.upload(np.array(descs, dtype=np.uint64).reshape(-1))
    d_rowkey = hipkern.alloc(m * 8)
    grid = 1 if one_block else max(1, min((n + 255) // 256, 4096))
    bufs = [b for o in outs for b in o.values()] + \
        [k for k in klens if k is not None]
    hipkern.launch("tpx_cache_pack_fixed", grid, 256,
                   [d_keep, d_rank, hipkern.i64(n), hipkern.i64(row0), d_desc,
                    hipkern.i32(len(descs)), d_rowkey])
    for b in bufs:
        b.check_canary()
    nb = (n + 63) // 64
    for c, (s0, s1, s2), o, kl in zip(dcols.cols, dcols.slots, outs, klens):
        if c.kind != "str":
            continue
        o["offsets"] = exscan(kl, m + 1)
        total = int(hipkern.download(o["offsets"], np.int64)[m])
        o["data"] = hipkern.alloc(total)
        grid = 1 if one_block else max(1, min((nb + 3) // 4, 8192))
        hipkern.launch("tpx_cache_gather_str", grid, 256,
                       [d_keep, d_rank, hipkern.i64(n), s0, s1,
                        s2 if s2 else hipkern.u64(0), o["offsets"], o["data"]])
    packed = []
    for c, o in zip(dcols.cols, outs):
        d = {}
        for key, buf in o.items():
            raw = hipkern.download(buf)
            d[key] = raw.view(np.int64).tolist() if key == "offsets" \
                else raw.tobytes()
            buf.check_canary()
        packed.append(d)
    rowkeys = hipkern.download(d_rowkey, np.int64).tolist()
    return rowkeys, packed

"""Plain sequential reference of the cache() pack (csrc/tpx_cache.hip.h,
pack_table in csrc/tpx_abi.cpp): one row after another, byte loops and python
lists, nothing cooperative. Shared by the CPU pin (test_cache_models_cpu.py)
and the kernel-level GPU test (test_gpu_cachepack.py).

A stage leaves, per output column, three sparse slots indexed by INPUT row:
slot 0 an 8-byte value (i64, f64 bits, bool as 0/1) or a string pointer,
slot 1 a 4-byte string length, slot 2 a 1-byte null flag. The pack keeps the
rows with keep[i] != 0, in order, and lays them out as the columnar source
reads them.
"""
import struct


class Col:
    """Sparse slots of one output column. kind: 'i64' | 'f64' | 'bool' |
    'str'. slot0: ints (values as unsigned 64-bit patterns / addresses);
    slot1: ints or None; slot2: 0/1 flags or None (non-optional)."""

    def __init__(self, kind, opt, slot0, slot1=None, slot2=None):
        self.kind, self.opt = kind, opt
        self.slot0, self.slot1, self.slot2 = slot0, slot1, slot2


class Memory:
    """Byte-addressable view of a few (base address, bytes) regions."""

    def __init__(self, regions):
        self.regions = list(regions)

    def byte(self, addr):
        for base, data in self.regions:
            if base <= addr < base + len(data):
                return data[addr - base]
        raise IndexError("read of unmapped address %#x" % addr)


def pack(keep, row0, cols, mem):
    """-> (rowkeys, packed): rowkeys = [row0 + i for kept i]; packed[k] is a
    dict per column: 'values' (bytes: 8 per row, bool 1 per row) or
    'offsets' (list of m+1 ints) + 'data' (bytes), and 'mask' (bytes) for an
    optional column."""
    n = len(keep)
    rowkeys = []
    packed = []
    for c in cols:
        d = {}
        if c.kind == "str":
            d["offsets"] = [0]
            d["data"] = bytearray()
        else:
            d["values"] = bytearray()
        if c.opt:
            d["mask"] = bytearray()
        packed.append(d)
    for i in range(n):
        if not keep[i]:
            continue
        rowkeys.append(row0 + i)
        for c, d in zip(cols, packed):
            null = bool(c.opt and c.slot2[i])
            if c.opt:
                d["mask"].append(1 if null else 0)
            if c.kind == "str":
                ln = 0 if (null or c.slot1[i] < 0) else c.slot1[i]
                for b in range(ln):          # the byte loop
                    d["data"].append(mem.byte(c.slot0[i] + b))
                d["offsets"].append(d["offsets"][-1] + ln)
            elif c.kind == "bool":
                d["values"].append(1 if c.slot0[i] != 0 else 0)
            else:
                d["values"] += struct.pack("<Q", c.slot0[i] & (2 ** 64 - 1))
    for d in packed:
        for key in ("values", "data", "mask"):
            if key in d:
                d[key] = bytes(d[key])
    return rowkeys, packed


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def i64_bits(x):
    return x & (2 ** 64 - 1)


def slots_from_rows(rows, kinds, base_addrs=(0x10000, 0x900000), seed=1):
    """Sparse slots for python `rows` (tuples; None = null) of columns
    `kinds` = [(kind, opt)], the way a stage would leave them: string bytes
    scattered over two source regions at every alignment 0..7, garbage in the
    value / length slots of null rows. -> (cols, regions)."""
    import random
    rng = random.Random(seed)
    regions = [bytearray(), bytearray()]
    cols = []
    for k, (kind, opt) in enumerate(kinds):
        s0, s1, s2 = [], [], []
        for r, row in enumerate(rows):
            v = row[k]
            null = v is None
            s2.append(1 if null else 0)
            if kind == "str":
                if null:
                    s0.append(rng.getrandbits(40))   # never dereferenced
                    s1.append(rng.choice([0, 5, 1 << 20]))
                    continue
                raw = v.encode("utf-8")
                which = (r + k) & 1
                reg = regions[which]
                want = (r * 3 + k) & 7               # alignment of the source
                while (base_addrs[which] + len(reg)) & 7 != want:
                    reg.append(0x2A)                  # filler between cells
                s0.append(base_addrs[which] + len(reg))
                reg += raw
                s1.append(len(raw))
            elif null:
                s0.append(rng.getrandbits(64))
            elif kind == "f64":
                s0.append(f64_bits(v))
            elif kind == "bool":
                s0.append(1 if v else 0)
            else:
                s0.append(i64_bits(v))
        cols.append(Col(kind, opt, s0, s1 if kind == "str" else None,
                        s2 if opt else None))
    return cols, [(base_addrs[0], bytes(regions[0])),
                  (base_addrs[1], bytes(regions[1]))]

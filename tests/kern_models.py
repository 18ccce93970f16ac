"""Plain sequential references for the fixed kernels of tpx_rt.hip.h, and the
inputs the kernel tests share with the CPU tests that pin these models
(tests/test_kern_models_cpu.py).

Nothing here is cooperative: byte loops, Python ints, dicts, math.fsum.
"""
import itertools
import math
import random

import numpy as np

CHUNK = 4096
M64 = (1 << 64) - 1


def s64(v):
    """Wrap a Python int to a signed 64-bit value."""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


# ---- row boundaries -----------------------------------------------------------

def row_ends(data, quotes_on=1):
    """Cumulative end offsets of the complete rows of `data`: one per newline
    outside quotes (every newline when quotes_on is 0)."""
    ends = []
    inside = False
    for i, b in enumerate(data):
        if quotes_on and b == 0x22:
            inside = not inside
        elif b == 0x0A and not inside:
            ends.append(i + 1)
    return ends


def chunk_stats(data, quotes_on=1):
    """Per 4 KB chunk: (quotes, newlines after an even number of the chunk's
    own quotes, newlines after an odd number of them)."""
    q, c0, c1 = [], [], []
    for a in range(0, len(data), CHUNK):
        nq = e = o = 0
        for b in data[a:a + CHUNK]:
            if quotes_on and b == 0x22:
                nq += 1
            elif b == 0x0A:
                if nq % 2:
                    o += 1
                else:
                    e += 1
        q.append(nq)
        c0.append(e)
        c1.append(o)
    return q, c0, c1


def rows_per_chunk(data, quotes_on=1):
    """How many complete rows end inside each 4 KB chunk."""
    rc = [0] * ((len(data) + CHUNK - 1) // CHUNK)
    for e in row_ends(data, quotes_on):
        rc[(e - 1) // CHUNK] += 1
    return rc


# ---- scan / reduce ------------------------------------------------------------

def exscan(vals):
    """Exclusive prefix sums mod 2^64 -> (list of signed i64, total)."""
    inc = list(itertools.accumulate(int(v) for v in vals))
    out = [0] + [s64(v) for v in inc[:-1]]
    return out[:len(inc)], (s64(inc[-1]) if inc else 0)


def exscan_array(vals):
    """exscan() for long inputs: (np.int64 array, total), same arithmetic."""
    n = len(vals)
    inc = np.fromiter((v & M64 for v in itertools.accumulate(vals.tolist())),
                      dtype=np.uint64, count=n).view(np.int64)
    out = np.zeros(n, dtype=np.int64)
    out[1:] = inc[:-1]
    return out, (int(inc[-1]) if n else 0)


def sum_i64(vals, keep):
    return s64(sum(int(v) for v, k in zip(vals, keep) if k))


def reduce_grid(n):
    """The product's grid for the reduce kernels (run_core)."""
    return min((n + 2047) // 2048, 1024)


def reduce_f64_order(vals, keep, nblocks, threads=256):
    """The evaluation order the header documents for the f64 reduce:
    per-thread partials over i = tid, tid+stride, ... in index order, a halving
    tree over the `threads` partials of each block (slot t += slot t+o for
    o = threads/2 .. 1), then one sequential pass over the block results.
    A masked-out item adds nothing; partials start at +0.0, so adding +0.0 in
    its place gives the same bits."""
    vals = np.asarray(vals, dtype=np.float64)
    keep = np.asarray(keep).astype(bool)
    stride = nblocks * threads
    rounds = (len(vals) + stride - 1) // stride
    padded = np.zeros(rounds * stride, dtype=np.float64)
    padded[:len(vals)] = np.where(keep, vals, 0.0)
    acc = np.zeros(stride, dtype=np.float64)
    with np.errstate(all="ignore"):
        for r in range(rounds):
            acc = acc + padded[r * stride:(r + 1) * stride]
        sh = acc.reshape(nblocks, threads).copy()
        o = threads // 2
        while o:
            sh[:, :o] = sh[:, :o] + sh[:, o:2 * o]
            o //= 2
        total = 0.0
        for p in sh[:, 0].tolist():
            total += p
    return total


def fsum_bound(vals, keep):
    """(math.fsum of the kept items, (m-1) * 2^-53 * sum|x|): any summation
    order of m finite doubles lies within that bound of the exact sum
    (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, to first
    order; inputs hold no subnormals, so no underflow term)."""
    kept = [float(v) for v, k in zip(vals, keep) if k]
    ref = math.fsum(kept)
    bound = max(len(kept) - 1, 0) * 2.0 ** -53 * math.fsum(abs(v) for v in kept)
    return ref, bound


# ---- hash aggregation -----------------------------------------------------------

def hash_i64(k):
    """Replica of tpx_hash_i64 (the murmur3 64-bit finalizer)."""
    x = k & M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def jhash_bytes(b):
    """Replica of tpx_jhash_bytes (FNV-1a with the header's offset basis)."""
    h = 1469598103934665603
    for c in b:
        h = ((h ^ c) * 1099511628211) & M64
    return h


def group_sum(keys, vals, keep, wrap=False):
    """{key: [count, sum]} over the kept rows; sums of ints wrap when asked."""
    out = {}
    for k, v, m in zip(keys, vals, keep):
        if not m:
            continue
        e = out.setdefault(k, [0, 0])
        e[0] += 1
        e[1] += v
    if wrap:
        for e in out.values():
            e[1] = s64(e[1])
    return out


def colliding_i64_keys(mask, slot, count, start=1):
    """The first `count` keys >= start whose hash lands on `slot` under mask."""
    out = []
    k = start
    while len(out) < count:
        if hash_i64(k) & mask == slot:
            out.append(k)
        k += 1
    return out


def colliding_str_keys(mask, slot, count, prefix=b"k"):
    out = []
    i = 0
    while len(out) < count:
        s = prefix + str(i).encode()
        if jhash_bytes(s) & mask == slot:
            out.append(s)
        i += 1
    return out


# ---- shared CSV inputs ------------------------------------------------------------
# Every case is built from whole "int,text,int" rows so that most of them are
# valid CSV and can also go through ctx.csv(); a feature is put on a chosen
# byte by padding with plain rows in front of it.

HEADER = b"a,b,c\n"


def _plain_rows(nbytes, rng):
    """Plain rows totalling exactly nbytes (nbytes == 0 or >= 6)."""
    assert nbytes == 0 or nbytes >= 6, nbytes
    out = []
    while nbytes:
        take = nbytes if nbytes < 12 + 6 else min(nbytes - 6, rng.randint(6, 60))
        if nbytes - take < 6 and nbytes != take:
            take = nbytes
        # "d,ttt,d\n": 5 bytes of frame + text
        out.append(b"%d,%s,%d\n" % (rng.randint(0, 9), b"t" * (take - 5),
                                    rng.randint(0, 9)))
        nbytes -= take
    return b"".join(out)


def _at(rng, target, row, feat_off, before=HEADER):
    """`before` + plain rows + row, with byte feat_off of row at `target`."""
    pad = target - feat_off - len(before)
    return before + _plain_rows(pad, rng) + row


def _random_rows(nbytes, rng, crlf=False):
    """About nbytes of random rows with quoted cells, "" pairs and quoted
    newlines (valid CSV)."""
    out = [HEADER]
    size = len(HEADER)
    eol = b"\r\n" if crlf else b"\n"
    while size < nbytes:
        kind = rng.randint(0, 5)
        if kind == 0:
            cell = b'"x\ny"'
        elif kind == 1:
            cell = b'"say ""hi"""'
        elif kind == 2:
            cell = b'"q,c\n\n"'
        else:
            cell = b"w" * rng.randint(0, 40)
        row = b"%d,%s,%d" % (rng.randint(-99, 99), cell, rng.randint(0, 9)) + eol
        out.append(row)
        size += len(row)
    return b"".join(out)


def csv_cases():
    """[(name, bytes, valid_csv)] — the boundary-scan inputs."""
    rng = random.Random(20)
    tail = _plain_rows(300, rng)
    cases = []

    def add(name, data, valid=True):
        cases.append((name, bytes(data), valid))

    body = _random_rows(41000, rng)
    for size in (1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 3 * 4096 + 1):
        add("cut%d" % size, body[:size], valid=False)  # may end inside quotes
    add("random40k", body)
    add("random_exact_8192", _at(rng, 8191, b"1,z,2\n", 5, before=body[:body.index(b"\n", 6000) + 1]))
    # an opening quote on byte 63 / 64 / 4095 / 4096 (cell closes 70 B later)
    qrow = b'5,"' + b"in\nside," * 8 + b'",6\n'
    for pos in (63, 64, 4095, 4096):
        add("quote_at_%d" % pos, _at(rng, pos, qrow, 2) + tail)
    # a closing quote on the same bytes
    crow = b'5,"in\nside",6\n'
    for pos in (63, 64, 4095, 4096):
        add("close_at_%d" % pos, _at(rng, pos, crow, 10) + tail)
    # an escaped "" pair straddling a lane edge (63|64) and a chunk edge
    erow = b'7,"he said ""\n"" twice\n",8\n'
    for pos in (63, 4095):
        add("escpair_at_%d" % pos, _at(rng, pos, erow, 11) + tail)
    # a quoted newline as the last byte of a chunk, then more quoted newlines
    nrow = b'3,"ab\n\ncd\n",4\n'
    add("quoted_nl_at_4095", _at(rng, 4095, nrow, 5) + tail)
    # a row's own newline on the last byte of a lane / a chunk
    add("nl_at_63", _at(rng, 63, b"1,z,2\n", 5) + tail)
    add("nl_at_4095", _at(rng, 4095, b"1,z,2\n", 5) + tail)
    # a chunk with no newline at all: a 9000-byte row
    add("long_row", HEADER + _plain_rows(500, rng) +
        b"1," + b"L" * 9000 + b",2\n" + tail)
    add("long_quoted_row", HEADER + _plain_rows(500, rng) +
        b'1,"' + b"L\n" * 4500 + b'",2\n' + tail)
    # a chunk that is all quotes: inside a quoted cell (2048 "" pairs), and
    # raw with an odd number of quotes in front of it
    allq = b'1,"' + b'"' * (CHUNK + 2 * 64) + b'",2\n'
    add("all_quotes_chunk", _at(rng, CHUNK - 64, allq, 3) + tail)
    add("all_quotes_odd", b'"' * (2 * CHUNK + 1) + b"\nx\n\"\ny\n",
        valid=False)
    add("crlf", _random_rows(9000, rng, crlf=True))
    add("no_trailing_newline", HEADER + _plain_rows(5000, rng) + b"1,end,2")
    add("only_newlines", b"\n" * (CHUNK + 65), valid=False)
    return cases


def ranged_emit_input():
    """About 40 KB over ten or more chunks: rows of mixed length, rows longer
    than 4 KB, a row's newline on byte 4095 of a chunk, and a row's newline
    that is the last valid one of its chunk, followed by quoted newlines up to
    and across the chunk's end."""
    rng = random.Random(31)
    d = _at(rng, CHUNK - 1, b"1,z,2\n", 5)                  # '\n' on byte 4095
    d += _plain_rows(1000, rng)
    # row ends at byte 2*4096-600; the next row is quoted newlines past the edge
    d = _at(rng, 2 * CHUNK - 600, b"1,z,2\n", 5, before=d)
    d += b'4,"' + b"q\n" * 500 + b'",5\n'
    d += _plain_rows(700, rng)
    d += b"1," + b"L" * 9500 + b",2\n"                        # empty chunks
    d += _plain_rows(3000, rng)
    d += b'1,"' + b"M" * 5000 + b'\n",2\n'
    d = _at(rng, 8 * CHUNK - 1, b"1,z,2\n", 5, before=d)   # '\n' on byte 4095
    d += b'9,"' + b"\n" * 4096 + b'",9\n'                     # whole chunk quoted
    d += _random_rows(6000, rng)[len(HEADER):]
    d += b"tail,no,newline"
    return d


# ---- shared numeric inputs --------------------------------------------------------

SCAN_SIZES = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4096,
              2048 * 2048 - 1, 2048 * 2048, 2048 * 2048 + 1]
REDUCE_SIZES = [1, 255, 256, 257, 2048, 2049, 262143, 262145, 2097153]


def f64_values(kind, n, seed=0):
    """Finite doubles without subnormals."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return (rng.standard_normal(n) * 1e3).astype(np.float64)
    if kind == "cancel":   # +1e16, 1.0, -1e16, 1.0, ...
        v = np.ones(n, dtype=np.float64)
        v[0::4] = 1e16
        v[2::4] = -1e16
        return v
    raise ValueError(kind)


def keep_mask(kind, n, seed=0):
    if kind == "all0":
        return np.zeros(n, dtype=np.uint8)
    if kind == "all1":
        return np.ones(n, dtype=np.uint8)
    return (np.random.default_rng(seed + 7).random(n) < 0.6).astype(np.uint8)

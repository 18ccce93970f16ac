"""Kernel-level differential tests of tpx_csv_chunk_stats and tpx_csv_emit_rows
(tpx_rt.hip.h) at the sizes where a coalesced scan can go wrong: the edges of a
16-byte piece, of a 1 KiB trip and of a 4 KiB chunk. Launched directly
(tests/hipkern.py) and compared with the byte loops of tests/kern_models.py;
every integer must be equal.

Each input is followed by the `"\\n` slack of tests/test_gpu_kernels.py, so a
kernel that counts a byte at or after `size` fails. Output buffers are
poisoned and carry a canary zone, which launch() checks.
"""
import functools
import random

import numpy as np
import pytest

from tests import hipkern as H
from tests import kern_models as M

pytestmark = pytest.mark.gpu

I64 = np.int64
POISON = H.POISON_I64
SLACK = b'"\n' * 40

SIZES = [1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191,
         3 * 4096 + 5]
# the alphabet of tests/host_boundary_test.cpp: the two classes, bytes one
# above them ('#', 0x0B), their high-bit twins (0xA2, 0x8A) and bystanders
ALPHABET = b'\r,a#\x0b\xa2\x8a'


def _seams(n, ats):
    """A quote at each byte of `ats` with a newline on either side."""
    s = bytearray(b"a" * n)
    for at in ats:
        if 1 <= at and at + 1 < n:
            s[at - 1], s[at], s[at + 1] = 0x0A, 0x22, 0x0A
    return bytes(s)


def _mix(n, pq, pn, seed):
    rng = random.Random(seed * 1000003 + n)
    out = bytearray(n)
    for i in range(n):
        u = rng.random()
        out[i] = (0x22 if u < pq else 0x0A if u < pq + pn
                  else ALPHABET[rng.randrange(len(ALPHABET))])
    return bytes(out)


def _cycle(pat, n):
    return (pat * (n // len(pat) + 1))[:n]


CONTENTS = {
    "no_newline": lambda n: [b"a" * n],
    "all_newline": lambda n: [b"\n" * n],      # 4096 rows per chunk
    "all_quote": lambda n: [b'"' * n],
    "quote_newline": lambda n: [_cycle(b'"\n', n), _cycle(b'\n"', n)],
    "seams": lambda n: [_seams(n, (15, 1023, 4095)),
                        _seams(n, (16, 1024, 4096))],
    "plus_one": lambda n: [_cycle(b'"\n#', n), _cycle(b'\n\x0b', n),
                           _cycle(b'"\n#\n\x0b', n)],
    "random": lambda n: [_mix(n, 0.01, 0.02, 1), _mix(n, 0.3, 0.3, 2),
                         _mix(n, 0.0, 0.5, 3)],
}


def _nchunks(size):
    return (size + M.CHUNK - 1) // M.CHUNK


def _grid_w(nch):
    return min((nch + 3) // 4, 8192)     # csv_boundary_and_core


def _i64s(buf):
    return H.download(buf, I64)


@functools.lru_cache(maxsize=None)
def _model(data, quotes_on):
    """(q, c0, c1, qscan, base, nrows, [0] + row ends), computed once."""
    mq, m0, m1 = M.chunk_stats(data, quotes_on)
    ends = M.row_ends(data, quotes_on)
    qscan, _ = M.exscan(mq)
    base, nrows = M.exscan(M.rows_per_chunk(data, quotes_on))
    assert nrows == len(ends)
    return mq, m0, m1, qscan, base, nrows, np.array([0] + ends, I64)


def _edges(base, nrows):
    e = {0, nrows}
    for b in base:
        e.update((b - 1, b, b + 1))
    return sorted(x for x in e if 0 <= x <= nrows)


def _check_input(data, quotes_on):
    size, nch = len(data), _nchunks(len(data))
    mq, m0, m1, qscan, base, nrows, model = _model(data, quotes_on)
    d_data = H.upload(data + SLACK)
    d_qs = H.upload(np.array(qscan, I64))
    d_base = H.upload(np.array(base, I64))
    tag = (size, quotes_on)
    for grid in sorted({_grid_w(nch), 1, 2}):
        q, c0, c1 = H.alloc(nch * 8), H.alloc(nch * 8), H.alloc(nch * 8)
        H.launch("tpx_csv_chunk_stats", grid, 256,
                 [d_data, H.i64(size), H.i64(nch), q, c0, c1,
                  H.i32(quotes_on)])
        assert _i64s(q).tolist() == mq, ("q", grid, tag)
        assert _i64s(c0).tolist() == m0, ("c0", grid, tag)
        assert _i64s(c1).tolist() == m1, ("c1", grid, tag)
        if nrows == 0:
            continue        # the product returns an empty result before emit
        offs = H.alloc((nrows + 1) * 8)
        H.launch("tpx_csv_emit_rows", grid, 256,
                 [d_data, H.i64(size), H.i64(nch), d_qs, d_base, offs,
                  H.i32(quotes_on), H.i64(0), H.i64(nrows)])
        assert np.array_equal(_i64s(offs), model), ("row_offs", grid, tag)
    if nrows == 0:
        return
    # ranged calls: all of row_offs[lo..hi] correct, nothing else touched
    # unless with the correct value (test_csv_emit_ranged)
    offs = H.alloc((nrows + 1) * 8)
    idx = np.arange(nrows + 1)
    edges = _edges(base, nrows)
    for lo in edges:
        for hi in edges:
            if hi <= lo:
                continue
            offs.fill(H.POISON)
            H.launch("tpx_csv_emit_rows", _grid_w(nch), 256,
                     [d_data, H.i64(size), H.i64(nch), d_qs, d_base, offs,
                      H.i32(quotes_on), H.i64(lo), H.i64(hi)])
            got = _i64s(offs)
            inside = (idx >= lo) & (idx <= hi)
            wrong_in = idx[inside & (got != model)]
            wrong_out = idx[~inside & (got != model) & (got != POISON)]
            assert not wrong_in.size and not wrong_out.size, (
                "range", lo, hi, tag, wrong_in[:4].tolist(),
                wrong_out[:4].tolist())


@pytest.mark.parametrize("quotes_on", [1, 0], ids=["quotes", "text"])
@pytest.mark.parametrize("kind", list(CONTENTS))
def test_boundary_kernels_at_the_seams(kind, quotes_on):
    for n in SIZES:
        for data in CONTENTS[kind](n):
            _check_input(data, quotes_on)

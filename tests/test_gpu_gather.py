"""Kernel-level test of tpx_csv_gather (tpx_rt.hip.h), the second step of the
fused csv sink, launched directly (tests/hipkern.py) against a numpy model
kept in this file; a CPU test checks the model against plain concatenation.

The scratch holds one region per 64-row batch, each starting 8-aligned and
reserved in multiples of 8 as tpx_wave_commit_csv reserves them, here in
shuffled order with poisoned gaps between them. The output buffers are
poisoned (hipkern.alloc) and longer than what the kernel may write, so the
poison before and after the written range and the canaries behind every buffer
show a stray store.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import hipkern as H

I64 = np.int64
U64 = np.uint64
POISON = H.POISON
GATHER = "tpx_csv_gather"
SCRATCH_POISON = 0x5E

NBS = [1, 2, 63, 64, 65, 257]
KEPT_CYCLE = [0, 1, 13, 64]
# bytes per batch: 0 through 7, 8, 9 (head only, one word, word + tail) and
# sizes around the 512 bytes a wave moves per trip; 17 entries, so the cycle
# drifts against KEPT_CYCLE
BYTES_CYCLE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1500]
BIG = 9000                      # one batch above 4096
ROW0 = 7_000_000_000            # row indices past 32 bits
BYTE0 = 5_000_000_000           # byte offsets past 32 bits
ROWS_BASE = 5                   # out_offs / out_rowidx entries before ours


def _kernel():
    """Add tpx_csv_gather to the harness's table of function handles, resolved
    from the module it has already loaded."""
    fns = H._module()
    if GATHER not in fns:
        hip = H._libs()[0]
        mod = H._module_cache[0]
        f = ctypes.c_void_p()
        H._check(hip.hipModuleGetFunction(ctypes.byref(f), mod,
                                          GATHER.encode()),
                 "hipModuleGetFunction(%s)" % GATHER)
        fns[GATHER] = f


@functools.lru_cache(maxsize=None)
def make_case(nb, align):
    """Descriptors, rmeta and scratch of nb batches as tpx_wave_commit_csv
    leaves them, plus the rows themselves for the plain-Python check."""
    rng = np.random.default_rng(1000 * nb + align)
    b_rows = np.zeros(nb, I64)
    b_bytes = np.zeros(nb, I64)
    rmeta = np.full(nb * 64, 0xDEADBEEFDEADBEEF, U64)
    rows = []                                  # per batch: [(lane, bytes)]
    for wb in range(nb):
        kept = KEPT_CYCLE[(wb + align) % 4]
        nbytes = BYTES_CYCLE[(wb + 3 * align) % len(BYTES_CYCLE)]
        if wb == nb // 2:
            kept, nbytes = 13, BIG
        if kept == 0:
            nbytes = 0
        cuts = np.sort(rng.integers(0, nbytes + 1, max(kept - 1, 0)))
        edges = np.concatenate(([0], cuts, [nbytes])) if kept else np.array([0])
        lanes = np.sort(rng.choice(64, size=kept, replace=False))
        batch = []
        for j in range(kept):
            size = int(edges[j + 1] - edges[j])
            batch.append((int(lanes[j]),
                          rng.integers(32, 127, size, dtype=np.uint8).tobytes()))
            rmeta[wb * 64 + j] = (int(lanes[j]) << 32) | int(edges[j])
        rows.append(batch)
        b_rows[wb] = kept
        b_bytes[wb] = nbytes
    # regions in shuffled order, 8-aligned, with poisoned gaps of 8..32 bytes
    order = rng.permutation(nb)
    b_off = np.zeros(nb, I64)
    pos = 8 * int(rng.integers(1, 4))
    for wb in order:
        b_off[wb] = pos
        pos += (int(b_bytes[wb]) + 7) // 8 * 8 + 8 * int(rng.integers(1, 5))
    scratch = np.full(pos, SCRATCH_POISON, np.uint8)
    for wb in range(nb):
        text = b"".join(r for _l, r in rows[wb])
        scratch[b_off[wb]:b_off[wb] + len(text)] = np.frombuffer(text, np.uint8)
    rows_scan = ROWS_BASE + np.cumsum(b_rows) - b_rows
    bytes_scan = align + np.cumsum(b_bytes) - b_bytes
    return dict(nb=nb, align=align, b_off=b_off, b_rows=b_rows,
                b_bytes=b_bytes, rmeta=rmeta, scratch=scratch, rows=rows,
                rows_scan=rows_scan.astype(I64),
                bytes_scan=bytes_scan.astype(I64))


def model_gather(c, out_len, n_entries):
    """What tpx_csv_gather leaves in (out, out_offs, out_rowidx), all three
    poisoned first."""
    out = np.full(out_len, POISON, np.uint8)
    offs = np.full(n_entries, H.POISON_I64, I64)
    ridx = np.full(n_entries, H.POISON_I64, I64)
    for wb in range(c["nb"]):
        k, nbytes = int(c["b_rows"][wb]), int(c["b_bytes"][wb])
        rb, bb = int(c["rows_scan"][wb]), int(c["bytes_scan"][wb])
        src = int(c["b_off"][wb])
        out[bb:bb + nbytes] = c["scratch"][src:src + nbytes]
        for j in range(k):
            m = int(c["rmeta"][wb * 64 + j])
            offs[rb + j] = BYTE0 + bb + (m & 0xFFFFFFFF)
            ridx[rb + j] = ROW0 + wb * 64 + (m >> 32)
    return out, offs, ridx


def _sizes(c):
    total_rows = int(c["b_rows"].sum())
    total_bytes = int(c["b_bytes"].sum())
    return (c["align"] + total_bytes + 24,      # out: poison on both sides
            ROWS_BASE + total_rows + 6)


@pytest.mark.parametrize("align", range(8))
@pytest.mark.parametrize("nb", NBS)
def test_model_is_plain_concatenation(nb, align):
    c = make_case(nb, align)
    out_len, n_entries = _sizes(c)
    out, offs, ridx = model_gather(c, out_len, n_entries)
    flat = [(wb * 64 + lane, r) for wb, batch in enumerate(c["rows"])
            for lane, r in batch]
    text = b"".join(r for _i, r in flat)
    a = align
    assert out[a:a + len(text)].tobytes() == text
    assert (out[:a] == POISON).all() and (out[a + len(text):] == POISON).all()
    starts = np.cumsum([0] + [len(r) for _i, r in flat])[:-1]
    n = len(flat)
    assert offs[ROWS_BASE:ROWS_BASE + n].tolist() == \
        [BYTE0 + a + int(s) for s in starts]
    assert ridx[ROWS_BASE:ROWS_BASE + n].tolist() == \
        [ROW0 + i for i, _r in flat]
    for arr in (offs, ridx):
        assert (arr[:ROWS_BASE] == H.POISON_I64).all()
        assert (arr[ROWS_BASE + n:] == H.POISON_I64).all()
    # the shapes the issue names are all present
    if nb >= 65:
        assert set(c["b_rows"].tolist()) == {0, 1, 13, 64}
        assert set(range(10)) <= set(c["b_bytes"].tolist())
    assert BIG in c["b_bytes"].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("align", range(8))
@pytest.mark.parametrize("nb", NBS)
def test_gather(nb, align):
    _kernel()
    c = make_case(nb, align)
    out_len, n_entries = _sizes(c)
    want_out, want_offs, want_ridx = model_gather(c, out_len, n_entries)
    d_scratch = H.upload(c["scratch"])
    d_in = [H.upload(c[k]) for k in ("b_off", "b_rows", "b_bytes",
                                     "rows_scan", "bytes_scan", "rmeta")]
    d_out = H.alloc(out_len)
    d_offs = H.alloc(n_entries * 8)
    d_ridx = H.alloc(n_entries * 8)
    # nb = 257 with 3 blocks of 4 waves: every wave takes many batches
    grid = 3 if nb == 257 else (nb + 3) // 4
    H.launch(GATHER, grid, 256,
             [d_scratch] + d_in + [H.i64(nb), H.i64(ROW0), d_out, d_offs,
                                   d_ridx, H.i64(BYTE0)])
    got_out = H.download(d_out)
    bad = np.nonzero(got_out != want_out)[0]
    assert bad.size == 0, bad[:8]
    assert np.array_equal(H.download(d_offs, I64), want_offs)
    assert np.array_equal(H.download(d_ridx, I64), want_ridx)
    # the kernel only reads these
    assert np.array_equal(H.download(d_scratch), c["scratch"])

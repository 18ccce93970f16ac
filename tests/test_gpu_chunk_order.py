"""The four-chunk pipeline of run_core (csrc/tpx_abi.cpp) through the engine.

Each chunk's compaction scans are queued behind its own main kernel, the host
reads the chunk totals from a pinned slot of the chunk's own, the writes run
on a stream of their own, and the last chunk writes in place in the final
buffer. Inputs of a little over 2^20 narrow rows reach that path; the expected
output is the oracle's result on one 4096-row block, repeated (see
tests/chunk_order_pipelines.py).
"""
import functools
import os

import pytest

import tuplex_amd
from oracle import pyoracle_csv
from tests import chunk_order_pipelines as CO
from tests.pipelines import apply_ops

pytestmark = pytest.mark.gpu

# one engine call for the whole file: the default split size would cut it into
# pieces of fewer than 2^20 rows, which run as a single chunk
CONF = {"tuplex.inputSplitSize": "1GB"}


@functools.lru_cache(maxsize=None)
def _oracle(kind):
    """(collect() rows, csv header line, csv body) of one block."""
    block = CO.mixed_block() if kind == "mixed" else CO.dropped_block()
    data = CO.HEADER + block
    rows = pyoracle_csv.run_csv_pipeline(data, CO.ops())
    assert rows["exception_counts"] == {}
    text = pyoracle_csv.run_csv_pipeline(data, CO.ops(), sink="csv")["csv_text"]
    head, body = text.split(b"\n", 1)
    return rows["output"], head + b"\n", body


# arrangement -> input body from the (mixed, dropped) blocks; the quarters are
# run_core's four row ranges
ARRANGEMENTS = {
    "mixed": lambda m, d: m * CO.BLOCKS,
    "first_quarter_dropped": lambda m, d: d * CO.QUARTER + m * (3 * CO.QUARTER),
    "last_quarter_dropped": lambda m, d: m * (3 * CO.QUARTER) + d * CO.QUARTER,
}
MIXED_BLOCKS = {"mixed": CO.BLOCKS, "first_quarter_dropped": 3 * CO.QUARTER,
                "last_quarter_dropped": 3 * CO.QUARTER}


@functools.lru_cache(maxsize=None)
def _input_bytes(arrangement):
    return CO.HEADER + ARRANGEMENTS[arrangement](CO.mixed_block(),
                                                 CO.dropped_block())


def _input_file(tmp_path, arrangement):
    p = os.path.join(str(tmp_path), arrangement + ".csv")
    with open(p, "wb") as f:
        f.write(_input_bytes(arrangement))
    return p


def _tocsv(ctx, src, dst):
    ds = apply_ops(ctx.csv(src), CO.ops())
    ds.tocsv(dst)
    assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason
    assert ctx.metrics.data.get("chunks", 1) == 1      # one execute, all rows
    with open(dst, "rb") as f:
        return f.read()


def test_dropped_block_is_dropped():
    rows, _head, body = _oracle("dropped")
    assert rows == [] and body == b""
    rows, _head, body = _oracle("mixed")
    assert 0 < len(rows) < CO.BLOCK_ROWS // 2 and body.count(b"\n") == len(rows)


@pytest.mark.parametrize("arrangement", sorted(ARRANGEMENTS))
def test_csv_sink_file_to_file(tmp_path, arrangement):
    """(a) mixed keep ratio; (b) a zero-byte first chunk, and an empty last
    chunk writing in place; (c) a second execute of the same stage in the
    same process (event pool, pinned slots) gives the same bytes."""
    _rows, head, body = _oracle("mixed")
    want = head + body * MIXED_BLOCKS[arrangement]
    src = _input_file(tmp_path, arrangement)
    ctx = tuplex_amd.Context(CONF)
    got1 = _tocsv(ctx, src, os.path.join(str(tmp_path), "out1.csv"))
    got2 = _tocsv(ctx, src, os.path.join(str(tmp_path), "out2.csv"))
    assert len(got1) == len(want)
    assert got1 == want
    assert got2 == got1


@pytest.mark.parametrize("arrangement", sorted(ARRANGEMENTS))
def test_mem_sink_collect(tmp_path, arrangement):
    """(d) the mem sink through the same ordering (8-byte header bias)."""
    rows, _head, _body = _oracle("mixed")
    src = _input_file(tmp_path, arrangement)
    ctx = tuplex_amd.Context(CONF)
    ds = apply_ops(ctx.csv(src), CO.ops())
    got = ds.collect()
    assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason
    assert ctx.metrics.data.get("chunks", 1) == 1
    assert ds.exception_counts == {}
    assert len(got) == MIXED_BLOCKS[arrangement] * len(rows)
    assert got == rows * MIXED_BLOCKS[arrangement]


def test_zillow_csv_sink_with_quoting(tmp_path):
    """Zillow-shaped rows with output cells that need quoting: the 64k-row
    dirty base tiled 20x, written with tocsv."""
    from tests.zillow_data import make_zillow_csv_bytes

    zillow_ops = CO.zillow_quoting_ops

    base, _ = make_zillow_csv_bytes(64000, seed=13, dirty_frac=0.01,
                                    header=True)
    header, body = base.split(b"\n", 1)
    src = os.path.join(str(tmp_path), "big.csv")
    with open(src, "wb") as f:
        f.write(header + b"\n" + body * 20)  # 1.28M rows
    ctx = tuplex_amd.Context(CONF)
    ds = apply_ops(ctx.csv(src), zillow_ops())
    dst = os.path.join(str(tmp_path), "out.csv")
    ds.tocsv(dst)
    assert ds._last_outcome.mode == "gpu", ds._last_outcome.fallback_reason
    assert ctx.metrics.data.get("chunks", 1) == 1
    ref = pyoracle_csv.run_csv_pipeline(base, zillow_ops(), sink="csv")
    head, ref_body = ref["csv_text"].split(b"\n", 1)
    assert b'"' in ref_body
    with open(dst, "rb") as f:
        got = f.read()
    assert got == head + b"\n" + ref_body * 20
    for k, v in ref["exception_counts"].items():
        assert ds.exception_counts.get(k, 0) == v * 20, (k, v)

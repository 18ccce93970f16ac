"""Inputs and stage of tests/test_gpu_chunk_order.py.

run_core (csrc/tpx_abi.cpp) splits an execute of >= 2^20 rows into four equal
row ranges. The inputs here are whole numbers of 4096-row blocks, 272 of them
(68 per range), so each range is a run of whole blocks and the expected output
is the oracle's result on one block, repeated.

The UDFs live at module level so that their source can be captured, and
precompile() puts the stage into the kernel cache at build time.
"""
import numpy as np

BLOCK_ROWS = 4096
BLOCKS = 272                    # 1 114 112 rows: just over the 2^20 threshold
QUARTER = BLOCKS // 4
HEADER = b"a,b\n"


def co_keep(x):
    return x["a"] < 250


def co_map(x):
    return (x["a"] + x["b"], x["b"])


def ops():
    return [("filter", co_keep), ("map", co_map)]


def zq_keep(x):
    return x["bedrooms"] < 4


def zillow_quoting_ops():
    """A short Zillow chain whose output keeps two columns with commas in
    their cells ("3 bds , 2 ba , 1,500 sqft", "$1,250,000"): the csv sink has
    to quote them."""
    from tests.test_codegen_compile import extractBd
    return [
        ("withColumn", "bedrooms", extractBd),
        ("filter", zq_keep),
        ("selectColumns", ["url", "address", "facts and features", "price",
                           "bedrooms"]),
    ]


def _block(a, b):
    return b"".join(b"%d,%d\n" % (int(x), int(y)) for x, y in zip(a, b))


def mixed_block(seed=7):
    """4096 rows, about a quarter of which pass co_keep, in no regular order."""
    rng = np.random.default_rng(seed)
    return _block(rng.integers(0, 1000, BLOCK_ROWS),
                  rng.integers(0, 100000, BLOCK_ROWS))


def dropped_block(seed=8):
    """4096 rows none of which passes co_keep."""
    rng = np.random.default_rng(seed)
    return _block(rng.integers(250, 1000, BLOCK_ROWS),
                  rng.integers(0, 100000, BLOCK_ROWS))


def precompile(verbose=False):
    from tests import pipelines
    from tuplex_amd import codegen, csvio, engine, plan
    glib = engine.GpuLib.get()
    sample = HEADER + mixed_block()
    _h, names, col_types = csvio.sniff(sample, [""], 0.9, None, None, b",")
    sp = plan.build_stage(col_types, names, ops())
    assert sp.compilable, sp.why_not_compilable
    n = 0
    for sink in ("mem", "csv"):
        src, desc = codegen.generate_stage(
            sp, source="csv", sink=sink,
            csv_info={"null_values": [""], "delimiter": ","})
        pipelines._stage_compile(glib, src, desc)
        n += 1
        if verbose:
            print("precompiled chunk-order:", sink)
    from tests.zillow_data import make_zillow_csv_bytes
    zdata, _ = make_zillow_csv_bytes(2000, seed=42, dirty_frac=0.02)
    _h, names, col_types = csvio.sniff(zdata, [""], 0.9, None, None, b",")
    sp = plan.build_stage(col_types, names, zillow_quoting_ops())
    assert sp.compilable, sp.why_not_compilable
    src, desc = codegen.generate_stage(
        sp, source="csv", sink="csv",
        csv_info={"null_values": [""], "delimiter": ","})
    pipelines._stage_compile(glib, src, desc)
    return n + 1

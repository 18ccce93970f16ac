"""Stages, inputs and runner of tests/test_gpu_cellindex.py.

One csv-source stage over mixed str / i64 / f64 / Option columns with one
filter, with the csv sink (fused window: the cell index overlays the wave's
output window) and with the mem sink (no window: the index has an LDS region
of its own), each generated with the wave-cooperative cell index
(TPX_CELL_INDEX=1) and without (TPX_CELL_INDEX=0). Two more stages — one column
above the index's limit, and a '|' delimiter — must not change with the
switch. The UDFs live at module level so that their source can be captured;
precompile() puts every build into the kernel cache at build time.
"""
import ctypes
import os
import struct

NAMES = ["name", "qty", "price", "note", "tag"]
HEADER = b"name,qty,price,note,tag\n"
TYPE_HINTS = {"name": "str", "qty": "i64", "price": "f64",
              "note": "opt_str", "tag": "opt_i64"}
KEEP_BELOW = 500
SPAN_CAP = 16344            # StageCodegen.SPAN_CAP: LDS staging window


def ci_keep(x):
    return x["qty"] < 500


def ci_up(x):
    return x.upper()


def ops(sink="csv"):
    """The csv sink writes no Option[i64] nulls, so its stage drops `tag`
    from the output (the column is still walked, as every cell is)."""
    out = [("filter", ci_keep), ("mapColumn", "name", ci_up)]
    if sink == "csv":
        out.append(("selectColumns", ["name", "qty", "price", "note"]))
    return out


def col_types():
    from tuplex_amd import ttypes as T
    return [T.STR, T.I64, T.F64, ("opt", T.STR), ("opt", T.I64)]


# ---- structured row generator ------------------------------------------------
# clean cell kinds: plain, empty, quoted with embedded commas, quoted with
# embedded newlines, quoted empty. The odd kinds are what the index must
# decline: escaped "", a stray quote pair inside an unquoted cell, junk after
# a closing quote, too few / too many cells, a bare CR, a UTF-8 cell.

ODD_KINDS = ["esc", "stray", "junk", "few", "many", "barecr", "utf8"]
# the device diverts these to the host (exception records); `stray` and
# `barecr` are ordinary cells that merely need quoting on output
DIVERTED = {"esc", "junk", "few", "many", "utf8"}


def clean_row(i, eol=b"\n", qty=None):
    name = [b"nm%d" % i, b'"Smith, J%d"' % i, b'"two\nlines %d"' % i,
            b'"a,b\n,c%d"' % i][i % 4]
    note = [b"plain", b"", b'""', b'"has, comma %d"' % i, b"n%d" % i][i % 5]
    tag = [b"%d" % (i * 3), b""][i % 2]
    qty = (i * 37) % 700 if qty is None else qty
    return b"%s,%d,%d.%s,%s,%s%s" % (name, qty, i % 90, [b"5", b"25"][i % 2],
                                    note, tag, eol)


def odd_row(i, kind, eol=b"\n"):
    """Row i of the given odd kind. Diverted kinds carry a qty the filter
    drops, so replaying them on the host yields no output row either."""
    qty = KEEP_BELOW + i if kind in DIVERTED else i % 400
    name = {"esc": b'"he said ""hi"" %d"' % i, "stray": b'ab"cd"e%d' % i,
            "junk": b'"q%d"junk' % i, "barecr": b"a\rb%d" % i,
            "utf8": b"n\xc3\xa9%d" % i}.get(kind, b"nm%d" % i)
    cells = [name, b"%d" % qty, b"1.5", b"note", b"7"]
    if kind == "few":
        cells = cells[:4]
    elif kind == "many":
        cells.append(b"extra")
    return b",".join(cells) + eol


def rows_clean(n, eol=b"\n"):
    return [clean_row(i, eol) for i in range(n)]


def rows_odd(kind):
    """Three batches and a few rows: the odd row alone in the middle of batch
    0, in lane 0 of batch 1 and in lane 63 of batch 2."""
    at = {31, 64, 191}
    return [odd_row(i, kind) if i in at else clean_row(i) for i in range(200)]


def rows_long_between():
    """64 rows of about 300 bytes (span above the staging window: that batch
    parses from global memory, unstaged) between two staged batches."""
    out = rows_clean(64)
    mid = [b"L%03d%s,%d,2.5,x,1\n" % (i, b"y" * 290, i) for i in range(64)]
    assert sum(len(r) for r in mid) > SPAN_CAP
    return out + mid + [clean_row(200 + i) for i in range(70)]


def _no_final_newline():
    rows = rows_clean(70)
    rows[-1] = rows[-1].rstrip(b"\n")
    return rows


CASES = {}
for _n in (1, 63, 64, 65, 129):
    CASES["n%d" % _n] = (lambda n=_n: rows_clean(n))
CASES["crlf"] = lambda: rows_clean(130, b"\r\n")
CASES["no_final_newline"] = _no_final_newline
CASES["long_between"] = rows_long_between
for _k in ODD_KINDS:
    CASES["odd_" + _k] = (lambda k=_k: rows_odd(k))


def case_body(case):
    return b"".join(CASES[case]())


# ---- stage builds -------------------------------------------------------------

BUILDS = {"index": "1", "walk": "0"}        # build -> TPX_CELL_INDEX


def _generate(types, names, stage_ops, sink, delimiter, build):
    from tuplex_amd import codegen, plan
    sp = plan.build_stage(types, names, stage_ops)
    assert sp.compilable, sp.why_not_compilable
    old = os.environ.get("TPX_CELL_INDEX")
    try:
        os.environ["TPX_CELL_INDEX"] = BUILDS[build]
        src, desc = codegen.generate_stage(
            sp, source="csv", sink=sink,
            csv_info={"null_values": [""], "delimiter": delimiter})
    finally:
        if old is None:
            os.environ.pop("TPX_CELL_INDEX", None)
        else:
            os.environ["TPX_CELL_INDEX"] = old
    return sp, src, desc


def generate(sink="csv", build="index"):
    """(stage plan, source, description) of the test stage."""
    return _generate(col_types(), NAMES, ops(sink), sink, ",", build)


def wide_keep(x):
    return x["c1"] < 500


def generate_wide(build="index"):
    """One column above the index's limit."""
    from tuplex_amd import codegen
    from tuplex_amd import ttypes as T
    n = codegen.StageCodegen.CI_MAX_COLS + 1
    types = [T.STR, T.I64] + [T.STR] * (n - 2)
    return _generate(types, ["c%d" % i for i in range(n)],
                     [("filter", wide_keep)], "csv", ",", build)


def generate_pipe(build="index"):
    """The test stage's shape with a '|' delimiter."""
    return _generate(col_types(), NAMES, ops("csv"), "csv", "|", build)


def precompile(verbose=False):
    from tests import pipelines
    from tuplex_amd import engine
    glib = engine.GpuLib.get()
    n = 0
    for sink in ("csv", "mem"):
        for build in BUILDS:
            _sp, src, desc = generate(sink, build)
            pipelines._stage_compile(glib, src, desc)
            n += 1
            if verbose:
                print("precompiled cell-index stage:", sink, build)
    return n


def execute(body, sink="csv", build="index"):
    """Run the stage over csv bytes (no header) through tpx_stage_execute_csv
    with flags 0. -> dict(data, offsets, indices, excs[, rows]) with excs a
    sorted list of (row, code, operator id, payload bytes) and, for the mem
    sink, rows the decoded output rows."""
    import numpy as np
    from tuplex_amd import rowfmt
    from tuplex_amd import ttypes as T
    from tuplex_amd.engine import GpuLib, TpxResult
    glib = GpuLib.get()
    glib.lib.tpx_set_device(0)
    sp, src, desc = generate(sink, build)
    stage = glib.compile_stage(src, desc)
    res = TpxResult()
    buf = (ctypes.c_uint8 * max(len(body), 1)).from_buffer_copy(
        body if body else b"\0")
    rc = glib.lib.tpx_stage_execute_csv(stage, buf, len(body), 0,
                                        ctypes.byref(res))
    if rc != 0:
        raise RuntimeError(glib.err())
    try:
        n = res.out_num_rows
        data = ctypes.string_at(res.out_data, res.out_size) \
            if res.out_size else b""
        # csv sink: n+1 offsets delimit the rows; mem sink: one per row
        n_offs = n + 1 if sink == "csv" else n
        offs = np.ctypeslib.as_array(res.out_row_offsets,
                                     shape=(n_offs,)).tolist() if n_offs else []
        idxs = np.ctypeslib.as_array(res.out_row_indices,
                                     shape=(n,)).tolist() if n else []
        excs = []
        if res.exc_num_rows:
            eb = ctypes.string_at(res.exc_data, res.exc_size)
            pos = 0
            for _ in range(res.exc_num_rows):
                row, code, opid, size = struct.unpack_from("<4q", eb, pos)
                excs.append((row, code, opid, eb[pos + 32:pos + 32 + size]))
                pos += 32 + size
        out = {"data": data, "offsets": offs, "indices": idxs,
               "excs": sorted(excs)}
        if sink == "mem":
            out["rows"] = rowfmt.deserialize_partition(
                data, T.tup(sp.gpu_output_types),
                offsets=offs if n else None) if data else []
        return out
    finally:
        glib.lib.tpx_result_free(ctypes.byref(res))

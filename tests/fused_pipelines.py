"""Stage, inputs and runner of tests/test_gpu_fused_sink.py.

A csv -> csv stage whose main kernel formats kept rows itself (the fused csv
sink: per-wave commit into a text scratch, per-batch descriptors, pair scan,
tpx_csv_gather), the same with TPX_FUSED_WINDOW=0 (rows formatted straight to
global memory, not through the per-wave LDS window) and the same stage
generated with TPX_FUSED_SINK=0 (columnar slots + tpx_stage_write). The UDFs
live at module level so that their source can be captured, and precompile()
puts all three builds into the kernel cache at build time.

Run as a program (`python -m tests.fused_pipelines CASE`) it executes one case
on the fused build and prints the result as one JSON line; the overflow test
starts it with TPX_TEXT_CAP0 set, which the library reads once per process.
"""
import ctypes
import hashlib
import json
import os
import struct
import sys

NAMES = ["name", "city", "n", "note"]
HEADER = b"name,city,n,note\n"
KEEP_BELOW = 500
SPAN_CAP = 16344            # StageCodegen.SPAN_CAP: LDS staging window
TEXT_WINDOW = 4096          # above any per-wave LDS output window


def fs_keep(x):
    return x["n"] < 500


def fs_label(x):
    if x["n"] < 3:
        return x["name"] + ' "' + x["city"] + '"'
    return x["name"] + "-" + x["city"]


def fs_cap(x):
    return x[0].upper() + x[1:].lower()


def ops():
    return [
        ("filter", fs_keep),
        ("withColumn", "label", fs_label),      # concat: allocates from the heap
        ("mapColumn", "city", fs_cap),          # capitalize: allocates too
        ("selectColumns", ["label", "city", "n", "note"]),
    ]


TYPE_HINTS = {"name": "str", "city": "str", "n": "i64", "note": "str"}


def _row(i, n, note=b"ok", name=None):
    name = name if name is not None else b"nm%d" % i
    return b"%s,cITY%d,%d,%s\n" % (name, i % 7, n, note)


def rows_pattern(count, pattern):
    """count rows, `all` kept, `none` kept or alternating."""
    out = []
    for i in range(count):
        keep = {"all": True, "none": False, "alt": i % 2 == 0}[pattern]
        out.append(_row(i, i % 400 if keep else KEEP_BELOW + i))
    return out


def rows_long_and_short():
    """64 rows of about 300 bytes (their span exceeds the staging window, so
    that batch parses from global memory) followed by short rows (staged)."""
    out = [_row(i, i, note=b"L%03d" % i + b"x" * 290) for i in range(64)]
    assert sum(len(r) for r in out) > SPAN_CAP
    out += [_row(100 + i, (100 + i) % 600) for i in range(70)]
    return out


def rows_quoting():
    """Kept cells that need quoting: a comma inside a quoted input cell, and
    (n < 3) a double quote that fs_label puts into its result. Most rows
    need none, so both the rescan and the plain-copy format paths run."""
    out = []
    for i in range(130):
        note = b'"has, comma %d"' % i if i % 5 == 0 else b"plain"
        name = b'"Smith, J%d"' % i if i % 11 == 0 else None
        out.append(_row(i, i % 8, note=note, name=name))
    return out


def rows_big_wave():
    """One batch whose text is far above TEXT_WINDOW (64 x ~200 bytes), between
    two small ones."""
    out = [_row(i, i) for i in range(64)]
    out += [_row(64 + i, i, note=b"w" * 180) for i in range(64)]
    out += [_row(128 + i, i) for i in range(10)]
    assert 64 * 180 > TEXT_WINDOW
    return out


def rows_malformed():
    """Rows the device diverts, inside batches of good rows. Wrong column
    counts are exceptions on the host path as well; the non-ASCII rows carry
    an n that the filter drops, so replaying them yields no output row
    either. -> (rows, indices of the diverted rows)."""
    out, bad = [], []
    for i in range(150):
        if i in (3, 64, 130):
            out.append(b"nm%d,only,%d\n" % (i, i))                 # 3 cells
            bad.append(i)
        elif i in (40, 127):
            out.append(b"nm%d,c,%d,x,extra\n" % (i, i))            # 5 cells
            bad.append(i)
        elif i in (17, 65):
            out.append(b"n\xc3\xa9%d,cITY,%d,ok\n" % (i, KEEP_BELOW + i))
            bad.append(i)
        else:
            out.append(_row(i, i % 700))
    return out, bad


CASES = {}
for _n in (1, 63, 64, 65, 129):
    for _p in ("all", "none", "alt"):
        CASES["n%d_%s" % (_n, _p)] = (lambda n=_n, p=_p: rows_pattern(n, p))
CASES["long_and_short"] = rows_long_and_short
CASES["quoting"] = rows_quoting
CASES["big_wave"] = rows_big_wave
CASES["malformed"] = lambda: rows_malformed()[0]


def case_body(case):
    return b"".join(CASES[case]())


# ---- stage builds -----------------------------------------------------------

BUILDS = {                      # build -> codegen-time switches
    "fused": {},                            # format through an LDS window
    "direct": {"TPX_FUSED_WINDOW": "0"},    # format straight to global memory
    "twopass": {"TPX_FUSED_SINK": "0"},
}
_SWITCHES = ("TPX_FUSED_SINK", "TPX_FUSED_WINDOW")


def generate(build="fused"):
    """(source, description) of the stage under the build's switches."""
    from tuplex_amd import codegen, plan
    from tuplex_amd import ttypes as T
    sp = plan.build_stage([T.STR, T.STR, T.I64, T.STR], NAMES, ops())
    assert sp.compilable, sp.why_not_compilable
    old = {k: os.environ.get(k) for k in _SWITCHES}
    try:
        for k in _SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(BUILDS[build])
        return codegen.generate_stage(
            sp, source="csv", sink="csv",
            csv_info={"null_values": [""], "delimiter": ","})
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def precompile(verbose=False):
    from tests import pipelines
    from tuplex_amd import engine
    glib = engine.GpuLib.get()
    for build in BUILDS:
        src, desc = generate(build)
        pipelines._stage_compile(glib, src, desc)
        if verbose:
            print("precompiled fused-sink stage:", build)
    return len(BUILDS)


def execute(body, build="fused"):
    """Run the stage over csv bytes (no header) through tpx_stage_execute_csv
    with flags 0. -> dict(text, offsets, indices, excs) with excs a sorted list
    of (row, code, operator id, payload bytes)."""
    import numpy as np
    from tuplex_amd.engine import GpuLib, TpxResult
    glib = GpuLib.get()
    glib.lib.tpx_set_device(0)
    src, desc = generate(build)
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
        text = ctypes.string_at(res.out_data, res.out_size) \
            if res.out_size else b""
        offs = np.ctypeslib.as_array(res.out_row_offsets,
                                     shape=(n + 1,)).tolist()
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
        return {"text": text, "offsets": offs, "indices": idxs,
                "excs": sorted(excs)}
    finally:
        glib.lib.tpx_result_free(ctypes.byref(res))


def digest(out):
    """A JSON-able summary that pins every byte of an execute() result."""
    h = hashlib.sha256()
    h.update(out["text"])
    h.update(repr((out["offsets"], out["indices"], out["excs"])).encode())
    return {"sha256": h.hexdigest(), "bytes": len(out["text"]),
            "rows": len(out["indices"]), "excs": len(out["excs"])}


if __name__ == "__main__":
    print(json.dumps(digest(execute(case_body(sys.argv[1])))))

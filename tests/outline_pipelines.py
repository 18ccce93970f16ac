"""Inputs and builds of tests/test_gpu_outline.py.

The stages are those of tests/cellindex_pipelines.py (csv and mem sink) and
tests/fused_pipelines.py, each generated with the cold paths out of line
(TPX_OUTLINE=1, the default) and inline (TPX_OUTLINE=0). Every input has at
most 130 rows, 64 + 64 + 2, so the last batch is partial, and puts a path
that TPX_OUTLINE moves next to the hot path in the same launch.
precompile() puts the TPX_OUTLINE=0 builds into the kernel cache at build
time; the default builds are there already.
"""
import contextlib
import os

from tests import cellindex_pipelines as CP
from tests import fused_pipelines as FP

LEVELS = ("1", "0")
CI_CAP = 958                # StageCodegen.CI_CAP: entries of the cell index
TEXT_WINDOW = 4096          # StageCodegen.WRITE_CAP: per-wave output window


@contextlib.contextmanager
def outline(level):
    old = os.environ.get("TPX_OUTLINE")
    os.environ["TPX_OUTLINE"] = level
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("TPX_OUTLINE", None)
        else:
            os.environ["TPX_OUTLINE"] = old


# ---- cell-index stage (name, qty, price, note, tag) ---------------------------

def ci_unstaged():
    """staged | unstaged (64 rows with a ~300 B cell) | staged, partial."""
    mid = [b"L%03d%s,%d,2.5,x,1\n" % (i, b"y" * 290, i) for i in range(64)]
    assert sum(len(r) for r in mid) > CP.SPAN_CAP
    return CP.rows_clean(64) + mid + [CP.clean_row(200 + i) for i in range(2)]


def ci_declined():
    """Batch 0: every kind of row the index declines, among accepted rows
    (which include quoted cells with embedded delimiters and newlines).
    Batch 1: four rows of 250 cells overflow the entry list, so the whole
    batch is walked. Batch 2: two accepted rows."""
    out = []
    for i in range(64):
        kind = {5: "esc", 11: "stray", 17: "junk", 23: "barecr", 29: "utf8",
                35: "few", 41: "many", 63: "esc"}.get(i)
        out.append(CP.odd_row(i, kind) if kind else CP.clean_row(i))
    for i in range(64, 128):
        if i % 16 == 3:
            out.append(b"nm%d,%d,1.5,n,7" % (i, CP.KEEP_BELOW + i)
                       + b",x" * 245 + b"\n")
        else:
            out.append(CP.clean_row(i))
    assert 4 * 250 > CI_CAP
    out += [CP.clean_row(128, qty=1), CP.clean_row(129, qty=2)]
    return out


def ci_direct():
    """Batch 0 fits the window; batch 1's kept text is far above it (64 rows
    with a 180 B note, a few of them quoted); batch 2 is partial."""
    out = [CP.clean_row(i, qty=i) for i in range(64)]
    for i in range(64, 128):
        note = b'"w, %s"' % (b"w" * 176) if i % 9 == 0 else b"w" * 180
        out.append(b"nm%d,%d,1.5,%s,7\n" % (i, i, note))
    assert 64 * 180 > TEXT_WINDOW
    out += [CP.clean_row(128, qty=1), CP.clean_row(129, qty=2)]
    return out


def ci_quoting():
    """Most kept rows need no quoting; a few per batch do."""
    out = []
    for i in range(130):
        name = b'"Smith, J%d"' % i if i % 13 == 0 else b"nm%d" % i
        note = b'"a ""q"" %d"' % i if i == 77 else b"plain"
        qty = CP.KEEP_BELOW + i if i == 77 else i
        out.append(b"%s,%d,2.25,%s,\n" % (name, qty, note))
    return out


def ci_badf64():
    """An f64 cell that does not parse, in lanes of batches with kept rows."""
    out = [CP.clean_row(i, qty=i) for i in range(130)]
    for i in (7, 64, 129):
        out[i] = b"nm%d,%d,12x.5,plain,7\n" % (i, i)
    return out


CI_CASES = {"unstaged": ci_unstaged, "declined": ci_declined,
            "direct": ci_direct, "quoting": ci_quoting, "badf64": ci_badf64}


def ci_execute(case, sink, level):
    with outline(level):
        return CP.execute(b"".join(CI_CASES[case]()), sink=sink, build="index")


# ---- fused-sink stage (name, city, n, note) -----------------------------------

def fs_unstaged():
    out = FP.rows_pattern(64, "alt")
    out += [FP._row(64 + i, i, note=b"L%03d" % i + b"x" * 290)
            for i in range(64)]
    assert sum(len(r) for r in out[64:]) > FP.SPAN_CAP
    return out + [FP._row(128, 1), FP._row(129, 2)]


def fs_direct_and_quoting():
    """Batch 0: a few rows to quote (n < 3 puts a '"' into the label) among
    plain ones; batch 1 above the window; batch 2 partial."""
    out = [FP._row(i, i % 16) for i in range(64)]
    out += [FP._row(64 + i, 10 + i, note=b"w" * 180) for i in range(64)]
    return out + [FP._row(128, 1), FP._row(129, 20)]


def fs_raises():
    """fs_cap takes x[0] of the city: an empty city raises IndexError in the
    UDF chain, in batches with kept rows; one such row is in the unstaged
    batch's neighbour and one in the partial batch."""
    out = [FP._row(i, i) for i in range(130)]
    for i in (9, 64, 129):
        out[i] = b"nm%d,,%d,ok\n" % (i, i)
    return out


FS_CASES = {"unstaged": fs_unstaged, "direct_quoting": fs_direct_and_quoting,
            "raises": fs_raises}


def fs_execute(case, level):
    with outline(level):
        return FP.execute(b"".join(FS_CASES[case]()), build="fused")


def precompile(verbose=False):
    from tests import pipelines
    from tuplex_amd import engine
    glib = engine.GpuLib.get()
    n = 0
    with outline("0"):
        for sink in ("csv", "mem"):
            _sp, src, desc = CP.generate(sink, "index")
            pipelines._stage_compile(glib, src, desc)
            n += 1
        src, desc = FP.generate("fused")
        pipelines._stage_compile(glib, src, desc)
        n += 1
    if verbose:
        print("precompiled inline builds:", n)
    return n

"""Regex-pipeline perf probe (GPU box): the nine-group Common-Log parse of the
logs workload over generated log lines, text source, device-resident input,
mem sink. Usage: python tests/regexprobe.py [rows_millions] [regex|strip]

  regex   ParseWithRegex (re.search, nine groups) on the device regex VM
  strip   the find/slice parser of the same workload, as a baseline

When the stage does not compile (a checkout without the regex VM) the same
pipeline is timed through the public API instead: that is the interpreter
fallback the whole stage takes there."""
import ctypes
import os
import sys
import tempfile
import time

sys.path.insert(0, ".")

from tests import regex_pipelines as RP  # noqa: E402
from tuplex_amd import codegen, plan  # noqa: E402
from tuplex_amd import ttypes as T  # noqa: E402


def main():
    mrows = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    which = sys.argv[2] if len(sys.argv) > 2 else "regex"
    fn = {"regex": RP.ParseWithRegex, "strip": RP.ParseWithStripTuple}[which]
    base = RP.well_formed_lines(50000, seed=11)
    reps = max(1, int(mrows * 1e6) // len(base))
    blob = RP.log_text_bytes(base) * reps
    n = len(base) * reps
    print("pipeline %s: %.2fM rows, %.1f MB" % (which, n / 1e6,
                                                len(blob) / 1e6), flush=True)

    ops = [("map", fn)]
    sp = plan.build_stage([T.STR], None, ops)
    if not sp.compilable:
        print("stage not compilable (%s): timing the interpreter fallback"
              % sp.why_not_compilable, flush=True)
        import tuplex_amd
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "access.log")
            with open(p, "wb") as f:
                f.write(blob)
            ctx = tuplex_amd.Context()
            t0 = time.perf_counter()
            ds = ctx.text(p).map(fn)
            got = ds.collect()
            wall = time.perf_counter() - t0
        assert len(got) == n
        print("mode %s wall %.2f s -> %.3f M rows/s"
              % (ds._last_outcome.mode, wall, n / wall / 1e6), flush=True)
        return

    from tuplex_amd.engine import GpuLib, TpxResult
    glib = GpuLib.get()
    assert glib.device_count() > 0
    src, desc = codegen.generate_stage(
        sp, source="csv", sink="mem",
        csv_info={"null_values": [], "delimiter": ",", "text_mode": True})
    stage = glib.compile_stage(src, desc)
    dev = glib.lib.tpx_dev_alloc(len(blob))
    assert dev
    buf = (ctypes.c_uint8 * len(blob)).from_buffer_copy(blob)
    assert glib.lib.tpx_dev_upload(dev, buf, len(blob)) == 0
    try:
        for it in range(7):
            t0 = time.perf_counter()
            res = TpxResult()
            rc = glib.lib.tpx_stage_execute_csv_dev(stage, dev, len(blob), 0,
                                                    0, ctypes.byref(res))
            assert rc == 0, glib.err()
            wall = (time.perf_counter() - t0) * 1e3
            assert res.out_num_rows + res.exc_num_rows == n, \
                (res.out_num_rows, res.exc_num_rows)
            if which == "regex":  # well-formed lines: nothing diverts
                assert res.exc_num_rows == 0, res.exc_num_rows
            if it >= 2:
                print("step %d wall %7.2f ms  kernels %6.2f d2h %6.2f  main "
                      "%6.3f compact %6.3f write %6.3f  -> %.1f M rows/s"
                      % (it, wall, res.t_kernel_ms, res.t_d2h_ms,
                         res.t_main_ms, res.t_compact_ms, res.t_write_ms,
                         n / wall / 1e3), flush=True)
            glib.lib.tpx_result_free(ctypes.byref(res))
    finally:
        glib.lib.tpx_dev_free(dev)


if __name__ == "__main__":
    main()

"""Hash-join perf probe (GPU box): a two-column csv left input resident in
HBM, inner-joined on its i64 key to a unique-key build side of N rows (i64
key, one str column), mem sink left on the device.
Usage: python tests/joinprobe.py [build_rows] [left_rows_millions]

Prints one JSON line: where the build side lives, the stage compile time from
a cold code-object cache (a private, empty cache directory), join_build_ms,
the table's bytes and the stage's rows/s (best of 5 timed executes after 2
warm-ups).

The script runs unchanged on a checkout without device join tables: there
the embedded table serves up to 65,536 build rows, and above that the stage
does not compile — the same pipeline is then timed through the public API,
which is the interpreter fallback the whole stage takes there."""
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")

from tuplex_amd import codegen, plan  # noqa: E402
from tuplex_amd import ttypes as T  # noqa: E402


def left_csv(n_left, n_build, seed=7):
    """key,val lines; keys uniform over twice the build key range (about
    half of the rows hit)."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 2 * n_build, size=n_left)
    vals = rng.integers(0, 1000, size=n_left)
    return ("\n".join("%d,%d" % kv for kv in zip(keys.tolist(),
                                                vals.tolist()))
            + "\n").encode(), keys


def main():
    n_build = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    n_left = int(float(sys.argv[2]) * 1e6) if len(sys.argv) > 2 else 4950000
    out = {"build_rows": n_build, "left_rows": n_left}
    t0 = time.perf_counter()
    build = [(i, "name-%d" % i) for i in range(n_build)]
    blob, keys = left_csv(n_left, n_build)
    hits = int((keys < n_build).sum())
    out["t_make_inputs_s"] = round(time.perf_counter() - t0, 2)
    jop = ("join", build, ["k", "name"], "key", "k", "inner", "", "", "", "")

    t0 = time.perf_counter()
    sp = plan.build_stage([T.I64, T.I64], ["key", "val"], [jop])
    out["t_plan_s"] = round(time.perf_counter() - t0, 2)
    if not sp.compilable:
        out["join_table"] = "none"
        out["mode"] = "fallback"
        out["reason"] = sp.why_not_compilable
        import tuplex_amd
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "left.csv")
            with open(p, "wb") as f:
                f.write(b"key,val\n" + blob)
            ctx = tuplex_amd.Context()
            rds = ctx.parallelize(build, columns=["k", "name"])
            t0 = time.perf_counter()
            ds = ctx.csv(p).join(rds, "key", "k")
            got = ds.collect()
            wall = time.perf_counter() - t0
        assert len(got) == hits, (len(got), hits)
        out["mode"] = ds._last_outcome.mode
        out["wall_s"] = round(wall, 2)
        out["stage_mrows_s"] = round(n_left / wall / 1e6, 4)
        print(json.dumps(out), flush=True)
        return

    from tuplex_amd import engine
    from tuplex_amd.engine import GpuLib, TpxResult
    glib = GpuLib.get()
    assert glib.device_count() > 0
    device_joins = getattr(sp, "device_joins", None) or []
    out["join_table"] = "device" if device_joins else "embedded"
    t0 = time.perf_counter()
    src, desc = codegen.generate_stage(
        sp, source="csv", sink="mem",
        csv_info={"null_values": [""], "delimiter": ",", "text_mode": False})
    out["t_codegen_s"] = round(time.perf_counter() - t0, 2)
    out["source_bytes"] = len(src)
    with tempfile.TemporaryDirectory() as cold:
        engine._CACHE_DIR = cold      # cold code-object cache
        t0 = time.perf_counter()
        stage = glib.compile_stage(src, desc)
        out["t_compile_s"] = round(time.perf_counter() - t0, 2)
    tabs = []
    if device_joins:
        from tuplex_amd import jointab
        t0 = time.perf_counter()
        tabs = jointab.stage_tables(glib, stage, sp, 0)
        out["t_table_s"] = round(time.perf_counter() - t0, 3)
        out["join_build_ms"] = round(sum(t.build_ms for _, t in tabs), 4)
        out["join_table_bytes"] = sum(t.bytes for _, t in tabs)
    dev = glib.lib.tpx_dev_alloc(len(blob))
    assert dev
    buf = np.frombuffer(blob, dtype=np.uint8)
    assert glib.lib.tpx_dev_upload(dev, buf.ctypes.data, len(blob)) == 0
    best = None
    try:
        for it in range(7):
            if tabs:
                jointab.bind_tables(stage, tabs)
            t0 = time.perf_counter()
            res = TpxResult()
            rc = glib.lib.tpx_stage_execute_csv_dev(stage, dev, len(blob), 0,
                                                    2, ctypes.byref(res))
            assert rc == 0, glib.err()
            wall = (time.perf_counter() - t0) * 1e3
            assert res.exc_num_rows == 0, res.exc_num_rows
            assert res.out_num_rows == hits, (res.out_num_rows, hits)
            if it >= 2 and (best is None or wall < best[0]):
                best = (wall, res.t_kernel_ms, res.t_main_ms)
            glib.lib.tpx_result_free(ctypes.byref(res))
    finally:
        glib.lib.tpx_dev_free(dev)
    out["mode"] = "gpu"
    out["wall_ms"] = round(best[0], 3)
    out["t_kernel_ms"] = round(best[1], 3)
    out["t_main_ms"] = round(best[2], 3)
    out["stage_mrows_s"] = round(n_left / best[0] / 1e3, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""cache() probe: time from the cache() call to the result of
cached.filter(...).aggregate(...) over Zillow-shaped rows (tests/zillow_data.py),
one warm-up and then REPEATS timed runs in one process, one JSON line per run.

    python tests/cacheprobe.py [--rows 1000000] [--repeats 4] [--tree DIR]

--tree runs the package of another checkout (the parent commit, say) with this
same script, so both sides execute the same pipeline; the post-cache UDFs
index columns by position because a host cache of a csv source used to drop
the header's names. With a device cache the last line also gives the pack's
bytes/s next to a plain device-to-device copy of the same bytes in the same
process — that copy, not a datasheet figure, is the pack's yardstick."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def add(a, b):
    return a + b


def acc_len(a, x):
    return a + len(x[2])


def run(ctx, path):
    t0 = time.perf_counter()
    ds = ctx.csv(path)
    ds = ds.filter(lambda x: x["state"] != "TX")
    cached = ds.cache()
    t1 = time.perf_counter()
    ds2 = cached.filter(lambda x: x[4] > 20000.0)
    ds2 = ds2.aggregate(add, acc_len, 0)
    got = ds2.collect()
    t2 = time.perf_counter()
    return got, t1 - t0, t2 - t1, cached, ds2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--csv", default=None, help="reuse an input file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    from tests.zillow_data import make_zillow_csv_bytes
    sys.path.insert(0, args.tree)
    import tuplex_amd

    tmp = tempfile.TemporaryDirectory()
    path = args.csv
    if not path:
        path = os.path.join(tmp.name, "zillow.csv")
        data, _ = make_zillow_csv_bytes(args.rows, seed=42, dirty_frac=0.0)
        with open(path, "wb") as f:
            f.write(data)
    ctx = tuplex_amd.Context()
    runs = []
    cached = None
    for r in range(args.repeats + 1):
        got, tc, t2, cached, ds2 = run(ctx, path)
        m1 = cached._last_outcome.metrics
        m2 = ds2._last_outcome.metrics
        rec = {"warmup": r == 0, "result": got, "t_cache_s": tc,
               "t_stage2_s": t2, "t_total_s": tc + t2,
               "cache": m1.get("cache"),
               "stage1_t_kernel_ms": m1.get("t_kernel_ms"),
               "stage1_t_pack_ms": m1.get("t_pack_ms"),
               "stage2_mode": ds2._last_outcome.mode,
               "stage2_t_main_ms": m2.get("t_main_ms"),
               "stage2_t_kernel_ms": m2.get("t_kernel_ms")}
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    src = cached._source
    if getattr(src, "kind", "") != "dcached":
        return
    nbytes = sum(t.bytes for t in src.tables)
    from tests import hipkern
    hip = hipkern._libs()[0]
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(a), nbytes) == 0
    assert hip.hipMalloc(ctypes.byref(b), nbytes) == 0
    best = None
    for _ in range(6):
        hip.hipDeviceSynchronize()
        t0 = time.perf_counter()
        assert hip.hipMemcpy(b, a, nbytes, 3) == 0  # device to device
        hip.hipDeviceSynchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    hip.hipFree(a)
    hip.hipFree(b)
    packs = [r["stage1_t_pack_ms"] for r in runs if not r["warmup"]]
    print(json.dumps({
        "table_bytes": nbytes, "table_rows": sum(t.rows for t in src.tables),
        "d2d_best_s": best, "d2d_GBps": nbytes / best / 1e9,
        "pack_GBps": [nbytes / (p / 1e3) / 1e9 for p in packs]}), flush=True)


if __name__ == "__main__":
    main()

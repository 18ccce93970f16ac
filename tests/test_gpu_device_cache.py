"""End-to-end tests of the device-resident cache(): a compiled csv pipeline's
kept rows stay in HBM as columnar partitions (metrics["cache"] == "device"),
downstream stages read them through the columnar source, and everything a
cached pipeline returns — rows, order, exception counts — equals the same
pipeline without cache(). Input and pipelines: tests/cache_pipelines.py
(precompiled by build()). The uncached reference of each shape is computed
once and shared."""
import os
import subprocess
import sys

import pytest

import tuplex_amd
from tests import cache_pipelines as CP
from tuplex_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dirty_csv(tmp_path_factory):
    p = os.path.join(str(tmp_path_factory.mktemp("dcache")), "in.csv")
    CP.write_csv(p, CP.N_DIRTY)
    return p


_plain = {}


def _uncached(path, post):
    """(rows, exception counts) of the pipeline without cache()."""
    if post not in _plain:
        ds = post(CP.stage1(tuplex_amd.Context(), path))
        _plain[post] = (ds.collect(), dict(ds.exception_counts))
    return _plain[post]


def _cached(ctx, path):
    cached = CP.stage1(ctx, path).cache()
    return cached, cached._last_outcome.metrics


@pytest.mark.parametrize("post,unordered,gpu2", [
    (CP.f_filter, False, True), (CP.f_map_filter, False, True),
    (CP.f_sum, False, True), (CP.f_sum_by_key, True, True),
    (CP.f_raises, False, True), (CP.f_resolve, False, False),
    (CP.f_ident, False, False)],
    ids=["filter", "map_filter", "sum", "sum_by_key", "stage2_exceptions",
         "deferred_resolve", "direct_collect"])
def test_cached_equals_uncached(dirty_csv, post, unordered, gpu2):
    want, wantc = _uncached(dirty_csv, post)
    assert len(want) > 0 and want != [0]
    cached, m = _cached(tuplex_amd.Context(), dirty_csv)
    assert m["cache"] == "device", m
    assert cached._source.kind == "dcached" and cached._source.tables
    ds = post(cached)
    got = ds.collect()
    if unordered:
        got, want = sorted(got), sorted(want)
    assert got == want
    assert ds.exception_counts == wantc
    assert "ValueError" in wantc          # 'notanint' stays an exception
    if gpu2:
        assert ds._last_outcome.mode == "gpu"
        assert ds._last_outcome.metrics["partitions"] >= 1
    if post is CP.f_raises:
        # the second stage raised on cached rows: replayed from the lazily
        # downloaded host copy of the partition
        assert wantc.get("ZeroDivisionError", 0) > 100
        assert any(t._host is not None for t in cached._source.tables)
    elif post is CP.f_resolve:
        assert "ZeroDivisionError" not in wantc
        assert len(got) > len(_uncached(dirty_csv, CP.f_ident)[0])
    else:
        assert wantc.get("ZeroDivisionError", 0) >= 1


def test_dirty_rows_are_where_the_design_puts_them(dirty_csv):
    """Rows the interpreter resolved are host extras, stored exceptions are
    pending, and the tables hold the rest; nothing was downloaded."""
    cached, m = _cached(tuplex_amd.Context(), dirty_csv)
    src = cached._source
    assert len(src.extras) >= 5 and len(src.pending) >= 5
    n_tab = sum(t.rows for t in src.tables)
    assert n_tab > 2000
    assert n_tab + len(src.extras) == len(_uncached(dirty_csv, CP.f_ident)[0])
    assert all(len(t.keys) == t.rows for t in src.tables)
    assert all(t._host is None for t in src.tables)
    assert cached._last_outcome.exception_counts == {}


def test_option_off_keeps_the_host_cache(dirty_csv):
    ctx = tuplex_amd.Context({"tuplex.gpu.deviceCache": False})
    cached, m = _cached(ctx, dirty_csv)
    assert m["cache"] == "host"
    assert m["cache_reason"] == "tuplex.gpu.deviceCache is off"
    assert cached._source.kind == "cached"
    for post in (CP.f_filter, CP.f_sum):
        want, wantc = _uncached(dirty_csv, post)
        ds = post(cached)
        assert ds.collect() == want and ds.exception_counts == wantc


def test_cache_of_cache_and_tocsv(dirty_csv, tmp_path):
    want, wantc = _uncached(dirty_csv, CP.f_filter)
    cached, _m = _cached(tuplex_amd.Context(), dirty_csv)
    again = cached.cache()
    ds = CP.f_filter(again)
    assert ds.collect() == want and ds.exception_counts == wantc
    p1 = os.path.join(str(tmp_path), "a.csv")
    p2 = os.path.join(str(tmp_path), "b.csv")
    CP.f_filter(CP.stage1(tuplex_amd.Context(), dirty_csv)).tocsv(p1)
    CP.f_filter(cached).tocsv(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()


def _xfer_run(path):
    """(result, d2h of cache(), h2d + d2h of the following filter+aggregate,
    h2d of cache())."""
    glib = engine.GpuLib.get()
    ctx = tuplex_amd.Context()
    h0, d0 = glib.xfer_stats()
    cached = CP.clean_source(ctx, path).cache()
    h1, d1 = glib.xfer_stats()
    assert cached._last_outcome.metrics["cache"] == "device"
    ds = CP.f_clean_sum(cached)
    got = ds.collect()
    h2, d2 = glib.xfer_stats()
    assert ds._last_outcome.mode == "gpu"
    return got, d1 - d0, (h2 - h1) + (d2 - d1), h1 - h0


def test_transfers_do_not_scale_with_rows(tmp_path):
    """Same script at N and 4N clean rows. cache() may bring back 8 bytes per
    row (the keys) more, plus 4 KiB; the stage over the cache nothing but
    4 KiB more. The host cache moves the row bytes (~100 B per row) each
    way."""
    n = 5000
    p1 = os.path.join(str(tmp_path), "n.csv")
    p4 = os.path.join(str(tmp_path), "n4.csv")
    CP.write_csv(p1, n, dirty=False)
    CP.write_csv(p4, 4 * n, dirty=False)
    got1, cache_d2h_1, stage2_1, up1 = _xfer_run(p1)
    got4, cache_d2h_4, stage2_4, up4 = _xfer_run(p4)
    assert got1 == [sum(a for a in range(n) if a % 3 == 0)]
    assert got4 == [sum(a for a in range(4 * n) if a % 3 == 0)]
    print("cache d2h %d -> %d, stage 2 h2d+d2h %d -> %d, cache h2d %d -> %d"
          % (cache_d2h_1, cache_d2h_4, stage2_1, stage2_4, up1, up4))
    # the counters do count: the input itself went up once
    assert up4 - up1 >= os.path.getsize(p4) - os.path.getsize(p1) - 64
    assert cache_d2h_4 - cache_d2h_1 <= 8 * 3 * n + 4096
    assert stage2_4 - stage2_1 <= 4096


_ALLOC_FAIL = r"""
import sys
sys.path.insert(0, %r)
import tuplex_amd
from tests import cache_pipelines as CP
ctx = tuplex_amd.Context()
want = CP.f_clean_sum(CP.clean_source(ctx, %r)).collect()
cached = CP.clean_source(ctx, %r).cache()
m = cached._last_outcome.metrics
assert m["cache"] == "host", m
assert m["cache_reason"].startswith("device allocation failed"), m
assert cached._source.kind == "cached"
assert CP.f_clean_sum(cached).collect() == want
print("FALLBACK-OK")
"""


def test_failed_table_allocation_falls_back_to_the_host_cache(tmp_path):
    """TPX_TABLE_MAX_BYTES (read once per process, hence the child) makes
    the table allocation fail: no partial table, today's host cache."""
    p = os.path.join(str(tmp_path), "in.csv")
    CP.write_csv(p, 400, dirty=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(str(tmp_path), "child.py")
    with open(script, "w") as f:
        f.write(_ALLOC_FAIL % (root, p, p))
    env = dict(os.environ, TPX_TABLE_MAX_BYTES="1024")
    out = subprocess.run([sys.executable, script], env=env, timeout=120,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"FALLBACK-OK" in out.stdout, \
        out.stdout.decode("utf-8", "replace")[-3000:]

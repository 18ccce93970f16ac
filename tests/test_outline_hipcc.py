"""Code-object guard for the out-of-line cold paths (no GPU): the Zillow bench
stage, compiled for gfx950 through tpx_stage_compile as
tests/test_cellindex_hipcc.py does, keeps tpx_stage_main free of VGPR spills
and at 40 960 B of LDS, and the code of tpx_stage_main plus every device
function of the object stays at or below half of what tpx_stage_main alone
was with everything inlined (789 552 B). The bound guards against re-inlining;
it is no tuning target (measured sizes: profiles/README.md, round 6)."""
import os
import re
import subprocess

from tests import test_cellindex_hipcc as H

PARENT_MAIN_BYTES = 789552
READELF = H.READELF


def _code_object(src, desc):
    cache = H._compile_only(src, desc)
    raw = src.encode()
    h = 1469598103934665603
    for c in raw:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    path = os.path.join(cache, "tpx_%016x_%d_g2.hsaco" % (h, len(raw)))
    assert os.path.exists(path), path
    return path


def _kernel_note(path, kernel, key):
    notes = subprocess.check_output([READELF, "--notes", path]).decode()
    # one metadata map per kernel, keys in alphabetical order
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s*\d+", notes,
                         re.S):
        blk = m.group(0)
        if re.search(r"\.name:\s*%s\s" % re.escape(kernel), blk):
            return int(re.search(r"\.%s:\s*(\d+)" % key, blk).group(1))
    raise AssertionError("%s not found in %s" % (kernel, path))


def _function_sizes(path):
    """-> ({kernel: bytes}, {device function: bytes}) from the symbol table;
    a kernel is a function with a NAME.kd descriptor beside it."""
    out = subprocess.check_output([READELF, "-sW", path]).decode()
    funcs, kds = {}, set()
    for ln in out.splitlines():
        f = ln.split()
        if len(f) < 8:
            continue
        if f[3] == "FUNC":
            funcs[f[7]] = int(f[2])
        elif f[7].endswith(".kd"):
            kds.add(f[7][:-3])
    kernels = {k: v for k, v in funcs.items() if k in kds}
    device = {k: v for k, v in funcs.items() if k not in kds}
    return kernels, device


def test_bench_stage_main_is_small_and_spill_free():
    old = os.environ.pop("TPX_OUTLINE", None)
    try:
        src, desc = H._bench_stage()[:2]
    finally:
        if old is not None:
            os.environ["TPX_OUTLINE"] = old
    assert "#define TPX_OUTLINE 1" in src
    path = _code_object(src, desc)
    spills = _kernel_note(path, "tpx_stage_main", "vgpr_spill_count")
    lds = _kernel_note(path, "tpx_stage_main", "group_segment_fixed_size")
    kernels, device = _function_sizes(path)
    main = kernels["tpx_stage_main"]
    total = main + sum(device.values())
    print("tpx_stage_main %d B, VGPR spills %d, LDS %d B" % (main, spills, lds))
    for name, size in sorted(device.items()):
        print("  %7d B  %s" % (size, name))
    print("total %d B (limit %d)" % (total, PARENT_MAIN_BYTES // 2))
    assert device, "no out-of-line device function in the object"
    assert spills == 0
    assert lds == H.LDS_LIMIT
    assert total <= PARENT_MAIN_BYTES // 2

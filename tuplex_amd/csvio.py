"""CSV source/sink host orchestration.

Replaces the reference's file-input path: FileInputOperator sampling + CSVStatistic
type sniffing (utils/src/CSVStatistic.cc; normal-case threshold
ContextOptions.cc:216), file splitting (LocalBackend.cc:552-658), CSVReader.cc:390
reading, and the tocsv merge (LocalBackend.cc:1104/:2378). Row-boundary detection
and parsing run on the GPU (quote-parity scan kernels + the generated fused parse,
csrc/tpx_rt.hip.h); this module handles sniffing, exception-row replay (raw-line
payloads, BADPARSE_STRING_INPUT semantics ExceptionCodes.h:118) and ordered merges.

Sniffing rules (restating CSVStatistic's behavior at subsystem level — the exact
sample statistics code is LLVM-independent but large; rule set documented in
DESIGN.md and mirrored bit-for-bit by the oracle):
 - header: if not specified, present iff every cell of row 0 fails numeric/bool
   parse while some cell in the remaining sample parses;
 - per column over the sample: i64 if (parses_i64 + nulls)/n >= normalcaseThreshold,
   else f64, else bool, else plain str; Option-wrapped iff nulls were seen (for
   numeric/bool columns); str columns stay plain str (null-value optimization off,
   the Zillow Z1 configuration).
"""
import csv as _pycsv
import ctypes
import glob
import io
import os
from typing import List, Optional

from . import codegen, jointab, plan, rowfmt
from . import ttypes as T
from . import resolve as _resolve
from . import presolve
from .engine import GpuLib, TpxResult, CollectOutcome


# ---- host-side RFC-4180 helpers (sniffing + replay; oracle mirrors these) --------

def split_rows(data: bytes) -> List[bytes]:
    """Row split by the quote-parity rule (matches the GPU scan exactly)."""
    rows = []
    start = 0
    parity = 0
    for i, b in enumerate(data):
        if b == 0x22:  # '"'
            parity ^= 1
        elif b == 0x0A and parity == 0:
            rows.append(data[start:i + 1])
            start = i + 1
    if start < len(data):
        rows.append(data[start:])
    return rows


def split_cells(line: bytes, delim: bytes = b","):
    """Cell split matching tpx_csv_next_cell: returns (cells, flags) where each
    cell is bytes (quoted cells: inner bytes, '""' NOT unescaped) and flags has
    bit1=escaped, bit2=bad structure."""
    end = len(line)
    while end > 0 and line[end - 1:end] in (b"\n", b"\r"):
        end -= 1
    cells, flags = [], 0
    p = 0
    more = True
    while more:
        more = False
        if p < end and line[p:p + 1] == b'"':
            s = p + 1
            q = s
            esc = False
            while q < end:
                if line[q:q + 1] == b'"':
                    if q + 1 < end and line[q + 1:q + 2] == b'"':
                        esc = True
                        q += 2
                        continue
                    break
                q += 1
            if q >= end:
                cells.append(line[p:end])
                flags |= 4
                return cells, flags
            cells.append(line[s:q])
            if esc:
                flags |= 2
            q += 1
            if q < end and line[q:q + 1] != delim:
                flags |= 4
            while q < end and line[q:q + 1] != delim:
                q += 1
            if q < end:
                more = True
                q += 1
            p = q
        else:
            q = p
            while q < end and line[q:q + 1] != delim:
                q += 1
            cells.append(line[p:q])
            if q < end:
                more = True
                q += 1
            p = q
    return cells, flags


_PYWS = " \t\n\r\x0b\x0c"


def _try_i64(s: str):
    """Host restatement of trim+fast_atoi64 (StringUtils.cc:22) for sniffing."""
    t = s.strip(_PYWS)
    if not t:
        return None
    i, n = 0, len(t)
    if t[0] == "-":
        i = 1
    j = i
    while j < n and "0" <= t[j] <= "9":
        j += 1
    if j != n:
        return None
    v = int(t[i:] or "0")
    return -v if t[0] == "-" else v


def try_f64(s: str):
    """Host restatement of trim+fast_atod ACCEPTANCE (StringUtils.cc:71 — incl.
    its quirks: '-', '.', 'e5' all parse). Value not needed for sniffing."""
    t = s.strip(_PYWS)
    if not t:
        return False
    p, n = 0, len(t)
    if t[p] in "+-":
        p += 1
    while p < n and t[p].isdigit():
        p += 1
    if p < n and t[p] == ".":
        p += 1
        while p < n and t[p].isdigit():
            p += 1
    if p < n and t[p] in "eE":
        p += 1
        if p < n and t[p] in "+-":
            p += 1
        while p < n and t[p].isdigit():
            p += 1
    if p == n:
        return True
    # nan/inf match only with nothing consumed before (no sign: fast_atod's
    # p==start precondition)
    return p == 0 and t.lower() in ("nan", "inf", "infinity")


_BOOL_STRS = {"true", "t", "yes", "y", "1", "false", "f", "no", "n", "0"}


def _try_bool(s: str):
    return s.strip(_PYWS).lower() in _BOOL_STRS


def apply_type_hints(col_types, names, hints):
    """context.csv type_hints (context.py:288): per-column overrides keyed by
    index or name; python types / typing.Optional map onto the lattice."""
    if not hints:
        return col_types
    import typing

    def to_t(h):
        if h is int:
            return T.I64
        if h is float:
            return T.F64
        if h is bool:
            return T.BOOL
        if h is str:
            return T.STR
        origin = typing.get_origin(h)
        if origin is typing.Union:
            args = [a for a in typing.get_args(h) if a is not type(None)]
            if len(args) == 1:
                return T.opt(to_t(args[0]))
        raise ValueError("unsupported type hint %r" % (h,))

    out = list(col_types)
    for k, h in hints.items():
        i = names.index(k) if isinstance(k, str) else int(k)
        out[i] = to_t(h)
    return out


def sniff_delimiter(sample: bytes) -> bytes:
    """Most frequent candidate separator in the first row, quotes respected
    (ContextOptions.cc csv.separators [',', ';', '|', '\\t'])."""
    first = split_rows(sample)[0]
    best, bestn = b",", -1
    for cand in (b",", b";", b"|", b"\t"):
        n = len(split_cells(first, cand)[0])
        if n > bestn:
            best, bestn = cand, n
    return best


def sniff(sample: bytes, null_values: List[str], threshold: float,
          header: Optional[bool], columns: Optional[List[str]],
          delim: bytes = b","):
    """Returns (has_header, column_names, column_types)."""
    rows = [split_cells(r, delim)[0] for r in split_rows(sample)]
    rows = [r for r in rows if r]
    if not rows:
        raise ValueError("empty csv sample")
    txt_rows = [[c.decode("utf-8", "replace") for c in r] for r in rows]

    def numericish(cell):
        return _try_i64(cell) is not None or try_f64(cell) or _try_bool(cell)

    if header is None:
        r0 = txt_rows[0]
        rest = txt_rows[1:1001]
        has_header = (len(txt_rows) > 1
                      and not any(numericish(c) for c in r0 if c)
                      and any(numericish(c) for r in rest for c in r))
    else:
        has_header = header
    names = None
    if has_header:
        names = txt_rows[0]
        data_rows = txt_rows[1:]
    else:
        data_rows = txt_rows
    if columns:
        names = list(columns)
    ncols = max(len(r) for r in data_rows[:1000]) if data_rows else len(names or [])
    if names is None:
        names = ["column%d" % i for i in range(ncols)]
    ncols = len(names)

    types = []
    nulls = set(null_values)
    for k in range(ncols):
        n = n_i = n_f = n_b = n_nul = 0
        for r in data_rows[:10000]:
            if k >= len(r):
                continue
            c = r[k]
            n += 1
            if c in nulls:
                n_nul += 1
            elif _try_i64(c) is not None:
                n_i += 1
                n_f += 1  # ints parse as floats too
            elif try_f64(c):
                n_f += 1
            elif _try_bool(c):
                n_b += 1
        if n == 0:
            types.append(T.STR)
            continue
        if (n_i + n_nul) / n >= threshold and n_i > 0:
            t = T.I64
        elif (n_f + n_nul) / n >= threshold and n_f > 0:
            t = T.F64
        elif (n_b + n_nul) / n >= threshold and n_b > 0:
            t = T.BOOL
        else:
            types.append(T.STR)
            continue
        types.append(T.opt(t) if n_nul > 0 else t)
    return has_header, names, types


# ---- replay of exception rows ----------------------------------------------------

def replay_csv_row(raw_line: bytes, col_types, null_values, logical_ops, columns,
                   delim: str = ",", used=None):
    """Interpreter replay of a diverted CSV row (BADPARSE semantics,
    ResolveTask.cc:459 interpreter path with parse_cells). Full RFC-4180 parse
    (with unescaping) then CPython-typed conversion; structure/convert failures
    keep the row an exception."""
    text = raw_line.decode("utf-8", "replace")
    text = text.rstrip("\n").rstrip("\r")
    try:
        cells = next(_pycsv.reader(io.StringIO(text), delimiter=delim))
    except (StopIteration, _pycsv.Error):
        return ("exc", _BadParse("unparseable line"))
    if len(cells) != len(col_types):
        return ("exc", _BadParse("cell count %d != %d" % (len(cells),
                                                          len(col_types))))
    vals = []
    for ci, (c, t) in enumerate(zip(cells, col_types)):
        base = T.deopt(t)
        if used is not None and ci not in used:
            vals.append(c)  # pushdown: unused column stays unconverted
            continue
        if T.is_opt(t) and c in null_values:
            vals.append(None)
            continue
        try:
            if base == T.I64:
                vals.append(int(c.strip(_PYWS)))
            elif base == T.F64:
                vals.append(float(c.strip(_PYWS)))
            elif base == T.BOOL:
                s = c.strip(_PYWS).lower()
                if s in ("true", "t", "yes", "y", "1"):
                    vals.append(True)
                elif s in ("false", "f", "no", "n", "0"):
                    vals.append(False)
                else:
                    raise ValueError(c)
            else:
                vals.append(c)
        except ValueError as e:
            return ("exc", e)
    if len(col_types) == 1:  # single-column datasets carry scalar rows
        return _resolve.replay_row(vals[0], logical_ops, columns,
                                   scalar_input=True)
    return _resolve.replay_row(tuple(vals), logical_ops, columns,
                               scalar_input=False)


def replay_text_row(raw_line: bytes, col_type, null_values, logical_ops):
    """text() replay: the value IS the line (minus newline); null_values map
    matching lines to None."""
    v = raw_line.decode("utf-8", "replace")
    if v.endswith("\n"):
        v = v[:-1]
    if v.endswith("\r"):
        v = v[:-1]
    if T.is_opt(col_type) and v in null_values:
        v = None
    return _resolve.replay_row(v, logical_ops, None, scalar_input=True)


def split_points(data, target: int):
    """Row-aligned chunk boundaries every ~target bytes with EXACT quote-parity
    (the reference's findLineStart purpose, CSVUtils.cc:1494: a ranged chunk must
    start at a true row start; quoted newlines must not split a row).

    Quote parity is established from per-block quote counts computed with
    numpy (SIMD, ~10 GB/s) instead of bytes.count over ever-growing ranges —
    the old form cost ~1.3 s/GB on the e2e file->file path. `data` may be any
    buffer (bytes or mmap)."""
    import numpy as _np
    n = len(data)
    points = [0]
    if n == 0:
        return [0, 0]
    arr = _np.frombuffer(data, dtype=_np.uint8)
    B = 1 << 22
    nb = (n + B - 1) // B
    # per-block quote counts: numpy releases the GIL, so big inputs fan the
    # blocks over a thread pool (~1.1 GB/s/core measured)
    counts = [0] * nb

    def _cnt(b):
        counts[b] = int(_np.count_nonzero(arr[b * B:(b + 1) * B] == 34))
    if nb > 64:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 8)) as ex:
            list(ex.map(_cnt, range(nb)))
    else:
        for b in range(nb):
            _cnt(b)
    qc = [0] * (nb + 1)  # qc[b] = quotes in data[:b*B]
    total_q = 0
    for b in range(nb):
        total_q += counts[b]
        qc[b + 1] = total_q

    def parity_before(p):
        b = p >> 22
        return (qc[b] + int(_np.count_nonzero(arr[b << 22:p] == 34))) & 1

    find = data.find
    pos = target
    while pos < n:
        nl = find(b"\n", pos)
        if total_q:
            while nl >= 0 and parity_before(nl):
                nl = find(b"\n", nl + 1)
        if nl < 0:
            break
        points.append(nl + 1)
        pos = nl + 1 + target
    points.append(n)
    return points


class _BadParse(Exception):
    """Internal marker for structurally bad CSV rows; surfaces as
    'BadParseStringInput' in exception_counts (BADPARSE_STRING_INPUT,
    ExceptionCodes.h:118)."""


_BadParse.__name__ = "BadParseStringInput"


# ---- multi-GPU plumbing ----------------------------------------------------------
#
# The reference fans ranged tasks over executor threads inside LocalBackend
# (LocalBackend.cc:491 createLoadAndTransformToMemoryTasks, :552-658 range
# split). The MI355X-native analog has two shapes, both driven from here:
#   * one PROCESS per GPU (torchrun; torch.distributed initialized): each rank
#     takes chunks ci % world == rank and the final merge is a collective
#     (RCCL over xGMI when the backend is nccl, gloo on CPU);
#   * one THREAD per GPU inside a single process (plain `Context()` user with
#     N visible devices): chunks are pulled from a shared queue by per-device
#     worker threads (hipSetDevice is per-thread; the .so keeps per-device
#     arenas/streams/modules), results merged in chunk order.
# Chunk ordering keys are composite (chunk_index << 40) + local_row so a
# worker never needs the row counts of chunks it didn't process.

_CHUNK_SHIFT = 40


def _dist():
    """torch.distributed if it is initialized (bench/torchrun path), else None.
    torch is deliberately NOT imported unless the caller runs distributed."""
    import sys
    if "torch" not in sys.modules:
        return None
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist
    except Exception:
        pass
    return None


def _gather_objects(dist, obj):
    """all_gather_object over the active backend; returns list of per-rank
    objects in rank order."""
    world = dist.get_world_size()
    out = [None] * world
    dist.all_gather_object(out, obj)
    return out


def _run_chunks_parallel(glib, csrc, desc, work, run_one, devices):
    """Run `run_one(ci, stage)` for every ci in `work`, fanned over one worker
    thread per device. Each thread pins its device and loads its own module
    (hipModuleLoadData is per-device). Exceptions propagate."""
    import queue as _q
    import threading
    q = _q.Queue()
    for ci in work:
        q.put(ci)
    errs = []

    def worker(dev):
        try:
            glib.lib.tpx_set_device(dev)
            stage_d = glib.compile_stage(csrc, desc)
            while True:
                try:
                    ci = q.get_nowait()
                except _q.Empty:
                    return
                run_one(ci, stage_d)
        except BaseException as e:  # noqa: BLE001 - surface to caller
            errs.append(e)

    threads = [threading.Thread(target=worker, args=(d,), daemon=True)
               for d in devices]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errs:
        raise errs[0]


def _stream_files_to_device(glib, fmeta, dev, total_len, metrics):
    """Stream the input files straight to HBM through a pinned double buffer:
    file reads land in pinned memory (readinto) while an uploader thread DMAs
    the previous block (pageable hipMemcpy runs ~6 GB/s; pinned ~20 GB/s and
    the read overlaps it). The host never holds the whole input. Returns
    False on any failure — caller falls back to the host-buffered path."""
    import queue as _q
    import threading as _thr
    import time as _time
    B = 64 << 20
    pin = [glib.lib.tpx_pinned_alloc(B), glib.lib.tpx_pinned_alloc(B)]
    if not (pin[0] and pin[1]):
        for p in pin:
            if p:
                glib.lib.tpx_pinned_free(p)
        return False
    views = [(ctypes.c_char * B).from_address(p) for p in pin]
    jobs = _q.Queue(maxsize=2)
    free_slots = _q.Queue()
    free_slots.put(0)
    free_slots.put(1)
    err = []

    def uploader():
        while True:
            item = jobs.get()
            if item is None:
                return
            bi, doff, n = item
            rc = glib.lib.tpx_dev_upload(dev + doff, pin[bi], n)
            if rc != 0:
                err.append(glib.err())
                return
            free_slots.put(bi)

    th = _thr.Thread(target=uploader, daemon=True)
    th.start()
    t0 = _time.perf_counter()
    ok = False
    try:
        off = 0
        for path, hdr, ln, needs_nl in fmeta:
            with open(path, "rb") as f:
                f.seek(hdr)
                rem = ln
                while rem > 0 and not err:
                    bi = free_slots.get(timeout=120)
                    n = min(B, rem)
                    got = f.readinto(memoryview(views[bi])[:n])
                    if got != n:  # file changed underneath us
                        return False
                    jobs.put((bi, off, n))
                    off += n
                    rem -= n
            if needs_nl and not err:
                bi = free_slots.get(timeout=120)
                views[bi][0] = b"\n"
                jobs.put((bi, off, 1))
                off += 1
        ok = not err and off == total_len
        return ok
    except Exception:  # noqa: BLE001 - caller falls back
        return False
    finally:
        try:
            jobs.put(None, timeout=120)
        except Exception:  # noqa: BLE001 - uploader already dead, queue full
            pass
        th.join(timeout=120)
        for p in pin:
            glib.lib.tpx_pinned_free(p)
        if ok:
            metrics["t_h2d_ms"] += (_time.perf_counter() - t0) * 1e3


# ---- main entry ------------------------------------------------------------------

def run_csv(context, src, logical_ops, sink=None,
            keep_exceptions=False, device_cache=False) -> CollectOutcome:
    """device_cache (cache() of an eligible pipeline, engine.
    cache_eligibility): each chunk's kept rows are packed into a columnar
    device table and stay in HBM (out.device_cache) — only their row keys
    come back. Where the run turns out not to allow it (fallback stage,
    nested output type, several devices, failed device allocation) the rows
    come back as always and out.cache_reason says why."""
    opts = context.options_obj
    out = CollectOutcome()
    if device_cache:
        out.cache_reason = "stage fell back to the interpreter"

    paths = sorted(glob.glob(src.pattern)) if not os.path.isfile(src.pattern) \
        else [src.pattern]
    if "," in src.pattern and not paths:
        paths = [p for pat in src.pattern.split(",")
                 for p in (sorted(glob.glob(pat)) if not os.path.isfile(pat)
                           else [pat])]
    if not paths:
        raise FileNotFoundError(src.pattern)

    text_mode = bool(getattr(src, "text_mode", False))
    if not text_mode and src.quotechar != '"':
        # the GPU scan is specialised to RFC-4180 '"'; other quote chars take the
        # interpreter path (correct, slow — like the reference's fallback mode)
        raise NotImplementedError(
            "quotechar %r: only '\"' runs on the GPU this round" % src.quotechar)
    # sniff from a bounded sample; files are NOT read eagerly — the resident
    # path streams them straight to the device (pinned ring, below) and the
    # ranged/fallback paths load lazily via _load_data()
    with open(paths[0], "rb") as _f0:
        sample = _f0.read(256 << 10)
    if text_mode:
        # text(): one str column, rows split on every newline, no sniffing
        has_header = False
        names = None
        col_types = [T.opt(T.STR) if src.null_values else T.STR]
        delim = b","  # unused in text mode
    else:
        # sniff on the first file's sample (FileInputOperator.cc:78 semantics)
        nl = sample.rfind(b"\n")
        if nl >= 0:
            sample = sample[:nl + 1]
        delim = (src.delimiter.encode() if src.delimiter
                 else sniff_delimiter(sample))
        has_header, names, col_types = sniff(sample, src.null_values,
                                             opts.normalcase_threshold,
                                             src.header, src.columns, delim)
        col_types = apply_type_hints(col_types, names,
                                     getattr(src, "type_hints", None))

    # per-file metadata: header skip, payload length, missing trailing \n
    fmeta = []  # (path, data_off, data_len, needs_nl)
    for p in paths:
        size = os.path.getsize(p)
        hdr = 0
        if has_header:
            with open(p, "rb") as f:
                head = f.read(256 << 10)
            hnl = head.find(b"\n")
            hdr = hnl + 1 if hnl >= 0 else size
        needs_nl = False
        if size - hdr > 0:
            with open(p, "rb") as f:
                f.seek(size - 1)
                needs_nl = f.read(1) != b"\n"
        fmeta.append((p, hdr, size - hdr, needs_nl))
    total_len = sum(ln + (1 if nn else 0) for _, _, ln, nn in fmeta)
    data = None  # lazily materialized host copy (ranged / fallback paths)

    def _load_data():
        nonlocal data
        if data is None:
            parts = []
            for p, hdr, ln, nn in fmeta:
                with open(p, "rb") as f:
                    f.seek(hdr)
                    b = f.read()
                if nn:
                    b += b"\n"
                parts.append(b)
            data = (b"".join(parts) if len(parts) != 1
                    else (parts[0] if parts else b""))
        return data

    sp = plan.build_stage(col_types, names, logical_ops,
                          join_table=plan.join_table_mode(opts))
    out.output_columns = sp.output_columns  # sniffed names: cache() keeps them
    sink_kind = "csv" if (sink is not None and sink[0] == "csv") else "mem"

    if not sp.compilable:
        return _run_csv_fallback(out, _load_data(), col_types,
                                 src.null_values, logical_ops, names, sink,
                                 sp.why_not_compilable, delim.decode(),
                                 out_cols=sp.output_columns,
                                 keep_exceptions=keep_exceptions)

    glib = GpuLib.get()
    if glib.device_count() == 0:
        raise RuntimeError("no HIP device visible — the normal-case path runs only "
                           "on GPU (no CPU fallback by design)")
    glib.lib.tpx_set_device(int(opts.get("tuplex.gpu.device", "0")))

    try:
        csrc, desc = codegen.generate_stage(
            sp, source="csv", sink=sink_kind,
            csv_info={"null_values": src.null_values,
                      "delimiter": delim.decode(),
                      "text_mode": text_mode})
    except codegen.CodegenError as e:
        return _run_csv_fallback(out, _load_data(), col_types,
                                 src.null_values, logical_ops, names, sink,
                                 str(e), delim.decode(),
                                 out_cols=sp.output_columns,
                                 keep_exceptions=keep_exceptions)
    stage = glib.compile_stage(csrc, desc)
    # device join tables: built once per (join op, device), bound before
    # every execute below; without device memory for one, interpreter path
    try:
        jtabs = jointab.stage_tables(
            glib, stage, sp, int(opts.get("tuplex.gpu.device", "0")))
    except jointab.JoinTableAlloc as e:
        return _run_csv_fallback(out, _load_data(), col_types,
                                 src.null_values, logical_ops, names, sink,
                                 str(e), delim.decode(),
                                 out_cols=sp.output_columns,
                                 keep_exceptions=keep_exceptions)

    # chunked execution at inputSplitSize boundaries (LocalBackend.cc:552-658:
    # one task per 64 MB range; here one execute per range, global row indices)
    # an explicitly-set tuplex.inputSplitSize wins (reference semantics);
    # otherwise the GPU default (bigger ranges, fewer sync points)
    split = (opts.input_split_size if opts.is_set("tuplex.inputSplitSize")
             else opts.gpu_input_split_size)
    split = max(split, 64 << 10)

    import struct as _s
    import numpy as _np
    import threading as _thr
    dist = _dist()
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist else (0, 1)
    ndev = glib.device_count()
    want = int(opts.get("tuplex.gpu.devices", "0") or "0")
    from .options import parse_size
    # resident fast path (1 rank, 1 device): skip host chunking entirely —
    # one H2D, one execute; the boundary scan runs device-side
    use_resident = (world == 1 and min(want or ndev, ndev) <= 1 and
                    not opts.is_set("tuplex.inputSplitSize") and
                    total_len <= parse_size(
                        opts.get("tuplex.gpu.residentMaxSize", "24GB")))
    if use_resident:
        chunks = [0, total_len]
    else:
        _load_data()
        chunks = ([0, total_len] if total_len <= split * 2
                  else split_points(data, split))

    out.mode = "gpu"
    out.metrics = {"t_h2d_ms": 0.0, "t_kernel_ms": 0.0, "t_d2h_ms": 0.0,
                   "bytes_in": 0, "bytes_out": 0, "chunks": len(chunks) - 1}
    jointab.add_metrics(out.metrics, sp, jtabs)
    nch = len(chunks) - 1
    # device cache: decided here for what only the run knows; dcache["on"]
    # drops to False if a table cannot be allocated (rows then come back to
    # the host for that chunk, and the tables made so far are downloaded)
    dcache = {"on": False}
    if device_cache:
        from .engine import DeviceTable, cache_eligibility
        where, why = cache_eligibility(opts, src, logical_ops,
                                       sp.gpu_output_types)
        if where == "device" and (sink_kind != "mem" or not keep_exceptions):
            where, why = "host", "not a mem-sink cache run"
        if where == "device" and (world > 1 or min(want or ndev, ndev) > 1):
            where, why = "host", "multi-device fan-out"
        if where == "device" and jtabs:
            where, why = "host", "stage probes a device join table"
        dcache["on"] = where == "device"
        out.cache_reason = why
        out.metrics["t_pack_ms"] = 0.0
    chunk_tabs = [None] * nch     # device cache: DeviceTable per chunk
    my_work = [ci for ci in range(nch) if ci % world == rank]
    # per-chunk result slots, merged in chunk order below
    chunk_rows = [None] * nch     # mem sink: list[(key,row)]
    chunk_text = [None] * nch     # csv sink: (text, idxs, offs, lo, hi)
    chunk_repl = [None] * nch     # {key: [rows]} host-replayed
    chunk_excs = [None] * nch     # {exc_name: count}
    chunk_pend = [None] * nch     # keep_exceptions: [(key, raw payload)]
    mlock = _thr.Lock()
    resolve_procs = int(opts.get("tuplex.gpu.resolveProcesses", "0") or "0")
    rpool = [None]                # lazily-started parallel resolver pool
    rpool_lock = _thr.Lock()
    # zero-copy input pointers: the C side only reads the chunk bytes during
    # the call (it uploads them itself), so point straight into `data`
    data_arr = (_np.frombuffer(data, dtype=_np.uint8)
                if data is not None else None)

    def run_one(ci, stage_h):
        base = ci << _CHUNK_SHIFT  # composite ordering key namespace
        clen = chunks[ci + 1] - chunks[ci]
        res = TpxResult()
        cptr = None
        if not resident_dev:
            cptr = ctypes.cast(data_arr.ctypes.data + chunks[ci],
                               ctypes.POINTER(ctypes.c_uint8))
        tab = ctypes.c_void_p()
        packed = False
        jointab.bind_tables(stage_h, jtabs)
        if dcache["on"]:
            if resident_dev:
                rc = glib.lib.tpx_stage_cache_csv_dev(
                    stage_h, resident_dev, clen, base, ctypes.byref(res),
                    ctypes.byref(tab))
            else:
                rc = glib.lib.tpx_stage_cache_csv(
                    stage_h, cptr, clen, base, ctypes.byref(res),
                    ctypes.byref(tab))
            if rc == 2:  # TPX_E_TABLE_ALLOC: no table — today's host cache
                dcache["on"] = False
                out.cache_reason = "device allocation failed: " + glib.err()
                glib.lib.tpx_result_free(ctypes.byref(res))
                res = TpxResult()
            else:
                packed = True
        if packed:
            pass
        elif resident_dev:
            rc = glib.lib.tpx_stage_execute_csv_dev(
                stage_h, resident_dev, clen, base, 0, ctypes.byref(res))
        else:
            rc = glib.lib.tpx_stage_execute_csv(
                stage_h, cptr, clen, base, ctypes.byref(res))
        if rc != 0:
            raise RuntimeError("csv stage execute failed: " + glib.err())
        try:
            with mlock:
                for k in ("t_h2d_ms", "t_kernel_ms", "t_d2h_ms"):
                    out.metrics[k] += getattr(res, k)
                out.metrics["bytes_in"] += res.bytes_in
                out.metrics["bytes_out"] += res.bytes_out
            repl, excs = {}, {}
            if res.exc_num_rows:
                eb = ctypes.string_at(res.exc_data, res.exc_size)
                pos = 0
                rows_keys, payloads = [], []
                for _ in range(res.exc_num_rows):
                    row, ecode, opid, size = _s.unpack_from("<4q", eb, pos)
                    payloads.append(eb[pos + 32:pos + 32 + size])
                    rows_keys.append(row)
                    pos += 32 + size
                if len(payloads) >= presolve.MIN_POOL_ROWS and \
                        resolve_procs != 1:
                    # parallel host resolver (LocalBackend.cc:1254 slow-path
                    # fan-out analog): replay on a process pool
                    with rpool_lock:
                        if rpool[0] is None:
                            rpool[0] = presolve.get_pool(
                                col_types, src.null_values, logical_ops,
                                names, delim.decode(), sp.used_source_cols,
                                text_mode, processes=resolve_procs)
                    results = rpool[0].resolve(payloads)
                else:
                    results = []
                    for payload in payloads:
                        if text_mode:
                            r = replay_text_row(payload, col_types[0],
                                                src.null_values, logical_ops)
                        else:
                            r = replay_csv_row(payload, col_types,
                                               src.null_values, logical_ops,
                                               names, delim.decode(),
                                               used=sp.used_source_cols)
                        results.append(presolve._shrink(r))
                pend = []
                for (row, r), payload in zip(zip(rows_keys, results),
                                             payloads):
                    if r[0] == "row":
                        repl[row] = [r[1]]
                    elif r[0] == "excname":
                        if keep_exceptions:
                            pend.append((row, payload))
                        else:
                            excs[r[1]] = excs.get(r[1], 0) + 1
                    elif r[0] == "rows":  # 1:N join expansion
                        repl[row] = r[1]
                        for nm in r[2]:
                            excs[nm] = excs.get(nm, 0) + 1
                chunk_pend[ci] = pend
            chunk_repl[ci] = repl
            chunk_excs[ci] = excs
            if packed:
                # the rows stayed in HBM; only their keys came back
                n_out = res.out_num_rows
                keys = _np.ctypeslib.as_array(
                    res.out_row_indices, shape=(n_out,)).copy() \
                    if n_out else _np.empty(0, _np.int64)
                with mlock:
                    out.metrics["t_pack_ms"] += res.t_write_ms
                if tab.value:
                    chunk_tabs[ci] = DeviceTable(glib, tab.value, keys,
                                                 sp.gpu_output_types)
            elif sink_kind == "mem":
                out_bytes = ctypes.string_at(res.out_data, res.out_size)
                _offs = (_np.ctypeslib.as_array(
                    res.out_row_offsets,
                    shape=(res.out_num_rows,)).copy()
                    if res.out_num_rows else None)
                rws = rowfmt.deserialize_partition(out_bytes,
                                                   T.tup(sp.gpu_output_types),
                                                   offsets=_offs)
                idxs = _np.ctypeslib.as_array(
                    res.out_row_indices, shape=(res.out_num_rows,)).tolist() \
                    if res.out_num_rows else []
                chunk_rows[ci] = list(zip(idxs, rws))
            else:
                # bulk numpy copies (a python list per row costs seconds at
                # millions of kept rows — the e2e path is host-bound on this)
                text = (ctypes.string_at(res.out_data, res.out_size)
                        if res.out_size else b"")
                n_out = res.out_num_rows
                idxs = _np.ctypeslib.as_array(
                    res.out_row_indices, shape=(n_out,)).copy() \
                    if n_out else _np.empty(0, _np.int64)
                offs = _np.ctypeslib.as_array(
                    res.out_row_offsets, shape=(n_out + 1,)).copy()
                chunk_text[ci] = (text, idxs, offs, base,
                                  base + res.in_num_rows)
        finally:
            glib.lib.tpx_result_free(ctypes.byref(res))

    use_devs = min(want or ndev, ndev, max(len(my_work), 1))
    resident_dev = 0
    if use_resident:
        resident_dev = glib.lib.tpx_dev_alloc(total_len)
        if resident_dev and not _stream_files_to_device(
                glib, fmeta, resident_dev, total_len, out.metrics):
            glib.lib.tpx_dev_free(resident_dev)
            resident_dev = 0
        if not resident_dev:
            # stream/alloc failed: fall back to the host-buffered ranged path
            _load_data()
            data_arr = _np.frombuffer(data, dtype=_np.uint8)
    if resident_dev:
        try:
            run_one(0, stage)
        finally:
            glib.lib.tpx_dev_free(resident_dev)
    elif world > 1 or use_devs <= 1:
        # distributed: one device per rank, already pinned above
        for ci in my_work:
            run_one(ci, stage)
    else:
        dev0 = int(opts.get("tuplex.gpu.device", "0"))
        devices = [(dev0 + k) % ndev for k in range(use_devs)]
        _run_chunks_parallel(glib, csrc, desc, my_work, run_one, devices)
        out.metrics["devices"] = use_devs
    # pools persist across executions (presolve._POOLS; atexit shutdown)

    if device_cache and not dcache["on"]:
        # a table could not be allocated part-way: the tables made before it
        # come back to the host, so the outcome is today's host cache
        for ci, t in enumerate(chunk_tabs):
            if t is not None:
                rws = t.host_rows()
                if len(t.col_types) == 1:
                    rws = [(v,) for v in rws]
                chunk_rows[ci] = list(zip(t.keys.tolist(), rws))
                t.free()
                chunk_tabs[ci] = None

    replayed = {}
    all_rows = []
    text_parts = []
    for ci in range(nch):
        if chunk_repl[ci]:
            replayed.update(chunk_repl[ci])
        for nm, c in (chunk_excs[ci] or {}).items():
            out.exception_counts[nm] = out.exception_counts.get(nm, 0) + c
        if chunk_rows[ci]:
            all_rows.extend(chunk_rows[ci])
        if chunk_text[ci] is not None:
            text_parts.append(chunk_text[ci])
        if chunk_pend[ci]:
            out.pending.extend(chunk_pend[ci])
    if keep_exceptions:
        _nv, _ct, _nm, _dl = src.null_values, col_types, names, delim.decode()
        _tm = text_mode

        def _csv_replayer(payload, ops, _memo={}):
            ck = (len(ops), id(ops[-1]) if ops else 0)
            used2 = _memo.get(ck, -1)
            if used2 == -1:
                try:
                    used2 = plan.build_stage(_ct, _nm, ops).used_source_cols
                except Exception:  # noqa: BLE001 - fallback: parse all cells
                    used2 = None
                _memo[ck] = used2
            if _tm:
                return replay_text_row(payload, _ct[0], _nv, ops)
            return replay_csv_row(payload, _ct, _nv, ops, _nm, _dl,
                                  used=used2)
        out.pending_replayer = _csv_replayer

    if dcache["on"]:
        out.device_cache = {
            "tables": [t for t in chunk_tabs if t is not None],
            "extras": sorted(((k, v) for k, lst in replayed.items()
                              for v in lst), key=lambda t: t[0]),
            "types": list(sp.gpu_output_types),
            "device": int(opts.get("tuplex.gpu.device", "0")),
        }
        out.cache_reason = None
        out.rows = []
        return out

    if dist and world > 1:
        out.metrics["world"] = world
        if sink_kind == "mem":
            # collective union of (key,row) lists + replays; every rank folds
            # the identical union so collect() is replicated (the aggregate
            # fast path below uses a true RCCL all_reduce instead)
            agg0 = next((op for op in logical_ops
                         if op[0] in ("aggregate", "aggregateByKey")), None)
            # scalar additive aggregate: schema-determined, identical on every
            # rank (same plan, same source) — safe to branch on collectively
            scalar_add = (sp.agg_expr is not None and sp.agg_key_idx is None
                          and not sp.agg_unique and agg0 is not None
                          and len(sp.gpu_output_types) == 1
                          and T.deopt(sp.gpu_output_types[0]) in (T.I64, T.F64))
            if scalar_add:
                # final combine: all_reduce of the local partial — RCCL over
                # xGMI when the backend is nccl (device tensor), gloo/CPU
                # otherwise; same code path either way so the gloo world-2
                # test covers it (LocalBackend.cc:1180-1207 thread-combine
                # analog). Replayed rows are data-dependent per rank, so agree
                # on the path with one flag reduce first; any replay anywhere
                # falls back to the object gather (host agg_fn fold).
                import torch
                is_int = T.deopt(sp.gpu_output_types[0]) == T.I64
                dev = (torch.device("cuda", torch.cuda.current_device())
                       if dist.get_backend() == "nccl" else
                       torch.device("cpu"))
                flag = torch.tensor([1 if replayed else 0], device=dev)
                dist.all_reduce(flag)
                if flag.item() == 0:
                    local = sum(r[0] for _, r in all_rows)
                    t = torch.tensor(
                        [local],
                        dtype=torch.int64 if is_int else torch.float64,
                        device=dev)
                    dist.all_reduce(t)
                    _, _, agg_fn, initial = agg0
                    out.rows = [t.item() + initial]
                    return out
            parts = _gather_objects(dist, (all_rows, replayed,
                                           out.exception_counts))
            all_rows, replayed, out.exception_counts = [], {}, {}
            for pr, pp, pe in parts:
                all_rows.extend(pr)
                replayed.update(pp)
                for nm, c in pe.items():
                    out.exception_counts[nm] = \
                        out.exception_counts.get(nm, 0) + c

    # ---- merge across chunks (global row indices; ResolveTask.cc:878 order) ----
    if sink_kind == "mem":
        all_rows.sort(key=lambda t: t[0])
        rows = [r for _, r in all_rows]
        if sp.agg_expr is not None and sp.agg_unique:
            # unique(): per-chunk tables emit (key, count); merge = key union
            # across chunks, plus replayed rows (createFinalHashmap analog)
            keys = dict.fromkeys(row[0] for row in rows)
            for i in sorted(replayed):
                for v in replayed[i]:
                    keys[v if not isinstance(v, tuple) else v[0]] = None
            out.rows = list(keys)
            return out
        agg = next((op for op in logical_ops
                    if op[0] in ("aggregate", "aggregateByKey")), None)
        if sp.agg_expr is not None:
            from .engine import _agg_row
            if sp.agg_key_idx is not None:
                _, combine_fn, agg_fn, initial, key_cols = agg[:5]
                table = {}
                for row in rows:  # per-chunk partials: sum per key, + initial once
                    table[row[0]] = table.get(row[0], initial) + row[1]
                ki = sp.output_columns.index(key_cols[0])
                for i in sorted(replayed):
                    for v in replayed[i]:
                        rt = v if isinstance(v, tuple) else (v,)
                        k = rt[ki]
                        table[k] = agg_fn(table.get(k, initial),
                                          _agg_row(v, sp.output_columns))
                out.rows = [(k, val) for k, val in table.items()]
            else:
                _, combine_fn, agg_fn, initial = agg
                acc = initial + sum(r[0] for r in rows)  # per-chunk partials
                for i in sorted(replayed):
                    for v in replayed[i]:
                        acc = agg_fn(acc, _agg_row(v, sp.output_columns))
                out.rows = [acc]
            return out
        merged = {}
        for i, row in all_rows:
            merged.setdefault(i, []).append(row[0] if len(row) == 1 else row)
        for i, lst in replayed.items():
            merged[i] = list(lst)
        from .engine import finalize_merged
        out.rows = finalize_merged(
            [v for i in sorted(merged) for v in merged[i]],
            logical_ops, sp.output_columns)
        if keep_exceptions:
            out.row_keys = [i for i in sorted(merged) for _ in merged[i]]
            if len(out.row_keys) != len(out.rows):
                out.row_keys = None  # trailing agg consumed row identity
    else:
        header_line = _format_csv_row(sp.output_columns or
                                      ["column%d" % i
                                       for i in range(len(sp.output_types))])
        segs = []  # (chunk_key, bytes) — key orders chunks across ranks
        for text, idxs, offs, row_lo, row_hi in text_parts:
            ci = row_lo >> _CHUNK_SHIFT
            if replayed:
                segs.append((ci, _merge_csv_segments(text, idxs, offs,
                                                     replayed, row_lo,
                                                     row_hi)))
            else:
                segs.append((ci, text))
        if dist and world > 1:
            # job-level exception counts are the union over ranks
            parts_e = _gather_objects(dist, dict(out.exception_counts))
            out.exception_counts = {}
            for pe in parts_e:
                for nm, c in pe.items():
                    out.exception_counts[nm] = \
                        out.exception_counts.get(nm, 0) + c
            path = sink[1]
            if path.endswith(".csv"):
                # single output file: gather segments to rank 0, write in
                # chunk order (executeInOrder analog across ranks)
                parts = _gather_objects(dist, segs)
                if rank == 0:
                    allsegs = sorted(s for p in parts for s in p)
                    _write_csv_output(path, header_line +
                                      b"".join(b for _, b in allsegs))
                dist.barrier()
            else:
                # directory sink: one part file per rank (the reference's
                # one-part-per-task layout), each with the header
                os.makedirs(path, exist_ok=True)
                with open(os.path.join(path, "part%d.csv" % rank), "wb") as f:
                    f.write(header_line + b"".join(b for _, b in segs))
                dist.barrier()
        else:
            _write_csv_output(sink[1],
                              [header_line] + [b for _, b in segs])
        out.rows = []
    return out


def _run_csv_fallback(out, data, col_types, null_values, logical_ops, names,
                      sink, why, delim=",", out_cols=None,
                      keep_exceptions=False):
    """Whole-stage interpreter fallback (non-compilable UDF) — the reference's
    fallback mode. Still semantically exact; slow by design. The trailing
    aggregate/aggregateByKey/unique fold over the PIPELINE's output columns
    (post-rename/withColumn names), not the source names."""
    out.mode = "fallback"
    out.fallback_reason = why
    dist = _dist()
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist else (0, 1)
    rows_out = {}
    all_lines = split_rows(data)
    # rank-sharded like the GPU path (contiguous blocks ~ reference ranges)
    blk = (len(all_lines) + world - 1) // world if world > 1 else len(all_lines)
    lo, hi = rank * blk, min((rank + 1) * blk, len(all_lines))
    for i in range(lo, hi):
        r = replay_csv_row(all_lines[i], col_types, null_values, logical_ops,
                           names, delim)
        if r[0] == "row":
            rows_out[i] = [r[1]]
        elif r[0] == "exc":
            if keep_exceptions:
                out.pending.append((i, all_lines[i]))
                continue
            nm = type(r[1]).__name__
            out.exception_counts[nm] = out.exception_counts.get(nm, 0) + 1
        elif r[0] == "rows":  # 1:N join expansion
            rows_out[i] = r[1]
            for e in r[2]:
                nm = type(e).__name__
                out.exception_counts[nm] = out.exception_counts.get(nm, 0) + 1
    if dist and world > 1:
        parts = _gather_objects(dist, (rows_out, out.exception_counts))
        rows_out, out.exception_counts = {}, {}
        for pr, pe in parts:
            rows_out.update(pr)
            for nm, c in pe.items():
                out.exception_counts[nm] = out.exception_counts.get(nm, 0) + c
    from .engine import finalize_merged, output_columns_of, _unwrap_row
    if out_cols is None:
        out_cols = output_columns_of(names, logical_ops)
    merged = [v if not isinstance(v, tuple) else _unwrap_row(v)
              for i in sorted(rows_out) for v in rows_out[i]]
    out.rows = finalize_merged(merged, logical_ops, out_cols)
    if keep_exceptions:
        out.row_keys = [i for i in sorted(rows_out) for _ in rows_out[i]]
        if len(out.row_keys) != len(out.rows):
            out.row_keys = None

        def _fb_replayer(payload, ops, _ct=col_types, _nv=null_values,
                         _nm=names, _dl=delim):
            return replay_csv_row(payload, _ct, _nv, ops, _nm, _dl)
        out.pending_replayer = _fb_replayer
    if sink is not None and sink[0] == "csv":
        header_line = _format_csv_row(out_cols or
                                      ["column%d" % i for i in
                                       range(max((len(_as_tup(v))
                                                  for v in out.rows), default=1))])
        body = b"".join(_format_csv_row(list(_as_tup(v))) for v in out.rows)
        if rank == 0:
            _write_csv_output(sink[1], header_line + body)
        if dist and world > 1:
            dist.barrier()
        out.rows = []
    return out


def _as_tup(v):
    return v if isinstance(v, tuple) else (v,)


def _format_cell(v) -> bytes:
    if v is None:
        s = ""
    elif isinstance(v, bool):
        s = "True" if v else "False"
    elif isinstance(v, float):
        s = "%f" % v  # the reference formats csv doubles with "%f"
                      # (PipelineBuilder.cc:1413)
    else:
        s = str(v)
    if any(c in s for c in ',"\n\r'):
        s = '"' + s.replace('"', '""') + '"'
    return s.encode("utf-8")


def _format_csv_row(vals) -> bytes:
    return b",".join(_format_cell(v) for v in vals) + b"\n"


def _merge_csv_segments(text: bytes, idxs, offs, replayed, row_lo,
                        row_hi) -> bytes:
    """Ordered merge of one chunk's GPU CSV text with host-resolved rows (the
    tocsv analog of executeInOrder). `replayed` keys are global input row
    indices; the chunk owns [row_lo, row_hi)."""
    n = len(idxs)
    rep = sorted((k, v) for k, v in replayed.items() if row_lo <= k < row_hi)
    segs = []
    gi = ri = 0
    while gi < n or ri < len(rep):
        if ri >= len(rep) or (gi < n and idxs[gi] < rep[ri][0]):
            start = gi
            bound = rep[ri][0] if ri < len(rep) else None
            while gi < n and (bound is None or idxs[gi] < bound):
                gi += 1
            segs.append(text[offs[start]:offs[gi]])
        else:
            for v in rep[ri][1]:
                row = v if isinstance(v, tuple) else (v,)
                segs.append(_format_csv_row(list(row)))
            ri += 1
    return b"".join(segs)


def _write_csv_output(path: str, content):
    """content: bytes or an iterable of byte segments (streamed write — no
    whole-output host buffer)."""
    if path.endswith(".csv"):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        target = path
    else:
        os.makedirs(path, exist_ok=True)
        target = os.path.join(path, "part0.csv")
    with open(target, "wb") as f:
        if isinstance(content, (bytes, bytearray)):
            f.write(content)
        else:
            f.writelines(content)

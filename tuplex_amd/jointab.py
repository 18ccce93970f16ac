"""Device join tables: the build side of a unique-key hash join in HBM.

plan.build_stage decides per join op whether its build side is embedded in
the generated source or lives in a tpx_jtable (op.join_dev, the schema the
generated probe was written for). This module packs the build rows into
columnar numpy buffers in the tpx_stage_execute_col slot layout, has the
library upload them and build the slot table (csrc/tpx_join.hip.h), keeps
the handle for as long as the build rows live, and binds it to a stage's
tpx_jt[] entry immediately before every run — stage handles are shared
between pipelines with the same source, so a binding never outlives a run.
"""
import ctypes

import numpy as np

TPX_E_TABLE_ALLOC = 2


class JoinTableAlloc(RuntimeError):
    """The table's device memory could not be had (hipMalloc failed or
    TPX_TABLE_MAX_BYTES): the stage takes the interpreter path."""


class BuildRows(list):
    """Materialised build rows of a join (DataSet.join). A list that can
    carry the device tables built from it, so that later chunks, streaming
    ranges and repeated actions of every DataSet derived from the join reuse
    them; they are freed with the rows."""
    __slots__ = ("_jtables",)

    def __init__(self, *a):
        super().__init__(*a)
        self._jtables = {}

    def __reduce__(self):   # the parallel resolver pickles ops: rows only
        return (list, (list(self),))


_DUMMY = np.zeros(8, dtype=np.uint8)   # a present, empty slot needs a pointer


def pack_columns(rrows, n_cols, rki, schema):
    """3 numpy arrays (or None) per build column, tpx_stage_execute_col
    layout: [values | int64 offsets (n+1)], [string bytes], [uint8 null mask].
    Vectorised: no per-cell python beyond C-level map/encode/join."""
    n = len(rrows)
    kinds = {j: (k, hn) for j, k, hn in schema["cols"]}
    kinds[rki] = ("str" if schema["key_str"] else "i64", False)
    columns = list(zip(*rrows)) if n else [()] * n_cols
    slots = []
    for j in range(n_cols):
        kind, has_null = kinds[j]
        col = columns[j]
        mask = None
        if has_null:
            obj = np.empty(n, dtype=object)
            obj[:] = col
            mask = np.equal(obj, None).astype(np.uint8)
            obj[mask != 0] = "" if kind == "str" else 0
            col = obj.tolist()
        if kind == "str":
            enc = list(map(str.encode, col))
            offs = np.zeros(n + 1, dtype=np.int64)
            if n:
                np.cumsum(np.fromiter(map(len, enc), dtype=np.int64, count=n),
                          out=offs[1:])
            data = np.frombuffer(b"".join(enc), dtype=np.uint8)
            slots += [offs, data, mask]
        elif kind == "f64":
            slots += [np.array(col, dtype=np.float64), None, mask]
        elif kind == "bool":
            slots += [np.array(col, dtype=np.bool_).view(np.uint8), None, mask]
        else:
            # raises OverflowError for an int outside int64
            slots += [np.array(col, dtype=np.int64), None, mask]
    return slots


class JoinTable:
    """One tpx_jtable, freed with this object."""

    def __init__(self, glib, handle):
        self._glib = glib
        self.handle = handle
        self.rows = int(glib.lib.tpx_jtable_rows(handle))
        self.bytes = int(glib.lib.tpx_jtable_bytes(handle))
        self.build_ms = float(glib.lib.tpx_jtable_build_ms(handle))

    @classmethod
    def build(cls, glib, stage, slots, n_rows, key_col, key_is_str):
        n = len(slots)
        slots = [np.ascontiguousarray(a) if a is not None else None
                 for a in slots]
        ptrs = (ctypes.c_void_p * n)(*[
            ctypes.c_void_p((a.ctypes.data if a.nbytes else
                             _DUMMY.ctypes.data) if a is not None else 0)
            for a in slots])
        nbytes = (ctypes.c_int64 * n)(*[a.nbytes if a is not None else 0
                                        for a in slots])
        h = ctypes.c_void_p()
        rc = glib.lib.tpx_jtable_build(stage, ptrs, nbytes, n // 3, n_rows,
                                       key_col, 1 if key_is_str else 0,
                                       ctypes.byref(h))
        if rc == TPX_E_TABLE_ALLOC:
            raise JoinTableAlloc("join table allocation failed: " + glib.err())
        if rc != 0 or not h.value:
            raise RuntimeError("tpx_jtable_build: " + glib.err())
        return cls(glib, h.value)

    def bind(self, stage, index):
        if self._glib.lib.tpx_stage_bind_jtable(stage, index,
                                                self.handle) != 0:
            raise RuntimeError("tpx_stage_bind_jtable: " + self._glib.err())

    def free(self):
        if self.handle:
            self._glib.lib.tpx_jtable_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def stage_tables(glib, stage, sp, device=0):
    """The JoinTable of every device join of sp on `device`, built once per
    (join op, device): kept on the build rows where DataSet.join made them
    (BuildRows), else on the op for this plan's life. Raises JoinTableAlloc."""
    tabs = []
    for op in getattr(sp, "device_joins", None) or []:
        rrows, rcols, _lki, rki, _how = op.join
        jd = op.join_dev
        store = getattr(rrows, "_jtables", None)
        if store is None:
            store = op.__dict__.setdefault("_jtables", {})
        key = (device, rki, jd["key_str"], tuple(jd["cols"]))
        tab = store.get(key)
        if tab is None:
            try:
                slots = pack_columns(rrows, len(rcols), rki, jd)
            except OverflowError:
                raise JoinTableAlloc("join table allocation failed: a build "
                                     "value is outside int64")
            tab = JoinTable.build(glib, stage, slots, len(rrows), rki,
                                  jd["key_str"])
            store[key] = tab
        tabs.append((jd["index"], tab))
    return tabs


def bind_tables(stage, tabs):
    for index, tab in tabs:
        tab.bind(stage, index)


def add_metrics(metrics, sp, tabs):
    """metrics["join_table"] and, for device tables, their bytes and the
    build kernels' HIP-event time."""
    if tabs:
        metrics["join_table"] = "device"
        metrics["join_table_bytes"] = sum(t.bytes for _, t in tabs)
        metrics["join_build_ms"] = sum(t.build_ms for _, t in tabs)
    elif any(op.kind == "join" for op in sp.ops):
        metrics["join_table"] = "embedded"

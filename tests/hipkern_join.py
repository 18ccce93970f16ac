"""Direct launches of the device join table kernels (csrc/tpx_join.hip.h), on
top of tests/hipkern.py: its buffers, canaries and launch are reused as they
are; only the module differs — the runtime header plus the join header plus
two tiny test-side probe kernels, compiled with hipkern's hipRTC options and
loaded once per process. The functions are registered in hipkern's function
table, so hipkern.launch runs them like any fixed kernel (synchronise, raise
on a HIP error, check the canary behind every buffer)."""
import ctypes

import numpy as np

from tests import hipkern
from tuplex_amd import codegen

KERNELS = ["tpx_join_build_i64", "tpx_join_build_str",
           "tj_probe_i64", "tj_probe_str"]

PROBE_SRC = r"""
extern "C" __global__ void tj_probe_i64(
        const long long* __restrict__ keys, long long m, void* slots,
        unsigned long long mask, long long n_rows, int* __restrict__ out) {
    TpxJoinTab t;
    t.slots = slots; t.mask = mask; t.n_rows = n_rows;
    t.n_cols = 1; t.key_col = 0;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = tpx_join_probe_i64(t, keys[i]);
}

extern "C" __global__ void tj_probe_str(
        const long long* __restrict__ qoffs, const char* __restrict__ qbytes,
        long long m, void* slots, unsigned long long mask, long long n_rows,
        const long long* koffs, const char* kbytes, int* __restrict__ out) {
    TpxJoinTab t;
    t.slots = slots; t.mask = mask; t.n_rows = n_rows;
    t.n_cols = 1; t.key_col = 0;
    t.cols[0] = koffs; t.cols[1] = kbytes; t.cols[2] = 0;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m)
        out[i] = tpx_join_probe_str(
            t, tstr{qbytes + qoffs[i], qoffs[i + 1] - qoffs[i]});
}
"""

_loaded = None


def source():
    return (codegen.runtime_header() + "\n" + codegen.join_header() + "\n"
            + PROBE_SRC)


def compile_code():
    """hipRTC-compile source() for gfx950. Needs no GPU."""
    rtc = hipkern._libs()[1]
    prog = ctypes.c_void_p()
    rc = rtc.hiprtcCreateProgram(ctypes.byref(prog), source().encode(),
                                 b"tpx_join_test.hip", 0, None, None)
    if rc != 0:
        raise hipkern.HipError("hiprtcCreateProgram: %d" % rc)
    opts = (ctypes.c_char_p * len(hipkern.HIPRTC_OPTS))(*hipkern.HIPRTC_OPTS)
    rc = rtc.hiprtcCompileProgram(prog, len(hipkern.HIPRTC_OPTS), opts)
    if rc != 0:
        n = ctypes.c_size_t(0)
        rtc.hiprtcGetProgramLogSize(prog, ctypes.byref(n))
        log = ctypes.create_string_buffer(max(n.value, 1))
        if n.value > 1:
            rtc.hiprtcGetProgramLog(prog, log)
        rtc.hiprtcDestroyProgram(ctypes.byref(prog))
        raise hipkern.HipError("hipRTC compile failed:\n"
                               + log.value.decode("utf-8", "replace")[:4000])
    n = ctypes.c_size_t(0)
    rtc.hiprtcGetCodeSize(prog, ctypes.byref(n))
    code = ctypes.create_string_buffer(n.value)
    rtc.hiprtcGetCode(prog, code)
    rtc.hiprtcDestroyProgram(ctypes.byref(prog))
    return code.raw


def _ensure():
    global _loaded
    fns = hipkern._module()
    if _loaded is None:
        hip = hipkern._libs()[0]
        code = compile_code()
        keep = ctypes.create_string_buffer(code, len(code))
        mod = ctypes.c_void_p()
        hipkern._check(hip.hipModuleLoadData(ctypes.byref(mod), keep),
                       "hipModuleLoadData")
        for name in KERNELS:
            f = ctypes.c_void_p()
            hipkern._check(hip.hipModuleGetFunction(ctypes.byref(f), mod,
                                                    name.encode()),
                           "hipModuleGetFunction(%s)" % name)
            fns[name] = f
        _loaded = (mod, keep)
    return fns


def _pack_strs(strs):
    enc = [s.encode("utf-8") for s in strs]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        offs[1:] = np.cumsum([len(b) for b in enc])
    return offs, b"".join(enc)


class BuiltTable:
    """A slot table built by one launch of the build kernel alone."""

    def __init__(self, keys, tsize, is_str, one_block=False):
        _ensure()
        self.n, self.tsize, self.is_str = len(keys), tsize, is_str
        n = self.n
        grid = 1 if one_block else max(1, min((n + 255) // 256, 8192))
        if is_str:
            offs, data = _pack_strs(keys)
            self.koffs, self.kbytes = hipkern.upload(offs), \
                hipkern.upload(data)
            self.slots = hipkern.alloc(tsize * 8, fill=0xFF)
            hipkern.launch("tpx_join_build_str", grid, 256,
                           [self.koffs, self.kbytes, hipkern.i64(n),
                            self.slots, hipkern.u64(tsize - 1)])
        else:
            self.keys = hipkern.upload(np.array(keys, dtype=np.int64))
            self.slots = hipkern.alloc(tsize * 16, fill=0xFF)
            hipkern.launch("tpx_join_build_i64", grid, 256,
                           [self.keys, hipkern.i64(n), self.slots,
                            hipkern.u64(tsize - 1)])

    def slot_rows(self):
        """Per slot the build row (-1 = empty), and for i64 tables the key,
        for str tables the upper 32 hash bits."""
        if self.is_str:
            w = hipkern.download(self.slots, np.uint64)
            rows = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32) \
                .view(np.int32)
            return rows.tolist(), (w >> np.uint64(32)).tolist()
        raw = hipkern.download(self.slots, np.int64).reshape(-1, 2)
        rows = (raw[:, 1] & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        return rows.tolist(), raw[:, 0].tolist()

    def probe(self, queries):
        """Build row (or -1) of every query key, by the probe functions."""
        m = len(queries)
        out = hipkern.alloc(m * 4)
        grid = max(1, (m + 255) // 256)
        if self.is_str:
            qo, qb = _pack_strs(queries)
            hipkern.launch("tj_probe_str", grid, 256,
                           [hipkern.upload(qo), hipkern.upload(qb),
                            hipkern.i64(m), self.slots,
                            hipkern.u64(self.tsize - 1), hipkern.i64(self.n),
                            self.koffs, self.kbytes, out])
        else:
            hipkern.launch("tj_probe_i64", grid, 256,
                           [hipkern.upload(np.array(queries, dtype=np.int64)),
                            hipkern.i64(m), self.slots,
                            hipkern.u64(self.tsize - 1), hipkern.i64(self.n),
                            out])
        return hipkern.download(out, np.int32).tolist()

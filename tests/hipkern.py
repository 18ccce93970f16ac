"""Direct launches of the fixed kernels of tpx_rt.hip.h, for kernel-level tests.

A small ctypes harness over the HIP runtime and hipRTC that libtpx_gpu.so
itself resolves (one HIP runtime per process; torch is never imported here).
The runtime header is compiled as it stands, with exactly the options of
compile_hiprtc in csrc/tpx_abi.cpp, once per process.

Every device buffer is followed by a 64-byte canary zone, and output buffers
are filled with a poison byte before a launch; launch() synchronises, raises
on any HIP error and then checks the canary of every buffer it was given, so
a kernel that writes past its output fails an assertion.
"""
import ctypes
import os

import numpy as np

from tuplex_amd import codegen

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), "tuplex_amd", "libtpx_gpu.so")

# compile_hiprtc's options (csrc/tpx_abi.cpp), verbatim
HIPRTC_OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17",
               b"-ffp-contract=off"]

KERNELS = [
    "tpx_csv_chunk_stats", "tpx_csv_select_counts", "tpx_csv_emit_rows",
    "tpx_scan_block", "tpx_scan_add", "tpx_pair_total",
    "tpx_reduce_f64", "tpx_reduce_f64_final",
    "tpx_reduce_i64", "tpx_reduce_i64_final",
    "tpx_hashagg_f64", "tpx_hashagg_i64", "tpx_hashagg_emit",
    "tpx_hashagg_str_f64", "tpx_hashagg_str_i64", "tpx_hashagg_str_emit",
]

POISON = 0xA5          # byte written over every output buffer before a launch
CANARY = 0xC7          # byte of the 64-byte zone after every buffer
CANARY_BYTES = 64
POISON_I64 = int(np.frombuffer(bytes([POISON]) * 8, dtype=np.int64)[0])

_H2D, _D2H = 1, 2

_libs_cache = None
_code_cache = None
_module_cache = None


class HipError(RuntimeError):
    pass


def source():
    """The source the harness compiles: the device runtime header alone."""
    return codegen.runtime_header()


def _loaded_path(stem):
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.rstrip("\n").split(" ")[-1]
            if os.path.basename(path).startswith(stem + ".so"):
                return path
    raise HipError("%s is not mapped by libtpx_gpu.so" % stem)


def _libs():
    """(hip, hiprtc): the very libraries libtpx_gpu.so pulled in."""
    global _libs_cache
    if _libs_cache is None:
        if not os.path.exists(LIB):
            raise HipError("libtpx_gpu.so not built")
        ctypes.CDLL(LIB)
        hip = ctypes.CDLL(_loaded_path("libamdhip64"))
        rtc = ctypes.CDLL(_loaded_path("libhiprtc"))
        hip.hipGetErrorString.restype = ctypes.c_char_p
        hip.hipGetErrorString.argtypes = [ctypes.c_int]
        hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p),
                                  ctypes.c_size_t]
        hip.hipFree.argtypes = [ctypes.c_void_p]
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_size_t, ctypes.c_int]
        hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                  ctypes.c_size_t]
        hip.hipModuleLoadData.argtypes = [ctypes.POINTER(ctypes.c_void_p),
                                          ctypes.c_void_p]
        hip.hipModuleGetFunction.argtypes = [ctypes.POINTER(ctypes.c_void_p),
                                             ctypes.c_void_p, ctypes.c_char_p]
        hip.hipModuleLaunchKernel.argtypes = (
            [ctypes.c_void_p] + [ctypes.c_uint] * 7 +
            [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
             ctypes.c_void_p])
        rtc.hiprtcGetErrorString.restype = ctypes.c_char_p
        rtc.hiprtcGetErrorString.argtypes = [ctypes.c_int]
        rtc.hiprtcCreateProgram.argtypes = [
            ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_char_p,
            ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        rtc.hiprtcCompileProgram.argtypes = [
            ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)]
        rtc.hiprtcGetProgramLogSize.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
        rtc.hiprtcGetProgramLog.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        rtc.hiprtcGetCodeSize.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
        rtc.hiprtcGetCode.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        rtc.hiprtcDestroyProgram.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        _libs_cache = (hip, rtc)
    return _libs_cache


def _check(rc, what):
    if rc != 0:
        hip = _libs()[0]
        msg = hip.hipGetErrorString(rc)
        raise HipError("%s: %s (%d)" % (what, (msg or b"?").decode(), rc))


def compile_code():
    """hipRTC-compile source() for gfx950 -> code object bytes. Needs no GPU."""
    global _code_cache
    if _code_cache is not None:
        return _code_cache
    rtc = _libs()[1]
    prog = ctypes.c_void_p()
    rc = rtc.hiprtcCreateProgram(ctypes.byref(prog), source().encode(),
                                 b"tpx_stage.hip", 0, None, None)
    if rc != 0:
        raise HipError("hiprtcCreateProgram: %s"
                       % rtc.hiprtcGetErrorString(rc).decode())
    opts = (ctypes.c_char_p * len(HIPRTC_OPTS))(*HIPRTC_OPTS)
    rc = rtc.hiprtcCompileProgram(prog, len(HIPRTC_OPTS), opts)
    if rc != 0:
        n = ctypes.c_size_t(0)
        rtc.hiprtcGetProgramLogSize(prog, ctypes.byref(n))
        log = ctypes.create_string_buffer(max(n.value, 1))
        if n.value > 1:
            rtc.hiprtcGetProgramLog(prog, log)
        rtc.hiprtcDestroyProgram(ctypes.byref(prog))
        raise HipError("hipRTC compile failed:\n"
                       + log.value.decode("utf-8", "replace")[:4000])
    n = ctypes.c_size_t(0)
    rtc.hiprtcGetCodeSize(prog, ctypes.byref(n))
    code = ctypes.create_string_buffer(n.value)
    rtc.hiprtcGetCode(prog, code)
    rtc.hiprtcDestroyProgram(ctypes.byref(prog))
    _code_cache = code.raw
    return _code_cache


def _module():
    """{kernel name: function handle}; compiled and loaded once per process."""
    global _module_cache
    if _module_cache is None:
        hip = _libs()[0]
        code = compile_code()
        _check(hip.hipSetDevice(0), "hipSetDevice")
        mod = ctypes.c_void_p()
        keep = ctypes.create_string_buffer(code, len(code))
        _check(hip.hipModuleLoadData(ctypes.byref(mod), keep),
               "hipModuleLoadData")
        fns = {}
        for name in KERNELS:
            f = ctypes.c_void_p()
            _check(hip.hipModuleGetFunction(ctypes.byref(f), mod,
                                            name.encode()),
                   "hipModuleGetFunction(%s)" % name)
            fns[name] = f
        _module_cache = (mod, keep, fns)
    return _module_cache[2]


class Buf:
    """A device buffer of `nbytes` bytes with a canary zone right after it."""

    def __init__(self, nbytes):
        hip = _libs()[0]
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        _check(hip.hipMalloc(ctypes.byref(p), self.nbytes + CANARY_BYTES),
               "hipMalloc")
        self.ptr = p.value
        _check(hip.hipMemset(self.ptr + self.nbytes, CANARY, CANARY_BYTES),
               "hipMemset")

    def fill(self, byte):
        if self.nbytes:
            _check(_libs()[0].hipMemset(self.ptr, byte, self.nbytes),
                   "hipMemset")
        return self

    def check_canary(self):
        z = np.empty(CANARY_BYTES, dtype=np.uint8)
        _check(_libs()[0].hipMemcpy(z.ctypes.data, self.ptr + self.nbytes,
                                    CANARY_BYTES, _D2H), "hipMemcpy")
        bad = np.nonzero(z != CANARY)[0]
        assert bad.size == 0, (
            "write past the end of a %d-byte buffer: canary bytes %s changed"
            % (self.nbytes, bad[:8].tolist()))

    def free(self):
        if self.ptr:
            _libs()[0].hipFree(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def alloc(nbytes, fill=POISON):
    """An output buffer, poisoned (or filled with `fill`; None leaves it)."""
    _module()
    b = Buf(nbytes)
    if fill is not None:
        b.fill(fill)
    return b


def upload(arr):
    """A device buffer holding the bytes of a numpy array / bytes object."""
    _module()
    if isinstance(arr, (bytes, bytearray)):
        arr = np.frombuffer(bytes(arr), dtype=np.uint8)
    arr = np.ascontiguousarray(arr)
    b = Buf(arr.nbytes)
    if arr.nbytes:
        _check(_libs()[0].hipMemcpy(b.ptr, arr.ctypes.data, arr.nbytes, _H2D),
               "hipMemcpy")
    return b


def download(buf, dtype=np.uint8, count=None, offset=0):
    """Copy `count` items of `dtype` from byte `offset` of buf to the host."""
    dt = np.dtype(dtype)
    if count is None:
        count = (buf.nbytes - offset) // dt.itemsize
    out = np.empty(count, dtype=dt)
    assert offset + out.nbytes <= buf.nbytes
    if out.nbytes:
        _check(_libs()[0].hipMemcpy(out.ctypes.data, buf.ptr + offset,
                                    out.nbytes, _D2H), "hipMemcpy")
    return out


def i64(v):
    return ctypes.c_longlong(int(v))


def u64(v):
    return ctypes.c_ulonglong(int(v))


def i32(v):
    return ctypes.c_int(int(v))


def launch(name, grid, block, args):
    """Launch a fixed kernel with Buf / i64() / u64() / i32() arguments,
    wait for it, raise on any HIP error, then check every buffer's canary."""
    hip = _libs()[0]
    fn = _module()[name]
    assert grid >= 1 and block >= 1
    holders = []
    for a in args:
        if isinstance(a, Buf):
            holders.append(ctypes.c_void_p(a.ptr))
        elif isinstance(a, (ctypes.c_longlong, ctypes.c_ulonglong,
                            ctypes.c_int)):
            holders.append(a)
        else:
            raise TypeError("launch argument %r: use a Buf, i64(), u64() or "
                            "i32()" % (a,))
    argv = (ctypes.c_void_p * len(holders))(
        *[ctypes.cast(ctypes.byref(h), ctypes.c_void_p) for h in holders])
    _check(hip.hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, 0, None,
                                     argv, None),
           "launch %s" % name)
    _check(hip.hipDeviceSynchronize(), "%s (synchronise)" % name)
    for a in args:
        if isinstance(a, Buf):
            a.check_canary()

"""The two test-only libraries of tests/device/devtest.hip through ctypes: "dpp" (libfsehip_devtest.so, the headers as the product compiles
them) and "shfl" (libfsehip_devtest_shfl.so, -DFSEHIP_NO_DPP_SCANS).  FSEHIP_DEVTEST_LIB / FSEHIP_DEVTEST_LIB_SHFL put another build of the same
file in their place (a mutated header: the check that the tests bite)."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("dpp", "shfl")
_FILES = {"dpp": "libfsehip_devtest.so", "shfl": "libfsehip_devtest_shfl.so"}
_ENV = {"dpp": "FSEHIP_DEVTEST_LIB", "shfl": "FSEHIP_DEVTEST_LIB_SHFL"}
HIP_SUCCESS, HIP_INVALID_VALUE = 0, 1
_LIBS = {}


def path(kind):
    return os.environ.get(_ENV[kind]) or os.path.join(ROOT, "tests", "device", _FILES[kind])


def load(kind):
    if kind not in _LIBS:
        p = path(kind)
        if not os.path.exists(p) and not os.environ.get(_ENV[kind]):
            import finitestateentropy_amd
            finitestateentropy_amd.build_library()
        lib = C.CDLL(p)
        lib.FSEHIP_devtest_run.restype = C.c_int
        lib.FSEHIP_devtest_run.argtypes = [C.c_char_p, C.c_longlong, C.c_longlong, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p]
        lib.FSEHIP_devtest_list.restype = C.c_size_t
        lib.FSEHIP_devtest_list.argtypes = [C.c_char_p, C.c_size_t]
        lib.FSEHIP_devtest_dpp.restype = C.c_int
        for f in (lib.FSEHIP_devtest_pl_size, lib.FSEHIP_devtest_pl_start):
            f.restype, f.argtypes = C.c_uint64, [C.c_uint64, C.c_uint, C.c_uint]
        lib.FSEHIP_devtest_tile.restype = C.c_uint64
        _LIBS[kind] = lib
    return _LIBS[kind]


def listing(lib):
    """{(name, a, b): (dwords in, dwords out)} as the library lists it"""
    need = lib.FSEHIP_devtest_list(None, 0)
    buf = C.create_string_buffer(need + 1)
    assert lib.FSEHIP_devtest_list(buf, need + 1) == need
    out = {}
    for line in buf.value.decode().splitlines():
        name, a, b, i, o = line.split()
        assert (name, int(a), int(b)) not in out, line
        out[(name, int(a), int(b))] = (int(i), int(o))
    return out


def run(lib, name, a, b, records, out_words, threads, payload=None):
    """records: (n, IN) dwords, one row per work item; payload: bytes behind them.  n is padded up to whole blocks with copies of the last row
    (every wave is full); returns the first n rows of the (n, OUT) dwords the kernel stored.  Needs a GPU."""
    import torch
    records = np.ascontiguousarray(records, dtype=np.uint32)
    n = records.shape[0]
    pad = -n % threads
    if pad:
        records = np.concatenate([records, np.repeat(records[-1:], pad, axis=0)])
    raw = records.view(np.uint8).reshape(-1)
    if payload is not None:
        raw = np.concatenate([raw, np.ascontiguousarray(payload).view(np.uint8).reshape(-1)])
    d_in = torch.from_numpy(raw.copy()).cuda()
    d_out = torch.full(((n + pad) * out_words * 4,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = lib.FSEHIP_devtest_run(name.encode(), a, b, n + pad, d_in.data_ptr(), d_in.numel(), d_out.data_ptr(), d_out.numel(), threads, None)
    assert rc == HIP_SUCCESS, (name, a, b, rc)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32).reshape(n + pad, out_words)[:n]


def u64_words(x):
    """(n,) or (n, k) 64-bit values -> (n, 2 k) dwords, low first"""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    return x.view(np.uint32).reshape(x.shape[0], -1)


def words_u64(w):
    w = np.ascontiguousarray(w, dtype=np.uint32)
    return w.view(np.uint64).reshape(w.shape[0], -1)

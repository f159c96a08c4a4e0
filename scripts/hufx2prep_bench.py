"""development aid: time the double-symbol table builder (FSEHIP_HUF_readDTableX2_batch) per 100k Proba14 headers at maxTableLog 12 and 11, beside
FSEHIP_HUF_readDTableX1_batch in the same run (device events around 5 calls each, after a warm-up; alternating rounds), with the write traffic
of the tables -- 4 << maxTableLog bytes each -- so that the distance from the store bound can be read off"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from finitestateentropy_amd.api import FseHip
hip = FseHip()
N, REPS, ROUNDS = 100000, 5, 3
src = hip.probagen_batch(14, N, 32768, 1)
blocks, sizes = hip.huf_compress_batch(src, table_log=11)
del src
ws = torch.empty(int(hip.lib.FSEHIP_HUF_readDTableX2_batch_workspaceSize(N)), dtype=torch.uint8, device="cuda")
res = torch.zeros(N, dtype=torch.int64, device="cuda")
tables = torch.zeros((N, 1 + (1 << 12)), dtype=torch.int32, device="cuda")
x1 = torch.zeros((N, 1 + (1 << 11)), dtype=torch.int32, device="cuda")


def run_x2(L):
    hip.huf_read_dtable_x2_batch(blocks, sizes, L, dtables=tables[:, :1 + (1 << L)], results=res, workspace=ws)


def run_x1():
    import ctypes as C
    from finitestateentropy_amd.api import _ptr, _sizes_arg, _stream, SZ
    ps, uni, keep = _sizes_arg(sizes, blocks)
    rc = hip.lib.FSEHIP_HUF_readDTableX1_batch(_ptr(x1), SZ(x1.stride(0)), C.c_uint(11), _ptr(res), _ptr(blocks), SZ(blocks.stride(0)), ps, uni, SZ(N), _ptr(ws),
                                               SZ(ws.numel()), _stream())
    assert rc == 0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


cases = (("X2 maxTableLog 12", lambda: run_x2(12), 4 << 12), ("X2 maxTableLog 11", lambda: run_x2(11), 4 << 11), ("X1 maxTableLog 11", run_x1, 2 << 12))
for name, fn, _ in cases:
    fn()
torch.cuda.synchronize()
assert bool((res > 0).all())
best = {}
for r in range(ROUNDS):
    for name, fn, nbytes in cases:
        ms = timed(fn)
        best.setdefault(name, []).append(ms)
for name, fn, nbytes in cases:
    t = sorted(best[name])
    print("%s: %s ms per %d headers (median %.3f) -- %.2f GB of tables, %.0f GB/s written" % (name, " ".join("%.3f" % v for v in t), N, t[len(t) // 2], N * nbytes / 1e9,
                                                                                          N * nbytes / 1e6 / t[len(t) // 2]))

"""development aid: the strided predicted-plane calls (FSEHIP_planes_split_pred_stride_dbatch / _merge_pred_stride_dbatch,
FSEHIP_tensor_compress_pred_stride_dbatch / _decompress_pred_stride_dbatch) next to the stride-1 predicted calls, at 1024 tensors of 1 MiB, the
workload and the protocol of predbench.py, on two interleaved sources generated on the device: int16 stereo (two different random walks) and
float32 xyz (a random-walk trajectory, each axis around an offset of its own):
  (a) a device-to-device copy of the same bytes (dst.copy_(src))
  (b) per element size 1, 2, 4, 8 over the same bytes: the stride-1 predicted split and merge -- the yardstick -- then the strided split and
      merge for the strides 2, 3, 4 and 8; "vs_stride1" = the strided kernel's GB/s over the stride-1 kernel's of this run (both move 2 n
      bytes), "bar" = whether that reaches 0.5 (held for elements of 2 and 4 bytes at the strides 2, 3, 4, the others are
      reported).  --parent-lib PATH: the stride-1 kernels are those of the library at PATH (the parent commit's build) loaded beside this
      tree's
  (c) per source (stereo: 2-byte elements, stride 2; xyz: 4-byte elements, stride 3) and codec: tensor_compress / tensor_decompress, the
      stride-1 composites, then the strided composites, with the frames' share of the bytes
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  GB/s =
content bytes / time.  Prints one JSON line per figure.
Usage: stridebench.py [--tensors 1024] [--tensor-kib 1024] [--block-size-id 5] [--parent-lib PATH]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd import _lib
from finitestateentropy_amd.api import FseHip

MIN_MS = 300.0
BAR = 0.5
STRIDES = (2, 3, 4, 8)
ap = argparse.ArgumentParser()
ap.add_argument("--tensors", type=int, default=1024); ap.add_argument("--tensor-kib", type=int, default=1024); ap.add_argument("--block-size-id", type=int, default=5)
ap.add_argument("--parent-lib", default=None)
args = ap.parse_args()
hip = FseHip()
one_hip, one_of = hip, "this tree"
if args.parent_lib:                                            # a second binding over the other library: its stride-1 kernels are the yardstick
    _lib._LIB = C.CDLL(os.path.abspath(args.parent_lib))
    one_hip, one_of = FseHip(), "the parent's library"
    _lib._LIB = hip.lib
    assert not hasattr(one_hip.lib, "FSEHIP_planes_split_pred_stride_dbatch"), "--parent-lib names a library that has the strided calls"
BSID = args.block_size_id


def timed(fn):
    """ms per call: one warm-up, then repeated until MIN_MS have passed between the two events"""
    fn(); torch.cuda.synchronize()
    reps, total = 0, 0.0
    while total < MIN_MS:
        n = 1 if reps == 0 else max(1, int(reps * (MIN_MS - total) / total) + 1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record(); b.synchronize()
        total += a.elapsed_time(b); reps += n
    return total / reps


def ws(fn, *a):
    fn.restype = C.c_size_t
    return torch.empty(max(int(fn(*a)), 1), dtype=torch.uint8, device="cuda")


def zigzag_back(raw, E, S):
    """zigzag(t[j] - t[j - S]) in runs of 1024 elements, with torch, of the elements of the bytes `raw` (a multiple of 1024 elements)"""
    dt = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[E]
    t = raw.view(dt).reshape(-1, 1024)
    p = torch.zeros_like(t)
    p[:, S:] = t[:, :-S]
    d = t - p
    return ((d << 1) ^ (d >> (8 * E - 1))).reshape(-1).view(torch.uint8)


n, tbytes = args.tensors, args.tensor_kib << 10
total = n * tbytes
gen = torch.Generator(device="cuda").manual_seed(1)
soff = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * tbytes)).cuda()


def walks(count, channels, lo, hi, dtype):
    """`count` elements: `channels` interleaved random walks with steps in [lo, hi), in slices to bound the int64 scratch"""
    out = torch.empty(count, dtype=dtype, device="cuda")
    rows, at, last = 1 << 24, 0, torch.zeros((1, channels), dtype=torch.int64, device="cuda")
    while at < count:
        m = min(rows * channels, count - at)
        w = torch.cumsum(torch.randint(lo, hi, (-(-m // channels), channels), generator=gen, device="cuda", dtype=torch.int64), 0) + last
        last = w[-1:].clone()
        out[at:at + m] = w.reshape(-1)[:m].to(dtype)
        at += m
    return out


def sources():
    yield "int16 stereo", 2, 2, walks(total // 2, 2, -40, 41, torch.int16).view(torch.uint8)
    steps = walks(total // 4, 3, -1000, 1001, torch.int32)      # the walk in units of 1e-7 around 100.0 / -37.0 / 5.5
    base = torch.tensor([100.0, -37.0, 5.5], device="cuda", dtype=torch.float64).repeat(-(-(total // 4) // 3))[:total // 4]
    yield "float32 xyz", 4, 3, (base + steps.to(torch.float64) * 1e-7).to(torch.float32).view(torch.uint8)


first = True
for source, srcE, srcS, src in sources():
    def report(what, codec, ms, **more):
        gbps = total / ms / 1e6
        print(json.dumps(dict(shape="%d x %d KiB" % (n, args.tensor_kib), source=source, what=what, codec=codec, GBps=round(gbps, 2), ms=round(ms, 3), **more)), flush=True)
        return gbps

    def against(what, gbps, one, E, S):
        more = dict(vs_stride1=round(gbps / one, 3), stride1_of=one_of)
        if E in (2, 4) and S in (2, 3, 4):
            more["bar"] = "%s %.1f of the stride-1 %s" % ("meets" if gbps >= BAR * one else "MISSES", BAR, what)
        return more
    other, planes = torch.empty_like(src), torch.empty_like(src)
    report("device copy (dst.copy_(src))", "-", timed(lambda: other.copy_(src)))
    for E in (1, 2, 4, 8) if first else ():                    # (b): the kernels' rates do not depend on the bytes; once
        poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); tres = torch.zeros(n, dtype=torch.int64, device="cuda")
        psz = torch.full((n * E,), tbytes // E, dtype=torch.int64, device="cuda"); mres = torch.zeros_like(tres)
        split = report("planes split predicted (stride 1), E = %d" % E, "-",
                       timed(lambda: one_hip.planes_split_pred_dbatch(src, soff, E, planes=planes, plane_offsets=poff, results=tres)), of=one_of)
        other.zero_()
        merge = report("planes merge predicted (stride 1), E = %d" % E, "-",
                       timed(lambda: one_hip.planes_merge_pred_dbatch(planes, poff, psz, soff, E, dst=other, results=mres)), of=one_of)
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        for S in STRIDES:
            ms = timed(lambda: hip.planes_split_pred_stride_dbatch(src, soff, E, S, planes=planes, plane_offsets=poff, results=tres))
            report("planes split strided, E = %d, S = %d" % (E, S), "-", ms, **against("split", total / ms / 1e6, split, E, S))
            z = zigzag_back(src[:tbytes], E, S)
            assert bool((tres == tbytes).all()) and all(torch.equal(planes[p * (tbytes // E):(p + 1) * (tbytes // E)], z[p::E]) for p in range(E))
            other.zero_()
            ms = timed(lambda: hip.planes_merge_pred_stride_dbatch(planes, poff, psz, soff, E, S, dst=other, results=mres))
            report("planes merge strided, E = %d, S = %d" % (E, S), "-", ms, **against("merge", total / ms / 1e6, merge, E, S))
            assert bool((mres == tbytes).all()) and torch.equal(other, src)
    first = False
    E, S = srcE, srcS
    poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); tres = torch.zeros(n, dtype=torch.int64, device="cuda"); mres = torch.zeros_like(tres)
    blocks = hip.planes_block_bound(total, n, E, BSID)
    L = hip.lib
    for codec, name in ((0, "fse"), (1, "huf")):
        kws = ws(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(codec))
        dws = ws(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks))
        frames = torch.empty(hip.frame_packed_bound(total, n * E, blocks, 0), dtype=torch.uint8, device="cuda")
        foff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); fres = torch.zeros(n * E, dtype=torch.int64, device="cuda")
        poff2 = torch.zeros_like(poff); pres = torch.zeros_like(fres)
        wkw = dict(dst=frames, max_total_blocks=blocks, frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, workspace=kws)
        rkw = dict(dst=other, max_total_blocks=blocks, planes=planes, plane_offsets=poff2, plane_results=pres, workspace=dws, results=mres)
        rows = (("tensor_compress", "tensor_decompress", lambda: hip.tensor_compress_dbatch(src, soff, E, BSID, codec, **wkw),
                 lambda: hip.tensor_decompress_dbatch(frames, foff, soff, E, **rkw)),
                ("tensor_compress_pred (stride 1)", "tensor_decompress_pred (stride 1)",
                 lambda: hip.tensor_compress_pred_dbatch(src, soff, E, codec=codec, block_size_id=BSID, **wkw), lambda: hip.tensor_decompress_pred_dbatch(frames, foff, soff, E, **rkw)),
                ("tensor_compress_pred_stride, S = %d" % S, "tensor_decompress_pred_stride, S = %d" % S,
                 lambda: hip.tensor_compress_pred_stride_dbatch(src, soff, E, S, codec=codec, block_size_id=BSID, **wkw),
                 lambda: hip.tensor_decompress_pred_stride_dbatch(frames, foff, soff, E, S, **rkw)))
        plain_bytes = None
        for wname, rname, write, read in rows:
            w_ms = timed(write)
            nbytes = int(foff[n * E].item())
            assert bool((fres > 0).all()) and bool((tres == tbytes).all())
            plain_bytes = plain_bytes or nbytes
            report(wname, name, w_ms, E=E, frame_bytes=nbytes, ratio=round(nbytes / total, 4), over_plain=round(nbytes / plain_bytes, 4))
            other.zero_()
            report(rname, name, timed(read), E=E)
            assert bool((mres == tbytes).all()) and torch.equal(other, src)
        del kws, dws, frames
    del src, other, planes
    torch.cuda.empty_cache()

"""development aid: the byte-plane calls (FSEHIP_planes_split_dbatch / _merge_dbatch, FSEHIP_tensor_compress_dbatch / _decompress_dbatch) on bf16
data -- N(0, 0.02) cut to bf16, generated on the device -- at 1024 tensors of 1 MiB:
  (a) a device-to-device copy of the same bytes (dst.copy_(src)): the yardstick of the two data kernels
  (b) the split alone, the merge alone
  (c) per codec: the plain packed writer and reader over the raw bytes, one frame per tensor (FSEHIP_frame_compress_packed_dbatch /
      _decompress_packed_dbatch) next to the two composite calls, one frame per plane, on the same bytes; "extra_ms" = composite minus plain
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  GB/s =
content bytes / time.  Prints one JSON line per figure.  Usage: planebench.py [--tensors 1024] [--tensor-kib 1024] [--block-size-id 5]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import FseHip

MIN_MS = 300.0
ap = argparse.ArgumentParser()
ap.add_argument("--tensors", type=int, default=1024); ap.add_argument("--tensor-kib", type=int, default=1024); ap.add_argument("--block-size-id", type=int, default=5)
args = ap.parse_args()
hip = FseHip()
BSID, E = args.block_size_id, 2


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


def report(what, codec, nbytes, ms, **more):
    print(json.dumps(dict(shape="%d x %d KiB bf16" % (args.tensors, args.tensor_kib), what=what, codec=codec, GBps=round(nbytes / ms / 1e6, 2), ms=round(ms, 3), **more)),
          flush=True)


def ws(fn, *a):
    fn.restype = C.c_size_t
    return torch.empty(max(int(fn(*a)), 1), dtype=torch.uint8, device="cuda")


n, tbytes = args.tensors, args.tensor_kib << 10
total = n * tbytes
gen = torch.Generator(device="cuda").manual_seed(1)
src = (torch.randn(total // 2, generator=gen, device="cuda") * 0.02).to(torch.bfloat16).view(torch.uint8)
soff = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * tbytes)).cuda()
other = torch.empty_like(src)
report("device copy (dst.copy_(src))", "-", total, timed(lambda: other.copy_(src)))

planes = torch.empty_like(src)
poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); tres = torch.zeros(n, dtype=torch.int64, device="cuda")
report("planes split", "-", total, timed(lambda: hip.planes_split_dbatch(src, soff, E, planes=planes, plane_offsets=poff, results=tres)))
assert bool((tres == tbytes).all()) and torch.equal(planes[:tbytes // 2], src[:tbytes:2]) and torch.equal(planes[tbytes // 2:tbytes], src[1:tbytes:2])
psz = torch.full((n * E,), tbytes // E, dtype=torch.int64, device="cuda"); mres = torch.zeros_like(tres)
report("planes merge", "-", total, timed(lambda: hip.planes_merge_dbatch(planes, poff, psz, soff, E, dst=other, results=mres)))
assert bool((mres == tbytes).all()) and torch.equal(other, src)

blocks_raw = n * hip.frame_block_count(tbytes, BSID)
blocks_pl = hip.planes_block_bound(total, n, E, BSID)
L = hip.lib
for codec, name in ((0, "fse"), (1, "huf")):
    # the plain packed writer and reader: one frame per tensor over the raw bytes
    kws = ws(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize, C.c_size_t(n), C.c_size_t(blocks_raw), C.c_uint(BSID), C.c_int(codec))
    frames = torch.empty(hip.frame_packed_bound(total, n * E, blocks_pl, 0), dtype=torch.uint8, device="cuda")
    foff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); fres = torch.zeros(n * E, dtype=torch.int64, device="cuda")
    plain_w = timed(lambda: hip.frame_compress_packed_dbatch(src, soff, BSID, codec, dst=frames, max_total_blocks=blocks_raw, dst_offsets=foff[:n + 1], workspace=kws,
                                                             results=fres[:n]))
    raw_bytes = int(foff[n].item())
    report("packed writer, raw bytes (1 frame per tensor)", name, total, plain_w, frame_bytes=raw_bytes, ratio=round(raw_bytes / total, 4))
    dws = ws(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, C.c_size_t(n), C.c_size_t(blocks_raw))
    boff = torch.zeros(n + 1, dtype=torch.int64, device="cuda"); bres = torch.zeros(n, dtype=torch.int64, device="cuda")
    other.zero_()
    plain_r = timed(lambda: hip.frame_decompress_packed_dbatch(frames, foff[:n + 1], dst=other, capacity=total, max_total_blocks=blocks_raw, dst_offsets=boff, workspace=dws,
                                                               results=bres))
    report("packed reader, raw bytes", name, total, plain_r)
    assert bool((bres == tbytes).all()) and torch.equal(other, src)
    del kws, dws
    # the composites: one frame per plane
    kws = ws(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks_pl), C.c_uint(BSID), C.c_int(codec))
    comp_w = timed(lambda: hip.tensor_compress_dbatch(src, soff, E, BSID, codec, dst=frames, max_total_blocks=blocks_pl, frame_offsets=foff, frame_results=fres,
                                                      tensor_results=tres, planes=planes, plane_offsets=poff, workspace=kws))
    pl_bytes = int(foff[n * E].item())
    assert bool((fres > 0).all()) and bool((tres == tbytes).all())
    report("tensor_compress (split + 1 frame per plane)", name, total, comp_w, frame_bytes=pl_bytes, ratio=round(pl_bytes / total, 4),
           planes_over_raw=round(pl_bytes / raw_bytes, 4), extra_ms=round(comp_w - plain_w, 3))
    dws = ws(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks_pl))
    poff2 = torch.zeros_like(poff); pres = torch.zeros_like(fres)
    other.zero_()
    comp_r = timed(lambda: hip.tensor_decompress_dbatch(frames, foff, soff, E, dst=other, max_total_blocks=blocks_pl, planes=planes, plane_offsets=poff2, plane_results=pres,
                                                        workspace=dws, results=mres))
    report("tensor_decompress (1 frame per plane + merge)", name, total, comp_r, extra_ms=round(comp_r - plain_r, 3))
    assert bool((mres == tbytes).all()) and torch.equal(other, src)
    del kws, dws, frames
    torch.cuda.empty_cache()

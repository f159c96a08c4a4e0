"""development aid: the predicted-plane calls (FSEHIP_planes_split_pred_dbatch / _merge_pred_dbatch, FSEHIP_tensor_compress_pred_dbatch /
_decompress_pred_dbatch) next to the plain byte-plane calls, at 1024 tensors of 1 MiB, the workload of planebench.py and deltabench.py, on
two sources generated on the device: sorted uint32 indices (density 1/16: a running sum of gaps of 1 .. 31) and an fp32 field (a sine over 40
radians per tensor plus 1e-4 noise):
  (a) a device-to-device copy of the same bytes (dst.copy_(src))
  (b) per element size 1, 2, 4, 8 over the same bytes: the plain split and merge, then the predicted split and merge; "vs_plain" = the
      predicted kernel's GB/s over the plain kernel's of this run (both move 2 n bytes), "bar" = whether that reaches 0.5 (DESIGN.md 4.4h;
      held for elements of 2 and 4 bytes, the others are reported).  The plain split of 1-byte elements moves nothing: its row is the copy.
      --parent-lib PATH: the plain kernels are those of the library at PATH (the parent commit's build) loaded beside this tree's
  (c) per codec, 4-byte elements: tensor_compress / tensor_decompress, then the predicted composites, with the frames' share of the bytes
      ("pred_over_plain": the predicted frames' bytes over the plain frames')
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  GB/s =
content bytes / time.  Prints one JSON line per figure.
Usage: predbench.py [--tensors 1024] [--tensor-kib 1024] [--block-size-id 5] [--parent-lib PATH]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd import _lib
from finitestateentropy_amd.api import FseHip

MIN_MS = 300.0
BAR = 0.5
ap = argparse.ArgumentParser()
ap.add_argument("--tensors", type=int, default=1024); ap.add_argument("--tensor-kib", type=int, default=1024); ap.add_argument("--block-size-id", type=int, default=5)
ap.add_argument("--parent-lib", default=None)
args = ap.parse_args()
hip = FseHip()
plain_hip, plain_of = hip, "this tree"
if args.parent_lib:                                            # a second binding over the other library: its plain kernels are the yardstick
    _lib._LIB = C.CDLL(os.path.abspath(args.parent_lib))
    plain_hip, plain_of = FseHip(), "the parent's library"
    _lib._LIB = hip.lib
    assert not hasattr(plain_hip.lib, "FSEHIP_planes_split_pred_dbatch"), "--parent-lib names a library that has the predicted calls"
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


def zigzag_prev(raw, E):
    """zigzag(t[j] - t[j - 1]) in runs of 1024 elements, with torch, of the elements of the bytes `raw` (a multiple of 1024 elements)"""
    dt = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[E]
    t = raw.view(dt).reshape(-1, 1024)
    p = torch.zeros_like(t)
    p[:, 1:] = t[:, :-1]
    d = t - p
    return ((d << 1) ^ (d >> (8 * E - 1))).reshape(-1).view(torch.uint8)


n, tbytes = args.tensors, args.tensor_kib << 10
total = n * tbytes
gen = torch.Generator(device="cuda").manual_seed(1)
soff = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * tbytes)).cuda()


def sources():
    gaps = torch.randint(1, 32, (total // 4,), generator=gen, device="cuda", dtype=torch.int64)
    yield "sorted uint32", (torch.cumsum(gaps, 0) & 0xFFFFFFFF).to(torch.int32).view(torch.uint8)
    del gaps
    x = torch.linspace(0, 40.0 * n, total // 4, device="cuda", dtype=torch.float64)
    yield "fp32 sine field", (torch.sin(x) + 1e-4 * torch.randn(total // 4, generator=gen, device="cuda", dtype=torch.float64)).to(torch.float32).view(torch.uint8)


for source, src in sources():
    def report(what, codec, ms, **more):
        gbps = total / ms / 1e6
        print(json.dumps(dict(shape="%d x %d KiB" % (n, args.tensor_kib), source=source, what=what, codec=codec, GBps=round(gbps, 2), ms=round(ms, 3), **more)), flush=True)
        return gbps

    def against(what, gbps, plain, E):
        more = dict(vs_plain=round(gbps / plain, 3), plain_of=plain_of)
        if E in (2, 4):
            more["bar"] = "%s %.1f of the plain %s" % ("meets" if gbps >= BAR * plain else "MISSES", BAR, what)
        return more
    other, planes = torch.empty_like(src), torch.empty_like(src)
    copy = report("device copy (dst.copy_(src))", "-", timed(lambda: other.copy_(src)))
    for E in (1, 2, 4, 8):
        poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); tres = torch.zeros(n, dtype=torch.int64, device="cuda")
        psz = torch.full((n * E,), tbytes // E, dtype=torch.int64, device="cuda"); mres = torch.zeros_like(tres)
        split = copy
        if E > 1:
            split = report("planes split, E = %d" % E, "-", timed(lambda: plain_hip.planes_split_dbatch(src, soff, E, planes=planes, plane_offsets=poff, results=tres)))
        else:
            plain_hip.planes_split_dbatch(src, soff, E, planes=planes, plane_offsets=poff, results=tres)
            planes.copy_(src)
        merge = report("planes merge, E = %d" % E, "-", timed(lambda: plain_hip.planes_merge_dbatch(planes, poff, psz, soff, E, dst=other, results=mres)))
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        ms = timed(lambda: hip.planes_split_pred_dbatch(src, soff, E, planes=planes, plane_offsets=poff, results=tres))
        report("planes split predicted, E = %d" % E, "-", ms, **against("split" if E > 1 else "copy", total / ms / 1e6, split, E))
        z = zigzag_prev(src[:tbytes], E)
        assert bool((tres == tbytes).all()) and all(torch.equal(planes[p * (tbytes // E):(p + 1) * (tbytes // E)], z[p::E]) for p in range(E))
        other.zero_()
        ms = timed(lambda: hip.planes_merge_pred_dbatch(planes, poff, psz, soff, E, dst=other, results=mres))
        report("planes merge predicted, E = %d" % E, "-", ms, **against("merge", total / ms / 1e6, merge, E))
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
    E = 4
    poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); tres = torch.zeros(n, dtype=torch.int64, device="cuda"); mres = torch.zeros_like(tres)
    blocks = hip.planes_block_bound(total, n, E, BSID)
    L = hip.lib
    for codec, name in ((0, "fse"), (1, "huf")):
        kws = ws(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(codec))
        dws = ws(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks))
        frames = torch.empty(hip.frame_packed_bound(total, n * E, blocks, 0), dtype=torch.uint8, device="cuda")
        foff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); fres = torch.zeros(n * E, dtype=torch.int64, device="cuda")
        poff2 = torch.zeros_like(poff); pres = torch.zeros_like(fres)
        comp_w = timed(lambda: hip.tensor_compress_dbatch(src, soff, E, BSID, codec, dst=frames, max_total_blocks=blocks, frame_offsets=foff, frame_results=fres,
                                                          tensor_results=tres, planes=planes, plane_offsets=poff, workspace=kws))
        plain_bytes = int(foff[n * E].item())
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        report("tensor_compress", name, comp_w, frame_bytes=plain_bytes, ratio=round(plain_bytes / total, 4))
        other.zero_()
        comp_r = timed(lambda: hip.tensor_decompress_dbatch(frames, foff, soff, E, dst=other, max_total_blocks=blocks, planes=planes, plane_offsets=poff2,
                                                            plane_results=pres, workspace=dws, results=mres))
        report("tensor_decompress", name, comp_r)
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        pred_w = timed(lambda: hip.tensor_compress_pred_dbatch(src, soff, E, codec=codec, block_size_id=BSID, dst=frames, max_total_blocks=blocks, frame_offsets=foff,
                                                               frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, workspace=kws))
        pred_bytes = int(foff[n * E].item())
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        report("tensor_compress_pred", name, pred_w, frame_bytes=pred_bytes, ratio=round(pred_bytes / total, 4), pred_over_plain=round(pred_bytes / plain_bytes, 4),
               vs_plain=round(comp_w / pred_w, 3))
        other.zero_()
        pred_r = timed(lambda: hip.tensor_decompress_pred_dbatch(frames, foff, soff, E, dst=other, max_total_blocks=blocks, planes=planes, plane_offsets=poff2,
                                                                 plane_results=pres, workspace=dws, results=mres))
        report("tensor_decompress_pred", name, pred_r, vs_plain=round(comp_r / pred_r, 3))
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        del kws, dws, frames
    del src, other, planes
    torch.cuda.empty_cache()

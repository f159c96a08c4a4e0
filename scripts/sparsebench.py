"""development aid: sparse planes (FSEHIP_sparse_pack_dbatch / _expand_dbatch, FSEHIP_tensor_compress_sparse_dbatch /
_decompress_sparse_dbatch) next to the dense delta calls, on the workload of deltabench.py -- a bf16 weight update generated on the device,
the base N(0, 0.02), the new tensors base + N(0, 2e-5) added in float32, both cut to bf16, 1024 tensors of 1 MiB:
  (a) the XOR split and the XOR merge into a destination of its own: the yardstick kernels, three streams of n bytes each
  (b) pack and expand over the planes the XOR split (and the SUB split) left, at `--permille`: "vs_split" / "vs_merge" = their GB/s over the
      XOR split's / merge's of this run, "bar" = whether that reaches 0.5; "content_share" = the contents' bytes over the planes'
  (c) per codec and per delta op: the dense composites (tensor_compress_delta / tensor_decompress_delta, separate destination) and the sparse
      ones from the same data in the same run, with the frames' share of the bytes: "sparse_over_dense" = the sparse frames' bytes over the
      dense frames', "vs_dense" = the dense call's time over the sparse call's (above 1: the sparse call is faster)
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  GB/s =
content bytes (the new tensors' bytes) / time.  Prints one JSON line per figure.
Usage: sparsebench.py [--tensors 1024] [--tensor-kib 1024] [--block-size-id 5] [--permille 500]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import FseHip

MIN_MS = 300.0
BAR = 0.5
ap = argparse.ArgumentParser()
ap.add_argument("--tensors", type=int, default=1024); ap.add_argument("--tensor-kib", type=int, default=1024); ap.add_argument("--block-size-id", type=int, default=5)
ap.add_argument("--permille", type=int, default=500)
args = ap.parse_args()
hip = FseHip()
BSID, E, PERMILLE = args.block_size_id, 2, args.permille


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
    gbps = nbytes / ms / 1e6
    print(json.dumps(dict(shape="%d x %d KiB bf16" % (args.tensors, args.tensor_kib), what=what, codec=codec, GBps=round(gbps, 2), ms=round(ms, 3), **more)), flush=True)
    return gbps


def ws(fn, *a, head=0):
    fn.restype = C.c_size_t
    return torch.empty(head + max(int(fn(*a)), 1), dtype=torch.uint8, device="cuda")


def bar(what, gbps, yard):
    return {"vs_" + what: round(gbps / yard, 3), "bar": "%s %.1f of the XOR %s" % ("meets" if gbps >= BAR * yard else "MISSES", BAR, what)}


n, tbytes = args.tensors, args.tensor_kib << 10
total = n * tbytes
gen = torch.Generator(device="cuda").manual_seed(1)
w = torch.randn(total // 2, generator=gen, device="cuda") * 0.02
base = w.to(torch.bfloat16).view(torch.uint8)
src = (w + torch.randn(total // 2, generator=gen, device="cuda") * 2e-5).to(torch.bfloat16).view(torch.uint8)
del w
soff = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * tbytes)).cuda()
other = torch.empty_like(src)
planes, contents, planes2 = torch.empty_like(src), torch.empty_like(src), torch.empty_like(src)
poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); tres = torch.zeros(n, dtype=torch.int64, device="cuda")
psz = torch.full((n * E,), tbytes // E, dtype=torch.int64, device="cuda"); mres = torch.zeros_like(tres)
coff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); ures = torch.zeros(n * E, dtype=torch.int64, device="cuda")
sws = torch.empty(hip.sparse_workspace_bound(total, n * E), dtype=torch.uint8, device="cuda")

# (a) and (b): the yardstick kernels, then pack and expand over the planes they left
for op, tag in ((0, "XOR"), (1, "SUB")):
    ms = timed(lambda: hip.planes_split_xor_dbatch(src, base, soff, E, planes=planes, plane_offsets=poff, results=tres, delta_op=op))
    g = report("planes split %s base" % tag, "-", total, ms)
    if not op:
        split = g
    ms = timed(lambda: hip.sparse_pack_dbatch(planes, poff, PERMILLE, contents=contents, content_offsets=coff, workspace=sws))
    cbytes = int(coff[n * E].item())
    sparse_units = int(((coff[1:] - coff[:-1]) < tbytes // E).sum().item())
    report("sparse pack of the %s planes" % tag, "-", total, ms, content_share=round(cbytes / total, 4), sparse_units="%d of %d" % (sparse_units, n * E),
           **bar("split", total / ms / 1e6, split))
    csz = coff[1:] - coff[:-1]
    ms = timed(lambda: hip.sparse_expand_dbatch(contents, coff, csz, poff, units=planes2, results=ures, workspace=sws))
    assert bool((ures == tbytes // E).all()) and torch.equal(planes2, planes)
    if not op:
        other.zero_()
        mms = timed(lambda: hip.planes_merge_xor_dbatch(planes, poff, psz, base, soff, E, dst=other, results=mres, delta_op=op))
        merge = report("planes merge XOR base, separate dst", "-", total, mms)
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
    report("sparse expand of the %s contents" % tag, "-", total, ms, **bar("merge", total / ms / 1e6, merge))

# (c) the composites, dense and sparse, from the same data
blocks = hip.planes_block_bound(total, n, E, BSID)
L = hip.lib
head = hip.sparse_workspace_bound(total, n * E)
for codec, name in ((0, "fse"), (1, "huf")):
    kws = ws(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(codec), head=head)
    dws = ws(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks), head=head)
    frames = torch.empty(hip.frame_packed_bound(total, n * E, blocks, 0), dtype=torch.uint8, device="cuda")
    foff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); fres = torch.zeros(n * E, dtype=torch.int64, device="cuda")
    poff2 = torch.zeros_like(poff); pres = torch.zeros_like(fres); cres = torch.zeros_like(fres)
    for op, tag in ((0, "XOR"), (1, "SUB")):
        dense_w = timed(lambda: hip.tensor_compress_delta_dbatch(src, base, soff, E, BSID, codec, dst=frames, max_total_blocks=blocks, frame_offsets=foff,
                                                                 frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, workspace=kws, delta_op=op))
        dense_bytes = int(foff[n * E].item())
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        report("tensor_compress_delta %s, dense" % tag, name, total, dense_w, frame_bytes=dense_bytes, ratio=round(dense_bytes / total, 4))
        other.zero_()
        dense_r = timed(lambda: hip.tensor_decompress_delta_dbatch(frames, foff, base, soff, E, dst=other, max_total_blocks=blocks, planes=planes, plane_offsets=poff2,
                                                                   plane_results=pres, workspace=dws, results=mres, delta_op=op))
        report("tensor_decompress_delta %s, dense, separate dst" % tag, name, total, dense_r)
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        sparse_w = timed(lambda: hip.tensor_compress_sparse_dbatch(src, soff, E, PERMILLE, base=base, codec=codec, block_size_id=BSID, dst=frames, max_total_blocks=blocks,
                                                                   frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff,
                                                                   contents=contents, content_offsets=coff, workspace=kws, delta_op=op))
        sparse_bytes = int(foff[n * E].item())
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        report("tensor_compress_sparse %s" % tag, name, total, sparse_w, frame_bytes=sparse_bytes, ratio=round(sparse_bytes / total, 4),
               sparse_over_dense=round(sparse_bytes / dense_bytes, 4), vs_dense=round(dense_w / sparse_w, 3))
        other.zero_()
        sparse_r = timed(lambda: hip.tensor_decompress_sparse_dbatch(frames, foff, soff, E, base=base, dst=other, max_total_blocks=blocks, contents=contents,
                                                                     content_offsets=coff, content_results=cres, planes=planes, plane_offsets=poff2, plane_results=pres,
                                                                     workspace=dws, results=mres, delta_op=op))
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        more = dict(vs_dense=round(dense_r / sparse_r, 3))
        if codec == 0:
            more["premise"] = "faster than the dense read" if sparse_r < dense_r else "NOT FASTER THAN THE DENSE READ"
        report("tensor_decompress_sparse %s, separate dst" % tag, name, total, sparse_r, **more)
    del kws, dws, frames
    torch.cuda.empty_cache()

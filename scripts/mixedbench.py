"""development aid: the packed frame writer with a codec per frame (FSEHIP_frame_compress_packed_mixed_dbatch, FSEHIP_tensor_compress_mixed_dbatch)
next to the calls it is built from, on the workload and with the protocol of deltabench.py -- a bf16 weight update generated on the device
(base N(0, 0.02), new = base + N(0, 2e-5) added in float32, both cut to bf16), 1024 tensors of 1 MiB, two byte planes each:
  (a) the routing's cost: GIVEN with all codecs FSE / all Huff0 against frame_compress_packed_dbatch with that codec, over the planes of the
      new tensors and over the planes of new XOR base
  (b) CHOOSE against the sum of the two plain writers over the same planes, its workspace next to theirs, and what it chose
  (c) the payoff: the delta written with the codecs CHOOSE picks at tolerance 50, with all FSE and with all Huff0 -- frame bytes, and
      tensor_decompress_delta_dbatch of each into a destination of its own and in place; likewise the plain tensors at tolerance 20 through
      tensor_decompress_dbatch
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  GB/s =
content bytes (the new tensors' bytes) / time.  Prints one JSON line per figure.
Usage: mixedbench.py [--tensors 1024] [--tensor-kib 1024] [--block-size-id 5]"""
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
    return ms


n, tbytes = args.tensors, args.tensor_kib << 10
total, nf = n * tbytes, n * E
gen = torch.Generator(device="cuda").manual_seed(1)
w = torch.randn(total // 2, generator=gen, device="cuda") * 0.02
base = w.to(torch.bfloat16).view(torch.uint8)
src = (w + torch.randn(total // 2, generator=gen, device="cuda") * 2e-5).to(torch.bfloat16).view(torch.uint8)
del w
soff = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * tbytes)).cuda()
blocks = hip.planes_block_bound(total, n, E, BSID)
L = hip.lib
L.FSEHIP_frame_compress_packed_dbatch_workspaceSize.restype = L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize.restype = C.c_size_t
P = [int(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize(C.c_size_t(nf), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(c))) for c in (0, 1)]
wgiven, wchoose = hip.frame_mixed_workspace_bound(nf, blocks, BSID, choose=False), hip.frame_mixed_workspace_bound(nf, blocks, BSID, choose=True)
print(json.dumps(dict(what="workspace bytes", frames=nf, blocks=blocks, packed_fse=P[0], packed_huf=P[1], mixed_given=wgiven, mixed_choose=wchoose,
                      choose_over_sum=round(wchoose / (P[0] + P[1]), 4))), flush=True)
wsp = torch.empty(wchoose, dtype=torch.uint8, device="cuda")             # one workspace serves every writer here: it is the largest
dws = torch.empty(int(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize(C.c_size_t(nf), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
fcap = hip.frame_packed_bound(total, nf, blocks, 0)
frames = torch.empty(fcap, dtype=torch.uint8, device="cuda"); ref = torch.empty(fcap, dtype=torch.uint8, device="cuda")
foff, roff = (torch.zeros(nf + 1, dtype=torch.int64, device="cuda") for _ in range(2))
fres, rres, pres = (torch.zeros(nf, dtype=torch.int64, device="cuda") for _ in range(3))
tres, mres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
planes, planes2, other = torch.empty_like(src), torch.empty_like(src), torch.empty_like(src)
poff, poff2 = (torch.zeros(nf + 1, dtype=torch.int64, device="cuda") for _ in range(2))
codecs = torch.zeros(nf, dtype=torch.uint8, device="cuda")
names = ("fse", "huf")

# ---- (a), (b): the writers alone, over planes that lie ready
for kind, tol in (("planes of the new tensors", 20), ("planes of new XOR base", 50)):
    if kind.endswith("base"):
        hip.planes_split_xor_dbatch(src, base, soff, E, planes=planes, plane_offsets=poff, results=tres)
    else:
        hip.planes_split_dbatch(src, soff, E, planes=planes, plane_offsets=poff, results=tres)
    plain_ms, plain_bytes = [], []
    for codec in (0, 1):
        ms = timed(lambda: hip.frame_compress_packed_dbatch(planes, poff, BSID, codec, dst=ref, max_total_blocks=blocks, dst_offsets=roff, workspace=wsp, results=rres))
        plain_ms.append(ms); plain_bytes.append(int(roff[nf].item()))
        report("frame_compress_packed_dbatch, " + kind, names[codec], total, ms, frame_bytes=plain_bytes[-1])
        codecs.fill_(codec)
        g = timed(lambda: hip.frame_compress_packed_mixed_dbatch(planes, poff, codecs, 0, BSID, dst=frames, max_total_blocks=blocks, dst_offsets=foff, workspace=wsp,
                                                                 results=fres))
        assert torch.equal(foff, roff) and torch.equal(fres, rres) and torch.equal(frames[:plain_bytes[-1]], ref[:plain_bytes[-1]])
        report("mixed writer GIVEN, all " + names[codec] + ", " + kind, names[codec], total, g, extra_ms=round(g - ms, 3), over_plain=round(g / ms, 3))
    out = torch.full((nf,), 7, dtype=torch.uint8, device="cuda")

    def choose():
        hip.lib.FSEHIP_frame_compress_packed_mixed_dbatch(C.c_void_p(frames.data_ptr()), C.c_uint64(fcap), C.c_void_p(foff.data_ptr()), C.c_void_p(fres.data_ptr()),
                                                          C.c_void_p(planes.data_ptr()), C.c_void_p(poff.data_ptr()), C.c_size_t(nf), C.c_size_t(blocks), C.c_uint(BSID),
                                                          C.c_void_p(out.data_ptr()), C.c_int(1), C.c_uint(tol), C.c_uint(0), C.c_void_p(wsp.data_ptr()),
                                                          C.c_size_t(wsp.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    c = timed(choose)
    assert bool((fres > 0).all()) and bool((out <= 1).all())
    picked = out.view(n, E).to(torch.int64).sum(0).tolist()
    report("mixed writer CHOOSE at tolerance %d, %s" % (tol, kind), "auto", total, c, frame_bytes=int(foff[nf].item()), huf_frames_per_plane=picked,
           sum_of_both_plain_writers_ms=round(sum(plain_ms), 3), over_sum=round(c / sum(plain_ms), 3), all_fse_bytes=plain_bytes[0], all_huf_bytes=plain_bytes[1])
    codecs.copy_(out)
    g = timed(lambda: hip.frame_compress_packed_mixed_dbatch(planes, poff, codecs, 0, BSID, dst=ref, max_total_blocks=blocks, dst_offsets=roff, workspace=wsp, results=rres))
    assert torch.equal(foff, roff) and torch.equal(fres, rres) and torch.equal(frames[:int(foff[nf])], ref[:int(foff[nf])])
    report("mixed writer GIVEN with the codecs CHOOSE gave back, " + kind, "auto", total, g)

# ---- (c): the payoff on the reading side
resident = torch.empty_like(src)
for delta, tol in ((True, 50), (False, 20)):
    b = base if delta else None
    label = "delta (new XOR base)" if delta else "new tensors"
    for way in ("auto", "fse", "huf"):
        given = None if way == "auto" else codecs.fill_(names.index(way))
        _, _, _, _, got = hip.tensor_compress_mixed_dbatch(src, soff, E, b, given, tol, BSID, dst=frames, max_total_blocks=blocks, frame_offsets=foff, frame_results=fres,
                                                           tensor_results=tres, planes=planes, plane_offsets=poff, workspace=wsp)
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        nbytes = int(foff[nf].item())
        more = dict(frame_bytes=nbytes, ratio=round(nbytes / total, 4), huf_frames_per_plane=got.view(n, E).to(torch.int64).sum(0).tolist())
        other.zero_()
        if delta:
            ms = timed(lambda: hip.tensor_decompress_delta_dbatch(frames, foff, base, soff, E, dst=other, max_total_blocks=blocks, planes=planes2, plane_offsets=poff2,
                                                                  plane_results=pres, workspace=dws, results=mres))
            report("tensor_decompress_delta, separate dst, %s written %s" % (label, way), way, total, ms, **more)
            assert bool((mres == tbytes).all()) and torch.equal(other, src)
            resident.copy_(base)
            hip.tensor_decompress_delta_dbatch(frames, foff, resident, soff, E, dst=resident, max_total_blocks=blocks, planes=planes2, plane_offsets=poff2,
                                               plane_results=pres, workspace=dws, results=mres)
            assert bool((mres == tbytes).all()) and torch.equal(resident, src)
            ms = timed(lambda: hip.tensor_decompress_delta_dbatch(frames, foff, resident, soff, E, dst=resident, max_total_blocks=blocks, planes=planes2,
                                                                  plane_offsets=poff2, plane_results=pres, workspace=dws, results=mres))
            report("tensor_decompress_delta, in place (dst == base), %s written %s" % (label, way), way, total, ms, **more)
        else:
            ms = timed(lambda: hip.tensor_decompress_dbatch(frames, foff, soff, E, dst=other, max_total_blocks=blocks, planes=planes2, plane_offsets=poff2,
                                                            plane_results=pres, workspace=dws, results=mres))
            report("tensor_decompress, %s written %s" % (label, way), way, total, ms, **more)
            assert bool((mres == tbytes).all()) and torch.equal(other, src)

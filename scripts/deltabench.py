"""development aid: the tensor-delta calls (FSEHIP_planes_split_xor_dbatch / _merge_xor_dbatch, FSEHIP_tensor_compress_delta_dbatch /
_decompress_delta_dbatch) next to the plain byte-plane calls, on a bf16 weight update generated on the device -- the base is N(0, 0.02), the
new tensors are base + N(0, 2e-5) added in float32, both cut to bf16 -- at 1024 tensors of 1 MiB, the workload of planebench.py:
  (a) a device-to-device copy of the same bytes (dst.copy_(src))
  (b) the plain split and merge, then the XOR split, the XOR merge into a destination of its own and the XOR merge in place (dst == base),
      then the same three with SUB (zigzag(new - base), delta_op 1); "vs_plain" = the delta kernel's GB/s over the plain kernel's of this
      run, "bar" = whether that reaches 0.6 (3 n bytes of traffic instead of 2 n, less a tenth for the third stream), "sub_vs_xor" = the SUB
      kernel's GB/s over the XOR kernel's
  (c) per codec: tensor_compress / tensor_decompress of the new tensors, then the delta composites against the base (separate destination and
      in place) with XOR and with SUB, with the frames' share of the bytes ("sub_over_xor": the SUB frames' bytes over the XOR frames')
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  GB/s =
content bytes (the new tensors' bytes) / time.  Prints one JSON line per figure.
Usage: deltabench.py [--tensors 1024] [--tensor-kib 1024] [--block-size-id 5]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import FseHip

MIN_MS = 300.0
BAR = 0.6
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
    gbps = nbytes / ms / 1e6
    print(json.dumps(dict(shape="%d x %d KiB bf16" % (args.tensors, args.tensor_kib), what=what, codec=codec, GBps=round(gbps, 2), ms=round(ms, 3), **more)), flush=True)
    return gbps


def ws(fn, *a):
    fn.restype = C.c_size_t
    return torch.empty(max(int(fn(*a)), 1), dtype=torch.uint8, device="cuda")


n, tbytes = args.tensors, args.tensor_kib << 10
total = n * tbytes
gen = torch.Generator(device="cuda").manual_seed(1)
w = torch.randn(total // 2, generator=gen, device="cuda") * 0.02
base = w.to(torch.bfloat16).view(torch.uint8)
src = (w + torch.randn(total // 2, generator=gen, device="cuda") * 2e-5).to(torch.bfloat16).view(torch.uint8)
del w
changed = int((src != base).sum().item())
soff = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * tbytes)).cuda()
other = torch.empty_like(src)
report("device copy (dst.copy_(src))", "-", total, timed(lambda: other.copy_(src)), bytes_that_differ_from_the_base=changed)

planes = torch.empty_like(src)
poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); tres = torch.zeros(n, dtype=torch.int64, device="cuda")
psz = torch.full((n * E,), tbytes // E, dtype=torch.int64, device="cuda"); mres = torch.zeros_like(tres)
split = report("planes split", "-", total, timed(lambda: hip.planes_split_dbatch(src, soff, E, planes=planes, plane_offsets=poff, results=tres)))
assert bool((tres == tbytes).all()) and torch.equal(planes[:tbytes // 2], src[:tbytes:2]) and torch.equal(planes[tbytes // 2:tbytes], src[1:tbytes:2])
merge = report("planes merge", "-", total, timed(lambda: hip.planes_merge_dbatch(planes, poff, psz, soff, E, dst=other, results=mres)))
assert bool((mres == tbytes).all()) and torch.equal(other, src)


def against(what, gbps, plain):
    return dict(vs_plain=round(gbps / plain, 3), bar="%s %.1f of the plain %s" % ("meets" if gbps >= BAR * plain else "MISSES", BAR, what))


def zigzag_sub(t, b):
    """zigzag(t - b) of the bf16 elements' bit patterns, with torch: what the SUB split's planes are the planes of"""
    d = t.view(torch.int16) - b.view(torch.int16)
    return ((d << 1) ^ (d >> 15)).view(torch.uint8)


# XOR, then SUB (zigzag(new - base) on the elements' bit patterns): the same data, the same buffers, the same run; "sub_vs_xor" = the SUB
# kernel's GB/s over the XOR kernel's
kernel_rate = {}
for op, tag in ((0, "XOR"), (1, "SUB")):
    def versus(what, row, gbps, plain):
        more = against(what, gbps, plain)
        if op:
            more["sub_vs_xor"] = round(gbps / kernel_rate[row], 3)
        else:
            kernel_rate[row] = gbps
        return more
    ms = timed(lambda: hip.planes_split_xor_dbatch(src, base, soff, E, planes=planes, plane_offsets=poff, results=tres, delta_op=op))
    report("planes split %s base" % tag, "-", total, ms, **versus("split", "split", total / ms / 1e6, split))
    x = zigzag_sub(src[:tbytes], base[:tbytes]) if op else src[:tbytes] ^ base[:tbytes]
    assert bool((tres == tbytes).all()) and torch.equal(planes[:tbytes // 2], x[::2]) and torch.equal(planes[tbytes // 2:tbytes], x[1::2])
    other.zero_()
    ms = timed(lambda: hip.planes_merge_xor_dbatch(planes, poff, psz, base, soff, E, dst=other, results=mres, delta_op=op))
    report("planes merge %s base, separate dst" % tag, "-", total, ms, **versus("merge", "merge", total / ms / 1e6, merge))
    assert bool((mres == tbytes).all()) and torch.equal(other, src)
    # in place: the buffer is the base before a call and the new tensors after it -- and the base again after the next one (XOR twice; with SUB
    # it moves on by the same difference each time), so every timed call does the same work; checked on one call over a fresh copy of the base
    resident = base.clone()
    hip.planes_merge_xor_dbatch(planes, poff, psz, resident, soff, E, dst=resident, results=mres, delta_op=op)
    assert bool((mres == tbytes).all()) and torch.equal(resident, src)
    ms = timed(lambda: hip.planes_merge_xor_dbatch(planes, poff, psz, resident, soff, E, dst=resident, results=mres, delta_op=op))
    report("planes merge %s base, in place (dst == base)" % tag, "-", total, ms, **versus("merge", "merge in place", total / ms / 1e6, merge))

blocks = hip.planes_block_bound(total, n, E, BSID)
L = hip.lib
for codec, name in ((0, "fse"), (1, "huf")):
    kws = ws(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(codec))
    dws = ws(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks))
    frames = torch.empty(hip.frame_packed_bound(total, n * E, blocks, 0), dtype=torch.uint8, device="cuda")
    foff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); fres = torch.zeros(n * E, dtype=torch.int64, device="cuda")
    poff2 = torch.zeros_like(poff); pres = torch.zeros_like(fres)
    # the plain composites over the new tensors
    comp_w = timed(lambda: hip.tensor_compress_dbatch(src, soff, E, BSID, codec, dst=frames, max_total_blocks=blocks, frame_offsets=foff, frame_results=fres,
                                                      tensor_results=tres, planes=planes, plane_offsets=poff, workspace=kws))
    plain_bytes = int(foff[n * E].item())
    assert bool((fres > 0).all()) and bool((tres == tbytes).all())
    report("tensor_compress of the new tensors", name, total, comp_w, frame_bytes=plain_bytes, ratio=round(plain_bytes / total, 4))
    other.zero_()
    comp_r = timed(lambda: hip.tensor_decompress_dbatch(frames, foff, soff, E, dst=other, max_total_blocks=blocks, planes=planes, plane_offsets=poff2, plane_results=pres,
                                                        workspace=dws, results=mres))
    report("tensor_decompress of the new tensors", name, total, comp_r)
    assert bool((mres == tbytes).all()) and torch.equal(other, src)
    # the delta composites against the base: XOR, then SUB; "sub_vs_xor" = the SUB call's GB/s over the XOR call's, "sub_over_xor" = its frame bytes
    # over the XOR frames'
    xor = {}
    for op, tag, form in ((0, "XOR", "new XOR base"), (1, "SUB", "zigzag(new - base)")):
        def versus(row, ms, **more):
            if op:
                more["sub_vs_xor"] = round(xor[row] / ms, 3)
            else:
                xor[row] = ms
            return more
        delta_w = timed(lambda: hip.tensor_compress_delta_dbatch(src, base, soff, E, BSID, codec, dst=frames, max_total_blocks=blocks, frame_offsets=foff,
                                                                 frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, workspace=kws, delta_op=op))
        delta_bytes = int(foff[n * E].item())
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        more = versus("compress", delta_w)
        if op:
            more["sub_over_xor"] = round(delta_bytes / xor["bytes"], 4)
        else:
            xor["bytes"] = delta_bytes
        report("tensor_compress_delta %s (%s)" % (tag, form), name, total, delta_w, frame_bytes=delta_bytes, ratio=round(delta_bytes / total, 4),
               delta_over_plain=round(delta_bytes / plain_bytes, 4), extra_ms=round(delta_w - comp_w, 3), **more)
        other.zero_()
        delta_r = timed(lambda: hip.tensor_decompress_delta_dbatch(frames, foff, base, soff, E, dst=other, max_total_blocks=blocks, planes=planes, plane_offsets=poff2,
                                                                   plane_results=pres, workspace=dws, results=mres, delta_op=op))
        report("tensor_decompress_delta %s, separate dst" % tag, name, total, delta_r, extra_ms=round(delta_r - comp_r, 3), **versus("decompress", delta_r))
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        resident.copy_(base)
        hip.tensor_decompress_delta_dbatch(frames, foff, resident, soff, E, dst=resident, max_total_blocks=blocks, planes=planes, plane_offsets=poff2, plane_results=pres,
                                           workspace=dws, results=mres, delta_op=op)
        assert bool((mres == tbytes).all()) and torch.equal(resident, src)
        delta_i = timed(lambda: hip.tensor_decompress_delta_dbatch(frames, foff, resident, soff, E, dst=resident, max_total_blocks=blocks, planes=planes,
                                                                   plane_offsets=poff2, plane_results=pres, workspace=dws, results=mres, delta_op=op))
        report("tensor_decompress_delta %s, in place (dst == base)" % tag, name, total, delta_i, extra_ms=round(delta_i - comp_r, 3), **versus("in place", delta_i))
    del kws, dws, frames
    torch.cuda.empty_cache()

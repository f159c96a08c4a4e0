"""development aid: windows of segmented tensors (FSEHIP_tensor_decompress_window_dbatch) next to the only way the library had to get those bytes,
the full FSEHIP_tensor_decompress_seg_dbatch on the same object in the same run -- 1 GiB of bf16 data, N(0, 0.02) generated on the device, cut
into
  (b) 8 tensors of 128 MiB      (c) one tensor of 1 GiB
with segment_log 18, per codec.  Windows: every whole element (the bar: within 3 % of the full call), and 1/8 of each tensor at its start, in
its middle (unaligned to a segment) and at its end (the bar: not slower than the full call).  Device events around the calls, repeated
until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  Every window's bytes are compared with the
source's.  One JSON line per figure: ms, the ratio to the full call and the ratio to 1/8 of the full call's time; the full call is timed a
second time behind the windows, to show what the order of the calls alone does.
Usage: windowbench.py [--total-mib 1024] [--block-size-id 5] [--segment-log 18]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import FseHip

MIN_MS = 200.0
ap = argparse.ArgumentParser()
ap.add_argument("--total-mib", type=int, default=1024); ap.add_argument("--block-size-id", type=int, default=5); ap.add_argument("--segment-log", type=int, default=18)
args = ap.parse_args()
hip = FseHip()
BSID, E, SEG_LOG = args.block_size_id, 2, args.segment_log


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


def i64(n):
    return torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")[:n]


def dev(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64).reshape(-1)).cuda()


total = args.total_mib << 20
gen = torch.Generator(device="cuda").manual_seed(1)
src = (torch.randn(total // 2, generator=gen, device="cuda") * 0.02).to(torch.bfloat16).view(torch.uint8)
planes, other = torch.empty_like(src), torch.empty_like(src)
L = hip.lib

for shape, n in (("b", 8), ("c", 1)):
    tbytes = total // n
    numel = tbytes // E
    name = "%d x %d MiB bf16" % (n, tbytes >> 20)
    soff_h = np.arange(n + 1, dtype=np.int64) * tbytes
    soff = torch.from_numpy(soff_h).cuda()
    blocks = hip.planes_block_bound(total, n, E, BSID)
    first = hip.planes_segment_first([tbytes] * n, E, SEG_LOG)
    nseg = int(first[-1])
    sf = dev(first)
    for codec, cname in ((0, "fse"), (1, "huf")):
        frames = torch.empty(hip.frame_packed_bound(total, nseg, blocks, 0), dtype=torch.uint8, device="cuda")
        foff, fres, so, tres, poff = i64(nseg + 1), i64(nseg), i64(nseg + 1), i64(n), i64(n * E + 1)
        hip.tensor_compress_seg_dbatch(src, soff, E, SEG_LOG, sf, n_segments=nseg, codec=codec, block_size_id=BSID, dst=frames, max_total_blocks=blocks, frame_offsets=foff,
                                       frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, seg_offsets=so)
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        # the yardstick: the full read, the parent's only way to those bytes
        dws = ws(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, C.c_size_t(nseg), C.c_size_t(blocks))
        so2, sres, poff2, psz, mres = i64(nseg + 1), i64(nseg), i64(n * E), i64(n * E), i64(n)
        other.zero_()
        full = timed(lambda: hip.tensor_decompress_seg_dbatch(frames, foff, soff, E, SEG_LOG, sf, n_segments=nseg, dst=other, max_total_blocks=blocks, planes=planes,
                                                              seg_offsets=so2, seg_results=sres, plane_offsets=poff2, plane_sizes=psz, workspace=dws, results=mres))
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        print(json.dumps(dict(shape=name, codec=cname, segment_log=SEG_LOG, call="full", frames=nseg, ms=round(full, 3), GBps=round(total / full / 1e6, 2))), flush=True)
        del dws
        share = numel // 8
        mid = (numel // 2 - share // 2) | 12345                                         # unaligned to a segment, to an element of sixteen, to anything
        for wname, a in (("all", 0), ("start", 0), ("middle", mid), ("end", numel - share)):
            b = numel if wname == "all" else a + share
            windows = [(a, b)] * n
            sel, wblocks = hip.planes_window_first([tbytes] * n, windows, E, SEG_LOG, BSID)
            nsel = int(sel[-1])
            wbytes = E * (b - a)
            doff = dev(np.arange(n + 1, dtype=np.int64) * wbytes)
            out = other[:n * wbytes]
            out.zero_()
            wws = ws(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, C.c_size_t(nsel), C.c_size_t(wblocks))
            wf, win = dev(sel), dev(windows)
            sfo, wo, wres, wpo, wps, res = i64(nsel + 1), i64(nsel + 1), i64(nsel), i64(n * E), i64(n * E), i64(n)
            wplanes = planes[:nsel << SEG_LOG]
            t = timed(lambda: hip.tensor_decompress_window_dbatch(frames, foff, soff, win, doff, E, SEG_LOG, sf, n_segments=nseg, sel_first=wf, n_selected=nsel, dst=out,
                                                                  max_total_blocks=wblocks, planes=wplanes, sel_frame_offsets=sfo, sel_offsets=wo, sel_results=wres,
                                                                  plane_offsets=wpo, plane_sizes=wps, workspace=wws, results=res))
            assert bool((res == wbytes).all())
            for i in range(n):
                assert torch.equal(out[i * wbytes:(i + 1) * wbytes], src[i * tbytes + a * E:i * tbytes + b * E]), (wname, i)
            print(json.dumps(dict(shape=name, codec=cname, segment_log=SEG_LOG, call="window", window=wname, elements=[a, b], frames=nsel, blocks=wblocks,
                                  scratch_MiB=round((nsel << SEG_LOG) / 2 ** 20, 1), ms=round(t, 3), GBps=round(n * wbytes / t / 1e6, 2), vs_full=round(t / full, 3),
                                  vs_eighth_of_full=round(t / (full / 8), 3))), flush=True)
            del wws
        # the yardstick once more, behind the windows: what the order of the calls alone does to it
        dws = ws(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, C.c_size_t(nseg), C.c_size_t(blocks))
        again = timed(lambda: hip.tensor_decompress_seg_dbatch(frames, foff, soff, E, SEG_LOG, sf, n_segments=nseg, dst=other, max_total_blocks=blocks, planes=planes,
                                                               seg_offsets=so2, seg_results=sres, plane_offsets=poff2, plane_sizes=psz, workspace=dws, results=mres))
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        print(json.dumps(dict(shape=name, codec=cname, segment_log=SEG_LOG, call="full again", frames=nseg, ms=round(again, 3), vs_full=round(again / full, 3))), flush=True)
        del dws, frames
        torch.cuda.empty_cache()

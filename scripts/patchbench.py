"""development aid: patching segmented tensors (FSEHIP_tensor_patch_window_dbatch) next to the only way the library had to the same object, the
full FSEHIP_tensor_compress_seg_dbatch of the changed tensors in the same run, and next to a device copy of as many bytes as the object has --
1 GiB of bf16 data, N(0, 0.02) generated on the device, cut into
  (b) 8 tensors of 128 MiB      (c) one tensor of 1 GiB
with segment_log 18, per codec.  The tensors change inside a window: every element, and 1/8 of each tensor at its start, in its middle
(unaligned to a segment) and at its end.  Device events around the calls, repeated until the timed region is at least MIN_MS long, after one
warm-up call of the same shape.  Every patched object is compared with the full call's for the changed tensors: offsets, results and every
byte up to the total (the bar for the window over every element; the defining identity for the others).  The splice is also timed alone:
with nothing selected it moves the object's bytes once.  One JSON line per figure.
Usage: patchbench.py [--total-mib 1024] [--block-size-id 5] [--segment-log 18]"""
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


def u8(n):
    return torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")


def dev(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64).reshape(-1)).cuda()


total = args.total_mib << 20
gen = torch.Generator(device="cuda").manual_seed(1)
src = (torch.randn(total // 2, generator=gen, device="cuda") * 0.02).to(torch.bfloat16).view(torch.uint8)
fresh = (torch.randn(total // 2, generator=gen, device="cuda") * 0.02).to(torch.bfloat16).view(torch.uint8)
planes, changed = torch.empty_like(src), torch.empty_like(src)
L = hip.lib

for shape, n in (("b", 8), ("c", 1)):
    tbytes = total // n
    numel = tbytes // E
    name = "%d x %d MiB bf16" % (n, tbytes >> 20)
    soff = torch.from_numpy(np.arange(n + 1, dtype=np.int64) * tbytes).cuda()
    blocks = hip.planes_block_bound(total, n, E, BSID)
    first = hip.planes_segment_first([tbytes] * n, E, SEG_LOG)
    nseg = int(first[-1])
    sf = dev(first)
    fcap = hip.frame_packed_bound(total, nseg, blocks, 0)
    scratch = u8(hip.planes_splice_scratch_bound(n, E, nseg))
    for codec, cname in ((0, "fse"), (1, "huf")):
        cws = ws(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize, C.c_size_t(nseg), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(codec))
        frames, full = u8(fcap), u8(fcap)
        foff, fres, so, tres, poff = i64(nseg + 1), i64(nseg), i64(nseg + 1), i64(n), i64(n * E + 1)
        goff, gres = i64(nseg + 1), i64(nseg)

        def compress(s, dst, off, res):
            hip.tensor_compress_seg_dbatch(s, soff, E, SEG_LOG, sf, n_segments=nseg, codec=codec, block_size_id=BSID, dst=dst, max_total_blocks=blocks, frame_offsets=off,
                                           frame_results=res, tensor_results=tres, planes=planes, plane_offsets=poff, seg_offsets=so, workspace=cws)
        # the yardsticks: the full compress, the parent's only way to the object, and a copy of as many bytes as the object has
        t_full = timed(lambda: compress(src, frames, foff, fres))
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        obytes = int(foff[-1])
        t_copy = timed(lambda: full[:obytes].copy_(frames[:obytes]))
        print(json.dumps(dict(shape=name, codec=cname, segment_log=SEG_LOG, call="full compress", frames=nseg, object_MiB=round(obytes / 2 ** 20, 1), ms=round(t_full, 3),
                              GBps=round(total / t_full / 1e6, 2))), flush=True)
        print(json.dumps(dict(shape=name, codec=cname, call="copy of the object", ms=round(t_copy, 4), GBps=round(obytes / t_copy / 1e6, 1))), flush=True)
        share = numel // 8
        mid = (numel // 2 - share // 2) | 12345                                         # unaligned to a segment, to an element of sixteen, to anything
        for wname, a in (("none", 0), ("all", 0), ("start", 0), ("middle", mid), ("end", numel - share)):
            b = a if wname == "none" else numel if wname == "all" else a + share
            windows = [(a, b)] * n
            changed.copy_(src)
            for i in range(n):
                changed[i * tbytes + a * E:i * tbytes + b * E] = fresh[i * tbytes + a * E:i * tbytes + b * E]
            sel, wblocks = hip.planes_window_first([tbytes] * n, windows, E, SEG_LOG, BSID)
            toff = hip.planes_stage_offsets([tbytes] * n, windows, E, SEG_LOG)
            nsel, sbytes = int(sel[-1]), int(toff[-1])
            new_cap = hip.frame_packed_bound(sbytes, nsel, wblocks, 0)
            out_cap = obytes + new_cap
            wws = ws(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize, C.c_size_t(nsel), C.c_size_t(wblocks), C.c_uint(BSID), C.c_int(codec))
            wf, win, tf = dev(sel), dev(windows), dev(toff)
            out, stage, newf = u8(out_cap), u8(sbytes), u8(new_cap)
            ooff, ores, pres, noff, nres, sso, spo, sres = i64(nseg + 1), i64(nseg), i64(n), i64(nsel + 1), i64(nsel), i64(nsel + 1), i64(n * E + 1), i64(n)
            old = frames[:obytes]

            def patch():
                hip.tensor_patch_window_dbatch(old, foff, fres, changed, soff, win, E, SEG_LOG, sf, n_segments=nseg, sel_first=wf, n_selected=nsel, stage_offsets=tf,
                                               codec=codec, block_size_id=BSID, max_total_blocks=wblocks, out=out, out_capacity=out_cap, out_offsets=ooff, out_results=ores,
                                               tensor_results=pres, stage=stage, stage_capacity=sbytes, stage_plane_offsets=spo, stage_seg_offsets=sso, stage_results=sres,
                                               new_frames=newf, new_capacity=new_cap, new_offsets=noff, new_results=nres, scratch=scratch, workspace=wws)

            def splice():
                hip.planes_splice_dbatch(old, foff, fres, newf, noff, nres, soff, win, sf, wf, E, SEG_LOG, n_segments=nseg, n_selected=nsel, stage_results=sres, out=out,
                                         out_capacity=out_cap, out_offsets=ooff, out_results=ores, tensor_results=pres, scratch=scratch)
            t = timed(patch)
            assert bool((pres == tbytes).all())
            # the same object as the full call's for the changed tensors
            compress(changed, full, goff, gres)
            nbytes = int(goff[-1])
            assert torch.equal(goff, ooff) and torch.equal(gres, ores) and torch.equal(full[:nbytes], out[:nbytes]), wname
            ts = timed(splice)
            assert bool((pres == tbytes).all()) and torch.equal(full[:nbytes], out[:nbytes]), wname
            print(json.dumps(dict(shape=name, codec=cname, segment_log=SEG_LOG, call="patch", window=wname, elements=[a, b], frames=nsel, blocks=wblocks,
                                  staged_MiB=round(sbytes / 2 ** 20, 1), object_MiB=round(nbytes / 2 ** 20, 1), same_as_full=True, ms=round(t, 3), vs_full=round(t / t_full, 3),
                                  vs_eighth_of_full=round(t / (t_full / 8), 3), vs_full_plus_copy=round(t / (t_full + t_copy), 3), splice_ms=round(ts, 4),
                                  splice_GBps=round(nbytes / ts / 1e6, 1), splice_vs_copy_rate=round((nbytes / ts) / (obytes / t_copy), 3))), flush=True)
            del wws, out, stage, newf
        # the yardstick once more, behind the patches: what the order of the calls alone does to it
        again = timed(lambda: compress(src, frames, foff, fres))
        print(json.dumps(dict(shape=name, codec=cname, segment_log=SEG_LOG, call="full compress again", ms=round(again, 3), vs_full=round(again / t_full, 3))), flush=True)
        del cws, frames, full
        torch.cuda.empty_cache()

"""development aid: windows of objects with a transform per tensor (FSEHIP_tensor_decompress_window_each_dbatch) next to the full read of the
same object in the same run (FSEHIP_tensor_decompress_seg_each_dbatch), and -- for the all-PLAIN object, whose frames are those of
FSEHIP_tensor_compress_seg_dbatch -- next to the existing window call (FSEHIP_tensor_decompress_window_dbatch) on the same tensors.  1 GiB of
bf16 data, N(0, 0.02) generated on the device, cut into
  (a) one tensor of 1 GiB      (b) 1024 tensors of 1 MiB
with segment_log 18, FSE, written as each-objects with the transforms GIVEN: all PLAIN, all PRED and, for (b), the mixed batch of eachbench.py --
tensor i from source i mod 3: a gaussian whose base is unrelated, an update pair, tensor == base -- with the transforms CHOSEN on the device
(mask 15), as compress_tensors_each(ts, "auto", base) writes it.  Windows: 1/8 of every tensor in its middle, its start off a run boundary of the
predicted planes (a % 1024 != 0), off a segment and off an element of sixteen.  Device events around the calls, repeated until the timed
region is at least MIN_MS long, after one warm-up call of the same shape.  Every window's bytes are compared with the source's.  One JSON
line per figure: ms, the scratch the call needs for decoded planes, the ratio to the full read and to 1/8 of the full read.  The existing
window call is timed five times first; the each-window of the PLAIN object is reported against the fastest and the slowest of the five.
Usage: eachwindowbench.py [--total-mib 1024] [--block-size-id 5] [--segment-log 18]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import EST_NAMES, FseHip

MIN_MS = 200.0
ap = argparse.ArgumentParser()
ap.add_argument("--total-mib", type=int, default=1024); ap.add_argument("--block-size-id", type=int, default=5); ap.add_argument("--segment-log", type=int, default=18)
args = ap.parse_args()
hip = FseHip()
BSID, E, SEG_LOG = args.block_size_id, 2, args.segment_log
PLAIN, PRED = 0, 1


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


def bf16(x):
    return x.to(torch.bfloat16).view(torch.uint8)


total = args.total_mib << 20
gen = torch.Generator(device="cuda").manual_seed(1)
src = bf16(torch.randn(total // 2, generator=gen, device="cuda") * 0.02)
planes, other = torch.empty_like(src), torch.empty_like(src)
L = hip.lib
RSIZE = L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize

for shape, n in (("a", 1), ("b", total >> 20)):
    tbytes = total // n
    numel = tbytes // E
    name = "%d x %d MiB bf16" % (n, tbytes >> 20)
    soff = dev(np.arange(n + 1, dtype=np.int64) * tbytes)
    blocks = hip.planes_block_bound(total, n, E, BSID)
    first = hip.planes_segment_first([tbytes] * n, E, SEG_LOG)
    nseg = int(first[-1])
    sf = dev(first)
    share = numel // 8
    a = (numel // 2 - share // 2) | 12345
    b = a + share
    assert a % 1024 and a % (1 << SEG_LOG) and b <= numel
    windows = [(a, b)] * n
    sel, wblocks = hip.planes_window_first([tbytes] * n, windows, E, SEG_LOG, BSID)
    nsel = int(sel[-1])
    wbytes = E * (b - a)
    doff = dev(np.arange(n + 1, dtype=np.int64) * wbytes)
    wf, win = dev(sel), dev(windows)
    objects = [("plain", torch.full((n,), PLAIN, dtype=torch.uint8, device="cuda"), None), ("pred", torch.full((n,), PRED, dtype=torch.uint8, device="cuda"), None)]
    if n > 1:
        objects.append(("mixed", None, "chosen"))
    frames = torch.empty(hip.frame_packed_bound(total, nseg, blocks, 0), dtype=torch.uint8, device="cuda")
    for oname, tr, how in objects:
        data, base = src, None
        if how == "chosen":                                     # tensor i from source i mod 3: a gaussian (base unrelated), an update of the base, tensor == base
            kind = torch.arange(n, device="cuda") % 3
            rows = lambda t: t.view(n, tbytes)
            base = bf16(torch.randn(total // 2, generator=gen, device="cuda") * 0.02)
            upd = bf16(base.view(torch.bfloat16).float() * (1 + 1e-3 * torch.randn(total // 2, generator=gen, device="cuda")))
            data = torch.where((kind == 0)[:, None], rows(src), torch.where((kind == 1)[:, None], rows(upd), rows(base))).reshape(-1).contiguous()
            del upd
        foff, fres, so, tres, poff = i64(nseg + 1), i64(nseg), i64(nseg + 1), i64(n), i64(n * E + 1)
        _, _, _, _, _, tr = hip.tensor_compress_seg_each_dbatch(data, soff, E, SEG_LOG, tr, base, 15 if how == "chosen" else None, 50, seg_first=sf, n_segments=nseg, codec=0,
                                                                block_size_id=BSID, dst=frames, max_total_blocks=blocks, frame_offsets=foff, frame_results=fres,
                                                                tensor_results=tres, planes=planes, plane_offsets=poff, seg_offsets=so)
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        picks = np.bincount(tr.cpu().numpy(), minlength=4).tolist()
        common = dict(shape=name, object=oname, transforms={EST_NAMES[c]: picks[c] for c in range(4) if picks[c]}, segment_log=SEG_LOG, frame_bytes=int(foff[-1].item()))
        # the yardstick: the full read of the same object
        dws = ws(RSIZE, C.c_size_t(nseg), C.c_size_t(blocks))
        so2, sres, poff2, psz, mres = i64(nseg + 1), i64(nseg), i64(n * E + 1), i64(n * E), i64(n)
        full = timed(lambda: hip.tensor_decompress_seg_each_dbatch(frames, foff, soff, E, SEG_LOG, tr, base, sf, n_segments=nseg, dst=other, max_total_blocks=blocks,
                                                                   planes=planes, seg_offsets=so2, seg_results=sres, plane_offsets=poff2, plane_sizes=psz, workspace=dws,
                                                                   results=mres))
        assert bool((mres == tbytes).all()) and torch.equal(other, data)
        print(json.dumps(dict(common, call="full each-read", frames=nseg, scratch_MiB=round(total / 2 ** 20, 1), ms=round(full, 3), GBps=round(total / full / 1e6, 2))),
              flush=True)
        del dws
        wws = ws(RSIZE, C.c_size_t(nsel), C.c_size_t(wblocks))
        sfo, wo, wres, wpo, wps, res = i64(nsel + 1), i64(nsel + 1), i64(nsel), i64(n * E), i64(n * E), i64(n)
        wplanes = planes[:nsel << SEG_LOG]
        out = other[:n * wbytes]
        wbase = None if base is None else torch.cat([base[i * tbytes + a * E:i * tbytes + b * E] for i in range(n)])       # the base in the destination's layout
        kw = dict(n_segments=nseg, sel_first=wf, n_selected=nsel, dst=out, max_total_blocks=wblocks, planes=wplanes, sel_frame_offsets=sfo, sel_offsets=wo,
                  sel_results=wres, plane_offsets=wpo, plane_sizes=wps, workspace=wws, results=res)

        def check(what):
            assert bool((res == wbytes).all()) and torch.equal(out.view(n, wbytes), data.view(n, tbytes)[:, a * E:b * E]), what
        spread = None
        if oname == "plain":                                    # the existing window call on the object of tensor_compress_seg_dbatch: the same frames
            frames2 = torch.empty_like(frames)
            foff2 = i64(nseg + 1)
            hip.tensor_compress_seg_dbatch(src, soff, E, SEG_LOG, sf, n_segments=nseg, codec=0, block_size_id=BSID, dst=frames2, max_total_blocks=blocks, frame_offsets=foff2,
                                           frame_results=i64(nseg), tensor_results=i64(n), planes=planes, plane_offsets=i64(n * E + 1), seg_offsets=i64(nseg + 1))
            assert torch.equal(foff2, foff) and torch.equal(frames2[:int(foff[-1])], frames[:int(foff[-1])]), "an all-PLAIN each-object is the segmented object"
            runs = []
            for _ in range(5):
                out.zero_()
                runs.append(timed(lambda: hip.tensor_decompress_window_dbatch(frames2, foff2, soff, win, doff, E, SEG_LOG, sf, **kw)))
                check("the existing window call")
            spread = (min(runs), max(runs))
            print(json.dumps(dict(common, call="existing window call, five runs", elements=[a, b], frames=nsel, ms=[round(x, 3) for x in runs],
                                  spread_permille=round(1000 * (spread[1] - spread[0]) / spread[0], 1))), flush=True)
            del frames2
        out.zero_()
        t = timed(lambda: hip.tensor_decompress_window_each_dbatch(frames, foff, soff, win, doff, E, SEG_LOG, tr, sf, base=wbase, **kw))
        check("the each-window")
        line = dict(common, call="each-window", elements=[a, b], lead=a % 1024, frames=nsel, blocks=wblocks, scratch_MiB=round((nsel << SEG_LOG) / 2 ** 20, 1), ms=round(t, 3),
                    GBps=round(n * wbytes / t / 1e6, 2), vs_full=round(t / full, 3), vs_eighth_of_full=round(t / (full / 8), 3))
        if spread is not None:
            line.update(vs_existing_fastest=round(t / spread[0], 3), vs_existing_slowest=round(t / spread[1], 3),
                        verdict="within the spread of the existing call" if t <= spread[1] else "SLOWER than the slowest run of the existing call")
        print(json.dumps(line), flush=True)
        del wws, wbase
        torch.cuda.empty_cache()
    del frames
    torch.cuda.empty_cache()

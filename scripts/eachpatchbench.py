"""development aid: patches of objects with a transform per tensor (FSEHIP_tensor_patch_window_each_dbatch) next to the only way the library had
to the same object, the full FSEHIP_tensor_compress_seg_each_dbatch of the changed tensors with the same transforms given, in the same run, and
-- for the all-PLAIN object, whose frames are those of FSEHIP_tensor_compress_seg_dbatch -- next to the existing patch call
(FSEHIP_tensor_patch_window_op_dbatch) on the byte-identical object.  1 GiB of bf16 data, N(0, 0.02) generated on the device, cut into 8
tensors of 128 MiB with segment_log 18, per codec, written as each-objects with the transforms GIVEN: all PLAIN, all PRED and mixed (tensor i
takes transform i mod 4; the base is the data before an update of one part in a thousand).  The tensors change inside a window: nothing,
every element, and 1/8 of each tensor at its start, in its middle (off a segment, off a run of the predicted planes, off an element of
sixteen) and at its end.  Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of
the same shape.  EVERY timed patch is compared with the full call's object for the changed tensors: offsets, results and every byte up to the
total -- the script asserts it.  The existing patch call is timed RUNS times per 1/8 window; the each-patch of the PLAIN object is reported
against the fastest and the slowest of them.  One JSON line per figure.
Usage: eachpatchbench.py [--total-mib 1024] [--block-size-id 5] [--segment-log 18]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import EST_NAMES, FseHip

MIN_MS, RUNS = 200.0, 5
ap = argparse.ArgumentParser()
ap.add_argument("--total-mib", type=int, default=1024); ap.add_argument("--block-size-id", type=int, default=5); ap.add_argument("--segment-log", type=int, default=18)
args = ap.parse_args()
hip = FseHip()
BSID, E, SEG_LOG, N = args.block_size_id, 2, args.segment_log, 8


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


def bf16(x):
    return x.to(torch.bfloat16).view(torch.uint8)


total = args.total_mib << 20
gen = torch.Generator(device="cuda").manual_seed(1)
base = bf16(torch.randn(total // 2, generator=gen, device="cuda") * 0.02)
src = bf16(base.view(torch.bfloat16).float() * (1 + 1e-3 * torch.randn(total // 2, generator=gen, device="cuda")))
fresh = bf16(base.view(torch.bfloat16).float() * (1 + 1e-3 * torch.randn(total // 2, generator=gen, device="cuda")))
planes, changed = torch.empty_like(src), torch.empty_like(src)
L = hip.lib
WSIZE = L.FSEHIP_frame_compress_packed_dbatch_workspaceSize

n = N
tbytes = total // n
numel = tbytes // E
name = "%d x %d MiB bf16" % (n, tbytes >> 20)
soff = dev(np.arange(n + 1, dtype=np.int64) * tbytes)
blocks = hip.planes_block_bound(total, n, E, BSID)
first = hip.planes_segment_first([tbytes] * n, E, SEG_LOG)
nseg = int(first[-1])
sf = dev(first)
fcap = hip.frame_packed_bound(total, nseg, blocks, 0)
scratch = u8(hip.planes_splice_scratch_bound(n, E, nseg))
share = numel // 8
mid = (numel // 2 - share // 2) | 12345                           # off a segment, off a run of 1024, off an element of sixteen
assert mid % 1024 and mid % (1 << SEG_LOG) and mid + share <= numel
WINDOWS = (("none", 0, 0), ("all", 0, numel), ("start", 0, share), ("middle", mid, mid + share), ("end", numel - share, numel))
OBJECTS = (("plain", [0] * n), ("pred", [1] * n), ("mixed", [i % 4 for i in range(n)]))

for codec, cname in ((0, "fse"), (1, "huf")):
    cws = ws(WSIZE, C.c_size_t(nseg), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(codec))
    frames, full = u8(fcap), u8(fcap)
    foff, fres, so, tres, poff = i64(nseg + 1), i64(nseg), i64(nseg + 1), i64(n), i64(n * E + 1)
    goff, gres = i64(nseg + 1), i64(nseg)
    fulls = {}
    for oname, ids in OBJECTS:
        tr = torch.tensor(ids, dtype=torch.uint8, device="cuda")

        def compress(s, dst, off, res):
            hip.tensor_compress_seg_each_dbatch(s, soff, E, SEG_LOG, tr, base, seg_first=sf, n_segments=nseg, codec=codec, block_size_id=BSID, dst=dst, max_total_blocks=blocks,
                                                frame_offsets=off, frame_results=res, tensor_results=tres, planes=planes, plane_offsets=poff, seg_offsets=so, workspace=cws)
        # the yardstick: the full compress with the same transforms given, the parent's only way to the object
        t_full = fulls[oname] = timed(lambda: compress(src, frames, foff, fres))
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        obytes = int(foff[-1])
        picks = np.bincount(np.asarray(ids), minlength=4).tolist()
        common = dict(shape=name, codec=cname, object=oname, transforms={EST_NAMES[c]: picks[c] for c in range(4) if picks[c]}, segment_log=SEG_LOG)
        print(json.dumps(dict(common, call="full each-compress, transforms given", frames=nseg, object_MiB=round(obytes / 2 ** 20, 1), ms=round(t_full, 3),
                              GBps=round(total / t_full / 1e6, 2))), flush=True)
        if oname == "plain":                                    # the object of tensor_compress_seg_dbatch: the same bytes
            hip.tensor_compress_seg_dbatch(src, soff, E, SEG_LOG, sf, n_segments=nseg, codec=codec, block_size_id=BSID, dst=full, max_total_blocks=blocks, frame_offsets=goff,
                                           frame_results=gres, tensor_results=i64(n), planes=planes, plane_offsets=i64(n * E + 1), seg_offsets=i64(nseg + 1), workspace=cws)
            assert torch.equal(goff, foff) and torch.equal(gres, fres) and torch.equal(full[:obytes], frames[:obytes]), "an all-PLAIN each-object is the segmented object"
        eighths = []
        for wname, a, b in WINDOWS:
            windows = [(a, b)] * n
            changed.copy_(src)
            for i in range(n):
                changed[i * tbytes + a * E:i * tbytes + b * E] = fresh[i * tbytes + a * E:i * tbytes + b * E]
            sel, wblocks = hip.planes_window_first([tbytes] * n, windows, E, SEG_LOG, BSID)
            toff = hip.planes_stage_offsets([tbytes] * n, windows, E, SEG_LOG)
            nsel, sbytes = int(sel[-1]), int(toff[-1])
            new_cap = hip.frame_packed_bound(sbytes, nsel, wblocks, 0)
            out_cap = obytes + new_cap
            wws = ws(WSIZE, C.c_size_t(nsel), C.c_size_t(wblocks), C.c_uint(BSID), C.c_int(codec))
            wf, win, tf = dev(sel), dev(windows), dev(toff)
            out, stage, newf = u8(out_cap), u8(sbytes), u8(new_cap)
            ooff, ores, pres, noff, nres, sso, spo, sres = i64(nseg + 1), i64(nseg), i64(n), i64(nsel + 1), i64(nsel), i64(nsel + 1), i64(n * E + 1), i64(n)
            old = frames[:obytes]
            kw = dict(n_segments=nseg, sel_first=wf, n_selected=nsel, stage_offsets=tf, codec=codec, block_size_id=BSID, max_total_blocks=wblocks, out=out, out_capacity=out_cap,
                      out_offsets=ooff, out_results=ores, tensor_results=pres, stage=stage, stage_capacity=sbytes, stage_plane_offsets=spo, stage_seg_offsets=sso,
                      stage_results=sres, new_frames=newf, new_capacity=new_cap, new_offsets=noff, new_results=nres, scratch=scratch, workspace=wws)
            # the full call's object for the changed tensors: what every timed patch below has to equal
            compress(changed, full, goff, gres)
            nbytes = int(goff[-1])

            def same(what):
                assert bool((pres == tbytes).all()) and torch.equal(goff, ooff) and torch.equal(gres, ores) and torch.equal(full[:nbytes], out[:nbytes]), (oname, wname, what)
            spread = None
            if oname == "plain" and wname in ("start", "middle", "end"):
                runs = []
                for _ in range(RUNS):
                    out.zero_(); ores.zero_()
                    runs.append(timed(lambda: hip.tensor_patch_window_dbatch(old, foff, fres, changed, soff, win, E, SEG_LOG, sf, **kw)))
                    same("the existing patch call")
                spread = (min(runs), max(runs))
                print(json.dumps(dict(common, call="existing patch call, %d runs" % RUNS, window=wname, elements=[a, b], frames=nsel, ms=[round(x, 3) for x in runs],
                                      spread_permille=round(1000 * (spread[1] - spread[0]) / spread[0], 1))), flush=True)
            out.zero_(); ores.zero_()
            t = timed(lambda: hip.tensor_patch_window_each_dbatch(old, foff, fres, changed, soff, win, E, SEG_LOG, tr, sf, base=base, **kw))
            same("the each-patch")
            line = dict(common, call="each-patch", window=wname, elements=[a, b], frames=nsel, blocks=wblocks, staged_MiB=round(sbytes / 2 ** 20, 1),
                        object_MiB=round(nbytes / 2 ** 20, 1), same_as_full=True, ms=round(t, 3), vs_full=round(t / t_full, 3), vs_eighth_of_full=round(t / (t_full / 8), 3))
            if wname in ("start", "middle", "end"):
                eighths.append(t)
                line.update(below_full=bool(t < t_full))
            if spread is not None:
                line.update(vs_existing_fastest=round(t / spread[0], 3), vs_existing_slowest=round(t / spread[1], 3),
                            verdict="within the spread of the existing call" if spread[0] <= t <= spread[1] else
                            "FASTER than the fastest run of the existing call" if t < spread[0] else "SLOWER than the slowest run of the existing call")
            print(json.dumps(line), flush=True)
            del wws, out, stage, newf
        fulls[oname + " eighth"] = sum(eighths) / len(eighths)
        again = timed(lambda: compress(src, frames, foff, fres))
        print(json.dumps(dict(common, call="full each-compress again", ms=round(again, 3), vs_full=round(again / t_full, 3))), flush=True)
    # what is expected: the PRED patch differs from the PLAIN patch by about what the two full compresses differ by
    print(json.dumps(dict(shape=name, codec=cname, call="pred against plain", full_pred_vs_plain=round(fulls["pred"] / fulls["plain"], 3),
                          eighth_patch_pred_vs_plain=round(fulls["pred eighth"] / fulls["plain eighth"], 3),
                          eighth_patch_mixed_vs_plain=round(fulls["mixed eighth"] / fulls["plain eighth"], 3))), flush=True)
    del cws, frames, full
    torch.cuda.empty_cache()

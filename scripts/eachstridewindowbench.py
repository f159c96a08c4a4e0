"""development aid: windows and patches of objects that hold a stride above 1 (FSEHIP_tensor_decompress_window_each_stride_dbatch,
FSEHIP_tensor_patch_window_each_stride_dbatch) next to the only things the library could do with such an object before -- the full read
(FSEHIP_tensor_decompress_seg_each_stride_dbatch) and the full compress of the changed tensors with transforms and strides given
(FSEHIP_tensor_compress_seg_each_stride_dbatch) -- and next to the stride-1 window calls (FSEHIP_tensor_decompress_window_each_dbatch,
FSEHIP_tensor_patch_window_each_dbatch) on the SAME data written as a stride-1 PRED object, all in the same run.  Interleaved data generated on
the device from a seed: int16 stereo (two random walks, stride 2) and float32 xyz (a random-walk trajectory, stride 3), cut into 8 tensors with
segment_log 18, per codec.  An eighth of every tensor is read, and is changed and patched: at its start, in its middle (off a segment, off a
run of the predicted planes, off an element of sixteen, the lead no multiple of the stride) and at its end.  Device events around the calls,
repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  EVERY timed read is compared with the slice
of the tensors and every timed patch with the full call's object for the changed tensors -- offsets, results and every byte up to the total:
the script asserts it.  One JSON line per figure.
Usage: eachstridewindowbench.py [--total-mib 512] [--block-size-id 5] [--segment-log 18]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import FseHip

MIN_MS = 200.0
PRED = 1
ap = argparse.ArgumentParser()
ap.add_argument("--total-mib", type=int, default=512); ap.add_argument("--block-size-id", type=int, default=5); ap.add_argument("--segment-log", type=int, default=18)
args = ap.parse_args()
hip = FseHip()
BSID, SEG_LOG, N = args.block_size_id, args.segment_log, 8


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


def stereo(numel, gen):
    """int16 stereo: two different random walks, interleaved (the sums wrap in 16 bits)"""
    steps = torch.randint(-40, 41, (numel // 2, 2), generator=gen, device="cuda", dtype=torch.int32)
    return (torch.cumsum(steps, 0, dtype=torch.int32) + torch.tensor([0, 3000], dtype=torch.int32, device="cuda")).to(torch.int16).reshape(-1).view(torch.uint8)


def xyz(numel, gen):
    """float32 xyz: a random-walk trajectory, each axis around an offset of its own; the last numel mod 3 elements are zeros"""
    pos = torch.tensor([100.0, -37.0, 5.5], device="cuda") + torch.cumsum(torch.randn((numel // 3, 3), generator=gen, device="cuda") * 1e-4, 0)
    out = torch.zeros(numel, dtype=torch.float32, device="cuda")
    out[:numel // 3 * 3] = pos.reshape(-1)
    return out.view(torch.uint8)


total = args.total_mib << 20
tbytes = total // N
L = hip.lib
RSIZE, WSIZE = L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, L.FSEHIP_frame_compress_packed_dbatch_workspaceSize

for dname, E, S, make in (("int16 stereo", 2, 2, stereo), ("float32 xyz", 4, 3, xyz)):
    numel = tbytes // E
    name = "%d x %d MiB %s" % (N, tbytes >> 20, dname)
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = torch.cat([make(numel, gen) for _ in range(N)])
    fresh = torch.cat([make(numel, gen) for _ in range(N)])
    planes, other, changed = torch.empty_like(src), torch.empty_like(src), torch.empty_like(src)
    soff = dev(np.arange(N + 1, dtype=np.int64) * tbytes)
    blocks = hip.planes_block_bound(total, N, E, BSID)
    first = hip.planes_segment_first([tbytes] * N, E, SEG_LOG)
    nseg = int(first[-1])
    sf = dev(first)
    fcap = hip.frame_packed_bound(total, nseg, blocks, 0)
    scratch = u8(hip.planes_splice_scratch_bound(N, E, nseg))
    share = numel // 8
    mid = (numel // 2 - share // 2) | 12347                       # off a segment, off a run of 1024, off an element of sixteen
    assert mid % 1024 and mid % (1 << SEG_LOG) and (mid % 1024) % S and mid + share <= numel
    WINDOWS = (("start", 0, share), ("middle", mid, mid + share), ("end", numel - share, numel))
    tr = torch.full((N,), PRED, dtype=torch.uint8, device="cuda")
    OBJECTS = (("stride %d" % S, torch.full((N,), S, dtype=torch.uint8, device="cuda")), ("stride 1", None))

    for codec, cname in ((0, "fse"), (1, "huf")):
        cws = ws(WSIZE, C.c_size_t(nseg), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(codec))
        dws = ws(RSIZE, C.c_size_t(nseg), C.c_size_t(blocks))
        frames, full = u8(fcap), u8(fcap)
        foff, fres, so, tres, poff = i64(nseg + 1), i64(nseg), i64(nseg + 1), i64(N), i64(N * E + 1)
        goff, gres = i64(nseg + 1), i64(nseg)
        sizes, reads, patches = {}, {}, {}
        for oname, st in OBJECTS:
            strided = st is not None

            def compress(s, dst, off, res):
                kw = dict(seg_first=sf, n_segments=nseg, codec=codec, block_size_id=BSID, dst=dst, max_total_blocks=blocks, frame_offsets=off, frame_results=res,
                          tensor_results=tres, planes=planes, plane_offsets=poff, seg_offsets=so, workspace=cws)
                if strided:
                    hip.tensor_compress_seg_each_stride_dbatch(s, soff, E, SEG_LOG, tr, st, **kw)
                else:
                    hip.tensor_compress_seg_each_dbatch(s, soff, E, SEG_LOG, tr, **kw)
            # the yardsticks: the full compress with transforms (and strides) given and the full read, all the parent has for a strided object
            t_comp = timed(lambda: compress(src, frames, foff, fres))
            assert bool((fres > 0).all()) and bool((tres == tbytes).all())
            obytes = sizes[oname] = int(foff[-1])
            so2, sres, poff2, psz, mres = i64(nseg + 1), i64(nseg), i64(N * E + 1), i64(N * E), i64(N)
            rkw = dict(n_segments=nseg, dst=other, max_total_blocks=blocks, planes=planes, seg_offsets=so2, seg_results=sres, plane_offsets=poff2, plane_sizes=psz,
                       workspace=dws, results=mres)
            if strided:
                t_read = timed(lambda: hip.tensor_decompress_seg_each_stride_dbatch(frames, foff, soff, E, SEG_LOG, tr, st, None, sf, **rkw))
            else:
                t_read = timed(lambda: hip.tensor_decompress_seg_each_dbatch(frames, foff, soff, E, SEG_LOG, tr, None, sf, **rkw))
            assert bool((mres == tbytes).all()) and torch.equal(other, src)
            common = dict(shape=name, codec=cname, object=oname, segment_log=SEG_LOG)
            print(json.dumps(dict(common, call="full compress, transforms%s given" % (" and strides" if strided else ""), frames=nseg,
                                  object_MiB=round(obytes / 2 ** 20, 1), ratio=round(total / obytes, 3), ms=round(t_comp, 3), GBps=round(total / t_comp / 1e6, 2))), flush=True)
            print(json.dumps(dict(common, call="full read", frames=nseg, ms=round(t_read, 3), GBps=round(total / t_read / 1e6, 2))), flush=True)
            for wname, a, b in WINDOWS:
                windows = [(a, b)] * N
                wbytes = E * (b - a)
                sel, wblocks = hip.planes_window_first([tbytes] * N, windows, E, SEG_LOG, BSID)
                nsel = int(sel[-1])
                wf, win = dev(sel), dev(windows)
                # ---- the read of the window
                doff = dev(np.arange(N + 1, dtype=np.int64) * wbytes)
                wws = ws(RSIZE, C.c_size_t(nsel), C.c_size_t(wblocks))
                sfo, wo, wres, wpo, wps, res = i64(nsel + 1), i64(nsel + 1), i64(nsel), i64(N * E), i64(N * E), i64(N)
                out = other[:N * wbytes]
                kw = dict(n_segments=nseg, sel_first=wf, n_selected=nsel, dst=out, max_total_blocks=wblocks, planes=planes[:nsel << SEG_LOG], sel_frame_offsets=sfo,
                          sel_offsets=wo, sel_results=wres, plane_offsets=wpo, plane_sizes=wps, workspace=wws, results=res)
                out.zero_()
                if strided:
                    t = timed(lambda: hip.tensor_decompress_window_each_stride_dbatch(frames, foff, soff, win, doff, E, SEG_LOG, tr, st, sf, **kw))
                else:
                    t = timed(lambda: hip.tensor_decompress_window_each_dbatch(frames, foff, soff, win, doff, E, SEG_LOG, tr, sf, **kw))
                assert bool((res == wbytes).all()) and torch.equal(out.view(N, wbytes), src.view(N, tbytes)[:, a * E:b * E]), (oname, wname, "the window read")
                reads[(oname, wname)] = t
                print(json.dumps(dict(common, call="window read", window=wname, elements=[a, b], lead=a % 1024, frames=nsel, same_as_slice=True, ms=round(t, 3),
                                      GBps=round(N * wbytes / t / 1e6, 2), vs_full_read=round(t / t_read, 3), vs_eighth_of_full_read=round(t / (t_read / 8), 3))), flush=True)
                del wws
                # ---- the patch of the window
                changed.copy_(src)
                for i in range(N):
                    changed[i * tbytes + a * E:i * tbytes + b * E] = fresh[i * tbytes + a * E:i * tbytes + b * E]
                toff = hip.planes_stage_offsets([tbytes] * N, windows, E, SEG_LOG)
                sbytes = int(toff[-1])
                new_cap = hip.frame_packed_bound(sbytes, nsel, wblocks, 0)
                out_cap = obytes + new_cap
                pws_ = ws(WSIZE, C.c_size_t(nsel), C.c_size_t(wblocks), C.c_uint(BSID), C.c_int(codec))
                tf = dev(toff)
                pout, stage, newf = u8(out_cap), u8(sbytes), u8(new_cap)
                ooff, ores, pres, noff, nres, sso, spo, stres = i64(nseg + 1), i64(nseg), i64(N), i64(nsel + 1), i64(nsel), i64(nsel + 1), i64(N * E + 1), i64(N)
                old = frames[:obytes]
                pkw = dict(n_segments=nseg, sel_first=wf, n_selected=nsel, stage_offsets=tf, codec=codec, block_size_id=BSID, max_total_blocks=wblocks, out=pout,
                           out_capacity=out_cap, out_offsets=ooff, out_results=ores, tensor_results=pres, stage=stage, stage_capacity=sbytes, stage_plane_offsets=spo,
                           stage_seg_offsets=sso, stage_results=stres, new_frames=newf, new_capacity=new_cap, new_offsets=noff, new_results=nres, scratch=scratch,
                           workspace=pws_)
                compress(changed, full, goff, gres)             # the full call's object for the changed tensors: what the timed patch has to equal
                nbytes = int(goff[-1])
                pout.zero_(); ores.zero_()
                if strided:
                    t = timed(lambda: hip.tensor_patch_window_each_stride_dbatch(old, foff, fres, changed, soff, win, E, SEG_LOG, tr, st, sf, **pkw))
                else:
                    t = timed(lambda: hip.tensor_patch_window_each_dbatch(old, foff, fres, changed, soff, win, E, SEG_LOG, tr, sf, **pkw))
                assert bool((pres == tbytes).all()) and torch.equal(goff, ooff) and torch.equal(gres, ores) and torch.equal(full[:nbytes], pout[:nbytes]), (oname, wname, "patch")
                patches[(oname, wname)] = t
                print(json.dumps(dict(common, call="window patch", window=wname, elements=[a, b], frames=nsel, staged_MiB=round(sbytes / 2 ** 20, 1),
                                      object_MiB=round(nbytes / 2 ** 20, 1), same_as_full=True, ms=round(t, 3), vs_full_compress=round(t / t_comp, 3),
                                      vs_eighth_of_full_compress=round(t / (t_comp / 8), 3))), flush=True)
                del pws_, pout, stage, newf
            del so2, sres, poff2, psz, mres
        # the strided window calls against the stride-1 window calls on the same data, and what the stride buys in bytes
        sname = OBJECTS[0][0]
        print(json.dumps(dict(shape=name, codec=cname, call="stride %d against stride 1" % S, object_bytes_ratio=round(sizes[sname] / sizes["stride 1"], 3),
                              window_read={w: round(reads[(sname, w)] / reads[("stride 1", w)], 3) for w, _, _ in WINDOWS},
                              window_patch={w: round(patches[(sname, w)] / patches[("stride 1", w)], 3) for w, _, _ in WINDOWS})), flush=True)
        del cws, dws, frames, full
        torch.cuda.empty_cache()
    del src, fresh, planes, other, changed, scratch
    torch.cuda.empty_cache()

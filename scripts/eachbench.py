"""development aid: the per-tensor-transform calls (FSEHIP_planes_split_each_dbatch / _merge_each_dbatch, FSEHIP_tensor_compress_seg_each_dbatch
with FSEHIP_TRANSFORMS_CHOOSE) next to the dedicated calls they are byte-identical to, the yardstick being THE PARENT COMMIT'S LIBRARY loaded
beside this tree's (--parent-lib PATH, required).
  (a) data kernels, 1024 tensors of 1 MiB of bf16 bytes generated on the device (a gaussian, its base an update of it), per element size
      1, 2, 4, 8 and per transform plain, pred, xor, sub: the parent's dedicated split and merge, then split_each and merge_each with the
      uniform transform array; "vs_dedicated" = the each kernel's GB/s over the dedicated kernel's, "bar" = whether that reaches 0.5 (DESIGN.md
      4.4h, 4.4k; held for elements of 2 and 4 bytes, the others are reported).  A fifth row: the four transforms in rotation over the
      tensors, against the mean of the four dedicated rates.  The plain split of 1-byte elements moves nothing: its yardstick is a device copy.
      Every each output is compared with the dedicated one (torch.equal) outside the timed region.
  (b) the segmented CHOOSE composite (FSE, segment_log 18, 2-byte elements) end to end on mixed batches -- the tensors drawn in rotation
      from estimatebench.py's sources (a gaussian pair, an update pair, tensor == base) -- with and without a base, against the parent's
      flow for the same batch at the C level: the estimate, the read-back of the choices, one gather and one segmented composite per chosen
      part (what compress_tensors_auto does).  Both times, the launches of each (the nodes of a captured graph; null where the capture
      fails), and the frame totals, which must be equal (asserted).
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape; the
parent's flow, which reads back, is timed by the host clock around synchronised repetitions.  Prints one JSON line per figure.
Usage: eachbench.py --parent-lib PATH [--tensors 1024] [--tensor-kib 1024] [--only data|composite]"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd import _lib
from finitestateentropy_amd.api import EST_NAMES, FseHip

MIN_MS, BAR, SEG_LOG, BSID = 300.0, 0.5, 18, 5
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True); ap.add_argument("--tensors", type=int, default=1024); ap.add_argument("--tensor-kib", type=int, default=1024)
ap.add_argument("--only", default=None, choices=("data", "composite"))
args = ap.parse_args()
hip = FseHip()
_lib._LIB = C.CDLL(os.path.abspath(args.parent_lib))            # a second binding over the parent's library: its dedicated calls are the yardstick
parent = FseHip()
_lib._LIB = hip.lib
assert not hasattr(parent.lib, "FSEHIP_planes_split_each_dbatch"), "--parent-lib names a library that has the each calls"


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


def timed_host(fn):
    """ms per call of a flow that synchronises by itself: the host clock around repetitions, a device synchronisation at both ends"""
    fn(); torch.cuda.synchronize()
    reps, total = 0, 0.0
    while total < MIN_MS:
        t0 = time.perf_counter()
        fn(); torch.cuda.synchronize()
        total += (time.perf_counter() - t0) * 1e3; reps += 1
    return total / reps


def _runtime():
    """the HIP runtime this process has loaded, for the three graph calls below"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    return C.CDLL("libamdhip64.so")


def kernel_nodes(fn):
    """the nodes of fn captured into a graph on a stream of its own (fn: kernel launches only, so a node is a launch); None where that fails"""
    try:
        rt = _runtime()
        s = torch.cuda.Stream()
        graph, count = C.c_void_p(), C.c_size_t(0)
        with torch.cuda.stream(s):
            fn(); s.synchronize()                               # (allocations and first-use work outside the capture)
            assert rt.hipStreamBeginCapture(C.c_void_p(s.cuda_stream), C.c_int(2)) == 0          # hipStreamCaptureModeRelaxed
            fn()
            assert rt.hipStreamEndCapture(C.c_void_p(s.cuda_stream), C.byref(graph)) == 0 and graph.value
        assert rt.hipGraphGetNodes(graph, None, C.byref(count)) == 0
        rt.hipGraphDestroy(graph)
        torch.cuda.synchronize()
        return int(count.value)
    except Exception as e:                                      # (a count is information, not a result)
        print(json.dumps(dict(what="launch count unavailable", error=repr(e)[:200])), flush=True)
        return None


n, tbytes = args.tensors, args.tensor_kib << 10
total = n * tbytes
gen = torch.Generator(device="cuda").manual_seed(1)
offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(tbytes)
soff = torch.from_numpy(offs.astype(np.int64)).cuda()
shape = "%d x %d KiB" % (n, args.tensor_kib)


def bf16(x):
    return x.to(torch.bfloat16).view(torch.uint8)


w = torch.randn(total // 2, generator=gen, device="cuda") * 0.02
src, base = bf16(w), bf16(w + torch.randn(total // 2, generator=gen, device="cuda") * 2e-5)


def report(what, ms, **more):
    gbps = total / ms / 1e6
    print(json.dumps(dict(shape=shape, what=what, GBps=round(gbps, 2), ms=round(ms, 3), **more)), flush=True)
    return gbps


# ---------------------------------------------------------------------------------------------------------------- (a) data kernels
if args.only in (None, "data"):
    planes, planes2, other, other2 = (torch.empty_like(src) for _ in range(4))
    copy = report("device copy (dst.copy_(src))", timed(lambda: other.copy_(src)))
    for E in (1, 2, 4, 8):
        poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); tres = torch.zeros(n, dtype=torch.int64, device="cuda")
        psz = torch.full((n * E,), tbytes // E, dtype=torch.int64, device="cuda"); mres = torch.zeros_like(tres)
        kw = dict(planes=planes, plane_offsets=poff, results=tres)
        ded_split = {"plain": lambda: parent.planes_split_dbatch(src, soff, E, **kw), "pred": lambda: parent.planes_split_pred_dbatch(src, soff, E, **kw),
                     "xor": lambda: parent.planes_split_xor_dbatch(src, base, soff, E, **kw), "sub": lambda: parent.planes_split_xor_dbatch(src, base, soff, E, delta_op=1, **kw)}
        mk = dict(dst=other, results=mres)
        ded_merge = {"plain": lambda: parent.planes_merge_dbatch(planes, poff, psz, soff, E, **mk), "pred": lambda: parent.planes_merge_pred_dbatch(planes, poff, psz, soff, E, **mk),
                     "xor": lambda: parent.planes_merge_xor_dbatch(planes, poff, psz, base, soff, E, **mk),
                     "sub": lambda: parent.planes_merge_xor_dbatch(planes, poff, psz, base, soff, E, delta_op=1, **mk)}
        rates = {"split": [], "merge": []}
        for c, name in enumerate(EST_NAMES):
            tr = torch.full((n,), c, dtype=torch.uint8, device="cuda")
            if E == 1 and name == "plain":                       # the dedicated call moves nothing: the planes are the tensor
                ds = copy
                planes.copy_(src)
            else:
                ds = report("dedicated split %s, E = %d (the parent's library)" % (name, E), timed(ded_split[name]))
            ms = timed(lambda: hip.planes_split_each_dbatch(src, soff, E, tr, base=base, planes=planes2, plane_offsets=poff, results=tres))
            assert bool((tres == tbytes).all()) and torch.equal(planes2, planes), (E, name)
            gb = total / ms / 1e6
            more = dict(vs_dedicated=round(gb / ds, 3))
            if E in (2, 4):
                more["bar"] = "%s %.1f of the dedicated split" % ("meets" if gb >= BAR * ds else "MISSES", BAR)
            report("split_each, uniform %s, E = %d" % (name, E), ms, **more)
            rates["split"].append(ds)
            other.zero_()
            dm = report("dedicated merge %s, E = %d (the parent's library)" % (name, E), timed(ded_merge[name]))
            assert bool((mres == tbytes).all()) and torch.equal(other, src)
            other2.zero_()
            ms = timed(lambda: hip.planes_merge_each_dbatch(planes, poff, psz, soff, E, tr, base=base, dst=other2, results=mres))
            assert bool((mres == tbytes).all()) and torch.equal(other2, src), (E, name)
            gb = total / ms / 1e6
            more = dict(vs_dedicated=round(gb / dm, 3))
            if E in (2, 4):
                more["bar"] = "%s %.1f of the dedicated merge" % ("meets" if gb >= BAR * dm else "MISSES", BAR)
            report("merge_each, uniform %s, E = %d" % (name, E), ms, **more)
            rates["merge"].append(dm)
        tr = (torch.arange(n, device="cuda") % 4).to(torch.uint8)   # the four in rotation: no single yardstick, the mean of the four
        ms = timed(lambda: hip.planes_split_each_dbatch(src, soff, E, tr, base=base, planes=planes2, plane_offsets=poff, results=tres))
        mean = sum(rates["split"]) / 4
        report("split_each, rotation, E = %d" % E, ms, vs_mean_of_dedicated=round(total / ms / 1e6 / mean, 3), mean_of_dedicated_GBps=round(mean, 2))
        other2.zero_()
        ms = timed(lambda: hip.planes_merge_each_dbatch(planes2, poff, psz, soff, E, tr, base=base, dst=other2, results=mres))
        assert bool((mres == tbytes).all()) and torch.equal(other2, src), (E, "rotation")
        mean = sum(rates["merge"]) / 4
        report("merge_each, rotation, E = %d" % E, ms, vs_mean_of_dedicated=round(total / ms / 1e6 / mean, 3), mean_of_dedicated_GBps=round(mean, 2))
    del planes, planes2, other, other2
    torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------------------- (b) the composite
if args.only in (None, "composite"):
    E = 2
    # the batch: tensor i from source i mod 3 -- a gaussian pair (base unrelated), an update pair, tensor == base
    kind = torch.arange(n, device="cuda") % 3
    unrelated = bf16(torch.randn(total // 2, generator=gen, device="cuda") * 0.02)
    rows = lambda t: t.view(n, tbytes)
    bmix = torch.where((kind == 0)[:, None], rows(unrelated), torch.where((kind == 1)[:, None], rows(base), rows(src))).reshape(-1).contiguous()
    del unrelated
    blocks = hip.planes_block_bound(total, n, E, BSID)
    first = hip.planes_segment_first([tbytes] * n, E, SEG_LOG)
    nf = int(first[-1])
    sfd = torch.from_numpy(first.astype(np.int64)).cuda()
    frames = torch.empty(hip.frame_packed_bound(total, nf, blocks, 0), dtype=torch.uint8, device="cuda")
    frames2 = torch.empty_like(frames)
    planes = torch.empty_like(src)
    foff, so = torch.zeros(nf + 1, dtype=torch.int64, device="cuda"), torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
    fres, tres, poff = torch.zeros(nf, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n * E + 1, dtype=torch.int64, device="cuda")
    chosen = torch.zeros(n, dtype=torch.uint8, device="cuda")
    hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize.restype = C.c_size_t
    wneed = int(hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize(C.c_size_t(nf), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(0)))
    ws = torch.empty(hip.tensor_each_workspace_head(n, E, True, 15) + wneed, dtype=torch.uint8, device="cuda")
    # the parent's flow: its outputs allocated once, like the composite's
    pb = torch.zeros(n * 4 * E, dtype=torch.int64, device="cuda"); eb = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
    ch = torch.zeros(n, dtype=torch.uint8, device="cuda"); eres = torch.zeros(n, dtype=torch.int64, device="cuda")
    ews = torch.empty(max(parent.planes_estimate_workspace_bound(n, E, 15), 1), dtype=torch.uint8, device="cuda")
    pws = torch.empty(wneed, dtype=torch.uint8, device="cuda")
    gathered, gbase = torch.empty_like(src), torch.empty_like(src)
    for mask, b in ((15, bmix), (3, None)):
        def each():
            hip.tensor_compress_seg_each_dbatch(src, soff, E, SEG_LOG, None, b, mask, 50, seg_first=sfd, n_segments=nf, block_size_id=BSID, dst=frames,
                                                max_total_blocks=blocks, frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff,
                                                seg_offsets=so, workspace=ws, chosen=chosen)
        state = {}

        def flow():
            """estimate, read-back, and per chosen part: gather its tensors (and bases) back to back, one segmented composite"""
            parent.planes_estimate_dbatch(src, soff, E, mask, 50, base=b, plane_bits=pb, est_bytes=eb, choice=ch, results=eres, workspace=ews)
            choice = ch.cpu().numpy()                           # the host read-back between the estimate and the compress
            for c, name in enumerate(EST_NAMES):
                idx = np.nonzero(choice == c)[0]
                if not len(idx):
                    continue
                m = len(idx)
                sel = torch.from_numpy(idx).cuda()
                sub = gathered[:m * tbytes]
                torch.index_select(rows(src), 0, sel, out=sub.view(m, tbytes))
                sb = None
                if c >= 2:
                    sb = gbase[:m * tbytes]
                    torch.index_select(rows(b), 0, sel, out=sb.view(m, tbytes))
                po = np.arange(m + 1, dtype=np.uint64) * np.uint64(tbytes)
                sf = first[:m * E + 1]
                k = dict(seg_first=sf, codec=0, block_size_id=BSID, dst=frames2, max_total_blocks=blocks, planes=planes, workspace=pws)
                if name == "pred":
                    _, fo, _, _, _ = parent.tensor_compress_seg_pred_dbatch(sub, po, E, SEG_LOG, **k)
                else:
                    _, fo, _, _, _ = parent.tensor_compress_seg_dbatch(sub, po, E, SEG_LOG, base=sb, delta_op=int(name == "sub"), **k)
                state.setdefault("ends", {})[name] = fo
                state.setdefault("parts", {})[name] = m
            return state
        each(); torch.cuda.synchronize()
        each_total = int(foff[-1].item())
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        picks = np.bincount(chosen.cpu().numpy(), minlength=4).tolist()
        flow(); torch.cuda.synchronize()
        flow_total = sum(int(fo[-1].item()) for fo in state["ends"].values())
        assert flow_total == each_total, (flow_total, each_total)      # the same frames, in one object or in parts
        assert {EST_NAMES[c]: picks[c] for c in range(4) if picks[c]} == state["parts"]
        each_ms, flow_ms, each_host_ms = timed(each), timed_host(flow), timed_host(each)
        nodes = kernel_nodes(each)
        # the parent's launches: the estimate, and per part one composite of its kind (captured with device arrays: launches only) and its gathers
        per = {"estimate": kernel_nodes(lambda: parent.planes_estimate_dbatch(src, soff, E, mask, 50, base=b, plane_bits=pb, est_bytes=eb, choice=ch, results=eres,
                                                                              workspace=ews))}
        dk = dict(seg_first=sfd, n_segments=nf, codec=0, block_size_id=BSID, dst=frames2, max_total_blocks=blocks, frame_offsets=foff, frame_results=fres,
                  tensor_results=tres, planes=planes, plane_offsets=poff, seg_offsets=so, workspace=pws)
        per["plain"] = kernel_nodes(lambda: parent.tensor_compress_seg_dbatch(src, soff, E, SEG_LOG, **dk))
        per["pred"] = kernel_nodes(lambda: parent.tensor_compress_seg_pred_dbatch(src, soff, E, SEG_LOG, **dk))
        if b is not None:
            per["xor"] = kernel_nodes(lambda: parent.tensor_compress_seg_dbatch(src, soff, E, SEG_LOG, base=b, delta_op=0, **dk))
            per["sub"] = kernel_nodes(lambda: parent.tensor_compress_seg_dbatch(src, soff, E, SEG_LOG, base=b, delta_op=1, **dk))
        flow_launches = None
        if all(v is not None for v in per.values()):
            flow_launches = per["estimate"] + sum(per[name] + (2 if name in ("xor", "sub") else 1) for name in state["parts"])
        what = "with a base, mask 15" if b is not None else "without a base, mask 3"
        report("segmented CHOOSE composite, %s" % what, each_ms, host_clock_ms=round(each_host_ms, 3), frame_bytes=each_total, chosen={EST_NAMES[c]: picks[c] for c in range(4) if picks[c]},
               kernel_launches=nodes, host_reads=0)
        report("the parent's flow (estimate, read-back, one gather and one composite per part), %s" % what, flow_ms, frame_bytes=flow_total, parts=len(state["parts"]),
               kernel_launches=flow_launches, launches_per_call=per, host_reads=1, each_over_flow=round(each_host_ms / flow_ms, 3),
               verdict="not slower than the parent's flow" if each_host_ms <= flow_ms else "SLOWER than the parent's flow")

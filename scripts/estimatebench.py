"""development aid: FSEHIP_planes_estimate_dbatch (one read of the tensors -> per tensor and candidate transform an estimated size and a
choice) next to what it replaces and what it is measured against, on bf16 bytes generated on the device, at 1024 tensors of 1 MiB and at one
tensor of 1 GiB, three sources each: a gaussian pair (tensor and base unrelated), an update pair (base = tensor + N(0, 2e-5)), and
tensor == base (every delta plane all zeros: the hot bin):
  (a) FSEHIP_planes_split_dbatch on the same bytes -- the yardstick for a kernel that reads the tensor once (it also writes it once);
      --parent-lib PATH: that of the library at PATH (the parent commit's build) loaded beside this tree's
  (b) the estimate with PLAIN | PRED (no base is read) and with all four candidates (the base is read too); "vs_split" = its time over (a)'s
  (c) the compress calls an exhaustive try would make, one per candidate (the segmented composites at segment_log 18, FSE): their frame
      bytes next to the estimates, "exhaustive" = the sum of their times, "estimate_then_one" = the estimate plus the one chosen compress,
      "verdict" = whether that is less
  (d) "zeros vs gaussian": the estimate's time on tensor == base over its time on the gaussian pair, all four candidates
--only-estimate: (b) and (d) alone (the A/B of differently configured builds through FSEHIP_LIB).
Then, once, on the four corpora of the header's table (tests/planes_estimate_corpus.py): the estimate of every candidate next to the real
frame bytes under FSE and Huff0 -- information, not a threshold.
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  GB/s =
tensor bytes / time.  Prints one JSON line per figure.
Usage: estimatebench.py [--shapes 1024x1024,1x1048576] [--parent-lib PATH] [--only-estimate] [--no-accuracy]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd import _lib
from finitestateentropy_amd.api import EST_NAMES, DeltaBase, FseHip, PredictedPlanes

MIN_MS = 200.0
E, SEG_LOG = 2, 18
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="1024x1024,1x1048576", help="tensors x KiB, comma separated")
ap.add_argument("--parent-lib", default=None); ap.add_argument("--only-estimate", action="store_true"); ap.add_argument("--no-accuracy", action="store_true")
args = ap.parse_args()
hip = FseHip()
split_hip, split_of = hip, "this tree"
if args.parent_lib:                                            # a second binding over the other library: its split is the yardstick
    _lib._LIB = C.CDLL(os.path.abspath(args.parent_lib))
    split_hip, split_of = FseHip(), "the parent's library"
    _lib._LIB = hip.lib
    assert not hasattr(split_hip.lib, "FSEHIP_planes_estimate_dbatch"), "--parent-lib names a library that has the estimate call"


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


def bf16(x):
    return x.to(torch.bfloat16).view(torch.uint8)


for shape in args.shapes.split(","):
    n, kib = (int(v) for v in shape.split("x"))
    tbytes = kib << 10
    total = n * tbytes
    gen = torch.Generator(device="cuda").manual_seed(1)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(tbytes)
    soff = torch.from_numpy(offs.astype(np.int64)).cuda()
    w = torch.randn(total // 2, generator=gen, device="cuda") * 0.02
    src = bf16(w)
    bases = {"gaussian pair": bf16(torch.randn(total // 2, generator=gen, device="cuda") * 0.02),
             "update pair": bf16(w + torch.randn(total // 2, generator=gen, device="cuda") * 2e-5), "tensor == base": src.clone()}
    del w
    pb = torch.zeros(n * 4 * E, dtype=torch.int64, device="cuda"); eb = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
    ch = torch.zeros(n, dtype=torch.uint8, device="cuda"); res = torch.zeros(n, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(hip.planes_estimate_workspace_bound(n, E, 15), 1), dtype=torch.uint8, device="cuda")
    planes = torch.empty_like(src)
    poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); tres = torch.zeros(n, dtype=torch.int64, device="cuda")

    def report(source, what, ms, **more):
        print(json.dumps(dict(shape="%d x %d KiB" % (n, kib), source=source, what=what, GBps=round(total / ms / 1e6, 2), ms=round(ms, 3), **more)), flush=True)
        return ms
    split_ms = report("-", "planes split, E = %d (%s)" % (E, split_of), timed(lambda: split_hip.planes_split_dbatch(src, soff, E, planes=planes, plane_offsets=poff, results=tres)))
    all_four = {}
    for source, base in bases.items():
        est = {}
        for mask, given in ((3, None), (15, base)):
            ms = timed(lambda: hip.planes_estimate_dbatch(src, soff, E, mask, 50, base=given, plane_bits=pb, est_bytes=eb, choice=ch, results=res, workspace=ws))
            assert bool((res == tbytes).all())
            sums = eb.view(n, 4).sum(0).cpu().tolist()
            picks = np.bincount(ch.cpu().numpy(), minlength=4).tolist()
            est[mask] = (ms, {EST_NAMES[c]: sums[c] for c in range(4) if (mask >> c) & 1}, {EST_NAMES[c]: picks[c] for c in range(4) if picks[c]})
            report(source, "estimate, mask %d" % mask, ms, vs_split=round(ms / split_ms, 3), estimates=est[mask][1], chosen=est[mask][2])
        all_four[source] = est[15][0]
        if args.only_estimate:
            continue
        blocks = hip.planes_block_bound(total, n, E, 5)
        first = hip.planes_segment_first([tbytes] * n, E, SEG_LOG)
        frames = torch.empty(hip.frame_packed_bound(total, int(first[-1]), blocks, 0), dtype=torch.uint8, device="cuda")
        kw = dict(seg_first=first, codec=0, dst=frames, max_total_blocks=blocks, planes=planes)
        calls = {"plain": lambda: hip.tensor_compress_seg_dbatch(src, offs, E, SEG_LOG, **kw),
                 "pred": lambda: hip.tensor_compress_seg_pred_dbatch(src, offs, E, SEG_LOG, **kw),
                 "xor": lambda: hip.tensor_compress_seg_dbatch(src, offs, E, SEG_LOG, base=base, delta_op=0, **kw),
                 "sub": lambda: hip.tensor_compress_seg_dbatch(src, offs, E, SEG_LOG, base=base, delta_op=1, **kw)}
        times, sizes = {}, {}
        for name, call in calls.items():
            times[name] = timed(call)
            _, foff, fres, _, _ = call()
            assert bool((fres > 0).all())
            sizes[name] = int(foff[-1].item())
            report(source, "tensor_compress_seg, %s" % name, times[name], frame_bytes=sizes[name])
        for mask, names in ((3, EST_NAMES[:2]), (15, EST_NAMES)):
            ms, sums, picks = est[mask]
            chosen = max(picks, key=picks.get)
            exhaustive, one = sum(times[k] for k in names), ms + times[chosen]
            report(source, "mask %d: exhaustive %s against estimate + %s" % (mask, "+".join(names), chosen), one, exhaustive_ms=round(exhaustive, 3),
                   estimate_then_one_ms=round(one, 3), verdict="less" if one < exhaustive else "NOT LESS", smallest_real=min(names, key=lambda k: sizes[k]),
                   estimates=sums, frame_bytes={k: sizes[k] for k in names})
        del frames
    ratio = all_four["tensor == base"] / all_four["gaussian pair"]
    print(json.dumps(dict(shape="%d x %d KiB" % (n, kib), what="zeros vs gaussian: estimate, mask 15, time on tensor == base over time on the gaussian pair", ratio=round(ratio, 3))),
          flush=True)
    del src, bases, planes, ws
    torch.cuda.empty_cache()

if not args.no_accuracy:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import planes_estimate_corpus as pe

    def dev(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda().view(dt)
    t, b = pe.update_pair()
    corpora = {"bf16 gaussian, 256 KiB": (dev(pe.bf16_gaussian(), torch.bfloat16), None), "sorted int64 below 2^40, 256 KiB": (dev(pe.sorted_int64(), torch.int64), None),
               "position ids arange % 4096 as u32, 128 KiB": (dev(pe.position_ids(), torch.int32), None),
               "bf16_update_pair(1 << 17)": (dev(t, torch.bfloat16), dev(b, torch.bfloat16))}
    for name, (x, base) in corpora.items():
        (rec,) = hip.estimate_tensors([x], base=None if base is None else [base])
        real = {}
        for codec, cname in ((0, "fse"), (1, "huf")):
            real[cname] = {"plain": hip.compress_tensors([x], codec).nbytes, "pred": hip.compress_tensors([x], PredictedPlanes(codec)).nbytes}
            if base is not None:
                real[cname]["xor"] = hip.compress_tensors([x], codec, base=[base]).nbytes
                real[cname]["sub"] = hip.compress_tensors([x], codec, base=DeltaBase([base], "sub")).nbytes
        print(json.dumps(dict(corpus=name, what="estimated bytes against real frame bytes", estimates=rec["estimates"], choice=rec["choice"], frame_bytes=real)), flush=True)

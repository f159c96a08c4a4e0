"""development aid: segmented planes (FSEHIP_tensor_compress_seg_dbatch / _decompress_seg_dbatch) next to the unsegmented tensor calls
(FSEHIP_tensor_compress_dbatch / _decompress_dbatch) on the same bytes -- 1 GiB of bf16 data, N(0, 0.02) generated on the device, cut into
  (a) 1024 tensors of 1 MiB      (b) 8 tensors of 128 MiB      (c) one tensor of 1 GiB
each unsegmented and with segment_log 18, 20 and 22, per codec, compress and decompress.  Device events around the calls, repeated until the
timed region is at least MIN_MS long, after one warm-up call of the same shape; the unsegmented calls of (b) and (c) get ONE timed repetition
(they take hundreds of milliseconds: one frame is one checksum chain).  GB/s = content bytes / time.  One JSON line per figure, then the
comparisons the table in DESIGN.md 4.4d is read by.  Usage: segbench.py [--total-mib 1024] [--block-size-id 5]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import FseHip

MIN_MS = 200.0
ap = argparse.ArgumentParser()
ap.add_argument("--total-mib", type=int, default=1024); ap.add_argument("--block-size-id", type=int, default=5)
args = ap.parse_args()
hip = FseHip()
BSID, E = args.block_size_id, 2
SEG_LOGS = (18, 20, 22)


def timed(fn, once=False):
    """ms per call: one warm-up, then repeated until MIN_MS have passed between the two events (once: a single repetition)"""
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
        if once:
            break
    return total / reps


def ws(fn, *a):
    fn.restype = C.c_size_t
    return torch.empty(max(int(fn(*a)), 1), dtype=torch.uint8, device="cuda")


def i64(n):
    return torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")[:n]


total = args.total_mib << 20
gen = torch.Generator(device="cuda").manual_seed(1)
src = (torch.randn(total // 2, generator=gen, device="cuda") * 0.02).to(torch.bfloat16).view(torch.uint8)
planes, other = torch.empty_like(src), torch.empty_like(src)
L = hip.lib
figures = {}

for shape, n in (("a", 1024), ("b", 8), ("c", 1)):
    tbytes = total // n
    name = "%d x %d MiB bf16" % (n, tbytes >> 20)
    soff_h = np.arange(n + 1, dtype=np.int64) * tbytes
    soff = torch.from_numpy(soff_h).cuda()
    blocks = hip.planes_block_bound(total, n, E, BSID)
    tres, mres, poff = i64(n), i64(n), i64(n * E + 1)
    for codec, cname in ((0, "fse"), (1, "huf")):
        for seg_log in (None,) + SEG_LOGS:
            first = None if seg_log is None else hip.planes_segment_first([tbytes] * n, E, seg_log)
            nfr = n * E if seg_log is None else int(first[-1])
            sf = None if first is None else torch.from_numpy(first.astype(np.int64)).cuda()
            frames = torch.empty(hip.frame_packed_bound(total, nfr, blocks, 0), dtype=torch.uint8, device="cuda")
            foff, fres, so = i64(nfr + 1), i64(nfr), i64(nfr + 1)
            kws = ws(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize, C.c_size_t(nfr), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(codec))
            once = seg_log is None and shape != "a"
            if seg_log is None:
                w = timed(lambda: hip.tensor_compress_dbatch(src, soff, E, BSID, codec, dst=frames, max_total_blocks=blocks, frame_offsets=foff, frame_results=fres,
                                                             tensor_results=tres, planes=planes, plane_offsets=poff, workspace=kws), once)
            else:
                w = timed(lambda: hip.tensor_compress_seg_dbatch(src, soff, E, seg_log, sf, n_segments=nfr, codec=codec, block_size_id=BSID, dst=frames,
                                                                 max_total_blocks=blocks, frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes,
                                                                 plane_offsets=poff, seg_offsets=so, workspace=kws))
            assert bool((fres > 0).all()) and bool((tres == tbytes).all())
            fbytes = int(foff[nfr].item())
            del kws
            dws = ws(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize, C.c_size_t(nfr), C.c_size_t(blocks))
            so2, sres, poff2, psz = i64(nfr + 1), i64(nfr), i64(n * E + 1), i64(n * E)
            other.zero_()
            if seg_log is None:
                r = timed(lambda: hip.tensor_decompress_dbatch(frames, foff, soff, E, dst=other, max_total_blocks=blocks, planes=planes, plane_offsets=poff2,
                                                               plane_results=psz, workspace=dws, results=mres), once)
            else:
                r = timed(lambda: hip.tensor_decompress_seg_dbatch(frames, foff, soff, E, seg_log, sf, n_segments=nfr, dst=other, max_total_blocks=blocks, planes=planes,
                                                                   seg_offsets=so2, seg_results=sres, plane_offsets=poff2[:n * E], plane_sizes=psz, workspace=dws,
                                                                   results=mres))
            assert bool((mres == tbytes).all()) and torch.equal(other, src)
            figures[(shape, cname, seg_log)] = (total / w / 1e6, total / r / 1e6, fbytes, nfr)
            print(json.dumps(dict(shape=name, codec=cname, segment_log=seg_log, frames=nfr, frame_bytes=fbytes, ratio=round(fbytes / total, 4),
                                  compress_GBps=round(total / w / 1e6, 2), compress_ms=round(w, 3), decompress_GBps=round(total / r / 1e6, 2), decompress_ms=round(r, 3),
                                  timed_once=once)), flush=True)
            del dws, frames
            torch.cuda.empty_cache()

# the comparisons: sizes differ by exactly 8 bytes per additional frame; (a) at 20 within 3 % of unsegmented; (b), (c) at 20 at least half of (a) unsegmented
for (shape, cname, seg_log), (w, r, fbytes, nfr) in figures.items():
    if seg_log is None:
        continue
    uw, ur, ubytes, unfr = figures[(shape, cname, None)]
    aw, ar = figures[("a", cname, None)][:2]
    print(json.dumps(dict(check=shape, codec=cname, segment_log=seg_log, size_is_unsegmented_plus_8_per_frame=fbytes == ubytes + 8 * (nfr - unfr),
                          compress_vs_unsegmented=round(w / uw, 3), decompress_vs_unsegmented=round(r / ur, 3),
                          compress_vs_a_unsegmented=round(w / aw, 3), decompress_vs_a_unsegmented=round(r / ar, 3))), flush=True)

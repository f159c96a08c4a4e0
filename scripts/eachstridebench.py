"""development aid: a stride per tensor and strides in the estimate (FSEHIP_planes_split_each_stride_dbatch / _merge_each_stride_dbatch,
FSEHIP_tensor_compress_each_stride_dbatch with CHOOSE, FSEHIP_planes_estimate_stride_dbatch) next to the PARENT commit's dedicated calls, at
1024 tensors of 1 MiB, the workload and the protocol of stridebench.py, on its two interleaved sources generated on the device (int16 stereo,
float32 xyz).  --parent-lib PATH (required): the parent commit's build of the library, loaded beside this tree's in the same process; every
yardstick figure is that library's on the same bytes.
  (A) per element size 2 and 4: the parent's FSEHIP_planes_split_pred_stride_dbatch / _merge_ at S = 2, 3, 4, then the each-stride split and
      merge with every tensor PRED at that stride, then with the batch cycling PLAIN / PRED S = 2 / PRED S = 3 (against the slower of the
      parent's S = 2 and S = 3); "vs_parent" = GB/s over the parent's, "bar" = whether that reaches 0.5 (bar A)
  (B) per source (stereo: 2-byte elements; xyz: 4-byte elements): what a caller does today to find the stride -- the parent's
      FSEHIP_tensor_compress_pred_stride_dbatch at S = 1, 2, 3, 4 and its plain FSEHIP_tensor_compress_dbatch, five frame totals -- then ONE
      FSEHIP_tensor_compress_each_stride_dbatch with CHOOSE over PLAIN | PRED and the strides {1, 2, 3, 4}; "bar" = its time below the sum of the
      five, and its frame total the smallest of the five.  Then the estimate alone: FSEHIP_planes_estimate_stride_dbatch over the four
      strides beside the parent's FSEHIP_planes_estimate_dbatch with PLAIN | PRED.
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  GB/s =
content bytes / time.  Prints one JSON line per figure.
Usage: eachstridebench.py --parent-lib PATH [--tensors 1024] [--tensor-kib 1024] [--block-size-id 5]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd import _lib
from finitestateentropy_amd.api import FseHip

MIN_MS = 300.0
BAR = 0.5
PLAIN, PRED = 0, 1
ap = argparse.ArgumentParser()
ap.add_argument("--tensors", type=int, default=1024); ap.add_argument("--tensor-kib", type=int, default=1024); ap.add_argument("--block-size-id", type=int, default=5)
ap.add_argument("--parent-lib", required=True)
args = ap.parse_args()
hip = FseHip()
_lib._LIB = C.CDLL(os.path.abspath(args.parent_lib))           # a second binding over the other library
old = FseHip()
_lib._LIB = hip.lib
assert not hasattr(old.lib, "FSEHIP_planes_split_each_stride_dbatch"), "--parent-lib names a library that has the each-stride calls"
BSID = args.block_size_id


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


n, tbytes = args.tensors, args.tensor_kib << 10
total = n * tbytes
gen = torch.Generator(device="cuda").manual_seed(1)
soff = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * tbytes)).cuda()


def walks(count, channels, lo, hi, dtype):
    """`count` elements: `channels` interleaved random walks with steps in [lo, hi), in slices to bound the int64 scratch (stridebench.py's)"""
    out = torch.empty(count, dtype=dtype, device="cuda")
    rows, at, last = 1 << 24, 0, torch.zeros((1, channels), dtype=torch.int64, device="cuda")
    while at < count:
        m = min(rows * channels, count - at)
        w = torch.cumsum(torch.randint(lo, hi, (-(-m // channels), channels), generator=gen, device="cuda", dtype=torch.int64), 0) + last
        last = w[-1:].clone()
        out[at:at + m] = w.reshape(-1)[:m].to(dtype)
        at += m
    return out


def sources():
    yield "int16 stereo", 2, 2, walks(total // 2, 2, -40, 41, torch.int16).view(torch.uint8)
    steps = walks(total // 4, 3, -1000, 1001, torch.int32)      # the walk in units of 1e-7 around 100.0 / -37.0 / 5.5
    base = torch.tensor([100.0, -37.0, 5.5], device="cuda", dtype=torch.float64).repeat(-(-(total // 4) // 3))[:total // 4]
    yield "float32 xyz", 4, 3, (base + steps.to(torch.float64) * 1e-7).to(torch.float32).view(torch.uint8)


def u8(values):
    return torch.tensor(values, dtype=torch.uint8).cuda()


for source, E, channels, src in sources():
    def report(what, ms, **more):
        gbps = total / ms / 1e6
        print(json.dumps(dict(shape="%d x %d KiB" % (n, args.tensor_kib), source=source, E=E, what=what, GBps=round(gbps, 2), ms=round(ms, 3), **more)), flush=True)
        return gbps

    def against(gbps, parent, what):
        return dict(vs_parent=round(gbps / parent, 3), bar="%s %.1f of the parent's %s" % ("meets" if gbps >= BAR * parent else "MISSES", BAR, what))
    other, planes = torch.empty_like(src), torch.empty_like(src)
    report("device copy (dst.copy_(src))", timed(lambda: other.copy_(src)))
    poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); tres = torch.zeros(n, dtype=torch.int64, device="cuda")
    psz = torch.full((n * E,), tbytes // E, dtype=torch.int64, device="cuda"); mres = torch.zeros_like(tres)
    # ---- (A) the data kernels
    parent = {}
    for S in (2, 3, 4):
        split = report("parent: planes split pred_stride, S = %d" % S, timed(lambda: old.planes_split_pred_stride_dbatch(src, soff, E, S, planes=planes, plane_offsets=poff, results=tres)))
        want = planes.clone()
        other.zero_()
        merge = report("parent: planes merge pred_stride, S = %d" % S, timed(lambda: old.planes_merge_pred_stride_dbatch(planes, poff, psz, soff, E, S, dst=other, results=mres)))
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        parent[S] = (split, merge)
        tr, st = u8([PRED] * n), u8([S] * n)
        planes.zero_()
        ms = timed(lambda: hip.planes_split_each_stride_dbatch(src, soff, E, tr, st, planes=planes, plane_offsets=poff, results=tres))
        assert bool((tres == tbytes).all()) and torch.equal(planes, want), "the parent's planes, byte for byte"
        report("each-stride split, all PRED S = %d" % S, ms, **against(total / ms / 1e6, split, "split at that stride"))
        other.zero_()
        ms = timed(lambda: hip.planes_merge_each_stride_dbatch(planes, poff, psz, soff, E, tr, st, dst=other, results=mres))
        assert bool((mres == tbytes).all()) and torch.equal(other, src)
        report("each-stride merge, all PRED S = %d" % S, ms, **against(total / ms / 1e6, merge, "merge at that stride"))
    tr, st = u8([(PLAIN, PRED, PRED)[i % 3] for i in range(n)]), u8([(1, 2, 3)[i % 3] for i in range(n)])
    ms = timed(lambda: hip.planes_split_each_stride_dbatch(src, soff, E, tr, st, planes=planes, plane_offsets=poff, results=tres))
    report("each-stride split, cycling PLAIN / PRED S = 2 / PRED S = 3", ms, **against(total / ms / 1e6, min(parent[2][0], parent[3][0]), "slower split of S = 2, 3"))
    other.zero_()
    ms = timed(lambda: hip.planes_merge_each_stride_dbatch(planes, poff, psz, soff, E, tr, st, dst=other, results=mres))
    assert bool((mres == tbytes).all()) and torch.equal(other, src)
    report("each-stride merge, cycling PLAIN / PRED S = 2 / PRED S = 3", ms, **against(total / ms / 1e6, min(parent[2][1], parent[3][1]), "slower merge of S = 2, 3"))
    # ---- (B) the estimate pays
    blocks = hip.planes_block_bound(total, n, E, BSID)
    L = hip.lib
    kws = ws(L.FSEHIP_frame_compress_packed_dbatch_workspaceSize, C.c_size_t(n * E), C.c_size_t(blocks), C.c_uint(BSID), C.c_int(0))
    frames = torch.empty(hip.frame_packed_bound(total, n * E, blocks, 0), dtype=torch.uint8, device="cuda")
    foff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda"); fres = torch.zeros(n * E, dtype=torch.int64, device="cuda")
    wkw = dict(dst=frames, max_total_blocks=blocks, frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, workspace=kws)
    today, sizes = 0.0, {}
    rows = [("plain", lambda: old.tensor_compress_dbatch(src, soff, E, BSID, 0, **wkw))]
    rows += [(S, (lambda S: lambda: old.tensor_compress_pred_stride_dbatch(src, soff, E, S, codec=0, block_size_id=BSID, **wkw))(S)) for S in (1, 2, 3, 4)]
    for key, write in rows:
        ms = timed(write)
        sizes[key] = int(foff[n * E].item())
        assert bool((fres > 0).all()) and bool((tres == tbytes).all())
        today += ms
        report("parent: tensor_compress %s" % ("plain" if key == "plain" else "pred_stride, S = %d" % key), ms, frame_bytes=sizes[key], ratio=round(sizes[key] / total, 4))
    mask, smask = 3, 0x0F
    head = hip.tensor_each_stride_workspace_head(n, E, True, mask, smask)
    cws = torch.empty(head + kws.numel(), dtype=torch.uint8, device="cuda")
    chosen, strides = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    ckw = dict(wkw, workspace=cws, chosen=chosen, chosen_strides=strides)
    ms = timed(lambda: hip.tensor_compress_each_stride_dbatch(src, soff, E, None, None, None, mask, smask, 50, codec=0, block_size_id=BSID, **ckw))
    nbytes = int(foff[n * E].item())
    assert bool((fres > 0).all()) and bool((tres == tbytes).all())
    tr_set, st_set = sorted(set(chosen.cpu().tolist())), sorted(set(strides.cpu().tolist()))
    best = min(sizes, key=sizes.get)
    ok = ms < today and nbytes == sizes[best] and tr_set == [PRED] and st_set == [channels]
    report("each-stride compress, CHOOSE over PLAIN | PRED and strides 1 .. 4", ms, frame_bytes=nbytes, ratio=round(nbytes / total, 4), chosen_transforms=tr_set,
           chosen_strides=st_set, today_ms=round(today, 3), vs_today=round(ms / today, 3), smallest_of_five=str(best),
           bar="%s: less time than the five calls of today, and their smallest frame total" % ("meets" if ok else "MISSES"))
    ews = torch.empty(hip.planes_estimate_stride_workspace_bound(n, E, mask, smask), dtype=torch.uint8, device="cuda")
    pb, eb, res = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (n * 4 * E, n * 4, n))
    seb, ch = torch.zeros(n * 8, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    old_ms = timed(lambda: old.planes_estimate_dbatch(src, soff, E, mask, 50, plane_bits=pb, est_bytes=eb, choice=ch, results=res, workspace=ews))
    report("parent: planes_estimate, PLAIN | PRED", old_ms)
    for sm, name in ((1, "stride 1"), (smask, "strides 1 .. 4"), (0xFF, "strides 1 .. 8")):
        ews = torch.empty(hip.planes_estimate_stride_workspace_bound(n, E, mask, sm), dtype=torch.uint8, device="cuda")
        ms = timed(lambda: hip.planes_estimate_stride_dbatch(src, soff, E, mask, sm, 50, plane_bits=pb, est_bytes=eb, choice=ch, results=res, stride_est_bytes=seb,
                                                             strides=strides, workspace=ews))
        report("planes_estimate_stride, PLAIN | PRED, " + name, ms, over_parent_estimate=round(ms / old_ms, 3), lds_kib=8 * bin(sm).count("1"),
               strides_found=sorted(set(strides.cpu().tolist())))
    del src, other, planes, frames, kws, cws, ews
    torch.cuda.empty_cache()

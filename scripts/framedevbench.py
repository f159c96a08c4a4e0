"""development aid: .fse frames written and read on DEVICE buffers (FSEHIP_frame_compress_dbatch / _decompress_dbatch, FSEHIP_XXH32_batch)
next to the host-buffer batch calls (FSEHIP_frame_compress_batch / _decompress_batch, pinned host memory, 4 threads) on the same contents.
  (a) 1024 frames of 1 MiB   (b) one frame of 256 MiB   (c) the checksum kernel alone on both shapes      P14, block-size id 5, both codecs
  (d) 100k frames of 4 KB, device calls only
The writer runs in both forms: fixed slots of FSEHIP_frame_compressBound each (offsets in) and packed (FSEHIP_frame_compress_packed_dbatch,
offsets out) -- "extra_ms" is the packed call minus the fixed-slot call of the same run.
On every shape the frames are also read as frames of UNKNOWN size: the plan alone (FSEHIP_frame_plan_dbatch: header walk, two scans, clamp)
and the packed call (FSEHIP_frame_decompress_packed_dbatch) beside the known-offset call on the same frames -- "extra_ms" is the packed call
minus the known-offset call of the same run.
Device calls: device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same
shape.  GB/s = content bytes / time.  Prints one JSON line per figure.  Usage: framedevbench.py [--frames 1024] [--frame-mib 1] [--big-mib 256]
[--small-frames 100000] [--small-kib 4] [--no-host]"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import FseHip

MIN_MS = 300.0
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1024); ap.add_argument("--frame-mib", type=int, default=1); ap.add_argument("--big-mib", type=int, default=256)
ap.add_argument("--small-frames", type=int, default=100000); ap.add_argument("--small-kib", type=int, default=4)
ap.add_argument("--no-host", action="store_true")
args = ap.parse_args()
hip = FseHip()
BSID = 5


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


def report(shape, what, codec, nbytes, ms, **more):
    print(json.dumps(dict(shape=shape, what=what, codec=codec, GBps=round(nbytes / ms / 1e6, 2), ms=round(ms, 3), **more)), flush=True)


def device_side(shape, n_frames, frame_bytes):
    total = n_frames * frame_bytes
    src = hip.probagen_batch(14, total // 32768, 32768, first_seed=1).reshape(-1)
    sizes = [frame_bytes] * n_frames
    soff = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).cuda()
    foff_h = hip.frame_dbatch_plan(sizes, BSID)
    foff = torch.from_numpy(foff_h.astype(np.int64)).cuda()
    nblk = sum(hip.frame_block_count(n, BSID) for n in sizes)
    frames = torch.empty(int(foff_h[-1]), dtype=torch.uint8, device="cuda"); back = torch.empty(total, dtype=torch.uint8, device="cuda")
    cres = torch.zeros(n_frames, dtype=torch.int64, device="cuda"); dres = torch.zeros_like(cres)
    h = torch.zeros(n_frames, dtype=torch.int32, device="cuda")
    ms = timed(lambda: hip.lib.FSEHIP_XXH32_batch(C.c_void_p(h.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(soff.data_ptr()), C.c_size_t(n_frames), C.c_uint32(0),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    report(shape, "xxh32", "-", total, ms, GBps_per_item=round(frame_bytes / ms / 1e6, 3))
    for codec, name in ((0, "fse"), (1, "huf")):
        cws = hip.frame_dbatch_workspace(n_frames, nblk, BSID, codec)
        w = lambda: hip.frame_compress_dbatch(src, soff, BSID, codec, dst=frames, dst_offsets=foff, max_total_blocks=nblk, workspace=cws, results=cres)
        fixed = timed(w)
        report(shape, "device write", name, total, fixed, frame_bytes=int(cres.sum().item()))
        # the packed writer on the same contents: frames back to back, offsets from the device -- "extra_ms" = packed minus fixed-slot, same run
        hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize.restype = C.c_size_t
        kws = torch.empty(int(hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize(C.c_size_t(n_frames), C.c_size_t(nblk), C.c_uint(BSID), C.c_int(codec))),
                          dtype=torch.uint8, device="cuda")
        kframes = torch.empty(hip.frame_packed_bound(total, n_frames, nblk, 0), dtype=torch.uint8, device="cuda")
        koff = torch.zeros(n_frames + 1, dtype=torch.int64, device="cuda"); kres = torch.zeros_like(cres)
        k = lambda: hip.frame_compress_packed_dbatch(src, soff, BSID, codec, dst=kframes, max_total_blocks=nblk, dst_offsets=koff, workspace=kws, results=kres)
        tight = timed(k)
        report(shape, "device write, packed (offsets out)", name, total, tight, frame_bytes=int(koff[-1].item()), extra_ms=round(tight - fixed, 3))
        assert torch.equal(kres, cres) and int(koff[-1].item()) == int(cres.sum().item())
        del kws, kframes
        # the reader is handed the frames packed back to back, as a file or a message would hold them
        sz = cres.cpu().numpy()
        assert (sz > 0).all()
        poff_h = np.concatenate([[0], np.cumsum(sz)]).astype(np.int64)
        packed = torch.cat([frames[int(foff_h[i]):int(foff_h[i]) + int(sz[i])] for i in range(n_frames)])
        poff = torch.from_numpy(poff_h).cuda()
        dws = hip.frame_dbatch_workspace(n_frames, nblk)
        r = lambda: hip.frame_decompress_dbatch(packed, poff, soff, dst=back, max_total_blocks=nblk, workspace=dws, results=dres)
        known = timed(r)
        report(shape, "device read", name, total, known)
        assert bool((dres == frame_bytes).all()) and torch.equal(back, src)
        # the same frames as frames of unknown size: exact promise, exact capacity (what a sizing query returns)
        pws = torch.empty(int(hip.lib.FSEHIP_frame_plan_dbatch_workspaceSize(C.c_size_t(n_frames))), dtype=torch.uint8, device="cuda")
        pd = torch.zeros(n_frames + 1, dtype=torch.int64, device="cuda"); pb = torch.zeros_like(pd)
        plan = timed(lambda: hip.frame_plan_dbatch(packed, poff, None, 0, dst_offsets=pd, block_first=pb, workspace=pws))
        assert torch.equal(pd, soff) and int(pb[-1].item()) == nblk
        report(shape, "device plan (header walk, scans)", name, total, plan)
        dres.zero_(); back.zero_(); pd.zero_()
        u = lambda: hip.frame_decompress_packed_dbatch(packed, poff, dst=back, capacity=total, max_total_blocks=nblk, dst_offsets=pd, workspace=dws, results=dres)
        unknown = timed(u)
        report(shape, "device read, sizes unknown (packed call)", name, total, unknown, extra_ms=round(unknown - known, 3), plan_ms=round(plan, 3))
        assert bool((dres == frame_bytes).all()) and torch.equal(back, src) and torch.equal(pd, soff)
        del pws
        del cws, dws, packed
    return src


def host_side(shape, src, n_frames, frame_bytes, threads=4):
    total = n_frames * frame_bytes
    pin = torch.empty(total, dtype=torch.uint8, pin_memory=True); pin.copy_(src); torch.cuda.synchronize()
    bound = int(hip.lib.FSEHIP_frame_compressBound(C.c_size_t(frame_bytes), C.c_uint(BSID)))
    outs = torch.empty(n_frames * bound, dtype=torch.uint8, pin_memory=True); backs = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    outs.zero_(); backs.zero_()                              # touched before the timed calls
    PA, SA = C.c_void_p * n_frames, C.c_size_t * n_frames
    fc, fd = hip.lib.FSEHIP_frame_compress_batch, hip.lib.FSEHIP_frame_decompress_batch
    fc.restype = fd.restype = C.c_size_t
    for codec, name in ((0, "fse"), (1, "huf")):
        res, res2 = SA(), SA()
        args_c = (PA(*[outs.data_ptr() + i * bound for i in range(n_frames)]), SA(*[bound] * n_frames), PA(*[pin.data_ptr() + i * frame_bytes for i in range(n_frames)]),
                  SA(*[frame_bytes] * n_frames), res, C.c_size_t(n_frames), C.c_uint(BSID), C.c_int(codec), C.c_uint(threads))

        def wall(f, a):
            assert f(*a) == 0                                # warm-up: the workers' arenas and streams
            reps, t0 = 0, time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < MIN_MS:
                assert f(*a) == 0; reps += 1
            return (time.perf_counter() - t0) * 1e3 / reps
        report(shape, "host batch write (pinned, %d threads)" % threads, name, total, wall(fc, args_c))
        args_d = (PA(*[backs.data_ptr() + i * frame_bytes for i in range(n_frames)]), SA(*[frame_bytes] * n_frames), PA(*[outs.data_ptr() + i * bound for i in range(n_frames)]),
                  SA(*[int(res[i]) for i in range(n_frames)]), res2, C.c_size_t(n_frames), C.c_uint(threads))
        report(shape, "host batch read (pinned, %d threads)" % threads, name, total, wall(fd, args_d))
        assert all(int(res2[i]) == frame_bytes for i in range(n_frames)) and torch.equal(backs, pin)


hip.lib.FSEHIP_frame_plan_dbatch_workspaceSize.restype = C.c_size_t
for shape, n_frames, frame_bytes, host in (("a: %d x %d MiB" % (args.frames, args.frame_mib), args.frames, args.frame_mib << 20, True),
                                           ("b: 1 x %d MiB" % args.big_mib, 1, args.big_mib << 20, True),
                                           ("d: %d x %d KiB" % (args.small_frames, args.small_kib), args.small_frames, args.small_kib << 10, False)):
    if n_frames == 0:
        continue
    src = device_side(shape, n_frames, frame_bytes)
    if host and not args.no_host:
        host_side(shape, src, n_frames, frame_bytes)
    del src
    torch.cuda.empty_cache()

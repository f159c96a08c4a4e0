"""development aid: the tensor digest and the gate (FSEHIP_tensor_digest_dbatch, FSEHIP_tensor_gate_dbatch) next to the kernels they are
measured against, on the workload of deltabench.py -- a bf16 weight update generated on the device, the base N(0, 0.02), the new tensors
base + N(0, 2e-5) added in float32, both cut to bf16 -- as `--tensors` tensors of `--tensor-kib` KiB (1024 x 1 MiB; 1 x 1 GiB):
  (a) the digest of the base tensors; the plain planes split and a device copy over the same bytes in the same run: "vs_split" = the split's
      time over the digest's (above 1: the digest is faster; the expectation is >= 1, it reads n bytes where the split moves 2 n)
  (b) for a single tensor the top level alone: the XXH32 chain over its 8 nt + 8 bytes, which the digest call runs once per seed
  (c) the gate over the frame offsets of the segmented sparse FSE SUB delta frames (segment_log 18)
  (d) the in-place read of those frames over the resident base, unchecked and checked (digest, gate, read over the gated offsets), each
      with the copy that puts the base back in front of it -- in place the read consumes its base; "check_ms" = the difference
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call of the same shape.  GB/s =
content bytes (the tensors' bytes) / time.  Prints one JSON line per figure.
Usage: digestbench.py [--tensors 1024] [--tensor-kib 1024] [--block-size-id 5]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import FseHip

MIN_MS = 300.0
ap = argparse.ArgumentParser()
ap.add_argument("--tensors", type=int, default=1024); ap.add_argument("--tensor-kib", type=int, default=1024); ap.add_argument("--block-size-id", type=int, default=5)
args = ap.parse_args()
hip = FseHip()
BSID, E, SEG_LOG, PERMILLE = args.block_size_id, 2, 18, 500


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


def report(what, nbytes, ms, **more):
    print(json.dumps(dict(shape="%d x %d KiB bf16" % (args.tensors, args.tensor_kib), what=what, GBps=round(nbytes / ms / 1e6, 2), ms=round(ms, 4), **more)), flush=True)


n, tbytes = args.tensors, args.tensor_kib << 10
total = n * tbytes
gen = torch.Generator(device="cuda").manual_seed(1)
w = torch.randn(total // 2, generator=gen, device="cuda") * 0.02
base = w.to(torch.bfloat16).view(torch.uint8)
src = (w + torch.randn(total // 2, generator=gen, device="cuda") * 2e-5).to(torch.bfloat16).view(torch.uint8)
del w
soff = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * tbytes)).cuda()
planes, resident = torch.empty_like(src), torch.empty_like(src)
poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda")
tres, dig, dres, gres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(5))
dws = torch.empty(hip.tensor_digest_workspace_bound(total, n), dtype=torch.uint8, device="cuda")

# (a) the digest, the plain split, a copy
digest_ms = timed(lambda: hip.tensor_digest_dbatch(base, soff, digests=dig, results=dres, workspace=dws))
assert bool((dres == tbytes).all())
expected = dig.clone()
split_ms = timed(lambda: hip.planes_split_dbatch(base, soff, E, planes=planes, plane_offsets=poff, results=tres))
copy_ms = timed(lambda: resident.copy_(base))
report("tensor digest", total, digest_ms, vs_split=round(split_ms / digest_ms, 3), vs_copy=round(copy_ms / digest_ms, 3),
       expectation="holds: no longer than the plain split" if digest_ms <= split_ms else "FAILS: LONGER THAN THE PLAIN SPLIT")
report("planes split, plain", total, split_ms)
report("device copy", total, copy_ms)

# (b) the top level of one tensor alone
nt = (tbytes + 32767) // 32768
chain = torch.zeros(8 * nt + 8, dtype=torch.uint8, device="cuda")
ends = torch.tensor([0, chain.numel()], dtype=torch.int64, device="cuda")
chain_ms = timed(lambda: hip.xxh32_batch(chain, ends))
report("XXH32 chain over the 8 nt + 8 bytes of one tensor, one seed", chain.numel(), chain_ms, nt=nt)

# (c) and (d): the segmented sparse FSE SUB delta frames, the gate, the in-place read unchecked and checked
sizes = [tbytes] * n
first = hip.planes_segment_first(sizes, E, SEG_LOG)
nseg = int(first[-1])
blocks = hip.planes_block_bound(total, n, E, BSID)
frames, foff, fres, _, _ = hip.tensor_compress_seg_sparse_dbatch(src, soff, E, SEG_LOG, PERMILLE, first, base=base, codec=0, block_size_id=BSID, max_total_blocks=blocks,
                                                                 delta_op=1)
assert bool((fres > 0).all())
frames = frames[:int(foff[nseg].item())].clone()
sf = torch.from_numpy(first.astype(np.int64)).cuda()
gated = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
gate_ms = timed(lambda: hip.tensor_gate_dbatch(foff, dig, dres, expected, E, frame_first=sf, n_frames=nseg, gated_offsets=gated, results=gres))
assert torch.equal(gated, foff[:nseg + 1]) and bool((gres == tbytes).all())
report("tensor gate", total, gate_ms, frames=nseg)

L = hip.lib
L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize.restype = C.c_size_t
rws = torch.empty(hip.sparse_workspace_bound(total, nseg) + int(L.FSEHIP_frame_decompress_packed_dbatch_workspaceSize(C.c_size_t(nseg), C.c_size_t(blocks))),
                  dtype=torch.uint8, device="cuda")
contents = torch.empty_like(src)
coff, so = (torch.zeros(nseg + 1, dtype=torch.int64, device="cuda") for _ in range(2))
cres, sres = (torch.zeros(nseg, dtype=torch.int64, device="cuda") for _ in range(2))
psz = torch.zeros(n * E, dtype=torch.int64, device="cuda")


def read(offsets):
    hip.tensor_decompress_seg_sparse_dbatch(frames, offsets, soff, E, SEG_LOG, sf, n_segments=nseg, base=resident, dst=resident, max_total_blocks=blocks,
                                            contents=contents, content_offsets=coff, content_results=cres, planes=planes, seg_offsets=so, seg_results=sres,
                                            plane_offsets=poff, plane_sizes=psz, workspace=rws, results=rres, delta_op=1)


def unchecked():
    resident.copy_(base)
    read(foff)


def checked():
    resident.copy_(base)
    hip.tensor_digest_dbatch(resident, soff, digests=dig, results=dres, workspace=dws)
    hip.tensor_gate_dbatch(foff, dig, dres, expected, E, frame_first=sf, n_frames=nseg, gated_offsets=gated, results=gres)
    read(gated)


plain_ms = timed(unchecked)
assert bool((rres == tbytes).all()) and torch.equal(resident, src)
checked_ms = timed(checked)
assert bool((rres == tbytes).all()) and bool((gres == tbytes).all()) and torch.equal(resident, src)
report("in-place seg sparse FSE SUB read, unchecked (with the copy in front)", total, plain_ms, read_ms=round(plain_ms - copy_ms, 4))
report("in-place seg sparse FSE SUB read, checked (copy, digest, gate, read)", total, checked_ms, check_ms=round(checked_ms - plain_ms, 4),
       over_unchecked=round((checked_ms - copy_ms) / (plain_ms - copy_ms), 3))
# a stale base: one element of the first tensor changed -- the first tensor keeps its bytes, the call says which
resident.copy_(base)
resident[7] ^= 1
hip.tensor_digest_dbatch(resident, soff, digests=dig, results=dres, workspace=dws)
hip.tensor_gate_dbatch(foff, dig, dres, expected, E, frame_first=sf, n_frames=nseg, gated_offsets=gated, results=gres)
read(gated)
torch.cuda.synchronize()
want = base[:tbytes].clone(); want[7] ^= 1
assert int(gres[0]) == -4 and int(rres[0]) < 0 and torch.equal(resident[:tbytes], want) and torch.equal(resident[tbytes:], src[tbytes:])
print(json.dumps(dict(shape="%d x %d KiB bf16" % (args.tensors, args.tensor_kib), what="stale first tensor", gate_result=int(gres[0]), read_result=int(rres[0]),
                      kept="every byte of it; the other tensors are the new ones")), flush=True)

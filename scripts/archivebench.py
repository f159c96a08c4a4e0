"""development aid: sealing and opening a tensor archive (FSEHIP_archive_seal_dbatch, FSEHIP_archive_open_dbatch) next to the composites whose
frames the archive carries, in the same run, on the bf16 weight update of deltabench.py (base N(0, 0.02), new = base + N(0, 2e-5) in float32,
both cut to bf16), as SUB deltas with FSE:
  (a) 1024 x 1 MiB, sparse planes at 500 permille (tensor_compress_sparse_dbatch / tensor_decompress_sparse_dbatch)
  (b) 1 x 1 GiB at segment_log 18 (tensor_compress_seg_dbatch / tensor_decompress_seg_dbatch)
The compress composite writes straight to archive[head_bytes:]; "seal" and "open" are the two archive calls alone, with every output and the
workspace given (launches only), "share" = their time over the composite's of the same batch.  The read is in place over a copy of the base,
with the arrays the open emitted; the copy in front of it is timed alone and taken off.
Device events around the calls, repeated until the timed region is at least MIN_MS long, after one warm-up call.  One JSON line per figure.
Usage: archivebench.py [--shape a|b|both] [--block-size-id 5]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from finitestateentropy_amd.api import ARCHIVE_DELTA, ARCHIVE_SPARSE, FseHip

MIN_MS = 300.0
ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="both"); ap.add_argument("--block-size-id", type=int, default=5)
args = ap.parse_args()
hip = FseHip()
BSID, E = args.block_size_id, 2


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


def run(name, n, tbytes, seg_log, permille):
    total = n * tbytes
    gen = torch.Generator(device="cuda").manual_seed(1)
    w = torch.randn(total // 2, generator=gen, device="cuda") * 0.02
    base = w.to(torch.bfloat16).view(torch.uint8)
    src = (w + torch.randn(total // 2, generator=gen, device="cuda") * 2e-5).to(torch.bfloat16).view(torch.uint8)
    del w
    soff = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * tbytes)).cuda()
    first = hip.planes_segment_first([tbytes] * n, E, seg_log) if seg_log else None
    nF = int(first[-1]) if seg_log else n * E
    sf = None if first is None else torch.from_numpy(first.astype(np.int64)).cuda()
    blocks = hip.planes_block_bound(total, n, E, BSID)
    flags = ARCHIVE_DELTA | (ARCHIVE_SPARSE if permille is not None else 0)
    info = hip.archive_info(E, n, nF, total, flags, BSID, seg_log, "sub", permille or 0, blocks, 0)
    head = int(info.headBytes)
    room = hip.frame_packed_bound(total, nF, blocks, 0)
    archive = torch.empty(head + room, dtype=torch.uint8, device="cuda")
    foff = torch.zeros(nF + 1, dtype=torch.int64, device="cuda")
    fres = torch.zeros(nF, dtype=torch.int64, device="cuda")
    tres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
    planes, resident = torch.empty_like(src), torch.empty_like(src)
    common = dict(base=base, codec=0, block_size_id=BSID, dst=archive[head:], dst_capacity=room, max_total_blocks=blocks, frame_offsets=foff, frame_results=fres,
                  tensor_results=tres, planes=planes, delta_op=1)

    def compress():
        if permille is not None:
            hip.tensor_compress_sparse_dbatch(src, soff, E, permille, **common)
        else:
            hip.tensor_compress_seg_dbatch(src, soff, E, seg_log, sf, n_segments=nF, **common)
    compress_ms = timed(compress)
    assert bool((fres > 0).all()) and bool((tres == tbytes).all())
    aws = torch.empty(hip.archive_workspace_bound(n, nF, head), dtype=torch.uint8, device="cuda")
    sres, verdict = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    seal_ms = timed(lambda: hip.archive_seal_dbatch(archive, info, soff, foff, fres, tres, result=sres, workspace=aws))
    size = int(sres.item())
    assert size == head + int(foff[nF].item()), size
    rinfo = hip.archive_inspect(archive[:64].cpu().numpy(), size)
    osoff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ofoff = torch.zeros(nF + 1, dtype=torch.int64, device="cuda")
    osf = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda") if seg_log else None
    sealed = archive[:size]
    open_ms = timed(lambda: hip.archive_open_dbatch(sealed, rinfo, src_offsets=osoff, frame_offsets=ofoff, seg_first=osf, verdict=verdict, workspace=aws))
    assert int(verdict.item()) == size and torch.equal(ofoff, foff) and torch.equal(osoff, soff) and (osf is None or torch.equal(osf, sf))
    frames = sealed[head:]

    def read():
        resident.copy_(base)
        if permille is not None:
            hip.tensor_decompress_sparse_dbatch(frames, ofoff, osoff, E, base=resident, dst=resident, max_total_blocks=blocks, planes=planes, results=rres, delta_op=1)
        else:
            hip.tensor_decompress_seg_dbatch(frames, ofoff, osoff, E, seg_log, osf, n_segments=nF, base=resident, dst=resident, max_total_blocks=blocks, planes=planes,
                                             results=rres, delta_op=1)
    copy_ms = timed(lambda: resident.copy_(base))
    read_ms = timed(read) - copy_ms
    assert bool((rres == tbytes).all()) and torch.equal(resident, src)
    for what, ms, more in (("compress composite into the archive", compress_ms, {}), ("seal", seal_ms, dict(share_of_compress=round(seal_ms / compress_ms, 4))),
                           ("decompress composite from the archive, in place", read_ms, {}), ("open", open_ms, dict(share_of_decompress=round(open_ms / read_ms, 4)))):
        print(json.dumps(dict(shape=name, what=what, ms=round(ms, 4), GBps=round(total / ms / 1e6, 2), frames=nF, head_bytes=head, archive_bytes=size, **more)), flush=True)


if args.shape in ("a", "both"):
    run("1024 x 1 MiB bf16, sparse 500 permille", 1024, 1 << 20, 0, 500)
if args.shape in ("b", "both"):
    run("1 x 1 GiB bf16, segment_log 18", 1, 1 << 30, 18, None)

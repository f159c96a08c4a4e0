"""Frames of unknown size on device buffers (FSEHIP_frame_plan_dbatch, FSEHIP_frame_decompress_packed_dbatch) against the Python restatement
of the inspection (frame_inspect_corpus.py), the host call FSEHIP_frame_inspect and the CPU oracle's reader -- oracle.frame_decompress with
the very slot the device call gave the frame; never against the library's own host reader."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_dev_corpus as fdc
import frame_inspect_corpus as fic
from oracle.oracle import is_error
from test_gpu_fse import s64

pytestmark = pytest.mark.gpu

FILL, TAIL = 0xA5, 64
GENERIC, TOO_SMALL, SRC_WRONG, CORRUPT = -1, -2, -3, -4
HIP_INVALID_VALUE = 1
SZ, VP = C.c_size_t, C.c_void_p


@pytest.fixture(scope="module")
def oracle(checker):
    return checker


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _cat(items):
    return np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(x, np.uint8) for x in items])


def _i64(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).cuda()


def _offsets(items):
    return np.concatenate([[0], np.cumsum([len(x) for x in items])]).astype(np.uint64)


def _slots(bounds, align_log):
    a = (1 << align_log) - 1
    return np.concatenate([[0], np.cumsum([(int(b) + a) & ~a for b in bounds])]).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the plan
def test_plan_of_the_whole_corpus_in_one_batch(hip, oracle):
    from finitestateentropy_amd.api import FRAME_INFO_DTYPE
    corpus, want = fic.corpus(oracle), fic.inspected(oracle)
    frames = [f for _, _, f in corpus]
    n = len(frames)
    assert n > 15 * 1024                                    # the scans cross many groups of 1024 entries
    for f, (rw, iw) in zip(frames, want):                   # the host call, the restatement: one truth
        rg, ig = hip.frame_inspect(f)
        assert rg == rw and ig == iw
    winfo = np.zeros(n, FRAME_INFO_DTYPE)
    for name, key in (("contentBound", "content_bound"), ("nBlocks", "n_blocks"), ("status", "status"), ("checksum22", "checksum22"),
                      ("codec", "codec"), ("blockSizeId", "block_size_id")):
        winfo[name] = [iw[key] for _, iw in want]
    bounds = winfo["contentBound"]
    wfirst = np.concatenate([[0], np.cumsum(winfo["nBlocks"])]).astype(np.uint64)
    # offsets on the device, and the batch as a view that does not start at the buffer's first byte
    buf = _dev(_cat([np.zeros(3, np.uint8)] + frames + [np.full(TAIL, FILL, np.uint8)]))
    batch = buf[3:]
    foff = _i64(_offsets(frames))
    for align_log in (0, 8):
        U = _slots(bounds, align_log)
        doff, bfirst, infos = hip.frame_plan_dbatch(batch, foff, None, align_log, with_infos=True)
        got = infos.cpu().numpy().view(FRAME_INFO_DTYPE)[:, 0]
        for name in FRAME_INFO_DTYPE.names:
            bad = np.nonzero((got[name] != winfo[name]).reshape(n, -1).any(axis=1))[0]
            assert bad.size == 0, (align_log, name, bad[:8], got[name][bad[:8]], winfo[name][bad[:8]])
        assert (bfirst.cpu().numpy().astype(np.uint64) == wfirst).all(), align_log
        assert (doff.cpu().numpy().astype(np.uint64) == U).all(), align_log
        k = n // 2
        while U[k] == U[k - 1]:
            k += 1
        assert 0 < U[k] < U[n]
        for cap in (0, int(U[k]), int(U[k]) - 1, int(U[n])):
            doff, bfirst = hip.frame_plan_dbatch(batch, foff, cap, align_log)
            assert (doff.cpu().numpy().astype(np.uint64) == np.minimum(U, np.uint64(cap))).all(), (align_log, cap)
            assert (bfirst.cpu().numpy().astype(np.uint64) == wfirst).all(), (align_log, cap)
    assert bool((buf[:3] == 0).all()) and bool((buf[-TAIL:] == FILL).all())


def test_plan_without_the_optional_outputs_and_of_no_frames(hip, oracle):
    frames = [f for _, f, _, _ in fic.bases(oracle)[:12]]
    bounds = [fic.inspect(f)[1]["content_bound"] for f in frames]
    d, foff = _dev(_cat(frames)), _i64(_offsets(frames))
    n = len(frames)
    doff = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    hip.lib.FSEHIP_frame_plan_dbatch_workspaceSize.restype = SZ
    ws = torch.empty(int(hip.lib.FSEHIP_frame_plan_dbatch_workspaceSize(SZ(n))), dtype=torch.uint8, device="cuda")
    plan = hip.lib.FSEHIP_frame_plan_dbatch
    stream = VP(torch.cuda.current_stream().cuda_stream)
    rc = plan(VP(doff.data_ptr()), None, None, VP(d.data_ptr()), VP(foff.data_ptr()), SZ(n), C.c_uint64((1 << 64) - 1), C.c_uint(4), VP(ws.data_ptr()), SZ(ws.numel()), stream)
    assert rc == 0
    assert doff.cpu().tolist() == [int(x) for x in _slots(bounds, 4)] + [-7]
    doff.fill_(-7); first = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    rc = plan(VP(doff.data_ptr()), VP(first.data_ptr()), None, VP(d.data_ptr()), VP(foff.data_ptr()), SZ(0), C.c_uint64(100), C.c_uint(0), VP(ws.data_ptr()), SZ(ws.numel()), stream)
    assert rc == 0
    assert doff.cpu().tolist()[:2] == [0, -7] and first.cpu().tolist() == [0, -7]


# ---------------------------------------------------------------------------------------------------------------- the packed reader
@pytest.fixture(scope="module")
def mixed(oracle):
    """both codecs, block-size ids 0 / 2 / 5, intact and damaged frames with empty frames between them; the last frame is an intact one of
    four blocks: -> (frames, content bounds, block counts)"""
    base = fic.bases(oracle)
    frames = [f for _, f, _, _ in base]
    damaged = [f for kind, _, f in fic.corpus(oracle) if kind != "base"]
    for f in damaged[::89]:
        frames += [f, np.zeros(0, np.uint8)]
    frames.append(fdc.frames(oracle, 0)[7])                 # P80, 3 * 1024 + 5 bytes
    infos = [fic.inspect(f)[1] for f in frames]
    assert {i["status"] for i in infos} == {0, 1, 3, 4} and {(i["codec"], i["block_size_id"]) for i in infos} >= {(0, 0), (1, 0), (0, 2), (1, 2), (0, 5), (1, 5)}
    return frames, [i["content_bound"] for i in infos], [i["n_blocks"] for i in infos]


def packed(hip, frames, capacity, max_total_blocks, align_log=0):
    """one packed call into a destination of `capacity` bytes with a tail of FILL behind it: -> (results, offsets, destination bytes)"""
    dst = torch.full((capacity + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    _, doff, res = hip.frame_decompress_packed_dbatch(_dev(_cat(frames)), _offsets(frames), dst=dst, capacity=capacity, max_total_blocks=max_total_blocks,
                                                      align_log=align_log)
    out = dst.cpu().numpy()
    assert (out[capacity:] == FILL).all(), "bytes at or behind dstCapacity"
    return res.cpu().numpy(), doff.cpu().numpy().astype(np.uint64), out


def check_packed(oracle, frames, res, doff, out, what, skip=()):
    """every result and every regenerated byte = the oracle's reader with the frame's slot as its capacity"""
    failed = 0
    for i, f in enumerate(frames):
        if i in skip:
            continue
        at, slot = int(doff[i]), int(doff[i + 1] - doff[i])
        ro, oo = oracle.frame_decompress(f, slot)
        assert int(res[i]) == s64(ro), (what, i, len(f), slot, int(res[i]), s64(ro))
        if not is_error(ro):
            assert (out[at:at + ro] == oo[:ro]).all(), (what, i)
        failed += is_error(ro)
    return failed


@pytest.mark.parametrize("align_log", [0, 8])
def test_packed_decode_of_a_mixed_batch(hip, oracle, mixed, align_log):
    frames, bounds, nblocks = mixed
    U = _slots(bounds, align_log)
    res, doff, out = packed(hip, frames, int(U[-1]), sum(nblocks), align_log)
    assert (doff == U).all()
    failed = check_packed(oracle, frames, res, doff, out, "mixed")
    print("%d frames, %d fail, %d bytes" % (len(frames), failed, int(U[-1])))
    assert failed >= 50 and len(frames) - failed >= 25
    # the reader of known sizes over the offsets the packed call wrote: the same results, the same bytes
    dst = torch.full((int(U[-1]) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    _, res2 = hip.frame_decompress_dbatch(_dev(_cat(frames)), _offsets(frames), _i64(doff), dst=dst, max_total_blocks=sum(nblocks))
    res2, out2 = res2.cpu().numpy(), dst.cpu().numpy()
    assert (res2 == res).all() and (out2[int(U[-1]):] == FILL).all()
    for i in np.nonzero(res > 0)[0]:
        at = int(doff[i])
        assert (out2[at:at + int(res[i])] == out[at:at + int(res[i])]).all(), i
    # the binding on its own: sizing query, exact promise, a destination of its own
    dst3, doff3, res3 = hip.frame_decompress_packed_dbatch(_dev(_cat(frames)), _offsets(frames), align_log=align_log)
    assert (doff3.cpu().numpy().astype(np.uint64) == U).all() and (res3.cpu().numpy() == res).all() and dst3.numel() == max(int(U[-1]), 1)


def test_packed_capacity_short_of_the_total(hip, oracle, mixed):
    frames, bounds, nblocks = mixed
    U = _slots(bounds, 0)
    n = len(frames)
    full, _, out_full = packed(hip, frames, int(U[-1]), sum(nblocks))
    # one byte short: the last frame (3077 bytes in four blocks) straddles the capacity
    res, doff, out = packed(hip, frames, int(U[-1]) - 1, sum(nblocks))
    assert (doff == np.minimum(U, U[-1] - np.uint64(1))).all() and int(doff[n] - doff[n - 1]) == 3076
    check_packed(oracle, frames, res, doff, out, "one short")
    assert full[n - 1] == 3077 and res[n - 1] == TOO_SMALL and (res[:n - 1] == full[:n - 1]).all()
    for i in np.nonzero(full[:n - 1] > 0)[0]:
        at = int(doff[i])
        assert (out[at:at + int(full[i])] == out_full[at:at + int(full[i])]).all(), i
    # the capacity ends inside an earlier frame: that one gets a short slot, every frame behind it an empty one
    k = max(i for i in range(n // 2) if full[i] > 100)
    cap = int(U[k]) + 5
    res, doff, out = packed(hip, frames, cap, sum(nblocks))
    assert (doff == np.minimum(U, np.uint64(cap))).all()
    check_packed(oracle, frames, res, doff, out, "inside frame %d" % k)
    assert (res[:k] == full[:k]).all() and res[k] == TOO_SMALL


def test_packed_promise_one_block_short(hip, oracle, mixed):
    frames, bounds, nblocks = mixed
    U = _slots(bounds, 0)
    n = len(frames)
    res, doff, out = packed(hip, frames, int(U[-1]), sum(nblocks) - 1)
    assert nblocks[n - 1] == 4 and res[n - 1] == GENERIC and (out[int(doff[n - 1]):int(doff[n])] == FILL).all(), "the last frame, its slot untouched"
    check_packed(oracle, frames, res, doff, out, "promise short", skip=(n - 1,))


def test_packed_and_plan_reject_bad_arguments(hip, oracle):
    frames = [f for _, f, _, _ in fic.bases(oracle)[:6]]
    bounds = [fic.inspect(f)[1]["content_bound"] for f in frames]
    nblk = sum(fic.inspect(f)[1]["n_blocks"] for f in frames)
    n, total = len(frames), int(sum(bounds))
    d, foff = _dev(_cat(frames)), _i64(_offsets(frames))
    dst = torch.full((total + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    doff = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda"); res = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    psize, rsize = hip.lib.FSEHIP_frame_plan_dbatch_workspaceSize, hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    psize.restype = SZ; rsize.restype = SZ
    pneed, rneed = int(psize(SZ(n))), int(rsize(SZ(n), SZ(nblk)))
    ws = torch.empty(max(pneed, rneed) + 256, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    for view in (ws[1:], ws[:pneed - 1]):                   # misaligned, one byte short
        with pytest.raises(RuntimeError, match="hipError %d" % HIP_INVALID_VALUE):
            hip.frame_plan_dbatch(d, foff, None, 0, dst_offsets=doff, workspace=view)
    for view in (ws[1:], ws[:rneed - 1]):
        with pytest.raises(RuntimeError, match="hipError %d" % HIP_INVALID_VALUE):
            hip.frame_decompress_packed_dbatch(d, foff, dst=dst, capacity=total, max_total_blocks=nblk, dst_offsets=doff, workspace=view, results=res)
    stream = VP(torch.cuda.current_stream().cuda_stream)
    for align_log in (13, 64, 0xFFFFFFFF):                  # the C ABI itself (the binding refuses these before it calls)
        rc = hip.lib.FSEHIP_frame_plan_dbatch(VP(doff.data_ptr()), None, None, VP(d.data_ptr()), VP(foff.data_ptr()), SZ(n), C.c_uint64(total), C.c_uint(align_log),
                                              VP(ws.data_ptr()), SZ(ws.numel()), stream)
        assert rc == HIP_INVALID_VALUE, align_log
        rc = hip.lib.FSEHIP_frame_decompress_packed_dbatch(VP(dst.data_ptr()), SZ(total), VP(doff.data_ptr()), VP(res.data_ptr()), VP(d.data_ptr()), VP(foff.data_ptr()),
                                                           SZ(n), SZ(nblk), C.c_uint(align_log), VP(ws.data_ptr()), SZ(ws.numel()), stream)
        assert rc == HIP_INVALID_VALUE, align_log
    torch.cuda.synchronize()
    assert bool((dst == FILL).all()) and bool((doff == -7).all()) and bool((res == -7).all())
    # the same buffers, good arguments
    hip.frame_decompress_packed_dbatch(d, foff, dst=dst, capacity=total, max_total_blocks=nblk, dst_offsets=doff, workspace=ws[:rneed], results=res)
    assert doff.cpu().tolist() == [int(x) for x in _slots(bounds, 0)] and res.cpu().tolist() == [int(b) for b in bounds]


# ---------------------------------------------------------------------------------------------------------------- graph
def test_packed_call_replays_from_a_hip_graph(hip, oracle):
    """captured once, replayed on frames of other sizes (and another codec) in the same buffers; the promise and the capacity are upper bounds"""
    sizes = [0, 1, 1025, 3 * 1024 + 5, 2500, 700, 40 * 1024 + 3]
    rng = np.random.default_rng(29)

    def make(trial):
        out, order = [], np.roll(sizes, trial)
        for i, n in enumerate(int(x) for x in order):
            data = rng.integers(0, 256, n, dtype=np.uint8) if n == 2500 else oracle.probagen_batch((14, 80, 20)[(trial + i) % 3], 1, max(n, 1), 100 * trial + i)[0][:n]
            r, f = oracle.frame_compress(data, 0, (trial + i) % 2)
            out.append((data, f[:r].copy()))
        return out

    n, total = len(sizes), int(sum(sizes))
    promise = sum(fdc.block_count(x) for x in sizes) + 9
    cap = total + 16 * n + 100                              # (slots are rounded up to 16 bytes)
    fbuf = torch.zeros(sum(fdc.bound(x) for x in sizes), dtype=torch.uint8, device="cuda")
    foff = torch.zeros(n + 1, dtype=torch.int64, device="cuda"); doff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    res = torch.zeros(n, dtype=torch.int64, device="cuda")
    dst = torch.full((cap + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize.restype = SZ
    ws = torch.empty(int(hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize(SZ(n), SZ(promise))), dtype=torch.uint8, device="cuda")

    def load(trial):
        items = make(trial)
        packed_frames = _cat([f for _, f in items])
        fbuf.zero_(); fbuf[:len(packed_frames)].copy_(_dev(packed_frames))
        foff.copy_(_i64(_offsets([f for _, f in items])))
        return items

    def work():
        hip.frame_decompress_packed_dbatch(fbuf, foff, dst=dst, capacity=cap, max_total_blocks=promise, align_log=4, dst_offsets=doff, workspace=ws, results=res)
    load(0); work(); torch.cuda.synchronize()               # one ordinary call first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # torch's capture stream: not the default stream
        work()
    for trial in (1, 2, 3):
        items = load(trial)
        dst.fill_(FILL); doff.zero_(); res.zero_()
        g.replay()
        torch.cuda.synchronize()
        out, off = dst.cpu().numpy(), doff.cpu().numpy()
        assert off.tolist() == [int(x) for x in _slots([len(d) for d, _ in items], 4)], trial
        assert res.cpu().tolist() == [len(d) for d, _ in items], trial
        for i, (data, _) in enumerate(items):
            assert (out[int(off[i]):int(off[i]) + len(data)] == data).all(), (trial, i)
        assert (out[cap:] == FILL).all(), trial

"""The packed frame writer on device buffers (FSEHIP_frame_compress_packed_dbatch: frames back to back at their real sizes, destination
offsets an output) against the CPU oracle's writer -- oracle.frame_compress gives every frame's bytes and size, frame_packed_corpus.py the
model of where frames of those sizes land and what each one's result is; never against the library's own fixed-slot or host writer.
Block-size id 0 (1 KB blocks) unless said otherwise.  Every destination is filled with 0xA5 and has a tail behind it: whatever is not a byte
of a frame that succeeded -- padding, the slots of frames that fail, the room behind the last frame, the tail -- must still be 0xA5."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_dev_corpus as fdc
import frame_packed_corpus as fpc
from frame_packed_corpus import GENERIC, TOO_SMALL

pytestmark = pytest.mark.gpu

FILL, TAIL = 0xA5, 64
HIP_INVALID_VALUE = 1
SZ, VP = C.c_size_t, C.c_void_p
ALL_FORMS = {(t, full) for t in (0, 1, 2) for full in (False, True)}


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


def _blocks(contents, bsid=0):
    return sum(fdc.block_count(len(c), bsid) for c in contents)


def write(hip, contents, codec, bsid=0, align_log=0, cap=None, room=None, promise=None):
    """one packed call into `room` bytes (default: the capacity; the capacity's default: FSEHIP_frame_packedBound) of FILL with a tail of FILL
    behind them: -> (results, offsets, every byte of the destination)"""
    n = len(contents)
    if cap is None:
        cap = hip.frame_packed_bound(sum(len(c) for c in contents), n, _blocks(contents, bsid), align_log)
    room = cap if room is None else room
    dst = torch.full((room + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    _, doff, res = hip.frame_compress_packed_dbatch(_dev(_cat(contents)), _offsets(contents), bsid, codec, dst=dst, capacity=cap,
                                                    max_total_blocks=_blocks(contents, bsid) if promise is None else promise, align_log=align_log)
    return [int(x) for x in res.cpu()], [int(x) for x in doff.cpu()], dst.cpu().numpy()


def check(want, res, off, out, align_log, cap, what):
    """want[i]: the oracle's frame of content i, or the (negative) error the frame ends with whatever the capacity.  Offsets and results are
    the model's, every frame that succeeds is the oracle's byte for byte, and no other byte of the destination was written."""
    sizes = [w if isinstance(w, int) else len(w) for w in want]
    assert off == fpc.packed_offsets(sizes, align_log, cap), what
    assert res == fpc.packed_results(sizes, align_log, cap), what
    written = np.zeros(len(out), bool)
    for i, w in enumerate(want):
        if res[i] > 0:
            assert (out[off[i]:off[i] + res[i]] == w).all(), (what, i)
            written[off[i]:off[i] + res[i]] = True
    assert (out[~written] == FILL).all(), (what, "bytes outside the frames", np.nonzero((out != FILL) & ~written)[0][:8])
    return sizes


def raw(hip, dst, cap, doff, res, src, soff, n, nblk, bsid, codec, align_log, ws):
    """FSEHIP_frame_compress_packed_dbatch itself (dst None: a NULL destination): -> its return value"""
    return hip.lib.FSEHIP_frame_compress_packed_dbatch(VP(dst.data_ptr() if dst is not None else 0), C.c_uint64(cap), VP(doff.data_ptr()), VP(res.data_ptr()),
                                                       VP(src.data_ptr()), VP(soff.data_ptr()), SZ(n), SZ(nblk), C.c_uint(bsid), C.c_int(codec), C.c_uint(align_log),
                                                       VP(ws.data_ptr()), SZ(ws.numel()), VP(torch.cuda.current_stream().cuda_stream))


def forms_of(res, off, out):
    forms = set()
    for r, at in zip(res, off):
        if r > 0:
            forms |= fdc.header_forms(out[at:at + r])
    return forms


# ---------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("align_log", [0, 8])
@pytest.mark.parametrize("codec", [0, 1])
def test_whole_corpus_and_a_long_batch(hip, oracle, codec, align_log):
    contents = [c for _, c in fdc.contents(oracle)]
    frames = fdc.frames(oracle, codec)
    assert _blocks(contents) > 1024                         # the 1100-block content: the scan of the record positions crosses groups
    res, off, out = write(hip, contents, codec, align_log=align_log)
    check(frames, res, off, out, align_log, fpc.NO_CAP, "corpus")
    assert forms_of(res, off, out) == ALL_FORMS, "all three block kinds, full and partial headers"
    assert res[0] == 8 and res[11] == 8                     # the empty contents: magic, id, end mark
    contents, frames = fpc.long_batch(oracle, codec)        # more than 2048 frames: the scan over frames crosses groups too
    res, off, out = write(hip, contents, codec, align_log=align_log, promise=_blocks(contents) + 1000)
    sizes = check(frames, res, off, out, align_log, fpc.NO_CAP, "long batch")
    assert len(res) > 2048 and off[-1] == sum((s + (1 << align_log) - 1) >> align_log << align_log for s in sizes)


def test_other_block_sizes(hip, oracle):
    k = 0
    for bsid in (2, 5):
        for codec in (0, 1):
            data, frame = fdc.big_frames(oracle)[k]; k += 1
            assert int(frame[4]) == bsid and len(data) == 150000
            tiny = np.array([7, 7, 7], np.uint8)
            r, f = oracle.frame_compress(tiny, bsid, codec)
            res, off, out = write(hip, [data, tiny, data], codec, bsid=bsid, align_log=4)
            check([frame, f[:r], frame], res, off, out, 4, fpc.NO_CAP, (bsid, codec))


# ---------------------------------------------------------------------------------------------------------------- 3, 4, 5, 6
def small(oracle, codec):
    """eleven small contents and, last, the P80 content of four blocks: -> (contents, the oracle's frames)"""
    pick = list(range(11)) + [7]
    contents = [fdc.contents(oracle)[i][1] for i in pick]
    assert fdc.block_count(len(contents[-1])) == 4
    return contents, [fdc.frames(oracle, codec)[i] for i in pick]


@pytest.mark.parametrize("codec", [0, 1])
def test_capacity_short_of_the_total(hip, oracle, codec):
    contents, frames = small(oracle, codec)
    n = len(contents)
    U = fpc.packed_offsets([len(f) for f in frames], 0)
    full, off_full, out_full = write(hip, contents, codec, cap=U[n])
    check(frames, full, off_full, out_full, 0, U[n], "exact capacity")
    assert full == [len(f) for f in frames]
    # one byte short: the last frame alone fails, its slot is untouched
    res, off, out = write(hip, contents, codec, cap=U[n] - 1, room=U[n])
    check(frames, res, off, out, 0, U[n] - 1, "one short")
    assert res[:n - 1] == full[:n - 1] and res[n - 1] == TOO_SMALL and off[n] - off[n - 1] == len(frames[-1]) - 1
    assert (out[:U[n - 1]] == out_full[:U[n - 1]]).all() and (out[U[n - 1]:] == FILL).all()
    # the capacity ends 5 bytes into an earlier frame: that one and every later one fail, nothing is written at or behind the capacity
    k = 6
    cap = U[k] + 5
    assert len(frames[k]) > 5
    res, off, out = write(hip, contents, codec, cap=cap, room=U[n])
    check(frames, res, off, out, 0, cap, "inside frame %d" % k)
    assert off == [min(u, cap) for u in U] and res[:k] == full[:k] and res[k:] == [TOO_SMALL] * (n - k)
    assert (out[:U[k]] == out_full[:U[k]]).all() and (out[U[k]:] == FILL).all()


@pytest.mark.parametrize("codec", [0, 1])
def test_promise_one_block_short(hip, oracle, codec):
    contents, frames = small(oracle, codec)
    n = len(contents)
    res, off, out = write(hip, contents, codec, align_log=4, promise=_blocks(contents) - 1)
    check(frames[:n - 1] + [GENERIC], res, off, out, 4, fpc.NO_CAP, "promise short")
    assert res[n - 1] == GENERIC and off[n] == off[n - 1], "the last frame, and it takes no room"
    # no promise at all: empty contents still give their 8-byte frames
    few = [np.zeros(0, np.uint8), np.array([1], np.uint8), np.zeros(0, np.uint8)]
    res, off, out = write(hip, few, codec, promise=0)
    check([frames[0], GENERIC, frames[0]], res, off, out, 0, fpc.NO_CAP, "promise 0")
    assert res == [8, GENERIC, 8] and off == [0, 8, 8, 16]


@pytest.mark.parametrize("codec", [0, 1])
def test_sizing_query(hip, oracle, codec):
    contents, frames = small(oracle, codec)
    n = len(contents)
    src, soff = _dev(_cat(contents)), _offsets(contents)
    hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize.restype = SZ
    ws = torch.empty(int(hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize(SZ(n), SZ(_blocks(contents)), C.c_uint(0), C.c_int(codec))),
                     dtype=torch.uint8, device="cuda")
    sizes = [len(f) for f in frames]
    for align_log in (0, 8):
        doff = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda"); res = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        assert raw(hip, None, (1 << 64) - 1, doff, res, src, _i64(soff), n, _blocks(contents), 0, codec, align_log, ws) == 0     # d_dst NULL, UINT64_MAX
        assert [int(x) for x in doff.cpu()] == fpc.packed_offsets(sizes, align_log) and [int(x) for x in res.cpu()] == sizes
        need = int(doff[n].item())
        res2, off2, out = write(hip, contents, codec, align_log=align_log, cap=need)
        check(frames, res2, off2, out, align_log, need, "at the queried capacity")
        assert res2 == sizes and off2 == [int(x) for x in doff.cpu()]
        # the binding on its own: a destination at FSEHIP_frame_packedBound (guarded, and checked for bytes outside the frames, in guard mode)
        dst3, doff3, res3 = hip.frame_compress_packed_dbatch(src, soff, 0, codec, align_log=align_log)
        assert dst3.numel() == fpc.packed_bound([len(c) for c in contents], 0, align_log)
        assert [int(x) for x in doff3.cpu()] == off2 and [int(x) for x in res3.cpu()] == sizes
        out3 = dst3.cpu().numpy()
        for i, f in enumerate(frames):
            assert (out3[off2[i]:off2[i] + len(f)] == f).all(), (align_log, i)


@pytest.mark.parametrize("codec", [0, 1])
def test_fixed_slot_call_is_unchanged(hip, oracle, codec):
    contents = [c for _, c in fdc.contents(oracle)]
    res, off, out = write(hip, contents, codec)
    foff = hip.frame_dbatch_plan([len(c) for c in contents], 0)              # every slot at FSEHIP_frame_compressBound
    dst = torch.full((int(foff[-1]) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    _, _, fres = hip.frame_compress_dbatch(_dev(_cat(contents)), _offsets(contents), 0, codec, dst=dst, dst_offsets=foff, max_total_blocks=_blocks(contents))
    fres, fout = [int(x) for x in fres.cpu()], dst.cpu().numpy()
    assert fres == res == [len(f) for f in fdc.frames(oracle, codec)]
    written = np.zeros(len(fout), bool)
    for i, r in enumerate(res):
        assert (fout[int(foff[i]):int(foff[i]) + r] == out[off[i]:off[i] + r]).all(), i
        written[int(foff[i]):int(foff[i]) + r] = True
    assert (fout[~written] == FILL).all()
    # ... and below the bound it still refuses, where the packed call needs no more than the frame
    caps = [fdc.bound(len(c)) for c in contents]
    caps[8] -= 1
    foff = np.concatenate([[0], np.cumsum(caps)]).astype(np.uint64)
    _, _, fres = hip.frame_compress_dbatch(_dev(_cat(contents)), _offsets(contents), 0, codec, dst=dst, dst_offsets=foff, max_total_blocks=_blocks(contents))
    fres = [int(x) for x in fres.cpu()]
    assert fres[8] == TOO_SMALL and fres[:8] + fres[9:] == res[:8] + res[9:]


# ---------------------------------------------------------------------------------------------------------------- 7
def test_bad_arguments_through_the_c_abi(hip, oracle):
    contents, frames = small(oracle, 0)
    n, nblk = len(contents), _blocks(contents)
    sizes = [len(f) for f in frames]
    cap = fpc.packed_offsets(sizes, 0)[-1]
    src, soff = _dev(_cat(contents)), _i64(_offsets(contents))
    dst = torch.full((cap + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    doff = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda"); res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    wsize = hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize
    wsize.restype = SZ
    need = int(wsize(SZ(n), SZ(nblk), C.c_uint(0), C.c_int(0)))
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0

    def call(bsid=0, codec=0, align_log=0, w=ws[:need], nf=n):
        return raw(hip, dst, cap, doff, res, src, soff, nf, nblk, bsid, codec, align_log, w)
    for bad in (dict(align_log=13), dict(align_log=64), dict(align_log=0xFFFFFFFF), dict(bsid=7), dict(bsid=255), dict(codec=2), dict(codec=-1),
                dict(w=ws[1:need + 1]), dict(w=ws[:need - 1])):
        assert call(**bad) == HIP_INVALID_VALUE, bad
    torch.cuda.synchronize()
    assert bool((dst == FILL).all()) and bool((doff == -7).all()) and bool((res == -7).all())
    # no frames: entry 0 of the offsets, nothing else
    assert call(nf=0) == 0
    torch.cuda.synchronize()
    assert doff.cpu().tolist() == [0] + [-7] * (n + 1) and bool((res == -7).all()) and bool((dst == FILL).all())
    # the same buffers, good arguments
    assert call() == 0
    torch.cuda.synchronize()
    check(frames, res.cpu().tolist()[:n], doff.cpu().tolist()[:n + 1], dst.cpu().numpy(), 0, cap, "good call")
    assert int(doff[n + 1]) == -7 and int(res[n]) == -7


# ---------------------------------------------------------------------------------------------------------------- 8
def test_writer_and_packed_reader_round_trip_in_one_hip_graph(hip, oracle):
    """One graph: the packed writer, then FSEHIP_frame_decompress_packed_dbatch fed with the offsets the writer has just produced -- no size
    leaves the device between them.  Captured once, replayed on contents of other sizes in the same buffers; capacities and promises are upper
    bounds.  The codec is an argument of the writer, fixed when the graph is captured, so the graph holds the chain once per codec (source,
    offsets and workspaces shared, outputs apart) and every replay runs both."""
    sizes = [0, 1, 1025, 3 * 1024 + 5, 2500, 700, 40 * 1024 + 3]
    rng = np.random.default_rng(31)
    ALIGN = 4

    def make(trial):
        out, order = [], np.roll(sizes, trial)
        for i, n in enumerate(int(x) for x in order):
            out.append(rng.integers(0, 256, n, dtype=np.uint8) if n == 2500 else oracle.probagen_batch((14, 80, 20)[(trial + i) % 3], 1, max(n, 1), 100 * trial + i)[0][:n])
        return out

    n, total = len(sizes), int(sum(sizes))
    promise = sum(fdc.block_count(x) for x in sizes) + 9
    fcap = hip.frame_packed_bound(total, n, promise, ALIGN)
    ccap = total + 16 * n + 100                             # (slots are rounded up to 16 bytes)
    src = torch.zeros(total, dtype=torch.uint8, device="cuda"); soff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize.restype = SZ
    hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize.restype = SZ
    wws = torch.empty(max(int(hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize(SZ(n), SZ(promise), C.c_uint(0), C.c_int(c))) for c in (0, 1)),
                      dtype=torch.uint8, device="cuda")
    rws = torch.empty(int(hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize(SZ(n), SZ(promise))), dtype=torch.uint8, device="cuda")
    chains = []
    for codec in (0, 1):
        chains.append(dict(codec=codec, frames=torch.full((fcap + TAIL,), FILL, dtype=torch.uint8, device="cuda"),
                           back=torch.full((ccap + TAIL,), FILL, dtype=torch.uint8, device="cuda"),
                           foff=torch.zeros(n + 1, dtype=torch.int64, device="cuda"), boff=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                           wres=torch.zeros(n, dtype=torch.int64, device="cuda"), rres=torch.zeros(n, dtype=torch.int64, device="cuda")))

    def load(trial):
        contents = make(trial)
        src.copy_(_dev(_cat(contents))); soff.copy_(_i64(_offsets(contents)))
        return contents

    def work():
        for c in chains:
            hip.frame_compress_packed_dbatch(src, soff, 0, c["codec"], dst=c["frames"], capacity=fcap, max_total_blocks=promise, align_log=ALIGN,
                                             dst_offsets=c["foff"], workspace=wws, results=c["wres"])
            hip.frame_decompress_packed_dbatch(c["frames"], c["foff"], dst=c["back"], capacity=ccap, max_total_blocks=promise, align_log=ALIGN,
                                               dst_offsets=c["boff"], workspace=rws, results=c["rres"])
    load(0); work(); torch.cuda.synchronize()               # one ordinary call first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # torch's capture stream: not the default stream
        work()
    for trial in (1, 2, 3):
        contents = load(trial)
        for c in chains:
            c["frames"].fill_(FILL); c["back"].fill_(FILL)
            for t in (c["foff"], c["boff"], c["wres"], c["rres"]):
                t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for c in chains:
            want = []
            for data in contents:
                r, f = oracle.frame_compress(data, 0, c["codec"])
                want.append(f[:r].copy())
            what = (trial, c["codec"])
            check(want, c["wres"].cpu().tolist(), c["foff"].cpu().tolist(), c["frames"].cpu().numpy(), ALIGN, fcap, what)
            boff, back = c["boff"].cpu().tolist(), c["back"].cpu().numpy()
            assert boff == fpc.packed_offsets([len(d) for d in contents], ALIGN, ccap), what
            assert c["rres"].cpu().tolist() == [len(d) for d in contents], what
            for i, data in enumerate(contents):
                assert (back[boff[i]:boff[i] + len(data)] == data).all(), (what, i)
            assert (back[ccap:] == FILL).all(), what

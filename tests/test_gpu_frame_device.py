"""The .fse frame on device buffers (FSEHIP_XXH32_batch, FSEHIP_frame_compress_dbatch, FSEHIP_frame_decompress_dbatch) against the CPU
oracle -- oracle.frame_compress / frame_decompress / xxh32, the restatement pinned against the reference's tool by test_frame_oracle.py;
never against the library's own host frame calls.  Block-size id 0 (1 KB blocks) unless said otherwise.

Guard bytes: capacities are differences of offsets, so there is no room for a guard BETWEEN two slots -- the helpers below therefore put a
7-byte slot of 0xA5 behind every real one, owned by an item that must fail without writing (the writer: an empty content, whose 8-byte
frame does not fit; the reader: an empty frame), and a tail behind the last."""
import numpy as np
import pytest
import torch

import frame_dev_corpus as fdc
from oracle.oracle import is_error
from test_frame_oracle import oversize_frames
from test_gpu_fse import s64

pytestmark = pytest.mark.gpu

GUARD, FILL, TAIL = 7, 0xA5, 64
GENERIC, TOO_SMALL, SRC_WRONG, CORRUPT = -1, -2, -3, -4
HIP_INVALID_VALUE = 1


@pytest.fixture(scope="module")
def oracle(checker):
    return checker


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _cat(items):
    return np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(x, np.uint8) for x in items])


def _same(got, want):
    """a result of the library (int64: -code) against the oracle's size_t"""
    return int(got) == s64(want)


def write(hip, contents, codec, bsid=0, caps=None, max_total_blocks=None, guards=True):
    """-> [(result, slot bytes)] of the real contents; asserts the guard slots, the tail and the bytes behind every frame untouched"""
    caps = [fdc.bound(len(c), bsid) for c in contents] if caps is None else caps
    items, slots = [], []
    for c, cap in zip(contents, caps):
        items.append(c); slots.append(cap)
        if guards:
            items.append(np.zeros(0, np.uint8)); slots.append(GUARD)
    soff = np.concatenate([[0], np.cumsum([len(x) for x in items])]).astype(np.uint64)
    doff = np.concatenate([[0], np.cumsum(slots)]).astype(np.uint64)
    dst = torch.full((int(doff[-1]) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    if max_total_blocks is None:
        max_total_blocks = sum(fdc.block_count(len(c), bsid) for c in contents)
    _, _, res = hip.frame_compress_dbatch(_dev(_cat(items)), soff, bsid, codec, dst=dst, dst_offsets=doff, max_total_blocks=max_total_blocks)
    res = res.cpu().numpy(); out = dst.cpu().numpy()
    assert (out[int(doff[-1]):] == FILL).all(), "tail"
    got = []
    step = 2 if guards else 1
    for i in range(len(contents)):
        k = step * i
        slot = out[int(doff[k]):int(doff[k + 1])]
        used = max(int(res[k]), 0)
        assert (slot[used:] == FILL).all(), ("bytes behind frame", i)
        if guards:
            assert res[k + 1] == TOO_SMALL and (out[int(doff[k + 1]):int(doff[k + 2])] == FILL).all(), ("guard slot", i)
        got.append((int(res[k]), slot))
    return got


def read(hip, frames, caps, max_total_blocks=None):
    """-> [(result, slot bytes)] of the real frames; asserts the guard slots and the tail untouched"""
    items, slots = [], []
    for f, cap in zip(frames, caps):
        items += [f, np.zeros(0, np.uint8)]; slots += [cap, GUARD]
    foff = np.concatenate([[0], np.cumsum([len(x) for x in items])]).astype(np.uint64)
    doff = np.concatenate([[0], np.cumsum(slots)]).astype(np.uint64)
    dst = torch.full((int(doff[-1]) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    _, res = hip.frame_decompress_dbatch(_dev(_cat(items)), foff, doff, dst=dst, max_total_blocks=max_total_blocks)
    res = res.cpu().numpy(); out = dst.cpu().numpy()
    assert (out[int(doff[-1]):] == FILL).all(), "tail"
    got = []
    for i in range(len(frames)):
        assert res[2 * i + 1] == SRC_WRONG and (out[int(doff[2 * i + 1]):int(doff[2 * i + 2])] == FILL).all(), ("guard slot", i)
        got.append((int(res[2 * i]), out[int(doff[2 * i]):int(doff[2 * i + 1])]))
    return got


def check_read(oracle, frames, caps, got, what):
    for i, (f, cap, (rg, og)) in enumerate(zip(frames, caps, got)):
        ro, oo = oracle.frame_decompress(f, cap)
        print("%s[%d]: oracle %d, device %d" % (what, i, s64(ro), rg))
        assert _same(rg, ro), (what, i, rg, s64(ro))
        if not is_error(ro):
            assert (og[:ro] == oo[:ro]).all(), (what, i)


# ---------------------------------------------------------------------------------------------------------------- XXH32
def test_xxh32_batch_every_alignment_and_tail(hip, oracle):
    base = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 70001]
    lengths = []
    for _ in range(16):                                     # sum(base) + 1 = 15 mod 16: every round starts one byte lower (mod 16) than the last
        lengths += base + [1]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    for k, n in enumerate(base):                            # one call, items back to back: every length starts at every alignment mod 16
        assert len(set(int(off[k + 19 * j]) % 16 for j in range(16))) == 16, n
    data = np.random.default_rng(1).integers(0, 256, int(off[-1]), dtype=np.uint8)
    assert oracle.xxh32(np.zeros(0, np.uint8)) == 0x02CC5D05
    d = _dev(data)
    for seed in (0, 0x9E3779B1):
        got = hip.xxh32_batch(d, off, seed).cpu().numpy()
        want = [oracle.xxh32(data[int(off[i]):int(off[i + 1])], seed) for i in range(len(lengths))]
        assert [int(x) for x in got] == want, seed
    # offsets already on the device, and a view that does not start at the buffer's first byte
    got = hip.xxh32_batch(d, torch.from_numpy(off[3:].astype(np.int64)).cuda(), 0).cpu().numpy()
    assert int(got[0]) == oracle.xxh32(data[int(off[3]):int(off[4])]) and int(got[-1]) == oracle.xxh32(data[int(off[-2]):])


# ---------------------------------------------------------------------------------------------------------------- writer
@pytest.fixture(scope="module")
def batch(oracle):
    names = [n for n, _ in fdc.contents(oracle)]
    return names, [c for _, c in fdc.contents(oracle)]


def _check_written(oracle, codec, got, what, skip=()):
    want = fdc.frames(oracle, codec)
    for i, (rg, og) in enumerate(got):
        if i in skip:
            continue
        assert rg == len(want[i]) and (og[:rg] == want[i]).all(), (what, codec, i, rg, len(want[i]))


@pytest.mark.parametrize("codec", [0, 1])
def test_writer_matches_oracle(hip, oracle, batch, codec):
    """the whole batch in one call, maxTotalBlocks exact: results and bytes are the oracle's, nothing else is written"""
    names, contents = batch
    frames = fdc.frames(oracle, codec)
    forms = set()
    for f in frames:
        forms |= fdc.header_forms(f)
    assert forms == {(t, full) for t in (0, 1, 2) for full in (False, True)}, "all three block kinds, full and partial headers"
    got = write(hip, contents, codec)
    _check_written(oracle, codec, got, "batch")
    assert got[0][0] == 8 and got[11][0] == 8               # the empty contents: magic, id, end mark
    assert (frames[1][5] >> 6) == (1 if codec == 0 else 2)  # one byte: FSE stores it raw, Huff0 as RLE
    # a generous promise changes nothing
    got = write(hip, contents, codec, max_total_blocks=sum(fdc.block_count(len(c)) for c in contents) + 1000)
    _check_written(oracle, codec, got, "generous")


@pytest.mark.parametrize("codec", [0, 1])
def test_writer_one_frame_and_more_frames_than_lanes(hip, oracle, batch, codec):
    names, contents = batch
    frames = fdc.frames(oracle, codec)
    for i, c in enumerate(contents):                        # nFrames = 1 (no guard items: the call sees one frame)
        (rg, og), = write(hip, [c], codec, guards=False)
        assert rg == len(frames[i]) and (og[:rg] == frames[i]).all(), (names[i], codec)
    got = write(hip, [contents[6]] * 65, codec)             # 65 x the 1025-byte content: 130 frames with the guard items
    for rg, og in got:
        assert rg == len(frames[6]) and (og[:rg] == frames[6]).all(), codec


@pytest.mark.parametrize("codec", [0, 1])
def test_writer_promise_one_short_and_slot_one_short(hip, oracle, batch, codec):
    names, contents = batch
    exact = sum(fdc.block_count(len(c)) for c in contents)
    got = write(hip, contents, codec, max_total_blocks=exact - 1)
    last = len(contents) - 1
    assert got[last][0] == GENERIC and (got[last][1] == FILL).all(), "exactly the last frame, its slot untouched"
    _check_written(oracle, codec, got, "one short", skip=(last,))
    caps = [fdc.bound(len(c)) for c in contents]
    caps[8] -= 1                                            # the 2500 bytes of noise, one byte under FSEHIP_frame_compressBound
    got = write(hip, contents, codec, caps=caps)
    assert got[8][0] == TOO_SMALL and (got[8][1] == FILL).all()
    _check_written(oracle, codec, got, "slot short", skip=(8,))


def test_writer_rejects_bad_arguments(hip, oracle, batch):
    c = batch[1][5]
    soff = np.array([0, len(c)], np.uint64); doff = np.array([0, fdc.bound(len(c))], np.uint64)
    dst = torch.full((int(doff[-1]),), FILL, dtype=torch.uint8, device="cuda")
    ws = hip.frame_dbatch_workspace(1, 1, 0, 0)
    for bsid, codec in ((7, 0), (0, 2)):
        with pytest.raises(RuntimeError, match="hipError %d" % HIP_INVALID_VALUE):
            hip.frame_compress_dbatch(_dev(c), soff, bsid, codec, dst=dst, dst_offsets=doff, max_total_blocks=1, workspace=ws)
    torch.cuda.synchronize()
    assert bool((dst == FILL).all())


# ---------------------------------------------------------------------------------------------------------------- reader
def test_reader_mixed_batch(hip, oracle, batch):
    """FSE and Huff0 frames interleaved in one call, plus frames at block-size ids 2 and 5: exact capacities, and larger by 100"""
    names, contents = batch
    frames, sizes = [], []
    for i, c in enumerate(contents):
        for codec in (0, 1):
            frames.append(fdc.frames(oracle, codec)[i]); sizes.append(len(c))
    for data, f in fdc.big_frames(oracle):
        frames.append(f); sizes.append(len(data))
    for extra in (0, 100):
        caps = [n + extra for n in sizes]
        got = read(hip, frames, caps)
        check_read(oracle, frames, caps, got, "intact+%d" % extra)
        for (rg, og), n in zip(got, sizes):
            assert rg == n
    # the promise: exact is fine; one short fails exactly the last frame that has blocks, which writes nothing
    nblocks = [fdc.block_count(n) for n in sizes[:-4]] + [fdc.block_count(150000, 2)] * 2 + [fdc.block_count(150000, 5)] * 2
    got = read(hip, frames, sizes, max_total_blocks=sum(nblocks))
    assert [r for r, _ in got] == sizes
    got = read(hip, frames, sizes, max_total_blocks=sum(nblocks) - 1)
    assert [r for r, _ in got[:-1]] == sizes[:-1] and got[-1][0] == GENERIC and (got[-1][1] == FILL).all()


@pytest.mark.parametrize("codec", [0, 1])
def test_reader_damaged_frames(hip, oracle, batch, codec):
    """what tests/test_gpu_frame.py does to the host reader: result = the oracle's, output equal wherever the oracle succeeds"""
    data = batch[1][7]                                      # P80, 3 * 1024 + 5 bytes
    frame = fdc.frames(oracle, codec)[7]
    r = len(frame)
    cases = []
    for pos in (r - 1, 0, 4, 5, 6, 7, 40, r - 3, r - 5):
        bad = frame.copy(); bad[pos] ^= 0x55; cases.append((bad, len(data)))
    cases += [(frame[:r - 4], len(data)), (frame[:9], len(data)), (frame[:5], len(data)), (frame, len(data) - 1), (frame, 1000)]
    rng = np.random.default_rng(3)
    for _ in range(6):
        bad = frame.copy(); idx = rng.integers(5, r, 3); bad[idx] = rng.integers(0, 256, 3); cases.append((bad, len(data)))
    cases += oversize_frames(oracle)
    frames, caps = [f for f, _ in cases], [c for _, c in cases]
    got = read(hip, frames, caps)                           # maxTotalBlocks = sum((F_i - 8) / 2), the binding's default
    check_read(oracle, frames, caps, got, "damaged")
    assert sum(1 for rg, _ in got if rg < 0) >= 10          # (the cases do fail)


def test_reader_block_that_regenerates_less_than_announced(hip, oracle):
    ab, frame = fdc.crafted_short_block(oracle, 0)
    assert len(ab) == 1724
    for cap in (1724, 2124):                                # what the oracle makes of it
        ro, oo = oracle.frame_decompress(frame, cap)
        assert ro == 1724 and (oo[:1724] == ab).all(), cap
    _, hframe = fdc.crafted_short_block(oracle, 1)
    ro, _ = oracle.frame_decompress(hframe, 2124)
    assert s64(ro) == CORRUPT
    frames = [frame, frame, frame, hframe, hframe]
    caps = [1724, 2124, 1723, 1724, 2124]
    got = read(hip, frames, caps)
    check_read(oracle, frames, caps, got, "crafted")
    assert got[0][0] == 1724 and got[1][0] == 1724 and got[3][0] == CORRUPT and got[4][0] == CORRUPT


# ---------------------------------------------------------------------------------------------------------------- graph
def test_writer_and_reader_replay_from_a_hip_graph(hip, oracle):
    from finitestateentropy_amd.api import FseHip
    sizes = [0, 1, 1025, 3 * 1024 + 5, 2500, 700, 40 * 1024 + 3]
    rng = np.random.default_rng(23)

    def make(trial):
        out = []
        for i, n in enumerate(sizes):
            if n == 2500:
                out.append(rng.integers(0, 256, n, dtype=np.uint8))
            else:
                out.append(oracle.probagen_batch((14, 80, 20)[(trial + i) % 3], 1, max(n, 1), 100 * trial + i)[0][:n])
        return out

    old = FseHip.guard
    FseHip.guard = 0                                        # (the guard's check synchronises: not inside a capture)
    try:
        for codec in (0, 1):
            nblk = sum(fdc.block_count(n) for n in sizes)
            soff = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).cuda()
            foff_h = hip.frame_dbatch_plan(sizes, 0)
            foff = torch.from_numpy(foff_h.astype(np.int64)).cuda()
            src = _dev(_cat(make(0)))
            frames = torch.zeros(int(foff_h[-1]), dtype=torch.uint8, device="cuda")
            back = torch.zeros(int(sum(sizes)), dtype=torch.uint8, device="cuda")
            cres = torch.zeros(len(sizes), dtype=torch.int64, device="cuda"); dres = torch.zeros_like(cres)
            rblk = int(sum((int(b) - 8) // 2 for b in np.diff(foff_h)))   # the reader is handed whole slots: frames with slack behind them
            cws = hip.frame_dbatch_workspace(len(sizes), nblk, 0, codec); dws = hip.frame_dbatch_workspace(len(sizes), rblk)

            def work():
                hip.frame_compress_dbatch(src, soff, 0, codec, dst=frames, dst_offsets=foff, max_total_blocks=nblk, workspace=cws, results=cres)
                hip.frame_decompress_dbatch(frames, foff, soff, dst=back, max_total_blocks=rblk, workspace=dws, results=dres)
            work(); torch.cuda.synchronize()                # one ordinary call first
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                       # torch's capture stream: not the default stream
                work()
            for trial in (1, 2):
                contents = make(trial)
                src.copy_(_dev(_cat(contents)))
                frames.zero_(); back.zero_()
                g.replay()
                torch.cuda.synchronize()
                fr, cr, dr, bk = frames.cpu().numpy(), cres.cpu().numpy(), dres.cpu().numpy(), back.cpu().numpy()
                at = 0
                for i, c in enumerate(contents):
                    ro, fo = oracle.frame_compress(c, 0, codec)
                    assert cr[i] == ro and (fr[int(foff_h[i]):int(foff_h[i]) + ro] == fo[:ro]).all(), (codec, trial, i)
                    assert dr[i] == len(c) and (bk[at:at + len(c)] == c).all(), (codec, trial, i)
                    at += len(c)
    finally:
        FseHip.guard = old

"""Predicted planes on the device (the six FSEHIP_*_pred_dbatch calls and the Python surface around PredictedPlanes) against the numpy model of
planes_pred_corpus.py -- the planes of zigzag(element - the element in front of it) in runs of 1024 elements -- and the CPU oracle's frames
of those planes; never against the library's own calls.  Block-size id 0 wherever frames are involved.  Every destination is filled with
0xA5 and has a tail behind it: whatever the contract does not give to the call must still be 0xA5 afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_mixed_corpus as fmc
import frame_packed_corpus as fpc
import planes_corpus as pc
import planes_pred_corpus as ppc
import planes_seg_corpus as pseg
from planes_corpus import CORRUPT, GENERIC, TILE, TOO_SMALL

pytestmark = pytest.mark.gpu

FILL, TAIL = 0xA5, 64
SHIFTS = ((0, 0), (1, 5), (8, 15), (3, 2))                  # two buffers, each off 16-byte alignment by an amount of its own
R = ppc.RUN
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _i64(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).cuda()


def _filled(n, shift=0, content=None):
    """n + TAIL bytes of FILL starting `shift` bytes behind an allocation's (256-byte aligned) start, the first bytes set to `content`"""
    t = torch.full((shift + n + TAIL,), FILL, dtype=torch.uint8, device="cuda")[shift:]
    if content is not None and len(content):
        t[:len(content)] = _dev(content)
    return t


def counts(E):
    """the element counts of the issue"""
    per = TILE // E
    return [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, per - 1, per, per + 1, 3 * per + 5]


def across(E, stride):
    """every ordered pair of edge values as neighbours across a boundary: pair k lies at the elements stride (k + 1) - 1 | stride (k + 1), on a
    smooth ramp.  stride 16: lane boundaries; 1024: run boundaries, and the merge's tile boundaries with them (a tile is 32 / E runs)"""
    vals = ppc.edge_values(E)
    pairs = [(x, y) for x in vals for y in vals]
    seq = (np.arange(stride * (len(pairs) + 1) + 3, dtype=np.uint64) * np.uint64(3)) & np.uint64((1 << (8 * E - 1)) - 1 if E < 8 else (1 << 40) - 1)
    for k, (x, y) in enumerate(pairs):
        seq[stride * (k + 1) - 1], seq[stride * (k + 1)] = x, y
    return seq.astype(ppc._U[E]).view(np.uint8).copy()


def _tensors(E):
    """every count of the issue as a tensor of whole elements (random bytes, and a smooth sequence for the larger ones) and again with
    n mod E != 0; sixty tensors of 0 .. 40 bytes that share a tile, so that what follows starts at odd addresses; the edge values as
    neighbours across lane, run and tile boundaries; and a tensor of several tiles behind the tiny ones"""
    if E not in _CACHE:
        rng = np.random.default_rng(600 + E)
        tensors = []
        for k, c in enumerate(counts(E)):
            tensors.append(rng.integers(0, 256, c * E, dtype=np.uint8))
            if E > 1:
                tensors.append(rng.integers(0, 256, c * E + 1 + k % (E - 1), dtype=np.uint8))
        tiny = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in rng.integers(0, 41, 60)]
        assert sum(len(t) for t in tiny) < TILE // 8
        tensors += tiny
        steps = rng.integers(-3, 4, 5 * TILE // E + 77).astype(np.int64)
        smooth = (np.cumsum(steps) + 1000).astype(np.uint64).astype(ppc._U[E]).view(np.uint8)
        tensors += [np.concatenate([smooth, np.arange(1, E, dtype=np.uint8)]), ppc.edge_sequence(E, 15), across(E, 16), across(E, 1024)]
        _CACHE[E] = tensors
    return _CACHE[E]


# ---------------------------------------------------------------------------------------------------------------- split
def run_split(hip, tensors, E, capacity=None, shift=(0, 0)):
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    src, planes = _filled(total, shift[0], pc.cat(tensors)), _filled(total, shift[1])
    poff = torch.full((n * E + 2,), -7, dtype=torch.int64, device="cuda")
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    hip.planes_split_pred_dbatch(src[:total], S, E, capacity=capacity, planes=planes, plane_offsets=poff, results=res)
    torch.cuda.synchronize()
    assert int(poff[n * E + 1]) == -7 and int(res[n]) == -7
    host = src.cpu().numpy()
    assert (host[:total] == pc.cat(tensors)).all() and (host[total:] == FILL).all(), "the source is only read"
    return planes.cpu().numpy(), poff.cpu().tolist()[:n * E + 1], res.cpu().tolist()[:n]


def check_split(got, tensors, E, capacity=None):
    out, poff, res = got
    want, written, P, wres = ppc.split_pred_model(tensors, E, capacity)
    assert poff == P and res == wres
    total = len(want)
    assert (out[:total][written] == want[written]).all(), np.nonzero((out[:total] != want) & written)[0][:8]
    outside = np.ones(len(out), bool)
    outside[:total] = ~written
    assert (out[outside] == FILL).all(), ("bytes outside the accepted tensors' planes", np.nonzero((out != FILL) & outside)[0][:8])


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_pred_against_the_model(hip, E):
    tensors = _tensors(E)
    sizes = [len(t) for t in tensors]
    assert all(c * E in sizes for c in counts(E)) and (E == 1 or all(any(c * E < s < (c + 1) * E for s in sizes) for c in counts(E)))
    assert sum(1 for s in sizes if s <= 40) >= 60 and max(sizes) > 5 * TILE
    for shift in SHIFTS:
        check_split(run_split(hip, tensors, E, shift=shift), tensors, E)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_pred_with_a_short_capacity(hip, E):
    tensors = _tensors(E)
    S = [int(x) for x in pc.offsets(tensors)]
    k = next(i for i, t in enumerate(tensors) if len(t) == TILE)
    for cap in (S[k] + 100, S[k + 1], S[k + 1] - 1, S[6], 0):  # inside a tensor, at a tensor's end, one short of it, at an early end, nothing
        got = run_split(hip, tensors, E, capacity=cap, shift=SHIFTS[1])
        check_split(got, tensors, E, cap)
        first = next(i for i in range(len(tensors)) if S[i + 1] > cap)
        assert got[2][first:] == [GENERIC] * (len(tensors) - first) and got[1][first * E:] == [S[first]] * (len(got[1]) - first * E)
        assert (got[0][S[first]:] == FILL).all(), "nothing of a refused tensor is written"


# ---------------------------------------------------------------------------------------------------------------- merge
def run_merge(hip, E, planes_buf, poff, psizes, D, capacity=None, shift=(0, 0)):
    n, room = len(D) - 1, int(D[-1])
    planes = _filled(len(planes_buf), shift[0], planes_buf)
    dst = _filled(room, shift[1])
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    out, _ = hip.planes_merge_pred_dbatch(planes[:max(len(planes_buf), 1)], _i64(poff), _i64(psizes), np.asarray(D, np.uint64), E, dst=dst,
                                          capacity=room if capacity is None else capacity, results=res)
    torch.cuda.synchronize()
    assert int(res[n]) == -7 and out.data_ptr() == dst.data_ptr()
    host = planes.cpu().numpy()
    assert (host[:len(planes_buf)] == planes_buf).all() and (host[len(planes_buf):] == FILL).all(), "the planes are only read"
    return dst.cpu().numpy(), res.cpu().tolist()[:n]


def check_merge(got, tensors, E, psizes, D, capacity):
    out, res = got
    want = [pc.merge_verdict(psizes[i * E:(i + 1) * E], int(D[i + 1]), int(D[i]), E, capacity) for i in range(len(tensors))]
    assert res == want
    written = np.zeros(len(out), bool)
    for i, raw in enumerate(tensors):
        if want[i] >= 0:
            assert want[i] == len(raw)
            assert (out[int(D[i]):int(D[i]) + len(raw)] == raw).all(), (i, len(raw), np.nonzero(out[int(D[i]):int(D[i]) + len(raw)] != raw)[0][:8])
            written[int(D[i]):int(D[i]) + len(raw)] = True
    assert (out[~written] == FILL).all(), ("bytes outside the good tensors", np.nonzero((out != FILL) & ~written)[0][:8])
    return want


@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_pred_against_the_model(hip, E):
    tensors = _tensors(E)
    buf, _, P, _ = ppc.split_pred_model(tensors, E)
    psizes = [pc.plane_size(len(t), p, E) for t in tensors for p in range(E)]
    D = [int(x) for x in pc.offsets(tensors)]
    for shift in SHIFTS:
        got = run_merge(hip, E, buf, P[:-1], psizes, D, shift=shift)
        assert check_merge(got, tensors, E, psizes, D, D[-1]) == [len(t) for t in tensors]


@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_pred_refusals_and_slots_with_room(hip, E):
    tensors = _tensors(E)
    n = len(tensors)
    sizes = [len(t) for t in tensors]
    behind, failed, wrong, short = n - 1, sizes.index(TILE), sizes.index(1025 * E), sizes.index(1023 * E)    # one tensor per rule, in the header's order
    slots = [s + (i % 3) for i, s in enumerate(sizes)]        # slots with some room to spare ...
    slots[short] = sizes[short] - 1                           # ... and one a byte short
    D = [0]
    for s in slots:
        D.append(D[-1] + s)
    buf, _, P, _ = ppc.split_pred_model(tensors, E)
    psizes = [pc.plane_size(s, p, E) for s in sizes for p in range(E)]
    if E > 1:
        psizes[wrong * E] -= 1; psizes[wrong * E + 1] += 1     # the same total, not the planes of one tensor
    else:
        wrong = None
    if E >= 4:
        psizes[failed * E + 1], psizes[failed * E + 3], first = -3, -4, -3
    elif E == 2:
        psizes[failed * E], psizes[failed * E + 1], first = -3, -4, -3
    else:
        psizes[failed * E], first = -3, -3
    cap = D[n] - 1                                             # the last slot ends behind the capacity
    got = run_merge(hip, E, buf, P[:-1], psizes, D, capacity=cap, shift=SHIFTS[2])
    want = check_merge(got, tensors, E, psizes, D, cap)
    assert want[behind] == GENERIC and want[failed] == first and (wrong is None or want[wrong] == CORRUPT) and want[short] == TOO_SMALL
    assert len([w for w in want if w < 0]) == (4 if wrong is not None else 3)


# ---------------------------------------------------------------------------------------------------------------- composites
def _corpus(E):
    """sorted indices, random bytes over a run and an element, nothing, a smooth tensor whose size is no multiple of E, the edge values as
    neighbours, a constant"""
    key = ("comp", E)
    if key not in _CACHE:
        rng = np.random.default_rng(300 + E)
        top = (1 << (8 * E - 1)) if E < 8 else 1 << 50
        idx = np.sort(rng.integers(0, top, 3000).astype(np.uint64)).astype(ppc._U[E]).view(np.uint8)
        smooth = (np.cumsum(rng.integers(-2, 3, 2500)) + 500).astype(np.uint64).astype(ppc._U[E]).view(np.uint8)
        _CACHE[key] = [idx, rng.integers(0, 256, 1025 * E, dtype=np.uint8), np.zeros(0, np.uint8), np.concatenate([smooth, np.arange(1, E, dtype=np.uint8)]),
                       ppc.edge_sequence(E, 15), np.tile(np.arange(7, 7 + E, dtype=np.uint8), 2100)]
    return _CACHE[key]


def _frames(oracle, units, codec):
    return [f[:r].copy() for u in units for r, f in [oracle.frame_compress(np.ascontiguousarray(u), 0, codec)]]


def _plane_frames(oracle, E, codec):
    key = ("frames", E, codec)
    if key not in _CACHE:
        _CACHE[key] = _frames(oracle, [pl for x in ppc.pred_all(_corpus(E), E) for pl in pc.planes_of(x, E)], codec)
    return _CACHE[key]


def run_compress(hip, tensors, E, codec, align_log, shift=(0, 0)):
    """codec 0 / 1, or an AutoCodec"""
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, align_log)
    dst, src, planes = _filled(fcap), _filled(total, shift[0], pc.cat(tensors)), _filled(total, shift[1])
    _, foff, fres, tres, chosen = hip.tensor_compress_pred_dbatch(src[:total], S, E, codec=codec, block_size_id=0, dst=dst, dst_capacity=fcap, max_total_blocks=blocks,
                                                                  align_log=align_log, planes=planes)
    torch.cuda.synchronize()
    assert (planes.cpu().numpy()[total:] == FILL).all() and (src.cpu().numpy()[:total] == pc.cat(tensors)).all()
    return dst, foff, fres, tres, fcap, (None if chosen is None else chosen.cpu().tolist())


def check_frames(want, dst, foff, fres, align_log, fcap, what):
    sizes = [len(w) for w in want]
    off, res, out = foff.cpu().tolist(), fres.cpu().tolist(), dst.cpu().numpy()
    assert off == fpc.packed_offsets(sizes, align_log, fcap), what
    assert res == fpc.packed_results(sizes, align_log, fcap) == sizes, what
    written = np.zeros(len(out), bool)
    for i, w in enumerate(want):
        assert (out[off[i]:off[i] + res[i]] == w).all(), (what, i)
        written[off[i]:off[i] + res[i]] = True
    assert (out[~written] == FILL).all(), (what, "bytes outside the frames", np.nonzero((out != FILL) & ~written)[0][:8])


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_tensor_compress_pred_gives_the_oracles_frame_of_every_predicted_plane(hip, checker, E, codec):
    tensors, want = _corpus(E), _plane_frames(checker, E, codec)
    assert len(tensors[2]) == 0 and len(tensors[3]) % E == E - 1 and len(want) == len(tensors) * E
    assert codec == 1 or all(len(f) < 64 for f in want[5 * E:]), "a constant tensor under FSE: a few bytes per block and plane"
    for align_log, shift in ((0, SHIFTS[1]), (8, SHIFTS[2])):
        dst, foff, fres, tres, fcap, chosen = run_compress(hip, tensors, E, codec, align_log, shift)
        assert chosen is None and tres.cpu().tolist() == [len(t) for t in tensors]
        check_frames(want, dst, foff, fres, align_log, fcap, (E, codec, align_log))


@pytest.mark.parametrize("E", pc.ELEMS)
def test_tensor_compress_pred_with_an_autocodec(hip, checker, E):
    from finitestateentropy_amd.api import AutoCodec
    tensors, F, H = _corpus(E), _plane_frames(checker, E, 0), _plane_frames(checker, E, 1)
    tol = 20
    dst, foff, fres, tres, fcap, chosen = run_compress(hip, tensors, E, AutoCodec(tol), 0)
    want = [fmc.expected_choice(len(f), len(h), tol)[0] for f, h in zip(F, H)]
    assert chosen == want, "the choice per plane is the mixed model's"
    check_frames([H[q] if c else F[q] for q, c in enumerate(want)], dst, foff, fres, 0, fcap, E)
    assert tres.cpu().tolist() == [len(t) for t in tensors]


def run_decompress(hip, frames, foff, D, E, blocks, shift=0):
    total = int(D[-1])
    back = _filled(total, shift)
    res = torch.full((len(D) - 1,), -7, dtype=torch.int64, device="cuda")
    hip.tensor_decompress_pred_dbatch(frames, foff, np.asarray(D, np.uint64), E, dst=back, dst_capacity=total, max_total_blocks=blocks, results=res)
    torch.cuda.synchronize()
    return back.cpu().numpy(), res.cpu().tolist()


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_tensor_decompress_pred_and_a_damaged_frame(hip, checker, E, codec):
    tensors, want = _corpus(E), _plane_frames(checker, E, codec)
    n, D = len(tensors), [int(x) for x in pc.offsets(tensors)]
    blocks = hip.planes_block_bound(D[-1], n, E, 0)
    dst, foff, fres, _, fcap, _ = run_compress(hip, tensors, E, codec, 0)
    check_frames(want, dst, foff, fres, 0, fcap, "the frames of the compress test")
    for shift in (0, 7):
        back, res = run_decompress(hip, dst, foff, D, E, blocks, shift)
        assert res == [len(t) for t in tensors]
        assert (back[:D[-1]] == pc.cat(tensors)).all() and (back[D[-1]:] == FILL).all()
    # one payload byte of one plane's frame flipped (tensor 1, random bytes: full 1 KB blocks): that tensor gets what the oracle's reader says of
    # that frame and is not written -- the fill pattern stays; every other tensor is right
    victim, plane = 1, E - 1
    f = victim * E + plane
    at = 5 + 3 + 40                                            # behind the frame's and the first block's header
    assert len(want[f]) > at + 8
    bad = want[f].copy()
    bad[at] ^= 0x55
    r, _ = checker.frame_decompress(bad, len(tensors[victim][plane::E]))
    assert r > (1 << 63), "the oracle's reader refuses the damaged frame"
    dst[int(foff[f]) + at] ^= 0x55
    back, res = run_decompress(hip, dst, foff, D, E, blocks, 3)
    assert res == [len(tensors[0]), r - (1 << 64)] + [len(t) for t in tensors[2:]]
    assert (back[D[victim]:D[victim + 1]] == FILL).all(), "a damaged frame leaves its tensor unwritten"
    assert (back[:D[victim]] == pc.cat(tensors[:victim])).all() and (back[D[victim + 1]:D[-1]] == pc.cat(tensors[victim + 1:])).all()
    assert (back[D[-1]:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- segments
def _seg_corpus(E, seg_log):
    """a smooth tensor over two segments and a bit, nothing, the edge values over exactly one segment per plane, random bytes of a size that is
    no multiple of E one element above a segment, sorted values over two segments and a half"""
    key = ("seg", E, seg_log)
    if key not in _CACHE:
        s = 1 << seg_log
        rng = np.random.default_rng(60 + E + seg_log)
        smooth = (np.cumsum(rng.integers(-2, 3, 2 * s + 100)) + 500).astype(np.uint64).astype(ppc._U[E]).view(np.uint8)
        edge = np.tile(ppc.edge_sequence(E, 0), -(-s * E // len(ppc.edge_sequence(E, 0))))[:E * s]
        top = (1 << (8 * E - 1)) if E < 8 else 1 << 50
        idx = np.sort(rng.integers(0, top, 5 * s // 2).astype(np.uint64)).astype(ppc._U[E]).view(np.uint8)
        _CACHE[key] = [smooth, np.zeros(0, np.uint8), edge, rng.integers(0, 256, E * (s + 1) + E - 1, dtype=np.uint8), idx]
    return _CACHE[key]


def _segments_of(tensors, E, seg_log):
    out = []
    for t in tensors:
        for pl in pc.planes_of(t, E):
            out += [np.ascontiguousarray(pl[a:a + (1 << seg_log)]) for a in (range(0, len(pl), 1 << seg_log) if len(pl) else [0])]
    return out


@pytest.mark.parametrize("seg_log", [10, 11])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_segmented_pred_frames_and_full_read_with_one_codec_and_with_choose(hip, checker, E, seg_log):
    from finitestateentropy_amd.api import AutoCodec
    tensors = _seg_corpus(E, seg_log)
    sizes = [len(t) for t in tensors]
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    first = pseg.seg_first(sizes, E, seg_log)
    units = _segments_of(ppc.pred_all(tensors, E), E, seg_log)
    F, H = _frames(checker, units, 0), _frames(checker, units, 1)
    assert len(F) == first[-1] > 5 * E
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, first[-1], blocks, 0)
    tol = 20
    choice = [fmc.expected_choice(len(f), len(h), tol)[0] for f, h in zip(F, H)]
    for codec, want in ((0, F), (1, H), (AutoCodec(tol), [H[q] if c else F[q] for q, c in enumerate(choice)])):
        dst, src, planes = _filled(fcap), _filled(total, 5, pc.cat(tensors)), _filled(total, 9)
        _, foff, fres, tres, chosen = hip.tensor_compress_seg_pred_dbatch(src[:total], S, E, seg_log, np.asarray(first, np.uint64), codec=codec, block_size_id=0, dst=dst,
                                                                          dst_capacity=fcap, max_total_blocks=blocks, planes=planes)
        torch.cuda.synchronize()
        assert tres.cpu().tolist() == sizes and (chosen is None if codec in (0, 1) else chosen.cpu().tolist() == choice)
        check_frames(want, dst, foff, fres, 0, fcap, (E, seg_log, codec))
        back = _filled(total, 11)
        _, res = hip.tensor_decompress_seg_pred_dbatch(dst, foff, S, E, seg_log, np.asarray(first, np.uint64), dst=back, dst_capacity=total, max_total_blocks=blocks)
        torch.cuda.synchronize()
        out = back.cpu().numpy()
        assert res.cpu().tolist() == sizes and (out[:total] == pc.cat(tensors)).all() and (out[total:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- graph
def test_pred_compress_and_decompress_in_one_hip_graph(hip, checker):
    """one captured graph -- a single stream, a linear chain -- holding the predicted compress and then the predicted decompress; replayed once
    over a changed source"""
    E, codec, ALIGN = 4, 0, 4
    sizes = [len(t) for t in _corpus(E)]
    n, S = len(sizes), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(S[-1])

    def source(seed):                                          # sorted values of the corpus' sizes
        rng = np.random.default_rng(seed)
        return [np.concatenate([np.sort(rng.integers(0, 1 << 28, s // E).astype("<u4")).view(np.uint8), np.arange(s % E, dtype=np.uint8)]) for s in sizes]
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, ALIGN)
    wsize, rsize = hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize, hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    wsize.restype = rsize.restype = C.c_size_t
    wws = torch.empty(int(wsize(C.c_size_t(n * E), C.c_size_t(blocks), C.c_uint(0), C.c_int(codec))), dtype=torch.uint8, device="cuda")
    rws = torch.empty(int(rsize(C.c_size_t(n * E), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
    src = torch.zeros(total, dtype=torch.uint8, device="cuda")
    soff = _i64(S)
    frames, back, planes, planes2 = _filled(fcap), _filled(total), _filled(total), _filled(total)
    foff, poff, poff2 = (torch.zeros(n * E + 1, dtype=torch.int64, device="cuda") for _ in range(3))
    fres, pres = (torch.zeros(n * E, dtype=torch.int64, device="cuda") for _ in range(2))
    tres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))

    def work():
        hip.tensor_compress_pred_dbatch(src, soff, E, codec=codec, block_size_id=0, dst=frames, dst_capacity=fcap, max_total_blocks=blocks, align_log=ALIGN,
                                        frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, workspace=wws)
        hip.tensor_decompress_pred_dbatch(frames, foff, soff, E, dst=back, dst_capacity=total, max_total_blocks=blocks, planes=planes2, planes_capacity=total,
                                          plane_offsets=poff2, plane_results=pres, workspace=rws, results=rres)
    src.copy_(_dev(pc.cat(source(0)))); work(); torch.cuda.synchronize()      # one ordinary call first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    tensors = source(1)
    assert not (pc.cat(tensors) == pc.cat(source(0))).all()
    src.copy_(_dev(pc.cat(tensors)))
    for t in (frames, back):
        t.fill_(FILL)
    for t in (foff, fres, tres, rres):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    want = _frames(checker, [pl for x in ppc.pred_all(tensors, E) for pl in pc.planes_of(x, E)], codec)
    check_frames(want, frames, foff, fres, ALIGN, fcap, "replay")
    assert tres.cpu().tolist() == rres.cpu().tolist() == sizes
    out = back.cpu().numpy()
    assert (out[:total] == pc.cat(tensors)).all() and (out[total:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- Python
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_predicted_planes_through_the_python_surface_and_an_archive(hip, checker, monkeypatch):
    from finitestateentropy_amd.api import AutoCodec, PredictedPlanes
    gen = torch.Generator(device="cuda").manual_seed(17)
    idx = torch.sort(torch.randint(0, 1 << 22, (40000,), generator=gen, device="cuda", dtype=torch.int32)).values
    field = torch.sin(torch.linspace(0, 40, 30000, device="cuda")) + 1e-4 * torch.randn(30000, generator=gen, device="cuda")
    offsets = torch.cumsum(torch.randint(0, 60, (3, 1100), generator=gen, device="cuda", dtype=torch.int64).reshape(-1), 0).reshape(3, 1100)
    audio = (torch.cumsum(torch.randint(-40, 41, (5000,), generator=gen, device="cuda"), 0)).to(torch.int16)
    image = torch.cumsum(torch.randint(-3, 4, (7, 333), generator=gen, device="cuda"), 1).to(torch.uint8)
    weights = (torch.randn((64, 33), generator=gen, device="cuda") * 0.02).to(torch.bfloat16)
    nan = torch.tensor([0x7FF8000000000001, -0x0010000000000000 + 2, 5], dtype=torch.int64, device="cuda").view(torch.float64)
    empty = torch.zeros((0, 3), device="cuda", dtype=torch.float32)
    ts = [idx, field, offsets, audio, image, weights, nan, empty]
    keep = [t.clone() for t in ts]
    obj = hip.compress_tensors(ts, codec=PredictedPlanes(1))
    assert obj.predictor == "prev" and obj.codec == PredictedPlanes(1) and obj.delta is False and obj.segment_log is None and obj.sparse_permille is None
    assert sorted(g["elem_bytes"] for g in obj.groups) == [1, 2, 4, 8]
    # the frames are the oracle's Huff0 frames of the model's planes, at the default block-size id
    for g in obj.groups:
        E = g["elem_bytes"]
        raws = [ts[i].contiguous().reshape(-1).view(torch.uint8).cpu().numpy() for i in g["index"]]
        off, res, out = g["frame_offsets"].cpu().tolist(), g["frame_results"].cpu().tolist(), g["frames"].cpu().numpy()
        q = 0
        for x in ppc.pred_all(raws, E):
            for pl in pc.planes_of(x, E):
                r, f = checker.frame_compress(np.ascontiguousarray(pl), 5, 1)
                assert res[q] == r and (out[off[q]:off[q] + r] == f[:r]).all(), (E, q)
                q += 1
    back = hip.decompress_tensors(obj)
    for a, b, k in zip(ts, back, keep):
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and _bits(a, b) and _bits(a, k)
    plain = hip.compress_tensors(ts, codec=1)
    print("mixed dtypes, %d bytes: Huff0 frames of the plain planes %d, of the predicted planes %d" % (sum(t.numel() * t.element_size() for t in ts), plain.nbytes,
                                                                                                       obj.nbytes))
    assert plain.predictor is None and 0 < obj.nbytes < plain.nbytes
    # through an archive and back: the codec travels in the meta JSON, the C head is that of a plain object
    buf = hip.archive_tensors(obj)
    info = hip.archive_inspect(buf[:64].cpu().numpy(), buf.numel())
    assert info.flags == 0 and info.deltaOp == 0 and info.sparsePermille == 0 and info.segLog == 0
    opened = hip.open_archive(buf)
    assert opened.predictor == "prev" and opened.codec == PredictedPlanes(1) and vars(opened)["predictor"] == "prev"
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(opened), ts))
    assert hip.open_archive(hip.archive_tensors(plain)).predictor is None
    # an AutoCodec inside, an earlier object given back as codec, and the segmented calls
    auto = hip.compress_tensors(ts, PredictedPlanes(AutoCodec(10)))
    again = hip.compress_tensors(ts, auto)
    assert auto.predictor == again.predictor == "prev" and all("codecs" in g for g in auto.groups)
    for g, h in zip(auto.groups, again.groups):
        assert torch.equal(g["frames"], h["frames"]) and torch.equal(g["codecs"], h["codecs"])
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(again), ts))
    seg = hip.compress_tensors_segmented(ts, 15, PredictedPlanes(0))
    assert seg.predictor == "prev" and seg.segment_log == 15
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(seg), ts))
    reopened = hip.open_archive(hip.archive_tensors(seg))
    assert reopened.predictor == "prev" and reopened.segment_log == 15 and reopened.codec == PredictedPlanes(0)
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(reopened), ts))

    # every refusal is raised before a launch: from here on a call into the library is a failure of the test
    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in ("FSEHIP_planes_split_pred_dbatch", "FSEHIP_planes_merge_pred_dbatch", "FSEHIP_tensor_compress_pred_dbatch", "FSEHIP_tensor_decompress_pred_dbatch",
                 "FSEHIP_tensor_compress_seg_pred_dbatch", "FSEHIP_tensor_decompress_seg_pred_dbatch", "FSEHIP_tensor_compress_dbatch", "FSEHIP_tensor_compress_delta_dbatch",
                 "FSEHIP_tensor_compress_seg_dbatch", "FSEHIP_tensor_decompress_window_dbatch", "FSEHIP_tensor_patch_window_dbatch"):
        monkeypatch.setattr(hip.lib, name, no_launch)
    with pytest.raises(ValueError):
        hip.compress_tensors(ts, PredictedPlanes(1), base=keep)
    with pytest.raises(ValueError):
        hip.compress_tensors_segmented(ts, 15, PredictedPlanes(0), base=keep)
    wins = [(0, 10)] * (len(ts) - 1) + [(0, 0)]
    for o in (seg, reopened, obj):
        with pytest.raises(ValueError):
            hip.decompress_tensor_windows(o, wins)
        with pytest.raises(ValueError):
            hip.patch_tensor_windows(o, ts, wins)
    with pytest.raises(ValueError):
        hip.decompress_tensors(obj, base=keep)

"""Strided predicted planes on the device (the six FSEHIP_*_pred_stride_dbatch calls and the Python surface around
PredictedPlanes(codec, stride)) against the numpy model of planes_stride_corpus.py -- the planes of zigzag(element - the element S in front
of it) in runs of 1024 elements, the chains restarting with every run -- and the CPU oracle's frames of those planes; never against the
library's own calls, except where stride 1 is held against the *_pred_dbatch calls it must equal.  Block-size id 0 wherever frames are
involved.  Every destination is filled with 0xA5 and has a tail behind it: whatever the contract does not give to the call must still be
0xA5 afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_mixed_corpus as fmc
import frame_packed_corpus as fpc
import planes_corpus as pc
import planes_seg_corpus as pseg
import planes_stride_corpus as sc
from planes_corpus import CORRUPT, GENERIC, TILE, TOO_SMALL

pytestmark = pytest.mark.gpu

FILL, TAIL = 0xA5, 64
SHIFTS = ((1, 5), (8, 15), (3, 2), (13, 7), (0, 9))         # two buffers, each off 16-byte alignment by an amount of its own
STRIDES = sc.STRIDES[1:]                                    # 2 .. 8: stride 1 launches the kernels of the predicted planes (the last section)
R = sc.RUN
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
    return [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025, 1032, 2047, 2048, 2049, per - 1, per, per + 1, 3 * per + 5]


def _base(E):
    """every count of the issue as a tensor of whole elements (random bytes) and again with n mod E != 0; sixty tensors of 0 .. 40 bytes that
    share a tile, so that what follows starts at odd addresses; and an interleaved smooth tensor of several tiles behind the tiny ones"""
    if E not in _CACHE:
        rng = np.random.default_rng(700 + E)
        tensors = []
        for k, c in enumerate(counts(E)):
            tensors.append(rng.integers(0, 256, c * E, dtype=np.uint8))
            if E > 1:
                tensors.append(rng.integers(0, 256, c * E + 1 + k % (E - 1), dtype=np.uint8))
        tiny = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in rng.integers(0, 41, 60)]
        assert sum(len(t) for t in tiny) < TILE // 8
        tensors += tiny
        steps = rng.integers(-3, 4, 5 * TILE // E + 77).astype(np.int64)
        smooth = (np.cumsum(steps) + 1000).astype(np.uint64).astype(sc._U[E]).view(np.uint8)
        tensors.append(np.concatenate([smooth, np.arange(1, E, dtype=np.uint8)]))
        _CACHE[E] = tensors
    return _CACHE[E]


def _tensors(E, S):
    """... and for the stride: the edge values as stride-neighbours across lane and run boundaries (the merge's tile boundaries among the
    latter), and the constant channels over four runs and a bit"""
    key = (E, S)
    if key not in _CACHE:
        _CACHE[key] = _base(E) + [sc.across(E, S, 16), sc.across(E, S, R), sc.channels(E, S, 4 * R + 7)]
    return _CACHE[key]


def _split_model(E, S):
    key = ("split", E, S)
    if key not in _CACHE:
        _CACHE[key] = sc.split_model(_tensors(E, S), E, S)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------- split
def run_split(hip, tensors, E, S, capacity=None, shift=(0, 0)):
    n, off = len(tensors), pc.offsets(tensors)
    total = int(off[-1])
    src, planes = _filled(total, shift[0], pc.cat(tensors)), _filled(total, shift[1])
    poff = torch.full((n * E + 2,), -7, dtype=torch.int64, device="cuda")
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    hip.planes_split_pred_stride_dbatch(src[:total], off, E, S, capacity=capacity, planes=planes, plane_offsets=poff, results=res)
    torch.cuda.synchronize()
    assert int(poff[n * E + 1]) == -7 and int(res[n]) == -7
    host = src.cpu().numpy()
    assert (host[:total] == pc.cat(tensors)).all() and (host[total:] == FILL).all(), "the source is only read"
    return planes.cpu().numpy(), poff.cpu().tolist()[:n * E + 1], res.cpu().tolist()[:n]


def check_split(got, model):
    out, poff, res = got
    want, written, P, wres = model
    assert poff == P and res == wres
    total = len(want)
    assert (out[:total][written] == want[written]).all(), np.nonzero((out[:total] != want) & written)[0][:8]
    outside = np.ones(len(out), bool)
    outside[:total] = ~written
    assert (out[outside] == FILL).all(), ("bytes outside the accepted tensors' planes", np.nonzero((out != FILL) & outside)[0][:8])


@pytest.mark.parametrize("S", STRIDES)
@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_against_the_model(hip, E, S):
    tensors = _tensors(E, S)
    sizes = [len(t) for t in tensors]
    assert all(c * E in sizes for c in counts(E)) and (E == 1 or all(any(c * E < s < (c + 1) * E for s in sizes) for c in counts(E)))
    assert sum(1 for s in sizes if s <= 40) >= 60 and max(sizes) > 5 * TILE
    for shift in (SHIFTS[S % 5], SHIFTS[(S + E) % 5]):
        check_split(run_split(hip, tensors, E, S, shift=shift), _split_model(E, S))


@pytest.mark.parametrize("S", STRIDES)
@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_with_a_short_capacity(hip, E, S):
    tensors = _tensors(E, S)
    off = [int(x) for x in pc.offsets(tensors)]
    k = next(i for i, t in enumerate(tensors) if len(t) == TILE)
    for cap in (off[k] + 100, off[k + 1] - 1, off[6], 0):     # inside a tensor, one short of a tensor's end, at an early end, nothing
        got = run_split(hip, tensors, E, S, capacity=cap, shift=SHIFTS[(S + 1) % 5])
        check_split(got, sc.split_model(tensors, E, S, cap))
        first = next(i for i in range(len(tensors)) if off[i + 1] > cap)
        assert got[2][first:] == [GENERIC] * (len(tensors) - first) and got[1][first * E:] == [off[first]] * (len(got[1]) - first * E)
        assert (got[0][off[first]:] == FILL).all(), "nothing of a refused tensor is written"


# ---------------------------------------------------------------------------------------------------------------- merge
def run_merge(hip, E, S, planes_buf, poff, psizes, D, capacity=None, shift=(0, 0)):
    n, room = len(D) - 1, int(D[-1])
    planes = _filled(len(planes_buf), shift[0], planes_buf)
    dst = _filled(room, shift[1])
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    out, _ = hip.planes_merge_pred_stride_dbatch(planes[:max(len(planes_buf), 1)], _i64(poff), _i64(psizes), np.asarray(D, np.uint64), E, S, dst=dst,
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


@pytest.mark.parametrize("S", STRIDES)
@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_against_the_model(hip, E, S):
    tensors = _tensors(E, S)
    buf, _, P, _ = _split_model(E, S)
    psizes = [pc.plane_size(len(t), p, E) for t in tensors for p in range(E)]
    D = [int(x) for x in pc.offsets(tensors)]
    for shift in (SHIFTS[(S + 2) % 5], SHIFTS[(S + E + 1) % 5]):
        got = run_merge(hip, E, S, buf, P[:-1], psizes, D, shift=shift)
        assert check_merge(got, tensors, E, psizes, D, D[-1]) == [len(t) for t in tensors]


@pytest.mark.parametrize("S", STRIDES)
@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_refusals_and_slots_with_room(hip, E, S):
    tensors = _tensors(E, S)
    n = len(tensors)
    sizes = [len(t) for t in tensors]
    behind, failed, wrong, short = n - 1, sizes.index(TILE), sizes.index(1025 * E), sizes.index(1023 * E)    # one tensor per rule, in the header's order
    slots = [s + (i % 3) for i, s in enumerate(sizes)]        # slots with some room to spare ...
    slots[short] = sizes[short] - 1                           # ... and one a byte short
    D = [0]
    for s in slots:
        D.append(D[-1] + s)
    buf, _, P, _ = _split_model(E, S)
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
    got = run_merge(hip, E, S, buf, P[:-1], psizes, D, capacity=cap, shift=SHIFTS[(S + 3) % 5])
    want = check_merge(got, tensors, E, psizes, D, cap)
    assert want[behind] == GENERIC and want[failed] == first and (wrong is None or want[wrong] == CORRUPT) and want[short] == TOO_SMALL
    assert len([w for w in want if w < 0]) == (4 if wrong is not None else 3)


@pytest.mark.parametrize("S", STRIDES)
@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_chains_restart_with_every_run_on_the_device(hip, E, S):
    """one tensor of 4 * 1024 + 7 elements whose channel c holds c + 1 everywhere: planes that are zero except the first S elements of every
    run, and the merge returns the tensor -- a chain phase carried across a run (S = 3, 5, 6, 7: 1024 mod S != 0) shows in both"""
    raw = sc.channels(E, S, 4 * R + 7)
    m = len(raw) // E
    out, poff, res = run_split(hip, [raw], E, S, shift=SHIFTS[S % 5])
    assert res == [len(raw)] and poff == [p * m for p in range(E + 1)]
    z = np.zeros(m, np.uint64)
    for p in range(E):
        z |= out[p * m:(p + 1) * m].astype(np.uint64) << np.uint64(8 * p)
    j = np.arange(m)
    head = j % R < S
    assert (z[~head] == 0).all(), ("a non-zero difference inside a run", np.nonzero((z != 0) & ~head)[0][:8])
    assert (z[head] == 2 * ((j[head] % S) + 1)).all(), "a chain head is coded as zigzag(t)"
    back, mres = run_merge(hip, E, S, out[:len(raw)], poff[:-1], [m] * E, [0, len(raw)], shift=SHIFTS[(S + 1) % 5])
    assert mres == [len(raw)] and (back[:len(raw)] == raw).all() and (back[len(raw):] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- composites
CSTRIDES = (2, 3)


def _corpus(E, S):
    """interleaved walks, random bytes over a run and an element, nothing, a smooth tensor whose size is no multiple of E, the edge values as
    stride-neighbours across lanes, the constant channels"""
    key = ("comp", E, S)
    if key not in _CACHE:
        rng = np.random.default_rng(300 + 10 * E + S)
        walks = (np.cumsum(rng.integers(-2, 3, (1000, S)), axis=0) + 500 * np.arange(1, S + 1)).reshape(-1)
        smooth = (np.cumsum(rng.integers(-2, 3, 2500)) + 500).astype(np.uint64).astype(sc._U[E]).view(np.uint8)
        _CACHE[key] = [walks.astype(np.uint64).astype(sc._U[E]).view(np.uint8).copy(), rng.integers(0, 256, 1025 * E, dtype=np.uint8), np.zeros(0, np.uint8),
                       np.concatenate([smooth, np.arange(1, E, dtype=np.uint8)]), sc.across(E, S, 16)[:E * 16 * 20], sc.channels(E, S, 2100)]
    return _CACHE[key]


def _frames(oracle, units, codec):
    return [f[:r].copy() for u in units for r, f in [oracle.frame_compress(np.ascontiguousarray(u), 0, codec)]]


def _plane_frames(oracle, E, S, codec):
    key = ("frames", E, S, codec)
    if key not in _CACHE:
        _CACHE[key] = _frames(oracle, [pl for x in sc.pred_all(_corpus(E, S), E, S) for pl in pc.planes_of(x, E)], codec)
    return _CACHE[key]


def run_compress(hip, tensors, E, S, codec, align_log, shift=(0, 0)):
    """codec 0 / 1, or an AutoCodec"""
    n, off = len(tensors), pc.offsets(tensors)
    total = int(off[-1])
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, align_log)
    dst, src, planes = _filled(fcap), _filled(total, shift[0], pc.cat(tensors)), _filled(total, shift[1])
    _, foff, fres, tres, chosen = hip.tensor_compress_pred_stride_dbatch(src[:total], off, E, S, codec=codec, block_size_id=0, dst=dst, dst_capacity=fcap,
                                                                         max_total_blocks=blocks, align_log=align_log, planes=planes)
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


def run_decompress(hip, frames, foff, D, E, S, blocks, shift=0):
    total = int(D[-1])
    back = _filled(total, shift)
    res = torch.full((len(D) - 1,), -7, dtype=torch.int64, device="cuda")
    hip.tensor_decompress_pred_stride_dbatch(frames, foff, np.asarray(D, np.uint64), E, S, dst=back, dst_capacity=total, max_total_blocks=blocks, results=res)
    torch.cuda.synchronize()
    return back.cpu().numpy(), res.cpu().tolist()


@pytest.mark.parametrize("S", CSTRIDES)
@pytest.mark.parametrize("E", pc.ELEMS)
def test_compress_gives_the_oracles_frames_and_decompress_survives_a_damaged_frame(hip, checker, E, S):
    from finitestateentropy_amd.api import AutoCodec
    tensors, F, H = _corpus(E, S), _plane_frames(checker, E, S, 0), _plane_frames(checker, E, S, 1)
    n, D = len(tensors), [int(x) for x in pc.offsets(tensors)]
    assert len(tensors[2]) == 0 and len(tensors[3]) % E == E - 1 and len(F) == n * E
    blocks = hip.planes_block_bound(D[-1], n, E, 0)
    codec = (E + S) % 2                                        # one codec per case, both over the cases
    want = H if codec else F
    dst, foff, fres, tres, fcap, chosen = run_compress(hip, tensors, E, S, codec, 8, SHIFTS[1])
    assert chosen is None and tres.cpu().tolist() == [len(t) for t in tensors]
    check_frames(want, dst, foff, fres, 8, fcap, (E, S, codec))
    for shift in (0, 7):
        back, res = run_decompress(hip, dst, foff, D, E, S, blocks, shift)
        assert res == [len(t) for t in tensors]
        assert (back[:D[-1]] == pc.cat(tensors)).all() and (back[D[-1]:] == FILL).all()
    # CHOOSE: the choice per plane is the mixed model's over the oracle's two frames
    tol = 20
    cdst, cfoff, cfres, ctres, cfcap, chosen = run_compress(hip, tensors, E, S, AutoCodec(tol), 0, SHIFTS[2])
    choice = [fmc.expected_choice(len(f), len(h), tol)[0] for f, h in zip(F, H)]
    assert chosen == choice and ctres.cpu().tolist() == [len(t) for t in tensors]
    check_frames([H[q] if c else F[q] for q, c in enumerate(choice)], cdst, cfoff, cfres, 0, cfcap, (E, S, "choose"))
    back, res = run_decompress(hip, cdst, cfoff, D, E, S, blocks, 5)
    assert res == [len(t) for t in tensors] and (back[:D[-1]] == pc.cat(tensors)).all() and (back[D[-1]:] == FILL).all()
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
    back, res = run_decompress(hip, dst, foff, D, E, S, blocks, 3)
    assert res == [len(tensors[0]), r - (1 << 64)] + [len(t) for t in tensors[2:]]
    assert (back[D[victim]:D[victim + 1]] == FILL).all(), "a damaged frame leaves its tensor unwritten"
    assert (back[:D[victim]] == pc.cat(tensors[:victim])).all() and (back[D[victim + 1]:D[-1]] == pc.cat(tensors[victim + 1:])).all()
    assert (back[D[-1]:] == FILL).all()


def _seg_corpus(E, S, seg_log):
    """interleaved walks over two segments and a bit, nothing, the edge values over exactly one segment per plane, random bytes of a size that
    is no multiple of E one element above a segment, the constant channels over two segments and a half"""
    key = ("seg", E, S, seg_log)
    if key not in _CACHE:
        s = 1 << seg_log
        rng = np.random.default_rng(60 + 10 * E + S + seg_log)
        walks = (np.cumsum(rng.integers(-2, 3, (-(-(2 * s + 100) // S), S)), axis=0) + 500 * np.arange(1, S + 1)).reshape(-1)[:2 * s + 100]
        edge = np.tile(sc.across(E, S, 16), -(-s * E // len(sc.across(E, S, 16))))[:E * s]
        _CACHE[key] = [walks.astype(np.uint64).astype(sc._U[E]).view(np.uint8).copy(), np.zeros(0, np.uint8), edge,
                       rng.integers(0, 256, E * (s + 1) + E - 1, dtype=np.uint8), sc.channels(E, S, 5 * s // 2)]
    return _CACHE[key]


def _segments_of(tensors, E, seg_log):
    out = []
    for t in tensors:
        for pl in pc.planes_of(t, E):
            out += [np.ascontiguousarray(pl[a:a + (1 << seg_log)]) for a in (range(0, len(pl), 1 << seg_log) if len(pl) else [0])]
    return out


@pytest.mark.parametrize("seg_log", [10, 11])
@pytest.mark.parametrize("S", CSTRIDES)
@pytest.mark.parametrize("E", pc.ELEMS)
def test_segmented_frames_and_full_read_with_one_codec_and_with_choose(hip, checker, E, S, seg_log):
    from finitestateentropy_amd.api import AutoCodec
    tensors = _seg_corpus(E, S, seg_log)
    sizes = [len(t) for t in tensors]
    n, off = len(tensors), pc.offsets(tensors)
    total = int(off[-1])
    first = pseg.seg_first(sizes, E, seg_log)
    units = _segments_of(sc.pred_all(tensors, E, S), E, seg_log)
    F, H = _frames(checker, units, 0), _frames(checker, units, 1)
    assert len(F) == first[-1] > 5 * E
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, first[-1], blocks, 0)
    tol = 20
    choice = [fmc.expected_choice(len(f), len(h), tol)[0] for f, h in zip(F, H)]
    one = (E + S + seg_log) % 2
    for codec, want in ((one, H if one else F), (AutoCodec(tol), [H[q] if c else F[q] for q, c in enumerate(choice)])):
        dst, src, planes = _filled(fcap), _filled(total, 5, pc.cat(tensors)), _filled(total, 9)
        _, foff, fres, tres, chosen = hip.tensor_compress_seg_pred_stride_dbatch(src[:total], off, E, S, seg_log, np.asarray(first, np.uint64), codec=codec,
                                                                                 block_size_id=0, dst=dst, dst_capacity=fcap, max_total_blocks=blocks, planes=planes)
        torch.cuda.synchronize()
        assert tres.cpu().tolist() == sizes and (chosen is None if codec in (0, 1) else chosen.cpu().tolist() == choice)
        check_frames(want, dst, foff, fres, 0, fcap, (E, S, seg_log, codec))
        back = _filled(total, 11)
        _, res = hip.tensor_decompress_seg_pred_stride_dbatch(dst, foff, off, E, S, seg_log, np.asarray(first, np.uint64), dst=back, dst_capacity=total,
                                                              max_total_blocks=blocks)
        torch.cuda.synchronize()
        out = back.cpu().numpy()
        assert res.cpu().tolist() == sizes and (out[:total] == pc.cat(tensors)).all() and (out[total:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- graph
def test_compress_and_decompress_in_one_hip_graph(hip, checker):
    """one captured graph -- a single stream, a linear chain -- holding the strided compress and then the strided decompress; replayed once
    over a changed source"""
    E, S, codec, ALIGN = 4, 3, 0, 4
    sizes = [len(t) for t in _corpus(E, S)]
    n, off = len(sizes), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(off[-1])

    def source(seed):                                          # three interleaved walks of the corpus' sizes
        rng = np.random.default_rng(seed)
        return [np.concatenate([(np.cumsum(rng.integers(-9, 10, (-(-(s // E) // 3), 3)), axis=0) + (1 << 20) * np.arange(1, 4)).reshape(-1)[:s // E].astype("<u4")
                                .view(np.uint8), np.arange(s % E, dtype=np.uint8)]) for s in sizes]
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, ALIGN)
    wsize, rsize = hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize, hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    wsize.restype = rsize.restype = C.c_size_t
    wws = torch.empty(int(wsize(C.c_size_t(n * E), C.c_size_t(blocks), C.c_uint(0), C.c_int(codec))), dtype=torch.uint8, device="cuda")
    rws = torch.empty(int(rsize(C.c_size_t(n * E), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
    src = torch.zeros(total, dtype=torch.uint8, device="cuda")
    soff = _i64(off)
    frames, back, planes, planes2 = _filled(fcap), _filled(total), _filled(total), _filled(total)
    foff, poff, poff2 = (torch.zeros(n * E + 1, dtype=torch.int64, device="cuda") for _ in range(3))
    fres, pres = (torch.zeros(n * E, dtype=torch.int64, device="cuda") for _ in range(2))
    tres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))

    def work():
        hip.tensor_compress_pred_stride_dbatch(src, soff, E, S, codec=codec, block_size_id=0, dst=frames, dst_capacity=fcap, max_total_blocks=blocks, align_log=ALIGN,
                                               frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, workspace=wws)
        hip.tensor_decompress_pred_stride_dbatch(frames, foff, soff, E, S, dst=back, dst_capacity=total, max_total_blocks=blocks, planes=planes2,
                                                 planes_capacity=total, plane_offsets=poff2, plane_results=pres, workspace=rws, results=rres)
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
    want = _frames(checker, [pl for x in sc.pred_all(tensors, E, S) for pl in pc.planes_of(x, E)], codec)
    check_frames(want, frames, foff, fres, ALIGN, fcap, "replay")
    assert tres.cpu().tolist() == rres.cpu().tolist() == sizes
    out = back.cpu().numpy()
    assert (out[:total] == pc.cat(tensors)).all() and (out[total:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- stride 1
@pytest.mark.parametrize("E", pc.ELEMS)
def test_stride_one_is_the_predicted_planes_call_for_call(hip, E):
    """all six _stride_ calls with stride 1 against the _pred_ calls on the same inputs: planes, offsets, results and frames are identical"""
    tensors = _base(E)
    n, off = len(tensors), pc.offsets(tensors)
    total = int(off[-1])
    src = _dev(pc.cat(tensors))
    psizes = _i64([pc.plane_size(len(t), p, E) for t in tensors for p in range(E)])

    def same(a, b):
        torch.cuda.synchronize()
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)
    a = hip.planes_split_pred_stride_dbatch(src, off, E, 1, planes=_filled(total, 3))
    b = hip.planes_split_pred_dbatch(src, off, E, planes=_filled(total, 3))
    same(a, b)
    ma = hip.planes_merge_pred_stride_dbatch(a[0][:total], a[1][:-1], psizes, off, E, 1, dst=_filled(total, 5), capacity=total)
    mb = hip.planes_merge_pred_dbatch(b[0][:total], b[1][:-1], psizes, off, E, dst=_filled(total, 5), capacity=total)
    same(ma, mb)
    assert (ma[0].cpu().numpy()[:total] == pc.cat(tensors)).all()
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, 0)
    ca = hip.tensor_compress_pred_stride_dbatch(src, off, E, 1, codec=1, block_size_id=0, dst=_filled(fcap), dst_capacity=fcap, max_total_blocks=blocks)
    cb = hip.tensor_compress_pred_dbatch(src, off, E, codec=1, block_size_id=0, dst=_filled(fcap), dst_capacity=fcap, max_total_blocks=blocks)
    same(ca, cb)
    da = hip.tensor_decompress_pred_stride_dbatch(ca[0], ca[1], off, E, 1, dst=_filled(total, 1), dst_capacity=total, max_total_blocks=blocks)
    db = hip.tensor_decompress_pred_dbatch(cb[0], cb[1], off, E, dst=_filled(total, 1), dst_capacity=total, max_total_blocks=blocks)
    same(da, db)
    assert (da[0].cpu().numpy()[:total] == pc.cat(tensors)).all()
    seg_log = 10
    first = np.asarray(pseg.seg_first([len(t) for t in tensors], E, seg_log), np.uint64)
    scap = hip.frame_packed_bound(total, int(first[-1]), blocks, 0)
    sa = hip.tensor_compress_seg_pred_stride_dbatch(src, off, E, 1, seg_log, first, codec=0, block_size_id=0, dst=_filled(scap), dst_capacity=scap, max_total_blocks=blocks)
    sb = hip.tensor_compress_seg_pred_dbatch(src, off, E, seg_log, first, codec=0, block_size_id=0, dst=_filled(scap), dst_capacity=scap, max_total_blocks=blocks)
    same(sa, sb)
    ua = hip.tensor_decompress_seg_pred_stride_dbatch(sa[0], sa[1], off, E, 1, seg_log, first, dst=_filled(total, 2), dst_capacity=total, max_total_blocks=blocks)
    ub = hip.tensor_decompress_seg_pred_dbatch(sb[0], sb[1], off, E, seg_log, first, dst=_filled(total, 2), dst_capacity=total, max_total_blocks=blocks)
    same(ua, ub)
    assert (ua[0].cpu().numpy()[:total] == pc.cat(tensors)).all()


# ---------------------------------------------------------------------------------------------------------------- Python
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_strided_planes_through_the_python_surface_and_an_archive(hip, checker, tmp_path):
    from finitestateentropy_amd.api import PredictedPlanes
    gen = torch.Generator(device="cuda").manual_seed(23)
    xyz = torch.cumsum(torch.randn((20000, 3), generator=gen, device="cuda") * 1e-3, 0) + torch.tensor([100.0, -37.0, 5.5], device="cuda")
    rgb = (torch.cumsum(torch.randint(-2, 3, (5000, 3), generator=gen, device="cuda"), 0) + torch.tensor([60, 128, 200], device="cuda")).to(torch.uint8)
    audio = (torch.cumsum(torch.randint(-40, 41, (7000, 3), generator=gen, device="cuda"), 0)).to(torch.int16)
    ids = torch.cumsum(torch.randint(0, 60, (1100, 3), generator=gen, device="cuda", dtype=torch.int64), 0)
    weights = (torch.randn((64, 33), generator=gen, device="cuda") * 0.02).to(torch.bfloat16)
    empty = torch.zeros((0, 3), device="cuda", dtype=torch.float32)
    ts = [xyz, rgb, audio, ids, weights, empty]
    keep = [t.clone() for t in ts]
    codec = PredictedPlanes(1, stride=3)
    obj = hip.compress_tensors(ts, codec=codec)
    assert obj.predictor == "prev3" and obj.codec == codec and obj.delta is False and obj.segment_log is None and obj.sparse_permille is None
    assert sorted(g["elem_bytes"] for g in obj.groups) == [1, 2, 4, 8]
    # the frames are the oracle's Huff0 frames of the model's planes, at the default block-size id
    for g in obj.groups:
        E = g["elem_bytes"]
        raws = [ts[i].contiguous().reshape(-1).view(torch.uint8).cpu().numpy() for i in g["index"]]
        off, res, out = g["frame_offsets"].cpu().tolist(), g["frame_results"].cpu().tolist(), g["frames"].cpu().numpy()
        q = 0
        for x in sc.pred_all(raws, E, 3):
            for pl in pc.planes_of(x, E):
                r, f = checker.frame_compress(np.ascontiguousarray(pl), 5, 1)
                assert res[q] == r and (out[off[q]:off[q] + r] == f[:r]).all(), (E, q)
                q += 1
    back = hip.decompress_tensors(obj)
    for a, b, k in zip(ts, back, keep):
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and _bits(a, b) and _bits(a, k)
    one = hip.compress_tensors(ts, codec=PredictedPlanes(1))
    print("three interleaved channels, %d bytes: Huff0 frames of the stride-1 planes %d, of the stride-3 planes %d"
          % (sum(t.numel() * t.element_size() for t in ts), one.nbytes, obj.nbytes))
    assert one.predictor == "prev" and 0 < obj.nbytes < one.nbytes
    # through an archive and back: the stride travels in the meta JSON, the C head is that of a plain object
    buf = hip.archive_tensors(obj)
    info = hip.archive_inspect(buf[:64].cpu().numpy(), buf.numel())
    assert info.flags == 0 and info.deltaOp == 0 and info.sparsePermille == 0 and info.segLog == 0
    opened = hip.open_archive(buf)
    assert opened.predictor == "prev3" and opened.codec == codec and vars(opened)["predictor"] == "prev3"
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(opened), ts))
    path = str(tmp_path / "strided.fsea")
    hip.save_tensors(obj, path)
    loaded = hip.load_tensors(path)
    assert loaded.predictor == "prev3" and all(_bits(a, b) for a, b in zip(hip.decompress_tensors(loaded), ts))
    seg = hip.compress_tensors_segmented(ts, 15, PredictedPlanes(0, stride=3))
    assert seg.predictor == "prev3" and seg.segment_log == 15
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(seg), ts))
    reopened = hip.open_archive(hip.archive_tensors(seg))
    assert reopened.predictor == "prev3" and reopened.segment_log == 15 and reopened.codec == PredictedPlanes(0, 3)
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(reopened), ts))
    # windows and patches of strided objects, and a base beside the codec: refused
    wins = [(0, 10)] * (len(ts) - 1) + [(0, 0)]
    for o in (seg, reopened, obj):
        for call in (hip.decompress_tensor_windows, hip.decompress_tensor_windows_each):
            with pytest.raises(ValueError):
                call(o, wins)
        for call in (hip.patch_tensor_windows, hip.patch_tensor_windows_each):
            with pytest.raises(ValueError):
                call(o, ts, wins)
    with pytest.raises(ValueError):
        hip.compress_tensors(ts, codec, base=keep)

"""Tensor deltas on the device (FSEHIP_planes_split_xor_dbatch / _merge_xor_dbatch, FSEHIP_tensor_compress_delta_dbatch / _decompress_delta_dbatch
and the compress_tensors pair with `base`) against the numpy model of planes_delta_corpus.py -- the planes of `tensor XOR base` -- and the CPU
oracle's frames of those planes; never against the library's own calls.  Block-size id 0 (1 KB blocks) wherever frames are involved.  Every
destination is filled with 0xA5 and has a tail behind it: whatever the contract does not give to the call must still be 0xA5 afterwards, and
in the in-place form whatever the call does not own must still be the base."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_packed_corpus as fpc
import planes_corpus as pc
import planes_delta_corpus as pdc
from planes_corpus import CORRUPT, GENERIC, TILE, TOO_SMALL

pytestmark = pytest.mark.gpu

FILL, TAIL = 0xA5, 64
SHIFTS = ((0, 0, 0), (1, 3, 5), (8, 2, 15))                  # three buffers, each off 16-byte alignment by an amount of its own
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


def _pairs(E):
    """the size list of the issue: random tensors and random bases"""
    if E not in _CACHE:
        sizes = pc.split_sizes(E)
        _CACHE[E] = (pc.random_tensors(sizes, 7 + E), pc.random_tensors(sizes, 170 + E))
    return _CACHE[E]


# ---------------------------------------------------------------------------------------------------------------- 5, 6
def run_split(hip, tensors, bases, E, capacity=None, shift=(0, 0, 0)):
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    src, base, planes = _filled(total, shift[0], pc.cat(tensors)), _filled(total, shift[1], pc.cat(bases)), _filled(total, shift[2])
    poff = torch.full((n * E + 2,), -7, dtype=torch.int64, device="cuda")
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    hip.planes_split_xor_dbatch(src[:total], base[:total], S, E, capacity=capacity, planes=planes, plane_offsets=poff, results=res)
    torch.cuda.synchronize()
    assert int(poff[n * E + 1]) == -7 and int(res[n]) == -7
    assert (src.cpu().numpy()[:total] == pc.cat(tensors)).all() and (base.cpu().numpy()[:total] == pc.cat(bases)).all(), "the inputs are only read"
    return planes.cpu().numpy(), poff.cpu().tolist()[:n * E + 1], res.cpu().tolist()[:n]


def check_split(got, tensors, bases, E, capacity=None):
    out, poff, res = got
    want, written, P, wres = pdc.split_xor_model(tensors, bases, E, capacity)
    assert poff == P and res == wres
    total = len(want)
    assert (out[:total][written] == want[written]).all(), np.nonzero((out[:total] != want) & written)[0][:8]
    outside = np.ones(len(out), bool)
    outside[:total] = ~written
    assert (out[outside] == FILL).all(), ("bytes outside the accepted tensors' planes", np.nonzero((out != FILL) & outside)[0][:8])


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_xor_against_the_model(hip, E):
    tensors, bases = _pairs(E)
    assert [len(t) for t in tensors][:3] == [1, E + 1, 15] and max(len(t) for t in tensors) == 3 * TILE + 5
    for shift in SHIFTS:
        check_split(run_split(hip, tensors, bases, E, shift=shift), tensors, bases, E)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_xor_with_a_short_capacity(hip, E):
    tensors, bases = _pairs(E)
    S = [int(x) for x in pc.offsets(tensors)]
    k = 11                                                   # the tensor of one tile less a byte
    assert len(tensors[k]) == TILE - 1
    for cap in (S[k] + 100, S[k + 1], S[k + 1] - 1, S[6], 0):  # inside a tensor, at a tensor's end, one short of it, at an early end, nothing
        got = run_split(hip, tensors, bases, E, capacity=cap, shift=SHIFTS[1])
        check_split(got, tensors, bases, E, cap)
        first = next(i for i in range(len(tensors)) if S[i + 1] > cap)
        assert got[2][first:] == [GENERIC] * (len(tensors) - first) and got[1][first * E:] == [S[first]] * (len(got[1]) - first * E)
        assert (got[0][S[first]:] == FILL).all(), "nothing of a refused tensor is written"


# ---------------------------------------------------------------------------------------------------------------- 7, 8, 9
def run_merge(hip, E, planes_buf, poff, psizes, D, base_buf, capacity=None, shift=(0, 0, 0), in_place=False):
    """-> (dst with its tail, results); base_buf: D[-1] bytes laid out by D.  in_place: dst IS the base buffer"""
    n, room = len(D) - 1, int(D[-1])
    planes = _filled(len(planes_buf), shift[0], planes_buf)
    base = _filled(room, shift[1], base_buf)
    dst = base if in_place else _filled(room, shift[2])
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    out, _ = hip.planes_merge_xor_dbatch(planes[:max(len(planes_buf), 1)], _i64(poff), _i64(psizes), base, np.asarray(D, np.uint64), E, dst=dst,
                                         capacity=room if capacity is None else capacity, results=res)
    torch.cuda.synchronize()
    assert int(res[n]) == -7 and out.data_ptr() == dst.data_ptr() and (dst.data_ptr() == base.data_ptr()) == in_place
    if not in_place:
        assert (base.cpu().numpy()[:room] == base_buf).all() and (base.cpu().numpy()[room:] == FILL).all(), "a base that is not the destination is only read"
    return dst.cpu().numpy(), res.cpu().tolist()[:n]


def check_merge(got, tensors, E, psizes, D, capacity, untouched):
    """untouched: what every byte outside the good tensors' n bytes must still be -- FILL, or (in place) the base with FILL behind it"""
    out, res = got
    want = [pc.merge_verdict(psizes[i * E:(i + 1) * E], int(D[i + 1]), int(D[i]), E, capacity) for i in range(len(tensors))]
    assert res == want
    written = np.zeros(len(out), bool)
    for i, raw in enumerate(tensors):
        if want[i] >= 0:
            assert want[i] == len(raw)
            assert (out[int(D[i]):int(D[i]) + len(raw)] == raw).all(), i
            written[int(D[i]):int(D[i]) + len(raw)] = True
    assert (out[~written] == untouched[~written]).all(), ("bytes outside the good tensors", np.nonzero((out != untouched) & ~written)[0][:8])
    return want


def _untouched(base_buf, in_place):
    u = np.full(len(base_buf) + TAIL, FILL, np.uint8)
    if in_place:
        u[:len(base_buf)] = base_buf
    return u


@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_xor_against_the_model_separate_and_in_place(hip, E):
    tensors, bases = _pairs(E)
    buf, _, P, _ = pdc.split_xor_model(tensors, bases, E)
    psizes = [pc.plane_size(len(t), p, E) for t in tensors for p in range(E)]
    D = [int(x) for x in pc.offsets(tensors)]
    base_buf = pc.cat(bases)
    for shift in SHIFTS:
        apart = run_merge(hip, E, buf, P[:-1], psizes, D, base_buf, shift=shift)
        assert check_merge(apart, tensors, E, psizes, D, D[-1], _untouched(base_buf, False)) == [len(t) for t in tensors]
        # in place: the buffer holds the bases before and the new tensors after
        inpl = run_merge(hip, E, buf, P[:-1], psizes, D, base_buf, shift=shift, in_place=True)
        check_merge(inpl, tensors, E, psizes, D, D[-1], _untouched(base_buf, True))
        assert inpl[1] == apart[1] and (inpl[0] == apart[0]).all(), "in place and into a separate destination: the same bytes"
        assert (inpl[0][:D[-1]] == pc.cat(tensors)).all()


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_xor_refusals(hip, E, in_place):
    tensors = _pairs(E)[0]
    n = len(tensors)
    behind, failed, wrong, short = n - 1, 12, 10, 9               # one tensor per rule, in the header's order: 3 T + 5, T, 1024 E + 1 and 1024 E - 1 bytes
    slots = [len(t) + (i % 3) for i, t in enumerate(tensors)]  # slots with some room to spare ...
    slots[short] = len(tensors[short]) - 1                     # ... and one a byte short
    D = [0]
    for s in slots:
        D.append(D[-1] + s)
    base_buf = np.random.default_rng(900 + E).integers(0, 256, D[n], dtype=np.uint8)          # the base lies where the destination lies: by D
    deltas = []
    for i, t in enumerate(tensors):
        b = np.zeros(len(t), np.uint8)
        have = base_buf[D[i]:D[i] + len(t)]
        b[:len(have)] = have
        deltas.append(t ^ b)
    buf, _, P, _ = pc.split_model(deltas, E)
    psizes = [pc.plane_size(len(t), p, E) for t in tensors for p in range(E)]
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
    got = run_merge(hip, E, buf, P[:-1], psizes, D, base_buf, capacity=cap, shift=SHIFTS[1], in_place=in_place)
    want = check_merge(got, tensors, E, psizes, D, cap, _untouched(base_buf, in_place))
    assert want[behind] == GENERIC and want[failed] == first and (wrong is None or want[wrong] == CORRUPT) and want[short] == TOO_SMALL
    bad = [i for i, w in enumerate(want) if w < 0]
    assert len(bad) == (4 if wrong is not None else 3)
    if in_place:
        for i in bad:                                          # a refused tensor's slot is still the base's bytes exactly, its good neighbours are updated
            assert (got[0][D[i]:D[i + 1]] == base_buf[D[i]:D[i + 1]]).all(), i
            for j in (i - 1, i + 1):
                if 0 <= j < n and want[j] > 0:
                    assert (got[0][D[j]:D[j] + want[j]] == tensors[j]).all() and (tensors[j] != base_buf[D[j]:D[j] + want[j]]).any(), (i, j)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_a_zero_base_is_the_plain_call(hip, E):
    """The plain and the XOR kernels are one template: against an all-zero base the XOR split writes what the plain split writes (planes,
    plane offsets, results) and the XOR merge what the plain merge writes (destination, results), into a separate destination and in place.
    The ragged batch of the corpus, every buffer off 16-byte alignment by an amount of its own."""
    tensors = _pairs(E)[0]
    n, S, shift = len(tensors), pc.offsets(tensors), SHIFTS[1]
    total = int(S[-1])
    assert 0 in [len(t) for t in tensors] and len(tensors[0]) == 1 and shift[0] % 16 == 1
    zeros = [np.zeros(len(t), np.uint8) for t in tensors]
    xored = run_split(hip, tensors, zeros, E, shift=shift)
    src, planes = _filled(total, shift[0], pc.cat(tensors)), _filled(total, shift[2])
    poff = torch.full((n * E + 2,), -7, dtype=torch.int64, device="cuda")
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    hip.planes_split_dbatch(src[:total], S, E, planes=planes, plane_offsets=poff, results=res)
    torch.cuda.synchronize()
    assert xored[1] == poff.cpu().tolist()[:n * E + 1] and xored[2] == res.cpu().tolist()[:n] == [len(t) for t in tensors]
    plain = planes.cpu().numpy()
    if E == 1:                                                 # (the plain split of bytes writes nothing: its planes are the source)
        assert (plain == FILL).all()
        plain[:total] = pc.cat(tensors)
    assert (xored[0] == plain).all(), np.nonzero(xored[0] != plain)[0][:8]

    slots = [len(t) + (i % 3) for i, t in enumerate(tensors)]  # slots with some room to spare, and one a byte short
    slots[9] = len(tensors[9]) - 1
    D = [0]
    for s in slots:
        D.append(D[-1] + s)
    buf, _, P, _ = pc.split_model(tensors, E)
    psizes = [pc.plane_size(len(t), p, E) for t in tensors for p in range(E)]
    zero_base = np.zeros(D[n], np.uint8)
    pbuf, dst = _filled(len(buf), shift[0], buf), _filled(D[n], shift[2])
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    hip.planes_merge_dbatch(pbuf[:len(buf)], _i64(P[:-1]), _i64(psizes), np.asarray(D, np.uint64), E, dst=dst, capacity=D[n], results=res)
    torch.cuda.synchronize()
    plain, pres = dst.cpu().numpy(), res.cpu().tolist()[:n]
    assert pres == [len(t) if i != 9 else TOO_SMALL for i, t in enumerate(tensors)]
    apart = run_merge(hip, E, buf, P[:-1], psizes, D, zero_base, shift=shift)
    assert apart[1] == pres and (apart[0] == plain).all(), np.nonzero(apart[0] != plain)[0][:8]
    inpl = run_merge(hip, E, buf, P[:-1], psizes, D, zero_base, shift=shift, in_place=True)
    written = np.zeros(len(plain), bool)                       # (what neither merge writes stays as it was: FILL there, the zero base here)
    for i, t in enumerate(tensors):
        if i != 9:
            written[D[i]:D[i] + len(t)] = True
    assert inpl[1] == pres and (inpl[0][written] == plain[written]).all() and (plain[~written] == FILL).all()
    assert (inpl[0][:D[n]][~written[:D[n]]] == 0).all() and (inpl[0][D[n]:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- 10, 11
def _delta_corpus(oracle, E, codec):
    """(tensors, bases, the oracle's frames of every plane of t ^ b): an unchanged tensor, random against random, the bf16 weight update of
    test_planes_delta_model.py cut to 48 KB, an empty tensor, and a tensor whose size is no multiple of E that differs from its base in a byte
    in sixteen"""
    key = ("delta", E, codec)
    if key not in _CACHE:
        rng = np.random.default_rng(300 + E)
        old, new = pdc.bf16_update_pair()
        same = rng.integers(0, 256, 3000 * E, dtype=np.uint8)
        odd_base = rng.integers(0, 256, 2500 * E + E - 1, dtype=np.uint8)
        odd = odd_base ^ (rng.integers(1, 256, odd_base.size, dtype=np.uint8) * (rng.integers(0, 16, odd_base.size) == 0)).astype(np.uint8)
        tensors = [same, rng.integers(0, 256, 1025 * E, dtype=np.uint8), new[:48 << 10], np.zeros(0, np.uint8), odd]
        bases = [same.copy(), rng.integers(0, 256, 1025 * E, dtype=np.uint8), old[:48 << 10], np.zeros(0, np.uint8), odd_base]
        frames = []
        for x in pdc.xor_all(tensors, bases):
            for pl in pc.planes_of(x, E):
                r, f = oracle.frame_compress(np.ascontiguousarray(pl), 0, codec)
                frames.append(f[:r].copy())
        _CACHE[key] = (tensors, bases, frames)
    return _CACHE[key]


def run_compress(hip, tensors, bases, E, codec, align_log):
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, align_log)
    dst = _filled(fcap)
    src, base = _filled(total, 0, pc.cat(tensors)), _filled(total, 0, pc.cat(bases))
    _, foff, fres, tres = hip.tensor_compress_delta_dbatch(src[:total], base[:total], S, E, 0, codec, dst=dst, dst_capacity=fcap, max_total_blocks=blocks,
                                                           align_log=align_log)
    torch.cuda.synchronize()
    return dst, foff, fres, tres, fcap


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


@pytest.mark.parametrize("align_log", [0, 8])
@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_tensor_compress_delta_gives_the_oracles_frame_of_every_plane_of_the_xor(hip, checker, E, codec, align_log):
    tensors, bases, want = _delta_corpus(checker, E, codec)
    assert (tensors[0] == bases[0]).all() and len(tensors[3]) == 0 and len(tensors[4]) % E == E - 1 and len(tensors[2]) == 48 << 10
    assert all(len(f) < 64 for f in want[:E]), "an unchanged tensor: a few bytes per block and plane"
    dst, foff, fres, tres, fcap = run_compress(hip, tensors, bases, E, codec, align_log)
    check_frames(want, dst, foff, fres, align_log, fcap, (E, codec, align_log))
    assert tres.cpu().tolist() == [len(t) for t in tensors]


def run_decompress(hip, frames, foff, bases, D, E, blocks, in_place):
    total = int(D[-1])
    base = _filled(total, 0, pc.cat(bases))
    back = base if in_place else _filled(total)
    res = torch.full((len(D) - 1,), -7, dtype=torch.int64, device="cuda")
    hip.tensor_decompress_delta_dbatch(frames, foff, base, np.asarray(D, np.uint64), E, dst=back, dst_capacity=total, max_total_blocks=blocks, results=res)
    torch.cuda.synchronize()
    return back.cpu().numpy(), res.cpu().tolist()


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_tensor_decompress_delta_separate_in_place_and_a_damaged_frame(hip, checker, E, codec):
    tensors, bases, want = _delta_corpus(checker, E, codec)
    n, D = len(tensors), [int(x) for x in pc.offsets(tensors)]
    blocks = hip.planes_block_bound(D[-1], n, E, 0)
    dst, foff, fres, _, fcap = run_compress(hip, tensors, bases, E, codec, 0)
    check_frames(want, dst, foff, fres, 0, fcap, "the frames of test 10")
    for in_place in (False, True):
        back, res = run_decompress(hip, dst, foff, bases, D, E, blocks, in_place)
        assert res == [len(t) for t in tensors]
        assert (back[:D[-1]] == pc.cat(tensors)).all() and (back[D[-1]:] == FILL).all()
    # one payload byte of one plane's frame flipped (tensor 1, random against random: full 1 KB blocks): that tensor gets what the oracle's reader
    # says of that frame and is not written -- the fill pattern stays (separate), the base stays (in place); every other tensor is right
    victim, plane = 1, E - 1
    f = victim * E + plane
    at = 5 + 3 + 40                                            # behind the frame's and the first block's header
    assert len(want[f]) > at + 8
    bad = want[f].copy()
    bad[at] ^= 0x55
    r, _ = checker.frame_decompress(bad, len(tensors[victim][plane::E]))
    assert r > (1 << 63), "the oracle's reader refuses the damaged frame"
    dst[int(foff[f]) + at] ^= 0x55
    for in_place in (False, True):
        back, res = run_decompress(hip, dst, foff, bases, D, E, blocks, in_place)
        assert res == [len(tensors[0]), r - (1 << 64)] + [len(t) for t in tensors[2:]]
        slot = back[D[victim]:D[victim + 1]]
        assert (slot == (bases[victim] if in_place else FILL)).all()
        assert (back[:D[victim]] == pc.cat(tensors[:victim])).all() and (back[D[victim + 1]:D[-1]] == pc.cat(tensors[victim + 1:])).all()
        assert (back[D[-1]:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- 12
def test_delta_compress_and_decompress_in_one_hip_graph(hip, checker):
    """one captured graph -- a single stream, a linear chain -- holding tensor_compress_delta_dbatch and then tensor_decompress_delta_dbatch into
    a destination of its own; replayed twice, the source changed in between, the base fixed"""
    E, codec, ALIGN = 2, 0, 4
    _, bases, _ = _delta_corpus(checker, E, codec)
    n, S = len(bases), pc.offsets(bases)
    total = int(S[-1])

    def source(seed):                                          # the bases with a byte in eight changed
        rng = np.random.default_rng(seed)
        return [b ^ (rng.integers(1, 256, b.size, dtype=np.uint8) * (rng.integers(0, 8, b.size) == 0)).astype(np.uint8) for b in bases]
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, ALIGN)
    wsize, rsize = hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize, hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    wsize.restype = rsize.restype = C.c_size_t
    wws = torch.empty(int(wsize(C.c_size_t(n * E), C.c_size_t(blocks), C.c_uint(0), C.c_int(codec))), dtype=torch.uint8, device="cuda")
    rws = torch.empty(int(rsize(C.c_size_t(n * E), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
    src = torch.zeros(total, dtype=torch.uint8, device="cuda")
    base = _dev(pc.cat(bases))
    soff = _i64(S)
    frames, back, planes, planes2 = _filled(fcap), _filled(total), _filled(total), _filled(total)
    foff, poff, poff2 = (torch.zeros(n * E + 1, dtype=torch.int64, device="cuda") for _ in range(3))
    fres, pres = (torch.zeros(n * E, dtype=torch.int64, device="cuda") for _ in range(2))
    tres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))

    def work():
        hip.tensor_compress_delta_dbatch(src, base, soff, E, 0, codec, dst=frames, dst_capacity=fcap, max_total_blocks=blocks, align_log=ALIGN, frame_offsets=foff,
                                         frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, workspace=wws)
        hip.tensor_decompress_delta_dbatch(frames, foff, base, soff, E, dst=back, dst_capacity=total, max_total_blocks=blocks, planes=planes2, planes_capacity=total,
                                           plane_offsets=poff2, plane_results=pres, workspace=rws, results=rres)
    src.copy_(_dev(pc.cat(source(0)))); work(); torch.cuda.synchronize()      # one ordinary call first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    seen = []
    for trial in (1, 2):
        tensors = source(trial)
        seen.append(pc.cat(tensors))
        src.copy_(_dev(seen[-1]))
        for t in (frames, back):
            t.fill_(FILL)
        for t in (foff, fres, tres, rres):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = [f[:r].copy() for x in pdc.xor_all(tensors, bases) for pl in pc.planes_of(x, E) for r, f in [checker.frame_compress(np.ascontiguousarray(pl), 0, codec)]]
        check_frames(want, frames, foff, fres, ALIGN, fcap, trial)
        assert tres.cpu().tolist() == rres.cpu().tolist() == [len(t) for t in tensors]
        out = back.cpu().numpy()
        assert (out[:total] == seen[-1]).all() and (out[total:] == FILL).all()
        assert (base.cpu().numpy() == pc.cat(bases)).all()
    assert not (seen[0] == seen[1]).all()


# ---------------------------------------------------------------------------------------------------------------- 13
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_compress_tensors_with_a_base_and_back(hip, monkeypatch):
    gen = torch.Generator(device="cuda").manual_seed(13)
    old_np, new_np = pdc.bf16_update_pair(1 << 16)
    old_bf, new_bf = (torch.from_numpy(x.copy()).cuda().view(torch.bfloat16).reshape(256, 256) for x in (old_np, new_np))
    old_f = torch.randn((1000, 3), generator=gen, device="cuda") * 0.02
    new_f = old_f + torch.randn((1000, 3), generator=gen, device="cuda") * 2e-5
    old_i = torch.randint(-128, 128, (4, 50), generator=gen, device="cuda", dtype=torch.int8)
    new_i = old_i.clone(); new_i[1, ::7] += 1
    old_d = torch.randint(-2 ** 62, 2 ** 62, (17,), generator=gen, device="cuda", dtype=torch.int64)
    old_d[:2] = torch.tensor([0x7FF8000000000001, 0xFFF0000000000002 - (1 << 64)], dtype=torch.int64)      # NaN payloads: bits, not values, count
    new_d = old_d.clone(); new_d[0] += 1; new_d[5] ^= 0xFF00
    old_d, new_d = old_d.view(torch.float64), new_d.view(torch.float64)
    assert bool(torch.isnan(new_d).any())
    empty = torch.zeros((0, 3), device="cuda", dtype=torch.float32)
    old, new = [old_bf, old_f, old_i, old_d, empty], [new_bf, new_f, new_i, new_d, empty.clone()]
    keep = [t.clone() for t in old]
    obj = hip.compress_tensors(new, base=old)
    assert obj.delta is True and sorted(g["elem_bytes"] for g in obj.groups) == [1, 2, 4, 8]
    back = hip.decompress_tensors(obj, base=old)
    assert len(back) == len(new)
    for a, b, o, k in zip(new, back, old, keep):
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and _bits(a, b)
        assert _bits(o, k) and (b.numel() == 0 or b.data_ptr() != o.data_ptr()), "the bases are as they were, the results own their memory"
    # the reason for the feature, on the device: the bf16 update against its base takes fewer bytes than on its own
    plain, delta = hip.compress_tensors([new_bf]), hip.compress_tensors([new_bf], base=[old_bf])
    print("bf16 update, %d bytes: frames of the planes %d, of the planes of the XOR with its base %d" % (new_bf.numel() * 2, plain.nbytes, delta.nbytes))
    assert plain.delta is False and 0 < delta.nbytes < plain.nbytes
    assert _bits(hip.decompress_tensors(delta, base=[old_bf])[0], new_bf) and _bits(hip.decompress_tensors(plain)[0], new_bf)

    # every mismatch is raised before a launch: from here on a call into the library is a failure of the test
    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in ("FSEHIP_tensor_compress_dbatch", "FSEHIP_tensor_compress_delta_dbatch", "FSEHIP_tensor_decompress_dbatch", "FSEHIP_tensor_decompress_delta_dbatch",
                 "FSEHIP_planes_split_xor_dbatch", "FSEHIP_planes_merge_xor_dbatch"):
        monkeypatch.setattr(hip.lib, name, no_launch)
    with pytest.raises(ValueError):
        hip.compress_tensors(new, base=old[:-1])                             # one base too few
    with pytest.raises(ValueError):
        hip.compress_tensors(new, base=[old_bf.reshape(-1)] + old[1:])       # another shape
    with pytest.raises(TypeError):
        hip.compress_tensors(new, base=[old_bf.view(torch.float16)] + old[1:])   # another dtype
    with pytest.raises(TypeError):
        hip.compress_tensors(new, base=[old_bf.cpu()] + old[1:])             # another device
    with pytest.raises(TypeError):
        hip.compress_tensors(new, base=[None] + old[1:])                     # no tensor
    with pytest.raises(ValueError):
        hip.decompress_tensors(obj)                                          # a delta object without its base
    with pytest.raises(ValueError):
        hip.decompress_tensors(plain, base=[old_bf])                         # a plain object with one
    with pytest.raises(ValueError):
        hip.decompress_tensors(obj, base=old[1:])
    with pytest.raises(TypeError):
        hip.decompress_tensors(obj, base=[old_bf.view(torch.int16)] + old[1:])

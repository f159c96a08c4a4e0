"""Arithmetic tensor deltas on the device (the ten FSEHIP_*_op_dbatch calls with FSEHIP_DELTA_SUB and the Python surface around DeltaBase) against
the numpy model of planes_sub_corpus.py -- the planes of zigzag(tensor - base) -- and the CPU oracle's frames of those planes; never against the
library's own calls, except where the point is that the *_op calls with FSEHIP_DELTA_XOR are the old XOR calls byte for byte.  Block-size id 0
wherever frames are involved.  Every destination is filled with 0xA5 and has a tail behind it: whatever the contract does not give to the
call must still be 0xA5 afterwards, and in the in-place form whatever the call does not own must still be the base."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_mixed_corpus as fmc
import frame_packed_corpus as fpc
import planes_corpus as pc
import planes_delta_corpus as pdc
import planes_seg_corpus as pseg
import planes_sub_corpus as psc
from planes_corpus import CORRUPT, GENERIC, TILE, TOO_SMALL

pytestmark = pytest.mark.gpu

FILL, TAIL = 0xA5, 64
SHIFTS = ((0, 0, 0), (1, 3, 5), (8, 2, 15))                  # three buffers, each off 16-byte alignment by an amount of its own
SUB, XOR = psc.SUB, psc.XOR
_CACHE = {}
# the C calls that take d_base, and where: the position of d_base among the arguments of the call without _op
BASE_AT = {"FSEHIP_planes_split_xor_dbatch": 4, "FSEHIP_planes_merge_xor_dbatch": 6, "FSEHIP_planes_split_window_dbatch": 4, "FSEHIP_tensor_compress_delta_dbatch": 6,
           "FSEHIP_tensor_decompress_delta_dbatch": 3, "FSEHIP_tensor_compress_mixed_dbatch": 6, "FSEHIP_tensor_compress_seg_dbatch": 6,
           "FSEHIP_tensor_decompress_seg_dbatch": 3, "FSEHIP_tensor_decompress_window_dbatch": 3, "FSEHIP_tensor_patch_window_dbatch": 12}


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
    """(tensors, bases): the size list of the issue, random against random (the first 15 tensors are those of test_gpu_planes_delta.py's refusal
    test, then 0 .. 40 bytes); the adversarial pairs cut into tensors of 15 elements -- below a chunk, every pattern goes the bytewise way --
    a tensor of one or two bytes, so that what follows starts at an odd address; and the adversarial pairs repeated over two chunks per lane of a
    workgroup and 19 elements more, with E - 1 bytes of a partial element behind them: every pattern goes through the chunks"""
    if E not in _CACHE:
        sizes = pc.split_sizes(E) + list(range(41))
        tensors, bases = pc.random_tensors(sizes, 7 + E), pc.random_tensors(sizes, 170 + E)
        t, b = psc.edge_pairs(E)
        for a in range(0, len(t), 15 * E):
            tensors.append(t[a:a + 15 * E]); bases.append(b[a:a + 15 * E])
        odd = 1 if sum(len(x) for x in tensors) % 2 == 0 else 2
        tensors.append(np.array([200, 7][:odd], np.uint8)); bases.append(np.array([100, 9][:odd], np.uint8))
        n_el = 2 * 256 * 16 + 19
        rep = -(-n_el * E // len(t))
        t, b = psc.edge_pairs(E, rep)
        extra = np.arange(1, E, dtype=np.uint8)
        tensors.append(np.concatenate([t[:n_el * E], 255 - extra])); bases.append(np.concatenate([b[:n_el * E], extra]))
        _CACHE[E] = (tensors, bases)
    return _CACHE[E]


# ---------------------------------------------------------------------------------------------------------------- split
def run_split(hip, tensors, bases, E, capacity=None, shift=(0, 0, 0), op=SUB):
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    src, base, planes = _filled(total, shift[0], pc.cat(tensors)), _filled(total, shift[1], pc.cat(bases)), _filled(total, shift[2])
    poff = torch.full((n * E + 2,), -7, dtype=torch.int64, device="cuda")
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    hip.planes_split_xor_dbatch(src[:total], base[:total], S, E, capacity=capacity, planes=planes, plane_offsets=poff, results=res, delta_op=op)
    torch.cuda.synchronize()
    assert int(poff[n * E + 1]) == -7 and int(res[n]) == -7
    assert (src.cpu().numpy()[:total] == pc.cat(tensors)).all() and (base.cpu().numpy()[:total] == pc.cat(bases)).all(), "the inputs are only read"
    return planes.cpu().numpy(), poff.cpu().tolist()[:n * E + 1], res.cpu().tolist()[:n]


def check_split(got, tensors, bases, E, capacity=None, op=SUB):
    out, poff, res = got
    want, written, P, wres = pc.split_model(psc.delta_all(tensors, bases, E, op), E, capacity)
    assert poff == P and res == wres
    total = len(want)
    assert (out[:total][written] == want[written]).all(), np.nonzero((out[:total] != want) & written)[0][:8]
    outside = np.ones(len(out), bool)
    outside[:total] = ~written
    assert (out[outside] == FILL).all(), ("bytes outside the accepted tensors' planes", np.nonzero((out != FILL) & outside)[0][:8])


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_sub_against_the_model(hip, E):
    tensors, bases = _pairs(E)
    sizes = [len(t) for t in tensors]
    assert sizes[:3] == [1, E + 1, 15] and 3 * TILE + 5 in sizes and 0 in sizes and sizes[-1] % E == E - 1 and sizes[-1] >= (2 * 256 * 16 + 16) * E
    assert any(0 < s < 16 * E for s in sizes) and pc.offsets(tensors)[-2] % 2 == 1
    for shift in SHIFTS:
        check_split(run_split(hip, tensors, bases, E, shift=shift), tensors, bases, E)
    # not symmetric: base against tensor gives other planes
    assert (run_split(hip, bases, tensors, E)[0] != run_split(hip, tensors, bases, E)[0]).any()


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_sub_with_a_short_capacity(hip, E):
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


# ---------------------------------------------------------------------------------------------------------------- merge
def run_merge(hip, E, planes_buf, poff, psizes, D, base_buf, capacity=None, shift=(0, 0, 0), in_place=False, op=SUB):
    """-> (dst with its tail, results); base_buf: D[-1] bytes laid out by D.  in_place: dst IS the base buffer"""
    n, room = len(D) - 1, int(D[-1])
    planes = _filled(len(planes_buf), shift[0], planes_buf)
    base = _filled(room, shift[1], base_buf)
    dst = base if in_place else _filled(room, shift[2])
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    out, _ = hip.planes_merge_xor_dbatch(planes[:max(len(planes_buf), 1)], _i64(poff), _i64(psizes), base, np.asarray(D, np.uint64), E, dst=dst,
                                         capacity=room if capacity is None else capacity, results=res, delta_op=op)
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
            assert (out[int(D[i]):int(D[i]) + len(raw)] == raw).all(), (i, np.nonzero(out[int(D[i]):int(D[i]) + len(raw)] != raw)[0][:8])
            written[int(D[i]):int(D[i]) + len(raw)] = True
    assert (out[~written] == untouched[~written]).all(), ("bytes outside the good tensors", np.nonzero((out != untouched) & ~written)[0][:8])
    return want


def _untouched(base_buf, in_place):
    u = np.full(len(base_buf) + TAIL, FILL, np.uint8)
    if in_place:
        u[:len(base_buf)] = base_buf
    return u


@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_sub_against_the_model_separate_and_in_place(hip, E):
    tensors, bases = _pairs(E)
    buf, _, P, _ = psc.split_sub_model(tensors, bases, E)
    psizes = [pc.plane_size(len(t), p, E) for t in tensors for p in range(E)]
    D = [int(x) for x in pc.offsets(tensors)]
    base_buf = pc.cat(bases)
    for shift in SHIFTS:
        apart = run_merge(hip, E, buf, P[:-1], psizes, D, base_buf, shift=shift)
        assert check_merge(apart, tensors, E, psizes, D, D[-1], _untouched(base_buf, False)) == [len(t) for t in tensors]
        inpl = run_merge(hip, E, buf, P[:-1], psizes, D, base_buf, shift=shift, in_place=True)
        check_merge(inpl, tensors, E, psizes, D, D[-1], _untouched(base_buf, True))
        assert inpl[1] == apart[1] and (inpl[0] == apart[0]).all(), "in place and into a separate destination: the same bytes"
        assert (inpl[0][:D[-1]] == pc.cat(tensors)).all()


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_sub_refusals(hip, E, in_place):
    tensors = _pairs(E)[0]
    n = len(tensors)
    behind, failed, wrong, short = n - 1, 12, 10, 9               # one tensor per rule, in the header's order: the last one, T, 1024 E + 1 and 1024 E - 1 bytes
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
        deltas.append(psc.forward(t, b, E))
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


# ---------------------------------------------------------------------------------------------------------------- composites
def _delta_corpus(oracle, E, codec, op=SUB):
    """(tensors, bases, the oracle's frames of every plane of the delta): an unchanged tensor, random against random, the bf16 weight update of
    test_planes_delta_model.py cut to 48 KB, an empty tensor, a tensor whose size is no multiple of E that differs from its base in a byte in
    sixteen, and the adversarial pairs"""
    key = ("delta", E, codec, op)
    if key not in _CACHE:
        rng = np.random.default_rng(300 + E)
        old, new = pdc.bf16_update_pair()
        same = rng.integers(0, 256, 3000 * E, dtype=np.uint8)
        odd_base = rng.integers(0, 256, 2500 * E + E - 1, dtype=np.uint8)
        odd = odd_base ^ (rng.integers(1, 256, odd_base.size, dtype=np.uint8) * (rng.integers(0, 16, odd_base.size) == 0)).astype(np.uint8)
        et, eb = psc.edge_pairs(E, 8)
        tensors = [same, rng.integers(0, 256, 1025 * E, dtype=np.uint8), new[:48 << 10], np.zeros(0, np.uint8), odd, et]
        bases = [same.copy(), rng.integers(0, 256, 1025 * E, dtype=np.uint8), old[:48 << 10], np.zeros(0, np.uint8), odd_base, eb]
        frames = []
        for x in psc.delta_all(tensors, bases, E, op):
            for pl in pc.planes_of(x, E):
                r, f = oracle.frame_compress(np.ascontiguousarray(pl), 0, codec)
                frames.append(f[:r].copy())
        _CACHE[key] = (tensors, bases, frames)
    return _CACHE[key]


def run_compress(hip, tensors, bases, E, codec, align_log, op=SUB, auto=None):
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, align_log)
    dst = _filled(fcap)
    src, base = _filled(total, 0, pc.cat(tensors)), _filled(total, 0, pc.cat(bases))
    if auto is not None:
        _, foff, fres, tres, chosen = hip.tensor_compress_mixed_dbatch(src[:total], S, E, base[:total], None, auto, 0, dst=dst, dst_capacity=fcap, max_total_blocks=blocks,
                                                                       align_log=align_log, delta_op=op)
        torch.cuda.synchronize()
        return dst, foff, fres, tres, fcap, chosen.cpu().tolist()
    _, foff, fres, tres = hip.tensor_compress_delta_dbatch(src[:total], base[:total], S, E, 0, codec, dst=dst, dst_capacity=fcap, max_total_blocks=blocks,
                                                           align_log=align_log, delta_op=op)
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


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_tensor_compress_sub_gives_the_oracles_frame_of_every_plane_of_the_delta(hip, checker, E, codec):
    tensors, bases, want = _delta_corpus(checker, E, codec)
    assert (tensors[0] == bases[0]).all() and len(tensors[3]) == 0 and len(tensors[4]) % E == E - 1 and len(tensors[2]) == 48 << 10
    assert all(len(f) < 64 for f in want[:E]), "an unchanged tensor: a few bytes per block and plane"
    for align_log in (0, 8):
        dst, foff, fres, tres, fcap = run_compress(hip, tensors, bases, E, codec, align_log)
        check_frames(want, dst, foff, fres, align_log, fcap, (E, codec, align_log))
        assert tres.cpu().tolist() == [len(t) for t in tensors]


@pytest.mark.parametrize("E", pc.ELEMS)
def test_tensor_compress_sub_with_an_autocodec(hip, checker, E):
    tensors, bases, F = _delta_corpus(checker, E, 0)
    _, _, H = _delta_corpus(checker, E, 1)
    tol = 20
    dst, foff, fres, tres, fcap, chosen = run_compress(hip, tensors, bases, E, None, 0, auto=tol)
    want = [fmc.expected_choice(len(f), len(h), tol)[0] for f, h in zip(F, H)]
    assert chosen == want, "the choice per plane is the mixed model's"
    check_frames([H[q] if c else F[q] for q, c in enumerate(want)], dst, foff, fres, 0, fcap, E)
    assert tres.cpu().tolist() == [len(t) for t in tensors]


def run_decompress(hip, frames, foff, bases, D, E, blocks, in_place, op=SUB):
    total = int(D[-1])
    base = _filled(total, 0, pc.cat(bases))
    back = base if in_place else _filled(total)
    res = torch.full((len(D) - 1,), -7, dtype=torch.int64, device="cuda")
    hip.tensor_decompress_delta_dbatch(frames, foff, base, np.asarray(D, np.uint64), E, dst=back, dst_capacity=total, max_total_blocks=blocks, results=res, delta_op=op)
    torch.cuda.synchronize()
    return back.cpu().numpy(), res.cpu().tolist()


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_tensor_decompress_sub_separate_in_place_and_a_damaged_frame(hip, checker, E, codec):
    tensors, bases, want = _delta_corpus(checker, E, codec)
    n, D = len(tensors), [int(x) for x in pc.offsets(tensors)]
    blocks = hip.planes_block_bound(D[-1], n, E, 0)
    dst, foff, fres, _, fcap = run_compress(hip, tensors, bases, E, codec, 0)
    check_frames(want, dst, foff, fres, 0, fcap, "the frames of the compress test")
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


def test_the_bf16_update_pair_takes_the_oracles_bytes_and_less_than_the_xor(hip, checker):
    """the whole pair of the issue at block-size id 5: the device's frames of both deltas are the oracle's, and their totals those of the issue"""
    old, new = pdc.bf16_update_pair()
    S = np.array([0, new.size], np.uint64)
    totals = {}
    for codec, bound, issue in ((0, 0.90, (69334, 59915)), (1, 0.95, (103787, 95708))):
        for op in (XOR, SUB):
            _, foff, fres, tres = hip.tensor_compress_delta_dbatch(_dev(new), _dev(old), S, 2, 5, codec, delta_op=op)
            out, off, res = _.cpu().numpy(), foff.cpu().tolist(), fres.cpu().tolist()
            for p, pl in enumerate(pc.planes_of(psc.delta_all([new], [old], 2, op)[0], 2)):
                r, f = checker.frame_compress(np.ascontiguousarray(pl), 5, codec)
                assert res[p] == r and (out[off[p]:off[p] + r] == f[:r]).all(), (codec, op, p)
            totals[codec, op] = sum(res)
        print("bf16 update pair, codec %d: frames of the XOR %d, of the SUB delta %d (%.3f)" % (codec, totals[codec, XOR], totals[codec, SUB],
                                                                                               totals[codec, SUB] / totals[codec, XOR]))
        assert (totals[codec, XOR], totals[codec, SUB]) == issue and totals[codec, SUB] < bound * totals[codec, XOR]


# ---------------------------------------------------------------------------------------------------------------- segments, windows, patches
def _seg_corpus(E, seg_log):
    """(tensors, bases): a bf16 update over two segments and a bit, nothing, the adversarial pairs over exactly one segment per plane, a tensor of
    a size that is no multiple of E one element above a segment, a skewed source of two segments and a half whose base differs in a byte in sixteen"""
    key = ("seg", E, seg_log)
    if key not in _CACHE:
        s = 1 << seg_log
        rng = np.random.default_rng(60 + E + seg_log)
        old, new = pdc.bf16_update_pair(1 << 15)
        n0 = E * (2 * s + 100)
        et, eb = psc.edge_pairs(E, -(-s * E // len(psc.edge_pairs(E)[0])))
        odd = rng.integers(0, 256, E * (s + 1) + E - 1, dtype=np.uint8)
        skew = rng.integers(0, 4, 5 * E * s // 2, dtype=np.uint8)
        tensors = [new[:n0], np.zeros(0, np.uint8), et[:E * s], odd, skew]
        bases = [old[:n0], np.zeros(0, np.uint8), eb[:E * s], (odd + (rng.integers(0, 16, odd.size) == 0)).astype(np.uint8),
                 skew ^ (rng.integers(1, 256, skew.size, dtype=np.uint8) * (rng.integers(0, 16, skew.size) == 0)).astype(np.uint8)]
        assert len(tensors[0]) == n0
        _CACHE[key] = (tensors, bases)
    return _CACHE[key]


def _segments_of(tensors, E, seg_log):
    out = []
    for t in tensors:
        for pl in pc.planes_of(t, E):
            out += [np.ascontiguousarray(pl[a:a + (1 << seg_log)]) for a in (range(0, len(pl), 1 << seg_log) if len(pl) else [0])]
    return out


def _seg_frames(oracle, tensors, bases, E, seg_log, codec):
    return [f[:r].copy() for seg in _segments_of(psc.sub_all(tensors, bases, E), E, seg_log) for r, f in [oracle.frame_compress(seg, 0, codec)]]


def run_seg_compress(hip, tensors, bases, E, seg_log, codec=0):
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    first = pseg.seg_first([len(t) for t in tensors], E, seg_log)
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, first[-1], blocks, 0)
    dst = _filled(fcap)
    src, base = _filled(total, 0, pc.cat(tensors)), _filled(total, 0, pc.cat(bases))
    _, foff, fres, tres, _ = hip.tensor_compress_seg_dbatch(src[:total], S, E, seg_log, np.asarray(first, np.uint64), base=base[:total], codec=codec, block_size_id=0,
                                                            dst=dst, dst_capacity=fcap, max_total_blocks=blocks, delta_op=SUB)
    torch.cuda.synchronize()
    return dst, foff, fres, tres, fcap, first


@pytest.mark.parametrize("seg_log", [10, 11])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_segmented_sub_frames_full_read_windows_and_patch(hip, checker, E, seg_log):
    tensors, bases = _seg_corpus(E, seg_log)
    sizes = [len(t) for t in tensors]
    n, D = len(tensors), [int(x) for x in pc.offsets(tensors)]
    want = _seg_frames(checker, tensors, bases, E, seg_log, 0)
    dst, foff, fres, tres, fcap, first = run_seg_compress(hip, tensors, bases, E, seg_log)
    assert len(want) == first[-1] > 5 * E and tres.cpu().tolist() == sizes
    check_frames(want, dst, foff, fres, 0, fcap, (E, seg_log))
    # the full read, into a destination of its own and in place
    for in_place in (False, True):
        base = _filled(D[-1], 0, pc.cat(bases))
        back = base if in_place else _filled(D[-1])
        _, res = hip.tensor_decompress_seg_dbatch(dst, foff, np.asarray(D, np.uint64), E, seg_log, np.asarray(first, np.uint64), base=base, dst=back, dst_capacity=D[-1],
                                                  max_total_blocks=hip.planes_block_bound(D[-1], n, E, 0), delta_op=SUB)
        torch.cuda.synchronize()
        out = back.cpu().numpy()
        assert res.cpu().tolist() == sizes and (out[:D[-1]] == pc.cat(tensors)).all() and (out[D[-1]:] == FILL).all()
    # windows that start and end inside segments (one empty, one of a single element, one over everything addressable)
    s = 1 << seg_log
    wins = [(s // 2 + 3, 2 * s + 7), (0, 0), (s - 1, s), (5, s + 1), (0, sizes[4] // E)]
    doff = np.concatenate([[0], np.cumsum([E * (b - a) for a, b in wins])]).astype(np.uint64)
    wbase = pc.cat([b[E * w[0]:E * w[1]] for b, w in zip(bases, wins)])
    room = int(doff[-1])
    for in_place in (False, True):
        base = _filled(room, 0, wbase)
        back = base if in_place else _filled(room)
        _, res = hip.tensor_decompress_window_dbatch(dst, foff, np.asarray(D, np.uint64), wins, doff, E, seg_log, np.asarray(first, np.uint64), base=base, dst=back,
                                                     dst_capacity=room, block_size_id=0, delta_op=SUB)
        torch.cuda.synchronize()
        out = back.cpu().numpy()
        assert res.cpu().tolist() == [E * (b - a) for a, b in wins]
        assert (out[:room] == pc.cat([t[E * w[0]:E * w[1]] for t, w in zip(tensors, wins)])).all() and (out[room:] == FILL).all()
    # a patch: the tensors change inside windows; the patched object is byte for byte the full SUB compress of the new tensors
    rng = np.random.default_rng(5 + E)
    pwins = [(s // 2 + 3, s + 7), (0, 0), (0, 0), (s - 2, s + 1), (s + 5, 2 * s)]
    newer = []
    for t, (a, b) in zip(tensors, pwins):
        t = t.copy()
        t[E * a:E * b] += rng.integers(1, 3, E * (b - a), dtype=np.uint8)
        newer.append(t)
    assert all((x != y).any() == (b > a) for x, y, (a, b) in zip(newer, tensors, pwins))
    full = run_seg_compress(hip, newer, bases, E, seg_log)
    total_new, total_old = int(full[1][-1]), int(foff[-1])
    out, ooff, ores, ptres, _ = hip.tensor_patch_window_dbatch(dst[:total_old].clone(), foff, fres, _dev(pc.cat(newer)), np.asarray(D, np.uint64), pwins, E, seg_log,
                                                               np.asarray(first, np.uint64), base=_dev(pc.cat(bases)), codec=0, block_size_id=0, delta_op=SUB)
    torch.cuda.synchronize()
    assert ptres.cpu().tolist() == sizes and ooff.cpu().tolist() == full[1].cpu().tolist() and ores.cpu().tolist() == full[2].cpu().tolist()
    assert (out.cpu().numpy()[:total_new] == full[0].cpu().numpy()[:total_new]).all()
    check_frames(_seg_frames(checker, newer, bases, E, seg_log, 0), full[0], full[1], full[2], 0, full[4], "the full compress of the new tensors")


def test_sub_compress_and_decompress_in_one_hip_graph(hip, checker):
    """one captured graph -- a single stream, a linear chain -- holding the SUB compress and then the SUB decompress into a destination of its own;
    replayed once over a changed source, the base fixed"""
    E, codec, ALIGN = 2, 0, 4
    _, bases, _ = _delta_corpus(checker, E, codec)
    n, S = len(bases), pc.offsets(bases)
    total = int(S[-1])

    def source(seed):                                          # the bases with one element in eight moved by -2 .. 2
        rng = np.random.default_rng(seed)
        out = []
        for b in bases:
            v = b[:len(b) // 2 * 2].view("<u2")
            moved = (v + (rng.integers(0, 5, v.size).astype("<u2") - np.uint16(2)) * (rng.integers(0, 8, v.size) == 0).astype("<u2")).astype("<u2")
            out.append(np.concatenate([moved.view(np.uint8), b[len(b) // 2 * 2:]]))
        return out
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
                                         frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, workspace=wws, delta_op=SUB)
        hip.tensor_decompress_delta_dbatch(frames, foff, base, soff, E, dst=back, dst_capacity=total, max_total_blocks=blocks, planes=planes2, planes_capacity=total,
                                           plane_offsets=poff2, plane_results=pres, workspace=rws, results=rres, delta_op=SUB)
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
    want = [f[:r].copy() for x in psc.sub_all(tensors, bases, E) for pl in pc.planes_of(x, E) for r, f in [checker.frame_compress(np.ascontiguousarray(pl), 0, codec)]]
    check_frames(want, frames, foff, fres, ALIGN, fcap, "replay")
    assert tres.cpu().tolist() == rres.cpu().tolist() == [len(t) for t in tensors]
    out = back.cpu().numpy()
    assert (out[:total] == pc.cat(tensors)).all() and (out[total:] == FILL).all()
    assert (base.cpu().numpy() == pc.cat(bases)).all()


# ---------------------------------------------------------------------------------------------------------------- old paths
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _same_object(a, b):
    assert len(a.groups) == len(b.groups) and a.delta == b.delta and a.delta_op == b.delta_op
    for g, h in zip(a.groups, b.groups):
        for key in ("frames", "frame_offsets", "frame_results", "tensor_results"):
            assert torch.equal(g[key], h[key]), key
        assert ("codecs" in g) == ("codecs" in h) and ("codecs" not in g or torch.equal(g["codecs"], h["codecs"]))


def _update(gen, dtype, shape):
    old = torch.randint(-100, 100, shape, generator=gen, device="cuda", dtype=torch.int32).to(dtype)
    new = old + (torch.randint(0, 8, shape, generator=gen, device="cuda") == 0).to(dtype)
    return old, new


def test_op_calls_with_xor_are_the_old_xor_calls(hip, monkeypatch):
    """every one of the ten *_op_dbatch calls with FSEHIP_DELTA_XOR against the call without _op: the same planes, frames, offsets, results and
    tensors, through the Python surface (which reaches the old names for XOR) with the old names rerouted to their siblings"""
    from finitestateentropy_amd.api import AutoCodec
    E = 4
    tensors, bases = _pairs(E)
    old_split = run_split(hip, tensors, bases, E, shift=SHIFTS[1], op=XOR)
    check_split(old_split, tensors, bases, E, op=XOR)
    buf, _, P, _ = pdc.split_xor_model(tensors, bases, E)
    psizes = [pc.plane_size(len(t), p, E) for t in tensors for p in range(E)]
    D = [int(x) for x in pc.offsets(tensors)]
    old_merge = run_merge(hip, E, buf, P[:-1], psizes, D, pc.cat(bases), shift=SHIFTS[1], op=XOR)
    assert (old_merge[0][:D[-1]] == pc.cat(tensors)).all()
    gen = torch.Generator(device="cuda").manual_seed(31)
    pairs = [_update(gen, torch.int16, (70, 100)), _update(gen, torch.int32, (5000,)), _update(gen, torch.int8, (3, 1000)), _update(gen, torch.int64, (2100,))]
    old, new = [p[0] for p in pairs], [p[1] for p in pairs]
    wins = [(100, 4100), None, (0, 3000), (2047, 2049)]
    newer = [t.clone() for t in new]
    for t, w in zip(newer, wins):
        if w is not None:
            t.view(-1)[w[0]:w[1]] += 1

    def flows():
        plain = hip.compress_tensors(new, 1, 0, base=old)
        auto = hip.compress_tensors(new, AutoCodec(20), 0, base=old)
        seg = hip.compress_tensors_segmented(new, 10, AutoCodec(0), 0, base=old)
        patched = hip.patch_tensor_windows(seg, newer, wins, base=old)
        k = 14                                               # the tensor of three tiles and five bytes: the segments that hold elements 100 .. 5000 of it, staged
        staged = hip.planes_split_window_dbatch(_dev(tensors[k]), [0, len(tensors[k])], [(100, 5000)], E, 10, base=_dev(bases[k]))
        return (plain, auto, seg, patched, hip.decompress_tensors(plain, base=old), hip.decompress_tensors(seg, base=old),
                hip.decompress_tensor_windows(seg, wins, base=old), hip.decompress_tensors(patched, base=old), list(staged))
    before = flows()
    calls = []
    for name, at in BASE_AT.items():
        sibling = getattr(hip.lib, name.replace("_xor_", "_").replace("_dbatch", "_op_dbatch"))

        def rerouted(*args, _f=sibling, _at=at, _name=name):
            calls.append(_name)
            return _f(*args[:_at + 1], C.c_uint(XOR), *args[_at + 1:])
        monkeypatch.setattr(hip.lib, name, rerouted)
    new_split = run_split(hip, tensors, bases, E, shift=SHIFTS[1], op=XOR)
    new_merge = run_merge(hip, E, buf, P[:-1], psizes, D, pc.cat(bases), shift=SHIFTS[1], op=XOR)
    after = flows()
    assert set(calls) == set(BASE_AT), "every call was reached through its sibling"
    assert (new_split[0] == old_split[0]).all() and new_split[1:] == old_split[1:] and (new_merge[0] == old_merge[0]).all() and new_merge[1] == old_merge[1]
    for a, b in zip(before[:4], after[:4]):
        _same_object(a, b)
    for a, b in zip(before[4:], after[4:]):
        assert all((x is None and y is None) or _bits(x, y) for x, y in zip(a, b))
    assert all(_bits(x, y) for x, y in zip(after[4], new)) and all(_bits(x, y) for x, y in zip(after[7], newer))


# ---------------------------------------------------------------------------------------------------------------- Python
def test_delta_base_through_the_python_surface(hip, monkeypatch):
    from finitestateentropy_amd.api import AutoCodec, DeltaBase
    gen = torch.Generator(device="cuda").manual_seed(13)
    old_np, new_np = pdc.bf16_update_pair(1 << 16)
    old_bf, new_bf = (torch.from_numpy(x.copy()).cuda().view(torch.bfloat16).reshape(256, 256) for x in (old_np, new_np))
    old_f = torch.randn((1000, 3), generator=gen, device="cuda") * 0.02
    new_f = old_f * (1 + torch.randn((1000, 3), generator=gen, device="cuda") * 1e-3)
    old_i = torch.randint(-128, 128, (4, 50), generator=gen, device="cuda", dtype=torch.int8)
    new_i = old_i.clone(); new_i[1, ::7] += 1
    old_d = torch.randint(-2 ** 62, 2 ** 62, (17,), generator=gen, device="cuda", dtype=torch.int64)
    old_d[:2] = torch.tensor([0x7FF8000000000001, 0xFFF0000000000002 - (1 << 64)], dtype=torch.int64)      # NaN payloads: bits, not values, count
    new_d = old_d.clone(); new_d[0] += 1; new_d[5] ^= 0xFF00; new_d[6] -= 1 << 40
    old_d, new_d = old_d.view(torch.float64), new_d.view(torch.float64)
    assert bool(torch.isnan(new_d).any())
    empty = torch.zeros((0, 3), device="cuda", dtype=torch.float32)
    old, new = [old_bf, old_f, old_i, old_d, empty], [new_bf, new_f, new_i, new_d, empty.clone()]
    keep = [t.clone() for t in old]
    obj = hip.compress_tensors(new, base=DeltaBase(old))
    assert obj.delta is True and obj.delta_op == "sub" and sorted(g["elem_bytes"] for g in obj.groups) == [1, 2, 4, 8]
    for base in (old, DeltaBase(old), DeltaBase(old, "sub"), tuple(old)):          # reading back with a plain base, or a DeltaBase of the object's op
        back = hip.decompress_tensors(obj, base=base)
        assert len(back) == len(new)
        for a, b, o, k in zip(new, back, old, keep):
            assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and _bits(a, b)
            assert _bits(o, k) and (b.numel() == 0 or b.data_ptr() != o.data_ptr()), "the bases are as they were, the results own their memory"
    # the op is the object's: an XOR object of the same pair has other frames, and "xor" through DeltaBase is the plain sequence
    xor = hip.compress_tensors(new, base=old)
    assert xor.delta_op == "xor" and "delta_op" not in vars(xor)
    _same_object(xor, hip.compress_tensors(new, base=DeltaBase(old, "xor")))
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(xor, base=DeltaBase(old, "xor")), new))
    one_sub, one_xor = hip.compress_tensors([new_bf], base=DeltaBase([old_bf])), hip.compress_tensors([new_bf], base=[old_bf])
    print("bf16 update, %d bytes: frames of the planes of the XOR %d, of the SUB delta %d" % (new_bf.numel() * 2, one_xor.nbytes, one_sub.nbytes))
    assert 0 < one_sub.nbytes < one_xor.nbytes
    # AutoCodec, an earlier object given back as codec, and the segmented calls
    auto = hip.compress_tensors(new, AutoCodec(10), base=DeltaBase(old))
    again = hip.compress_tensors(new, auto, base=DeltaBase(old))
    assert auto.delta_op == again.delta_op == "sub"
    _same_object(auto, again)
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(again, base=old), new))
    seg = hip.compress_tensors_segmented(new, 15, 0, base=DeltaBase(old))
    assert seg.delta_op == "sub" and seg.segment_log == 15
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(seg, base=old), new))
    wins = [(1000, 40000), (5, 2000), None, (0, 17), (0, 0)]
    got = hip.decompress_tensor_windows(seg, wins, base=DeltaBase(old))
    for t, w, x in zip(new, wins, got):
        assert (x is None) == (w is None) and (w is None or _bits(x, t.reshape(-1)[w[0]:w[1]]))
    newer = [t.clone() for t in new]
    newer[0].view(-1)[1000:40000] *= 1.001
    newer[3].view(torch.int64)[3] += 5
    patched = hip.patch_tensor_windows(seg, newer, wins, base=old)
    assert patched.delta_op == "sub"
    _same_object(patched, hip.compress_tensors_segmented(newer, 15, 0, base=DeltaBase(old)))
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensors(patched, base=DeltaBase(old)), newer))

    # every mismatch is raised before a launch: from here on a call into the library is a failure of the test
    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in list(BASE_AT) + [n.replace("_xor_", "_").replace("_dbatch", "_op_dbatch") for n in BASE_AT] + ["FSEHIP_tensor_compress_dbatch", "FSEHIP_tensor_decompress_dbatch"]:
        monkeypatch.setattr(hip.lib, name, no_launch)
    with pytest.raises(ValueError):
        DeltaBase(old, "add")
    with pytest.raises(ValueError):
        hip.decompress_tensors(obj, base=DeltaBase(old, "xor"))              # a base that contradicts the object's op
    with pytest.raises(ValueError):
        hip.decompress_tensors(xor, base=DeltaBase(old))
    with pytest.raises(ValueError):
        hip.decompress_tensor_windows(seg, wins, base=DeltaBase(old, "xor"))
    with pytest.raises(ValueError):
        hip.patch_tensor_windows(seg, newer, wins, base=DeltaBase(old, "xor"))
    with pytest.raises(ValueError):
        hip.compress_tensors(new, base=DeltaBase(old[:-1]))                  # one base too few
    with pytest.raises(ValueError):
        hip.compress_tensors(new, base=DeltaBase([old_bf.reshape(-1)] + old[1:]))
    with pytest.raises(TypeError):
        hip.compress_tensors(new, base=DeltaBase([old_bf.view(torch.float16)] + old[1:]))
    with pytest.raises(TypeError):
        hip.compress_tensors(new, base=DeltaBase([None] + old[1:]))
    with pytest.raises(ValueError):
        hip.decompress_tensors(obj)                                          # a delta object without its base
    with pytest.raises(ValueError):
        hip.decompress_tensors(hip_plain(hip), base=DeltaBase([old_bf]))     # a plain object with one
    with pytest.raises(ValueError):
        hip.decompress_tensors(obj, base=DeltaBase(old[1:]))
    with pytest.raises(ValueError):
        hip.tensor_compress_delta_dbatch(torch.zeros(8, dtype=torch.uint8, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda"), [0, 8], 2, delta_op=2)


def hip_plain(hip):
    """a plain object that needs no call: what compress_tensors([]) gives"""
    return hip.compress_tensors([])

"""A transform per tensor on the device (the six FSEHIP_*_each_dbatch calls and compress_tensors_each) -- byte for byte against the four
dedicated calls run per transform on the same tensors, and against the dispatching numpy model of planes_each_corpus.py.  Tile T = 32 KB,
run = 1024 elements, block-size id 0 wherever frames are involved.  Every destination is filled with 0xA5 and has a tail behind it:
whatever the contract does not give to the call must still be 0xA5 afterwards."""
import numpy as np
import pytest
import torch

import planes_corpus as pc
import planes_each_corpus as pe
import planes_estimate_corpus as pest
import planes_pred_corpus as ppc
from planes_corpus import GENERIC, TILE
from planes_each_corpus import IDS, PLAIN, PRED, SUB, XOR

pytestmark = pytest.mark.gpu

FILL, TAIL = 0xA5, 64
SHIFTS = ((0, 0, 0), (1, 5, 9), (8, 15, 3), (3, 2, 13))     # source, base, destination: each off 16-byte alignment by an amount of its own
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
    return list(range(34)) + [1023, 1024, 1025, 2047, 2048, 2049, per - 1, per, per + 1, 3 * per + 5]


def _corpus(E):
    """-> (tensors, bases, tiny, cross): every count of the issue as whole elements and again with n mod E != 0; then sixty tiny tensors that
    share one tile (tensors[tiny[0]:tiny[1]]); then seventeen tensors of exactly one tile, each starting where a tile starts
    (tensors[cross[0]:cross[1]]: neighbours across a tile boundary), the list in front of them padded to a tile; a smooth tensor of several
    tiles and the edge values as neighbours behind them.  The base of every tensor is a near copy or random"""
    if E not in _CACHE:
        rng = np.random.default_rng(700 + E)
        tensors = []
        for k, c in enumerate(counts(E)):
            tensors.append(rng.integers(0, 256, c * E, dtype=np.uint8))
            if E > 1:
                tensors.append(rng.integers(0, 256, c * E + 1 + k % (E - 1), dtype=np.uint8))
        at = sum(len(t) for t in tensors)
        tensors.append(rng.integers(0, 256, -at % TILE, dtype=np.uint8))          # the tiny ones start a tile ...
        tiny = (len(tensors), len(tensors) + 60)
        tensors += [rng.integers(0, 256, int(n), dtype=np.uint8) for n in rng.integers(1, 41, 60)]
        assert sum(len(t) for t in tensors[tiny[0]:tiny[1]]) < TILE // 8, "... and share it"
        at = sum(len(t) for t in tensors)
        tensors.append(rng.integers(0, 256, -at % TILE, dtype=np.uint8))
        cross = (len(tensors), len(tensors) + 17)
        tensors += [rng.integers(0, 256, TILE, dtype=np.uint8) for _ in range(17)]
        steps = rng.integers(-3, 4, 5 * TILE // E + 77).astype(np.int64)
        smooth = (np.cumsum(steps) + 1000).astype(np.uint64).astype(ppc._U[E]).view(np.uint8)
        tensors += [np.concatenate([smooth, np.arange(1, E, dtype=np.uint8)]), ppc.edge_sequence(E, 15)]
        bases = []
        for k, t in enumerate(tensors):
            b = rng.integers(0, 256, len(t), dtype=np.uint8)
            if k % 3 == 0 and len(t):                          # a near copy: most bytes equal, the deltas' zero planes
                b = t.copy()
                b[rng.integers(0, len(t), max(len(t) // 50, 1))] ^= 1
            bases.append(b)
        bases[-1] = np.roll(tensors[-1], 3 * E)
        _CACHE[E] = (tensors, bases, tiny, cross)
    return _CACHE[E]


def _arrays(E):
    """the transform arrays of the mix: the four uniform ones, and two walks over all 16 ordered pairs, placed so that every pair occurs
    between neighbours among the sixty tiny tensors of one tile and across the tile boundaries of the seventeen"""
    tensors, _, tiny, cross = _corpus(E)
    n = len(tensors)
    mixes = []
    for lead in (0, 7):
        tr = pe.cycle_all_pairs(n, lead)
        assert pe.neighbour_pairs(tr, tiny[0], tiny[1]) == set(pe.PAIRS) and pe.neighbour_pairs(tr, cross[0], cross[1]) == set(pe.PAIRS)
        mixes.append(tr)
    return [[tr] * n for tr in IDS] + mixes


def _dedicated(hip, E):
    """the planes of the four dedicated splits on the corpus, each run once: transform -> (planes as numpy, plane offsets, results)"""
    key = ("dedicated", E)
    if key not in _CACHE:
        tensors, bases, _, _ = _corpus(E)
        S = pc.offsets(tensors)
        src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))
        runs = {PLAIN: hip.planes_split_dbatch(src, S, E), PRED: hip.planes_split_pred_dbatch(src, S, E), XOR: hip.planes_split_xor_dbatch(src, base, S, E),
                SUB: hip.planes_split_xor_dbatch(src, base, S, E, delta_op=1)}
        torch.cuda.synchronize()
        _CACHE[key] = {tr: (p.cpu().numpy()[:int(S[-1])], o.cpu().tolist(), r.cpu().tolist()) for tr, (p, o, r) in runs.items()}
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------- split
def run_split(hip, tensors, bases, E, transforms, capacity=None, shift=(0, 0, 0), offsets=None):
    S = pc.offsets(tensors) if offsets is None else np.asarray(offsets, np.uint64)
    n, total = len(S) - 1, sum(len(t) for t in tensors)
    src, planes = _filled(total, shift[0], pc.cat(tensors)), _filled(total, shift[2])
    base = None if bases is None else _filled(total, shift[1], pc.cat(bases))
    poff = torch.full((n * E + 2,), -7, dtype=torch.int64, device="cuda")
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    tr = _filled(n, 1, np.asarray(transforms, np.uint8))
    hip.planes_split_each_dbatch(src[:total], S, E, tr[:n], base=None if base is None else base[:total], capacity=capacity, planes=planes, plane_offsets=poff, results=res)
    torch.cuda.synchronize()
    assert int(poff[n * E + 1]) == -7 and int(res[n]) == -7
    for buf, content in ((src, pc.cat(tensors)), (base, None if bases is None else pc.cat(bases)), (tr, np.asarray(transforms, np.uint8))):
        if buf is not None:
            host = buf.cpu().numpy()
            assert (host[:len(content)] == content).all() and (host[len(content):] == FILL).all(), "the source, the base and the transforms are only read"
    return planes.cpu().numpy(), poff.cpu().tolist()[:n * E + 1], res.cpu().tolist()[:n]


def check_split(got, tensors, bases, E, transforms, capacity=None):
    out, poff, res = got
    want, written, P, wres = pe.split_each_model(tensors, bases, E, transforms, capacity)
    assert poff == P and res == wres
    total = len(want)
    assert (out[:total][written] == want[written]).all(), np.nonzero((out[:total] != want) & written)[0][:8]
    outside = np.ones(len(out), bool)
    outside[:total] = ~written
    assert (out[outside] == FILL).all(), ("bytes outside the accepted tensors' planes", np.nonzero((out != FILL) & outside)[0][:8])


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_each_byte_for_byte(hip, E):
    tensors, bases, _, _ = _corpus(E)
    sizes = [len(t) for t in tensors]
    assert all(c * E in sizes for c in counts(E)) and (E == 1 or all(any(c * E < s < (c + 1) * E for s in sizes) for c in counts(E)))
    S = [int(x) for x in pc.offsets(tensors)]
    ded = _dedicated(hip, E)
    for k, transforms in enumerate(_arrays(E)):
        got = run_split(hip, tensors, bases, E, transforms, shift=SHIFTS[k % 4])
        check_split(got, tensors, bases, E, transforms)                                    # the model ...
        assert all(got[1] == ded[tr][1] and got[2] == ded[tr][2] for tr in IDS), "the layout and the results of every dedicated call"
        for i, tr in enumerate(transforms):                                                # ... and the dedicated call of every tensor's transform
            assert (got[0][S[i]:S[i + 1]] == ded[tr][0][S[i]:S[i + 1]]).all(), (k, i, tr)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_each_refusals_and_a_short_capacity(hip, E):
    tensors, bases, tiny, _ = _corpus(E)
    n = len(tensors)
    S = [int(x) for x in pc.offsets(tensors)]
    # transform bytes 4 and 0xFF among good ones, inside the shared tile and in front of large tensors
    transforms = pe.cycle_all_pairs(n, 3)
    for i in (2, 5, tiny[0] + 7, tiny[0] + 8, tiny[1] + 3, n - 2):
        transforms[i] = 4 if i % 2 else 0xFF
    got = run_split(hip, tensors, bases, E, transforms, shift=SHIFTS[1])
    check_split(got, tensors, bases, E, transforms)
    assert all(got[2][i] == GENERIC and (got[0][S[i]:S[i + 1]] == FILL).all() for i in (2, 5, tiny[0] + 7, n - 2))
    # XOR and SUB with a NULL base: refused per tensor, PLAIN and PRED run
    transforms = pe.cycle_all_pairs(n, 1)
    got = run_split(hip, tensors, None, E, transforms, shift=SHIFTS[2])
    check_split(got, tensors, None, E, transforms)
    assert [r == GENERIC for r in got[2]] == [tr >= XOR for tr in transforms]
    # a short capacity: inside a tensor, at a tensor's end, one short of it, nothing
    k = next(i for i, t in enumerate(tensors) if len(t) == TILE)
    transforms = pe.cycle_all_pairs(n, 11)
    for cap in (S[k] + 100, S[k + 1], S[k + 1] - 1, S[6], 0):
        got = run_split(hip, tensors, bases, E, transforms, capacity=cap, shift=SHIFTS[3])
        check_split(got, tensors, bases, E, transforms, cap)
        first = next(i for i in range(n) if S[i + 1] > cap)
        assert got[2][first:] == [GENERIC] * (n - first) and (got[0][S[first]:] == FILL).all(), "nothing of a refused tensor is written"


@pytest.mark.parametrize("E", pc.ELEMS)
def test_a_decreasing_offset_slot(hip, E):
    """offsets that decrease are the caller's error; what holds: the layout and the results are those of the dedicated call, the tensors the
    slot does not touch are split as ever, and no byte outside [0, capacity) is written"""
    rng = np.random.default_rng(43)
    flat, bflat = rng.integers(0, 256, 320, dtype=np.uint8), rng.integers(0, 256, 320, dtype=np.uint8)
    offsets = [0, 100, 60, 200, 300, 370]                       # slot 1 decreases, slot 4 ends behind the capacity
    for tr in IDS:
        got = run_split(hip, [flat], [bflat], E, [tr] * 5, capacity=320, offsets=offsets, shift=SHIFTS[1])
        src = _dev(flat)
        _, poff, res = hip.planes_split_pred_dbatch(src, np.asarray(offsets, np.uint64), E, capacity=320)
        torch.cuda.synchronize()
        assert got[1] == poff.cpu().tolist() and got[2] == res.cpu().tolist() == [100, 0, 140, 100, GENERIC]
        want = pe.split_each_model([flat[200:300]], [bflat[200:300]], E, [tr])[0]
        assert (got[0][200:300] == want).all() and (got[0][300:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- merge
def run_merge(hip, E, planes_buf, poff, psizes, D, transforms, bases=None, in_place=False, capacity=None, shift=(0, 0, 0)):
    n, room = len(D) - 1, int(D[-1])
    planes = _filled(len(planes_buf), shift[0], planes_buf)
    content = None if bases is None else pc.cat(bases)
    dst = _filled(room, shift[2], content if in_place else None)
    base = None if bases is None else dst if in_place else _filled(room, shift[1], content)
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    tr = _filled(n, 1, np.asarray(transforms, np.uint8))
    out, _ = hip.planes_merge_each_dbatch(planes[:max(len(planes_buf), 1)], _i64(poff), _i64(psizes), np.asarray(D, np.uint64), E, tr[:n],
                                          base=None if base is None else base[:room], dst=dst, capacity=room if capacity is None else capacity, results=res)
    torch.cuda.synchronize()
    assert int(res[n]) == -7 and out.data_ptr() == dst.data_ptr()
    host = planes.cpu().numpy()
    assert (host[:len(planes_buf)] == planes_buf).all() and (host[len(planes_buf):] == FILL).all(), "the planes are only read"
    if base is not None and not in_place:
        host = base.cpu().numpy()
        assert (host[:room] == content).all() and (host[room:] == FILL).all(), "the base is only read"
    return dst.cpu().numpy(), res.cpu().tolist()[:n]


@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_each_is_the_exact_inverse(hip, E):
    tensors, bases, _, _ = _corpus(E)
    n = len(tensors)
    S = [int(x) for x in pc.offsets(tensors)]
    ded = _dedicated(hip, E)
    flat = pc.cat(tensors)
    for k, transforms in enumerate(_arrays(E)):
        planes, _, P, _ = pe.split_each_model(tensors, bases, E, transforms)
        if len(set(transforms)) == 1:
            assert (planes == ded[transforms[0]][0]).all(), "the planes the dedicated split wrote: merged back below"
        psz = [P[j + 1] - P[j] for j in range(n * E)]
        for in_place in (False, True):
            out, res = run_merge(hip, E, planes, P[:-1], psz, S, transforms, bases, in_place, shift=SHIFTS[(k + in_place) % 4])
            assert res == [len(t) for t in tensors] and (out[:S[-1]] == flat).all() and (out[S[-1]:] == FILL).all(), (k, in_place)
    # without a base: PLAIN and PRED tensors are rebuilt, XOR and SUB ones refused and not written
    transforms = pe.cycle_all_pairs(n, 9)
    planes, _, P, _ = pe.split_each_model(tensors, bases, E, transforms)
    psz = [P[j + 1] - P[j] for j in range(n * E)]
    out, res = run_merge(hip, E, planes, P[:-1], psz, S, transforms, None, shift=SHIFTS[2])
    for i, tr in enumerate(transforms):
        assert res[i] == (len(tensors[i]) if tr < XOR else GENERIC) and (out[S[i]:S[i + 1]] == (tensors[i] if tr < XOR else FILL)).all(), i


@pytest.mark.parametrize("E", pc.ELEMS)
def test_a_refused_tensor_in_an_in_place_merge_keeps_its_old_bytes(hip, E):
    tensors, bases, tiny, _ = _corpus(E)
    n = len(tensors)
    S = [int(x) for x in pc.offsets(tensors)]
    transforms = pe.cycle_all_pairs(n, 2)
    planes, _, P, _ = pe.split_each_model(tensors, bases, E, transforms)
    psz = [P[j + 1] - P[j] for j in range(n * E)]
    refused = [3, tiny[0] + 5, tiny[0] + 6, n - 2, n - 1]
    given = list(transforms)
    for i in refused:
        given[i] = 4 if i % 2 else 0xFF
    damaged = next(i for i in range(n) if len(tensors[i]) == 2049 * E)      # ... and a tensor one of whose planes failed in the reader
    psz[damaged * E + E - 1] = GENERIC
    out, res = run_merge(hip, E, planes, P[:-1], psz, S, given, bases, True, shift=SHIFTS[3])
    for i in range(n):
        if i in refused:
            assert res[i] == GENERIC and (out[S[i]:S[i + 1]] == bases[i]).all(), i
        elif i == damaged:
            assert res[i] < 0 and (out[S[i]:S[i + 1]] == bases[i]).all(), "a failed tensor keeps its old bytes too"
        else:
            assert res[i] == len(tensors[i]) and (out[S[i]:S[i + 1]] == tensors[i]).all(), i
    assert (out[S[-1]:] == FILL).all()
    # a short capacity, and a slot that is too small
    cap = S[n - 3] + 5
    out, res = run_merge(hip, E, planes, P[:-1], [P[j + 1] - P[j] for j in range(n * E)], S, transforms, bases, False, capacity=cap, shift=SHIFTS[1])
    first = next(i for i in range(n) if S[i + 1] > cap)
    assert res[first:] == [GENERIC] * (n - first) and (out[S[first]:] == FILL).all() and (out[:S[first]] == pc.cat(tensors)[:S[first]]).all()


# ---------------------------------------------------------------------------------------------------------------- composites
def _small(E):
    """a short list for the composites: empty, tiny, odd, more than a run, a tile and more; bases near or random"""
    key = ("small", E)
    if key not in _CACHE:
        rng = np.random.default_rng(800 + E)
        sizes = [0, 1, 33 * E + (E > 1), 1025 * E, 2049 * E + (E > 1), TILE + E + (E > 1), 3000, 16 * E]
        tensors = []
        for k, s in enumerate(sizes):
            if k % 2:
                tensors.append(rng.integers(0, 256, s, dtype=np.uint8))
            else:                                               # compressible: a slow walk as elements of E bytes
                walk = (np.cumsum(rng.integers(-2, 3, s // E + 1)) + 500).astype(np.uint64).astype(ppc._U[E]).view(np.uint8)
                tensors.append(walk[:s].copy())
        bases = []
        for k, t in enumerate(tensors):
            b = t.copy()
            if len(b):
                b[rng.integers(0, len(b), max(len(b) // 40, 1))] ^= 3
            bases.append(b if k % 3 else rng.integers(0, 256, len(t), dtype=np.uint8))
        _CACHE[key] = (tensors, bases)
    return _CACHE[key]


def _frames(dst, foff, first):
    """per tensor the bytes of its frames, back to back"""
    dst, foff = dst.cpu().numpy(), foff.cpu().tolist()
    return [dst[foff[a]:foff[b]].tobytes() for a, b in zip(first, first[1:])]


@pytest.mark.parametrize("segment_log", [None, 10, 11])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_composites_write_the_frames_of_the_dedicated_composites(hip, E, segment_log):
    from finitestateentropy_amd.api import AutoCodec
    tensors, bases = _small(E)
    n, S = len(tensors), pc.offsets(tensors)
    src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))
    seg = segment_log is not None
    sf = hip.planes_segment_first(np.diff(S.astype(np.int64)), E, segment_log) if seg else None
    first = [int(sf[i * E]) for i in range(n + 1)] if seg else [i * E for i in range(n + 1)]
    for codec in (0, AutoCodec()):
        auto = isinstance(codec, AutoCodec)
        ded = {}
        for tr in IDS:                                          # the dedicated composite of every transform over the whole list
            b, op = (base if tr >= XOR else None), int(tr == SUB)
            if tr == PRED:
                r = (hip.tensor_compress_seg_pred_dbatch(src, S, E, segment_log, sf, codec=codec, block_size_id=0) if seg else
                     hip.tensor_compress_pred_dbatch(src, S, E, codec=codec, block_size_id=0))
            elif seg:
                r = hip.tensor_compress_seg_dbatch(src, S, E, segment_log, sf, base=b, codec=codec, block_size_id=0, delta_op=op)
            elif auto:
                r = hip.tensor_compress_mixed_dbatch(src, S, E, b, None, codec.tolerance_permille, 0, delta_op=op)
            elif b is None:
                r = hip.tensor_compress_dbatch(src, S, E, 0, codec) + (None,)
            else:
                r = hip.tensor_compress_delta_dbatch(src, b, S, E, 0, codec, delta_op=op) + (None,)
            assert int(r[2].min()) >= 0 and r[3].cpu().tolist() == [len(t) for t in tensors]
            ded[tr] = (_frames(r[0], r[1], first), None if r[4] is None else r[4].cpu().tolist())
        for transforms in ([tr] * n for tr in IDS), (pe.cycle_all_pairs(n, 0),), (pe.cycle_all_pairs(n, 5),):
            for given in transforms:
                if seg:
                    dst, foff, fres, tres, codecs, tr = hip.tensor_compress_seg_each_dbatch(src, S, E, segment_log, given, base, seg_first=sf, codec=codec, block_size_id=0)
                else:
                    dst, foff, fres, tres, codecs, tr = hip.tensor_compress_each_dbatch(src, S, E, given, base, codec=codec, block_size_id=0)
                assert int(fres.min()) >= 0 and tres.cpu().tolist() == [len(t) for t in tensors] and tr.cpu().tolist() == given
                got = _frames(dst, foff, first)
                for i, t in enumerate(given):
                    assert got[i] == ded[t][0][i], (E, segment_log, auto, given, i)
                    assert not auto or codecs.cpu().tolist()[first[i]:first[i + 1]] == ded[t][1][first[i]:first[i + 1]], "the codec of every frame"
                # ... and back, in place over a copy of the bases
                held = base.clone()
                total = int(foff[-1])
                if seg:
                    out, res = hip.tensor_decompress_seg_each_dbatch(dst[:total], foff, S, E, segment_log, given, held, sf, dst=held)
                else:
                    out, res = hip.tensor_decompress_each_dbatch(dst[:total], foff, S, E, given, held, dst=held)
                assert res.cpu().tolist() == [len(t) for t in tensors] and torch.equal(out, src)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_a_damaged_frame_fails_its_tensor_alone(hip, E):
    tensors, bases = _small(E)
    n, S = len(tensors), pc.offsets(tensors)
    src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))
    given = pe.cycle_all_pairs(n, 4)
    dst, foff, fres, _, _, _ = hip.tensor_compress_each_dbatch(src, S, E, given, base, block_size_id=0)
    k = 4                                                       # 2049 elements: frame k * E, its last byte is the checksum's
    total = int(foff[-1])
    frames = dst[:total].clone()
    frames[int(foff[k * E]) + int(fres[k * E]) - 1] ^= 0x40
    held = base.clone()
    out, res = hip.tensor_decompress_each_dbatch(frames, foff, S, E, given, held, dst=held)
    res = res.cpu().tolist()
    assert res[k] < 0 and res[:k] + res[k + 1:] == [len(t) for i, t in enumerate(tensors) if i != k]
    a, b = int(S[k]), int(S[k + 1])
    assert torch.equal(out[:a], src[:a]) and torch.equal(out[b:], src[b:]) and torch.equal(out[a:b], base[a:b]), "the failed tensor keeps its old bytes"


# ---------------------------------------------------------------------------------------------------------------- transform CHOOSE
def _choosy(E, seed=0):
    """tensors whose best transforms differ: random bytes (plain), a slow walk (pred), a near copy of its base (xor / sub), zeros, nothing"""
    rng = np.random.default_rng(900 + E + seed)
    m = 3 * TILE // E + 5
    walk = (np.cumsum(rng.integers(-2, 3, m)) + 70000).astype(np.uint64).astype(ppc._U[E]).view(np.uint8).copy()
    noise = rng.integers(0, 256, 2 * TILE + 3, dtype=np.uint8)
    upd = rng.integers(0, 256, TILE + E * 7, dtype=np.uint8)
    ubase = upd.copy()
    ubase[rng.integers(0, len(upd), len(upd) // 64)] += 1
    tensors = [noise, walk, upd, np.zeros(777, np.uint8), np.zeros(0, np.uint8), walk[:1025 * E]]
    bases = [rng.integers(0, 256, len(noise), dtype=np.uint8), rng.integers(0, 256, len(walk), dtype=np.uint8), ubase, np.zeros(777, np.uint8), np.zeros(0, np.uint8),
             rng.integers(0, 256, 1025 * E, dtype=np.uint8)]
    return tensors, bases


@pytest.mark.parametrize("segment_log", [None, 10])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_choose_writes_the_estimate_s_choice_and_round_trips(hip, E, segment_log):
    tensors, bases = _choosy(E)
    n, S = len(tensors), pc.offsets(tensors)
    src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))
    for mask, margin, b in ((15, 50, base), (3, 0, None), (14, 300, base), (10, 1000, base)):
        _, eb, ch, _ = hip.planes_estimate_dbatch(src, S, E, mask, margin, base=b)
        est = torch.full((n * 4 + 1,), -7, dtype=torch.int64, device="cuda")
        if segment_log is None:
            dst, foff, fres, tres, _, tr = hip.tensor_compress_each_dbatch(src, S, E, None, b, mask, margin, est, block_size_id=0)
        else:
            dst, foff, fres, tres, _, tr = hip.tensor_compress_seg_each_dbatch(src, S, E, segment_log, None, b, mask, margin, est, block_size_id=0)
        want = ch.cpu().tolist()
        assert tr.cpu().tolist() == want and est.cpu().tolist() == eb.cpu().tolist() + [-7], (E, mask, margin)
        assert want == pest.estimate_model(tensors, E, mask, bases if b is not None else None, margin)[2], "the model's choice"
        assert mask != 15 or len(set(want)) >= 3, want
        assert int(fres.min()) >= 0 and tres.cpu().tolist() == [len(t) for t in tensors]
        # choose once, then give: the same frames
        if segment_log is None:
            again = hip.tensor_compress_each_dbatch(src, S, E, tr, b, block_size_id=0)
            held = None if b is None else b.clone()
            out, res = hip.tensor_decompress_each_dbatch(dst[:int(foff[-1])], foff, S, E, tr, held, dst=held)
        else:
            again = hip.tensor_compress_seg_each_dbatch(src, S, E, segment_log, tr, b, block_size_id=0)
            held = None if b is None else b.clone()
            out, res = hip.tensor_decompress_seg_each_dbatch(dst[:int(foff[-1])], foff, S, E, segment_log, tr, held, dst=held)
        assert torch.equal(again[1], foff) and torch.equal(again[0][:int(foff[-1])], dst[:int(foff[-1])])
        assert res.cpu().tolist() == [len(t) for t in tensors] and torch.equal(out[:int(S[-1])], src), "the round trip is exact"


# ---------------------------------------------------------------------------------------------------------------- graph
@pytest.mark.parametrize("choose", [True, False])
def test_the_composite_in_a_hip_graph_follows_changed_sources_and_transforms(hip, choose):
    """one graph of the segmented composite, captured once: CHOOSE replayed over changed sources whose best transforms differ returns the new
    choices and the new frames with no host read in between; GIVEN replayed with the array's contents changed writes the new frames.  The
    segment layout is host arithmetic on the sizes, so the loads keep the three sizes and rotate the KINDS of content (random bytes, a
    slow walk, a near copy of the base) over them"""
    import ctypes as C
    E, L = 2, 10
    t0, b0 = _choosy(E)
    order = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
    plans = [[PLAIN, PRED, SUB], [SUB, XOR, PRED], [PRED, PLAIN, XOR]]
    sizes = sorted(len(t0[i]) for i in (0, 1, 2))
    n, cap = 3, sum(sizes)
    S = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    sf = hip.planes_segment_first(sizes, E, L)
    nf = int(sf[-1])
    blocks = hip.planes_block_bound(cap, n, E, 0)
    src, base, planes = (torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(3))
    soff, sfd = _i64(S), _i64(sf)
    given, chosen = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(hip.frame_packed_bound(cap, nf, blocks, 0), dtype=torch.uint8, device="cuda")
    foff, so = torch.zeros(nf + 1, dtype=torch.int64, device="cuda"), torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
    fres, tres, poff = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (nf, n, n * E + 1))
    hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize.restype = C.c_size_t
    need = hip.tensor_each_workspace_head(n, E, choose, 15) + int(hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize(C.c_size_t(nf), C.c_size_t(blocks), C.c_uint(0),
                                                                                                                           C.c_int(0)))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def load(k):
        ts = [np.resize(t0[i], sizes[j]) for j, i in enumerate(order[k])]
        bs = [np.resize(b0[i], sizes[j]) for j, i in enumerate(order[k])]
        src.copy_(_dev(pc.cat(ts))); base.copy_(_dev(pc.cat(bs))); given.copy_(_dev(plans[k]))
        return ts, bs

    def work():
        hip.tensor_compress_seg_each_dbatch(src, soff, E, L, None if choose else given, base, 15 if choose else None, 50, seg_first=sfd, n_segments=nf, block_size_id=0,
                                            dst=dst, max_total_blocks=blocks, frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes,
                                            plane_offsets=poff, seg_offsets=so, workspace=ws, chosen=chosen if choose else None)

    def direct(ts, bs, tr):
        """the same batch through a call of its own, everything allocated afresh"""
        d, fo, _, _, _, _ = hip.tensor_compress_seg_each_dbatch(_dev(pc.cat(ts)), S, E, L, tr, _dev(pc.cat(bs)), seg_first=sf, block_size_id=0)
        torch.cuda.synchronize()
        return d[:int(fo[-1])].cpu().numpy().tobytes(), fo.cpu().tolist()
    load(0)
    work()                                                      # one ordinary call first
    torch.cuda.synchronize()
    seen = [chosen.cpu().tolist()]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    for k in (1, 2):
        ts, bs = load(k)
        for t in (dst, foff, fres, tres, chosen):
            t.fill_(3)
        ws.fill_(0x5A)
        g.replay()
        torch.cuda.synchronize()
        want_tr = pest.estimate_model(ts, E, 15, bs, 50)[2] if choose else plans[k]
        if choose:
            assert chosen.cpu().tolist() == want_tr and want_tr not in seen, (k, want_tr, seen)
            seen.append(want_tr)
        want = direct(ts, bs, want_tr)
        assert foff.cpu().tolist() == want[1] and dst[:int(foff[-1])].cpu().numpy().tobytes() == want[0], k
        assert int(fres.min()) >= 0 and tres.cpu().tolist() == sizes
        held = _dev(pc.cat(bs))
        out, res = hip.tensor_decompress_seg_each_dbatch(dst[:int(foff[-1])], foff, S, E, L, want_tr, held, sf, dst=held)
        assert res.cpu().tolist() == sizes and torch.equal(out, src)


# ---------------------------------------------------------------------------------------------------------------- Python
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _mixed_list():
    """the estimate test's mixed list: sorted int64, bf16 gaussian, a bf16 update, position ids, random bytes -- and the bases of the whole
    list: the update's own, for every other tensor something unrelated of its dtype and shape"""
    if "mixed" not in _CACHE:
        rng = np.random.default_rng(5)
        t, b = pest.update_pair()
        ts = [_dev(pest.sorted_int64()).view(torch.int64), _dev(pest.bf16_gaussian()).view(torch.bfloat16), _dev(t).view(torch.bfloat16),
              _dev(pest.position_ids()).view(torch.int32).reshape(8, 4096), _dev(rng.integers(0, 256, 5005, dtype=np.uint8)).reshape(5, 1001)]
        bases = [_dev(rng.integers(0, 1 << 40, 1 << 15).astype("<u8").view(np.uint8)).view(torch.int64), _dev(pc.bf16_gaussian(1 << 17, seed=9)).view(torch.bfloat16),
                 _dev(b).view(torch.bfloat16), _dev(rng.integers(0, 1 << 30, 1 << 15).astype("<u4").view(np.uint8)).view(torch.int32).reshape(8, 4096),
                 _dev(rng.integers(0, 256, 5005, dtype=np.uint8)).reshape(5, 1001)]
        _CACHE["mixed"] = (ts, bases)
    return _CACHE["mixed"]


@pytest.mark.parametrize("segment_log", [None, 18])
def test_compress_tensors_each_on_the_mixed_list(hip, segment_log):
    from finitestateentropy_amd.api import CompressedTensors
    ts, bases = _mixed_list()
    keep = [t.clone() for t in ts]
    for base in (None, bases):
        bundle = hip.compress_tensors_auto(ts, base=base, segment_log=segment_log)
        obj = hip.compress_tensors_each(ts, "auto", base, segment_log=segment_log)
        assert isinstance(obj, CompressedTensors) and obj.segment_log == segment_log and not obj.delta and obj.predictor is None
        assert obj.transforms == [r["choice"] for r in bundle.estimates] == ["pred", "plain", "sub" if base is not None else "plain", "pred", "plain"]
        assert obj.nbytes == bundle.nbytes, "the same frames, in one object"
        assert [g["elem_bytes"] for g in obj.groups] == [1, 2, 4, 8] and sorted(i for g in obj.groups for i in g["index"]) == list(range(len(ts)))
        # choose once, then give
        again = hip.compress_tensors_each(ts, obj.transforms, base, segment_log=segment_log)
        assert again.transforms == obj.transforms and all(torch.equal(a["frames"], b["frames"]) for a, b in zip(again.groups, obj.groups))
        # through an archive and back
        opened = hip.open_archive(hip.archive_tensors(obj))
        assert opened.transforms == obj.transforms and opened.segment_log == segment_log and opened.nbytes == obj.nbytes
        for o in (obj, opened):
            back = hip.decompress_tensors(o, base=base)
            assert len(back) == len(ts)
            for a, r, k in zip(ts, back, keep):
                assert a.dtype == r.dtype and a.shape == r.shape and a.device == r.device and _bits(a, r) and _bits(a, k)
        if base is not None:
            with pytest.raises(ValueError):
                hip.decompress_tensors(obj)
        else:
            assert all(_bits(a, r) for a, r in zip(ts, hip.decompress_tensors(obj, base=bases))), "a base that no tensor needs is not looked at"
        if segment_log is not None:
            with pytest.raises(ValueError):
                hip.decompress_tensor_windows(obj, [None] * len(ts), base=base)
    # every name given by hand, a zero-byte tensor among them
    ts2 = ts + [torch.zeros((0, 7), dtype=torch.float32, device="cuda")]
    names = ["sub", "xor", "pred", "plain", "sub", "xor"]
    obj = hip.compress_tensors_each(ts2, names, bases + [ts2[-1]], segment_log=segment_log)
    assert obj.transforms == names
    back = hip.decompress_tensors(hip.open_archive(hip.archive_tensors(obj)), base=bases + [ts2[-1]])
    assert all(_bits(a, r) and a.shape == r.shape for a, r in zip(ts2, back))

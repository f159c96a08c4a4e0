"""Segmented planes on the device (FSEHIP_planes_segments_dbatch / _fold_segments_dbatch, FSEHIP_tensor_compress_seg_dbatch / _decompress_seg_dbatch
and compress_tensors_segmented) against the numpy model of planes_seg_corpus.py and the CPU oracle's frame of every segment.  Block-size
id 0 with segLog 10 and 11: a few KB already make several segments.  Every output array is longer than the contract and pre-filled: whatever
the contract does not give to a call must still hold the fill afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_mixed_corpus as fmc
import frame_packed_corpus as fpc
import planes_corpus as pc
import planes_seg_corpus as psc
from planes_corpus import CORRUPT, GENERIC

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = 0xA5, 64, -7
SEG_LOGS = (10, 11)
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _i64(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).cuda()


def _marked(n, head=None):
    """n entries and one more, all MARK, the first ones `head`"""
    t = torch.full((n + 1,), MARK, dtype=torch.int64, device="cuda")
    if head is not None and len(head):
        t[:len(head)] = _i64(head)
    return t


def _filled(n, content=None):
    t = torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    if content is not None and len(content):
        t[:len(content)] = _dev(content)
    return t


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the segments kernel
def run_segments(hip, sizes, E, seg_log, first=None, capacity=None):
    n = len(sizes)
    right = psc.seg_first(sizes, E, seg_log)
    first = right if first is None else first
    P, split_res = psc.split_offsets(sizes, E, capacity)
    nseg = first[-1]
    so, tres = _marked(nseg + 1), _marked(n, split_res)
    poff, sf = _i64(P), _i64(first)
    hip.planes_segments_dbatch(poff, _offsets(sizes), sf, E, seg_log, n_segments=nseg, tensor_results=tres, seg_offsets=so)
    torch.cuda.synchronize()
    assert int(so[nseg + 1]) == MARK and int(tres[n]) == MARK, "one entry per segment and one more, one result per tensor"
    assert poff.cpu().tolist() == P and sf.cpu().tolist() == first, "the inputs are only read"
    want_off, want_res = psc.segments_model(sizes, E, seg_log, first, capacity)
    assert tres.cpu().tolist()[:n] == want_res
    assert so.cpu().tolist()[:nseg + 1] == want_off
    return want_off, want_res


def _long_sizes(E, seg_log):
    s = 1 << seg_log
    return psc.seg_sizes(E, seg_log) + [E * 65 * s + 5, 7, E * 1030 * s + 1]


@pytest.mark.parametrize("seg_log", SEG_LOGS)
@pytest.mark.parametrize("E", psc.ELEMS)
def test_segments_against_the_model(hip, E, seg_log):
    sizes = _long_sizes(E, seg_log)
    counts = np.diff(psc.seg_first(sizes, E, seg_log))
    assert 0 in sizes and 64 < counts[-3 * E] <= 1024 < counts[-E]
    off, res = run_segments(hip, sizes, E, seg_log)
    assert res == sizes and off[-1] == sum(sizes) and off == sorted(off)
    # the binding's own destination (guarded in guard mode) and its own segFirst
    P, _ = psc.split_offsets(sizes, E)
    so, tres = hip.planes_segments_dbatch(_i64(P), _offsets(sizes), psc.seg_first(sizes, E, seg_log), E, seg_log)
    assert so.cpu().tolist() == off and tres.cpu().tolist() == [0] * len(sizes)
    # more than 1024 planes of one segment each, an empty tensor among them
    many = [3 * E] * (1100 // E + 1) + [0] + [2 * E + 1] * 5
    assert len(many) * E > 1024 and psc.seg_first(many, E, seg_log)[-1] == len(many) * E
    run_segments(hip, many, E, seg_log)


@pytest.mark.parametrize("E", psc.ELEMS)
def test_segments_refuse_only_the_tensor_whose_counts_are_wrong(hip, E):
    seg_log = 10
    sizes = _long_sizes(E, seg_log)
    right = psc.seg_first(sizes, E, seg_log)
    victim = 7                                               # planes of 2 seg + 1 bytes (plane 0) and 2 seg
    wrong = list(right)
    wrong[victim * E + 1] -= 1                               # its first plane a segment short, the next plane (E == 1: the next tensor) one too many
    off, res = run_segments(hip, sizes, E, seg_log, wrong)
    refused = [i for i, r in enumerate(res) if r < 0]
    assert refused == ([victim] if E > 1 else [victim, victim + 1])
    good, _ = psc.segments_model(sizes, E, seg_log)
    a, b = right[refused[0] * E], right[(refused[-1] + 1) * E]
    assert off[:a] == good[:a] and off[b:] == good[b:] and set(off[a:wrong[(victim + 1) * E]]) == {sum(sizes[:victim])}
    # a count of nothing for every plane of a tensor: it is refused and has no entry at all
    gone = right[(victim + 1) * E] - right[victim * E]
    none = [x if j <= victim * E else right[victim * E] if j <= (victim + 1) * E else x - gone for j, x in enumerate(right)]
    off, res = run_segments(hip, sizes, E, seg_log, none)
    assert [i for i, r in enumerate(res) if r < 0] == [victim] and off == good[:a] + good[a + gone:]


@pytest.mark.parametrize("E", psc.ELEMS)
def test_segments_with_a_short_capacity(hip, E):
    seg_log = 11
    sizes = _long_sizes(E, seg_log)
    S = [int(x) for x in _offsets(sizes)]
    for cap in (S[5] + 1, S[5], S[-1] - 1, 0):
        off, res = run_segments(hip, sizes, E, seg_log, capacity=cap)
        bad = next(i for i in range(len(sizes)) if S[i + 1] > cap)
        a = psc.seg_first(sizes, E, seg_log)[bad * E]
        assert res[bad:] == [GENERIC] * (len(sizes) - bad) and off[a:] == [S[bad]] * (len(off) - a), "refused tensors keep their segment count, all of them empty"


# ---------------------------------------------------------------------------------------------------------------- the fold
def run_fold(hip, off, res, first, seg_log):
    npl, nseg = len(first) - 1, first[-1]
    assert len(off) == nseg + 1 and len(res) == nseg
    po, ps = _marked(npl), _marked(npl)
    doff, dres, sf = _i64(off), _i64(res), _i64(first)
    hip.planes_fold_segments_dbatch(doff, dres, sf, seg_log, n_segments=nseg, plane_offsets=po, plane_sizes=ps)
    torch.cuda.synchronize()
    assert int(po[npl]) == MARK and int(ps[npl]) == MARK
    assert doff.cpu().tolist() == off and dres.cpu().tolist() == res and sf.cpu().tolist() == first, "the inputs are only read"
    want = psc.fold_model(off, res, first, seg_log)
    assert ps.cpu().tolist()[:npl] == want[1]
    assert po.cpu().tolist()[:npl] == want[0]
    return want


@pytest.mark.parametrize("seg_log", SEG_LOGS)
@pytest.mark.parametrize("E", psc.ELEMS)
def test_fold_against_the_model(hip, E, seg_log):
    s = 1 << seg_log
    sizes = _long_sizes(E, seg_log)
    first = psc.seg_first(sizes, E, seg_log)
    off, _ = psc.segments_model(sizes, E, seg_log)
    good = [off[q + 1] - off[q] for q in range(first[-1])]
    po, ps = run_fold(hip, off, good, first, seg_log)
    assert ps == psc.plane_sizes(sizes, E) and po == psc.split_offsets(sizes, E)[0][:-1]
    # the binding's own destinations (guarded in guard mode)
    gpo, gps = hip.planes_fold_segments_dbatch(_i64(off), _i64(good), first, seg_log)
    assert gpo.cpu().tolist() == po and gps.cpu().tolist() == ps
    # errors and damage, each in a plane of its own
    long65, long1030 = first[-3 * E - 1], first[-E - 1]      # the first planes of the two long tensors
    res = list(good)
    res[long65 + 65], res[long65 + 3] = -2, -3               # two errors, the later one in an earlier lane's second round
    res[long1030 + 1029], res[long1030 + 64], res[long1030 + 1000] = -4, -5, -1
    res[first[7 * E] + 1] = s - 1                            # a short middle segment of the plane of 2 seg + 1 bytes
    res[first[4 * E] + 1] = 2                                # a last segment of 2 bytes where 1 was written: within 1 .. seg, only the sum differs
    res[first[0]] = -8                                       # a plane of one segment
    bad_off = list(off)
    if E > 1:
        bad_off[first[6 * E + 1] + 1] += 1                   # a gap inside plane 1 of the tensor of planes of 2 seg bytes
    _, ps = run_fold(hip, bad_off, res, first, seg_log)
    assert ps[-3 * E] == -3 and ps[-E] == -5 and ps[7 * E] == CORRUPT and ps[4 * E] == s + 2 and ps[0] == -8
    assert E == 1 or ps[6 * E + 1] == CORRUPT
    assert sum(1 for a, b in zip(ps, psc.plane_sizes(sizes, E)) if a != b) == (6 if E > 1 else 5)


def test_fold_one_case_per_branch_and_many_small_planes(hip):
    for seg_log in SEG_LOGS:
        off, res, first, want = [], [], [0], []
        for _, o, r, w in psc.fold_cases(seg_log):
            off += o[:-1]
            res += r
            first.append(first[-1] + len(r))
            want.append(w)
        off.append(12345)
        assert run_fold(hip, off, res, first, seg_log)[1] == want
    n = 1100
    sizes = [int(x) for x in np.random.default_rng(3).integers(0, 1025, n)]
    off = [int(x) for x in _offsets(sizes)]
    res = list(sizes)
    res[500], res[1099] = -3, 1025
    _, ps = run_fold(hip, off, res, list(range(n + 1)), 10)
    assert ps[500] == -3 and ps[1099] == CORRUPT and ps[:500] == sizes[:500]
    # a segFirst that runs past the segments: clamped, nothing outside the arrays is read
    run_fold_clamped = hip.planes_fold_segments_dbatch(_i64(off[:11]), _i64(res[:10]), _i64([0, 4, 40, 30]), 10, n_segments=10)
    torch.cuda.synchronize()
    assert run_fold_clamped[1].numel() == 3


# ---------------------------------------------------------------------------------------------------------------- the composites
def _corpus(E, seg_log):
    """(tensors, bases): compressible bf16 data over two segments and a bit, nothing, noise of exactly one segment per plane, a constant of a size
    that is no multiple of E, a skewed source of two segments and a half per plane; the bases differ from them in a byte in sixteen"""
    key = ("corpus", E, seg_log)
    if key not in _CACHE:
        s = 1 << seg_log
        rng = np.random.default_rng(60 + E + seg_log)
        tensors = [pc.bf16_gaussian(E * (2 * s + 100) // 2, 5 + E), np.zeros(0, np.uint8), rng.integers(0, 256, E * s, dtype=np.uint8),
                   np.full(E * (s + 1) + E - 1, 77, np.uint8), rng.integers(0, 4, 5 * E * s // 2, dtype=np.uint8)]
        bases = [t ^ (rng.integers(1, 256, t.size, dtype=np.uint8) * (rng.integers(0, 16, t.size) == 0)).astype(np.uint8) for t in tensors]
        _CACHE[key] = (tensors, bases)
    return _CACHE[key]


def _segments_of(tensors, E, seg_log):
    out = []
    for t in tensors:
        for pl in pc.planes_of(t, E):
            out += [np.ascontiguousarray(pl[a:a + (1 << seg_log)]) for a in (range(0, len(pl), 1 << seg_log) if len(pl) else [0])]
    return out


def _frames(oracle, E, seg_log, xor, codec):
    """the oracle's frame of every segment of every plane of the corpus (xor: of tensor XOR base)"""
    key = ("frames", E, seg_log, xor, codec)
    if key not in _CACHE:
        tensors, bases = _corpus(E, seg_log)
        data = [t ^ b for t, b in zip(tensors, bases)] if xor else tensors
        out = []
        for seg in _segments_of(data, E, seg_log):
            r, f = oracle.frame_compress(seg, 0, codec)
            out.append(f[:r].copy())
        _CACHE[key] = out
    return _CACHE[key]


def run_compress(hip, tensors, bases, E, seg_log, align_log, codec=0, codecs=None):
    n, S = len(tensors), _offsets([len(t) for t in tensors])
    total = int(S[-1])
    first = psc.seg_first([len(t) for t in tensors], E, seg_log)
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, first[-1], blocks, align_log)
    dst = _filled(fcap)
    src = _filled(total, pc.cat(tensors))
    base = None if bases is None else _filled(total, pc.cat(bases))[:total]
    _, foff, fres, tres, chosen = hip.tensor_compress_seg_dbatch(src[:total], S, E, seg_log, np.asarray(first, np.uint64), base=base, codec=codec, codecs=codecs,
                                                                  block_size_id=0, dst=dst, dst_capacity=fcap, max_total_blocks=blocks, align_log=align_log)
    torch.cuda.synchronize()
    assert foff.numel() == first[-1] + 1 and fres.numel() == first[-1]
    return dst, foff, fres, tres, chosen, fcap


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


@pytest.mark.parametrize("form", ["plain", "base", "given", "chosen"])
@pytest.mark.parametrize("E", psc.ELEMS)
def test_tensor_compress_seg_gives_the_oracles_frame_of_every_segment(hip, checker, E, form):
    from finitestateentropy_amd.api import AutoCodec
    for seg_log in SEG_LOGS:
        tensors, bases = _corpus(E, seg_log)
        xor = form != "plain"
        F, H = _frames(checker, E, seg_log, xor, 0), _frames(checker, E, seg_log, xor, 1)
        nseg = psc.seg_first([len(t) for t in tensors], E, seg_log)[-1]
        assert len(F) == len(H) == nseg > 5 * E
        for align_log in (0, 6):
            what = (E, form, seg_log, align_log)
            if form in ("plain", "base"):
                for codec, want in ((0, F), (1, H)):
                    dst, foff, fres, tres, chosen, fcap = run_compress(hip, tensors, bases if xor else None, E, seg_log, align_log, codec)
                    assert chosen is None
                    check_frames(want, dst, foff, fres, align_log, fcap, what)
            elif form == "given":
                given = [(q // 3) % 2 for q in range(nseg)]
                dst, foff, fres, tres, chosen, fcap = run_compress(hip, tensors, bases, E, seg_log, align_log, codecs=_dev(given))
                assert chosen.cpu().tolist() == given
                check_frames([H[q] if c else F[q] for q, c in enumerate(given)], dst, foff, fres, align_log, fcap, what)
            else:
                tol = 20
                dst, foff, fres, tres, chosen, fcap = run_compress(hip, tensors, bases, E, seg_log, align_log, AutoCodec(tol))
                want = [fmc.expected_choice(len(f), len(h), tol)[0] for f, h in zip(F, H)]
                assert chosen.cpu().tolist() == want, "the choice per segment is the mixed model's"
                check_frames([H[q] if c else F[q] for q, c in enumerate(want)], dst, foff, fres, align_log, fcap, what)
            assert tres.cpu().tolist() == [len(t) for t in tensors]


def run_decompress(hip, frames, foff, tensors, bases, E, seg_log, first, in_place=False, blocks=None):
    D = _offsets([len(t) for t in tensors])
    total = int(D[-1])
    base = None if bases is None else _filled(total, pc.cat(bases))
    back = base if in_place else _filled(total)
    res = _marked(len(tensors))
    hip.tensor_decompress_seg_dbatch(frames, foff, D, E, seg_log, np.asarray(first, np.uint64), base=base, dst=back, dst_capacity=total,
                                     max_total_blocks=hip.planes_block_bound(total, len(tensors), E, 0) if blocks is None else blocks, results=res)
    torch.cuda.synchronize()
    assert int(res[len(tensors)]) == MARK
    if base is not None and not in_place:
        assert (base.cpu().numpy()[:total] == pc.cat(bases)).all(), "a base that is not the destination is only read"
    return back.cpu().numpy(), res.cpu().tolist()[:len(tensors)]


@pytest.mark.parametrize("form", ["plain", "xor", "in_place"])
@pytest.mark.parametrize("E", psc.ELEMS)
def test_round_trip_a_damaged_segment_and_another_segment_size(hip, checker, E, form):
    seg_log = 10
    tensors, bases = _corpus(E, seg_log)
    xor, in_place = form != "plain", form == "in_place"
    sizes = [len(t) for t in tensors]
    D = [int(x) for x in _offsets(sizes)]
    first = psc.seg_first(sizes, E, seg_log)
    dst, foff, fres, _, _, fcap = run_compress(hip, tensors, bases if xor else None, E, seg_log, 0, 1)
    want = _frames(checker, E, seg_log, xor, 1)
    check_frames(want, dst, foff, fres, 0, fcap, form)
    back, res = run_decompress(hip, dst, foff, tensors, bases if xor else None, E, seg_log, first, in_place)
    assert res == sizes and (back[:D[-1]] == pc.cat(tensors)).all() and (back[D[-1]:] == FILL).all()
    # written with segLog 10, read with 11 and the sender's segFirst: every plane of more than one segment is not what the reader expects
    back, res = run_decompress(hip, dst, foff, tensors, bases if xor else None, E, 11, first, in_place)
    several = [any(first[j + 1] - first[j] > 1 for j in range(i * E, (i + 1) * E)) for i in range(len(tensors))]
    assert several == [True, False, False, True, True]
    assert res == [CORRUPT if m else n for m, n in zip(several, sizes)]
    untouched = pc.cat(bases) if in_place else np.full(D[-1], FILL, np.uint8)
    for i, m in enumerate(several):
        assert (back[D[i]:D[i + 1]] == (untouched if m else pc.cat(tensors))[D[i]:D[i + 1]]).all(), i
    # one byte flipped in the frame of a middle segment (tensor 4, noise of four symbols: compressed blocks): that tensor alone fails, with what the
    # oracle's reader says of that frame, and its slot -- in place: its old bytes -- is untouched
    victim = 4
    f = first[victim * E] + 1
    assert first[victim * E + 1] - first[victim * E] == 3
    at = 5 + 3 + 40
    assert len(want[f]) > at + 8
    bad = want[f].copy()
    bad[at] ^= 0x55
    r, _ = checker.frame_decompress(bad, 1 << seg_log)
    assert r > (1 << 63), "the oracle's reader refuses the damaged frame"
    dst[int(foff[f]) + at] ^= 0x55
    back, res = run_decompress(hip, dst, foff, tensors, bases if xor else None, E, seg_log, first, in_place)
    assert res == sizes[:victim] + [r - (1 << 64)] + sizes[victim + 1:]
    assert (back[D[victim]:D[victim + 1]] == untouched[D[victim]:D[victim + 1]]).all()
    assert (back[:D[victim]] == pc.cat(tensors)[:D[victim]]).all() and (back[D[victim + 1]:D[-1]] == pc.cat(tensors)[D[victim + 1]:]).all()
    assert (back[D[-1]:] == FILL).all()


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("E", psc.ELEMS)
def test_planes_of_at_most_one_segment_give_the_unsegmented_frames(hip, E, codec):
    seg_log = 12
    s = 1 << seg_log
    tensors = pc.random_tensors([E * s, 0, E * s - 1, 5, E * 700 + 3], 80 + E)
    tensors[0] = pc.bf16_gaussian(E * s // 2, 9)
    n, S = len(tensors), _offsets([len(t) for t in tensors])
    first = psc.seg_first([len(t) for t in tensors], E, seg_log)
    assert first == list(range(n * E + 1))
    src = _dev(pc.cat(tensors))
    for align_log in (0, 6):
        a = hip.tensor_compress_dbatch(src, S, E, 0, codec, align_log=align_log)
        b = hip.tensor_compress_seg_dbatch(src, S, E, seg_log, codec=codec, block_size_id=0, align_log=align_log)
        torch.cuda.synchronize()
        assert b[4] is None
        for x, y in zip(a[1:], b[1:4]):
            assert torch.equal(x, y)
        off, res = a[1].cpu().tolist(), a[2].cpu().tolist()
        assert min(res) >= 8
        for q in range(n * E):
            assert torch.equal(a[0][off[q]:off[q] + res[q]], b[0][off[q]:off[q] + res[q]]), (align_log, q)


def test_seg_compress_and_decompress_in_one_hip_graph(hip, checker):
    """one captured graph -- a single stream, a linear chain -- holding tensor_compress_seg_dbatch and then tensor_decompress_seg_dbatch; replayed
    twice, the source changed in between"""
    E, codec, ALIGN, seg_log = 2, 0, 4, 10
    shapes, _ = _corpus(E, seg_log)
    sizes = [len(t) for t in shapes]
    n, S = len(sizes), _offsets(sizes)
    total = int(S[-1])
    first = psc.seg_first(sizes, E, seg_log)
    nseg = first[-1]
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, nseg, blocks, ALIGN)
    wsize, rsize = hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize, hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    wsize.restype = rsize.restype = C.c_size_t
    wws = torch.empty(int(wsize(C.c_size_t(nseg), C.c_size_t(blocks), C.c_uint(0), C.c_int(codec))), dtype=torch.uint8, device="cuda")
    rws = torch.empty(int(rsize(C.c_size_t(nseg), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
    src = torch.zeros(total, dtype=torch.uint8, device="cuda")
    soff, sf = _i64(S), _i64(first)
    frames, back, planes, planes2 = _filled(fcap), _filled(total), _filled(total), _filled(total)
    foff, so, so2 = (torch.zeros(nseg + 1, dtype=torch.int64, device="cuda") for _ in range(3))
    fres, sres = (torch.zeros(nseg, dtype=torch.int64, device="cuda") for _ in range(2))
    poff = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda")
    poff2, psz = (torch.zeros(n * E, dtype=torch.int64, device="cuda") for _ in range(2))
    tres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))

    def work():
        hip.tensor_compress_seg_dbatch(src, soff, E, seg_log, sf, n_segments=nseg, codec=codec, block_size_id=0, dst=frames, dst_capacity=fcap, max_total_blocks=blocks,
                                       align_log=ALIGN, frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, seg_offsets=so,
                                       workspace=wws)
        hip.tensor_decompress_seg_dbatch(frames, foff, soff, E, seg_log, sf, n_segments=nseg, dst=back, dst_capacity=total, max_total_blocks=blocks, planes=planes2,
                                         planes_capacity=total, seg_offsets=so2, seg_results=sres, plane_offsets=poff2, plane_sizes=psz, workspace=rws, results=rres)

    def source(seed):
        return pc.random_tensors(sizes, seed) if seed % 2 else [np.asarray(t) for t in shapes]
    src.copy_(_dev(pc.cat(source(0)))); work(); torch.cuda.synchronize()
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
        want = [f[:r].copy() for seg in _segments_of(tensors, E, seg_log) for r, f in [checker.frame_compress(seg, 0, codec)]]
        check_frames(want, frames, foff, fres, ALIGN, fcap, trial)
        assert tres.cpu().tolist() == rres.cpu().tolist() == sizes
        out = back.cpu().numpy()
        assert (out[:total] == seen[-1]).all() and (out[total:] == FILL).all()
    assert not (seen[0] == seen[1]).all()


# ---------------------------------------------------------------------------------------------------------------- the user-facing pair
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_compress_tensors_segmented(hip, monkeypatch):
    from finitestateentropy_amd.api import AutoCodec
    gen = torch.Generator(device="cuda").manual_seed(23)
    old_bf = (torch.randn((96, 100), generator=gen, device="cuda") * 0.02).to(torch.bfloat16)
    new_bf = (old_bf.float() * (1 + 1e-2 * torch.randn((96, 100), generator=gen, device="cuda"))).to(torch.bfloat16)
    old_f = torch.randn((1500, 3), generator=gen, device="cuda") * 0.02
    new_f = old_f + torch.randn((1500, 3), generator=gen, device="cuda") * 2e-5
    old_i = torch.randint(-128, 128, (40, 50), generator=gen, device="cuda", dtype=torch.int8)
    new_i = old_i.clone(); new_i[1, ::7] += 1
    old_d = torch.randint(-2 ** 62, 2 ** 62, (300,), generator=gen, device="cuda", dtype=torch.int64)
    new_d = old_d.clone(); new_d[5] ^= 0xFF00
    empty = torch.zeros((0, 3), device="cuda", dtype=torch.float32)
    old, new = [old_bf, old_f, old_i, old_d, empty], [new_bf, new_f, new_i, new_d, empty.clone()]
    for kw in (dict(), dict(codec=1), dict(base=old), dict(codec=AutoCodec(20), base=old)):
        obj = hip.compress_tensors_segmented(new, 10, block_size_id=0, **kw)
        assert obj.segment_log == 10 and obj.delta is ("base" in kw) and sorted(g["elem_bytes"] for g in obj.groups) == [1, 2, 4, 8]
        for g in obj.groups:
            want = psc.seg_first(g["sizes"], g["elem_bytes"], 10)
            assert [int(x) for x in g["seg_first"]] == want and g["frame_results"].numel() == want[-1] and g["frame_offsets"].numel() == want[-1] + 1
            assert ("codecs" in g) == isinstance(kw.get("codec"), AutoCodec) and ("codecs" not in g or g["codecs"].numel() == want[-1])
        assert max(int(g["seg_first"][-1]) - len(g["sizes"]) * g["elem_bytes"] for g in obj.groups) > 0, "some plane has several segments"
        back = hip.decompress_tensors(obj, base=kw.get("base"))
        for a, b in zip(new, back):
            assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and _bits(a, b)
        # the same blocks, eight bytes per additional frame
        whole = hip.compress_tensors(new, block_size_id=0, **kw)
        extra = sum(int(g["seg_first"][-1]) - len(g["sizes"]) * g["elem_bytes"] for g in obj.groups)
        if not isinstance(kw.get("codec"), AutoCodec):
            assert obj.nbytes == whole.nbytes + 8 * extra
    # the AutoCodec object given back: its codecs, per segment, given again
    again = hip.compress_tensors_segmented(old, 10, codec=obj, block_size_id=0, base=old)
    assert again.codec == AutoCodec(20) and again.segment_log == 10
    for g, e in zip(again.groups, obj.groups):
        assert torch.equal(g["codecs"], e["codecs"])
    for a, b in zip(old, hip.decompress_tensors(again, base=old)):
        assert _bits(a, b)
    unsegmented = hip.compress_tensors(new, codec=AutoCodec(20), block_size_id=0)
    # without segments: today's object, field for field
    a, b = hip.compress_tensors(new, block_size_id=0, base=old), hip.compress_tensors(new, 0, 0, old)
    assert a.segment_log is None and set(vars(a)) == set(vars(b)) == {"groups", "dtypes", "shapes", "device", "codec", "block_size_id", "delta"}
    assert all(set(g) == {"elem_bytes", "index", "sizes", "frames", "frame_offsets", "frame_results", "tensor_results"} for g in a.groups)
    for ga, gb in zip(a.groups, b.groups):
        assert all(torch.equal(ga[k], gb[k]) if isinstance(ga[k], torch.Tensor) else ga[k] == gb[k] for k in ga)

    # every mismatch is raised before a launch: from here on a call into the library is a failure of the test
    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in ("FSEHIP_tensor_compress_dbatch", "FSEHIP_tensor_compress_delta_dbatch", "FSEHIP_tensor_compress_mixed_dbatch", "FSEHIP_tensor_compress_seg_dbatch",
                 "FSEHIP_tensor_decompress_seg_dbatch", "FSEHIP_planes_segments_dbatch", "FSEHIP_planes_fold_segments_dbatch"):
        monkeypatch.setattr(hip.lib, name, no_launch)
    with pytest.raises(ValueError):
        hip.compress_tensors(old, codec=obj, block_size_id=0, base=old)                       # written with segment_log 10, given back without
    with pytest.raises(ValueError):
        hip.compress_tensors_segmented(old, 11, codec=obj, block_size_id=0, base=old)
    with pytest.raises(ValueError):
        hip.compress_tensors_segmented(new, 10, codec=unsegmented, block_size_id=0)         # written without, given back with
    with pytest.raises(ValueError):
        hip.compress_tensors_segmented(new, 9, block_size_id=0)
    with pytest.raises(ValueError):
        hip.compress_tensors_segmented(new, 14, block_size_id=5)                            # a segment of less than a block
    with pytest.raises(ValueError):
        hip.compress_tensors_segmented(new, 31)
    with pytest.raises(ValueError):
        hip.compress_tensors_segmented(new, 20.0)

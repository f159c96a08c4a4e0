"""Patching segmented tensors on the device (FSEHIP_planes_split_window_dbatch, FSEHIP_planes_splice_dbatch, FSEHIP_tensor_patch_window_dbatch
and patch_tensor_windows) against the numpy model of planes_patch_corpus.py and the CPU oracle's frame of every segment.  Block-size id 0 with
segLog 10 and 11: a few KB already make several segments.  Every array is longer than its contract and pre-filled: whatever the contract
does not give to a call must still hold the fill afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_mixed_corpus as fmc
import frame_packed_corpus as fpc
import planes_corpus as pc
import planes_patch_corpus as ppc
import planes_seg_corpus as psc
import planes_window_corpus as pwc
from planes_corpus import CORRUPT, GENERIC, TOO_SMALL

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = 0xA5, 64, -7
SEG_LOGS = (10, 11)
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _i64(a):
    """python ints of 64 bits, signed or not, flattened: the bits are what counts"""
    flat = np.asarray(a, dtype=object).reshape(-1)
    return torch.from_numpy(np.array([int(x) % (1 << 64) for x in flat], dtype=np.uint64).view(np.int64)).cuda()


def _marked(n, head=None):
    """n entries and one more, all MARK, the first ones `head`"""
    t = torch.full((n + 1,), MARK, dtype=torch.int64, device="cuda")
    if head is not None and len(head):
        t[:len(head)] = _i64(head)
    return t


def _filled(n, content=None, shift=0):
    """n bytes (and a tail) of FILL that start `shift` bytes behind a 256-byte boundary, the first ones `content`"""
    t = torch.full((shift + n + TAIL,), FILL, dtype=torch.uint8, device="cuda")[shift:]
    if content is not None and len(content):
        t[:len(content)] = _dev(content)
    return t


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the window split
def run_split(hip, tensors, windows, E, seg_log, bases=None, shift=0, stage_off=None, stage_cap=None, capacity=None):
    n, sizes = len(tensors), [len(t) for t in tensors]
    S = _offsets(sizes)
    total = int(S[-1])
    want, written, P, res = ppc.stage_model(tensors, windows, E, seg_log, bases, stage_off, stage_cap, capacity)
    T = ppc.stage_offsets(sizes, [w if pwc.window_valid(m, w[0], w[1], E) else (0, 0) for m, w in zip(sizes, windows)], E, seg_log) if stage_off is None else stage_off
    cap = len(want)
    src = _filled(total, pc.cat(tensors), shift)
    base = None if bases is None else _filled(total, pc.cat(bases), (shift + 7) % 16)[:total]
    stage = _filled(cap, None, (5 * shift + 3) % 16)
    poff, sres = _marked(n * E + 1), _marked(n)
    win = _i64(windows)
    hip.planes_split_window_dbatch(src[:total], S, win, E, seg_log, stage_offsets=_i64(T), base=base, capacity=capacity, stage=stage, stage_capacity=cap,
                                   plane_offsets=poff, results=sres)
    torch.cuda.synchronize()
    assert int(poff[n * E + 1]) == MARK and int(sres[n]) == MARK
    assert poff.cpu().tolist()[:n * E + 1] == P and sres.cpu().tolist()[:n] == res
    got = stage.cpu().numpy()
    assert (got[:cap][written] == want[written]).all(), np.nonzero(written & (got[:cap] != want))[0][:8]
    assert (got[:cap][~written] == FILL).all() and (got[cap:] == FILL).all(), "nothing outside the staged planes is written"
    assert (src.cpu().numpy()[:total] == pc.cat(tensors)).all() and (base is None or (base.cpu().numpy() == pc.cat(bases)).all()), "the inputs are only read"
    return res


@pytest.mark.parametrize("form", ["plain", "xor"])
@pytest.mark.parametrize("E", ppc.ELEMS)
def test_split_window_against_the_model(hip, E, form):
    for seg_log in SEG_LOGS:
        s = 1 << seg_log
        rng = np.random.default_rng(E + seg_log)
        sizes = pwc.window_sizes(E, seg_log)
        assert {0, 1, s - 1, s, s + 1, 2 * s, 2 * s + 1} <= set(psc.plane_sizes(sizes, E))
        tensors = pc.random_tensors(sizes, 11 + E + seg_log)
        bases = pc.random_tensors(sizes, 12 + E + seg_log) if form == "xor" else None
        # every alignment of the source, the base and the stage; windows that start and end on, one short of and one behind a segment boundary
        for shift in range(16):
            windows = []
            for i, n in enumerate(sizes):
                cand = pwc.boundary_windows(n // E, seg_log)
                windows.append(cand[int(rng.integers(0, len(cand)))])
            res = run_split(hip, tensors, windows, E, seg_log, bases, shift)
            assert all((r > 0) == (a < b) for r, (a, b) in zip(res, windows))
        # a partial last element inside the last selected segment, and just behind it
        run_split(hip, tensors, [(max(n // E - 1, 0), n // E) for n in sizes], E, seg_log, bases, 1)
        assert sizes[10] == 2 * E * s + E - 1
        res = run_split(hip, tensors, [(0, n // E) if i != 10 else (s, 2 * s) for i, n in enumerate(sizes)], E, seg_log, bases, 2)
        assert res[10] == E * s and res[-1] == sizes[-1]


@pytest.mark.parametrize("E", ppc.ELEMS)
def test_split_window_long_planes_many_tensors_and_refusals(hip, E):
    seg_log = 10
    s = 1 << seg_log
    # a plane with more than 1024 selected segments, several tiles per staged tensor
    sizes = [E * 65 * s + 5, 7, E * 1030 * s + 1]
    tensors = pc.random_tensors(sizes, 50 + E)
    windows = [(s - 1, 65 * s), (0, 7 // E), (3 * s + 1, 1030 * s)]
    assert np.diff(pwc.window_first(sizes, windows, E, seg_log)[0])[-1] > 1024
    run_split(hip, tensors, windows, E, seg_log, None, 9)
    run_split(hip, tensors, windows, E, seg_log, pc.random_tensors(sizes, 51 + E), 6)
    # more than 1024 tensors with a window of one segment each, tensors with nothing selected among them
    many = [3 * E] * 1400 + [0] + [2 * E + 1] * 5
    windows = [(0, 0) if i % 5 == 2 else (i % 3, 3) for i in range(len(many) - 6)] + [(0, 0)] + [(0, 2), (1, 2), (2, 2), (0, 1), (1, 1)]
    run_split(hip, pc.random_tensors(many, 52 + E), windows, E, seg_log, None, 3)
    # refusals: a bad window, a pair of stage offsets that does not hold the sub-tensor, a stage and a source capacity that cut a tensor off
    sizes = pwc.window_sizes(E, seg_log)
    tensors = pc.random_tensors(sizes, 53 + E)
    good = [(0, n // E) for n in sizes]
    staged = run_split(hip, tensors, good, E, seg_log)
    assert min(staged) >= 0 and staged[7] == sizes[7] and staged[-1] == sizes[-1]
    for bad in ((0, sizes[7] // E + 1), (5, 4), (1 << 63, 1 << 63)):
        w = list(good)
        w[7] = bad
        res = run_split(hip, tensors, w, E, seg_log)
        assert res == staged[:7] + [GENERIC] + staged[8:]
    T = ppc.stage_offsets(sizes, good, E, seg_log)
    wrong = [t + (1 if i > 7 else 0) for i, t in enumerate(T)]                                     # tensor 7 has a byte too many, the others are moved
    res = run_split(hip, tensors, good, E, seg_log, None, 4, stage_off=wrong, stage_cap=wrong[-1])
    assert res == staged[:7] + [GENERIC] + staged[8:]
    res = run_split(hip, tensors, good, E, seg_log, None, 5, stage_cap=T[-1] - 1)
    assert res == staged[:-1] + [GENERIC]
    res = run_split(hip, tensors, good, E, seg_log, None, 0, capacity=sum(sizes) - 1)
    assert res == staged[:-1] + [GENERIC]


# ---------------------------------------------------------------------------------------------------------------- the splice alone
def _invented(lens, align_log, seed, gap=0):
    """frames of invented bytes of these lengths (negative: a frame that failed, no room) packed at an alignment -> (buffer, offsets)"""
    off = fpc.packed_offsets(lens, align_log)
    off = [x + gap for x in off]
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, off[-1] + 5, dtype=np.uint8)
    return buf, off


def run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR, fresh, C_=None, NC=None, out_cap=None, seg_first=None, sel_first=None, stage_res=None,
               frames_cap=None, new_cap=None, shift=0):
    n = len(sizes)
    first = psc.seg_first(sizes, E, seg_log) if seg_first is None else seg_first
    sel = pwc.window_first(sizes, windows, E, seg_log)[0] if sel_first is None else sel_first
    nseg, nsel = len(R), len(NR)
    frames_cap = len(frames) if frames_cap is None else frames_cap
    new_cap = len(fresh) if new_cap is None else new_cap
    m = ppc.splice_model(F, R, NF, NR, sizes, windows, E, seg_log, frames_cap, new_cap, 1 << 60, C_, NC, first, sel, nsel, stage_res)
    out_cap = m["off"][-1] + 9 if out_cap is None else out_cap
    m = ppc.splice_model(F, R, NF, NR, sizes, windows, E, seg_log, frames_cap, new_cap, out_cap, C_, NC, first, sel, nsel, stage_res)
    out = _filled(out_cap, None, shift)
    ooff, ores, tres = _marked(nseg + 1), _marked(nseg), _marked(n)
    ocod = None if C_ is None else _filled(nseg)
    d_frames, d_fresh = _filled(len(frames), frames, (shift + 3) % 16), _filled(len(fresh), fresh, (shift + 11) % 16)
    args = dict(n_segments=nseg, n_selected=nsel, codecs=None if C_ is None else _dev(C_), new_codecs=None if C_ is None or not nsel else _dev(NC),
                stage_results=None if stage_res is None else _i64(stage_res), frames_capacity=frames_cap, new_capacity=new_cap, out=out, out_capacity=out_cap,
                out_offsets=ooff, out_results=ores, out_codecs=ocod, tensor_results=tres)
    hip.planes_splice_dbatch(d_frames[:len(frames)], _i64(F), _i64(R), d_fresh[:max(len(fresh), 1)], _i64(NF), _i64(NR), _offsets(sizes), _i64(windows), _i64(first),
                             _i64(sel), E, seg_log, **args)
    torch.cuda.synchronize()
    assert int(ooff[nseg + 1]) == MARK and int(ores[nseg]) == MARK and int(tres[n]) == MARK
    assert tres.cpu().tolist()[:n] == m["tres"]
    assert ooff.cpu().tolist()[:nseg + 1] == m["off"] and ores.cpu().tolist()[:nseg] == m["res"]
    if C_ is not None:
        got = ocod.cpu().tolist()
        assert got[:nseg] == m["codecs"] and set(got[nseg:]) == {FILL}
    want = ppc.splice_bytes(m, frames, fresh, F, NF, out_cap + TAIL, FILL)
    got = out.cpu().numpy()
    assert (got == want).all(), np.nonzero(got != want)[0][:8]
    return m


def _splice_case(E, seg_log, align_log, seed, big=False):
    s = 1 << seg_log
    sizes = [E * 3 * s, E * 2 * s + 1, 0, E * (s + 1), E * 40 * s, E * s, 5 * E]
    first = psc.seg_first(sizes, E, seg_log)
    rng = np.random.default_rng(seed)
    R = [8 if q % 5 == 0 else int(rng.integers(8, 60)) for q in range(first[-1])]
    if big:
        R[3], R[first[4 * E] + 7] = 40000, 33000                      # frames across tile boundaries of the output
    frames, F = _invented(R, align_log, seed + 1)
    return sizes, first, R, frames, F


def _new_frames(sizes, windows, E, seg_log, align_log, seed, big=False):
    nsel = pwc.window_first(sizes, windows, E, seg_log)[0][-1]
    rng = np.random.default_rng(seed)
    NR = [8 if r % 4 == 1 else int(rng.integers(8, 90)) for r in range(nsel)]
    if big and nsel > 2:
        NR[1] = 70001
    fresh, NF = _invented(NR, align_log, seed + 1)
    return NR, fresh, NF


@pytest.mark.parametrize("align_log", [0, 6])
@pytest.mark.parametrize("E", ppc.ELEMS)
def test_splice_against_the_model(hip, E, align_log):
    seg_log = 10
    s = 1 << seg_log
    sizes, first, R, frames, F = _splice_case(E, seg_log, align_log, 100 + E, big=True)
    everything = [(0, n // E) for n in sizes]
    selections = {"nothing": [(0, 0)] * len(sizes), "everything": everything, "alternate": [w if i % 2 == 0 else (1, 1) for i, w in enumerate(everything)],
                  "parts": [(s - 1, s + 1), (2 * s, 2 * s), (0, 0), (s, s + 1), (7 * s, 31 * s + 1), (0, 0), (4, 5)]}
    for k, (name, windows) in enumerate(selections.items()):
        NR, fresh, NF = _new_frames(sizes, windows, E, seg_log, align_log, 200 + E + k, big=True)
        m = run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR, fresh, shift=k + 1)
        assert m["tres"] == sizes and ([x[0] for x in m["src"]].count("new") == len(NR))
        if name == "nothing":
            assert m["off"] == [x - F[0] for x in F] and m["res"] == R
        if name == "everything":
            assert [x[0] for x in m["src"]].count("old") == E + (E > 1), "the empty tensor's frames, and the segment of the partial last element"
        # with codecs, and a capacity one byte short: nothing is written, every tensor has dstSize_tooSmall, the offsets are whole
        C_ = [q % 2 for q in range(len(R))]
        NC = [(r // 2) % 2 for r in range(len(NR))]
        run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR, fresh, C_, NC, shift=k + 5)
        short = run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR, fresh, C_, NC, out_cap=m["off"][-1] - 1)
        assert short["tres"] == [TOO_SMALL] * len(sizes) and short["off"] == m["off"]
        run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR, fresh, out_cap=m["off"][-1])
    # frames of eight bytes only, and an object that does not start at 0
    R8 = [8] * len(R)
    frames8, F8 = _invented(R8, align_log, 7, gap=24)
    windows = selections["parts"]
    nsel = pwc.window_first(sizes, windows, E, seg_log)[0][-1]
    fresh8, NF8 = _invented([8] * nsel, align_log, 8)
    m = run_splice(hip, sizes, windows, E, seg_log, F8, R8, frames8, NF8, [8] * nsel, fresh8)
    assert m["off"][-1] == F8[-1] - 24


@pytest.mark.parametrize("E", ppc.ELEMS)
def test_splice_refuses_a_tensor_whole(hip, E):
    seg_log, align_log = 10, 0
    s = 1 << seg_log
    sizes, first, R, frames, F = _splice_case(E, seg_log, align_log, 300 + E)
    windows = [(s - 1, s + 1), (0, 2 * s), (0, 0), (s, s + 1), (7 * s, 31 * s + 1), (0, s), (4, 5)]
    sel = pwc.window_first(sizes, windows, E, seg_log)[0]
    NR, fresh, NF = _new_frames(sizes, windows, E, seg_log, align_log, 301 + E)
    good = run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR, fresh)
    victim = 4
    a, b = first[victim * E], first[(victim + 1) * E]

    def alone(m, code):
        assert m["tres"] == sizes[:victim] + [code] + sizes[victim + 1:]
        assert m["src"][:a] == good["src"][:a] and m["src"][b:] == good["src"][b:] and all(x is None or x[0] == "old" for x in m["src"][a:b])
    # old extents: not monotone, behind the capacity, a result that its extent does not hold -- in a selected and in an unselected frame
    for q, what in ((a + 2, "short"), (a + 9, "short"), (a + 20, "swap"), (b - 1, "error")):
        F2, R2 = list(F), list(R)
        if what == "short":
            R2[q] = F[q + 1] - F[q] + 1
        elif what == "swap":
            F2[q], F2[q + 1] = F2[q + 1] + 1, F2[q]
        else:
            R2[q] = -3
        alone(run_splice(hip, sizes, windows, E, seg_log, F2, R2, frames, NF, NR, fresh), CORRUPT)
    cut = F[b - 3] + 1                                                # the capacity ends inside the tensor's frames: the tensors behind it are refused too
    m = run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR, fresh, frames_cap=cut)
    assert m["tres"] == sizes[:victim] + [CORRUPT] * (len(sizes) - victim)
    F2 = list(F)
    F2[b - 1] = 1 << 62
    alone(run_splice(hip, sizes, windows, E, seg_log, F2, R, frames, NF, NR, fresh), CORRUPT)
    # the writer's errors: the first in plane and segment order; a new frame outside its buffer
    NR2 = list(NR)
    NR2[sel[victim * E] + 5], NR2[sel[victim * E] + 2] = -9, -6
    alone(run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR2, fresh), -6)
    NR2 = list(NR)
    NR2[sel[victim * E] + 1] = NF[sel[victim * E] + 2] - NF[sel[victim * E] + 1] + 1
    alone(run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR2, fresh), CORRUPT)
    # the split's error, a bad window, wrong counts in either array
    alone(run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR, fresh, stage_res=[0, 5, 0, 7, -1, 3, 3]), GENERIC)
    for bad in ((0, 40 * s + 1), (9, 8)):
        w = list(windows)
        w[victim] = bad
        alone(run_splice(hip, sizes, w, E, seg_log, F, R, frames, NF, NR, fresh, sel_first=sel), GENERIC)
    if E > 1:
        wrong = list(sel)
        wrong[victim * E + 1] -= 1
        alone(run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR, fresh, sel_first=wrong), GENERIC)
        wrong = list(first)
        wrong[victim * E + 1] += 1
        alone(run_splice(hip, sizes, windows, E, seg_log, F, R, frames, NF, NR, fresh, seg_first=wrong), GENERIC)


# ---------------------------------------------------------------------------------------------------------------- the composite
def _corpus(E, seg_log):
    """(old, new, other, bases, windows): compressible bf16 data over two segments and a bit, nothing, noise of exactly one segment per plane, a
    constant of a size that is no multiple of E, a skewed source of two segments and a half per plane, noise that nothing selects.  `new` differs
    from `old` inside the windows only, `other` everywhere; the bases differ from `old` in a byte in sixteen"""
    key = ("corpus", E, seg_log)
    if key not in _CACHE:
        s = 1 << seg_log
        rng = np.random.default_rng(60 + E + seg_log)
        old = [pc.bf16_gaussian(E * (2 * s + 100) // 2, 5 + E), np.zeros(0, np.uint8), rng.integers(0, 256, E * s, dtype=np.uint8),
               np.full(E * (s + 1) + E - 1, 77, np.uint8), rng.integers(0, 4, 5 * E * s // 2, dtype=np.uint8), rng.integers(0, 256, E * (s + 3), dtype=np.uint8)]
        windows = [(s - 1, s + 1), (0, 0), (5, 9), (3, s + 1), (2 * s, 2 * s + 7), (3, 3)]
        fresh = [pc.bf16_gaussian(E * (2 * s + 100) // 2, 6 + E)] + [t ^ rng.integers(1, 4, t.size, dtype=np.uint8) for t in old[1:]]
        new = [t.copy() for t in old]
        for t, f, (a, b) in zip(new, fresh, windows):
            t[a * E:b * E] = f[a * E:b * E]
        bases = [t ^ (rng.integers(1, 256, t.size, dtype=np.uint8) * (rng.integers(0, 16, t.size) == 0)).astype(np.uint8) for t in old]
        _CACHE[key] = (old, new, fresh, bases, windows)
    return _CACHE[key]


def _segments_of(tensors, E, seg_log):
    out = []
    for t in tensors:
        for pl in pc.planes_of(t, E):
            out += [np.ascontiguousarray(pl[a:a + (1 << seg_log)]) for a in (range(0, len(pl), 1 << seg_log) if len(pl) else [0])]
    return out


def _frames(oracle, E, seg_log, which, xor, codec):
    """the oracle's frame of every segment of every plane of old (0), new (1) or other (2) (xor: XOR base)"""
    key = ("frames", E, seg_log, which, xor, codec)
    if key not in _CACHE:
        c = _corpus(E, seg_log)
        data = [t ^ b for t, b in zip(c[which], c[3])] if xor else c[which]
        memo = _CACHE.setdefault(("memo", codec), {})
        out = []
        for seg in _segments_of(data, E, seg_log):
            k = seg.tobytes()
            if k not in memo:
                r, f = oracle.frame_compress(seg, 0, codec)
                memo[k] = f[:r].copy()
            out.append(memo[k])
        _CACHE[key] = out
    return _CACHE[key]


def compress(hip, tensors, bases, E, seg_log, align_log, codec=0, codecs=None):
    S = _offsets([len(t) for t in tensors])
    first = psc.seg_first([len(t) for t in tensors], E, seg_log)
    dst, foff, fres, tres, chosen = hip.tensor_compress_seg_dbatch(_dev(pc.cat(tensors)), S, E, seg_log, np.asarray(first, np.uint64),
                                                                    base=None if bases is None else _dev(pc.cat(bases)), codec=codec, codecs=codecs, block_size_id=0,
                                                                    align_log=align_log)
    torch.cuda.synchronize()
    total = int(foff[-1])
    return dst[:total].clone(), foff, fres, chosen


def run_patch(hip, obj, tensors, bases, windows, E, seg_log, align_log, codec=0, new_codecs=None, shift=0, **kw):
    frames, foff, fres, codecs = obj
    n, sizes = len(tensors), [len(t) for t in tensors]
    S = _offsets(sizes)
    total = int(S[-1])
    nseg = fres.numel()
    src = _filled(total, pc.cat(tensors), shift)[:total]
    base = None if bases is None else _filled(total, pc.cat(bases), (shift + 5) % 16)[:total]
    out_cap = frames.numel() + hip.frame_packed_bound(total, nseg, hip.planes_block_bound(total, n, E, 0), align_log)
    out = _filled(out_cap, None, (3 * shift + 1) % 16)
    ooff, ores, tres = _marked(nseg + 1), _marked(nseg), _marked(n)
    ocod = None if codecs is None else _filled(nseg)
    before = frames.clone()
    hip.tensor_patch_window_dbatch(frames, foff, fres, src, S, windows, E, seg_log, base=base, codec=codec, codecs=codecs, new_codecs=new_codecs, block_size_id=0,
                                   align_log=align_log, out=out, out_capacity=out_cap, out_offsets=ooff, out_results=ores, out_codecs=ocod, tensor_results=tres, **kw)
    torch.cuda.synchronize()
    assert int(ooff[nseg + 1]) == MARK and int(ores[nseg]) == MARK and int(tres[n]) == MARK and torch.equal(frames, before)
    assert ocod is None or set(ocod.cpu().tolist()[nseg:]) == {FILL}
    return out, ooff[:nseg + 1], ores[:nseg], tres.cpu().tolist()[:n], None if ocod is None else ocod.cpu().tolist()[:nseg], out_cap


def check_frames(want, dst, foff, fres, align_log, fcap, what):
    sizes = [len(w) for w in want]
    off, res, out = foff.cpu().tolist(), fres.cpu().tolist(), dst.cpu().numpy()
    assert off == fpc.packed_offsets(sizes, align_log, fcap), what
    assert res == sizes, what
    written = np.zeros(len(out), bool)
    for i, w in enumerate(want):
        assert (out[off[i]:off[i] + res[i]] == w).all(), (what, i)
        written[off[i]:off[i] + res[i]] = True
    assert (out[~written] == FILL).all(), (what, "bytes outside the frames", np.nonzero((out != FILL) & ~written)[0][:8])


@pytest.mark.parametrize("form", ["plain", "base", "given", "chosen"])
@pytest.mark.parametrize("E", ppc.ELEMS)
def test_the_patch_of_old_with_new_is_the_compress_of_new(hip, checker, E, form):
    from finitestateentropy_amd.api import AutoCodec
    for seg_log in SEG_LOGS:
        old, new, _, bases, windows = _corpus(E, seg_log)
        xor = form != "plain"
        sizes = [len(t) for t in old]
        sel = ppc.selected_frames(sizes, windows, E, seg_log)
        F, H = _frames(checker, E, seg_log, 1, xor, 0), _frames(checker, E, seg_log, 1, xor, 1)
        nseg = len(F)
        assert 0 < len(sel) < nseg and any(len(_frames(checker, E, seg_log, 0, xor, 0)[q]) != len(F[q]) for q in sel)
        for k, align_log in enumerate((0, 6)):
            what = (E, form, seg_log, align_log)
            if form in ("plain", "base"):
                for codec, want in ((0, F), (1, H)):
                    obj = compress(hip, old, bases if xor else None, E, seg_log, align_log, codec)
                    out, ooff, ores, tres, ocod, cap = run_patch(hip, obj, new, bases if xor else None, windows, E, seg_log, align_log, codec, shift=3 * k + codec + 1)
                    assert ocod is None and tres == sizes
                    check_frames(want, out, ooff, ores, align_log, cap, what)
                    # ... and is what the full call writes for `new`
                    full = compress(hip, new, bases if xor else None, E, seg_log, align_log, codec)
                    assert torch.equal(full[1], ooff) and torch.equal(full[2], ores) and torch.equal(full[0], out[:int(ooff[-1])])
            elif form == "given":
                given = [(q // 3) % 2 for q in range(nseg)]
                obj = compress(hip, old, bases, E, seg_log, align_log, codecs=_dev(given))
                out, ooff, ores, tres, ocod, cap = run_patch(hip, obj, new, bases, windows, E, seg_log, align_log, new_codecs=_dev([given[q] for q in sel]), shift=7)
                assert ocod == given and tres == sizes
                check_frames([H[q] if c else F[q] for q, c in enumerate(given)], out, ooff, ores, align_log, cap, what)
            else:
                tol = 20
                obj = compress(hip, old, bases, E, seg_log, align_log, AutoCodec(tol))
                out, ooff, ores, tres, ocod, cap = run_patch(hip, obj, new, bases, windows, E, seg_log, align_log, AutoCodec(tol), shift=12)
                want = [fmc.expected_choice(len(f), len(h), tol)[0] for f, h in zip(F, H)]
                assert ocod == want and tres == sizes, "the choice per segment is the mixed model's"
                check_frames([H[q] if c else F[q] for q, c in enumerate(want)], out, ooff, ores, align_log, cap, what)


@pytest.mark.parametrize("E", ppc.ELEMS)
def test_patch_refuses_a_tensor_whole_and_patches_the_others(hip, checker, E):
    seg_log, align_log, codec = 10, 0, 1
    old, new, _, _, windows = _corpus(E, seg_log)
    sizes = [len(t) for t in old]
    first, (sel, blocks) = psc.seg_first(sizes, E, seg_log), pwc.window_first(sizes, windows, E, seg_log)
    T = ppc.stage_offsets(sizes, windows, E, seg_log)
    O, N = _frames(checker, E, seg_log, 0, False, codec), _frames(checker, E, seg_log, 1, False, codec)
    obj = compress(hip, old, None, E, seg_log, align_log, codec)

    def kept(victims):
        return [O[q] if any(first[v * E] <= q < first[(v + 1) * E] for v in victims) else N[q] for q in range(len(O))]

    def patch(w=windows, **kw):
        kw.setdefault("sel_first", np.asarray(sel, np.uint64))
        kw.setdefault("stage_offsets", np.asarray(T, np.uint64))
        kw.setdefault("max_total_blocks", blocks)
        return run_patch(hip, obj, new, None, w, E, seg_log, align_log, codec, **kw)
    out, ooff, ores, tres, _, cap = patch()
    assert tres == sizes
    check_frames(N, out, ooff, ores, align_log, cap, "the exact block count")
    # a bad window: the counts in selFirst and the stage offsets are those of no window
    for bad in ((0, sizes[0] // E + 1), (7, 6)):
        w = list(windows)
        w[0] = bad
        out, ooff, ores, tres, _, cap = patch(w)
        assert tres == [GENERIC] + sizes[1:]
        check_frames(kept([0]), out, ooff, ores, align_log, cap, bad)
    # wrong counts in either array
    if E > 1:
        wrong = list(sel)
        wrong[4 * E + 1] -= 1
        out, ooff, ores, tres, _, cap = patch(sel_first=np.asarray(wrong, np.uint64))
        assert tres == sizes[:4] + [GENERIC] + sizes[5:]
        check_frames(kept([4]), out, ooff, ores, align_log, cap, "selFirst")
        wrong = list(first)
        wrong[1] += 1
        out, ooff, ores, tres, _, cap = patch(seg_first=np.asarray(wrong, np.uint64), n_segments=first[-1])
        assert tres == [GENERIC] + sizes[1:]
        check_frames(kept([0]), out, ooff, ores, align_log, cap, "segFirst")
    # a block promise one short: the last selected frame fails, its tensor keeps all its frames
    out, ooff, ores, tres, _, cap = patch(max_total_blocks=blocks - 1)
    assert tres == sizes[:4] + [GENERIC] + sizes[5:]
    check_frames(kept([4]), out, ooff, ores, align_log, cap, "a block short")


def _decompress(hip, frames, foff, sizes, bases, E, seg_log, first):
    D = _offsets(sizes)
    total = int(D[-1])
    base = None if bases is None else _dev(pc.cat(bases))
    back, res = hip.tensor_decompress_seg_dbatch(frames, foff, D, E, seg_log, np.asarray(first, np.uint64), base=base, dst=base,
                                                 max_total_blocks=hip.planes_block_bound(total, len(sizes), E, 0))
    torch.cuda.synchronize()
    assert res.cpu().tolist() == sizes
    return back.cpu().numpy()[:total]


@pytest.mark.parametrize("form", ["plain", "xor"])
@pytest.mark.parametrize("E", ppc.ELEMS)
def test_round_trip_new_inside_the_selected_segments_old_elsewhere(hip, E, form):
    seg_log = 10
    s = 1 << seg_log
    old, _, other, bases, windows = _corpus(E, seg_log)
    bases = bases if form == "xor" else None
    sizes = [len(t) for t in old]
    first = psc.seg_first(sizes, E, seg_log)
    obj = compress(hip, old, bases, E, seg_log, 0, 0)
    out, ooff, ores, tres, _, _ = run_patch(hip, obj, other, bases, windows, E, seg_log, 0, 0)
    assert tres == sizes
    want = []
    for o, x, (a, b) in zip(old, other, windows):
        at, m = ppc.sub_range(len(o), a, b, E, seg_log)
        w = o.copy()
        w[at:at + m] = x[at:at + m]
        assert m == 0 or (m >= (b - a) * E and not (o[at:at + m] == x[at:at + m]).all())
        want.append(w)
    back = _decompress(hip, out, ooff, sizes, bases, E, seg_log, first)
    assert (back == pc.cat(want)).all()
    # a window read of the patched object: the window itself and a window across the patch's edge
    for wins in (windows, [(max(a - 3, 0), min(b + 3, len(t) // E)) for t, (a, b) in zip(old, windows)]):
        doff = _offsets([E * (b - a) for a, b in wins])
        base = None if bases is None else _dev(pc.cat([x[a * E:b * E] for x, (a, b) in zip(bases, wins)]))
        dst, res = hip.tensor_decompress_window_dbatch(out, ooff, _offsets(sizes), wins, doff, E, seg_log, np.asarray(first, np.uint64), base=base, dst=base, block_size_id=0)
        torch.cuda.synchronize()
        assert res.cpu().tolist() == [E * (b - a) for a, b in wins]
        assert (dst.cpu().numpy()[:int(doff[-1])] == pc.cat([w[a * E:b * E] for w, (a, b) in zip(want, wins)])).all()


def test_the_patch_in_one_hip_graph_replayed_with_moved_windows(hip, checker):
    E, codec, ALIGN, seg_log = 2, 0, 6, 10
    s = 1 << seg_log
    rng = np.random.default_rng(5)
    sizes = [E * 6 * s, E * (4 * s + 9) + 1, E * 5 * s]
    old = [pc.bf16_gaussian(sizes[0] // 2, 3), rng.integers(0, 4, sizes[1], dtype=np.uint8), rng.integers(0, 256, sizes[2], dtype=np.uint8)]
    n, S = len(sizes), _offsets(sizes)
    total = int(S[-1])
    first = psc.seg_first(sizes, E, seg_log)
    nseg = first[-1]
    moves = [[(s - 1, s + 1), (0, 0), (2 * s + 5, 3 * s)], [(3 * s + 7, 4 * s + 1), (4, 4), (5, s)], [(4 * s, 6 * s), (9, 9), (4 * s + 1, 4 * s + 2)]]
    firsts = [pwc.window_first(sizes, w, E, seg_log) for w in moves]
    stages = [ppc.stage_offsets(sizes, w, E, seg_log) for w in moves]
    assert all(f[0] == firsts[0][0] for f in firsts) and all(t == stages[0] for t in stages), "the same selection sizes"
    sel, nsel, blocks = firsts[0][0], firsts[0][0][-1], max(f[1] for f in firsts)
    obj = compress(hip, old, None, E, seg_log, ALIGN, codec)
    frames, foff, fres, _ = obj
    wsize = hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize
    wsize.restype = C.c_size_t
    ws = torch.empty(int(wsize(C.c_size_t(nsel), C.c_size_t(blocks), C.c_uint(0), C.c_int(codec))), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(hip.planes_splice_scratch_bound(n, E, nseg), dtype=torch.uint8, device="cuda")
    new_cap = hip.frame_packed_bound(stages[0][-1], nsel, blocks, ALIGN)
    out_cap = frames.numel() + new_cap
    src = torch.zeros(total, dtype=torch.uint8, device="cuda")
    win = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    soff, sf, wf, toff = _i64(S), _i64(first), _i64(sel), _i64(stages[0])
    out, stage, fresh = _filled(out_cap), _filled(stages[0][-1]), _filled(new_cap)
    ooff, noff, sso = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda"), torch.zeros(nsel + 1, dtype=torch.int64, device="cuda"), torch.zeros(nsel + 1, dtype=torch.int64, device="cuda")
    ores, nres = torch.zeros(nseg, dtype=torch.int64, device="cuda"), torch.zeros(nsel, dtype=torch.int64, device="cuda")
    spo = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda")
    tres, sres = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")

    def work():
        hip.tensor_patch_window_dbatch(frames, foff, fres, src, soff, win, E, seg_log, sf, n_segments=nseg, sel_first=wf, n_selected=nsel, stage_offsets=toff, codec=codec,
                                       block_size_id=0, max_total_blocks=blocks, align_log=ALIGN, out=out, out_capacity=out_cap, out_offsets=ooff, out_results=ores,
                                       tensor_results=tres, stage=stage, stage_capacity=stages[0][-1], stage_plane_offsets=spo, stage_seg_offsets=sso, stage_results=sres,
                                       new_frames=fresh, new_capacity=new_cap, new_offsets=noff, new_results=nres, scratch=scratch, workspace=ws)

    def source(k):
        new = [t.copy() for t in old]
        for t, (a, b) in zip(new, moves[k]):
            t[a * E:b * E] ^= np.random.default_rng(70 + k).integers(1, 4, (b - a) * E, dtype=np.uint8)
        return new
    src.copy_(_dev(pc.cat(source(0)))); win.copy_(_i64(moves[0])); work(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    for k in (1, 2):
        new = source(k)
        src.copy_(_dev(pc.cat(new)))
        win.copy_(_i64(moves[k]))
        out.fill_(FILL)
        for t in (ooff, ores, tres):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = [f[:r].copy() for seg in _segments_of(new, E, seg_log) for r, f in [checker.frame_compress(seg, 0, codec)]]
        check_frames(want, out, ooff, ores, ALIGN, out_cap, k)
        assert tres.cpu().tolist() == sizes


# ---------------------------------------------------------------------------------------------------------------- the user-facing call
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_patch_tensor_windows(hip, monkeypatch):
    from finitestateentropy_amd import api
    from finitestateentropy_amd.api import AutoCodec
    gen = torch.Generator(device="cuda").manual_seed(29)
    old_bf = (torch.randn((96, 100), generator=gen, device="cuda") * 0.02).to(torch.bfloat16)
    old_f = torch.randn((1500, 3), generator=gen, device="cuda") * 0.02
    old_i = torch.randint(-128, 128, (40, 50), generator=gen, device="cuda", dtype=torch.int8)
    old_d = torch.randint(-2 ** 62, 2 ** 62, (300,), generator=gen, device="cuda", dtype=torch.int64)
    old_h = (torch.randn((3000,), generator=gen, device="cuda")).to(torch.float16)
    empty = torch.zeros((0, 3), device="cuda", dtype=torch.float32)
    old = [old_bf, old_f, old_i, old_d, old_h, empty]
    windows = [(100 * 10, 100 * 30), (4499, 4500), None, (0, 300), None, (0, 0)]
    new = [t.clone() for t in old]
    new[0].view(-1)[1000:3000] = (torch.randn((2000,), generator=gen, device="cuda") * 0.02).to(torch.bfloat16)
    new[1].view(-1)[4499] = 1.5
    new[3] ^= 0xFF00
    for kw in (dict(), dict(codec=1), dict(base=True), dict(codec=AutoCodec(20), base=True), dict(codec=AutoCodec(20))):
        base = old if kw.pop("base", False) else None
        bases = None if base is None else [b.clone() for b in base]
        obj = hip.compress_tensors_segmented(old, 10, block_size_id=0, base=base, **kw)
        snap = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in g.items()} for g in obj.groups]
        got = hip.patch_tensor_windows(obj, new, windows, base=base)
        want = hip.compress_tensors_segmented(new, 10, block_size_id=0, base=base, **kw)
        assert got is not obj and got.segment_log == 10 and got.delta is (base is not None) and got.codec == obj.codec and got.block_size_id == 0
        assert got.dtypes == want.dtypes and got.shapes == want.shapes and got.nbytes == want.nbytes
        for g, w, o, sn in zip(got.groups, want.groups, obj.groups, snap):
            assert set(g) == set(w) and g["index"] == w["index"] and g["sizes"] == w["sizes"] and [int(x) for x in g["seg_first"]] == [int(x) for x in w["seg_first"]]
            for k in ("frames", "frame_offsets", "frame_results", "tensor_results") + (("codecs",) if "codecs" in w else ()):
                assert torch.equal(g[k], w[k]), (kw, g["elem_bytes"], k)
                assert torch.equal(o[k], sn[k]) and g[k].data_ptr() != o[k].data_ptr(), "the object given is left as it is, the new one shares nothing with it"
        for a, b in zip(new, hip.decompress_tensors(got, base=bases)):
            assert a.dtype == b.dtype and a.shape == b.shape and _bits(a, b)
        back = hip.decompress_tensor_windows(got, [(990, 3010), (4490, 4500), (3, 9), None, (0, 3000), None], base=bases)
        assert _bits(back[0], new[0].view(-1)[990:3010]) and _bits(back[1], new[1].view(-1)[4490:4500]) and _bits(back[4], new[4])
    assert _bits(api.decompress_tensors(api.patch_tensor_windows(obj, new, windows))[0], new[0])
    deltas = hip.compress_tensors_segmented(old, 10, block_size_id=0, base=old)
    # nothing changed: a copy of the object
    same = hip.patch_tensor_windows(obj, old, [None] * len(old))
    assert all(torch.equal(g["frames"], o["frames"]) and g["frames"].data_ptr() != o["frames"].data_ptr() for g, o in zip(same.groups, obj.groups))

    # every mismatch is raised before a launch: from here on a call into the library is a failure of the test
    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in ("FSEHIP_tensor_patch_window_dbatch", "FSEHIP_planes_splice_dbatch", "FSEHIP_planes_split_window_dbatch", "FSEHIP_tensor_compress_seg_dbatch"):
        monkeypatch.setattr(hip.lib, name, no_launch)
    with pytest.raises(ValueError):
        hip.patch_tensor_windows(hip.compress_tensors(old[:1], block_size_id=0), new[:1], windows[:1])          # not segmented
    with pytest.raises(ValueError):
        hip.patch_tensor_windows(deltas, new, windows)                                                          # deltas without their base
    with pytest.raises(ValueError):
        hip.patch_tensor_windows(obj, new[:-1], windows)
    with pytest.raises(ValueError):
        hip.patch_tensor_windows(obj, new, windows[:-1])
    with pytest.raises(TypeError):
        hip.patch_tensor_windows(obj, [new[0].float()] + new[1:], windows)
    with pytest.raises(TypeError):
        hip.patch_tensor_windows(obj, [new[0].cpu()] + new[1:], windows)
    with pytest.raises(ValueError):
        hip.patch_tensor_windows(obj, [new[0].reshape(100, 96)] + new[1:], windows)
    for bad in ((5, 4), (0, 9601), (-1, 3), (0.0, 3), (1, 2, 3), 7):
        with pytest.raises(ValueError):
            hip.patch_tensor_windows(obj, new, [bad] + windows[1:])
    with pytest.raises(ValueError):
        hip.patch_tensor_windows(obj, new, windows, base=old)                                                   # a base for an object without deltas

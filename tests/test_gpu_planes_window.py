"""Windows of segmented tensors on the device (FSEHIP_planes_select_window_dbatch / _fold_window_dbatch, FSEHIP_tensor_decompress_window_dbatch and
decompress_tensor_windows) against the numpy model of planes_window_corpus.py and the tensors' own bytes.  Block-size id 0 with segLog 10 and
11: a few KB already make several segments.  Every array is longer than its contract and pre-filled: whatever the contract does not give to
a call must still hold the fill afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import planes_corpus as pc
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


def _filled(n, content=None):
    t = torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    if content is not None and len(content):
        t[:len(content)] = _dev(content)
    return t


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.uint64)


def _frame_layout(first):
    """offsets of frames of invented sizes, one per segment"""
    F = [0]
    for q in range(first[-1]):
        F.append(F[-1] + 8 + (q * 7) % 23)
    return F


# ---------------------------------------------------------------------------------------------------------------- the selection
def run_select(hip, sizes, windows, E, seg_log, seg_first=None, sel_first=None, nsel=None):
    n = len(sizes)
    first = psc.seg_first(sizes, E, seg_log) if seg_first is None else seg_first
    right = pwc.window_first(sizes, windows, E, seg_log)
    sel = right[0] if sel_first is None else sel_first
    nsel = sel[-1] if nsel is None else nsel
    nseg = psc.seg_first(sizes, E, seg_log)[-1]
    F = _frame_layout([nseg])
    out = _marked(nsel + 1)
    foff, sf, wf, win = _i64(F), _i64(first), _i64(sel), _i64(windows)
    got = hip.planes_select_window_dbatch(foff, _offsets(sizes), win, sf, wf, E, seg_log, n_segments=nseg, n_selected=nsel, sel_frame_offsets=out)
    torch.cuda.synchronize()
    assert got.numel() == nsel + 1 and int(out[nsel + 1]) == MARK, "one entry per selected frame and one more"
    assert foff.cpu().tolist() == F and sf.cpu().tolist() == list(first) and wf.cpu().tolist() == list(sel), "the inputs are only read"
    assert [x % (1 << 64) for x in win.cpu().tolist()] == [x for w in windows for x in w]
    want = pwc.select_model(F, sizes, windows, E, seg_log, first, sel, nsel)
    assert out.cpu().tolist()[:nsel + 1] == want
    return want, F


def _long_sizes(E, seg_log):
    s = 1 << seg_log
    return pwc.window_sizes(E, seg_log) + [E * 65 * s + 5, 7, E * 1030 * s + 1]


def _long_windows(sizes, E, seg_log, rng):
    """a boundary window for every tensor, nothing for every third; most of the two long ones"""
    s = 1 << seg_log
    out = []
    for i, n in enumerate(sizes):
        cand = pwc.boundary_windows(n // E, seg_log)
        out.append((n // E // 2, n // E // 2) if i % 3 == 1 else cand[int(rng.integers(0, len(cand)))])
    out[-3], out[-1] = (s - 1, 65 * s), (3 * s + 1, 1030 * s)
    return out


@pytest.mark.parametrize("seg_log", SEG_LOGS)
@pytest.mark.parametrize("E", pwc.ELEMS)
def test_select_against_the_model(hip, E, seg_log):
    rng = np.random.default_rng(E + seg_log)
    sizes = _long_sizes(E, seg_log)
    for rnd in range(4):
        windows = _long_windows(sizes, E, seg_log, rng)
        counts = np.diff(pwc.window_first(sizes, windows, E, seg_log)[0])
        assert 64 < counts[-3 * E] <= 1024 < counts[-E] and 0 in counts[:-3 * E]
        off, F = run_select(hip, sizes, windows, E, seg_log)
        assert off == sorted(off) and off[0] >= F[0] and off[-1] <= F[-1]
    # the binding's own destination (guarded in guard mode) and host arrays
    first, (sel, _) = psc.seg_first(sizes, E, seg_log), pwc.window_first(sizes, windows, E, seg_log)
    got = hip.planes_select_window_dbatch(_i64(F), _offsets(sizes), windows, first, sel, E, seg_log)
    assert got.cpu().tolist() == off
    # more than 1024 tensors of one segment per plane with a window each, tensors with nothing selected among them
    many = [3 * E] * 1400 + [0] + [2 * E + 1] * 5
    windows = [(0, 0) if i % 5 == 2 else (i % 3, 3) for i in range(len(many) - 6)] + [(0, 0)] + [(0, 2), (1, 2), (2, 2), (0, 1), (1, 1)]
    assert pwc.window_first(many, windows, E, seg_log)[0][-1] == E * sum(1 for a, b in windows if a < b) > E * 1024
    run_select(hip, many, windows, E, seg_log)
    run_select(hip, many, [(1, 1)] * len(many[:-6]) + [(0, 0)] * 6, E, seg_log)                # nothing selected: one entry, F[0]


@pytest.mark.parametrize("E", pwc.ELEMS)
def test_select_refuses_only_the_tensor_whose_window_or_counts_are_wrong(hip, E):
    seg_log = 10
    s = 1 << seg_log
    sizes = _long_sizes(E, seg_log)
    windows = [(0, n // E) for n in sizes]
    victim = 7                                               # planes of 2 seg bytes: two segments each
    first, (sel, _) = psc.seg_first(sizes, E, seg_log), pwc.window_first(sizes, windows, E, seg_log)
    good, F = run_select(hip, sizes, windows, E, seg_log)
    a, b = sel[victim * E], sel[(victim + 1) * E]
    assert b - a == 2 * E

    def refused_alone(got):
        assert got[:a] == good[:a] and got[b:] == good[b:] and got[a:b] == [F[first[(victim + 1) * E]]] * (b - a)
    # a count too small in selFirst for its first plane, the next plane (E == 1: the next tensor) one too many
    wrong = list(sel)
    wrong[victim * E + 1] -= 1
    got, _ = run_select(hip, sizes, windows, E, seg_log, sel_first=wrong)
    if E > 1:
        refused_alone(got)
    else:
        assert got[:a] == good[:a] and got[sel[victim + 2]:] == good[sel[victim + 2]:] and set(got[a:a + 1]) == {F[first[victim + 1]]}
    # a count that is not its own in segFirst
    wrong = list(first)
    wrong[victim * E + 1] += 1
    got, _ = run_select(hip, sizes, windows, E, seg_log, seg_first=wrong)
    if E > 1:
        refused_alone(got)
    # a window that ends behind the last whole element, a window that ends in front of its start: the counts in selFirst are those of no window
    for bad in ((0, 2 * s + 1), (5, 4), (1 << 63, 1 << 63), ((1 << 63) - 1, 2)):
        w = list(windows)
        w[victim] = bad
        refused_alone(run_select(hip, sizes, w, E, seg_log, sel_first=sel)[0])
    # a selection that ends behind nSelected: the last tensors are refused, nothing behind the arrays is touched
    got, _ = run_select(hip, sizes, windows, E, seg_log, nsel=sel[-1] - 1)
    assert got[:sel[-E - 1]] == good[:sel[-E - 1]] and set(got[sel[-E - 1]:]) == {F[first[-1]]}
    # arrays of nonsense: every index is clamped (the outputs are unspecified, the arrays around them are not)
    rng = np.random.default_rng(9)
    n, nsel, nseg = len(sizes), sel[-1], first[-1]
    nonsense = [int(x) for x in rng.integers(0, 1 << 62, len(sel))]
    out = _marked(nsel + 1)
    hip.planes_select_window_dbatch(_i64(F), _offsets(sizes), _i64([int(x) for x in rng.integers(0, 1 << 62, 2 * n)]), _i64(sorted(nonsense)), _i64(sorted(nonsense[::-1])),
                                    E, seg_log, n_segments=nseg, n_selected=nsel, sel_frame_offsets=out)
    hip.planes_select_window_dbatch(_i64(F), _offsets(sizes), _i64(windows), _i64(nonsense), _i64(sel), E, seg_log, n_segments=nseg, n_selected=nsel, sel_frame_offsets=out)
    hip.planes_select_window_dbatch(_i64(F), _offsets(sizes), _i64(windows), _i64(first), _i64(nonsense), E, seg_log, n_segments=nseg, n_selected=nsel, sel_frame_offsets=out)
    torch.cuda.synchronize()
    assert int(out[nsel + 1]) == MARK and set(out.cpu().tolist()[:nsel + 1]) <= set(F)


# ---------------------------------------------------------------------------------------------------------------- the fold
def good_decode(sizes, windows, E, seg_log, at=0):
    """(offsets, results) as the packed reader leaves them for the selected segments decoded back to back from `at`"""
    seg = 1 << seg_log
    off, res = [at], []
    for n, (a, b) in zip(sizes, windows):
        for p in range(E):
            size = pc.plane_size(int(n), p, E)
            for k in pwc.selected(size, a, b, seg_log):
                res.append(min(seg, size - k * seg))
                off.append(off[-1] + res[-1])
    return off, res


def run_fold(hip, off, res, sizes, windows, E, seg_log, seg_first=None, sel_first=None, nsel=None):
    n = len(sizes)
    npl = n * E
    first = psc.seg_first(sizes, E, seg_log) if seg_first is None else seg_first
    sel = pwc.window_first(sizes, windows, E, seg_log)[0] if sel_first is None else sel_first
    nsel = sel[-1] if nsel is None else nsel
    assert len(off) >= nsel + 1 and len(res) >= nsel
    po, ps = _marked(npl), _marked(npl)
    doff, dres, sf, wf, win = _i64(off), _i64(res), _i64(first), _i64(sel), _i64(windows)
    hip.planes_fold_window_dbatch(doff, dres, _offsets(sizes), win, sf, wf, E, seg_log, n_selected=nsel, plane_offsets=po, plane_sizes=ps)
    torch.cuda.synchronize()
    assert int(po[npl]) == MARK and int(ps[npl]) == MARK
    assert doff.cpu().tolist() == off and dres.cpu().tolist() == res and sf.cpu().tolist() == list(first) and wf.cpu().tolist() == list(sel), "the inputs are only read"
    want = pwc.fold_model(off, res, sizes, windows, E, seg_log, first, sel, nsel)
    assert ps.cpu().tolist()[:npl] == want[1]
    assert po.cpu().tolist()[:npl] == want[0]
    return want


@pytest.mark.parametrize("seg_log", SEG_LOGS)
@pytest.mark.parametrize("E", pwc.ELEMS)
def test_fold_against_the_model(hip, E, seg_log):
    s = 1 << seg_log
    rng = np.random.default_rng(30 + E + seg_log)
    sizes = _long_sizes(E, seg_log)
    for rnd in range(3):
        windows = _long_windows(sizes, E, seg_log, rng)
        off, good = good_decode(sizes, windows, E, seg_log, 16 * rnd)
        po, ps = run_fold(hip, off, good, sizes, windows, E, seg_log)
        assert ps == [b - a for a, b in windows for _ in range(E)]
    sel = pwc.window_first(sizes, windows, E, seg_log)[0]
    # the binding's own destinations (guarded in guard mode)
    gpo, gps = hip.planes_fold_window_dbatch(_i64(off), _i64(good), _offsets(sizes), windows, psc.seg_first(sizes, E, seg_log), sel, E, seg_log)
    assert gpo.cpu().tolist() == po and gps.cpu().tolist() == ps
    # errors and damage, each in a plane of its own
    long65, long1030 = sel[-3 * E - 1], sel[-E - 1]          # the first planes of the two long tensors: segments 0 .. 64 and 3 .. 1029
    res = list(good)
    res[long65 + 64], res[long65 + 3] = -2, -3               # two errors, the later one in an earlier lane's second round
    res[long1030 + 1026], res[long1030 + 64], res[long1030 + 1000] = -4, -5, -1
    bad_off = list(off)
    if E > 1:
        res[sel[-3 * E] + 7] = s - 1                         # a short middle segment of the second plane of the first long tensor
        bad_off[sel[-E] + 70] += 1                           # a gap inside the second plane of the second one
    _, got = run_fold(hip, bad_off, res, sizes, windows, E, seg_log)
    assert got[-3 * E] == -3 and got[-E] == -5 and (E == 1 or (got[-3 * E + 1] == CORRUPT and got[-E + 1] == CORRUPT))
    assert sum(1 for x, y in zip(got, ps) if x != y) == (4 if E > 1 else 2)
    # a last selected segment of 1 .. seg bytes that is not what the plane holds there: the full read's fold would take it
    windows = [(0, n // E) for n in sizes]
    off, good = good_decode(sizes, windows, E, seg_log)
    sel = pwc.window_first(sizes, windows, E, seg_log)[0]
    victim = 12                                              # planes of 3 seg + 5 bytes and a byte more for the first E / 2
    res = list(good)
    assert res[sel[victim * E + 1] - 1] == 5 + (E > 1)
    res[sel[victim * E + 1] - 1] -= 1
    _, got = run_fold(hip, off, res, sizes, windows, E, seg_log)
    assert got[victim * E] == CORRUPT and got[victim * E + 1:(victim + 1) * E] == [3 * s + 5] * (E - 1)


def test_fold_one_case_per_branch_refusals_and_many_small_planes(hip):
    E = 1
    for seg_log in SEG_LOGS:
        sizes, windows, off, res, sel, want, refuse = [], [], [], [], [0], [], []
        for _, size, a, b, refused, o, r, w in pwc.fold_cases(seg_log):
            sizes.append(size)
            windows.append((a, b))
            cnt = len(pwc.selected(size, a, b, seg_log))
            off += o[:-1] if r else [77] * cnt
            res += r if r else [1 << seg_log] * cnt
            sel.append(sel[-1] + cnt + (1 if refused else 0))   # refused: a count that is not the window's
            off += [0] * refused
            res += [0] * refused
            want.append(w)
        off.append(12345)
        po, ps = run_fold(hip, off, res, sizes, windows, E, seg_log, sel_first=sel)
        assert list(zip(po, ps)) == want
    # a tensor refused for its window, for segFirst, and for a selection behind nSelected
    seg_log, E = 10, 2
    sizes = [E * 3000, E * 500, E * 1024]
    windows = [(1000, 2100), (0, 500), (3, 9)]
    off, res = good_decode(sizes, windows, E, seg_log)
    sel = pwc.window_first(sizes, windows, E, seg_log)[0]
    assert run_fold(hip, off, res, sizes, windows, E, seg_log)[1] == [1100, 1100, 500, 500, 6, 6]
    assert run_fold(hip, off, res, sizes, [(1000, 3001), (0, 500), (3, 9)], E, seg_log, sel_first=sel)[1] == [GENERIC, GENERIC, 500, 500, 6, 6]
    assert run_fold(hip, off, res, sizes, [(1000, 2100), (2, 1), (3, 9)], E, seg_log, sel_first=sel)[1] == [1100, 1100, GENERIC, GENERIC, 6, 6]
    first = psc.seg_first(sizes, E, seg_log)
    assert run_fold(hip, off, res, sizes, windows, E, seg_log, seg_first=first[:-1] + [first[-1] + 1])[1] == [1100, 1100, 500, 500, GENERIC, GENERIC]
    assert run_fold(hip, off, res, sizes, windows, E, seg_log, nsel=sel[-1] - 1)[1] == [1100, 1100, 500, 500, GENERIC, GENERIC]
    # more than 1024 planes of one selected segment
    n = 1100
    sizes = [int(x) for x in np.random.default_rng(3).integers(1, 1025, n)]
    windows = [(x % 3 if x > 3 else 0, x) for x in sizes]
    off, res = good_decode(sizes, windows, 1, 10)
    res[500], res[1099] = -3, sizes[1099] - 1
    _, ps = run_fold(hip, off, res, sizes, windows, 1, 10)
    assert ps[500] == -3 and ps[1099] == CORRUPT and ps[:500] == [b - a for a, b in windows[:500]]
    # arrays of nonsense: clamped, nothing outside the arrays is read or written (run_fold checks the marks)
    nonsense = [int(x) for x in np.random.default_rng(4).integers(0, 1 << 62, n + 1)]
    run_fold(hip, off, res, sizes, windows, 1, 10, sel_first=sorted(nonsense), nsel=n)
    run_fold(hip, off, res, sizes, windows, 1, 10, seg_first=sorted(nonsense))
    run_fold(hip, off, res, sizes, [(x, y) for x, y in zip(nonsense, nonsense[1:])], 1, 10, sel_first=list(range(n + 1)))


# ---------------------------------------------------------------------------------------------------------------- the composite
def _corpus(E, seg_log):
    """(tensors, bases): compressible bf16 data over two segments and a bit, nothing, noise of exactly one segment per plane, three symbols in turn, of a size
    that is no multiple of E, a skewed source of two segments and a half per plane, fewer bytes than an element; the bases differ from them in a
    byte in sixteen"""
    key = ("corpus", E, seg_log)
    if key not in _CACHE:
        s = 1 << seg_log
        rng = np.random.default_rng(60 + E + seg_log)
        tensors = [pc.bf16_gaussian(E * (2 * s + 100) // 2, 5 + E), np.zeros(0, np.uint8), rng.integers(0, 256, E * s, dtype=np.uint8),
                   (77 + np.arange(E * (s + 1) + E - 1) % 3).astype(np.uint8), rng.integers(0, 4, 5 * E * s // 2, dtype=np.uint8),
                   rng.integers(0, 256, E - 1, dtype=np.uint8)]
        bases = [t ^ (rng.integers(1, 256, t.size, dtype=np.uint8) * (rng.integers(0, 16, t.size) == 0)).astype(np.uint8) for t in tensors]
        _CACHE[key] = (tensors, bases)
    return _CACHE[key]


def _compressed(hip, E, seg_log, form):
    """the corpus as segment frames written by the device: form "fse" / "huf", "mixed" (a codec per segment, alternating in threes), "xor-fse" /
    "xor-huf" (tensor XOR base) -> (frames, frame offsets, segFirst); the full read gives the tensors back"""
    key = ("frames", E, seg_log, form)
    if key not in _CACHE:
        tensors, bases = _corpus(E, seg_log)
        sizes = [len(t) for t in tensors]
        S = _offsets(sizes)
        first = psc.seg_first(sizes, E, seg_log)
        src = _dev(pc.cat(tensors))
        base = _dev(pc.cat(bases)) if form.startswith("xor") else None
        codecs = _dev([(q // 3) % 2 for q in range(first[-1])]) if form == "mixed" else None
        dst, foff, fres, tres, _ = hip.tensor_compress_seg_dbatch(src, S, E, seg_log, np.asarray(first, np.uint64), base=base, codec=int(form.endswith("huf")),
                                                                  codecs=codecs, block_size_id=0)
        assert tres.cpu().tolist() == sizes and int(fres.min()) >= 8
        back, res = hip.tensor_decompress_seg_dbatch(dst, foff, S, E, seg_log, np.asarray(first, np.uint64), base=base)
        assert res.cpu().tolist() == sizes and torch.equal(back[:src.numel()], src)
        _CACHE[key] = (dst.clone(), foff.clone(), first)
    return _CACHE[key]


def _slots(windows, E, pads=None, lead=0):
    """destination offsets: the first slot `lead` bytes into the buffer, slot i holds its window and pads[i] bytes more, so that the slots start off
    every alignment"""
    pads = [(3 * i + 1) % 17 for i in range(len(windows))] if pads is None else pads
    return _offsets([E * (b - a) + p for (a, b), p in zip(windows, pads)]) + np.uint64(lead)


def run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D=None, bases=None, in_place=False, blocks=None, cap=None, seg_first_log=None, n_segments=None):
    """the composite with every array marked: -> (destination bytes, results); the slot of tensor i is D[i] .. D[i+1]"""
    sizes = [len(t) for t in tensors]
    n = len(sizes)
    D = _slots(windows, E) if D is None else D
    total = int(D[-1])
    image = np.full(total, FILL, np.uint8)
    if bases is not None:                                    # the base has the layout of the destination: the same windows of the bases in the slots
        for i, (a, b) in enumerate(windows):
            image[int(D[i]):int(D[i]) + E * (b - a)] = bases[i][a * E:b * E]
    base = None if bases is None else _filled(total, image)
    back = base if in_place else _filled(total)
    sel, exact = pwc.window_first(sizes, windows, E, seg_log if seg_first_log is None else seg_first_log)
    nsel = sel[-1]
    res, sfo, so, sres = _marked(n), _marked(nsel + 1), _marked(nsel + 1), _marked(nsel)
    poff, psz = _marked(n * E), _marked(n * E)
    planes = _filled(max(nsel, 1) << seg_log)
    hip.tensor_decompress_window_dbatch(frames, foff, _offsets(sizes), windows, D, E, seg_log, np.asarray(first, np.uint64), n_segments=n_segments,
                                        sel_first=np.asarray(sel, np.uint64), base=base, dst=back, dst_capacity=total if cap is None else cap,
                                        max_total_blocks=exact if blocks is None else blocks, planes=planes, planes_capacity=nsel << seg_log, sel_frame_offsets=sfo,
                                        sel_offsets=so, sel_results=sres, plane_offsets=poff, plane_sizes=psz, results=res)
    torch.cuda.synchronize()
    assert int(res[n]) == MARK and int(sfo[nsel + 1]) == MARK and int(so[nsel + 1]) == MARK and int(sres[nsel]) == MARK and int(poff[n * E]) == MARK
    assert int(psz[n * E]) == MARK and bool((planes[nsel << seg_log:] == FILL).all()) and bool((back[total:] == FILL).all())
    if base is not None and not in_place:
        assert (base.cpu().numpy()[:total] == image).all(), "a base that is not the destination is only read"
    return back.cpu().numpy()[:total], res.cpu().tolist()[:n], image


def check_window(out, res, tensors, windows, E, D, untouched=None, failed=()):
    want = np.full(len(out), FILL, np.uint8) if untouched is None else untouched.copy()
    for i, (t, (a, b)) in enumerate(zip(tensors, windows)):
        if i not in failed:
            assert res[i] == E * (b - a), (i, res[i])
            want[int(D[i]):int(D[i]) + E * (b - a)] = t[a * E:b * E]
    bad = np.nonzero(out != want)[0]
    assert bad.size == 0, ("bytes that differ", bad[:8], [i for i in range(len(tensors)) if D[i] <= bad[0] < D[i + 1]])


@pytest.mark.parametrize("form", ["fse", "huf", "mixed"])
@pytest.mark.parametrize("E", pwc.ELEMS)
def test_window_is_the_slice_of_the_tensor_for_every_boundary_window(hip, E, form):
    for seg_log in SEG_LOGS:
        tensors, _ = _corpus(E, seg_log)
        frames, foff, first = _compressed(hip, E, seg_log, form)
        cands = [pwc.boundary_windows(len(t) // E, seg_log) for t in tensors]
        assert E == 1 or (any(len(t) > E and len(t) % E for t in tensors) and any(0 < len(t) < E for t in tensors))
        seen = set()
        for rnd in range(max(len(c) for c in cands)):
            windows = [c[(rnd + 3 * i) % len(c)] for i, c in enumerate(cands)]
            D = _slots(windows, E, [(rnd + 5 * i) % 16 for i in range(len(tensors))], rnd % 16)
            out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D)
            check_window(out, res, tensors, windows, E, D)
            seen |= {int(D[i]) % 16 for i, (a, b) in enumerate(windows) if b - a > 16}
        assert seen == set(range(16)), "destination slots off every alignment"
        # every window of every tensor at once is the full read
        windows = [(0, len(t) // E) for t in tensors]
        out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log)
        check_window(out, res, tensors, windows, E, _slots(windows, E))


@pytest.mark.parametrize("E", pwc.ELEMS)
def test_small_slots_capacity_block_promise_and_nothing_selected(hip, E):
    seg_log = 10
    s = 1 << seg_log
    tensors, _ = _corpus(E, seg_log)
    frames, foff, first = _compressed(hip, E, seg_log, "fse")
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s, s + 1), (s + 7, 2 * s + 9), (0, 0)]
    # a slot one byte short: dstSize_tooSmall and the slot is untouched; a slot of exactly the window's bytes
    D = _slots(windows, E, [3, 0, -1, 0, 0, 2])
    out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D)
    assert res[2] == TOO_SMALL
    check_window(out, res, tensors, windows, E, D, failed=(2,))
    # dstCapacity in front of the last slots' end: GENERIC for them, nothing at or behind it is written
    D = _slots(windows, E)
    for cap, failed in ((int(D[5]) - 1, (4, 5)), (int(D[4]) - 1, (3, 4, 5)), (int(D[5]), (5,))):
        out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D, cap=cap)
        assert [res[i] for i in failed] == [GENERIC] * len(failed)
        check_window(out, res, tensors, windows, E, D, failed=failed)
    # a block promise one short: the last selected frame is beyond it and gets GENERIC -- its tensor does, the others are whole
    _, exact = pwc.window_first([len(t) for t in tensors], windows, E, seg_log)
    out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D, blocks=exact - 1)
    assert res[4] == GENERIC
    check_window(out, res, tensors, windows, E, D, failed=(4,))
    # nothing selected
    windows = [(7, 7), (0, 0), (s, s), (0, 0), (1, 1), (0, 0)]
    D = _slots(windows, E)
    out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D)
    assert res == [0] * len(tensors) and (out == FILL).all()
    # a window that is none: its tensor alone is refused
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, 4), (s, s + 1), (s + 7, 2 * s + 9), (0, 0)]
    sel = pwc.window_first([len(t) for t in tensors], [w if i != 2 else (5, 5) for i, w in enumerate(windows)], E, seg_log)
    D = _slots([w if i != 2 else (0, 4) for i, w in enumerate(windows)], E)
    n = len(tensors)
    back, r = _filled(int(D[-1])), _marked(n)
    hip.tensor_decompress_window_dbatch(frames, foff, _offsets([len(t) for t in tensors]), windows, D, E, seg_log, np.asarray(first, np.uint64),
                                        sel_first=np.asarray(sel[0], np.uint64), max_total_blocks=sel[1], dst=back, dst_capacity=int(D[-1]), results=r)
    torch.cuda.synchronize()
    res = r.cpu().tolist()[:n]
    assert res[2] == GENERIC
    check_window(back.cpu().numpy()[:int(D[-1])], res, tensors, windows, E, D, failed=(2,))


@pytest.mark.parametrize("form", ["fse", "xor-huf", "in_place"])
@pytest.mark.parametrize("E", pwc.ELEMS)
def test_damage_in_a_selected_segment_in_an_unselected_one_and_another_segment_size(hip, checker, E, form):
    seg_log = 10
    s = 1 << seg_log
    tensors, bases = _corpus(E, seg_log)
    xor, in_place = form != "fse", form == "in_place"
    frames, foff, first = _compressed(hip, E, seg_log, "xor-fse" if in_place else form)
    frames = frames.clone()
    kw = dict(bases=bases if xor else None, in_place=in_place)
    victim = 4                                               # noise of four symbols, three segments per plane: compressed blocks
    assert first[victim * E + 1] - first[victim * E] == 3
    inside, across = [(3, 40), (0, 0), (0, s), (1, 2), (5, s - 3), (0, 0)], [(3, 40), (0, 0), (0, s), (1, 2), (5, s + 3), (0, 0)]
    D1, D2 = _slots(inside, E), _slots(across, E)
    f = first[victim * E] + 1                                # the middle segment of its plane 0: behind the selected frame of `inside`, selected by `across`
    at = 5 + 3 + 40
    lo, size = int(foff[f]), int(foff[f + 1] - foff[f])
    assert size > at + 8
    frames[lo + at] ^= 0x55
    r, _ = checker.frame_decompress(frames[lo:lo + size].cpu().numpy(), s)
    assert r > (1 << 63), "the oracle's reader refuses the damaged frame"
    # unselected, in the gap behind a selected frame: nothing changes
    out, res, image = run_window(hip, frames, foff, first, tensors, inside, E, seg_log, D1, **kw)
    check_window(out, res, tensors, inside, E, D1, untouched=image if in_place else None)
    # selected: that tensor alone fails, with what the oracle's reader says of that frame, and its slot -- in place: its old bytes -- is untouched
    out, res, image = run_window(hip, frames, foff, first, tensors, across, E, seg_log, D2, **kw)
    assert res[victim] == r - (1 << 64)
    check_window(out, res, tensors, across, E, D2, untouched=image if in_place else None, failed=(victim,))
    frames[lo + at] ^= 0x55
    out, res, image = run_window(hip, frames, foff, first, tensors, across, E, seg_log, D2, **kw)
    check_window(out, res, tensors, across, E, D2, untouched=image if in_place else None)
    # written with segLog 10, read with 11 and the sender's segFirst: every tensor with a plane of several segments is refused, the others are read
    windows = [(3, 40), (0, 0), (0, s), (1, 2), (5, s - 3), (0, 0)]
    several = [any(first[j + 1] - first[j] > 1 for j in range(i * E, (i + 1) * E)) for i in range(len(tensors))]
    assert several == [True, False, False, True, True, False]
    D = _slots(windows, E)
    out, res, image = run_window(hip, frames, foff, first, tensors, windows, E, 11, D, seg_first_log=11, **kw)
    failed = tuple(i for i, m in enumerate(several) if m)
    assert [res[i] for i in failed] == [GENERIC] * 3
    check_window(out, res, tensors, windows, E, D, untouched=image if in_place else None, failed=failed)
    # ... and with the reader's own segFirst for 11 over the same frames: the first tensor's frames are not the segments the reader takes them for
    sizes = [len(t) for t in tensors]
    own = psc.seg_first(sizes, E, 11)
    assert own[-1] < first[-1]
    windows = [(3, 2 * s + 40), (0, 0), (0, s), (1, 2), (5, s - 3), (0, 0)]
    D = _slots(windows, E)
    out, res, image = run_window(hip, frames, foff[:own[-1] + 1].clone(), own, tensors, windows, E, 11, D, seg_first_log=11, **kw)
    assert res[0] == CORRUPT and all(x < 0 or x == E * (b - a) for x, (a, b) in zip(res, windows))
    want = image if in_place else np.full(len(out), FILL, np.uint8)
    for i, x in enumerate(res):                              # nothing is written outside the slots of the tensors that report a size
        lo, hi = (int(D[i]), int(D[i]) + max(x, 0))
        want[lo:hi] = out[lo:hi]
    assert (out == want).all()


@pytest.mark.parametrize("codec", ["fse", "huf"])
@pytest.mark.parametrize("E", pwc.ELEMS)
def test_xor_windows_plain_and_patching_resident_tensors_in_place(hip, E, codec):
    seg_log = 11
    s = 1 << seg_log
    tensors, bases = _corpus(E, seg_log)
    frames, foff, first = _compressed(hip, E, seg_log, "xor-" + codec)
    sizes = [len(t) for t in tensors]
    T = [int(x) for x in _offsets(sizes)]
    for windows in ([(s - 1, s + 1), (0, 0), (7, 1000), (0, s + 1), (s, 2 * s + 5), (0, 0)], [(0, len(t) // E) for t in tensors],
                    [(2 * s, 2 * s + 100), (0, 0), (s - 1, s), (s, s), (0, 5 * s // 2), (0, 0)]):
        # plain: the base in the destination's layout, destination of its own
        D = _slots(windows, E)
        out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D, bases=bases)
        check_window(out, res, tensors, windows, E, D)
        # in place over the RESIDENT tensors: slot i starts at T[i] + a * E; only bytes [a * E, b * E) of every tensor change
        n = len(tensors)
        resident = _filled(T[-1], pc.cat(bases))
        D = np.asarray([T[i] + windows[i][0] * E for i in range(n)] + [T[-1]], np.uint64)
        r = _marked(n)
        sel, blocks = pwc.window_first(sizes, windows, E, seg_log)
        hip.tensor_decompress_window_dbatch(frames, foff, _offsets(sizes), windows, D, E, seg_log, np.asarray(first, np.uint64), sel_first=np.asarray(sel, np.uint64),
                                            max_total_blocks=blocks, base=resident, dst=resident, dst_capacity=T[-1], results=r)
        torch.cuda.synchronize()
        assert r.cpu().tolist() == [E * (b - a) for a, b in windows] + [MARK]
        want = np.concatenate([pc.cat(bases), np.full(TAIL, FILL, np.uint8)])
        for i, (a, b) in enumerate(windows):
            want[T[i] + a * E:T[i] + b * E] = tensors[i][a * E:b * E]
        assert (resident.cpu().numpy() == want).all()


def test_window_composite_in_one_hip_graph(hip):
    """one captured graph -- a single stream, a linear chain -- holding tensor_decompress_window_dbatch; replayed twice, the windows moved in between
    (inside the same segments: the counts, and with them every launch size, stay)"""
    E, seg_log = 2, 10
    s = 1 << seg_log
    tensors, _ = _corpus(E, seg_log)
    frames, foff, first = _compressed(hip, E, seg_log, "huf")
    sizes = [len(t) for t in tensors]
    n = len(sizes)
    both = ([(s - 1, 2 * s + 1), (0, 0), (5, s), (s - 1, s + 1), (s + 7, 2 * s + 9), (0, 0)], [(s - 3, 2 * s + 3), (0, 0), (2, s - 3), (s - 2, s + 1), (s + 8, 2 * s + 10), (0, 0)])
    sel, blocks = pwc.window_first(sizes, both[0], E, seg_log)
    assert pwc.window_first(sizes, both[1], E, seg_log) == (sel, blocks)
    nsel, nseg = sel[-1], first[-1]
    D = _slots([(0, max(b - a, d - c)) for (a, b), (c, d) in zip(*both)], E)
    total = int(D[-1])
    rsize = hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    rsize.restype = C.c_size_t
    ws = torch.empty(int(rsize(C.c_size_t(nsel), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
    soff, doff, sf, wf, win = _i64(_offsets(sizes)), _i64(D), _i64(first), _i64(sel), _i64(both[0])
    back, planes = _filled(total), _filled(nsel << seg_log)
    sfo, so = (torch.zeros(nsel + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    sres = torch.zeros(nsel, dtype=torch.int64, device="cuda")
    poff, psz = (torch.zeros(n * E, dtype=torch.int64, device="cuda") for _ in range(2))
    res = torch.zeros(n, dtype=torch.int64, device="cuda")

    def work():
        hip.tensor_decompress_window_dbatch(frames, foff, soff, win, doff, E, seg_log, sf, n_segments=nseg, sel_first=wf, n_selected=nsel, dst=back, dst_capacity=total,
                                            max_total_blocks=blocks, planes=planes, planes_capacity=nsel << seg_log, sel_frame_offsets=sfo, sel_offsets=so,
                                            sel_results=sres, plane_offsets=poff, plane_sizes=psz, workspace=ws, results=res)
    work(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    outs = []
    for windows in (both[1], both[0]):
        win.copy_(_i64(windows))
        back.fill_(FILL)
        res.zero_()
        g.replay()
        torch.cuda.synchronize()
        outs.append(back.cpu().numpy())
        assert (outs[-1][total:] == FILL).all()
        check_window(outs[-1][:total], res.cpu().tolist(), tensors, windows, E, D)
    assert not (outs[0] == outs[1]).all()


# ---------------------------------------------------------------------------------------------------------------- the user-facing call
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_decompress_tensor_windows(hip, monkeypatch):
    import finitestateentropy_amd.api as api
    gen = torch.Generator(device="cuda").manual_seed(29)
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
    shard = [(12 * 100, 24 * 100), None, (1023, 1025), (0, 300), (0, 0)]           # rows 12 .. 23 of 96: a 1 / 8 shard
    for kw in (dict(), dict(codec=1), dict(base=old), dict(codec=api.AutoCodec(20), base=old)):
        obj = hip.compress_tensors_segmented(new, 10, block_size_id=0, **kw)
        keep = [t.clone() for t in old]
        for windows in (shard, [(0, t.numel()) for t in new], [None] * 5, [(5, 5), (4499, 4500), None, (299, 300), None]):
            back = hip.decompress_tensor_windows(obj, windows, base=kw.get("base"))
            assert len(back) == 5
            for t, w, b in zip(new, windows, back):
                if w is None:
                    assert b is None
                    continue
                assert b.dtype == t.dtype and b.device == t.device and b.dim() == 1 and b.numel() == w[1] - w[0] and _bits(t.reshape(-1)[w[0]:w[1]], b)
                assert b.untyped_storage().nbytes() <= max(b.numel() * b.element_size(), 1) + 64, "it owns its memory, and no more than its window"
        assert all(_bits(a, b) for a, b in zip(old, keep)), "the bases are not changed"
        # a window over every element is decompress_tensors
        for a, b in zip(hip.decompress_tensors(obj, base=kw.get("base")), hip.decompress_tensor_windows(obj, [(0, t.numel()) for t in new], base=kw.get("base"))):
            assert _bits(a, b)
    assert _bits(api.decompress_tensor_windows(obj, shard, base=old)[0], new_bf.reshape(-1)[1200:2400]), "the module-level function"
    plain, whole = hip.compress_tensors_segmented(new, 10, block_size_id=0), hip.compress_tensors(new, block_size_id=0)

    # every mismatch is raised before a launch: from here on a call into the library is a failure of the test
    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in ("FSEHIP_tensor_decompress_window_dbatch", "FSEHIP_planes_select_window_dbatch", "FSEHIP_planes_fold_window_dbatch", "FSEHIP_tensor_decompress_seg_dbatch"):
        monkeypatch.setattr(hip.lib, name, no_launch)
    for o, w, b in ((whole, shard, None), (obj, shard, None), (plain, shard, old), (plain, shard[:4], None), (plain, [(0, 9601)] + shard[1:], None),
                    (plain, [(3, 2)] + shard[1:], None), (plain, [(-1, 2)] + shard[1:], None), (plain, [(0.0, 2)] + shard[1:], None), (plain, [(0, 1, 2)] + shard[1:], None),
                    (plain, [5] + shard[1:], None), (obj, shard, old[:4]), (plain, shard[:4] + [(0, 1)], None)):
        with pytest.raises(ValueError):
            hip.decompress_tensor_windows(o, w, base=b)

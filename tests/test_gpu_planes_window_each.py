"""Windows of tensors with a transform per tensor on the device (FSEHIP_planes_merge_window_each_dbatch, FSEHIP_tensor_decompress_window_each_dbatch
and decompress_tensor_windows_each) against the numpy model of planes_window_each_corpus.py and the tensors' own bytes.  Block-size id 0 with
segLog 10 and 11: a few KB already make several segments, and a segment of 1024 bytes is exactly one run of the predicted planes.  Every array
is longer than its contract and pre-filled: whatever the contract does not give to a call must still hold the fill afterwards -- the bytes in
front of a slot are where a lead that was not suppressed would land."""
import ctypes as C

import numpy as np
import pytest
import torch

import planes_corpus as pc
import planes_each_corpus as pe
import planes_seg_corpus as psc
import planes_window_corpus as pwc
import planes_window_each_corpus as pwe
from planes_corpus import GENERIC, TILE, TOO_SMALL
from planes_each_corpus import PLAIN, PRED, SUB, XOR

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = pwe.FILL, 64, -7
SEG_LOGS = (10, 11)
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _i64(a):
    """python ints of 64 bits, signed or not, flattened: the bits are what counts"""
    flat = np.asarray(a, dtype=object).reshape(-1)
    return torch.from_numpy(np.array([int(x) % (1 << 64) for x in flat], dtype=np.uint64).view(np.int64)).cuda()


def _marked(n):
    return torch.full((n + 1,), MARK, dtype=torch.int64, device="cuda")


def _filled(n, content=None):
    t = torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    if content is not None and len(content):
        t[:len(content)] = _dev(content)
    return t


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- 1, 2: the merge alone
def _plane_buffer(tensors, bases, transforms, windows, E, lead=3):
    """the whole planes of every tensor back to back behind `lead` bytes of fill -> (buffer, PO at the window's first byte, PS = b - a)"""
    parts, PO, PS, at = [np.full(lead, FILL, np.uint8)], [], [], lead
    for t, b, tr, (a, c) in zip(tensors, bases, transforms, windows):
        for p in pwe.whole_planes(t, b, E, tr if tr in pe.IDS else PLAIN):
            PO.append(at + a); PS.append(c - a); parts.append(p); at += len(p)
    return np.concatenate(parts), PO, PS


def run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, image=None, in_place=False, no_base=False, capacity=None):
    """-> (destination bytes, results).  image: what the base holds (the destination's layout); in place the destination starts as it"""
    n, total = len(D) - 1, int(D[-1])
    planes = _filled(len(planes_buf), planes_buf)
    base = None if no_base else _filled(total, image)
    dst = base if in_place else _filled(total)
    res = _marked(n)
    tr = _filled(n, np.asarray(transforms, np.uint8))
    out, _ = hip.planes_merge_window_each_dbatch(planes[:len(planes_buf)], _i64(PO), _i64(PS), np.asarray(D, np.uint64), windows, E, tr[:n],
                                                 base=None if base is None else base[:total], dst=dst, capacity=total if capacity is None else capacity, results=res)
    torch.cuda.synchronize()
    assert int(res[n]) == MARK and out.data_ptr() == dst.data_ptr()
    assert (planes.cpu().numpy()[:len(planes_buf)] == planes_buf).all(), "the planes are only read"
    if base is not None and not in_place:
        assert (base.cpu().numpy()[:total] == image).all(), "a base that is not the destination is only read"
    host = dst.cpu().numpy()
    assert (host[total:] == FILL).all(), "nothing behind the capacity"
    return host[:total], res.cpu().tolist()[:n]


def _base_image(bases, windows, D, E):
    image = np.full(int(D[-1]), FILL, np.uint8)
    for i, (a, b) in enumerate(windows):
        image[int(D[i]):int(D[i]) + E * (b - a)] = bases[i][a * E:b * E]
    return image


def check_slots(out, res, tensors, windows, E, D, untouched=None, failed=()):
    want = np.full(len(out), FILL, np.uint8) if untouched is None else untouched.copy()
    for i, (t, (a, b)) in enumerate(zip(tensors, windows)):
        if i not in failed:
            assert res[i] == E * (b - a), (i, res[i])
            want[int(D[i]):int(D[i]) + E * (b - a)] = t[a * E:b * E]
    bad = np.nonzero(out != want)[0]
    assert bad.size == 0, ("bytes that differ", bad[:8], [i for i in range(len(tensors)) if D[i] <= bad[0] < D[i + 1]], [int(out[x]) for x in bad[:8]])


@pytest.mark.parametrize("E", pc.ELEMS)
def test_window_merge_against_the_model(hip, E):
    c = pwe.merge_corpus(E)
    missing = [name for name, held in pwe.shapes(c, E).items() if not held]
    assert not missing, missing
    tensors, bases, transforms, windows, D = c["tensors"], c["bases"], c["transforms"], c["windows"], c["D"]
    planes_buf, PO, PS = _plane_buffer(tensors, bases, transforms, windows, E)
    for i in (0, 70, 200):                                       # the model, which the CPU suite holds against the whole inverse, says the same as the slice
        (a, b), at = windows[i], [PO[i * E + p] - windows[i][0] for p in range(E)]
        whole = [planes_buf[at[p]:at[p] + pc.plane_size(len(tensors[i]), p, E)] for p in range(E)]
        assert (pwe.window_merge_model(whole, bases[i][a * E:b * E], E, transforms[i], a, b) == tensors[i][a * E:b * E]).all()
    image = _base_image(bases, windows, D, E)
    out, res = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, image)
    check_slots(out, res, tensors, windows, E, D)
    # in place: the destination holds the windows of the bases; PLAIN and PRED tensors overwrite theirs, the gaps stay
    out, res = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, image, in_place=True)
    check_slots(out, res, tensors, windows, E, D, untouched=image)
    # without a base: XOR and SUB tensors are refused alone and not written
    out, res = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, no_base=True)
    failed = tuple(i for i, tr in enumerate(transforms) if tr >= XOR)
    assert failed and [res[i] for i in failed] == [GENERIC] * len(failed)
    check_slots(out, res, tensors, windows, E, D, failed=failed)


@pytest.mark.parametrize("E", [1, 8])
def test_the_extra_tile_of_a_lead(hip, E):
    """one PRED tensor whose slot starts at destination offset 0 and is E elements short of a tile: one item of the plain merge's mapping, but
    with the largest lead the virtual tensor needs two tiles"""
    a = 1023
    cnt = TILE - 1 if E == 1 else TILE // E - 1
    b = a + cnt
    assert (E * cnt) // TILE + 1 == 1 and -(-(E * (cnt + a % 1024)) // TILE) == 2
    rng = np.random.default_rng(E)
    x = (np.cumsum(rng.integers(-9, 10, b + 5)) + 70000).astype("<u8")
    t = np.ascontiguousarray(x.view(np.uint8).reshape(-1, 8)[:, :E]).reshape(-1)
    planes_buf, PO, PS = _plane_buffer([t], [t], [PRED], [(a, b)], E, lead=0)
    out, res = run_merge(hip, E, planes_buf, PO, PS, [0, E * cnt], [(a, b)], [PRED], no_base=True)
    check_slots(out, res, [t], [(a, b)], E, [0, E * cnt])
    # the same window two slots further on, behind an empty window and a tiny one: the search key steps by two per tensor
    ws, D = [(7, 7), (1, 3), (a, b)], [0, 0, 2 * E, 2 * E + E * cnt]
    planes_buf, PO, PS = _plane_buffer([t] * 3, [t] * 3, [PRED] * 3, ws, E, lead=0)
    out, res = run_merge(hip, E, planes_buf, PO, PS, D, ws, [PRED] * 3, no_base=True)
    check_slots(out, res, [t] * 3, ws, E, D)


# ---------------------------------------------------------------------------------------------------------------- 3: the composite
TRANSFORMS = [PRED, PLAIN, SUB, XOR, PLAIN, PRED, PRED, XOR]


def _corpus(E, seg_log, seed=0):
    """(tensors, bases) for TRANSFORMS: compressible bf16 data over two segments and a bit (PRED), nothing, noise of exactly one segment per plane
    (SUB), three symbols in turn, of a size that is no multiple of E (XOR), a skewed source of two segments and a half per plane (PLAIN), fewer bytes
    than an element, a skewed source of three segments and five elements (PRED: compressed blocks in every segment), two segments of a slow walk
    (XOR); the bases differ from the tensors in a byte in sixteen"""
    key = ("corpus", E, seg_log, seed)
    if key not in _CACHE:
        s = 1 << seg_log
        rng = np.random.default_rng(60 + E + seg_log + 1000 * seed)
        walk = (np.cumsum(rng.integers(-2, 3, 2 * s)) + 500).astype("<u8")
        tensors = [pc.bf16_gaussian(E * (2 * s + 100) // 2, 5 + E + seed), np.zeros(0, np.uint8), rng.integers(0, 256, E * s, dtype=np.uint8),
                   (77 + np.arange(E * (s + 1) + E - 1) % 3).astype(np.uint8), rng.integers(0, 4, 5 * E * s // 2, dtype=np.uint8),
                   rng.integers(0, 256, E - 1, dtype=np.uint8), rng.integers(0, 4, E * (3 * s + 5), dtype=np.uint8),
                   np.ascontiguousarray(walk.view(np.uint8).reshape(-1, 8)[:, :E]).reshape(-1)]
        bases = [t ^ (rng.integers(1, 256, t.size, dtype=np.uint8) * (rng.integers(0, 16, t.size) == 0)).astype(np.uint8) for t in tensors]
        _CACHE[key] = (tensors, bases)
    return _CACHE[key]


def _codec(form):
    from finitestateentropy_amd.api import AutoCodec
    return {"fse": 0, "huf": 1, "choose": AutoCodec(20)}[form]


def _compressed(hip, E, seg_log, form, transforms=TRANSFORMS, seed=0):
    """the corpus as segment frames written by tensor_compress_seg_each_dbatch with the transforms GIVEN -> (frames, frame offsets, segFirst);
    the full read gives the tensors back"""
    key = ("frames", E, seg_log, form, tuple(transforms), seed)
    if key not in _CACHE:
        tensors, bases = _corpus(E, seg_log, seed)
        sizes = [len(t) for t in tensors]
        S = _offsets(sizes)
        first = psc.seg_first(sizes, E, seg_log)
        src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))
        dst, foff, fres, tres, _, _ = hip.tensor_compress_seg_each_dbatch(src, S, E, seg_log, list(transforms), base, seg_first=np.asarray(first, np.uint64),
                                                                          codec=_codec(form), block_size_id=0)
        assert tres.cpu().tolist() == sizes and int(fres.min()) >= 8
        back, res = hip.tensor_decompress_seg_each_dbatch(dst, foff, S, E, seg_log, list(transforms), base, np.asarray(first, np.uint64))
        assert res.cpu().tolist() == sizes and torch.equal(back[:src.numel()], src)
        _CACHE[key] = (dst.clone(), foff.clone(), first)
    return _CACHE[key]


def _first(hip, sizes, windows, E, seg_log):
    """FSEHIP_planes_windowFirst itself: (selFirst, blocks) -- and the model's, which knows nothing of a lead"""
    n = len(sizes)
    off = (C.c_uint64 * (n + 1))(*[int(x) for x in _offsets(sizes)])
    win = (C.c_uint64 * (2 * n))(*[int(x) for w in windows for x in w])
    sel, blocks = (C.c_uint64 * (n * E + 1))(), C.c_size_t(0)
    f = hip.lib.FSEHIP_planes_windowFirst
    f.restype = C.c_size_t
    r = f(sel, C.byref(blocks), off, win, C.c_size_t(n), C.c_uint(E), C.c_uint(seg_log), C.c_uint(0))
    assert r == sel[n * E] and (list(sel), blocks.value) == tuple(pwc.window_first(sizes, windows, E, seg_log))
    return list(sel), blocks.value


def _slots(windows, E, pads=None, lead=0):
    pads = [(3 * i + 1) % 17 for i in range(len(windows))] if pads is None else pads
    return _offsets([E * (b - a) + p for (a, b), p in zip(windows, pads)]) + np.uint64(lead)


def run_window(hip, frames, foff, first, tensors, windows, E, seg_log, transforms=TRANSFORMS, D=None, bases=None, in_place=False, cap=None, sel=None,
               planes_capacity=None, old=False, held=None):
    """the composite with every array marked, nSelected and the block promise those of FSEHIP_planes_windowFirst, a planes buffer of exactly
    nSelected segments: -> (destination bytes, results, what the base held).  old: tensor_decompress_window_dbatch on the same arguments.
    held: the windows of the bases that the base buffer holds (default: `windows`; for windows that are none)"""
    sizes = [len(t) for t in tensors]
    n = len(sizes)
    D = _slots(windows, E) if D is None else D
    total = int(D[-1])
    image = np.full(total, FILL, np.uint8) if bases is None else _base_image(bases, windows if held is None else held, D, E)
    base = None if bases is None else _filled(total, image)
    back = base if in_place else _filled(total)
    sel, blocks = _first(hip, sizes, windows, E, seg_log) if sel is None else sel
    nsel = sel[-1]
    res, sfo, so, sres, poff, psz = _marked(n), _marked(nsel + 1), _marked(nsel + 1), _marked(nsel), _marked(n * E), _marked(n * E)
    planes = _filled(max(nsel, 1) << seg_log)
    kw = dict(sel_first=np.asarray(sel, np.uint64), base=base, dst=back, dst_capacity=total if cap is None else cap, max_total_blocks=blocks, planes=planes,
              planes_capacity=nsel << seg_log if planes_capacity is None else planes_capacity, sel_frame_offsets=sfo, sel_offsets=so, sel_results=sres,
              plane_offsets=poff, plane_sizes=psz, results=res)
    if old:
        hip.tensor_decompress_window_dbatch(frames, foff, _offsets(sizes), windows, D, E, seg_log, np.asarray(first, np.uint64), **kw)
    else:
        tr = _filled(n, np.asarray(transforms, np.uint8))
        hip.tensor_decompress_window_each_dbatch(frames, foff, _offsets(sizes), windows, D, E, seg_log, tr[:n], np.asarray(first, np.uint64), **kw)
    torch.cuda.synchronize()
    assert int(res[n]) == MARK and int(sfo[nsel + 1]) == MARK and int(so[nsel + 1]) == MARK and int(sres[nsel]) == MARK and int(poff[n * E]) == MARK
    assert int(psz[n * E]) == MARK and bool((planes[nsel << seg_log:] == FILL).all()) and bool((back[total:] == FILL).all())
    if base is not None and not in_place:
        assert (base.cpu().numpy()[:total] == image).all(), "a base that is not the destination is only read"
    return back.cpu().numpy()[:total], res.cpu().tolist()[:n], image


@pytest.mark.parametrize("form", ["fse", "huf", "choose"])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_window_is_the_slice_of_the_tensor_for_every_boundary_window(hip, E, form):
    assert set(TRANSFORMS) == set(pe.IDS)
    for seg_log in SEG_LOGS:
        tensors, bases = _corpus(E, seg_log)
        frames, foff, first = _compressed(hip, E, seg_log, form)
        cands = [pwc.boundary_windows(len(t) // E, seg_log) for t in tensors]
        seen, leads = set(), set()
        for rnd in range(max(len(c) for c in cands)):
            windows = [c[(rnd + 3 * i) % len(c)] for i, c in enumerate(cands)]
            D = _slots(windows, E, [(rnd + 5 * i) % 16 for i in range(len(tensors))], rnd % 16)
            out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D=D, bases=bases)
            check_slots(out, res, tensors, windows, E, D)
            seen |= {int(D[i]) % 16 for i, (a, b) in enumerate(windows) if b - a > 16}
            leads |= {pwe.lead(tr, a, b) for tr, (a, b) in zip(TRANSFORMS, windows)}
        assert seen == set(range(16)), "destination slots off every alignment"
        assert {0, 1, 1023} <= leads, "windows of PRED tensors on a run start, one behind it and one in front of the next"
        # every window of every tensor at once is the full read
        windows = [(0, len(t) // E) for t in tensors]
        out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, bases=bases)
        check_slots(out, res, tensors, windows, E, _slots(windows, E))


# ---------------------------------------------------------------------------------------------------------------- 4: damage
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_damage_in_a_selected_segment_and_in_unselected_ones(hip, checker, E, in_place):
    seg_log = 10
    s = 1 << seg_log
    tensors, bases = _corpus(E, seg_log)
    frames, foff, first = _compressed(hip, E, seg_log, "fse")
    frames = frames.clone()
    victim = 6                                               # PRED, noise of four symbols, four segments per plane: compressed blocks
    assert TRANSFORMS[victim] == PRED and first[victim * E + 1] - first[victim * E] == 4
    # the victim's window lies in segment 1 of every plane and starts five elements into its run: the lead is read from segment 1 itself
    windows = [(3, 40), (0, 0), (0, s), (1, 2), (5, s + 3), (0, 0), (s + 5, 2 * s - 3), (s - 1, s + 1)]
    assert pwe.lead(PRED, *windows[victim]) == 5
    D = _slots(windows, E)
    kw = dict(D=D, bases=bases, in_place=in_place)

    def flip(segment, at=5 + 3 + 40):
        f = first[victim * E] + segment                      # plane 0 of the victim
        lo, size = int(foff[f]), int(foff[f + 1] - foff[f])
        assert size > at + 8
        frames[lo + at] ^= 0x55
        return checker.frame_decompress(frames[lo:lo + size].cpu().numpy(), s)[0]
    # unselected: the segment in front of the window, and the one behind it, which lies in the extent of the selected frame
    for segment in (0, 2):
        r = flip(segment)
        assert r > (1 << 63), "the oracle's reader refuses the damaged frame"
        out, res, image = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, **kw)
        check_slots(out, res, tensors, windows, E, D, untouched=image if in_place else None)
        flip(segment)
    # selected: that tensor alone fails, with what the oracle's reader says of the frame, and its slot -- in place: its old bytes -- is untouched
    r = flip(1)
    assert r > (1 << 63)
    out, res, image = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, **kw)
    assert res[victim] == r - (1 << 64)
    check_slots(out, res, tensors, windows, E, D, untouched=image if in_place else None, failed=(victim,))
    flip(1)
    out, res, image = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, **kw)
    check_slots(out, res, tensors, windows, E, D, untouched=image if in_place else None)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_a_short_slot_and_a_short_planes_capacity_refuse_as_the_window_call_does(hip, E):
    """on an object of PLAIN tensors, whose frames are those of tensor_compress_seg_dbatch: both calls, the same arguments"""
    seg_log = 10
    s = 1 << seg_log
    tensors, _ = _corpus(E, seg_log)
    plain = [PLAIN] * len(tensors)
    frames, foff, first = _compressed(hip, E, seg_log, "fse", plain)
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s, s + 1), (s + 7, 2 * s + 9), (0, 0), (s + 5, 3 * s), (7, 2 * s)]
    sel, _ = _first(hip, [len(t) for t in tensors], windows, E, seg_log)
    D = _slots(windows, E, [3, 0, -1, 0, -E, 2, 1, 0])             # two slots that are short, by a byte and by an element
    decoded = sum(min(s, pc.plane_size(len(t), p, E) - k * s) for t, (a, b) in zip(tensors, windows) for p in range(E)
                  for k in pwc.selected(pc.plane_size(len(t), p, E), a, b, seg_log))
    assert decoded < sel[-1] << seg_log, "the last segments of planes are short: the decoded bytes lie back to back"
    for pcap in (None, decoded, decoded - 1, s):                   # all there is room for, exactly that, a byte less (the last frame, tensor 7's), one segment
        got = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, plain, D=D, planes_capacity=pcap)
        want = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D=D, planes_capacity=pcap, old=True)
        assert got[1] == want[1] and (got[0] == want[0]).all(), pcap
        assert got[1][2] == TOO_SMALL and got[1][4] == TOO_SMALL
        failed = tuple(i for i, r in enumerate(got[1]) if r < 0)
        assert failed == (2, 4) if pcap in (None, decoded) else (7 in failed and set(failed) > {2, 4}), (pcap, got[1])
        check_slots(got[0], got[1], tensors, windows, E, D, failed=failed)
    # the same with the transforms of the corpus: a PRED tensor whose slot is short is not written either
    frames, foff, first = _compressed(hip, E, seg_log, "fse")
    D = _slots(windows, E, [3, 0, 0, 0, 0, 2, -1, 0])
    out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D=D, bases=_corpus(E, seg_log)[1])
    assert res[6] == TOO_SMALL
    check_slots(out, res, tensors, windows, E, D, failed=(6,))
    # dstCapacity in front of the last slots' end: GENERIC for them, nothing at or behind it is written
    D = _slots(windows, E)
    out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D=D, bases=_corpus(E, seg_log)[1], cap=int(D[7]) - 1)
    assert res[6] == res[7] == GENERIC
    check_slots(out, res, tensors, windows, E, D, failed=(6, 7))


# ---------------------------------------------------------------------------------------------------------------- 5: refusals of one tensor
@pytest.mark.parametrize("E", pc.ELEMS)
def test_refusals_of_one_tensor(hip, E):
    seg_log = 10
    s = 1 << seg_log
    tensors, bases = _corpus(E, seg_log)
    frames, foff, first = _compressed(hip, E, seg_log, "huf")
    sizes = [len(t) for t in tensors]
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s, s + 1), (s + 7, 2 * s + 9), (0, 0), (s + 5, 3 * s), (7, 2 * s)]
    D = _slots(windows, E)
    # a transform byte that is none of the four (the estimate's 0xFF), on a PRED tensor with a lead and on a SUB tensor
    for k in (6, 2):
        tr = list(TRANSFORMS)
        tr[k] = 0xFF
        out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, tr, D=D, bases=bases)
        assert res[k] == GENERIC
        check_slots(out, res, tensors, windows, E, D, failed=(k,))
    # no base: the XOR and SUB tensors alone
    out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D=D)
    failed = tuple(i for i, tr in enumerate(TRANSFORMS) if tr >= XOR)
    assert [res[i] for i in failed] == [GENERIC] * len(failed)
    check_slots(out, res, tensors, windows, E, D, failed=failed)
    # a window with a > b, and one that ends behind its tensor: the selection takes nothing for them (what windowFirst says of an empty window)
    for k, w in ((6, (s + 5, s + 4)), (0, (s - 1, len(tensors[0]) // E + 1)), (7, (2 * s + 1, 2 * s))):
        bad = [w if i == k else x for i, x in enumerate(windows)]
        sel = _first(hip, sizes, [(5, 5) if i == k else x for i, x in enumerate(windows)], E, seg_log)
        slot = [(0, 4) if i == k else x for i, x in enumerate(windows)]
        Dk = _slots(slot, E)
        out, res, _ = run_window(hip, frames, foff, first, tensors, bad, E, seg_log, D=Dk, bases=bases, sel=sel, held=slot)
        assert res[k] == GENERIC, (k, res)
        check_slots(out, res, tensors, bad, E, Dk, failed=(k,))


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_merge_refuses_windows_that_disagree_and_a_lead_in_front_of_the_planes(hip, E):
    rng = np.random.default_rng(80 + E)
    m = 1500
    tensors = [rng.integers(0, 256, m * E, dtype=np.uint8) for _ in range(6)]
    transforms = [PRED, PLAIN, PRED, SUB, PRED, XOR]
    windows = [(1023, 1400), (3, 90), (5, 700), (17, 1040), (1030, 1500), (0, 16)]
    D = [int(x) for x in _slots(windows, E, lead=9)]
    planes_buf, PO, PS = _plane_buffer(tensors, tensors[::-1], transforms, windows, E, lead=0)
    image = _base_image(tensors[::-1], windows, D, E)
    out, res = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, image)
    check_slots(out, res, tensors, windows, E, D)

    def verdicts(ws, po, tr=transforms):
        return [pwe.merge_verdict(tr[i], True, ws[i][0], ws[i][1], E, PS[i * E:(i + 1) * E], po[i * E:(i + 1) * E], D[i + 1] - D[i]) for i in range(6)]
    # d_windows that disagree with the plane sizes -- one element more, one fewer at either end -- and a > b
    for k, w in ((0, (1023, 1401)), (1, (4, 90)), (3, (18, 1040)), (4, (1500, 1030)), (2, (700, 5))):
        ws = [w if i == k else x for i, x in enumerate(windows)]
        out, res = run_merge(hip, E, planes_buf, PO, PS, D, ws, transforms, image)
        assert res == verdicts(ws, PO) and res[k] == GENERIC and [r for i, r in enumerate(res) if i != k] == [E * (b - a) for i, (a, b) in enumerate(windows) if i != k]
        check_slots(out, res, tensors, windows, E, D, failed=(k,))
    # a PRED plane offset smaller than its lead: tensor 0 is the first in the planes buffer, its planes start at 0.  The window says lead 1023,
    # the offset of one plane says 1022 bytes in front of it
    for p in range(E):
        po = list(PO)
        po[p] = 1022
        ws = list(windows)
        out, res = run_merge(hip, E, planes_buf, po, PS, D, ws, transforms, image)
        assert res == verdicts(ws, po) and res[0] == GENERIC
        check_slots(out, res, tensors, windows, E, D, failed=(0,))
    # planes that start at offset 0 are fine for a transform without a lead and for a PRED window on a run start
    for tr0, w0 in ((PLAIN, (1023, 1400)), (PRED, (0, 377)), (PRED, (1024, 1401))):
        tr, ws = [tr0] + transforms[1:], [w0] + windows[1:]
        buf, po, ps = _plane_buffer(tensors, tensors[::-1], tr, ws, E, lead=0)
        po[0] = 0                                               # plane 0 of tensor 0: the window's bytes moved to the very start of the buffer
        buf[:w0[1] - w0[0]] = buf[w0[0]:w0[1]].copy()
        want = [t.copy() for t in tensors]
        if tr0 == PRED and w0[0]:                               # ... which for PRED is right only because a run starts there: nothing in front is needed
            assert w0[0] % 1024 == 0
        out, res = run_merge(hip, E, buf, po, ps, D, ws, tr, image)
        assert res == verdicts(ws, po, tr) == [E * (b - a) for a, b in ws]
        check_slots(out, res, want, ws, E, D)


# ---------------------------------------------------------------------------------------------------------------- 6: in place
@pytest.mark.parametrize("codec", ["fse", "huf"])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_windows_over_resident_tensors_in_place(hip, E, codec):
    """XOR and SUB tensors rebuilt over the resident window slices of their bases, PLAIN and PRED tensors written beside them"""
    seg_log = 11
    s = 1 << seg_log
    tensors, bases = _corpus(E, seg_log)
    frames, foff, first = _compressed(hip, E, seg_log, codec)
    sizes = [len(t) for t in tensors]
    T = [int(x) for x in _offsets(sizes)]
    n = len(tensors)
    for windows in ([(s - 1, s + 1), (0, 0), (7, 1000), (0, s + 1), (s, 2 * s + 5), (0, 0), (1023, 3 * s), (5, s + 9)], [(0, len(t) // E) for t in tensors],
                    [(2 * s, 2 * s + 100), (0, 0), (s - 1, s), (s, s), (0, 5 * s // 2), (0, 0), (2 * s + 1025, 3 * s + 5), (1, 2)]):
        resident = _filled(T[-1], pc.cat(bases))
        D = np.asarray([T[i] + windows[i][0] * E for i in range(n)] + [T[-1]], np.uint64)
        r = _marked(n)
        sel, blocks = _first(hip, sizes, windows, E, seg_log)
        hip.tensor_decompress_window_each_dbatch(frames, foff, _offsets(sizes), windows, D, E, seg_log, TRANSFORMS, np.asarray(first, np.uint64),
                                                 sel_first=np.asarray(sel, np.uint64), max_total_blocks=blocks, base=resident, dst=resident, dst_capacity=T[-1], results=r)
        torch.cuda.synchronize()
        assert r.cpu().tolist() == [E * (b - a) for a, b in windows] + [MARK]
        want = np.concatenate([pc.cat(bases), np.full(TAIL, FILL, np.uint8)])
        for i, (a, b) in enumerate(windows):
            want[T[i] + a * E:T[i] + b * E] = tensors[i][a * E:b * E]
        assert (resident.cpu().numpy() == want).all()


# ---------------------------------------------------------------------------------------------------------------- 7: one captured graph
def test_window_each_composite_in_one_hip_graph(hip):
    """one captured graph -- a single stream, a linear chain -- holding tensor_decompress_window_each_dbatch; replayed after the frames were written
    anew, in place, from changed tensors of the same sizes (the counts, and with them every launch size, stay)"""
    E, seg_log = 2, 10
    s = 1 << seg_log
    both = [_corpus(E, seg_log, seed) for seed in (0, 1)]
    sizes = [len(t) for t in both[0][0]]
    assert sizes == [len(t) for t in both[1][0]] and any((a != b).any() for a, b in zip(both[0][0], both[1][0]))
    n = len(sizes)
    first = psc.seg_first(sizes, E, seg_log)
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s - 1, s + 1), (s + 7, 2 * s + 9), (0, 0), (s + 5, 3 * s + 2), (1023, s + 40)]
    sel, blocks = _first(hip, sizes, windows, E, seg_log)
    nsel, nseg = sel[-1], first[-1]
    D = _slots(windows, E)
    total = int(D[-1])
    S = _offsets(sizes)
    room = hip.frame_packed_bound(int(S[-1]), nseg, hip.planes_block_bound(int(S[-1]), n, E, 0))
    frames = torch.zeros(room, dtype=torch.uint8, device="cuda")
    foff = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
    src, sbase = torch.zeros(int(S[-1]), dtype=torch.uint8, device="cuda"), torch.zeros(int(S[-1]), dtype=torch.uint8, device="cuda")

    def write(k):
        src.copy_(_dev(pc.cat(both[k][0]))); sbase.copy_(_dev(pc.cat(both[k][1])))
        _, _, fres, tres, _, _ = hip.tensor_compress_seg_each_dbatch(src, S, E, seg_log, TRANSFORMS, sbase, seg_first=np.asarray(first, np.uint64), codec=1, block_size_id=0,
                                                                     dst=frames, frame_offsets=foff)
        assert tres.cpu().tolist() == sizes and int(fres.min()) >= 8
    rsize = hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    rsize.restype = C.c_size_t
    ws = torch.empty(int(rsize(C.c_size_t(nsel), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
    soff, doff, sf, wf, win, tr = _i64(S), _i64(D), _i64(first), _i64(sel), _i64(windows), _dev(TRANSFORMS)
    back, base, planes = _filled(total), _filled(total), _filled(nsel << seg_log)
    sfo, so = (torch.zeros(nsel + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    sres = torch.zeros(nsel, dtype=torch.int64, device="cuda")
    poff, psz = (torch.zeros(n * E, dtype=torch.int64, device="cuda") for _ in range(2))
    res = torch.zeros(n, dtype=torch.int64, device="cuda")

    def work():
        hip.tensor_decompress_window_each_dbatch(frames, foff, soff, win, doff, E, seg_log, tr, sf, n_segments=nseg, sel_first=wf, n_selected=nsel, base=base, dst=back,
                                                 dst_capacity=total, max_total_blocks=blocks, planes=planes, planes_capacity=nsel << seg_log, sel_frame_offsets=sfo,
                                                 sel_offsets=so, sel_results=sres, plane_offsets=poff, plane_sizes=psz, workspace=ws, results=res)
    write(0)
    base[:total] = _dev(_base_image(both[0][1], windows, D, E))
    work(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    outs = []
    for k in (1, 0):
        write(k)
        base[:total] = _dev(_base_image(both[k][1], windows, D, E))
        back.fill_(FILL)
        res.zero_()
        g.replay()
        torch.cuda.synchronize()
        outs.append(back.cpu().numpy())
        assert (outs[-1][total:] == FILL).all()
        check_slots(outs[-1][:total], res.cpu().tolist(), both[k][0], windows, E, D)
    assert not (outs[0] == outs[1]).all()


# ---------------------------------------------------------------------------------------------------------------- 8: the user-facing call
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_decompress_tensor_windows_each(hip, monkeypatch):
    import finitestateentropy_amd.api as api
    gen = torch.Generator(device="cuda").manual_seed(31)
    old_bf = (torch.randn((96, 1000), generator=gen, device="cuda") * 0.02).to(torch.bfloat16)
    new_bf = (old_bf.float() * (1 + 1e-2 * torch.randn((96, 1000), generator=gen, device="cuda"))).to(torch.bfloat16)
    old_f = torch.randn((15000, 3), generator=gen, device="cuda") * 0.02
    new_f = old_f + torch.randn((15000, 3), generator=gen, device="cuda") * 2e-5
    old_i = torch.randint(-128, 128, (400, 500), generator=gen, device="cuda", dtype=torch.int8)
    new_i = old_i.clone(); new_i[1, ::7] += 1
    new_d = torch.cumsum(torch.randint(0, 1000, (70000,), generator=gen, device="cuda", dtype=torch.int64), 0)       # sorted: the estimate takes "pred"
    old_d = torch.randint(-2 ** 62, 2 ** 62, (70000,), generator=gen, device="cuda", dtype=torch.int64)
    empty = torch.zeros((0, 3), device="cuda", dtype=torch.float32)
    old, new = [old_bf, old_f, old_i, old_d, empty], [new_bf, new_f, new_i, new_d, empty.clone()]
    numel = [t.numel() for t in new]
    shard = [(12 * 1000, 24 * 1000), None, (1023, 1025), (70000 // 8 + 3, 70000 // 4), (0, 0)]        # rows 12 .. 23 of 96: a 1 / 8 shard
    sets = (shard, [(0, m) for m in numel], [None] * 5, [(5, 5), (44999, 45000), None, (33791, 69999), None], [(1023, 95000), (2047, 2049), (1025, 199999), (1, 2), None])
    auto = hip.compress_tensors_each(new, "auto", old, segment_log=15)
    assert len(auto.transforms) == 5 and set(auto.transforms) <= set(api.EST_NAMES)
    given = hip.compress_tensors_each(new, ["pred", "xor", "plain", "pred", "sub"], old, segment_log=15)
    nobase = hip.compress_tensors_each(new, ["pred", "plain", "pred", "pred", "plain"], segment_log=15)
    predicted = hip.compress_tensors_segmented(new, 15, api.PredictedPlanes(0))
    plain = hip.compress_tensors_segmented(new, 15)
    delta = hip.compress_tensors_segmented(new, 15, base=api.DeltaBase(old, "sub"))
    reopened = hip.open_archive(hip.archive_tensors(auto))
    assert reopened.transforms == auto.transforms and reopened.segment_log == 15
    objs = ((auto, old), (given, old), (nobase, None), (predicted, None), (plain, None), (delta, api.DeltaBase(old, "sub")), (reopened, old))
    keep = [t.clone() for t in old]
    for obj, base in objs:
        whole = hip.decompress_tensors(obj, base=base)
        assert all(_bits(a, b) for a, b in zip(whole, new))
        for windows in sets:
            back = hip.decompress_tensor_windows_each(obj, windows, base=base)
            assert len(back) == 5
            for t, w, b in zip(whole, windows, back):
                if w is None:
                    assert b is None
                    continue
                assert b.dtype == t.dtype and b.device == t.device and b.dim() == 1 and b.numel() == w[1] - w[0] and _bits(t.reshape(-1)[w[0]:w[1]], b)
                assert b.untyped_storage().nbytes() <= max(b.numel() * b.element_size(), 1) + 64, "it owns its memory, and no more than its window"
    assert all(_bits(a, b) for a, b in zip(old, keep)), "the bases are not changed"
    assert _bits(api.decompress_tensor_windows_each(auto, shard, base=old)[0], new_bf.reshape(-1)[12000:24000]), "the module-level function"
    unsegmented, sparse = hip.compress_tensors_each(new, "auto", old), hip.compress_tensors_segmented(new, 15, api.SparsePlanes(0))
    other = hip.compress_tensors_segmented(new, 15, api.PredictedPlanes(0))
    other.predictor = "next"

    # every mismatch is raised before a launch: from here on a call into the library is a failure of the test
    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in ("FSEHIP_tensor_decompress_window_each_dbatch", "FSEHIP_planes_merge_window_each_dbatch", "FSEHIP_tensor_decompress_window_dbatch",
                 "FSEHIP_planes_select_window_dbatch", "FSEHIP_planes_fold_window_dbatch", "FSEHIP_tensor_decompress_seg_each_dbatch", "FSEHIP_tensor_patch_window_dbatch"):
        monkeypatch.setattr(hip.lib, name, no_launch)
    for o, w, b in ((unsegmented, shard, old), (sparse, shard, None), (auto, shard[:4], old), (auto, [(0, 96001)] + shard[1:], old), (auto, [(3, 2)] + shard[1:], old),
                    (auto, [(-1, 2)] + shard[1:], old), (auto, [(0.0, 2)] + shard[1:], old), (auto, [(0, 1, 2)] + shard[1:], old), (auto, [5] + shard[1:], old),
                    (other, shard, None), (auto, shard, None), (given, shard, None), (nobase, shard, old), (predicted, shard, old), (plain, shard, old),
                    (delta, shard, None), (delta, shard, api.DeltaBase(old, "xor")), (auto, shard, old[:4])):
        with pytest.raises(ValueError):
            hip.decompress_tensor_windows_each(o, w, base=b)
    # the old name keeps refusing these objects
    for o, b in ((auto, old), (reopened, old), (predicted, None)):
        with pytest.raises(ValueError):
            hip.decompress_tensor_windows(o, shard, base=b)
        with pytest.raises(ValueError):
            hip.patch_tensor_windows(o, new, shard, base=b)

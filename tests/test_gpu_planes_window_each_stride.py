"""Windows of tensors with a stride per tensor on the device (FSEHIP_planes_merge_window_each_stride_dbatch,
FSEHIP_tensor_decompress_window_each_stride_dbatch and decompress_tensor_windows_each_stride) against the numpy model of
planes_window_each_stride_corpus.py, the tensors' own bytes and the _window_each_ siblings.  Block-size id 0 with segLog 10 and 11: a few KB
already make several segments, and a segment of 1024 bytes is exactly one run of the predicted planes.  Every array is longer than its contract
and pre-filled: whatever the contract does not give to a call must still hold the fill afterwards -- the bytes in front of a slot are where a
lead that was not suppressed would land."""
import ctypes as C

import numpy as np
import pytest
import torch

import planes_corpus as pc
import planes_each_corpus as pe
import planes_seg_corpus as psc
import planes_window_corpus as pwc
import planes_window_each_stride_corpus as pws
from planes_corpus import GENERIC, TILE
from planes_each_corpus import PLAIN, PRED, SUB, XOR

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = pws.FILL, 64, -7
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
def _plane_buffer(tensors, bases, transforms, strides, windows, E, lead=3):
    """the whole planes of every tensor back to back behind `lead` bytes of fill -> (buffer, PO at the window's first byte, PS = b - a).  A
    tensor that the call is to refuse has the planes of stride 1"""
    parts, PO, PS, at = [np.full(lead, FILL, np.uint8)], [], [], lead
    for t, b, tr, st, (a, c) in zip(tensors, bases, transforms, strides, windows):
        st = st if tr == PRED and 1 <= st <= 8 else 1
        for p in pws.whole_planes(t, b, E, tr if tr in pe.IDS else PLAIN, st):
            PO.append(at + a); PS.append(c - a); parts.append(p); at += len(p)
    return np.concatenate(parts), PO, PS


def run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, strides, image=None, in_place=False, no_base=False, sibling=False):
    """-> (destination bytes, results).  image: what the base holds (the destination's layout); in place the destination starts as it.
    strides None: a NULL d_strides.  sibling: FSEHIP_planes_merge_window_each_dbatch on the same arguments"""
    n, total = len(D) - 1, int(D[-1])
    planes = _filled(len(planes_buf), planes_buf)
    base = None if no_base else _filled(total, image)
    dst = base if in_place else _filled(total)
    res = _marked(n)
    tr = _filled(n, np.asarray(transforms, np.uint8))
    st = None if strides is None else _filled(n, np.asarray(strides, np.uint8))
    args = (planes[:len(planes_buf)], _i64(PO), _i64(PS), np.asarray(D, np.uint64), windows, E, tr[:n])
    kw = dict(base=None if base is None else base[:total], dst=dst, capacity=total, results=res)
    if sibling:
        out, _ = hip.planes_merge_window_each_dbatch(*args, **kw)
    else:
        out, _ = hip.planes_merge_window_each_stride_dbatch(*args, None if st is None else st[:n], **kw)
    torch.cuda.synchronize()
    assert int(res[n]) == MARK and out.data_ptr() == dst.data_ptr()
    assert (planes.cpu().numpy()[:len(planes_buf)] == planes_buf).all(), "the planes are only read"
    assert st is None or (st.cpu().numpy()[:n] == np.asarray(strides, np.uint8)).all(), "the strides are only read"
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
    c = pws.merge_corpus(E)
    missing = [name for name, held in pws.shapes(c, E).items() if not held]
    assert not missing, missing
    tensors, bases, transforms, strides, windows, D = c["tensors"], c["bases"], c["transforms"], c["strides"], c["windows"], c["D"]
    planes_buf, PO, PS = _plane_buffer(tensors, bases, transforms, strides, windows, E)
    for i in (0, 1, 62, c["first_med"] + 40, len(tensors) - 3):   # the model, which the CPU suite holds against the whole inverse, says the same as the slice
        (a, b), at = windows[i], [PO[i * E + p] - windows[i][0] for p in range(E)]
        whole = [planes_buf[at[p]:at[p] + pc.plane_size(len(tensors[i]), p, E)] for p in range(E)]
        assert (pws.window_merge_model(whole, bases[i][a * E:b * E], E, transforms[i], strides[i], a, b) == tensors[i][a * E:b * E]).all()
    image = _base_image(bases, windows, D, E)
    out, res = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, strides, image)
    check_slots(out, res, tensors, windows, E, D)
    # in place: the destination holds the windows of the bases; PLAIN and PRED tensors overwrite theirs, the gaps stay
    out, res = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, strides, image, in_place=True)
    check_slots(out, res, tensors, windows, E, D, untouched=image)
    # without a base: XOR and SUB tensors are refused alone and not written
    out, res = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, strides, no_base=True)
    failed = tuple(i for i, tr in enumerate(transforms) if tr >= XOR)
    assert failed and [res[i] for i in failed] == [GENERIC] * len(failed)
    check_slots(out, res, tensors, windows, E, D, failed=failed)


@pytest.mark.parametrize("S", [3, 7])
@pytest.mark.parametrize("E", [1, 8])
def test_the_extra_tile_of_a_lead_at_a_stride_that_does_not_divide_16(hip, E, S):
    """one PRED tensor whose slot starts at destination offset 0 and is E elements short of a tile: one item of the plain merge's mapping, but
    with the largest lead the virtual tensor needs two tiles"""
    a = 1023
    cnt = TILE - 1 if E == 1 else TILE // E - 1
    b = a + cnt
    assert (E * cnt) // TILE + 1 == 1 and -(-(E * (cnt + a % 1024)) // TILE) == 2 and 16 % S
    rng = np.random.default_rng(E + S)
    t = pws._smooth(rng, b + 5, E, S)
    planes_buf, PO, PS = _plane_buffer([t], [t], [PRED], [S], [(a, b)], E, lead=0)
    out, res = run_merge(hip, E, planes_buf, PO, PS, [0, E * cnt], [(a, b)], [PRED], [S], no_base=True)
    check_slots(out, res, [t], [(a, b)], E, [0, E * cnt])
    # the same window two slots further on, behind an empty window and one shorter than S: the search key steps by two per tensor
    ws, D = [(7, 7), (1, 3), (a, b)], [0, 0, 2 * E, 2 * E + E * cnt]
    planes_buf, PO, PS = _plane_buffer([t] * 3, [t] * 3, [PRED] * 3, [S] * 3, ws, E, lead=0)
    out, res = run_merge(hip, E, planes_buf, PO, PS, D, ws, [PRED] * 3, [S] * 3, no_base=True)
    check_slots(out, res, [t] * 3, ws, E, D)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_null_strides_and_all_ones_are_the_sibling_byte_for_byte(hip, E):
    """on the corpus of the merge test, whose PRED planes at strides above 1 are then simply other data: destination and results of
    FSEHIP_planes_merge_window_each_dbatch, FSEHIP_planes_merge_window_each_stride_dbatch with d_strides NULL and with all ones"""
    c = pws.merge_corpus(E)
    tensors, bases, transforms, strides, windows, D = c["tensors"], c["bases"], c["transforms"], c["strides"], c["windows"], c["D"]
    planes_buf, PO, PS = _plane_buffer(tensors, bases, transforms, strides, windows, E)
    image = _base_image(bases, windows, D, E)
    want = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, None, image, sibling=True)
    assert min(want[1]) >= 0
    for st in (None, [1] * len(tensors)):
        got = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, st, image)
        assert got[1] == want[1] and (got[0] == want[0]).all()
    # ... and the bytes are not those of the strided call, which reads the same planes as what they are
    out, _ = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, strides, image)
    assert (out != want[0]).any()


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_merge_refuses_one_tensor(hip, E):
    """a PRED tensor whose stride byte is 0 or 9, a window that disagrees with the verdict, a lead in front of the planes buffer: GENERIC for
    that tensor alone, the others are served, in place the refused tensor keeps its bytes; the stride byte of another transform is not read"""
    rng = np.random.default_rng(90 + E)
    m = 1500
    tensors = [rng.integers(0, 256, m * E, dtype=np.uint8) for _ in range(6)]
    transforms = [PRED, PLAIN, PRED, SUB, PRED, XOR]
    strides = [3, 0, 8, 0xFF, 5, 9]
    windows = [(1023, 1400), (3, 90), (5, 700), (17, 1040), (1030, 1500), (0, 16)]
    D = [int(x) for x in _offsets([E * (b - a) + (3 * i + 1) % 17 for i, (a, b) in enumerate(windows)]) + np.uint64(9)]
    bases = tensors[::-1]
    planes_buf, PO, PS = _plane_buffer(tensors, bases, transforms, strides, windows, E, lead=0)
    image = _base_image(bases, windows, D, E)
    out, res = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, strides, image)
    check_slots(out, res, tensors, windows, E, D)

    def verdicts(ws, po, st):
        return [pws.merge_verdict(transforms[i], st[i], True, ws[i][0], ws[i][1], E, PS[i * E:(i + 1) * E], po[i * E:(i + 1) * E], D[i + 1] - D[i]) for i in range(6)]
    good = [E * (b - a) for a, b in windows]
    for k in (0, 2, 4):
        for bad in (0, 9, 0xFF):
            st = [bad if i == k else x for i, x in enumerate(strides)]
            for in_place in (False, True):
                out, res = run_merge(hip, E, planes_buf, PO, PS, D, windows, transforms, st, image, in_place=in_place)
                assert res == verdicts(windows, PO, st) == good[:k] + [GENERIC] + good[k + 1:]
                check_slots(out, res, tensors, windows, E, D, untouched=image if in_place else None, failed=(k,))
    # d_windows that disagree with the plane sizes -- one element more, one fewer at either end -- and a > b
    for k, w in ((0, (1023, 1401)), (2, (6, 700)), (4, (1500, 1030)), (3, (18, 1040))):
        ws = [w if i == k else x for i, x in enumerate(windows)]
        out, res = run_merge(hip, E, planes_buf, PO, PS, D, ws, transforms, strides, image)
        assert res == verdicts(ws, PO, strides) == good[:k] + [GENERIC] + good[k + 1:]
        check_slots(out, res, tensors, windows, E, D, failed=(k,))
    # a PRED plane offset smaller than its lead: tensor 0 is the first in the planes buffer, its planes start at 0
    for p in range(E):
        po = list(PO)
        po[p] = 1022
        out, res = run_merge(hip, E, planes_buf, po, PS, D, windows, transforms, strides, image)
        assert res == verdicts(windows, po, strides) and res[0] == GENERIC and res[1:] == good[1:]
        check_slots(out, res, tensors, windows, E, D, failed=(0,))


# ---------------------------------------------------------------------------------------------------------------- 3: the composite
TRANSFORMS = [PRED, PLAIN, SUB, XOR, PLAIN, PRED, PRED, XOR]
STRIDES = [3, 0xFF, 0, 9, 1, 2, 5, 0]                          # (read for the PRED tensors alone)


def _corpus(E, seg_log, seed=0):
    """(tensors, bases) for TRANSFORMS: three interleaved walks over two segments and a bit (PRED at 3), nothing, noise of exactly one segment
    per plane (SUB), three symbols in turn, of a size that is no multiple of E (XOR), a skewed source of two segments and a half per plane
    (PLAIN), fewer bytes than an element (PRED at 2), a skewed source of three segments and five elements (PRED at 5: compressed blocks in
    every segment), two segments of a slow walk (XOR); the bases differ from the tensors in a byte in sixteen"""
    key = ("corpus", E, seg_log, seed)
    if key not in _CACHE:
        s = 1 << seg_log
        rng = np.random.default_rng(160 + E + seg_log + 1000 * seed)
        walk = (np.cumsum(rng.integers(-2, 3, 2 * s)) + 500).astype("<u8")
        tensors = [pws._smooth(rng, 2 * s + 100, E, 3), np.zeros(0, np.uint8), rng.integers(0, 256, E * s, dtype=np.uint8),
                   (77 + np.arange(E * (s + 1) + E - 1) % 3).astype(np.uint8), rng.integers(0, 4, 5 * E * s // 2, dtype=np.uint8),
                   rng.integers(0, 256, E - 1, dtype=np.uint8), rng.integers(0, 4, E * (3 * s + 5), dtype=np.uint8),
                   np.ascontiguousarray(walk.view(np.uint8).reshape(-1, 8)[:, :E]).reshape(-1)]
        bases = [t ^ (rng.integers(1, 256, t.size, dtype=np.uint8) * (rng.integers(0, 16, t.size) == 0)).astype(np.uint8) for t in tensors]
        _CACHE[key] = (tensors, bases)
    return _CACHE[key]


def _codec(form):
    from finitestateentropy_amd.api import AutoCodec
    return {"fse": 0, "huf": 1, "choose": AutoCodec(20)}[form]


def _compressed(hip, E, seg_log, form, strides=STRIDES, seed=0):
    """the corpus as segment frames written by tensor_compress_seg_each_stride_dbatch with transforms and strides GIVEN -> (frames, frame
    offsets, segFirst); the full read gives the tensors back"""
    key = ("frames", E, seg_log, form, None if strides is None else tuple(strides), seed)
    if key not in _CACHE:
        tensors, bases = _corpus(E, seg_log, seed)
        sizes = [len(t) for t in tensors]
        S = _offsets(sizes)
        first = psc.seg_first(sizes, E, seg_log)
        src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))
        st = None if strides is None else _dev(strides)
        dst, foff, fres, tres = hip.tensor_compress_seg_each_stride_dbatch(src, S, E, seg_log, list(TRANSFORMS), st, base, seg_first=np.asarray(first, np.uint64),
                                                                           codec=_codec(form), block_size_id=0)[:4]
        assert tres.cpu().tolist() == sizes and int(fres.min()) >= 8
        back, res = hip.tensor_decompress_seg_each_stride_dbatch(dst, foff, S, E, seg_log, list(TRANSFORMS), st, base, np.asarray(first, np.uint64))
        assert res.cpu().tolist() == sizes and torch.equal(back[:src.numel()], src)
        _CACHE[key] = (dst.clone(), foff.clone(), first)
    return _CACHE[key]


def _first(hip, sizes, windows, E, seg_log):
    """FSEHIP_planes_windowFirst itself: (selFirst, blocks) -- and the model's, which knows nothing of a lead or a stride"""
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


def run_window(hip, frames, foff, first, tensors, windows, E, seg_log, strides=STRIDES, D=None, bases=None, in_place=False, sibling=False):
    """the composite with every array marked, nSelected and the block promise those of FSEHIP_planes_windowFirst, a planes buffer of exactly
    nSelected segments: -> (destination bytes, results, what the base held).  strides None: a NULL d_strides.  sibling:
    tensor_decompress_window_each_dbatch on the same arguments"""
    sizes = [len(t) for t in tensors]
    n = len(sizes)
    D = _slots(windows, E) if D is None else D
    total = int(D[-1])
    image = np.full(total, FILL, np.uint8) if bases is None else _base_image(bases, windows, D, E)
    base = None if bases is None else _filled(total, image)
    back = base if in_place else _filled(total)
    sel, blocks = _first(hip, sizes, windows, E, seg_log)
    nsel = sel[-1]
    res, sfo, so, sres, poff, psz = _marked(n), _marked(nsel + 1), _marked(nsel + 1), _marked(nsel), _marked(n * E), _marked(n * E)
    planes = _filled(max(nsel, 1) << seg_log)
    kw = dict(sel_first=np.asarray(sel, np.uint64), base=base, dst=back, dst_capacity=total, max_total_blocks=blocks, planes=planes, planes_capacity=nsel << seg_log,
              sel_frame_offsets=sfo, sel_offsets=so, sel_results=sres, plane_offsets=poff, plane_sizes=psz, results=res)
    tr = _filled(n, np.asarray(TRANSFORMS, np.uint8))
    if sibling:
        hip.tensor_decompress_window_each_dbatch(frames, foff, _offsets(sizes), windows, D, E, seg_log, tr[:n], np.asarray(first, np.uint64), **kw)
    else:
        st = None if strides is None else _filled(n, np.asarray(strides, np.uint8))[:n]
        hip.tensor_decompress_window_each_stride_dbatch(frames, foff, _offsets(sizes), windows, D, E, seg_log, tr[:n], st, np.asarray(first, np.uint64), **kw)
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
        leads = set()
        for rnd in range(max(len(c) for c in cands)):
            windows = [c[(rnd + 3 * i) % len(c)] for i, c in enumerate(cands)]
            D = _slots(windows, E, [(rnd + 5 * i) % 16 for i in range(len(tensors))], rnd % 16)
            out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D=D, bases=bases)
            check_slots(out, res, tensors, windows, E, D)
            leads |= {(st, pws.lead(tr, a, b)) for tr, st, (a, b) in zip(TRANSFORMS, STRIDES, windows) if tr == PRED}
        assert {(S, L) for S in (3, 5) for L in (0, 1, 1023)} <= leads, "windows of strided tensors on a run start, one behind it and one in front of the next"
        # every window of every tensor at once is the full read
        windows = [(0, len(t) // E) for t in tensors]
        out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, bases=bases)
        check_slots(out, res, tensors, windows, E, _slots(windows, E))


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_composite_with_null_strides_and_all_ones_is_the_sibling(hip, E):
    seg_log = 10
    s = 1 << seg_log
    tensors, bases = _corpus(E, seg_log)
    frames, foff, first = _compressed(hip, E, seg_log, "huf", None)
    ones = _compressed(hip, E, seg_log, "huf", [1] * 8)
    end = int(foff[-1])
    assert torch.equal(ones[1], foff) and torch.equal(ones[0][:end], frames[:end]), "stride 1 given writes the frames of no strides"
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s, s + 1), (s + 7, 2 * s + 9), (0, 0), (s + 5, 3 * s), (7, 2 * s)]
    want = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, bases=bases, sibling=True)
    check_slots(want[0], want[1], tensors, windows, E, _slots(windows, E))
    for st in (None, [1] * 8, [1, 0, 9, 0xFF, 0, 1, 1, 7]):
        got = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, strides=st, bases=bases)
        assert got[1] == want[1] and (got[0] == want[0]).all(), st


# ---------------------------------------------------------------------------------------------------------------- 4: refusals and damage
@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_composite_refuses_one_tensor(hip, E):
    seg_log = 10
    s = 1 << seg_log
    tensors, bases = _corpus(E, seg_log)
    frames, foff, first = _compressed(hip, E, seg_log, "huf")
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s, s + 1), (s + 7, 2 * s + 9), (0, 0), (s + 5, 3 * s), (7, 2 * s)]
    D = _slots(windows, E)
    for k in (0, 6):                                            # PRED tensors with a lead
        for bad in (0, 9):
            st = [bad if i == k else x for i, x in enumerate(STRIDES)]
            for in_place in (False, True):
                out, res, image = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, strides=st, D=D, bases=bases, in_place=in_place)
                assert res[k] == GENERIC
                check_slots(out, res, tensors, windows, E, D, untouched=image if in_place else None, failed=(k,))
    # no base: the XOR and SUB tensors alone
    out, res, _ = run_window(hip, frames, foff, first, tensors, windows, E, seg_log, D=D)
    failed = tuple(i for i, tr in enumerate(TRANSFORMS) if tr >= XOR)
    assert [res[i] for i in failed] == [GENERIC] * len(failed)
    check_slots(out, res, tensors, windows, E, D, failed=failed)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_damage_in_a_selected_segment_and_in_unselected_ones(hip, checker, E, in_place):
    seg_log = 10
    s = 1 << seg_log
    tensors, bases = _corpus(E, seg_log)
    frames, foff, first = _compressed(hip, E, seg_log, "fse")
    frames = frames.clone()
    victim = 6                                               # PRED at stride 5, noise of four symbols, four segments per plane: compressed blocks
    assert TRANSFORMS[victim] == PRED and STRIDES[victim] == 5 and first[victim * E + 1] - first[victim * E] == 4
    # the victim's window lies in segment 1 of every plane and starts seven elements into its run: a lead that is no multiple of 5, read from segment 1 itself
    windows = [(3, 40), (0, 0), (0, s), (1, 2), (5, s + 3), (0, 0), (s + 7, 2 * s - 3), (s - 1, s + 1)]
    assert pws.lead(PRED, *windows[victim]) == 7
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


# ---------------------------------------------------------------------------------------------------------------- 5: one captured graph
def test_window_each_stride_composite_in_one_hip_graph(hip):
    """one captured graph -- a single stream, a linear chain -- holding tensor_decompress_window_each_stride_dbatch; replayed twice after the frames
    were written anew, in place, from changed tensors of the same sizes (the counts, and with them every launch size, stay)"""
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
    tr, st = _dev(TRANSFORMS), _dev(STRIDES)

    def write(k):
        src.copy_(_dev(pc.cat(both[k][0]))); sbase.copy_(_dev(pc.cat(both[k][1])))
        _, _, fres, tres = hip.tensor_compress_seg_each_stride_dbatch(src, S, E, seg_log, TRANSFORMS, st, sbase, seg_first=np.asarray(first, np.uint64), codec=1,
                                                                      block_size_id=0, dst=frames, frame_offsets=foff)[:4]
        assert tres.cpu().tolist() == sizes and int(fres.min()) >= 8
    rsize = hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    rsize.restype = C.c_size_t
    ws = torch.empty(int(rsize(C.c_size_t(nsel), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
    soff, doff, sf, wf, win = _i64(S), _i64(D), _i64(first), _i64(sel), _i64(windows)
    back, base, planes = _filled(total), _filled(total), _filled(nsel << seg_log)
    sfo, so = (torch.zeros(nsel + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    sres = torch.zeros(nsel, dtype=torch.int64, device="cuda")
    poff, psz = (torch.zeros(n * E, dtype=torch.int64, device="cuda") for _ in range(2))
    res = torch.zeros(n, dtype=torch.int64, device="cuda")

    def work():
        hip.tensor_decompress_window_each_stride_dbatch(frames, foff, soff, win, doff, E, seg_log, tr, st, sf, n_segments=nseg, sel_first=wf, n_selected=nsel, base=base,
                                                        dst=back, dst_capacity=total, max_total_blocks=blocks, planes=planes, planes_capacity=nsel << seg_log,
                                                        sel_frame_offsets=sfo, sel_offsets=so, sel_results=sres, plane_offsets=poff, plane_sizes=psz, workspace=ws,
                                                        results=res)
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


# ---------------------------------------------------------------------------------------------------------------- 6: the user-facing call
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def user_tensors():
    """five tensors whose strides are [2, 3, 4, 1, 1]: stereo int16, float32 xyz, int32 boxes, sorted int64, bf16 weights"""
    gen = torch.Generator(device="cuda").manual_seed(41)

    def walk(shape, step, dtype):
        return torch.cumsum(torch.randint(-step, step + 1, shape, generator=gen, device="cuda", dtype=torch.int64), 0).to(dtype)
    stereo = (walk((30000, 2), 40, torch.int64) + torch.tensor([0, 3000], device="cuda")).to(torch.int16)
    xyz = torch.tensor([100.0, -37.0, 5.5], device="cuda") + torch.cumsum(torch.randn((15000, 3), generator=gen, device="cuda") * 1e-4, 0)
    boxes = torch.stack([walk((9000,), 50, torch.int64) + 100000, walk((9000,), 3, torch.int64) + 500, torch.randint(64, 72, (9000,), generator=gen, device="cuda"),
                         torch.randint(200, 216, (9000,), generator=gen, device="cuda")], 1).to(torch.int32)
    ids = torch.cumsum(torch.randint(0, 1000, (40000,), generator=gen, device="cuda", dtype=torch.int64), 0)
    bf = (torch.randn((96, 500), generator=gen, device="cuda") * 0.02).to(torch.bfloat16)
    return [stereo, xyz, boxes, ids, bf]


USER_NAMES, USER_STRIDES = ["pred", "pred", "pred", "pred", "plain"], [2, 3, 4, 1, 1]


def test_decompress_tensor_windows_each_stride(hip):
    import finitestateentropy_amd.api as api
    new = user_tensors()
    numel = [t.numel() for t in new]
    shard = [(60000 // 8 + 1, 60000 // 4), None, (1023, 1025), (40000 // 8 + 3, 40000 // 4), (0, 0)]
    sets = (shard, [(0, m) for m in numel], [None] * 5, [(5, 5), (44999, 45000), None, (33791, 39999), None], [(1023, 59000), (2047, 2049), (1025, 35999), (1, 2), None])
    given = hip.compress_tensors_each(new, USER_NAMES, segment_log=15, strides=USER_STRIDES)
    assert given.strides == USER_STRIDES and given.transforms == USER_NAMES
    auto = hip.compress_tensors_each(new, "auto", segment_log=15, strides=(1, 2, 3, 4))
    assert auto.transforms[0] == "pred" and auto.strides[0] == 2 and len(auto.strides) == 5, "the stereo walk finds its channel count"
    predicted = hip.compress_tensors_segmented([new[1], new[1][:1000]], 15, api.PredictedPlanes(0, stride=3))
    assert predicted.predictor == "prev3"
    reopened = hip.open_archive(hip.archive_tensors(given))
    assert reopened.strides == USER_STRIDES and reopened.segment_log == 15
    again = hip.open_archive(hip.archive_tensors(predicted))
    assert again.predictor == "prev3"
    plain = hip.compress_tensors_each(new, ["pred", "plain", "pred", "pred", "plain"], segment_log=15)          # everything the _each call takes: stride 1 everywhere
    for obj in (given, auto, reopened, plain):
        whole = hip.decompress_tensors(obj)
        assert all(_bits(a, b) for a, b in zip(whole, new))
        for windows in sets:
            back = hip.decompress_tensor_windows_each_stride(obj, windows)
            assert len(back) == 5
            for t, w, b in zip(whole, windows, back):
                if w is None:
                    assert b is None
                    continue
                assert b.dtype == t.dtype and b.device == t.device and b.dim() == 1 and b.numel() == w[1] - w[0] and _bits(t.reshape(-1)[w[0]:w[1]], b)
    assert all(_bits(a, b) for a, b in zip(hip.decompress_tensor_windows_each(plain, shard), hip.decompress_tensor_windows_each_stride(plain, shard)) if a is not None)
    for obj in (predicted, again):
        for windows in ([(1025, 44000), (7, 999)], [(0, 45000), None], [(44999, 45000), (1, 2)], [(2047, 2049), (0, 3000)]):
            back = hip.decompress_tensor_windows_each_stride(obj, windows)
            for t, w, b in zip([new[1], new[1][:1000]], windows, back):
                assert (w is None and b is None) or _bits(t.reshape(-1)[w[0]:w[1]], b)
    assert _bits(api.decompress_tensor_windows_each_stride(given, shard)[0], new[0].reshape(-1)[shard[0][0]:shard[0][1]]), "the module-level function"
    # the calls without _stride keep refusing these objects
    for obj in (given, reopened, predicted, again):
        with pytest.raises(ValueError):
            hip.decompress_tensor_windows_each(obj, shard[:len(obj.dtypes)])
        with pytest.raises(ValueError):
            hip.decompress_tensor_windows(obj, shard[:len(obj.dtypes)])

"""Patching tensors with a stride per tensor on the device (FSEHIP_planes_split_window_each_stride_dbatch,
FSEHIP_tensor_patch_window_each_stride_dbatch and patch_tensor_windows_each_stride) against the library's own dedicated calls -- the strided
split of the whole tensor, the full compress with transforms and strides given, the _window_each_ siblings -- and the numpy model of
planes_window_each_stride_corpus.py.  Block-size id 0 with segLog 10 and 11: a few KB already make several segments, and a segment of 1024
bytes is exactly one run of the predicted planes.  Every array is longer than its contract and pre-filled: whatever the contract does not give
to a call must still hold the fill afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import planes_corpus as pc
import planes_each_corpus as pe
import planes_each_stride_corpus as pes
import planes_patch_corpus as ppc
import planes_seg_corpus as psc
import planes_window_corpus as pwc
import planes_window_each_stride_corpus as pws
from planes_corpus import GENERIC
from planes_each_corpus import PLAIN, PRED, SUB, XOR

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = pws.FILL, 64, -7
SEG_LOGS = (10, 11)
LEAD = 7                                                       # T[0] of the split test: guard bytes in front of the stage
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _i64(a):
    """python ints of 64 bits, signed or not, flattened: the bits are what counts"""
    flat = np.asarray(a, dtype=object).reshape(-1)
    return torch.from_numpy(np.array([int(x) % (1 << 64) for x in flat], dtype=np.uint64).view(np.int64)).cuda()


def _marked(n):
    return torch.full((n + 1,), MARK, dtype=torch.int64, device="cuda")


def _filled(n, content=None, shift=0):
    """n bytes (and a tail) of FILL that start `shift` bytes behind a 256-byte boundary, the first ones `content`"""
    t = torch.full((shift + n + TAIL,), FILL, dtype=torch.uint8, device="cuda")[shift:]
    if content is not None and len(content):
        t[:len(content)] = content if isinstance(content, torch.Tensor) else _dev(content)
    return t


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- 1: the split alone
def run_split(hip, tensors, bases, transforms, strides, windows, E, seg_log, T, shift=0, sibling=False):
    """-> (stage bytes with their tail, plane offsets, results).  strides None: a NULL d_strides.  sibling: FSEHIP_planes_split_window_each_dbatch"""
    n, sizes = len(tensors), [len(t) for t in tensors]
    S = _offsets(sizes)
    total, cap = int(S[-1]), int(T[-1])
    src = _filled(total, pc.cat(tensors), shift)
    base = None if bases is None else _filled(total, pc.cat(bases), (shift + 7) % 16)[:total]
    stage = _filled(cap, None, (5 * shift + 3) % 16)
    poff, sres = _marked(n * E + 1), _marked(n)
    kw = dict(stage_offsets=_i64(T), base=base, stage=stage, stage_capacity=cap, plane_offsets=poff, results=sres)
    tr = _filled(n, np.asarray(transforms, np.uint8))
    if sibling:
        hip.planes_split_window_each_dbatch(src[:total], S, _i64(windows), E, seg_log, tr[:n], **kw)
    else:
        st = None if strides is None else _filled(n, np.asarray(strides, np.uint8))[:n]
        hip.planes_split_window_each_stride_dbatch(src[:total], S, _i64(windows), E, seg_log, tr[:n], st, **kw)
    torch.cuda.synchronize()
    assert int(poff[n * E + 1]) == MARK and int(sres[n]) == MARK
    assert (src.cpu().numpy()[:total] == pc.cat(tensors)).all() and (base is None or (base.cpu().numpy() == pc.cat(bases)).all()), "the inputs are only read"
    return stage.cpu().numpy(), poff.cpu().tolist()[:n * E + 1], sres.cpu().tolist()[:n]


def check_stage(got, model, T):
    stage, P, res = got
    want, written, mP, mres = model
    cap = len(want)
    assert P == mP and res == mres
    bad = np.nonzero(written & (stage[:cap] != want))[0]
    assert bad.size == 0, ("staged bytes that differ", bad[:8], [i for i in range(len(T) - 1) if T[i] <= bad[0] < T[i + 1]])
    assert (stage[:cap][~written] == FILL).all() and (stage[cap:] == FILL).all(), "nothing outside the staged planes is written: the guard bytes survive"


def _split_corpus(E, seg_log):
    """the merge corpus of planes_window_each_stride_corpus.py with the stage offsets of its windows from LEAD on"""
    c = pws.merge_corpus(E)
    sizes = [len(t) for t in c["tensors"]]
    c["T"] = [LEAD + x for x in ppc.stage_offsets(sizes, c["windows"], E, seg_log)]
    return c


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_window_each_stride_against_the_model_and_the_whole_split(hip, E):
    seg_log = 10
    c = _split_corpus(E, seg_log)
    tensors, bases, transforms, strides, windows, T = c["tensors"], c["bases"], c["transforms"], c["strides"], c["windows"], c["T"]
    n = len(tensors)
    # the mixed batch against the model, whose bytes are the segments of the planes of transform(WHOLE tensor)
    model = pws.stage_model(tensors, windows, E, seg_log, transforms, strides, bases, stage_off=T)
    assert min(model[3]) >= 0 and max(model[3]) > 2 * pc.TILE
    got = run_split(hip, tensors, bases, transforms, strides, windows, E, seg_log, T, shift=3)
    check_stage(got, model, T)
    # the staged bytes are segments k0 .. k1 of what FSEHIP_planes_split_each_stride_dbatch writes for the WHOLE tensors
    S = [int(x) for x in _offsets([len(t) for t in tensors])]
    planes, poff, pres = hip.planes_split_each_stride_dbatch(_dev(pc.cat(tensors)), np.asarray(S, np.uint64), E, _dev(transforms), _dev(strides), _dev(pc.cat(bases)))
    torch.cuda.synchronize()
    assert pres.cpu().tolist() == [len(t) for t in tensors]
    whole, PO = planes.cpu().numpy(), poff.cpu().tolist()
    stage, P, res = got
    for i, (t, (a, b)) in enumerate(zip(tensors, windows)):
        at, m = ppc.sub_range(len(t), a, b, E, seg_log)
        assert res[i] == m
        for p in range(E):
            lo, size = PO[i * E + p] + at // E, pc.plane_size(m, p, E)
            assert P[i * E + p + 1] - P[i * E + p] == size
            assert (stage[P[i * E + p]:P[i * E + p] + size] == whole[lo:lo + size]).all(), (i, p)
    # d_strides NULL and all ones: byte for byte the sibling -- stage, plane offsets and results
    old = run_split(hip, tensors, bases, transforms, None, windows, E, seg_log, T, shift=5, sibling=True)
    for st in (None, [1] * n):
        new = run_split(hip, tensors, bases, transforms, st, windows, E, seg_log, T, shift=5)
        assert new[1] == old[1] and new[2] == old[2] and (new[0] == old[0]).all()
    assert (old[0] != stage).any()


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_window_each_stride_refusals(hip, E):
    """rule 1 with its new cause, for that tensor alone: a PRED tensor whose stride byte is 0, 9 or 0xFF; the byte of another transform is not read"""
    seg_log = 10
    s = 1 << seg_log
    rng = np.random.default_rng(140 + E)
    sizes = [E * (2 * s + 9) + E - 1, E * s, E * (3 * s + 5), 5 * E, E * (s + 1)]
    tensors = [rng.integers(0, 256, x, dtype=np.uint8) for x in sizes]
    bases = [rng.integers(0, 256, x, dtype=np.uint8) for x in sizes]
    transforms, strides = [PRED, SUB, PRED, XOR, PLAIN], [3, 0, 8, 9, 0xFF]
    windows = [(s + 5, 2 * s + 9), (3, 9), (1023, 2 * s + 1), (0, 5), (s, s + 1)]
    T = [11 + x for x in ppc.stage_offsets(sizes, windows, E, seg_log)]
    good = pws.stage_model(tensors, windows, E, seg_log, transforms, strides, bases, stage_off=T)
    assert min(good[3]) > 0
    check_stage(run_split(hip, tensors, bases, transforms, strides, windows, E, seg_log, T), good, T)
    for k in (0, 2):
        for bad in (0, 9, 0xFF):
            st = [bad if i == k else x for i, x in enumerate(strides)]
            got = run_split(hip, tensors, bases, transforms, st, windows, E, seg_log, T)
            check_stage(got, pws.stage_model(tensors, windows, E, seg_log, transforms, st, bases, stage_off=T), T)
            assert got[2] == good[3][:k] + [GENERIC] + good[3][k + 1:] and got[1][k * E:(k + 1) * E] == [T[k]] * E
    got = run_split(hip, tensors, None, transforms, strides, windows, E, seg_log, T)
    check_stage(got, pws.stage_model(tensors, windows, E, seg_log, transforms, strides, None, stage_off=T), T)
    assert got[2] == [good[3][0], GENERIC, good[3][2], GENERIC, good[3][4]]


# ---------------------------------------------------------------------------------------------------------------- 2: the composite
TRANSFORMS = [PRED, PLAIN, SUB, XOR, PLAIN, PRED, PRED, XOR]
STRIDES = [3, 0xFF, 0, 9, 1, 2, 5, 0]                          # (read for the PRED tensors alone)


def _corpus(E, seg_log, seed=0):
    """(old, fresh, bases) for TRANSFORMS: three interleaved walks over two segments and a bit (PRED at 3), nothing, noise of exactly one
    segment per plane (SUB), three symbols in turn, of a size that is no multiple of E (XOR), a skewed source of two segments and a half per
    plane (PLAIN), fewer bytes than an element, a skewed source of three segments and five elements (PRED at 5: compressed blocks in every
    segment), two segments of a slow walk (XOR); `fresh` differs from `old` everywhere and is as compressible; the bases differ from `old` in
    a byte in sixteen"""
    key = ("corpus", E, seg_log, seed)
    if key not in _CACHE:
        s = 1 << seg_log
        rng = np.random.default_rng(260 + E + seg_log + 1000 * seed)
        walk = (np.cumsum(rng.integers(-2, 3, 2 * s)) + 500).astype("<u8")
        old = [pws._smooth(rng, 2 * s + 100, E, 3), np.zeros(0, np.uint8), rng.integers(0, 256, E * s, dtype=np.uint8),
               (77 + np.arange(E * (s + 1) + E - 1) % 3).astype(np.uint8), rng.integers(0, 4, 5 * E * s // 2, dtype=np.uint8),
               rng.integers(0, 256, E - 1, dtype=np.uint8), rng.integers(0, 4, E * (3 * s + 5), dtype=np.uint8),
               np.ascontiguousarray(walk.view(np.uint8).reshape(-1, 8)[:, :E]).reshape(-1)]
        fresh = [pws._smooth(rng, 2 * s + 100, E, 3)] + [t ^ rng.integers(1, 4, t.size, dtype=np.uint8) for t in old[1:]]
        bases = [t ^ (rng.integers(1, 256, t.size, dtype=np.uint8) * (rng.integers(0, 16, t.size) == 0)).astype(np.uint8) for t in old]
        _CACHE[key] = (old, fresh, bases)
    return _CACHE[key]


def _changed(old, fresh, windows, E):
    """old with the elements [a, b) of every tensor taken from fresh: it differs from old inside the windows only"""
    new = [t.copy() for t in old]
    for t, f, (a, b) in zip(new, fresh, windows):
        t[a * E:b * E] = f[a * E:b * E]
    return new


def _codec(form):
    from finitestateentropy_amd.api import AutoCodec
    return {"fse": 0, "huf": 1, "given": 0, "chosen": AutoCodec(20)}[form]


def _given(nseg):
    return [(q // 3) % 2 for q in range(nseg)]


def compress(hip, tensors, bases, E, seg_log, form, align_log, strides=STRIDES, each=False):
    """tensor_compress_seg_each_stride_dbatch with transforms and strides GIVEN -> (frames cut to their total, frame offsets, frame results, codecs
    or None).  strides None: a NULL d_strides; each: tensor_compress_seg_each_dbatch"""
    sizes = [len(t) for t in tensors]
    S = _offsets(sizes)
    first = psc.seg_first(sizes, E, seg_log)
    codecs = _dev(_given(first[-1])) if form == "given" else None
    kw = dict(seg_first=np.asarray(first, np.uint64), codec=_codec(form), codecs=codecs, block_size_id=0, align_log=align_log)
    src, base = _dev(pc.cat(tensors)), None if bases is None else _dev(pc.cat(bases))
    if each:
        got = hip.tensor_compress_seg_each_dbatch(src, S, E, seg_log, list(TRANSFORMS), base, **kw)
    else:
        got = hip.tensor_compress_seg_each_stride_dbatch(src, S, E, seg_log, list(TRANSFORMS), None if strides is None else _dev(strides), base, **kw)
    dst, foff, fres, tres, chosen = got[:5]
    torch.cuda.synchronize()
    st = [1] * len(sizes) if each or strides is None else strides
    assert tres.cpu().tolist() == [x if pes.accepted(tr, s, bases is not None) else GENERIC for x, tr, s in zip(sizes, TRANSFORMS, st)]
    return dst[:int(foff[-1])].clone(), foff, fres, chosen


def _first(hip, sizes, windows, E, seg_log):
    """FSEHIP_planes_windowFirst itself: (selFirst, blocks) -- and the model's"""
    n = len(sizes)
    off = (C.c_uint64 * (n + 1))(*[int(x) for x in _offsets(sizes)])
    win = (C.c_uint64 * (2 * n))(*[int(x) for w in windows for x in w])
    sel, blocks = (C.c_uint64 * (n * E + 1))(), C.c_size_t(0)
    f = hip.lib.FSEHIP_planes_windowFirst
    f.restype = C.c_size_t
    r = f(sel, C.byref(blocks), off, win, C.c_size_t(n), C.c_uint(E), C.c_uint(seg_log), C.c_uint(0))
    assert r == sel[n * E] and (list(sel), blocks.value) == tuple(pwc.window_first(sizes, windows, E, seg_log))
    return list(sel), blocks.value


def run_patch(hip, obj, tensors, bases, windows, E, seg_log, form, align_log, strides=STRIDES, shift=0, sibling=False):
    """the composite with every array marked; nSelected and the block promise those of FSEHIP_planes_windowFirst, the stage exactly the bytes the
    stage-offset arithmetic gives: -> (out, out offsets, out results, tensor results, out codecs, out capacity).  strides None: a NULL
    d_strides; sibling: tensor_patch_window_each_dbatch on the same arguments"""
    frames, foff, fres, codecs = obj
    n, sizes = len(tensors), [len(t) for t in tensors]
    S = _offsets(sizes)
    total = int(S[-1])
    nseg = fres.numel()
    sel, blocks = _first(hip, sizes, windows, E, seg_log)
    nsel = sel[-1]
    T = ppc.stage_offsets(sizes, windows, E, seg_log)
    src = _filled(total, pc.cat(tensors), shift)[:total]
    base = None if bases is None else _filled(total, pc.cat(bases), (shift + 5) % 16)[:total]
    new_cap = hip.frame_packed_bound(int(T[-1]), nsel, blocks, align_log)
    cap = frames.numel() + new_cap
    out = _filled(cap, None, (3 * shift + 1) % 16)
    stage, fresh = _filled(int(T[-1]), None, (shift + 9) % 16), _filled(new_cap)
    ooff, ores, tres, spo, sso, sres, noff, nres = (_marked(nseg + 1), _marked(nseg), _marked(n), _marked(n * E + 1), _marked(nsel + 1), _marked(n), _marked(nsel + 1),
                                                    _marked(nsel))
    ocod = None if codecs is None else _filled(nseg)
    new_codecs = _dev([_given(nseg)[q] for q in ppc.selected_frames(sizes, windows, E, seg_log)]) if form == "given" else None
    before = frames.clone()
    tr = _filled(n, np.asarray(TRANSFORMS, np.uint8))
    kw = dict(sel_first=np.asarray(sel, np.uint64), stage_offsets=np.asarray(T, np.uint64), base=base, codec=_codec(form), codecs=codecs, new_codecs=new_codecs,
              block_size_id=0, align_log=align_log, out=out, out_capacity=cap, out_offsets=ooff, out_results=ores, out_codecs=ocod, tensor_results=tres, stage=stage,
              stage_capacity=int(T[-1]), stage_plane_offsets=spo, stage_seg_offsets=sso, stage_results=sres, new_frames=fresh, new_capacity=new_cap, new_offsets=noff,
              new_results=nres, max_total_blocks=blocks, seg_first=np.asarray(psc.seg_first(sizes, E, seg_log), np.uint64))
    if sibling:
        hip.tensor_patch_window_each_dbatch(frames, foff, fres, src, S, windows, E, seg_log, tr[:n], **kw)
    else:
        st = None if strides is None else _filled(n, np.asarray(strides, np.uint8))[:n]
        hip.tensor_patch_window_each_stride_dbatch(frames, foff, fres, src, S, windows, E, seg_log, tr[:n], st, **kw)
    torch.cuda.synchronize()
    assert int(ooff[nseg + 1]) == MARK and int(ores[nseg]) == MARK and int(tres[n]) == MARK and torch.equal(frames, before)
    assert int(spo[n * E + 1]) == MARK and int(sso[nsel + 1]) == MARK and int(sres[n]) == MARK and int(noff[nsel + 1]) == MARK and int(nres[nsel]) == MARK
    assert bool((stage[int(T[-1]):] == FILL).all()) and bool((fresh[new_cap:] == FILL).all()) and bool((out[cap:] == FILL).all())
    assert ocod is None or set(ocod.cpu().tolist()[nseg:]) == {FILL}
    return out, ooff[:nseg + 1], ores[:nseg], tres.cpu().tolist()[:n], None if ocod is None else ocod[:nseg], cap


def same_object(got, full, what):
    """offsets, results, codecs and every frame byte; behind the frames' real bytes the patch's output holds its fill"""
    out, ooff, ores, _, ocod, _ = got
    frames, foff, fres, codecs = full
    assert torch.equal(ooff, foff) and torch.equal(ores, fres), what
    assert (ocod is None) == (codecs is None) and (ocod is None or torch.equal(ocod, codecs[:ocod.numel()])), what
    off, res = foff.cpu().tolist(), fres.cpu().tolist()
    a, b = out.cpu().numpy(), frames.cpu().numpy()
    written = np.zeros(len(a), bool)
    for q, r in enumerate(res):
        assert r >= 8 and (a[off[q]:off[q] + r] == b[off[q]:off[q] + r]).all(), (what, q)
        written[off[q]:off[q] + r] = True
    assert (a[~written] == FILL).all(), (what, "bytes outside the frames")


@pytest.mark.parametrize("form", ["fse", "huf", "given", "chosen"])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_patch_of_old_with_new_is_the_compress_of_new_for_every_boundary_window(hip, E, form):
    assert set(TRANSFORMS) == set(pe.IDS)
    for seg_log in SEG_LOGS:
        old, fresh, bases = _corpus(E, seg_log)
        sizes = [len(t) for t in old]
        S = _offsets(sizes)
        first = np.asarray(psc.seg_first(sizes, E, seg_log), np.uint64)
        objs = {align_log: compress(hip, old, bases, E, seg_log, form, align_log) for align_log in (0, 6)}
        cands = [pwc.boundary_windows(len(t) // E, seg_log) for t in old]
        starts, changed = set(), 0
        for rnd in range(max(len(c) for c in cands)):
            windows = [c[(rnd + 3 * i) % len(c)] for i, c in enumerate(cands)]
            align_log = (0, 6)[rnd % 2]
            new = _changed(old, fresh, windows, E)
            got = run_patch(hip, objs[align_log], new, bases, windows, E, seg_log, form, align_log, shift=rnd % 16)
            assert got[3] == sizes, (rnd, got[3])
            full = compress(hip, new, bases, E, seg_log, form, align_log)
            same_object(got, full, (E, form, seg_log, rnd))
            changed += not torch.equal(full[0], objs[align_log][0])
            starts |= {(st, a % 1024) for tr, st, (a, b) in zip(TRANSFORMS, STRIDES, windows) if tr == PRED and a < b}
            if rnd % 4 == 0:                                   # ... and it reads back as the new tensors
                back, res = hip.tensor_decompress_seg_each_stride_dbatch(got[0], got[1], S, E, seg_log, list(TRANSFORMS), _dev(STRIDES), _dev(pc.cat(bases)), first)
                torch.cuda.synchronize()
                assert res.cpu().tolist() == sizes and (back.cpu().numpy()[:int(S[-1])] == pc.cat(new)).all()
        assert changed > rnd // 2 and {(S_, L) for S_ in (3, 5) for L in (0, 1, 1023)} <= starts, "strided windows on a run start, one behind it, one in front of the next"
        # every element, and nothing selected: the full compress, and a copy of the object
        everything = [(0, len(t) // E) for t in old]
        new = _changed(old, fresh, everything, E)               # (the n mod E bytes behind the last whole element lie in no window)
        same_object(run_patch(hip, objs[0], new, bases, everything, E, seg_log, form, 0), compress(hip, new, bases, E, seg_log, form, 0), "everything")
        same_object(run_patch(hip, objs[6], fresh, bases, [(0, 0)] * len(old), E, seg_log, form, 6), objs[6], "nothing")


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_patch_with_null_strides_and_all_ones_is_the_sibling(hip, E):
    seg_log, form = 10, "huf"
    s = 1 << seg_log
    old, fresh, bases = _corpus(E, seg_log)
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s, s + 1), (s + 7, 2 * s + 9), (0, 0), (s + 5, 3 * s), (1023, s + 40)]
    new = _changed(old, fresh, windows, E)
    obj = compress(hip, old, bases, E, seg_log, form, 0, each=True)
    want = run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0, sibling=True)
    same_object(want, compress(hip, new, bases, E, seg_log, form, 0, each=True), "the sibling")
    for st in (None, [1] * 8, [1, 0, 9, 0xFF, 0, 1, 1, 7]):
        got = run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0, strides=st)
        assert got[3] == want[3] and all(torch.equal(x, y) for x, y in zip(got[:3], want[:3])), st
    assert not torch.equal(compress(hip, new, bases, E, seg_log, form, 0)[0], compress(hip, new, bases, E, seg_log, form, 0, each=True)[0]), "the strided object is another"


# ---------------------------------------------------------------------------------------------------------------- 3: refusals of one tensor
@pytest.mark.parametrize("E", pc.ELEMS)
def test_patch_each_stride_refuses_a_tensor_whole_and_patches_the_others(hip, E):
    """a PRED tensor whose stride byte is 0 or 9: GENERIC for it alone, it keeps ALL its old frames, its neighbours are patched"""
    seg_log, form = 10, "huf"
    s = 1 << seg_log
    old, fresh, bases = _corpus(E, seg_log)
    sizes = [len(t) for t in old]
    n = len(sizes)
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s, s + 1), (s + 7, 2 * s + 9), (0, 0), (s + 5, 3 * s), (1023, s + 40)]
    new = _changed(old, fresh, windows, E)
    obj = compress(hip, old, bases, E, seg_log, form, 0)
    same_object(run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0), compress(hip, new, bases, E, seg_log, form, 0), "nothing refused")
    for k in (0, 6):
        kept = compress(hip, [old[i] if i == k else new[i] for i in range(n)], bases, E, seg_log, form, 0)      # the full compress of: new, but the victim as it was
        for bad in (0, 9):
            st = [bad if i == k else x for i, x in enumerate(STRIDES)]
            got = run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0, strides=st)
            assert got[3] == [GENERIC if i == k else sizes[i] for i in range(n)], (k, bad, got[3])
            same_object(got, kept, (k, bad))
    # no base: the XOR and SUB tensors alone
    victims = tuple(i for i, tr in enumerate(TRANSFORMS) if tr >= XOR)
    got = run_patch(hip, obj, new, None, windows, E, seg_log, form, 0)
    assert got[3] == [GENERIC if i in victims else sizes[i] for i in range(n)]
    same_object(got, compress(hip, [old[i] if i in victims else new[i] for i in range(n)], bases, E, seg_log, form, 0), "no base")


# ---------------------------------------------------------------------------------------------------------------- 4: one captured graph
def test_patch_each_stride_composite_in_one_hip_graph(hip):
    """one captured graph -- a single stream, a linear chain -- holding tensor_patch_window_each_stride_dbatch; replayed twice after the tensors and
    the old object were changed (the sizes, the windows' counts and with them every launch size stay)"""
    E, seg_log, form, ALIGN = 2, 10, "fse", 6
    s = 1 << seg_log
    both = [_corpus(E, seg_log, seed) for seed in (0, 1)]
    sizes = [len(t) for t in both[0][0]]
    assert sizes == [len(t) for t in both[1][0]]
    n, S = len(sizes), _offsets(sizes)
    total = int(S[-1])
    first = psc.seg_first(sizes, E, seg_log)
    nseg = first[-1]
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s - 1, s + 1), (s + 7, 2 * s + 9), (0, 0), (s + 5, 3 * s + 2), (1023, s + 40)]
    sel, blocks = _first(hip, sizes, windows, E, seg_log)
    nsel = sel[-1]
    T = ppc.stage_offsets(sizes, windows, E, seg_log)
    objs = [compress(hip, both[k][0], both[k][2], E, seg_log, form, ALIGN) for k in (0, 1)]
    room = max(o[0].numel() for o in objs) + 64
    frames = torch.zeros(room, dtype=torch.uint8, device="cuda")
    foff, fres = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda"), torch.zeros(nseg, dtype=torch.int64, device="cuda")
    wsize = hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize
    wsize.restype = C.c_size_t
    ws = torch.empty(int(wsize(C.c_size_t(nsel), C.c_size_t(blocks), C.c_uint(0), C.c_int(0))), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(hip.planes_splice_scratch_bound(n, E, nseg), dtype=torch.uint8, device="cuda")
    new_cap = hip.frame_packed_bound(T[-1], nsel, blocks, ALIGN)
    out_cap = room + new_cap
    src, base = torch.zeros(total, dtype=torch.uint8, device="cuda"), torch.zeros(total, dtype=torch.uint8, device="cuda")
    soff, sf, wf, toff, win, tr, st = _i64(S), _i64(first), _i64(sel), _i64(T), _i64(windows), _dev(TRANSFORMS), _dev(STRIDES)
    out, stage, fresh = _filled(out_cap), _filled(T[-1]), _filled(new_cap)
    ooff, noff, sso = (torch.zeros(k + 1, dtype=torch.int64, device="cuda") for k in (nseg, nsel, nsel))
    ores, nres = torch.zeros(nseg, dtype=torch.int64, device="cuda"), torch.zeros(nsel, dtype=torch.int64, device="cuda")
    spo = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda")
    tres, sres = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")

    def work():
        hip.tensor_patch_window_each_stride_dbatch(frames, foff, fres, src, soff, win, E, seg_log, tr, st, sf, n_segments=nseg, sel_first=wf, n_selected=nsel,
                                                   stage_offsets=toff, base=base, codec=0, block_size_id=0, max_total_blocks=blocks, align_log=ALIGN, frames_capacity=room,
                                                   out=out, out_capacity=out_cap, out_offsets=ooff, out_results=ores, tensor_results=tres, stage=stage, stage_capacity=T[-1],
                                                   stage_plane_offsets=spo, stage_seg_offsets=sso, stage_results=sres, new_frames=fresh, new_capacity=new_cap,
                                                   new_offsets=noff, new_results=nres, scratch=scratch, workspace=ws)

    def load(k):
        """the old object of corpus k, and its tensors changed inside the windows"""
        new = _changed(both[k][0], both[k][1], windows, E)
        src.copy_(_dev(pc.cat(new))); base.copy_(_dev(pc.cat(both[k][2])))
        frames.zero_()
        frames[:objs[k][0].numel()] = objs[k][0]
        foff.copy_(objs[k][1]); fres.copy_(objs[k][2])
        return new
    load(0); work(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    outs = []
    for k in (1, 0):
        new = load(k)
        out.fill_(FILL)
        for t in (ooff, ores, tres):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert tres.cpu().tolist() == sizes
        same_object((out, ooff, ores, None, None, out_cap), compress(hip, new, both[k][2], E, seg_log, form, ALIGN), k)
        outs.append(out.cpu().numpy())
    assert not (outs[0] == outs[1]).all()


# ---------------------------------------------------------------------------------------------------------------- 5: the user-facing call
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_patch_tensor_windows_each_stride(hip):
    import finitestateentropy_amd.api as api
    from test_gpu_planes_window_each_stride import USER_NAMES, USER_STRIDES, user_tensors
    old = user_tensors()
    windows = [(60000 // 8 + 1, 60000 // 4), (44999, 45000), None, (1023, 2050), (0, 0)]
    new = [t.clone() for t in old]
    new[0].view(-1)[7501:15000] += 3
    new[1].view(-1)[44999] = 1.5
    new[3].view(-1)[1023:2050] += 7
    kw = dict(segment_log=10, block_size_id=0)
    cases = [("given", lambda t: hip.compress_tensors_each(t, USER_NAMES, strides=USER_STRIDES, **kw)),
             ("chosen codecs", lambda t: hip.compress_tensors_each(t, USER_NAMES, codec=api.AutoCodec(20), strides=USER_STRIDES, **kw)),
             ("stride 1 everywhere", lambda t: hip.compress_tensors_each(t, USER_NAMES, **kw)),
             ("predicted at 3", lambda t: hip.compress_tensors_segmented([t[1]], 10, api.PredictedPlanes(0, stride=3), block_size_id=0))]
    for name, write in cases:
        single = name.startswith("predicted")
        ts, ws = ([new[1]], [windows[1]]) if single else (new, windows)
        obj = write(old)
        for what, o in ((name, obj), (name + ", reopened", hip.open_archive(hip.archive_tensors(obj)))):
            snap = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in g.items()} for g in o.groups]
            got = hip.patch_tensor_windows_each_stride(o, ts, ws)
            want = write(new)
            assert got is not o and got.segment_log == 10 and got.block_size_id == 0 and got.codec == o.codec, what
            assert got.transforms == o.transforms == want.transforms and got.predictor == o.predictor == want.predictor, what
            assert getattr(got, "strides", None) == getattr(o, "strides", None) == getattr(want, "strides", None), what
            for g, w, og, sn in zip(got.groups, want.groups, o.groups, snap):
                assert g["index"] == w["index"] and g["sizes"] == w["sizes"] and [int(x) for x in g["seg_first"]] == [int(x) for x in w["seg_first"]]
                for k in ("frames", "frame_offsets", "frame_results", "tensor_results") + (("codecs",) if "codecs" in w else ()):
                    assert torch.equal(g[k], w[k]), (what, g["elem_bytes"], k)
                    assert torch.equal(og[k], sn[k]) and g[k].data_ptr() != og[k].data_ptr(), "the object given is left as it is, the new one shares nothing with it"
            assert all(_bits(x, y) for x, y in zip(ts, hip.decompress_tensors(got))), what
            back = hip.decompress_tensor_windows_each_stride(got, [(44990, 45000)] if single else [(7490, 15010), (44990, 45000), (3, 9), (0, 3000), None])
            assert _bits(back[0], ts[0].view(-1)[44990:45000] if single else new[0].view(-1)[7490:15010]), what
            assert single or (_bits(back[1], new[1].view(-1)[44990:45000]) and _bits(back[2], new[2].view(-1)[3:9]) and _bits(back[3], new[3][:3000]) and back[4] is None)
            again = hip.open_archive(hip.archive_tensors(got))
            assert getattr(again, "strides", None) == getattr(got, "strides", None) and again.predictor == got.predictor, what
            assert all(_bits(x, y) for x, y in zip(ts, hip.decompress_tensors(again))), what
    given = cases[0][1](old)
    assert given.strides == USER_STRIDES
    assert _bits(api.decompress_tensors(api.patch_tensor_windows_each_stride(given, new, windows))[0], new[0]), "the module-level function"
    # the calls without _stride keep refusing these objects
    predicted = cases[3][1](old)
    for o, t, w in ((given, new, windows), (predicted, [new[1]], [windows[1]])):
        with pytest.raises(ValueError):
            hip.patch_tensor_windows_each(o, t, w)
        with pytest.raises(ValueError, match="patches are not supported"):
            hip.patch_tensor_windows(o, t, w)

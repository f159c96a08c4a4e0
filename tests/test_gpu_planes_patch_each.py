"""Patching tensors with a transform per tensor on the device (FSEHIP_planes_split_window_each_dbatch, FSEHIP_tensor_patch_window_each_dbatch and
patch_tensor_windows_each) against the library's own dedicated calls -- the window split with one op, the predicted split of the whole tensor,
the full compress with the transforms given -- and the numpy model of planes_patch_each_corpus.py.  Block-size id 0 with segLog 10 and 11: a few
KB already make several segments, and a segment of 1024 bytes is exactly one run of the predicted planes.  Every array is longer than its
contract and pre-filled: whatever the contract does not give to a call must still hold the fill afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import planes_corpus as pc
import planes_each_corpus as pe
import planes_patch_corpus as ppc
import planes_patch_each_corpus as ppe
import planes_seg_corpus as psc
import planes_window_corpus as pwc
from planes_corpus import CORRUPT, GENERIC, TOO_SMALL
from planes_each_corpus import PLAIN, PRED, SUB, XOR

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = ppe.FILL, 64, -7
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


def _filled(n, content=None, shift=0):
    """n bytes (and a tail) of FILL that start `shift` bytes behind a 256-byte boundary, the first ones `content`"""
    t = torch.full((shift + n + TAIL,), FILL, dtype=torch.uint8, device="cuda")[shift:]
    if content is not None and len(content):
        t[:len(content)] = content if isinstance(content, torch.Tensor) else _dev(content)
    return t


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- 1: the split alone
def run_split(hip, tensors, bases, transforms, windows, E, seg_log, T, shift=0, stage_cap=None, capacity=None, old_op=None):
    """-> (stage bytes with their tail, plane offsets, results).  old_op None: the new call; "plain" / 0 / 1: FSEHIP_planes_split_window(_op)_dbatch
    on the same arguments, without a base, with XOR, with SUB"""
    n, sizes = len(tensors), [len(t) for t in tensors]
    S = _offsets(sizes)
    total = int(S[-1])
    cap = int(T[-1]) if stage_cap is None else stage_cap
    src = _filled(total, pc.cat(tensors), shift)
    base = None if bases is None else _filled(total, pc.cat(bases), (shift + 7) % 16)[:total]
    stage = _filled(cap, None, (5 * shift + 3) % 16)
    poff, sres = _marked(n * E + 1), _marked(n)
    kw = dict(stage_offsets=_i64(T), capacity=capacity, stage=stage, stage_capacity=cap, plane_offsets=poff, results=sres)
    if old_op is None:
        tr = _filled(n, np.asarray(transforms, np.uint8))
        hip.planes_split_window_each_dbatch(src[:total], S, _i64(windows), E, seg_log, tr[:n], base=base, **kw)
    else:
        hip.planes_split_window_dbatch(src[:total], S, _i64(windows), E, seg_log, base=None if old_op == "plain" else base, delta_op=0 if old_op == "plain" else old_op, **kw)
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


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_window_each_against_the_model_and_the_dedicated_calls(hip, E):
    seg_log = 10
    c = ppe.split_corpus(E, seg_log)
    missing = [name for name, held in ppe.shapes(c, E, seg_log).items() if not held]
    assert not missing, missing
    tensors, bases, transforms, windows, T = c["tensors"], c["bases"], c["transforms"], c["windows"], c["T"]
    n = len(tensors)
    # the mixed batch against the model, whose bytes are the segments of the planes of transform(WHOLE tensor)
    model = ppe.stage_each_model(tensors, windows, E, seg_log, transforms, bases, stage_off=T)
    assert min(model[3]) >= 0
    check_stage(run_split(hip, tensors, bases, transforms, windows, E, seg_log, T, shift=3), model, T)
    # without a base: the XOR and SUB tensors are refused alone, their entries collapse, nothing of them is staged
    model = ppe.stage_each_model(tensors, windows, E, seg_log, transforms, None, stage_off=T)
    refused = [i for i in range(n) if transforms[i] >= XOR]
    assert refused and [model[3][i] for i in refused] == [GENERIC] * len(refused)
    check_stage(run_split(hip, tensors, None, transforms, windows, E, seg_log, T, shift=9), model, T)
    # all PLAIN, all XOR, all SUB: byte for byte FSEHIP_planes_split_window_op_dbatch -- stage, plane offsets and results
    for tr, op in ((PLAIN, "plain"), (XOR, 0), (SUB, 1)):
        new = run_split(hip, tensors, bases, [tr] * n, windows, E, seg_log, T, shift=5)
        old = run_split(hip, tensors, bases, None, windows, E, seg_log, T, shift=5, old_op=op)
        assert new[1] == old[1] and new[2] == old[2] and (new[0] == old[0]).all(), tr
    # all PRED: the segment slices of FSEHIP_planes_split_pred_dbatch of the WHOLE tensors
    S = [int(x) for x in _offsets([len(t) for t in tensors])]
    planes, poff, pres = hip.planes_split_pred_dbatch(_dev(pc.cat(tensors)), np.asarray(S, np.uint64), E)
    torch.cuda.synchronize()
    assert pres.cpu().tolist() == [len(t) for t in tensors]
    whole, PO = planes.cpu().numpy(), poff.cpu().tolist()
    stage, P, res = run_split(hip, tensors, None, [PRED] * n, windows, E, seg_log, T, shift=1)
    for i, (t, (a, b)) in enumerate(zip(tensors, windows)):
        at, m = ppc.sub_range(len(t), a, b, E, seg_log)
        assert res[i] == m
        for p in range(E):
            lo, size = PO[i * E + p] + at // E, pc.plane_size(m, p, E)
            assert P[i * E + p + 1] - P[i * E + p] == size
            assert (stage[P[i * E + p]:P[i * E + p] + size] == whole[lo:lo + size]).all(), (i, p)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_window_each_refusals(hip, E):
    """rule 1 with its new cause, each for that tensor alone: a byte 0xFF, XOR / SUB without a base, a > b, b beyond the tensor, a pair of stage
    offsets that does not hold the sub-tensor, a stage and a source capacity that cut a tensor off"""
    seg_log = 10
    s = 1 << seg_log
    rng = np.random.default_rng(40 + E)
    sizes = [E * (2 * s + 9) + E - 1, E * s, E * (3 * s + 5), 5 * E, E * (s + 1)]
    tensors = [rng.integers(0, 256, x, dtype=np.uint8) for x in sizes]
    bases = [rng.integers(0, 256, x, dtype=np.uint8) for x in sizes]
    transforms = [PRED, SUB, PRED, XOR, PLAIN]
    windows = [(s + 5, 2 * s + 9), (3, 9), (1023, 2 * s + 1), (0, 5), (s, s + 1)]
    T = [11 + x for x in ppc.stage_offsets(sizes, windows, E, seg_log)]
    good = ppe.stage_each_model(tensors, windows, E, seg_log, transforms, bases, stage_off=T)
    assert min(good[3]) > 0
    check_stage(run_split(hip, tensors, bases, transforms, windows, E, seg_log, T), good, T)

    def alone(k, got, model):
        check_stage(got, model, T)
        assert got[2] == good[3][:k] + [GENERIC] + good[3][k + 1:] and got[1][k * E:(k + 1) * E] == [T[k]] * E
    for k in (0, 1, 4):
        tr = list(transforms)
        tr[k] = 0xFF if k != 4 else 4
        alone(k, run_split(hip, tensors, bases, tr, windows, E, seg_log, T), ppe.stage_each_model(tensors, windows, E, seg_log, tr, bases, stage_off=T))
    got = run_split(hip, tensors, None, transforms, windows, E, seg_log, T)
    check_stage(got, ppe.stage_each_model(tensors, windows, E, seg_log, transforms, None, stage_off=T), T)
    assert got[2] == [good[3][0], GENERIC, good[3][2], GENERIC, good[3][4]]
    for k, bad in ((0, (s + 6, s + 5)), (2, (1023, 3 * s + 6)), (2, (1 << 63, 1 << 63))):
        w = list(windows)
        w[k] = bad
        alone(k, run_split(hip, tensors, bases, transforms, w, E, seg_log, T), ppe.stage_each_model(tensors, w, E, seg_log, transforms, bases, stage_off=T))
    wrong = [t + (1 if i > 2 else 0) for i, t in enumerate(T)]                                     # tensor 2 has a byte too many, the ones behind it are moved
    got = run_split(hip, tensors, bases, transforms, windows, E, seg_log, wrong, stage_cap=wrong[-1])
    check_stage(got, ppe.stage_each_model(tensors, windows, E, seg_log, transforms, bases, stage_off=wrong, stage_cap=wrong[-1]), wrong)
    assert got[2] == good[3][:2] + [GENERIC] + good[3][3:]
    got = run_split(hip, tensors, bases, transforms, windows, E, seg_log, T, stage_cap=T[-1] - 1)
    check_stage(got, ppe.stage_each_model(tensors, windows, E, seg_log, transforms, bases, stage_off=T, stage_cap=T[-1] - 1), T)
    assert got[2] == good[3][:-1] + [GENERIC]
    got = run_split(hip, tensors, bases, transforms, windows, E, seg_log, T, capacity=sum(sizes) - 1)
    check_stage(got, ppe.stage_each_model(tensors, windows, E, seg_log, transforms, bases, stage_off=T, capacity=sum(sizes) - 1), T)
    assert got[2] == good[3][:-1] + [GENERIC]


# ---------------------------------------------------------------------------------------------------------------- 2: the composite
TRANSFORMS = [PRED, PLAIN, SUB, XOR, PLAIN, PRED, PRED, XOR]


def _corpus(E, seg_log, seed=0):
    """(old, fresh, bases) for TRANSFORMS: compressible bf16 data over two segments and a bit (PRED), nothing, noise of exactly one segment per plane
    (SUB), three symbols in turn, of a size that is no multiple of E (XOR), a skewed source of two segments and a half per plane (PLAIN), fewer bytes
    than an element, a skewed source of three segments and five elements (PRED: compressed blocks in every segment), two segments of a slow walk
    (XOR); `fresh` differs from `old` everywhere and is as compressible; the bases differ from `old` in a byte in sixteen"""
    key = ("corpus", E, seg_log, seed)
    if key not in _CACHE:
        s = 1 << seg_log
        rng = np.random.default_rng(60 + E + seg_log + 1000 * seed)
        walk = (np.cumsum(rng.integers(-2, 3, 2 * s)) + 500).astype("<u8")
        old = [pc.bf16_gaussian(E * (2 * s + 100) // 2, 5 + E + seed), np.zeros(0, np.uint8), rng.integers(0, 256, E * s, dtype=np.uint8),
               (77 + np.arange(E * (s + 1) + E - 1) % 3).astype(np.uint8), rng.integers(0, 4, 5 * E * s // 2, dtype=np.uint8),
               rng.integers(0, 256, E - 1, dtype=np.uint8), rng.integers(0, 4, E * (3 * s + 5), dtype=np.uint8),
               np.ascontiguousarray(walk.view(np.uint8).reshape(-1, 8)[:, :E]).reshape(-1)]
        fresh = [pc.bf16_gaussian(E * (2 * s + 100) // 2, 9 + E + seed)] + [t ^ rng.integers(1, 4, t.size, dtype=np.uint8) for t in old[1:]]
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


def compress(hip, tensors, bases, E, seg_log, form, align_log, transforms=TRANSFORMS):
    """tensor_compress_seg_each_dbatch with the transforms GIVEN -> (frames cut to their total, frame offsets, frame results, codecs or None)"""
    sizes = [len(t) for t in tensors]
    S = _offsets(sizes)
    first = psc.seg_first(sizes, E, seg_log)
    codecs = _dev(_given(first[-1])) if form == "given" else None
    dst, foff, fres, tres, chosen, _ = hip.tensor_compress_seg_each_dbatch(_dev(pc.cat(tensors)), S, E, seg_log, list(transforms), None if bases is None else _dev(pc.cat(bases)),
                                                                           seg_first=np.asarray(first, np.uint64), codec=_codec(form), codecs=codecs, block_size_id=0,
                                                                           align_log=align_log)
    torch.cuda.synchronize()
    assert tres.cpu().tolist() == [x if pe.accepted(tr, bases is not None) else GENERIC for x, tr in zip(sizes, transforms)]
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


def run_patch(hip, obj, tensors, bases, windows, E, seg_log, form, align_log, transforms=TRANSFORMS, shift=0, sel=None, T=None, out_cap=None, **kw):
    """the composite with every array marked; nSelected and the block promise those of FSEHIP_planes_windowFirst, the stage exactly the bytes the
    stage-offset arithmetic gives: -> (out, out offsets, out results, tensor results, out codecs, out capacity)"""
    frames, foff, fres, codecs = obj
    n, sizes = len(tensors), [len(t) for t in tensors]
    S = _offsets(sizes)
    total = int(S[-1])
    nseg = fres.numel()
    sel, blocks = _first(hip, sizes, windows, E, seg_log) if sel is None else sel
    nsel = sel[-1]
    T = ppc.stage_offsets(sizes, windows, E, seg_log) if T is None else T
    src = _filled(total, pc.cat(tensors), shift)[:total]
    base = None if bases is None else _filled(total, pc.cat(bases), (shift + 5) % 16)[:total]
    new_cap = hip.frame_packed_bound(int(T[-1]), nsel, blocks, align_log)
    cap = frames.numel() + new_cap if out_cap is None else out_cap
    out = _filled(cap, None, (3 * shift + 1) % 16)
    stage, fresh = _filled(int(T[-1]), None, (shift + 9) % 16), _filled(new_cap)
    ooff, ores, tres, spo, sso, sres, noff, nres = (_marked(nseg + 1), _marked(nseg), _marked(n), _marked(n * E + 1), _marked(nsel + 1), _marked(n), _marked(nsel + 1),
                                                    _marked(nsel))
    ocod = None if codecs is None else _filled(nseg)
    new_codecs = _dev([_given(nseg)[q] for q in ppc.selected_frames(sizes, windows, E, seg_log)]) if form == "given" else None
    kw.setdefault("max_total_blocks", blocks)
    kw.setdefault("seg_first", np.asarray(psc.seg_first(sizes, E, seg_log), np.uint64))
    before = frames.clone()
    tr = _filled(n, np.asarray(transforms, np.uint8))
    hip.tensor_patch_window_each_dbatch(frames, foff, fres, src, S, windows, E, seg_log, tr[:n], sel_first=np.asarray(sel, np.uint64),
                                        stage_offsets=np.asarray(T, np.uint64), base=base, codec=_codec(form), codecs=codecs, new_codecs=new_codecs, block_size_id=0,
                                        align_log=align_log, out=out, out_capacity=cap, out_offsets=ooff, out_results=ores, out_codecs=ocod, tensor_results=tres,
                                        stage=stage, stage_capacity=int(T[-1]), stage_plane_offsets=spo, stage_seg_offsets=sso, stage_results=sres, new_frames=fresh,
                                        new_capacity=new_cap, new_offsets=noff, new_results=nres, **kw)
    torch.cuda.synchronize()
    assert int(ooff[nseg + 1]) == MARK and int(ores[nseg]) == MARK and int(tres[n]) == MARK and torch.equal(frames, before)
    assert int(spo[n * E + 1]) == MARK and int(sso[nsel + 1]) == MARK and int(sres[n]) == MARK and int(noff[nsel + 1]) == MARK and int(nres[nsel]) == MARK
    assert bool((stage[int(T[-1]):] == FILL).all()) and bool((fresh[new_cap:] == FILL).all()) and bool((out[cap:] == FILL).all())
    assert ocod is None or set(ocod.cpu().tolist()[nseg:]) == {FILL}
    assert (tr.cpu().numpy()[:n] == np.asarray(transforms, np.uint8)).all(), "the transforms are only read"
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
        first = psc.seg_first(sizes, E, seg_log)
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
            starts |= {a % 1024 for tr, (a, b) in zip(TRANSFORMS, windows) if tr == PRED and a < b}
        assert changed > rnd // 2 and {0, 1, 1023} <= starts, "PRED windows on a run start, one behind it and one in front of the next"
        # every element, and nothing selected: the full compress, and a copy of the object
        everything = [(0, len(t) // E) for t in old]
        new = _changed(old, fresh, everything, E)               # (the n mod E bytes behind the last whole element lie in no window)
        same_object(run_patch(hip, objs[0], new, bases, everything, E, seg_log, form, 0), compress(hip, new, bases, E, seg_log, form, 0), "everything")
        same_object(run_patch(hip, objs[6], fresh, bases, [(0, 0)] * len(old), E, seg_log, form, 6), objs[6], "nothing")
        assert first[-1] == objs[0][2].numel()


# ---------------------------------------------------------------------------------------------------------------- 3: the result reads back
@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_patched_object_reads_back_as_the_new_tensors(hip, E):
    seg_log = 10
    s = 1 << seg_log
    old, fresh, bases = _corpus(E, seg_log)
    sizes = [len(t) for t in old]
    first = np.asarray(psc.seg_first(sizes, E, seg_log), np.uint64)
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s, s + 1), (s + 7, 2 * s + 9), (0, 0), (s + 5, 3 * s), (1023, s + 40)]
    new = _changed(old, fresh, windows, E)
    out, ooff, ores, tres, _, _ = run_patch(hip, compress(hip, old, bases, E, seg_log, "huf", 0), new, bases, windows, E, seg_log, "huf", 0)
    assert tres == sizes
    S = _offsets(sizes)
    base = _dev(pc.cat(bases))
    back, res = hip.tensor_decompress_seg_each_dbatch(out, ooff, S, E, seg_log, list(TRANSFORMS), base, first)
    torch.cuda.synchronize()
    assert res.cpu().tolist() == sizes and (back.cpu().numpy()[:int(S[-1])] == pc.cat(new)).all()
    # the window read: the windows themselves, and windows across the patch's edges
    for wins in (windows, [(max(a - 3, 0), min(b + 3, len(t) // E)) for t, (a, b) in zip(old, windows)]):
        doff = _offsets([E * (b - a) for a, b in wins])
        wbase = _dev(pc.cat([x[a * E:b * E] for x, (a, b) in zip(bases, wins)] + [np.zeros(1, np.uint8)]))
        dst, res = hip.tensor_decompress_window_each_dbatch(out, ooff, S, wins, doff, E, seg_log, list(TRANSFORMS), first, base=wbase, dst=wbase,
                                                            dst_capacity=int(doff[-1]), block_size_id=0)
        torch.cuda.synchronize()
        assert res.cpu().tolist() == [E * (b - a) for a, b in wins]
        assert (dst.cpu().numpy()[:int(doff[-1])] == pc.cat([w[a * E:b * E] for w, (a, b) in zip(new, wins)])).all()


# ---------------------------------------------------------------------------------------------------------------- 4: refusals of one tensor
@pytest.mark.parametrize("E", pc.ELEMS)
def test_patch_each_refuses_a_tensor_whole_and_patches_the_others(hip, E):
    """refusals of checked values: the tensor keeps ALL its old frames, its neighbours are patched"""
    seg_log, form = 10, "huf"
    s = 1 << seg_log
    old, fresh, bases = _corpus(E, seg_log)
    sizes = [len(t) for t in old]
    n = len(sizes)
    first = psc.seg_first(sizes, E, seg_log)
    windows = [(s - 1, 2 * s + 1), (0, 0), (5, s), (s, s + 1), (s + 7, 2 * s + 9), (0, 0), (s + 5, 3 * s), (1023, s + 40)]
    new = _changed(old, fresh, windows, E)
    sel = _first(hip, sizes, windows, E, seg_log)
    T = ppc.stage_offsets(sizes, windows, E, seg_log)
    obj = compress(hip, old, bases, E, seg_log, form, 0)
    full = compress(hip, new, bases, E, seg_log, form, 0)
    same_object(run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0), full, "nothing refused")

    def kept(victims, bases_=bases):
        """the full compress of: new, but the victims as they were"""
        mixed = [old[i] if i in victims else new[i] for i in range(n)]
        return compress(hip, mixed, bases, E, seg_log, form, 0)

    def alone(got, victims, code, what):
        assert got[3] == [code if i in victims else sizes[i] for i in range(n)], (what, got[3])
        same_object(got, kept(victims), what)
    # a transform byte that is none of the four, on a PRED tensor and on a SUB tensor
    for k in (6, 2):
        tr = list(TRANSFORMS)
        tr[k] = 0xFF
        alone(run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0, tr), (k,), GENERIC, ("0xFF", k))
    # no base: the XOR and SUB tensors alone
    victims = tuple(i for i, tr in enumerate(TRANSFORMS) if tr >= XOR)
    alone(run_patch(hip, obj, new, None, windows, E, seg_log, form, 0), victims, GENERIC, "no base")
    # a > b, and b beyond the tensor: the counts in selFirst and the stage offsets are those of no window
    for k, bad in ((6, (s + 5, s + 4)), (0, (s - 1, sizes[0] // E + 1))):
        w = [bad if i == k else x for i, x in enumerate(windows)]
        none = [(5, 5) if i == k else x for i, x in enumerate(windows)]
        got = run_patch(hip, obj, new, bases, w, E, seg_log, form, 0, sel=_first(hip, sizes, none, E, seg_log), T=ppc.stage_offsets(sizes, none, E, seg_log))
        alone(got, (k,), GENERIC, bad)
    # a pair of stage offsets that does not hold the sub-tensor: tensor 4 has a byte too many, the ones behind it are moved and still hold theirs
    wrong = [t + (1 if i > 4 else 0) for i, t in enumerate(T)]
    alone(run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0, T=wrong), (4,), GENERIC, "stage offsets")
    # counts in selFirst or segFirst that disagree
    if E > 1:
        bad = list(sel[0])
        bad[4 * E + 1] -= 1
        alone(run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0, sel=(bad, sel[1])), (4,), GENERIC, "selFirst")
        bad = list(first)
        bad[1] += 1
        alone(run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0, seg_first=np.asarray(bad, np.uint64), n_segments=first[-1]), (0,), GENERIC, "segFirst")
    # rule 3: an old frame extent that is not one -- a result its extent does not hold, in an unselected frame of tensor 6
    frames, foff, fres, codecs = obj
    q = first[6 * E]                                              # segment 0 of plane 0: the window starts in segment 1
    fres2 = fres.clone()
    fres2[q] = int(foff[q + 1] - foff[q]) + 1
    got = run_patch(hip, (frames, foff, fres2, codecs), new, bases, windows, E, seg_log, form, 0)
    assert got[3] == [CORRUPT if i == 6 else sizes[i] for i in range(n)]
    want = kept((6,))
    res = got[2].cpu().tolist()
    assert res[q] == GENERIC and res[:q] + res[q + 1:] == want[2].cpu().tolist()[:q] + want[2].cpu().tolist()[q + 1:]
    # rule 4: a block promise one short -- the last selected frame fails, its tensor keeps all its frames
    got = run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0, max_total_blocks=sel[1] - 1)
    alone(got, (7,), GENERIC, "a block short")
    # a short outCapacity: dstSize_tooSmall for all, nothing written, the offsets whole
    need = int(full[1][-1])
    got = run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0, out_cap=need - 1)
    assert got[3] == [TOO_SMALL] * n and torch.equal(got[1], full[1]) and bool((got[0] == FILL).all())
    same_object(run_patch(hip, obj, new, bases, windows, E, seg_log, form, 0, out_cap=need), full, "exactly enough")


# ---------------------------------------------------------------------------------------------------------------- 5: one captured graph
def test_patch_each_composite_in_one_hip_graph(hip):
    """one captured graph -- a single stream, a linear chain -- holding tensor_patch_window_each_dbatch; replayed after the tensors and the old object
    were changed (the sizes, the windows' counts and with them every launch size stay)"""
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
    soff, sf, wf, toff, win, tr = _i64(S), _i64(first), _i64(sel), _i64(T), _i64(windows), _dev(TRANSFORMS)
    out, stage, fresh = _filled(out_cap), _filled(T[-1]), _filled(new_cap)
    ooff, noff, sso = (torch.zeros(k + 1, dtype=torch.int64, device="cuda") for k in (nseg, nsel, nsel))
    ores, nres = torch.zeros(nseg, dtype=torch.int64, device="cuda"), torch.zeros(nsel, dtype=torch.int64, device="cuda")
    spo = torch.zeros(n * E + 1, dtype=torch.int64, device="cuda")
    tres, sres = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")

    def work():
        hip.tensor_patch_window_each_dbatch(frames, foff, fres, src, soff, win, E, seg_log, tr, sf, n_segments=nseg, sel_first=wf, n_selected=nsel, stage_offsets=toff,
                                            base=base, codec=0, block_size_id=0, max_total_blocks=blocks, align_log=ALIGN, frames_capacity=room, out=out, out_capacity=out_cap,
                                            out_offsets=ooff, out_results=ores, tensor_results=tres, stage=stage, stage_capacity=T[-1], stage_plane_offsets=spo,
                                            stage_seg_offsets=sso, stage_results=sres, new_frames=fresh, new_capacity=new_cap, new_offsets=noff, new_results=nres,
                                            scratch=scratch, workspace=ws)

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


# ---------------------------------------------------------------------------------------------------------------- 6: the user-facing call
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_patch_tensor_windows_each(hip, monkeypatch):
    import finitestateentropy_amd.api as api
    gen = torch.Generator(device="cuda").manual_seed(37)
    base_bf = (torch.randn((96, 100), generator=gen, device="cuda") * 0.02).to(torch.bfloat16)
    old_bf = (base_bf.float() * (1 + 1e-2 * torch.randn((96, 100), generator=gen, device="cuda"))).to(torch.bfloat16)
    base_f = torch.randn((1500, 3), generator=gen, device="cuda") * 0.02
    old_f = base_f + torch.randn((1500, 3), generator=gen, device="cuda") * 2e-5
    base_i = torch.randint(-128, 128, (40, 50), generator=gen, device="cuda", dtype=torch.int8)
    old_i = base_i.clone(); old_i[1, ::7] += 1
    old_d = torch.cumsum(torch.randint(0, 1000, (3000,), generator=gen, device="cuda", dtype=torch.int64), 0)         # sorted: the estimate takes "pred"
    base_d = torch.randint(-2 ** 62, 2 ** 62, (3000,), generator=gen, device="cuda", dtype=torch.int64)
    empty = torch.zeros((0, 3), device="cuda", dtype=torch.float32)
    base, old = [base_bf, base_f, base_i, base_d, empty], [old_bf, old_f, old_i, old_d, empty.clone()]
    windows = [(100 * 12, 100 * 24), (4499, 4500), None, (1023, 2050), (0, 0)]                                         # rows 12 .. 23 of 96: a 1 / 8 shard
    new = [t.clone() for t in old]
    new[0].view(-1)[1200:2400] = (base_bf.view(-1)[1200:2400].float() * 1.01).to(torch.bfloat16)
    new[1].view(-1)[4499] = 1.5
    new[3].view(-1)[1023:2050] += 7
    kw = dict(segment_log=10, block_size_id=0)
    cases = [("auto", lambda t: hip.compress_tensors_each(t, "auto", base, **kw), base),
             ("given", lambda t: hip.compress_tensors_each(t, ["pred", "xor", "plain", "pred", "sub"], base, codec=1, **kw), base),
             ("chosen codecs", lambda t: hip.compress_tensors_each(t, ["sub", "plain", "pred", "pred", "plain"], base, codec=api.AutoCodec(20), **kw), base),
             ("no base", lambda t: hip.compress_tensors_each(t, ["pred", "plain", "pred", "pred", "plain"], **kw), None),
             ("predicted", lambda t: hip.compress_tensors_segmented(t, 10, api.PredictedPlanes(1), block_size_id=0), None),
             ("plain", lambda t: hip.compress_tensors_segmented(t, 10, block_size_id=0), None),
             ("sub delta", lambda t: hip.compress_tensors_segmented(t, 10, block_size_id=0, base=api.DeltaBase(base, "sub")), api.DeltaBase(base, "sub"))]
    keep = [t.clone() for t in base]
    for name, write, b in cases:
        obj = write(old)
        objs = [(name, obj)]
        if obj.transforms is not None:
            objs.append((name + ", reopened", hip.open_archive(hip.archive_tensors(obj))))
        for what, o in objs:
            snap = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in g.items()} for g in o.groups]
            got = hip.patch_tensor_windows_each(o, new, windows, base=b)
            want = hip.compress_tensors_each(new, o.transforms, base, codec=o.codec, **kw) if o.transforms is not None and b is not None else \
                hip.compress_tensors_each(new, o.transforms, codec=o.codec, **kw) if o.transforms is not None else write(new)
            assert got is not o and got.segment_log == 10 and got.block_size_id == 0 and got.delta == o.delta and got.delta_op == o.delta_op, what
            assert got.transforms == o.transforms and got.predictor == o.predictor and got.codec == o.codec and got.transforms == want.transforms, what
            assert got.dtypes == want.dtypes and got.shapes == want.shapes and got.nbytes == want.nbytes, what
            for g, w, og, sn in zip(got.groups, want.groups, o.groups, snap):
                assert set(g) == set(w) and g["index"] == w["index"] and g["sizes"] == w["sizes"] and [int(x) for x in g["seg_first"]] == [int(x) for x in w["seg_first"]]
                for k in ("frames", "frame_offsets", "frame_results", "tensor_results") + (("codecs",) if "codecs" in w else ()):
                    assert torch.equal(g[k], w[k]), (what, g["elem_bytes"], k)
                    assert torch.equal(og[k], sn[k]) and g[k].data_ptr() != og[k].data_ptr(), "the object given is left as it is, the new one shares nothing with it"
            assert all(_bits(x, y) for x, y in zip(new, hip.decompress_tensors(got, base=b))), what
            back = hip.decompress_tensor_windows_each(got, [(1190, 2410), (4490, 4500), (3, 9), (0, 3000), None], base=b)
            assert _bits(back[0], new[0].view(-1)[1190:2410]) and _bits(back[1], new[1].view(-1)[4490:4500]) and _bits(back[2], new[2].view(-1)[3:9]), what
            assert _bits(back[3], new[3]) and back[4] is None, what
            again = hip.open_archive(hip.archive_tensors(got))
            assert again.transforms == got.transforms and all(_bits(x, y) for x, y in zip(new, hip.decompress_tensors(again, base=b))), what
    assert all(_bits(x, y) for x, y in zip(base, keep)), "the bases are not changed"
    auto = cases[0][1](old)
    assert len(auto.transforms) == 5 and set(auto.transforms) <= set(api.EST_NAMES)
    assert _bits(api.decompress_tensors(api.patch_tensor_windows_each(auto, new, windows, base=base), base=base)[0], new[0]), "the module-level function"
    # nothing changed: a copy of the object
    same = hip.patch_tensor_windows_each(auto, old, [None] * 5, base=base)
    assert same.transforms == auto.transforms and all(torch.equal(g["frames"], o["frames"]) and g["frames"].data_ptr() != o["frames"].data_ptr()
                                                      for g, o in zip(same.groups, auto.groups))
    sparse, unsegmented = hip.compress_tensors_segmented(old, 10, api.SparsePlanes(0), block_size_id=0), hip.compress_tensors_each(old, "auto", base, block_size_id=0)
    predicted, delta = cases[4][1](old), cases[6][1](old)

    # every mismatch is raised before a launch: from here on a call into the library is a failure of the test
    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in ("FSEHIP_tensor_patch_window_each_dbatch", "FSEHIP_planes_split_window_each_dbatch", "FSEHIP_tensor_patch_window_dbatch", "FSEHIP_planes_splice_dbatch",
                 "FSEHIP_tensor_compress_seg_each_dbatch"):
        monkeypatch.setattr(hip.lib, name, no_launch)
    for o, t, w, b in ((unsegmented, new, windows, base), (sparse, new, windows, None), (auto, new[:4], windows, base), (auto, new, windows[:4], base),
                       (auto, new, [(0, 9601)] + windows[1:], base), (auto, new, [(3, 2)] + windows[1:], base), (auto, new, [(0.0, 2)] + windows[1:], base),
                       (auto, new, [5] + windows[1:], base), (auto, [new[0].reshape(100, 96)] + new[1:], windows, base), (auto, new, windows, None),
                       (auto, new, windows, base[:4]), (predicted, new, windows, base), (delta, new, windows, None), (delta, new, windows, api.DeltaBase(base, "xor"))):
        with pytest.raises(ValueError):
            hip.patch_tensor_windows_each(o, t, w, base=b)
    for t in ([new[0].float()] + new[1:], [new[0].cpu()] + new[1:]):
        with pytest.raises(TypeError):
            hip.patch_tensor_windows_each(auto, t, windows, base=base)
    # the old name keeps refusing these objects
    for o, b in ((auto, base), (predicted, None)):
        with pytest.raises(ValueError, match="patches are not supported"):
            hip.patch_tensor_windows(o, new, windows, base=b)

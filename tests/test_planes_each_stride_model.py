"""Strides in the estimate and a stride per tensor without a device (include/fsehip.h, the sections of those names): the composed model of
planes_each_stride_corpus.py against the models it is made of, the choice rule on the corpora of the feature, then the library's eight new
exports and the workspace head, every argument refusal decided before any device call with nothing written (the pointers are host
memory), and the Python surface on a library object that fails the test when it is called."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_each_corpus as pe
import planes_each_stride_corpus as pes
import planes_estimate_corpus as pest
import planes_stride_corpus as psc
from planes_each_stride_corpus import PLAIN, PRED, SUB, XOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
GIVEN, CHOOSE = 0, 1
SZ, VP, U64, UI, CI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint, C.c_int
SIX = ("FSEHIP_planes_split_each_stride_dbatch", "FSEHIP_planes_merge_each_stride_dbatch", "FSEHIP_tensor_compress_each_stride_dbatch",
       "FSEHIP_tensor_compress_seg_each_stride_dbatch", "FSEHIP_tensor_decompress_each_stride_dbatch", "FSEHIP_tensor_decompress_seg_each_stride_dbatch")
EIGHT = SIX + ("FSEHIP_planes_estimate_stride_workspaceBound", "FSEHIP_planes_estimate_stride_dbatch")
HEAD = "FSEHIP_tensor_each_stride_workspaceHead"


@pytest.fixture(scope="module")
def lib():
    """fails on the parent commit: the exports are missing there"""
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    lib = C.CDLL(path)
    for name in EIGHT + (HEAD,):
        getattr(lib, name)
    return lib


# ---------------------------------------------------------------------------------------------------------------- the model
def _tensors(E, seed):
    rng = np.random.default_rng(seed)
    sizes = [0, 1, E, 3 * E, 7 * E + (E > 1), 16 * E, 1023 * E, 1025 * E + E - 1, (1024 + 5) * E, 4 * 1024 * E + 7 * E]
    walk = (np.cumsum(rng.integers(-3, 4, 5000)) + 900).astype(np.uint64).astype(psc._U[E]).view(np.uint8)
    return [walk[:n].copy() if k % 2 else rng.integers(0, 256, n, dtype=np.uint8) for k, n in enumerate(sizes)]


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_stride_estimate_is_the_cost_of_the_strided_split_s_planes(E):
    tensors = _tensors(E, 60 + E)
    bases = [np.roll(t, E) for t in tensors]
    bits, est, choice, res, sest, strides = pes.estimate_stride_model(tensors, E, 15, 0xFF, bases, 50)
    for i, t in enumerate(tensors):
        want = []
        for S in pes.STRIDES:
            buf, _, P, _ = psc.split_model([t], E, S)                                     # the definition: the planes of the strided split ...
            planes = [buf[P[p]:P[p + 1]] for p in range(E)]
            assert [len(p) for p in planes] == [pc.plane_size(len(t), p, E) for p in range(E)]
            want.append(sum(min(len(p), (pest.bits256(np.bincount(p, minlength=256)) + 2047) >> 11) for p in planes))      # ... under the header's cost
        assert sest[8 * i:8 * i + 8] == want, i
        assert strides[i] == pes.choose_stride(want, 0xFF, 50) and est[4 * i + PRED] == want[strides[i] - 1], "the PRED slot holds the chosen stride's numbers"
    # single strides: the entry of that stride alone, all-ones elsewhere, and it is the stride
    for S in pes.STRIDES:
        one = pes.estimate_stride_model(tensors, E, 3, 1 << (S - 1), None, 50)
        assert one[5] == [S] * len(tensors)
        assert all(one[4][8 * i + k] == (sest[8 * i + k] if k == S - 1 else pest.ONES) for i in range(len(tensors)) for k in range(8))


@pytest.mark.parametrize("E", pc.ELEMS)
def test_stride_mask_one_is_the_estimate_model(E):
    tensors = _tensors(E, 70 + E)
    bases = [np.roll(t, 2 * E) for t in tensors]
    for mask, margin, b in ((15, 50, bases), (3, 0, None), (2, 50, None), (13, 300, bases), (1, 50, None)):
        got = pes.estimate_stride_model(tensors, E, mask, 1, b, margin)
        assert got[:4] == pest.estimate_model(tensors, E, mask, b, margin), (mask, margin)
        assert got[5] == [1] * len(tensors)
        assert all(x == pest.ONES for k, x in enumerate(got[4]) if k % 8 or not mask & 2)
        assert not mask & 2 or [got[4][8 * i] for i in range(len(tensors))] == [got[1][4 * i + PRED] for i in range(len(tensors))], "stride 1's entry: the PRED estimate"
    # refused tensors: all-ones and 0xFF
    flat = np.arange(320, dtype=np.uint8)
    offsets = [0, 100, 60, 200, 300, 370]
    units = [flat[a:b] if a <= b <= 320 else flat[:0] for a, b in zip(offsets, offsets[1:])]
    got = pes.estimate_stride_model(units, E, 3, 0x0F, None, 50, capacity=320, offsets=offsets)
    assert got[3] == [100, pc.GENERIC, 140, 100, pc.GENERIC] and got[5][1] == got[5][4] == pes.NO_STRIDE and got[4][8:16] == [pest.ONES] * 8


def test_the_split_model_dispatches_to_the_dedicated_models():
    for E in pc.ELEMS:
        tensors = _tensors(E, 80 + E)
        bases = [np.roll(t, E) for t in tensors]
        n = len(tensors)
        S = [int(x) for x in pc.offsets(tensors)]
        tr, st = pes.cycle_transforms_and_strides(n, 17 * E)
        out, written, P, res = pes.split_each_stride_model(tensors, bases, E, tr, st)
        assert written.all() and res == [len(t) for t in tensors]
        for i in range(n):
            want = psc.split_model(tensors, E, st[i])[0] if tr[i] == PRED else pe.split_each_model(tensors, bases, E, [tr[i]] * n)[0]
            assert (out[S[i]:S[i + 1]] == want[S[i]:S[i + 1]]).all(), (E, i)
            planes = [out[P[i * E + p]:P[i * E + p + 1]] for p in range(E)]
            assert (pes.merge_each_stride_one(planes, bases[i], E, tr[i], st[i]) == tensors[i]).all(), (E, i)
        # strides None is the model of a transform per tensor; garbage strides on other transforms are ignored; 0 and 9 refuse a PRED tensor alone
        a, b = pes.split_each_stride_model(tensors, bases, E, tr, None), pe.split_each_model(tensors, bases, E, tr)
        assert (a[0] == b[0]).all() and a[2:] == b[2:]
        tr2 = [PLAIN, PRED, XOR, SUB, PRED, PRED, PLAIN, PRED, SUB, XOR]
        st2 = [0, 0, 9, 200, 9, 3, 255, 8, 0, 77]
        out, written, P2, res = pes.split_each_stride_model(tensors, bases, E, tr2, st2)
        assert P2 == P and [r == pc.GENERIC for r in res] == [k in (1, 4) for k in range(n)]
        assert not written[S[1]:S[2]].any() and not written[S[4]:S[5]].any() and written[S[5]:].all() and written[S[2]:S[4]].all()


def test_the_cycle_holds_every_ordered_pair_of_the_eleven_kinds():
    for lead in (0, 5, 120):
        tr, st = pes.cycle_transforms_and_strides(122, lead)
        pairs = set(zip(zip(tr, st), zip(tr[1:], st[1:])))
        assert len(pairs) == 121 and {s for t, s in zip(tr, st) if t == PRED} == set(pes.STRIDES)


# ---------------------------------------------------------------------------------------------------------------- the choice
_TABLE = {}


def _table_estimates():
    """per corpus of the table (its first 2^16 elements): the plain estimate and the eight stride estimates, computed once"""
    if not _TABLE:
        for name, (E, t, stride, tr) in pes.table(1 << 16).items():
            plain = pest.est_bytes(pest.candidate_planes(t, None, E, PLAIN))
            _TABLE[name] = (plain, [pest.est_bytes(pes.stride_planes(t, E, S)) for S in pes.STRIDES], stride, tr)
    return _TABLE


def test_the_rule_chooses_the_channel_count_on_the_corpora():
    for name, (plain, sest, stride, tr) in _table_estimates().items():
        for margin in (0, 50) + ((200,) if name == "boxes" else ()):
            got = pes.choose_stride(sest, 0xFF, margin)
            choice = pest.choose([plain, sest[got - 1], pest.ONES, pest.ONES], 3, margin)
            assert (got, choice) == (stride, tr), (name, margin, plain, sest)
    plain, sest, _, _ = _table_estimates()["stereo"]
    assert sest[1] * 100 < plain * 55 and plain < sest[0] and sest[1] < sest[3] < sest[5] < sest[7], "stereo: stride 2 nearly halves it, stride 1 is worse than plain, the multiples cost a little more"


def test_hysteresis_keeps_the_lower_stride():
    est = [1000, 951, 949, 901, 900, 10 ** 9, 10 ** 9, 860]
    assert pes.choose_stride(est, 0xFF, 0) == 8 and pes.choose_stride(est, 0xFF, 50) == 4 and pes.choose_stride(est, 0xFF, 1000) == 1
    assert pes.choose_stride(est, 0b00000110, 50) == 2 and pes.choose_stride(est, 0b00000110, 0) == 3, "the lowest requested stride starts"
    assert pes.choose_stride([500, 475] + [pest.ONES] * 6, 3, 50) == 1 and pes.choose_stride([500, 474] + [pest.ONES] * 6, 3, 50) == 2, "strictly more than the margin"
    assert pes.choose_stride([0, 0, 0, 0, 0, 0, 0, 0], 0xFF, 0) == 1, "equal estimates: the lower stride"
    assert pes.settled([PRED, PLAIN, pest.NO_CHOICE, SUB], [3, 2, 0xFF, 4]) == [3, 1, 0xFF, 1]


# ---------------------------------------------------------------------------------------------------------------- the library
def _r256(x):
    return (x + 255) & ~255


def test_exports_header_and_python_names(lib):
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    for name in EIGHT + (HEAD,):
        assert name in header, name
    from finitestateentropy_amd import api
    for name in ("planes_estimate_stride_workspace_bound", "planes_estimate_stride_dbatch", "tensor_each_stride_workspace_head", "planes_split_each_stride_dbatch",
                 "planes_merge_each_stride_dbatch", "tensor_compress_each_stride_dbatch", "tensor_compress_seg_each_stride_dbatch", "tensor_decompress_each_stride_dbatch",
                 "tensor_decompress_seg_each_stride_dbatch"):
        assert callable(getattr(api.FseHip, name)), name
    par = inspect.signature(api.FseHip.compress_tensors_each).parameters
    assert list(par)[-1] == "strides" and par["strides"].default is None
    par = inspect.signature(api.FseHip.estimate_tensors).parameters
    assert list(par)[-1] == "strides" and par["strides"].default is None
    assert api.CompressedTensors.strides is None, "the class-level default"


def test_the_workspace_bounds_are_host_arithmetic(lib):
    bound, old, head, ohead = (lib.FSEHIP_planes_estimate_stride_workspaceBound, lib.FSEHIP_planes_estimate_workspaceBound, lib.FSEHIP_tensor_each_stride_workspaceHead,
                               lib.FSEHIP_tensor_each_workspaceHead)
    bound.restype = old.restype = head.restype = ohead.restype = SZ
    for E in pc.ELEMS:
        for n in (0, 1, 3, 33, 4096, (1 << 24) - 1):
            for mask in range(1, 16):
                assert bound(SZ(n), UI(E), UI(mask), UI(1)) == old(SZ(n), UI(E), UI(mask)), "strideMask 1: the bound of the existing call"
                assert head(SZ(n), UI(E), CI(CHOOSE), UI(mask), UI(1)) == ohead(SZ(n), UI(E), CI(CHOOSE), UI(mask))
                assert head(SZ(n), UI(E), CI(GIVEN), UI(mask), UI(0xFF)) == 0 and head(SZ(n), UI(E), CI(GIVEN), UI(0), UI(0)) == 0
                for smask in (2, 0x0F, 0x80, 0xFF):
                    if not mask & 2:
                        assert bound(SZ(n), UI(E), UI(mask), UI(smask)) > (1 << 62) and head(SZ(n), UI(E), CI(CHOOSE), UI(mask), UI(smask)) > (1 << 62)
                        continue
                    sets = bin(mask & ~2).count("1") + bin(smask).count("1")
                    want = _r256(n * sets * E * 1024)
                    assert bound(SZ(n), UI(E), UI(mask), UI(smask)) == want and want % 256 == 0, (E, n, mask, smask)
                    got = head(SZ(n), UI(E), CI(CHOOSE), UI(mask), UI(smask))
                    assert got == want + _r256(n * 4 * E * 8) + _r256(n * 4 * 8) + _r256(n * 8) and got % 256 == 0
    for n, E, mask, smask in ((1, 2, 3, 0), (1, 2, 3, 0x100), (1, 2, 3, 0xFFFFFFFF), (1, 2, 0, 1), (1, 2, 16, 1), (1, 3, 3, 1), (1 << 24, 2, 3, 1), (1, 2, 1, 3), (1, 2, 13, 2)):
        assert bound(SZ(n), UI(E), UI(mask), UI(smask)) > (1 << 62), (n, E, mask, smask)
        assert head(SZ(n), UI(E), CI(CHOOSE), UI(mask), UI(smask)) > (1 << 62), (n, E, mask, smask)
    assert head(SZ(1), UI(2), CI(2), UI(3), UI(1)) > (1 << 62) and head(SZ(1), UI(3), CI(GIVEN), UI(3), UI(1)) > (1 << 62)


def test_every_argument_refusal_without_a_device(lib):
    for f in (HEAD, "FSEHIP_planes_estimate_stride_workspaceBound", "FSEHIP_frame_compress_packed_dbatch_workspaceSize", "FSEHIP_frame_mixedWorkspaceBound",
              "FSEHIP_frame_decompress_packed_dbatch_workspaceSize"):
        getattr(lib, f).restype = SZ
    n, E, blocks, nseg = 1, 2, 8, 2
    head = getattr(lib, HEAD)(SZ(n), UI(E), CI(CHOOSE), UI(15), UI(0xFF))
    need = head + max(lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize(SZ(4), SZ(blocks), UI(0), CI(0)),
                      lib.FSEHIP_frame_mixedWorkspaceBound(SZ(4), SZ(blocks), UI(0), CI(1)),
                      lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize(SZ(4), SZ(blocks)))
    assert need < (1 << 30)
    GUARD = 0xF9
    a = (C.c_uint8 * 256)(*([GUARD] * 256))                     # stands for every output: offsets, results, transforms, strides, planes, frames
    room = (C.c_uint8 * (need + 512))(*([GUARD] * (need + 512)))
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    wb = SZ(need)

    # ---- the estimate
    ewb = lib.FSEHIP_planes_estimate_stride_workspaceBound(SZ(n), UI(E), UI(15), UI(0xFF))

    def est(q=None, base=p, sest=p, E=E, n=n, cap=8, mask=15, margin=50, smask=0xFF, w=ws, wb=SZ(ewb)):
        q = list(q or [p] * 7)                                  # plane bits, est bytes, choice, results, strides, src, offsets
        return lib.FSEHIP_planes_estimate_stride_dbatch(q[0], q[1], q[2], q[3], sest, q[4], q[5], base, q[6], SZ(n), UI(E), U64(cap), UI(mask), UI(margin), w, wb,
                                                        UI(smask), null)
    for k in range(7):
        q = [p] * 7
        q[k] = null
        assert est(q) == HIP_INVALID_VALUE, k
    for smask in (0, 0x100, 0x1FF, 0x80000001, 0xFFFFFFFF):
        assert est(smask=smask) == HIP_INVALID_VALUE, smask
    for mask, smask in ((1, 2), (1, 3), (13, 0xFF), (12, 0x80), (5, 0x10)):
        assert est(mask=mask, smask=smask) == HIP_INVALID_VALUE, "a stride set beyond stride 1 without PRED among the candidates"
    for mask in (0, 16, 0x8000000F):
        assert est(mask=mask) == HIP_INVALID_VALUE and est(mask=mask, smask=1) == HIP_INVALID_VALUE
    assert est(base=null) == HIP_INVALID_VALUE and est(base=null, mask=6, smask=3) == HIP_INVALID_VALUE, "XOR or SUB without a base"
    for bad in (0, 3, 16):
        assert est(E=bad) == HIP_INVALID_VALUE
    assert est(margin=1001) == HIP_INVALID_VALUE and est(wb=SZ(ewb - 1)) == HIP_INVALID_VALUE and est(w=null) == HIP_INVALID_VALUE
    assert est(w=VP(ws.value + 8)) == HIP_INVALID_VALUE and est(n=1 << 24) == HIP_INVALID_VALUE and est(cap=1 << 46) == HIP_INVALID_VALUE

    # ---- split and merge (d_strides and d_base may be NULL: those calls would launch, they are not made here)
    def split(q=None, E=E, n=n, cap=8):                       # q: planes, plane offsets, results, src, base, transforms, strides, offsets
        q = list(q or [p] * 8)
        return lib.FSEHIP_planes_split_each_stride_dbatch(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], SZ(n), UI(E), U64(cap), null)

    def merge(q=None, E=E, n=n, cap=8):                       # q: dst, dst offsets, results, planes, plane offsets, plane sizes, base, transforms, strides
        q = list(q or [p] * 9)
        return lib.FSEHIP_planes_merge_each_stride_dbatch(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], SZ(n), UI(E), U64(cap), null)
    for k in (0, 1, 2, 3, 5, 7):
        q = [p] * 8
        q[k] = null
        assert split(q) == HIP_INVALID_VALUE, k
    for k in (0, 1, 2, 3, 4, 5, 7):
        q = [p] * 9
        q[k] = null
        assert merge(q) == HIP_INVALID_VALUE, k
    for bad in (0, 3, 5, 16, 0xFFFFFFFF):
        assert split(E=bad) == HIP_INVALID_VALUE and merge(E=bad) == HIP_INVALID_VALUE, bad
    assert split(cap=1 << 46) == HIP_INVALID_VALUE and merge(cap=1 << 46) == HIP_INVALID_VALUE and split(n=1 << 30) == HIP_INVALID_VALUE and merge(n=1 << 30) == HIP_INVALID_VALUE

    # ---- the compress composites
    def comp(seg, q=None, base=p, strides=p, est=p, policy=CHOOSE, mask=15, smask=0x0F, margin=50, E=E, n=n, cap=8, segLog=10, blocks=blocks, bsid=0, codec=0, codecs=null,
             cpolicy=0, tol=0, align=0, w=ws, wb=wb):
        # q: dst, frame offsets, frame results, tensor results, src, transforms, src offsets, planes, plane offsets [, seg first, seg offsets]
        q = list(q or [p] * 11)
        front = (q[0], U64(256), q[1], q[2], q[3], q[4], base, q[5], strides, CI(policy), UI(mask), UI(smask), UI(margin), est, q[6], SZ(n), UI(E), U64(cap))
        writer = (SZ(blocks), UI(bsid), CI(codec), codecs, CI(cpolicy), UI(tol), UI(align), q[7], q[8])
        if seg:
            return lib.FSEHIP_tensor_compress_seg_each_stride_dbatch(*front, q[9], SZ(nseg), UI(segLog), *writer, q[10], w, wb, null)
        return lib.FSEHIP_tensor_compress_each_stride_dbatch(*front, *writer, w, wb, null)
    for seg in (False, True):
        for k in range(1, 11 if seg else 9):
            q = [p] * 11
            q[k] = null
            assert comp(seg, q) == HIP_INVALID_VALUE, (seg, k)
        for smask in (0, 0x100, 0xFFFFFFFF):
            assert comp(seg, smask=smask) == HIP_INVALID_VALUE, smask
        assert comp(seg, mask=13, smask=3) == HIP_INVALID_VALUE and comp(seg, mask=1, smask=0x80) == HIP_INVALID_VALUE, "strides without PRED among the candidates"
        assert comp(seg, strides=null, smask=3) == HIP_INVALID_VALUE, "CHOOSE over strides needs the array it writes"
        for bad in (0, 3, 5, 16):
            assert comp(seg, E=bad) == HIP_INVALID_VALUE, bad
        for policy in (2, -1, 7):
            assert comp(seg, policy=policy) == HIP_INVALID_VALUE
        for mask in (0, 16, 31, 0xFFFFFFFF):
            assert comp(seg, mask=mask) == HIP_INVALID_VALUE, mask
        assert comp(seg, mask=15, base=null) == HIP_INVALID_VALUE and comp(seg, margin=1001) == HIP_INVALID_VALUE
        assert comp(seg, w=VP(ws.value + 16)) == HIP_INVALID_VALUE and comp(seg, w=null) == HIP_INVALID_VALUE
        assert comp(seg, wb=SZ(head - 1)) == HIP_INVALID_VALUE and comp(seg, wb=SZ(head)) == HIP_INVALID_VALUE, "room for the estimate alone: the writer has none"
        assert comp(seg, policy=GIVEN, wb=SZ(0)) == HIP_INVALID_VALUE and comp(seg, policy=GIVEN, smask=0, wb=SZ(0)) == HIP_INVALID_VALUE
        assert comp(seg, cap=1 << 46) == HIP_INVALID_VALUE and comp(seg, n=1 << 24) == HIP_INVALID_VALUE and comp(seg, n=1 << 30, policy=GIVEN) == HIP_INVALID_VALUE
        assert comp(seg, codec=2) == HIP_INVALID_VALUE and comp(seg, bsid=7) == HIP_INVALID_VALUE and comp(seg, align=13) == HIP_INVALID_VALUE
        assert comp(seg, codecs=p, cpolicy=2) == HIP_INVALID_VALUE and comp(seg, codecs=p, cpolicy=1, tol=1001) == HIP_INVALID_VALUE
    assert comp(True, segLog=9) == HIP_INVALID_VALUE and comp(True, segLog=31) == HIP_INVALID_VALUE and comp(True, segLog=10, bsid=1) == HIP_INVALID_VALUE

    # ---- the decompress composites
    def dec(seg, q=None, strides=p, E=E, n=n, cap=8, segLog=10, blocks=blocks, w=ws, wb=wb):
        # q: dst, dst offsets, transforms, results, frames, frame offsets, planes, plane offsets, plane results [, seg first, seg offsets, seg results]
        q = list(q or [p] * 12)
        front = (q[0], q[1], U64(cap), p, q[2], strides, q[3], q[4], q[5], SZ(n), UI(E))
        if seg:
            return lib.FSEHIP_tensor_decompress_seg_each_stride_dbatch(*front, q[9], SZ(nseg), UI(segLog), SZ(blocks), q[6], U64(64), q[10], q[11], q[7], q[8], w, wb, null)
        return lib.FSEHIP_tensor_decompress_each_stride_dbatch(*front, SZ(blocks), q[6], U64(64), q[7], q[8], w, wb, null)
    for seg in (False, True):
        for k in range(12 if seg else 9):
            q = [p] * 12
            q[k] = null
            assert dec(seg, q) == HIP_INVALID_VALUE, (seg, k)
        for bad in (0, 3, 5, 16):
            assert dec(seg, E=bad) == HIP_INVALID_VALUE, bad
        assert dec(seg, cap=1 << 46) == HIP_INVALID_VALUE and dec(seg, n=1 << 30) == HIP_INVALID_VALUE and dec(seg, blocks=1 << 31) == HIP_INVALID_VALUE
        assert dec(seg, w=VP(ws.value + 16)) == HIP_INVALID_VALUE and dec(seg, wb=SZ(0)) == HIP_INVALID_VALUE and dec(seg, strides=null, wb=SZ(0)) == HIP_INVALID_VALUE
    assert dec(True, segLog=9) == HIP_INVALID_VALUE and dec(True, segLog=31) == HIP_INVALID_VALUE
    assert all(x == GUARD for x in a) and all(x == GUARD for x in bytes(room)), "nothing is written"


# ---------------------------------------------------------------------------------------------------------------- Python
class _Trap:
    """stands for the library: any call, any launch fails the test"""

    def __getattr__(self, name):
        pytest.fail("the library was reached for (%s) in front of a ValueError that comes before any launch" % name)


def test_the_python_surface_in_front_of_any_launch():
    import json

    import torch

    from finitestateentropy_amd import api
    hip = api.FseHip.__new__(api.FseHip)
    hip.lib = _Trap()
    # today's behaviour by default
    obj = hip.compress_tensors_each([])
    assert obj.transforms == [] and obj.strides is None
    assert hip.estimate_tensors([]) == [] and hip.estimate_tensors([], strides=(1, 2, 3)) == []
    obj = hip.compress_tensors_each([], "auto", strides=(1, 2, 3, 4))
    assert obj.transforms == [] and obj.strides == [] and hip.decompress_tensors(obj) == []
    assert hip.compress_tensors_each([], [], strides=[]).strides == []
    # 1: a stride outside 1 .. 8
    for bad in ((0,), (9,), (1, 2, 16), (-1,), (2.0,), (True,), (), "12"):
        with pytest.raises(ValueError):
            hip.compress_tensors_each([], "auto", strides=bad)
        with pytest.raises(ValueError):
            hip.estimate_tensors([], strides=bad)
    for bad in ([0], [9], [2.0], [1, 1]):                          # (given with the names: one per tensor, looked at before the tensors are)
        with pytest.raises(ValueError):
            hip.compress_tensors_each([np.zeros(4)], ["pred"], strides=bad)
    # 2: strides without PRED among the candidates
    with pytest.raises(ValueError, match="pred"):
        hip.estimate_tensors([], candidates=("plain",), strides=(1, 2))
    with pytest.raises(ValueError, match="pred"):
        hip.estimate_tensors([], base=[], candidates=("plain", "xor", "sub"), strides=(2,))
    # 3, 4: windows and patches of an object with a stride above 1
    held = api.CompressedTensors([], [torch.int16, torch.float32], [(8,), (6,)], None, 0, 5)
    held.segment_log, held.transforms, held.strides = 18, ["pred", "plain"], [2, 1]
    with pytest.raises(ValueError, match="stride above 1"):
        hip.decompress_tensor_windows_each(held, [None, None])
    with pytest.raises(ValueError, match="stride above 1"):
        hip.patch_tensor_windows_each(held, [None, None], [None, None])
    for bad in ([2], [0, 1], [9, 1], [2, "1"]):
        held.strides = bad
        with pytest.raises(ValueError):
            hip.decompress_tensors(held)
    # the meta JSON: strides only where one exceeds 1
    held.strides = [2, 1]
    meta = api.FseHip._archive_meta(held, 0, 1, [0, 1], 0, 0)
    assert meta["transforms"] == ["pred", "plain"] and meta["strides"] == [2, 1] and json.loads(json.dumps(meta)) == meta
    assert api.FseHip._archive_meta(held, 0, 2, [1], 0, 0)["strides"] == [1], "per group, in the group's order"
    for quiet in ([1, 1], None):
        held.strides = quiet
        assert "strides" not in api.FseHip._archive_meta(held, 0, 1, [0, 1], 0, 0), "an object of stride 1 keeps the meta bytes it always had"

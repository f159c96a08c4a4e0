"""Patching tensors with a transform per tensor without a device (include/fsehip.h, the section of that name): the numpy model
(planes_patch_each_corpus.py) -- the planes of transform(sub-tensor) are segments k0 .. k1 of the planes of transform(tensor), and a change inside
the window leaves every plane byte outside the selected segments as it was --, the shapes the split test's corpus must hold, the library's
exports and Python names, and every argument refusal of the two C calls, decided before any device call with nothing written (the pointers
are host memory)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_each_corpus as pe
import planes_patch_corpus as ppc
import planes_patch_each_corpus as ppe
import planes_window_each_corpus as pwe
from planes_each_corpus import IDS, PLAIN, PRED, SUB, XOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI, I = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint, C.c_int
TWO = ("FSEHIP_planes_split_window_each_dbatch", "FSEHIP_tensor_patch_window_each_dbatch")
SEG_LOG = 10


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


# ---------------------------------------------------------------------------------------------------------------- the model
def _tensor(rng, m, E, tail):
    t = rng.integers(0, 256, m * E + tail, dtype=np.uint8)
    if m:                                                       # a smooth half: small differences
        x = (np.cumsum(rng.integers(-2, 3, m)) + 300).astype("<u8")
        t[:m // 2 * E] = np.ascontiguousarray(x.view(np.uint8).reshape(-1, 8)[:m // 2, :E]).reshape(-1)
    return t


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_planes_of_the_sub_tensor_are_the_segments_of_the_planes_of_the_tensor(E):
    """for all four transforms, every window between the ends, tensor sizes with and without a partial last element"""
    rng = np.random.default_rng(170 + E)
    for m in (0, 1, 15, 17, 1023, 1025, 2051, 3100):
        for tail in {0, E - 1}:
            t, b = _tensor(rng, m, E, tail), rng.integers(0, 256, m * E + tail, dtype=np.uint8)
            for tr in IDS:
                for a, c in pwe.window_set(m):
                    want = ppe.segment_slices(t, b, E, tr, a, c, SEG_LOG)
                    got = ppe.sub_planes(t, b, E, tr, a, c, SEG_LOG)
                    assert len(want) == len(got) == E and all(w.shape == g.shape and (w == g).all() for w, g in zip(want, got)), (m, tail, tr, a, c)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_a_change_inside_the_window_leaves_the_planes_outside_the_selected_segments(E):
    """the identity the patch rests on: old and new differ inside [a, b) only => the planes of transform(new) differ from those of transform(old)
    inside segments k0 .. k1 only -- for PRED too, whose difference at element b reads element b - 1: b lies in a selected segment or starts a run"""
    rng = np.random.default_rng(180 + E)
    s = 1 << SEG_LOG
    for m in (17, 1025, 2051, 3100):
        for tail in {0, E - 1}:
            old, base = _tensor(rng, m, E, tail), rng.integers(0, 256, m * E + tail, dtype=np.uint8)
            for a, c in pwe.window_set(m):
                new = old.copy()
                new[a * E:c * E] ^= rng.integers(1, 256, (c - a) * E, dtype=np.uint8)
                at, n = ppc.sub_range(len(old), a, c, E, SEG_LOG)
                k0, k1 = at // E, at // E + pc.plane_size(n, 0, E)
                assert k0 % s == 0 and (n == 0 or k0 <= a < c <= k1)
                for tr in IDS:
                    po, pn = pwe.whole_planes(old, base, E, tr), pwe.whole_planes(new, base, E, tr)
                    for p in range(E):
                        hi = k0 + pc.plane_size(n, p, E)
                        assert (po[p][:k0] == pn[p][:k0]).all() and (po[p][hi:] == pn[p][hi:]).all(), (m, tail, tr, a, c, p)
                    if c > a:
                        assert any((x != y).any() for x, y in zip(po, pn))


def test_a_sub_tensor_off_a_run_start_would_be_wrong():
    """the model told apart from a split that cuts anywhere: PRED planes of a sub-tensor that starts one element behind a run start differ from
    the tensor's own there -- the patch is right because segLog >= FSEHIP_PRED_RUN_LOG, not by accident"""
    E, m = 2, 3000
    t = np.random.default_rng(4).integers(1, 256, m * E, dtype=np.uint8)
    whole = pwe.whole_planes(t, None, E, PRED)
    for cut in (1, 1023, 1025):
        sub = pc.planes_of(pe.forward(t[cut * E:], None, E, PRED), E)
        assert any((sub[p] != whole[p][cut:]).any() for p in range(E)), cut
    for cut in (0, 1024, 2048):
        sub = pc.planes_of(pe.forward(t[cut * E:], None, E, PRED), E)
        assert all((sub[p] == whole[p][cut:]).all() for p in range(E)), cut
    assert SEG_LOG >= 10 and pwe.RUN == 1 << 10


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_corpus_holds_the_shapes_the_split_test_needs(E):
    c = ppe.split_corpus(E, SEG_LOG)
    missing = [name for name, held in ppe.shapes(c, E, SEG_LOG).items() if not held]
    assert not missing, missing
    assert all(a in pwe.ends(m) and b in pwe.ends(m) and a <= b for (a, b), m in zip(c["windows"], c["counts"]))
    assert all(len(t) // E == m and len(t) == len(b) for t, b, m in zip(c["tensors"], c["bases"], c["counts"]))
    sizes = [len(t) for t in c["tensors"]]
    assert [x - ppe.LEAD for x in c["T"]] == ppc.stage_offsets(sizes, c["windows"], E, SEG_LOG)


def test_the_stage_model_refuses_by_rule_1():
    E = 2
    rng = np.random.default_rng(9)
    tensors = [rng.integers(0, 256, 2 * 1500, dtype=np.uint8) for _ in range(4)]
    windows = [(5, 1030), (0, 0), (1024, 1500), (1023, 1024)]
    good = ppe.stage_each_model(tensors, windows, E, SEG_LOG, [PRED, SUB, XOR, PLAIN], bases=tensors[::-1])
    assert good[3] == [2 * 1500, 0, 2 * 476, 2 * 1024]
    plain = ppc.stage_model(tensors, windows, E, SEG_LOG)
    same = ppe.stage_each_model(tensors, windows, E, SEG_LOG, [PLAIN] * 4)
    assert (plain[0] == same[0]).all() and plain[2:] == same[2:], "all PLAIN is the model of the existing split"
    xor = ppc.stage_model(tensors, windows, E, SEG_LOG, tensors[::-1])
    same = ppe.stage_each_model(tensors, windows, E, SEG_LOG, [XOR] * 4, tensors[::-1])
    assert (xor[0] == same[0]).all() and xor[2:] == same[2:]
    T = ppc.stage_offsets([len(t) for t in tensors], windows, E, SEG_LOG)
    for tr, bases, bad in (([PRED, SUB, XOR, PLAIN], None, (1, 2)), ([0xFF, PLAIN, PRED, 4], tensors, (0, 3))):
        out, written, P, res = ppe.stage_each_model(tensors, windows, E, SEG_LOG, tr, bases)
        for i in range(4):
            if i in bad:
                assert res[i] == pc.GENERIC and P[i * E:(i + 1) * E] == [T[i]] * E and not written[T[i]:T[i + 1]].any()
            else:
                assert res[i] == good[3][i] and written[T[i]:T[i + 1]].all()


# ---------------------------------------------------------------------------------------------------------------- the library
def test_exports_and_python_names(lib):
    """fails on the parent commit: none of these exists there"""
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    for name in TWO:
        getattr(lib, name)
        assert name in header, name
    declared = set(__import__("re").findall(r"\b(FSEHIP_\w+_workspace(?:Size|Bound|Head))\s*\(", header))
    assert not any("patch" in d or "window_each" in d for d in declared), "no workspace function of its own: the packed writer's"
    import finitestateentropy_amd
    from finitestateentropy_amd import api
    assert "patch_tensor_windows_each" in finitestateentropy_amd.__all__
    assert finitestateentropy_amd.patch_tensor_windows_each is api.patch_tensor_windows_each
    for name in ("planes_split_window_each_dbatch", "tensor_patch_window_each_dbatch", "patch_tensor_windows_each"):
        assert callable(getattr(api.FseHip, name)), name
    assert list(inspect.signature(api.patch_tensor_windows_each).parameters) == ["obj", "tensors", "windows", "base"]
    assert list(inspect.signature(api.patch_tensor_windows).parameters) == ["obj", "tensors", "windows", "base"], "unchanged"
    for old, new in ((api.FseHip.planes_split_window_dbatch, api.FseHip.planes_split_window_each_dbatch),
                     (api.FseHip.tensor_patch_window_dbatch, api.FseHip.tensor_patch_window_each_dbatch)):
        old, new = inspect.signature(old).parameters, inspect.signature(new).parameters
        assert [k for k in new if k != "transforms"] == [k for k in old if k != "delta_op"], "the patch call's arguments, transforms for the op"


def test_the_prototypes_take_transforms_where_the_op_calls_take_the_op():
    """the header's two prototypes against those of the calls they extend: the same argument list with `const uint8_t* d_transforms` in place
    of `unsigned deltaOp`"""
    import re
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()

    def params(name):
        m = re.search(r"FSEHIP_API int %s\s*\(([^;]*)\);" % name, header)
        return [" ".join(p.split()) for p in m.group(1).split(",")]
    for old, new in (("FSEHIP_planes_split_window_op_dbatch", TWO[0]), ("FSEHIP_tensor_patch_window_op_dbatch", TWO[1])):
        assert [("const uint8_t* d_transforms" if p == "unsigned deltaOp" else p) for p in params(old)] == params(new)


def test_every_argument_refusal_without_a_device(lib):
    need = lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize
    need.restype = SZ
    bound = lib.FSEHIP_planes_spliceScratchBound
    bound.restype = SZ
    mixed = lib.FSEHIP_frame_mixedWorkspaceBound
    mixed.restype = SZ
    n, nseg, nsel, blocks = 1, 4, 2, 4
    wsize, ssize = need(SZ(nsel), SZ(blocks), UI(0), I(0)), bound(SZ(n), UI(2), SZ(nseg))
    msize = mixed(SZ(nsel), SZ(blocks), UI(0), I(1))
    assert 1 < wsize < (1 << 28) and 1 < ssize < (1 << 20) and wsize <= msize < (1 << 28)
    GUARD = 0xF9
    a = (C.c_uint8 * 256)(*([GUARD] * 256))                     # stands for every array
    big = max(wsize, msize)
    room = (C.c_uint8 * (big + 512))(*([GUARD] * (big + 512)))
    sroom = (C.c_uint8 * (ssize + 512))(*([GUARD] * (ssize + 512)))
    p, null = C.cast(a, VP), VP(0)
    ws, sc = VP((C.addressof(room) + 255) & ~255), VP((C.addressof(sroom) + 255) & ~255)

    # ---- the split: stage, plane offsets, results, src, base, transforms, src offsets, windows, stage offsets
    def split(q=None, E=2, seg_log=10, n=1, cap=8, scap=8):
        q = list(q or [p] * 9)
        return lib.FSEHIP_planes_split_window_each_dbatch(*q, SZ(n), UI(E), UI(seg_log), U64(cap), U64(scap), null)
    for k in range(9):
        if k != 4:                                             # (the base may be NULL: that call would launch, it is not made here)
            assert split([null if x == k else p for x in range(9)]) == HIP_INVALID_VALUE, k
    for bad in (0, 3, 5, 16, 0xFFFFFFFF):
        assert split(E=bad) == HIP_INVALID_VALUE, bad
    for seg_log in (0, 9, 31, 40):
        assert split(seg_log=seg_log) == HIP_INVALID_VALUE, seg_log
    assert split(n=1 << 30) == HIP_INVALID_VALUE, "2^31 planes"
    assert split(scap=1 << 46) == HIP_INVALID_VALUE and split(scap=32768 << 24) == HIP_INVALID_VALUE and split(n=1 << 24, E=1) == HIP_INVALID_VALUE, "the launch limit"

    # ---- the composite
    names = ("out", "ooff", "ores", "tres", "frames", "foff", "fres", "src", "tr", "soff", "win", "sf", "wf", "toff", "stage", "spo", "sso", "sres", "new", "noff", "nres")

    def patch(E=2, seg_log=10, n=n, nseg=nseg, nsel=nsel, blocks=blocks, bsid=0, codec=0, policy=0, tol=0, align=0, ocap=8, scap=8, base=p, codecs=(null, null, null),
              s=sc, sb=ssize, w=ws, wb=wsize, **nulls):
        assert set(nulls) <= set(names)
        q = {k: null if k in nulls else p for k in names}
        ocod, cod, ncod = codecs
        return lib.FSEHIP_tensor_patch_window_each_dbatch(
            q["out"], U64(ocap), q["ooff"], q["ores"], ocod, q["tres"], q["frames"], U64(8), q["foff"], q["fres"], cod, q["src"], base, q["tr"], q["soff"], U64(8),
            q["win"], SZ(n), UI(E), q["sf"], SZ(nseg), UI(seg_log), q["wf"], SZ(nsel), q["toff"], U64(scap), SZ(blocks), UI(bsid), I(codec), ncod, I(policy), UI(tol),
            UI(align), q["stage"], q["spo"], q["sso"], q["sres"], q["new"], U64(8), q["noff"], q["nres"], s, SZ(sb), w, SZ(wb), null)
    for name in names:                                          # null pointers, d_transforms among them
        assert patch(**{name: True}) == HIP_INVALID_VALUE, name
    for E in (0, 3, 5, 16, 0xFFFFFFFF):
        assert patch(E=E) == HIP_INVALID_VALUE, E
    for seg_log in (0, 9, 31, 40):
        assert patch(seg_log=seg_log) == HIP_INVALID_VALUE, seg_log
    assert patch(seg_log=10, bsid=1) == HIP_INVALID_VALUE and patch(bsid=7, seg_log=20) == HIP_INVALID_VALUE, "segLog below 10 + blockSizeId, a block-size id that is none"
    assert patch(nseg=4, nsel=5, wb=need(SZ(5), SZ(blocks), UI(0), I(0))) == HIP_INVALID_VALUE, "more selected frames than frames"
    for big_n in (1 << 31, 1 << 40):
        assert patch(nseg=big_n, sb=1 << 62) == HIP_INVALID_VALUE and patch(blocks=big_n) == HIP_INVALID_VALUE
    assert patch(n=1 << 30, sb=1 << 62) == HIP_INVALID_VALUE, "2^31 planes"
    assert patch(ocap=1 << 46) == HIP_INVALID_VALUE and patch(scap=1 << 46) == HIP_INVALID_VALUE and patch(scap=32768 << 24) == HIP_INVALID_VALUE, "the launch limits"
    assert patch(codec=2) == HIP_INVALID_VALUE and patch(codec=-1) == HIP_INVALID_VALUE and patch(align=13) == HIP_INVALID_VALUE
    assert patch(wb=wsize - 1) == HIP_INVALID_VALUE and patch(wb=0) == HIP_INVALID_VALUE, "a short writer workspace"
    assert patch(w=VP(ws.value + 128)) == HIP_INVALID_VALUE, "a misaligned workspace"
    assert patch(sb=ssize - 1) == HIP_INVALID_VALUE and patch(sb=0) == HIP_INVALID_VALUE and patch(s=null) == HIP_INVALID_VALUE, "short scratch"
    assert patch(s=VP(sc.value + 128)) == HIP_INVALID_VALUE, "misaligned scratch"
    # codecs: all three or none; a policy and a tolerance that are none; the mixed writer's workspace
    assert patch(codecs=(p, null, null)) == HIP_INVALID_VALUE and patch(codecs=(null, p, null)) == HIP_INVALID_VALUE and patch(codecs=(null, null, p)) == HIP_INVALID_VALUE
    assert patch(codecs=(p, p, null)) == HIP_INVALID_VALUE
    assert patch(codecs=(p, p, p), policy=2, wb=msize) == HIP_INVALID_VALUE and patch(codecs=(p, p, p), policy=1, tol=1001, wb=msize) == HIP_INVALID_VALUE
    assert patch(codecs=(p, p, p), policy=1, wb=msize - 1) == HIP_INVALID_VALUE
    assert patch(base=null, wb=wsize - 1) == HIP_INVALID_VALUE, "a null base is no refusal by itself"
    assert all(x == GUARD for x in a) and all(x == GUARD for x in bytes(room)) and all(x == GUARD for x in bytes(sroom)), "nothing is written"


def test_python_refusals_in_front_of_any_launch():
    import torch
    from finitestateentropy_amd import api
    hip = api.FseHip.__new__(api.FseHip)                          # (no launch below: nothing here has a device)
    hip.lib = C.CDLL(os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so"))
    patch = hip.patch_tensor_windows_each
    got = patch(hip.compress_tensors_each([], segment_log=18), [], [])
    assert got.transforms == [] and got.segment_log == 18 and got.groups == []
    with pytest.raises(ValueError, match="not segmented"):
        patch(hip.compress_tensors_each([]), [], [])
    held = api.CompressedTensors([], [torch.float32], [(8,)], None, 0, 5)
    held.segment_log = 18
    t = torch.zeros(8)
    for ts, ws in (([], [(0, 1)]), ([t, t], [(0, 1)]), ([t], []), ([t], [(0, 1), (0, 1)])):
        with pytest.raises(ValueError, match="tensors|windows"):
            patch(held, ts, ws)
    for w in ([(3, 2)], [(0, 9)], [(-1, 2)], [(0.0, 1)], [5], [(0, 1, 2)]):
        with pytest.raises(ValueError, match="window"):
            patch(held, [t], w)
    for bad in (t, t.to(torch.float64), np.zeros(8, np.float32)):  # a CPU tensor, another dtype, no tensor
        with pytest.raises(TypeError):
            patch(held, [bad], [(0, 1)])
    held.sparse_permille = 500
    with pytest.raises(ValueError, match="sparse"):
        patch(held, [t], [(0, 1)])
    held.sparse_permille = None
    held.predictor = "next"
    with pytest.raises(ValueError, match="predictor"):
        patch(held, [t], [(0, 1)])
    held.predictor = "prev"
    with pytest.raises(ValueError, match="base"):
        patch(held, [t], [(0, 1)], base=[t])
    held.transforms = ["pred"]
    with pytest.raises(ValueError, match="predictor does not go"):
        patch(held, [t], [(0, 1)])
    held.predictor = None
    held.transforms = ["sub"]
    with pytest.raises(ValueError, match="needs its base"):
        patch(held, [t], [(0, 1)])
    held.transforms = ["pred"]
    with pytest.raises(ValueError, match="does not belong"):
        patch(held, [t], [(0, 1)], base=[t])
    for bad in (["delta"], ["plain", "pred"], [], [1]):
        held.transforms = bad
        with pytest.raises(ValueError, match="transforms"):
            patch(held, [t], [(0, 1)])
    held.transforms = None
    with pytest.raises(ValueError, match="no deltas"):
        patch(held, [t], [(0, 1)], base=[t])
    held.delta = True
    with pytest.raises(ValueError, match="needs its base"):
        patch(held, [t], [(0, 1)])
    # the old name keeps refusing each-objects and predicted objects, as it did
    each = hip.compress_tensors_each([], segment_log=18)
    with pytest.raises(ValueError, match="patches are not supported"):
        hip.patch_tensor_windows(each, [], [])
    pred = api.CompressedTensors([], [], [], None, api.PredictedPlanes(0), 5)
    pred.segment_log, pred.predictor = 18, "prev"
    with pytest.raises(ValueError, match="patches are not supported"):
        hip.patch_tensor_windows(pred, [], [])

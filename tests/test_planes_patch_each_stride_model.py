"""Patching tensors with a stride per tensor without a device (include/fsehip.h, "windows and patches of tensors with a stride per tensor"): the
patch's claim on the numpy model (planes_window_each_stride_corpus.py) -- the planes of the strided transform of a sub-tensor that starts on a
run are segments k0 .. k1 of the planes of the strided transform of the tensor, and a change inside the window leaves every plane byte outside
the selected segments as it was --, the stage model's refusals, the argument refusals of the two writing C calls (host memory: decided before
any device call, nothing written) and the Python surface in front of any launch."""
import ctypes as C
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_patch_corpus as ppc
import planes_patch_each_corpus as ppe
import planes_stride_corpus as psc
import planes_window_each_stride_corpus as pws
from planes_each_corpus import IDS, PLAIN, PRED, SUB, XOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI, I = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint, C.c_int
SEG_LOG = 10


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(LIB)


def _tensor(rng, m, E, tail):
    t = rng.integers(0, 256, m * E + tail, dtype=np.uint8)
    if m:                                                       # a smooth half: small differences
        x = (np.cumsum(rng.integers(-2, 3, m)) + 300).astype("<u8")
        t[:m // 2 * E] = np.ascontiguousarray(x.view(np.uint8).reshape(-1, 8)[:m // 2, :E]).reshape(-1)
    return t


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_planes_of_the_sub_tensor_are_the_segments_of_the_planes_of_the_tensor(E):
    """the patch's claim, for every stride, every window between the ends, tensor sizes with and without a partial last element"""
    rng = np.random.default_rng(370 + E)
    for m in (0, 1, 7, 17, 1023, 1033, 2051, 3100):
        for tail in {0, E - 1}:
            t = _tensor(rng, m, E, tail)
            for S in (1,) + pws.STRIDES:
                for a, c in pws.window_set(m, S):
                    want = pws.segment_slices(t, None, E, PRED, S, a, c, SEG_LOG)
                    got = pws.sub_planes(t, None, E, PRED, S, a, c, SEG_LOG)
                    assert len(want) == len(got) == E and all(w.shape == g.shape and (w == g).all() for w, g in zip(want, got)), (m, tail, S, a, c)
    t, b = _tensor(rng, 2051, E, 0), rng.integers(0, 256, 2051 * E, dtype=np.uint8)
    for tr in (PLAIN, XOR, SUB):                                # the other three, whatever the stride byte: those of planes_patch_each_corpus.py
        for a, c in pws.window_set(2051, 5):
            want = ppe.segment_slices(t, b, E, tr, a, c, SEG_LOG)
            assert all((w == g).all() for w, g in zip(want, pws.sub_planes(t, b, E, tr, 0xFF, a, c, SEG_LOG)))


@pytest.mark.parametrize("E", pc.ELEMS)
def test_a_change_inside_the_window_leaves_the_planes_outside_the_selected_segments(E):
    """old and new differ inside [a, b) only => their strided planes differ inside segments k0 .. k1 only: the differences at b .. b + S - 1
    read the elements b - S .. b - 1, and each of them lies in a selected segment or is a chain head of the next run"""
    rng = np.random.default_rng(380 + E)
    s = 1 << SEG_LOG
    for m in (17, 1033, 2051, 3100):
        old = _tensor(rng, m, E, E - 1)
        for S in pws.STRIDES:
            for a, c in pws.window_set(m, S):
                new = old.copy()
                new[a * E:c * E] ^= rng.integers(1, 256, (c - a) * E, dtype=np.uint8)
                at, n = ppc.sub_range(len(old), a, c, E, SEG_LOG)
                k0 = at // E
                assert k0 % s == 0
                po, pn = pws.whole_planes(old, None, E, PRED, S), pws.whole_planes(new, None, E, PRED, S)
                for p in range(E):
                    hi = k0 + pc.plane_size(n, p, E)
                    assert (po[p][:k0] == pn[p][:k0]).all() and (po[p][hi:] == pn[p][hi:]).all(), (m, S, a, c, p)


def test_a_sub_tensor_off_a_run_start_would_be_wrong():
    """the model told apart from a split that cuts anywhere: the chains of a sub-tensor that starts S elements behind a run start are not the
    tensor's -- the patch is right because a segment starts a run, for every chain"""
    E, m, S = 2, 3000, 3
    t = np.random.default_rng(4).integers(1, 256, m * E, dtype=np.uint8)
    whole = pws.whole_planes(t, None, E, PRED, S)
    for cut in (1, S, 1023, 1024 + S):
        sub = pc.planes_of(psc.forward(t[cut * E:], E, S), E)
        assert any((sub[p] != whole[p][cut:]).any() for p in range(E)), cut
    for cut in (0, 1024, 2048):
        sub = pc.planes_of(psc.forward(t[cut * E:], E, S), E)
        assert all((sub[p] == whole[p][cut:]).all() for p in range(E)), cut


def test_the_stage_model_refuses_by_rule_1():
    E = 2
    rng = np.random.default_rng(9)
    tensors = [rng.integers(0, 256, 2 * 1500, dtype=np.uint8) for _ in range(4)]
    windows = [(5, 1030), (0, 0), (1024, 1500), (1023, 1024)]
    tr = [PRED, SUB, PRED, PLAIN]
    good = pws.stage_model(tensors, windows, E, SEG_LOG, tr, [3, 0, 8, 0xFF], bases=tensors[::-1])
    assert good[3] == [2 * 1500, 0, 2 * 476, 2 * 1024]
    ones = pws.stage_model(tensors, windows, E, SEG_LOG, tr, [1, 1, 1, 1], bases=tensors[::-1])
    same = ppe.stage_each_model(tensors, windows, E, SEG_LOG, tr, bases=tensors[::-1])
    assert (ones[0] == same[0]).all() and ones[2:] == same[2:], "stride 1 everywhere is the model of the _window_each_ split"
    assert (good[0] != ones[0]).any()
    T = ppc.stage_offsets([len(t) for t in tensors], windows, E, SEG_LOG)
    for st, bad in (([0, 0, 8, 0], (0,)), ([3, 9, 9, 9], (2,)), ([0xFF, 1, 0, 1], (0, 2))):
        out, written, P, res = pws.stage_model(tensors, windows, E, SEG_LOG, tr, st, bases=tensors[::-1])
        for i in range(4):
            if i in bad:
                assert res[i] == pc.GENERIC and P[i * E:(i + 1) * E] == [T[i]] * E and not written[T[i]:T[i + 1]].any()
            else:
                assert res[i] == good[3][i] and written[T[i]:T[i + 1]].all()


# ---------------------------------------------------------------------------------------------------------------- the library
def test_every_argument_refusal_of_the_writing_calls_without_a_device(lib):
    need = lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize
    need.restype = SZ
    bound = lib.FSEHIP_planes_spliceScratchBound
    bound.restype = SZ
    mixed = lib.FSEHIP_frame_mixedWorkspaceBound
    mixed.restype = SZ
    n, nseg, nsel, blocks = 1, 4, 2, 4
    wsize, ssize = need(SZ(nsel), SZ(blocks), UI(0), I(0)), bound(SZ(n), UI(2), SZ(nseg))
    msize = mixed(SZ(nsel), SZ(blocks), UI(0), I(1))
    GUARD = 0xF9
    a = (C.c_uint8 * 256)(*([GUARD] * 256))                     # stands for every array
    big = max(wsize, msize)
    room = (C.c_uint8 * (big + 512))(*([GUARD] * (big + 512)))
    sroom = (C.c_uint8 * (ssize + 512))(*([GUARD] * (ssize + 512)))
    p, null = C.cast(a, VP), VP(0)
    ws, sc = VP((C.addressof(room) + 255) & ~255), VP((C.addressof(sroom) + 255) & ~255)

    # ---- the split: stage, plane offsets, results, src, base, transforms, strides, src offsets, windows, stage offsets
    def split(q=None, E=2, seg_log=10, n=1, cap=8, scap=8):
        q = list(q or [p] * 10)
        return lib.FSEHIP_planes_split_window_each_stride_dbatch(*q, SZ(n), UI(E), UI(seg_log), U64(cap), U64(scap), null)
    for strides in (p, null):                                   # (a NULL d_strides is no refusal)
        for k in range(10):
            if k not in (4, 6):                                 # (the base and the strides may be NULL: those calls would launch)
                assert split([null if x == k else strides if x == 6 else p for x in range(10)]) == HIP_INVALID_VALUE, k
    for bad in (0, 3, 5, 16, 0xFFFFFFFF):
        assert split(E=bad) == HIP_INVALID_VALUE, bad
    for seg_log in (0, 9, 31, 40):
        assert split(seg_log=seg_log) == HIP_INVALID_VALUE, seg_log
    assert split(n=1 << 30) == HIP_INVALID_VALUE, "2^31 planes"
    assert split(scap=1 << 46) == HIP_INVALID_VALUE and split(scap=32768 << 24) == HIP_INVALID_VALUE and split(n=1 << 24, E=1) == HIP_INVALID_VALUE, "the launch limit"

    # ---- the composite
    names = ("out", "ooff", "ores", "tres", "frames", "foff", "fres", "src", "tr", "soff", "win", "sf", "wf", "toff", "stage", "spo", "sso", "sres", "new", "noff", "nres")

    def patch(E=2, seg_log=10, n=n, nseg=nseg, nsel=nsel, blocks=blocks, bsid=0, codec=0, policy=0, tol=0, align=0, ocap=8, scap=8, base=p, st=p,
              codecs=(null, null, null), s=sc, sb=ssize, w=ws, wb=wsize, **nulls):
        assert set(nulls) <= set(names)
        q = {k: null if k in nulls else p for k in names}
        ocod, cod, ncod = codecs
        return lib.FSEHIP_tensor_patch_window_each_stride_dbatch(
            q["out"], U64(ocap), q["ooff"], q["ores"], ocod, q["tres"], q["frames"], U64(8), q["foff"], q["fres"], cod, q["src"], base, q["tr"], st, q["soff"], U64(8),
            q["win"], SZ(n), UI(E), q["sf"], SZ(nseg), UI(seg_log), q["wf"], SZ(nsel), q["toff"], U64(scap), SZ(blocks), UI(bsid), I(codec), ncod, I(policy), UI(tol),
            UI(align), q["stage"], q["spo"], q["sso"], q["sres"], q["new"], U64(8), q["noff"], q["nres"], s, SZ(sb), w, SZ(wb), null)
    for st in (p, null):
        for name in names:                                      # null pointers, d_transforms among them
            assert patch(st=st, **{name: True}) == HIP_INVALID_VALUE, name
    for E in (0, 3, 5, 16, 0xFFFFFFFF):
        assert patch(E=E) == HIP_INVALID_VALUE, E
    for seg_log in (0, 9, 31, 40):
        assert patch(seg_log=seg_log) == HIP_INVALID_VALUE, seg_log
    assert patch(seg_log=10, bsid=1) == HIP_INVALID_VALUE and patch(bsid=7, seg_log=20) == HIP_INVALID_VALUE
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
    assert patch(codecs=(p, null, null)) == HIP_INVALID_VALUE and patch(codecs=(null, p, null)) == HIP_INVALID_VALUE and patch(codecs=(null, null, p)) == HIP_INVALID_VALUE
    assert patch(codecs=(p, p, p), policy=2, wb=msize) == HIP_INVALID_VALUE and patch(codecs=(p, p, p), policy=1, tol=1001, wb=msize) == HIP_INVALID_VALUE
    assert patch(base=null, st=null, wb=wsize - 1) == HIP_INVALID_VALUE, "a null base and null strides are no refusal by themselves"
    assert all(x == GUARD for x in a) and all(x == GUARD for x in bytes(room)) and all(x == GUARD for x in bytes(sroom)), "nothing is written"


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_python_refusals_in_front_of_any_launch(monkeypatch):
    import torch
    from finitestateentropy_amd import api
    hip = api.FseHip.__new__(api.FseHip)                          # (no launch below: nothing here has a device)
    hip.lib = C.CDLL(LIB)

    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in ("FSEHIP_tensor_patch_window_each_stride_dbatch", "FSEHIP_planes_split_window_each_stride_dbatch", "FSEHIP_tensor_patch_window_each_dbatch",
                 "FSEHIP_tensor_patch_window_dbatch"):
        monkeypatch.setattr(hip.lib, name, no_launch, raising=False)
    patch = hip.patch_tensor_windows_each_stride
    got = patch(hip.compress_tensors_each([], strides=(1, 2, 3), segment_log=18), [], [])
    assert got.transforms == [] and got.strides == [] and got.segment_log == 18 and got.groups == []
    got = patch(hip.compress_tensors_each([], segment_log=18), [], [])
    assert got.transforms == [] and getattr(got, "strides", None) is None
    with pytest.raises(ValueError, match="not segmented"):
        patch(hip.compress_tensors_each([], strides=(1, 2)), [], [])
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
    for bad in ("next", "prev0", "prev1", "prev9"):
        held.predictor = bad
        with pytest.raises(ValueError, match="predictor"):
            patch(held, [t], [(0, 1)])
    held.predictor = "prev4"
    with pytest.raises(ValueError, match="base"):
        patch(held, [t], [(0, 1)], base=[t])
    held.predictor = None
    held.transforms = ["pred"]
    for bad in ([0], [9], [True], [2.0], [1, 2], []):
        held.strides = bad
        with pytest.raises(ValueError, match="stride"):
            patch(held, [t], [(0, 1)])
    held.strides = [4]
    with pytest.raises(ValueError, match="does not belong"):
        patch(held, [t], [(0, 1)], base=[t])
    held.transforms = ["sub"]
    with pytest.raises(ValueError, match="needs its base"):
        patch(held, [t], [(0, 1)])
    for bad in (["delta"], ["plain", "pred"], [], [1]):
        held.transforms = bad
        with pytest.raises(ValueError, match="transforms"):
            patch(held, [t], [(0, 1)])
    # the old functions keep refusing an object that holds a stride above 1
    held.transforms, held.strides = ["pred"], [4]
    with pytest.raises(ValueError, match="stride above 1"):
        hip.patch_tensor_windows_each(held, [t], [(0, 1)])
    with pytest.raises(ValueError, match="patches are not supported"):
        hip.patch_tensor_windows(held, [t], [(0, 1)])

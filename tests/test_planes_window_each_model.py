"""Windows of tensors with a transform per tensor without a device (include/fsehip.h, the section of that name): the numpy model of the
window merge (planes_window_each_corpus.py) against the slice of the whole inverse, the shapes the merge test's corpus must hold, the
library's exports and Python names, and every argument refusal of the two C calls, decided before any device call with nothing written
(the pointers are host memory)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_each_corpus as pe
import planes_pred_corpus as ppc
import planes_window_each_corpus as pwe
from planes_each_corpus import IDS, PRED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint
TWO = ("FSEHIP_planes_merge_window_each_dbatch", "FSEHIP_tensor_decompress_window_each_dbatch")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_window_model_is_the_slice_of_the_whole_inverse(E):
    rng = np.random.default_rng(70 + E)
    for m in (0, 1, 15, 17, 1023, 1025, 2048, 2051, 3100):
        for tail in {0, E - 1}:                                 # trailing n mod E bytes: never part of a window
            t, b = (rng.integers(0, 256, m * E + tail, dtype=np.uint8) for _ in range(2))
            if m:                                               # a smooth half: small differences
                x = (np.cumsum(rng.integers(-2, 3, m)) + 300).astype("<u8")
                t[:m // 2 * E] = np.ascontiguousarray(x.view(np.uint8).reshape(-1, 8)[:m // 2, :E]).reshape(-1)
            for tr in IDS:
                planes = pwe.whole_planes(t, b, E, tr)
                whole = pe.inverse(pc.merge_one(planes, E), b, E, tr)
                assert (whole == t).all()
                for a, c in pwe.window_set(m):
                    got = pwe.window_merge_model(planes, b[a * E:c * E], E, tr, a, c)
                    assert got.size == (c - a) * E and (got == whole[a * E:c * E]).all(), (m, tr, a, c)


def test_a_window_without_its_lead_is_wrong():
    """the model told apart from the merge that forgets the lead: inverting a PRED window from a instead of from the run's start"""
    E, m = 2, 3000
    t = np.random.default_rng(3).integers(1, 256, m * E, dtype=np.uint8)
    planes = pwe.whole_planes(t, None, E, PRED)
    for a, b in ((1, 40), (1023, 1030), (1025, 2050)):
        naive = ppc.inverse(pc.merge_one([p[a:b] for p in planes], E), E)
        assert (naive != t[a * E:b * E]).any() and (pwe.window_merge_model(planes, None, E, PRED, a, b) == t[a * E:b * E]).all()
    assert [pwe.lead(PRED, a, b) for a, b in ((0, 5), (1, 5), (1023, 1024), (1024, 1025), (2047, 2051), (7, 7))] == [0, 1, 1023, 0, 1023, 0]
    assert all(pwe.lead(tr, 1023, 2000) == 0 for tr in IDS if tr != PRED)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_corpus_holds_the_shapes_the_merge_test_needs(E):
    c = pwe.merge_corpus(E)
    missing = [name for name, held in pwe.shapes(c, E).items() if not held]
    assert not missing, missing
    assert all(a in pwe.ends(m) and b in pwe.ends(m) and a <= b for (a, b), m in zip(c["windows"], c["counts"]))
    assert all(len(t) // E == m and len(t) == len(b) for t, b, m in zip(c["tensors"], c["bases"], c["counts"]))
    # the extra tile of the work mapping: a virtual tensor that needs one tile more than its slot has items without the doubled count
    T = pc.TILE
    n, L, D0 = T - 1, 1023, 0
    items = (D0 + n) // T - D0 // T + 1
    assert items == 1 and -(-(n + L) // T) == 2 and (D0 + n) // T - D0 // T + 2 >= -(-(n + L) // T)
    for E2 in pc.ELEMS:                                         # ... and one more is always enough: L E < T
        assert 1023 * E2 < T


def test_the_merge_verdict_model():
    E = 2
    ok = dict(tr=PRED, has_base=False, a=5, b=9, E=E, plane_sizes=[4, 4], plane_offsets=[5, 100], slot=8)
    assert pwe.merge_verdict(**ok) == 8
    assert pwe.merge_verdict(**{**ok, "plane_offsets": [4, 100]}) == pc.GENERIC, "the lead in front of the planes buffer"
    assert pwe.merge_verdict(**{**ok, "tr": pe.PLAIN, "plane_offsets": [0, 0]}) == 8
    assert pwe.merge_verdict(**{**ok, "a": 9, "b": 5}) == pc.GENERIC and pwe.merge_verdict(**{**ok, "b": 10}) == pc.GENERIC
    assert pwe.merge_verdict(**{**ok, "tr": pe.XOR}) == pc.GENERIC and pwe.merge_verdict(**{**ok, "tr": 0xFF, "has_base": True}) == pc.GENERIC
    assert pwe.merge_verdict(**{**ok, "slot": 7}) == pc.TOO_SMALL and pwe.merge_verdict(**{**ok, "plane_sizes": [4, 5]}) == pc.CORRUPT
    assert pwe.merge_verdict(**{**ok, "a": 1023, "b": 1023, "plane_sizes": [0, 0], "plane_offsets": [0, 0]}) == 0, "an empty window has no lead"


# ---------------------------------------------------------------------------------------------------------------- the library
def test_exports_and_python_names(lib):
    """fails on the parent commit: none of these exists there"""
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    for name in TWO:
        getattr(lib, name)
        assert name in header, name
    declared = set(__import__("re").findall(r"\b(FSEHIP_\w+_workspace(?:Size|Bound|Head))\s*\(", header))
    assert not any("window_each" in d for d in declared), "no workspace function of its own: the packed reader's"
    import finitestateentropy_amd
    from finitestateentropy_amd import api
    assert "decompress_tensor_windows_each" in finitestateentropy_amd.__all__
    assert finitestateentropy_amd.decompress_tensor_windows_each is api.decompress_tensor_windows_each
    for name in ("planes_merge_window_each_dbatch", "tensor_decompress_window_each_dbatch", "decompress_tensor_windows_each"):
        assert callable(getattr(api.FseHip, name)), name
    assert list(inspect.signature(api.decompress_tensor_windows_each).parameters) == ["obj", "windows", "base"]
    assert list(inspect.signature(api.decompress_tensor_windows).parameters) == ["obj", "windows", "base"], "unchanged"
    old = inspect.signature(api.FseHip.tensor_decompress_window_dbatch).parameters
    new = inspect.signature(api.FseHip.tensor_decompress_window_each_dbatch).parameters
    assert [k for k in new if k != "transforms"] == [k for k in old if k != "delta_op"], "the window call's arguments, transforms for the op"


def test_every_argument_refusal_without_a_device(lib):
    need = lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    need.restype = SZ
    nsel, blocks = 2, 4
    wsize = need(SZ(nsel), SZ(blocks))
    assert 1 < wsize < (1 << 28)
    GUARD = 0xF9
    a = (C.c_uint8 * 256)(*([GUARD] * 256))                     # stands for every array
    room = (C.c_uint8 * (wsize + 512))(*([GUARD] * (wsize + 512)))
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)

    def merge(q=None, E=2, n=1, cap=8):           # q: dst, dst offsets, results, planes, plane offsets, plane sizes, base, transforms, windows
        q = list(q or [p] * 9)
        return lib.FSEHIP_planes_merge_window_each_dbatch(*q, SZ(n), UI(E), U64(cap), null)

    for k in range(9):
        if k != 6:                                             # (the base may be NULL: that call would launch, it is not made here)
            assert merge([null if x == k else p for x in range(9)]) == HIP_INVALID_VALUE, k
    for bad in (0, 3, 5, 16, 0xFFFFFFFF):
        assert merge(E=bad) == HIP_INVALID_VALUE, bad
    assert merge(n=1 << 30) == HIP_INVALID_VALUE, "2^31 planes"
    assert merge(cap=1 << 46) == HIP_INVALID_VALUE and merge(cap=32768 << 24) == HIP_INVALID_VALUE
    # the launch limit with the DOUBLED tensor count: 2^23 tensors are 2^23 + 1 workgroups for the merge, 2^24 + 1 for the window form
    assert merge(n=1 << 23, E=1) == HIP_INVALID_VALUE and merge(n=(1 << 23) - 1, E=1, cap=2 * 32768) == HIP_INVALID_VALUE
    names = ("dst", "doff", "tr", "res", "frames", "foff", "soff", "win", "sf", "wf", "planes", "sfo", "so", "sres", "poff", "psz")

    def window(E=2, seg_log=10, n=1, nseg=4, nsel=nsel, blocks=blocks, cap=8, base=p, w=ws, wb=wsize, **nulls):
        assert set(nulls) <= set(names)
        q = {k: null if k in nulls else p for k in names}
        return lib.FSEHIP_tensor_decompress_window_each_dbatch(
            q["dst"], q["doff"], U64(cap), base, q["tr"], q["res"], q["frames"], q["foff"], q["soff"], q["win"], SZ(n), UI(E), q["sf"], SZ(nseg), UI(seg_log), q["wf"],
            SZ(nsel), SZ(blocks), q["planes"], U64(8), q["sfo"], q["so"], q["sres"], q["poff"], q["psz"], w, SZ(wb), null)

    for name in names:                                          # null pointers, d_transforms among them
        assert window(**{name: True}) == HIP_INVALID_VALUE, name
    for E in (0, 3, 5, 16, 0xFFFFFFFF):
        assert window(E=E) == HIP_INVALID_VALUE, E
    for seg_log in (0, 9, 31, 40):
        assert window(seg_log=seg_log) == HIP_INVALID_VALUE, seg_log
    assert window(nseg=4, nsel=5, wb=need(SZ(5), SZ(blocks))) == HIP_INVALID_VALUE, "more selected frames than frames"
    for big in (1 << 31, 1 << 40):
        assert window(nseg=big) == HIP_INVALID_VALUE and window(blocks=big) == HIP_INVALID_VALUE
    assert window(n=1 << 30) == HIP_INVALID_VALUE, "2^31 planes"
    assert window(wb=wsize - 1) == HIP_INVALID_VALUE and window(wb=0) == HIP_INVALID_VALUE and window(w=null, wb=0) == HIP_INVALID_VALUE, "a short reader workspace"
    assert window(w=VP(ws.value + 128)) == HIP_INVALID_VALUE, "a misaligned workspace"
    assert window(cap=1 << 46) == HIP_INVALID_VALUE and window(cap=32768 << 24) == HIP_INVALID_VALUE, "a capacity the merge cannot launch for"
    assert window(n=1 << 23, E=1) == HIP_INVALID_VALUE, "the launch limit with the doubled tensor count"
    assert window(base=null, wb=wsize - 1) == HIP_INVALID_VALUE, "a null base is no refusal by itself"
    assert all(x == GUARD for x in a) and all(x == GUARD for x in bytes(room)), "nothing is written"


def test_python_refusals_in_front_of_any_launch(monkeypatch):
    from finitestateentropy_amd import api
    hip = api.FseHip.__new__(api.FseHip)                          # (no launch below: nothing here has a device)
    hip.lib = C.CDLL(os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so"))
    read = hip.decompress_tensor_windows_each
    assert read(hip.compress_tensors_each([], segment_log=18), []) == []
    with pytest.raises(ValueError, match="not segmented"):
        read(hip.compress_tensors_each([]), [])
    held = api.CompressedTensors([], [None], [(8,)], None, 0, 5)
    held.segment_log = 18
    for w in ([], [(0, 1), (0, 1)], [(3, 2)], [(0, 9)], [(-1, 2)], [(0.0, 1)], [5], [(0, 1, 2)]):
        with pytest.raises(ValueError):
            read(held, w)
    held.sparse_permille = 500
    with pytest.raises(ValueError, match="sparse"):
        read(held, [(0, 1)])
    held.sparse_permille = None
    held.predictor = "next"
    with pytest.raises(ValueError, match="predictor"):
        read(held, [(0, 1)])
    held.predictor = "prev"
    with pytest.raises(ValueError, match="base"):
        read(held, [(0, 1)], base=[None])
    held.predictor = None
    held.transforms = ["sub"]
    with pytest.raises(ValueError, match="needs its base"):
        read(held, [(0, 1)])
    held.transforms = ["pred"]
    with pytest.raises(ValueError, match="does not belong"):
        read(held, [(0, 1)], base=[None])
    for bad in (["delta"], ["plain", "pred"], []):
        held.transforms = bad
        with pytest.raises(ValueError):
            read(held, [(0, 1)])
    held.transforms = None
    with pytest.raises(ValueError, match="no deltas"):
        read(held, [(0, 1)], base=[None])
    held.delta = True
    with pytest.raises(ValueError, match="needs its base"):
        read(held, [(0, 1)])
    # the old name keeps refusing, and says where to go
    each = hip.compress_tensors_each([], segment_log=18)
    with pytest.raises(ValueError, match="decompress_tensor_windows_each"):
        hip.decompress_tensor_windows(each, [])
    with pytest.raises(ValueError, match="patches are not supported"):
        hip.patch_tensor_windows(each, [], [])

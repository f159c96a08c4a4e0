"""Windows of tensors with a stride per tensor without a device (include/fsehip.h, "windows and patches of tensors with a stride per tensor"):
the numpy model (planes_window_each_stride_corpus.py) against the slice of the tensor for every element size and stride, the shapes the merge
test's corpus must hold, the work mapping's one extra tile, the verdict rules with the stride's refusal, the library's exports and prototypes,
the argument refusals of the two reading C calls (the pointers are host memory: decided before any device call, nothing written) and the
Python surface in front of any launch."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import planes_corpus as pc
import planes_each_stride_corpus as pes
import planes_stride_corpus as psc
import planes_window_each_corpus as pwe
import planes_window_each_stride_corpus as pws
from planes_each_corpus import IDS, PLAIN, PRED, SUB, XOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint
FOUR = ("FSEHIP_planes_merge_window_each_stride_dbatch", "FSEHIP_tensor_decompress_window_each_stride_dbatch", "FSEHIP_planes_split_window_each_stride_dbatch",
        "FSEHIP_tensor_patch_window_each_stride_dbatch")
LIB = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(LIB)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_window_model_is_the_slice_of_the_tensor(E):
    """every stride 1 .. 8, every window between the ends, tensor sizes around a chunk and around one and two runs, with and without a partial
    last element; the other three transforms are those of planes_window_each_corpus.py whatever the stride byte holds"""
    rng = np.random.default_rng(270 + E)
    for m in (1, 7, 17, 1023, 1033, 2051):
        for tail in {0, E - 1}:
            t, b = rng.integers(0, 256, m * E + tail, dtype=np.uint8), rng.integers(0, 256, m * E + tail, dtype=np.uint8)
            for S in (1,) + pws.STRIDES:
                planes = pws.whole_planes(t, b, E, PRED, S)
                assert (pes.merge_each_stride_one(planes, b, E, PRED, S) == t).all()
                for a, c in pws.window_set(m, S):
                    got = pws.window_merge_model(planes, None, E, PRED, S, a, c)
                    assert got.shape == ((c - a) * E,) and (got == t[a * E:c * E]).all(), (m, tail, S, a, c)
            for tr in (PLAIN, XOR, SUB):
                planes = pws.whole_planes(t, b, E, tr, 0xFF)
                for a, c in pws.window_set(m, 3):
                    assert (pws.window_merge_model(planes, b[a * E:c * E], E, tr, 0, a, c) == t[a * E:c * E]).all(), (m, tail, tr, a, c)


def test_the_lead_must_be_summed_chain_by_chain():
    """the model told apart from two wrong ones: stride 1 over strided planes, and chains counted from the window's start"""
    E, S, m = 2, 3, 2051
    t = np.random.default_rng(5).integers(1, 256, m * E, dtype=np.uint8)
    planes = pws.whole_planes(t, None, E, PRED, S)
    for a, c in ((1025, 1100), (5, 900), (1023, 1024)):
        want = t[a * E:c * E]
        assert (pws.window_merge_model(planes, None, E, PRED, S, a, c) == want).all()
        assert (pws.window_merge_model(planes, None, E, PRED, 1, a, c) != want).any(), "stride 1 is another transform"
        cut = psc.inverse(pc.merge_one([p[a:c] for p in planes], E), E, S)
        assert (cut != want).any(), "without the lead the chains start with the wrong sums"
    assert [pws.lead(PRED, a, b) for a, b in ((0, 5), (2, 5), (1023, 1024), (1024 + 7, 1040), (7, 7))] == [0, 2, 1023, 7, 0]


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_corpus_holds_the_shapes_the_merge_test_needs(E):
    c = pws.merge_corpus(E)
    missing = [name for name, held in pws.shapes(c, E).items() if not held]
    assert not missing, missing
    assert all(len(t) // E == m and len(t) == len(b) for t, b, m in zip(c["tensors"], c["bases"], c["counts"]))
    assert all(0 <= a <= b <= m for (a, b), m in zip(c["windows"], c["counts"]))


def _items(D, n_tensors, capacity, i):
    """the workgroups that the window key floor(D[j] / T) + 2 j gives tensor i out of the ceil(capacity / T) + 2 nTensors that are launched"""
    T = pc.TILE
    key = [D[j] // T + 2 * j for j in range(n_tensors)]
    grid = -(-capacity // T) + 2 * n_tensors
    return (key[i + 1] if i + 1 < n_tensors else grid) - key[i]


def test_the_virtual_tensor_needs_at_most_one_tile_beyond_the_plain_items():
    T = pc.TILE
    # the worst case: E = 1, D = 0, n = T - 1, L = 1023 -- one item under the plain key, two tiles
    n, L, E = T - 1, 1023, 1
    assert n // T + 1 == 1 and -(-(n + L * E) // T) == 2
    assert _items([0, n], 1, n, 0) >= 2
    # ... followed by another tensor, whose key lies two further on: exactly the two
    assert _items([0, n, n + 5], 2, n + 5, 0) == 2 and _items([0, n, n + 5], 2, n + 5, 1) >= 1
    assert all(1023 * E2 < T for E2 in pc.ELEMS), "L E < T: one more tile is always enough"
    for E in pc.ELEMS:                                          # every tensor of the corpus has the items its virtual tensor needs
        c = pws.merge_corpus(E)
        D, w, tr = c["D"], c["windows"], c["transforms"]
        cnt = len(w)
        for i, (a, b) in enumerate(w):
            need = -(-(E * (b - a + pws.lead(tr[i], a, b))) // T)
            assert _items(D, cnt, D[-1], i) >= need, (E, i)


def test_the_merge_verdict_model():
    E = 2
    ok = dict(tr=PRED, st=3, has_base=False, a=5, b=9, E=E, plane_sizes=[4, 4], plane_offsets=[5, 100], slot=8)
    assert pws.merge_verdict(**ok) == 8
    for st in (0, 9, 0xFF):
        assert pws.merge_verdict(**{**ok, "st": st}) == pc.GENERIC, st
        for tr in (PLAIN, XOR, SUB):
            assert pws.merge_verdict(**{**ok, "tr": tr, "st": st, "has_base": True}) == 8, "the stride byte of another transform is not read"
    assert pws.merge_verdict(**{**ok, "plane_offsets": [4, 100]}) == pc.GENERIC, "the lead in front of the planes buffer, at every stride"
    assert pws.merge_verdict(**{**ok, "b": 10}) == pc.GENERIC and pws.merge_verdict(**{**ok, "a": 9, "b": 5}) == pc.GENERIC
    assert pws.merge_verdict(**{**ok, "slot": 7}) == pc.TOO_SMALL and pws.merge_verdict(**{**ok, "plane_sizes": [4, 5]}) == pc.CORRUPT
    assert pws.merge_verdict(**{**ok, "st": 1}) == pwe.merge_verdict(**{k: v for k, v in ok.items() if k != "st"}), "stride 1 is the model of the sibling"


# ---------------------------------------------------------------------------------------------------------------- the library
def _params(header, name):
    m = re.search(r"FSEHIP_API int %s\s*\(([^;]*)\);" % name, header)
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_prototypes_take_d_strides_behind_d_transforms():
    """fails on the parent commit: none of the four is declared there"""
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    assert "windows and patches of tensors with a stride per tensor" in header.lower()
    for new in FOUR:
        old = _params(header, new.replace("_each_stride_", "_each_"))
        k = old.index("const uint8_t* d_transforms")
        assert _params(header, new) == old[:k + 1] + ["const uint8_t* d_strides"] + old[k + 1:], new


def test_exports_and_python_names(lib):
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    for name in FOUR:
        getattr(lib, name)
    declared = set(re.findall(r"\b(FSEHIP_\w+_workspace(?:Size|Bound|Head))\s*\(", header))
    assert not any("window_each" in d for d in declared), "no workspace function of their own"
    import finitestateentropy_amd
    from finitestateentropy_amd import api
    for name, args in (("decompress_tensor_windows_each_stride", ["obj", "windows", "base"]), ("patch_tensor_windows_each_stride", ["obj", "tensors", "windows", "base"])):
        assert name in finitestateentropy_amd.__all__ and getattr(finitestateentropy_amd, name) is getattr(api, name)
        assert callable(getattr(api.FseHip, name)) and list(inspect.signature(getattr(api, name)).parameters) == args
    for name in FOUR:
        py = name[len("FSEHIP_"):]
        new = list(inspect.signature(getattr(api.FseHip, py)).parameters)
        old = [k for k in inspect.signature(getattr(api.FseHip, py.replace("_each_stride_", "_each_"))).parameters if not k.startswith("_")]
        k = old.index("transforms")
        assert new == old[:k + 1] + ["strides"] + old[k + 1:], py
        assert inspect.signature(getattr(api.FseHip, py)).parameters["strides"].default is None


def test_every_argument_refusal_of_the_reading_calls_without_a_device(lib):
    need = lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    need.restype = SZ
    nsel, blocks = 2, 4
    wsize = need(SZ(nsel), SZ(blocks))
    GUARD = 0xF9
    a = (C.c_uint8 * 256)(*([GUARD] * 256))                     # stands for every array
    room = (C.c_uint8 * (wsize + 512))(*([GUARD] * (wsize + 512)))
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)

    def merge(q=None, E=2, n=1, cap=8):           # q: dst, dst offsets, results, planes, plane offsets, plane sizes, base, transforms, strides, windows
        q = list(q or [p] * 10)
        return lib.FSEHIP_planes_merge_window_each_stride_dbatch(*q, SZ(n), UI(E), U64(cap), null)
    for strides in (p, null):                                   # (a NULL d_strides is no refusal)
        for k in range(10):
            if k not in (6, 8):                                 # (the base and the strides may be NULL: those calls would launch)
                assert merge([null if x == k else strides if x == 8 else p for x in range(10)]) == HIP_INVALID_VALUE, k
    for bad in (0, 3, 5, 16, 0xFFFFFFFF):
        assert merge(E=bad) == HIP_INVALID_VALUE, bad
    assert merge(n=1 << 30) == HIP_INVALID_VALUE, "2^31 planes"
    assert merge(cap=1 << 46) == HIP_INVALID_VALUE and merge(cap=32768 << 24) == HIP_INVALID_VALUE
    assert merge(n=1 << 23, E=1) == HIP_INVALID_VALUE and merge(n=(1 << 23) - 1, E=1, cap=2 * 32768) == HIP_INVALID_VALUE, "the doubled tensor count"
    names = ("dst", "doff", "tr", "res", "frames", "foff", "soff", "win", "sf", "wf", "planes", "sfo", "so", "sres", "poff", "psz")

    def window(E=2, seg_log=10, n=1, nseg=4, nsel=nsel, blocks=blocks, cap=8, base=p, st=p, w=ws, wb=wsize, **nulls):
        assert set(nulls) <= set(names)
        q = {k: null if k in nulls else p for k in names}
        return lib.FSEHIP_tensor_decompress_window_each_stride_dbatch(
            q["dst"], q["doff"], U64(cap), base, q["tr"], st, q["res"], q["frames"], q["foff"], q["soff"], q["win"], SZ(n), UI(E), q["sf"], SZ(nseg), UI(seg_log),
            q["wf"], SZ(nsel), SZ(blocks), q["planes"], U64(8), q["sfo"], q["so"], q["sres"], q["poff"], q["psz"], w, SZ(wb), null)
    for st in (p, null):
        for name in names:
            assert window(st=st, **{name: True}) == HIP_INVALID_VALUE, name
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
    assert window(cap=1 << 46) == HIP_INVALID_VALUE and window(cap=32768 << 24) == HIP_INVALID_VALUE and window(n=1 << 23, E=1) == HIP_INVALID_VALUE
    assert window(base=null, st=null, wb=wsize - 1) == HIP_INVALID_VALUE, "a null base and null strides are no refusal by themselves"
    assert all(x == GUARD for x in a) and all(x == GUARD for x in bytes(room)), "nothing is written"


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def _trapped(monkeypatch):
    """a handle whose every FSEHIP_ device call is a failure of the test: what is raised below is raised in front of any launch"""
    from finitestateentropy_amd import api
    hip = api.FseHip.__new__(api.FseHip)
    hip.lib = C.CDLL(LIB)

    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in FOUR + tuple(n.replace("_each_stride_", "_each_") for n in FOUR) + ("FSEHIP_tensor_decompress_window_dbatch", "FSEHIP_tensor_patch_window_dbatch",
                                                                                   "FSEHIP_planes_select_window_dbatch", "FSEHIP_planes_fold_window_dbatch"):
        monkeypatch.setattr(hip.lib, name, no_launch, raising=False)
    return api, hip


def test_python_refusals_in_front_of_any_launch(monkeypatch):
    api, hip = _trapped(monkeypatch)
    read = hip.decompress_tensor_windows_each_stride
    assert read(hip.compress_tensors_each([], segment_log=18), []) == []
    assert read(hip.compress_tensors_each([], strides=(1, 2, 3), segment_log=18), []) == []
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
    for bad in ("next", "prev0", "prev1", "prev9", "prev22", 3):
        held.predictor = bad
        with pytest.raises(ValueError, match="predictor"):
            read(held, [(0, 1)])
    held.predictor = "prev3"
    with pytest.raises(ValueError, match="base"):
        read(held, [(0, 1)], base=[None])
    held.predictor = None
    held.transforms = ["pred"]
    for bad in ([0], [9], [True], [2.0], [1, 2], [], ["2"]):
        held.strides = bad
        with pytest.raises(ValueError, match="stride"):
            read(held, [(0, 1)])
    held.strides = [3]
    with pytest.raises(ValueError, match="does not belong"):
        read(held, [(0, 1)], base=[None])
    held.predictor = "prev3"
    with pytest.raises(ValueError, match="predictor does not go"):
        read(held, [(0, 1)])
    held.predictor = None
    held.transforms = ["sub"]
    with pytest.raises(ValueError, match="needs its base"):
        read(held, [(0, 1)])
    for bad in (["delta"], ["plain", "pred"], []):
        held.transforms = bad
        with pytest.raises(ValueError):
            read(held, [(0, 1)])
    held.transforms, held.strides = None, None
    with pytest.raises(ValueError, match="no deltas"):
        read(held, [(0, 1)], base=[None])


def test_the_old_functions_keep_refusing_strided_objects(monkeypatch):
    api, hip = _trapped(monkeypatch)
    import torch
    t = torch.zeros(8)
    held = api.CompressedTensors([], [torch.float32], [(8,)], None, 0, 5)
    held.segment_log, held.transforms, held.strides = 18, ["pred"], [3]
    with pytest.raises(ValueError, match="stride above 1"):
        hip.decompress_tensor_windows_each(held, [(0, 1)])
    with pytest.raises(ValueError, match="stride above 1"):
        hip.patch_tensor_windows_each(held, [t], [(0, 1)])
    for f, args in ((hip.decompress_tensor_windows, ([(0, 1)],)), (hip.patch_tensor_windows, ([t], [(0, 1)]))):
        with pytest.raises(ValueError):
            f(held, *args)
    pred = api.CompressedTensors([], [torch.float32], [(8,)], None, api.PredictedPlanes(0, stride=3), 5)
    pred.segment_log, pred.predictor = 18, "prev3"
    with pytest.raises(ValueError, match="only \"prev\" is known"):
        hip.decompress_tensor_windows_each(pred, [(0, 1)])
    with pytest.raises(ValueError, match="only \"prev\" is known"):
        hip.patch_tensor_windows_each(pred, [t], [(0, 1)])
    for f, args in ((hip.decompress_tensor_windows, ([(0, 1)],)), (hip.patch_tensor_windows, ([t], [(0, 1)]))):
        with pytest.raises(ValueError):
            f(pred, *args)
    assert "patch_tensor_windows_each_stride" in api.PredictedPlanes.__doc__ and "are refused" not in api.PredictedPlanes.__doc__

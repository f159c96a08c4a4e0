"""A transform per tensor without a device (include/fsehip.h, "a transform per tensor"): the dispatching model of planes_each_corpus.py as
a bijection and against the dedicated models it is made of, then the library's exports, the workspace head answered by host arithmetic,
every argument refusal of the six calls decided before any device call with nothing written (the pointers are host memory), and the
Python surface with the ValueErrors of the out-of-scope list."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_each_corpus as pe
import planes_pred_corpus as ppc
import planes_sub_corpus as psc
from planes_each_corpus import PLAIN, PRED, SUB, XOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
GIVEN, CHOOSE = 0, 1
SZ, VP, U64, UI, CI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint, C.c_int
SIX = ("FSEHIP_planes_split_each_dbatch", "FSEHIP_planes_merge_each_dbatch", "FSEHIP_tensor_compress_each_dbatch", "FSEHIP_tensor_decompress_each_dbatch",
       "FSEHIP_tensor_compress_seg_each_dbatch", "FSEHIP_tensor_decompress_seg_each_dbatch")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


# ---------------------------------------------------------------------------------------------------------------- the model
def _pairs(E, seed):
    rng = np.random.default_rng(seed)
    sizes = [0, 1, E, E + 1, 16 * E, 16 * E + E - 1 if E > 1 else 17, 1024 * E + 3, 2049 * E + (E > 1)]
    return [rng.integers(0, 256, n, dtype=np.uint8) for n in sizes], [rng.integers(0, 256, n, dtype=np.uint8) for n in sizes]


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_model_is_a_bijection(E):
    tensors, bases = _pairs(E, 40 + E)
    edge_t, edge_b = psc.edge_pairs(E)
    seq = ppc.edge_sequence(E, 15)
    tensors, bases = tensors + [edge_t, seq], bases + [edge_b, np.roll(seq, 3 * E)]
    for tr in pe.IDS:
        for t, b in zip(tensors, bases):
            z = pe.forward(t, b, E, tr)
            assert len(z) == len(t) and (pe.inverse(z, b, E, tr) == t).all(), (tr, len(t))
            assert (z[len(t) // E * E:] == (t ^ b if tr == XOR else psc.forward(t, b, 1) if tr == SUB else t)[len(t) // E * E:]).all(), "the trailing n mod E bytes"
    transforms = pe.cycle_all_pairs(len(tensors), 5)
    out, written, P, res = pe.split_each_model(tensors, bases, E, transforms)
    assert written.all() and res == [len(t) for t in tensors]
    for i, t in enumerate(tensors):
        planes = [out[P[i * E + p]:P[i * E + p + 1]] for p in range(E)]
        assert (pe.merge_each_one(planes, bases[i], E, transforms[i]) == t).all(), i


@pytest.mark.parametrize("E", pc.ELEMS)
def test_the_model_dispatches_to_the_dedicated_models(E):
    tensors, bases = _pairs(E, 50 + E)
    n = len(tensors)
    want = {PLAIN: pc.split_model(tensors, E), PRED: ppc.split_pred_model(tensors, E), XOR: pc.split_model([t ^ b for t, b in zip(tensors, bases)], E),
            SUB: psc.split_sub_model(tensors, bases, E)}
    for tr in pe.IDS:
        got = pe.split_each_model(tensors, bases, E, [tr] * n)
        assert (got[0] == want[tr][0]).all() and got[2] == want[tr][2] and got[3] == want[tr][3], tr
    # a mixed array: tensor i's planes are those of the uniform run of its transform
    transforms = pe.cycle_all_pairs(n)
    out, _, P, _ = pe.split_each_model(tensors, bases, E, transforms)
    S = [int(x) for x in pc.offsets(tensors)]
    for i, tr in enumerate(transforms):
        assert (out[S[i]:S[i + 1]] == want[tr][0][S[i]:S[i + 1]]).all(), i
    # refusals: an unknown byte, the estimate's 0xFF, XOR and SUB without a base; nothing of those tensors is written, the others are
    out, written, P2, res = pe.split_each_model(tensors, None, E, [PLAIN, 4, 0xFF, XOR, SUB, PRED, PLAIN, PRED])
    assert P2 == P and res == [len(tensors[0])] + [pc.GENERIC] * 4 + [len(t) for t in tensors[5:]]
    assert not written[S[1]:S[5]].any() and written[S[5]:].all()


def test_the_cycle_holds_every_ordered_pair():
    for lead in range(16):
        assert pe.neighbour_pairs(pe.cycle_all_pairs(17, lead)) == set(pe.PAIRS), lead
    assert pe.neighbour_pairs(pe.cycle_all_pairs(60), 0, 60) == set(pe.PAIRS)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_exports_and_python_names():
    """fails on the parent commit: none of these exists there"""
    lib = C.CDLL(os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so"))
    for name in SIX + ("FSEHIP_tensor_each_workspaceHead",):
        getattr(lib, name)
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    for name in SIX + ("FSEHIP_tensor_each_workspaceHead", "FSEHIP_TRANSFORMS_GIVEN", "FSEHIP_TRANSFORMS_CHOOSE"):
        assert name in header, name
    import finitestateentropy_amd
    from finitestateentropy_amd import api
    assert "compress_tensors_each" in finitestateentropy_amd.__all__ and finitestateentropy_amd.compress_tensors_each is api.compress_tensors_each
    for name in ("planes_split_each_dbatch", "planes_merge_each_dbatch", "tensor_compress_each_dbatch", "tensor_decompress_each_dbatch",
                 "tensor_compress_seg_each_dbatch", "tensor_decompress_seg_each_dbatch", "tensor_each_workspace_head", "compress_tensors_each"):
        assert callable(getattr(api.FseHip, name)), name
    assert list(inspect.signature(api.compress_tensors_each).parameters) == ["tensors", "transforms", "base", "codec", "block_size_id", "segment_log", "margin_permille"]
    par = inspect.signature(api.compress_tensors_each).parameters
    assert [par[k].default for k in par if k != "tensors"] == ["auto", None, 0, 5, None, 50]
    assert api.CompressedTensors.transforms is None, "the class-level default"
    assert list(inspect.signature(api.decompress_tensors).parameters) == ["obj", "base"], "unchanged"
    assert list(inspect.signature(api.compress_tensors_auto).parameters) == ["tensors", "base", "codec", "block_size_id", "segment_log", "margin_permille"], "unchanged"


def _r256(x):
    return (x + 255) & ~255


def test_the_workspace_head_is_host_arithmetic(lib):
    head, est = lib.FSEHIP_tensor_each_workspaceHead, lib.FSEHIP_planes_estimate_workspaceBound
    head.restype = est.restype = SZ
    for E in pc.ELEMS:
        for n in (0, 1, 2, 3, 31, 32, 33, 100, 4096, (1 << 24) - 1):
            assert head(SZ(n), UI(E), CI(GIVEN), UI(0)) == 0 and head(SZ(n), UI(E), CI(GIVEN), UI(0xFFFF)) == 0, "given: nothing in front of the writer's workspace"
            for mask in range(1, 16):
                want = est(SZ(n), UI(E), UI(mask)) + _r256(n * 4 * E * 8) + _r256(n * 4 * 8) + _r256(n * 8)
                got = head(SZ(n), UI(E), CI(CHOOSE), UI(mask))
                assert got == want and got % 256 == 0, (E, n, mask)
    for n, E, policy, mask in ((1, 2, CHOOSE, 0), (1, 2, CHOOSE, 16), (1, 3, CHOOSE, 1), (1, 3, GIVEN, 1), (1, 2, 2, 1), (1, 2, -1, 1), (1 << 24, 2, CHOOSE, 1),
                               (1, 0, GIVEN, 0)):
        assert head(SZ(n), UI(E), CI(policy), UI(mask)) > (1 << 62), (n, E, policy, mask)


def test_every_argument_refusal_without_a_device(lib):
    for f in ("FSEHIP_tensor_each_workspaceHead", "FSEHIP_frame_compress_packed_dbatch_workspaceSize", "FSEHIP_frame_mixedWorkspaceBound",
              "FSEHIP_frame_decompress_packed_dbatch_workspaceSize"):
        getattr(lib, f).restype = SZ
    n, E, blocks, nseg = 1, 2, 8, 2
    head = lib.FSEHIP_tensor_each_workspaceHead(SZ(n), UI(E), CI(CHOOSE), UI(15))
    need = head + max(lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize(SZ(4), SZ(blocks), UI(0), CI(0)),
                      lib.FSEHIP_frame_mixedWorkspaceBound(SZ(4), SZ(blocks), UI(0), CI(1)),
                      lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize(SZ(4), SZ(blocks)))
    assert need < (1 << 30)
    GUARD = 0xF9
    a = (C.c_uint8 * 256)(*([GUARD] * 256))                     # stands for every output: offsets, results, transforms, planes, frames
    room = (C.c_uint8 * (need + 512))(*([GUARD] * (need + 512)))
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    wb = SZ(need)

    def split(q=None, E=E, n=n, cap=8):                       # q: planes, plane offsets, results, src, base, transforms, offsets
        q = list(q or [p] * 7)
        return lib.FSEHIP_planes_split_each_dbatch(q[0], q[1], q[2], q[3], q[4], q[5], q[6], SZ(n), UI(E), U64(cap), null)

    def merge(q=None, E=E, n=n, cap=8):                       # q: dst, dst offsets, results, planes, plane offsets, plane sizes, base, transforms
        q = list(q or [p] * 8)
        return lib.FSEHIP_planes_merge_each_dbatch(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], SZ(n), UI(E), U64(cap), null)

    for k in range(7):
        if k != 4:                                             # (the base may be NULL: that call would launch, it is not made here)
            q = [p] * 7
            q[k] = null
            assert split(q) == HIP_INVALID_VALUE, k
    for k in range(8):
        if k != 6:
            q = [p] * 8
            q[k] = null
            assert merge(q) == HIP_INVALID_VALUE, k
    for bad in (0, 3, 5, 16, 0xFFFFFFFF):
        assert split(E=bad) == HIP_INVALID_VALUE and merge(E=bad) == HIP_INVALID_VALUE, bad
    assert split(cap=1 << 46) == HIP_INVALID_VALUE and merge(cap=1 << 46) == HIP_INVALID_VALUE and split(n=1 << 30) == HIP_INVALID_VALUE
    assert split(cap=32768 << 24) == HIP_INVALID_VALUE and merge(n=1 << 30) == HIP_INVALID_VALUE

    def comp(seg, q=None, base=p, est=p, policy=CHOOSE, mask=15, margin=50, E=E, n=n, cap=8, segLog=10, blocks=blocks, bsid=0, codec=0, codecs=null, cpolicy=0, tol=0,
             align=0, w=ws, wb=wb):
        # q: dst, frame offsets, frame results, tensor results, src, transforms, src offsets, planes, plane offsets [, seg first, seg offsets]
        q = list(q or [p] * 11)
        front = (q[0], U64(256), q[1], q[2], q[3], q[4], base, q[5], CI(policy), UI(mask), UI(margin), est, q[6], SZ(n), UI(E), U64(cap))
        writer = (SZ(blocks), UI(bsid), CI(codec), codecs, CI(cpolicy), UI(tol), UI(align), q[7], q[8])
        if seg:
            return lib.FSEHIP_tensor_compress_seg_each_dbatch(*front, q[9], SZ(nseg), UI(segLog), *writer, q[10], w, wb, null)
        return lib.FSEHIP_tensor_compress_each_dbatch(*front, *writer, w, wb, null)

    for seg in (False, True):
        for k in range(1, 11 if seg else 9):                   # (q[0], the frames: the writer's own check, made behind the launches of the split)
            q = [p] * 11
            q[k] = null
            assert comp(seg, q) == HIP_INVALID_VALUE, (seg, k)
        for bad in (0, 3, 5, 16):
            assert comp(seg, E=bad) == HIP_INVALID_VALUE, bad
        for policy in (2, -1, 7):
            assert comp(seg, policy=policy) == HIP_INVALID_VALUE, "an unknown transform policy"
        for mask in (0, 16, 31, 0x100, 0xFFFFFFFF):
            assert comp(seg, mask=mask) == HIP_INVALID_VALUE, mask
        for mask in (4, 8, 12, 5, 15):
            assert comp(seg, mask=mask, base=null) == HIP_INVALID_VALUE, "XOR or SUB in the mask without a base"
        assert comp(seg, margin=1001) == HIP_INVALID_VALUE and comp(seg, margin=0xFFFFFFFF) == HIP_INVALID_VALUE
        assert comp(seg, w=VP(ws.value + 16)) == HIP_INVALID_VALUE and comp(seg, w=null) == HIP_INVALID_VALUE, "a misaligned workspace, none"
        assert comp(seg, wb=SZ(head - 1)) == HIP_INVALID_VALUE and comp(seg, wb=SZ(head)) == HIP_INVALID_VALUE, "room for the estimate alone: the writer has none"
        assert comp(seg, policy=GIVEN, wb=SZ(0)) == HIP_INVALID_VALUE, "given: the writer's workspace is still needed"
        assert comp(seg, cap=1 << 46) == HIP_INVALID_VALUE and comp(seg, n=1 << 24) == HIP_INVALID_VALUE and comp(seg, n=1 << 30, policy=GIVEN) == HIP_INVALID_VALUE
        assert comp(seg, codec=2) == HIP_INVALID_VALUE and comp(seg, bsid=7) == HIP_INVALID_VALUE and comp(seg, align=13) == HIP_INVALID_VALUE, "the writer's refusals"
        assert comp(seg, codecs=p, cpolicy=2) == HIP_INVALID_VALUE and comp(seg, codecs=p, cpolicy=1, tol=1001) == HIP_INVALID_VALUE, "the mixed writer's"
    assert comp(True, segLog=9) == HIP_INVALID_VALUE and comp(True, segLog=31) == HIP_INVALID_VALUE and comp(True, segLog=10, bsid=1) == HIP_INVALID_VALUE

    def dec(seg, q=None, E=E, n=n, cap=8, segLog=10, blocks=blocks, w=ws, wb=wb):
        # q: dst, dst offsets, transforms, results, frames, frame offsets, planes, plane offsets, plane results [, seg first, seg offsets, seg results]
        q = list(q or [p] * 12)
        front = (q[0], q[1], U64(cap), p, q[2], q[3], q[4], q[5], SZ(n), UI(E))
        if seg:
            return lib.FSEHIP_tensor_decompress_seg_each_dbatch(*front, q[9], SZ(nseg), UI(segLog), SZ(blocks), q[6], U64(64), q[10], q[11], q[7], q[8], w, wb, null)
        return lib.FSEHIP_tensor_decompress_each_dbatch(*front, SZ(blocks), q[6], U64(64), q[7], q[8], w, wb, null)

    for seg in (False, True):
        for k in range(12 if seg else 9):
            q = [p] * 12
            q[k] = null
            assert dec(seg, q) == HIP_INVALID_VALUE, (seg, k)
        for bad in (0, 3, 5, 16):
            assert dec(seg, E=bad) == HIP_INVALID_VALUE, bad
        assert dec(seg, cap=1 << 46) == HIP_INVALID_VALUE and dec(seg, n=1 << 30) == HIP_INVALID_VALUE and dec(seg, blocks=1 << 31) == HIP_INVALID_VALUE
        assert dec(seg, w=VP(ws.value + 16)) == HIP_INVALID_VALUE and dec(seg, wb=SZ(0)) == HIP_INVALID_VALUE
    assert dec(True, segLog=9) == HIP_INVALID_VALUE and dec(True, segLog=31) == HIP_INVALID_VALUE
    assert all(x == GUARD for x in a) and all(x == GUARD for x in bytes(room)), "nothing is written"


def test_python_refusals_in_front_of_any_launch():
    from finitestateentropy_amd import api
    hip = api.FseHip.__new__(api.FseHip)                          # (no launch below: nothing here has a device)
    hip.lib = C.CDLL(os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so"))
    assert hip.tensor_each_workspace_head(3, 2, False) == 0 and hip.tensor_each_workspace_head(3, 2, True, 3) == 3 * 2 * 2 * 1024 + 3 * 256
    with pytest.raises(ValueError):
        hip.tensor_each_workspace_head(3, 2, True, 0)
    obj = hip.compress_tensors_each([])
    assert isinstance(obj, api.CompressedTensors) and obj.transforms == [] and obj.groups == [] and obj.nbytes == 0 and not obj.delta
    assert hip.decompress_tensors(obj) == []
    assert hip.compress_tensors_each([], segment_log=18).segment_log == 18
    # the out-of-scope list, and the arguments
    for codec in (api.SparsePlanes(0), api.PredictedPlanes(0), obj, 2, True, None):
        with pytest.raises(ValueError):
            hip.compress_tensors_each([], codec=codec)
    with pytest.raises(ValueError):
        hip.compress_tensors_each([], base=api.DeltaBase([], "sub", check=True))
    assert hip.compress_tensors_each([], base=api.DeltaBase([], "sub")).transforms == []
    for bad in ("plain", "best", ["plain"], ["delta"], [0], 7):
        with pytest.raises((ValueError, TypeError)):
            hip.compress_tensors_each([], transforms=bad)
    for bad in (-1, 1001, 2.5, True, None):
        with pytest.raises(ValueError):
            hip.compress_tensors_each([], margin_permille=bad)
    for bad in (9, 31, 2.0):
        with pytest.raises(ValueError):
            hip.compress_tensors_each([], segment_log=bad)
    with pytest.raises(ValueError):
        hip.compress_tensors_each([], base=[1])
    with pytest.raises(TypeError):
        hip.compress_tensors_each([np.zeros(4)])
    with pytest.raises(ValueError):
        hip.compress_tensors_each([np.zeros(4)], transforms=["xor"])         # a delta without a base: refused before the tensors are looked at
    # reading: a base where a name is "xor" or "sub", names that are names, no windows and no patches
    held = api.CompressedTensors([], [None], [()], None, 0, 5)
    held.transforms = ["sub"]
    with pytest.raises(ValueError):
        hip.decompress_tensors(held)
    held.transforms = ["plain", "pred"]
    with pytest.raises(ValueError):
        hip.decompress_tensors(held)
    held.transforms = ["delta"]
    with pytest.raises(ValueError):
        hip.decompress_tensors(held)
    seg = hip.compress_tensors_each([], segment_log=18)
    with pytest.raises(ValueError, match="transform per tensor"):
        hip.decompress_tensor_windows(seg, [])
    with pytest.raises(ValueError, match="transform per tensor"):
        hip.patch_tensor_windows(seg, [], [])
    auto = api.CompressedTensors([], [], [], None, api.AutoCodec(), 5)
    auto.transforms = []
    with pytest.raises(ValueError, match="transform per tensor"):
        hip.compress_tensors([], codec=auto)

"""Predicted planes without a device (include/fsehip.h, "predicted planes"): the numpy model of planes_pred_corpus.py is the issue's transform
on Python integers and a bijection -- every size from 0 to 40 bytes and around one and three runs, the edge values as neighbours in both
directions -- a constant tensor leaves one non-zero element per run, the trailing bytes pass unchanged, a tensor's planes do not depend on
where it lies; the library exports the six *_pred_dbatch calls and refuses bad arguments before any device call with nothing written; the
Python surface (PredictedPlanes, CompressedTensors.predictor, the archive's meta JSON) is as specified and the pinned signatures are
unchanged; and the reason for the feature: the oracle's FSE frames of the predicted planes of sorted uint32 indices take at most 0.5, and
of a noisy fp32 sine field at most 0.75, of the frames of the plain planes."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_pred_corpus as ppc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI, CI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint, C.c_int
EXPORTS = ("FSEHIP_planes_split_pred_dbatch", "FSEHIP_planes_merge_pred_dbatch", "FSEHIP_tensor_compress_pred_dbatch", "FSEHIP_tensor_decompress_pred_dbatch",
           "FSEHIP_tensor_compress_seg_pred_dbatch", "FSEHIP_tensor_decompress_seg_pred_dbatch")
R = ppc.RUN


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


def _ints(raw, E):
    return [int.from_bytes(bytes(raw[k:k + E]), "little") for k in range(0, len(raw) - len(raw) % E, E)]


def _ref_forward(t, E):
    """the issue's definition on Python integers"""
    W = 8 * E
    out = []
    for j, x in enumerate(t):
        d = (x - (0 if j % R == 0 else t[j - 1])) % (1 << W)
        out.append(((d << 1) % (1 << W)) ^ ((1 << W) - 1 if d >> (W - 1) else 0))
    return out


def _ref_inverse(z, E):
    W = 8 * E
    out = []
    for j, x in enumerate(z):
        d = (x >> 1) ^ ((1 << W) - 1 if x & 1 else 0)
        out.append((d + (0 if j % R == 0 else out[j - 1])) % (1 << W))
    return out


def model_sizes(E):
    return list(range(41)) + [E * 1023 + 3, E * 1024, E * 1025 + 1, E * 3077 + E - 1]


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("E", pc.ELEMS)
def test_model_is_the_definition_and_a_bijection_at_every_size(E):
    assert ppc.RUN_LOG == 10 and R == 1024
    for n, raw in zip(model_sizes(E), pc.random_tensors(model_sizes(E), 50 + E)):
        z = ppc.forward(raw, E)
        assert len(z) == n and _ints(z, E) == _ref_forward(_ints(raw, E), E)
        assert (z[n // E * E:] == raw[n // E * E:]).all(), "the trailing n mod E bytes pass unchanged"
        assert (ppc.inverse(z, E) == raw).all() and _ints(ppc.inverse(z, E), E) == _ref_inverse(_ints(z, E), E)
        # the inverse is a bijection as well: any bytes are the differences of some tensor
        assert (ppc.forward(ppc.inverse(raw, E), E) == raw).all()
    # E == 1: all 256 differences occur behind every predecessor
    if E == 1:
        t = np.stack([np.repeat(np.arange(256, dtype=np.uint8), 256), np.tile(np.arange(256, dtype=np.uint8), 256)], axis=1).reshape(-1)
        z = ppc.forward(t, 1)
        inside = np.arange(1, len(t), 2)                     # (odd positions: none starts a run)
        for y in range(256):
            at = inside[t[inside - 1] == y]
            assert len(at) == 256 and len(set(z[at].tolist())) == 256


@pytest.mark.parametrize("E", pc.ELEMS)
def test_edge_values_as_neighbours_in_both_directions(E):
    vals, W = ppc.edge_values(E), 8 * E
    assert {0, 1, (1 << (W - 1)) - 1, 1 << (W - 1), (1 << W) - 1, (1 << (W - 8)) - 1, 1 << (W - 8)} <= set(vals)
    assert E != 8 or {(1 << 32) - 1, 1 << 32} <= set(vals)
    for lead in (0, 1, 14, 15, 16, 1022, 1023, 1024):           # the pairs across lane and run boundaries
        raw = ppc.edge_sequence(E, lead)
        t = _ints(raw, E)
        assert len(t) == lead + 3 * len(vals) ** 2
        pairs = set(zip(t[lead:], t[lead + 1:]))
        assert all((x, y) in pairs and (y, x) in pairs for x in vals for y in vals), "every value beside every other, both ways round"
        z = ppc.forward(raw, E)
        assert _ints(z, E) == _ref_forward(t, E) and (ppc.inverse(z, E) == raw).all()
    # the most negative difference is its own negative: 2^W - 1, and back; +1 and -1 beside each other give 2 and 1
    top = np.frombuffer((1 << (W - 1)).to_bytes(E, "little"), np.uint8)
    assert bytes(ppc.forward(top, E)) == b"\xff" * E
    seq = np.array([5, 6, 5], np.uint64).astype(ppc._U[E]).view(np.uint8)
    assert _ints(ppc.forward(seq, E), E) == [10, 2, 1]


@pytest.mark.parametrize("E", pc.ELEMS)
def test_constant_tensors_runs_restart_and_position_independence(E):
    value = np.arange(3, 3 + E, dtype=np.uint8)
    n_el = 3 * R + 77
    z = ppc.forward(np.tile(value, n_el), E).reshape(-1, E)
    assert np.flatnonzero(z.any(axis=1)).tolist() == [0, R, 2 * R, 3 * R], "one non-zero element per run"
    assert (z[0] == z[R]).all()
    # a run restarts: what lies in front of a run does not reach into it, and changing one element changes two differences at most
    raw = pc.random_tensors([E * (2 * R + 9)], 9 + E)[0]
    other = raw.copy()
    other[:E * R] ^= 0x5A
    assert (ppc.forward(other, E)[E * R:] == ppc.forward(raw, E)[E * R:]).all()
    other = raw.copy()
    other[E * 700] ^= 1
    changed = np.flatnonzero((ppc.forward(other, E) != ppc.forward(raw, E)).reshape(-1, E).any(axis=1)).tolist()
    assert changed == [700, 701]
    # the planes of a tensor do not depend on where it lies in the batch
    sizes = [E * 1030 + (E - 1), 5, E * 40]
    a = pc.random_tensors(sizes, 77)
    out, written, P, res = ppc.split_pred_model(a, E)
    out2, _, P2, _ = ppc.split_pred_model([np.zeros(13, np.uint8)] + a, E)
    assert written.all() and res == sizes and (out2[13:] == out).all() and [x - 13 for x in P2[E:]] == P
    for i, raw in enumerate(a):
        planes = [out[P[i * E + p]:P[i * E + p + 1]] for p in range(E)]
        assert [len(x) for x in planes] == [pc.plane_size(len(raw), p, E) for p in range(E)]
        assert all((planes[p] == ppc.forward(raw, E)[p::E]).all() for p in range(E)) and (ppc.merge_pred_one(planes, E) == raw).all()


# ---------------------------------------------------------------------------------------------------------------- 2
def _calls(lib, a, room):
    """name -> f(**changes): each of the six calls on one tensor with arguments nothing but the named change refuses"""
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    big = SZ(1 << 40)

    def split(ptrs=None, E=2, n=1, cap=8):                  # ptrs: planes, plane offsets, results, src, source offsets
        q = list(ptrs or [p] * 5)
        return lib.FSEHIP_planes_split_pred_dbatch(*q, SZ(n), UI(E), U64(cap), null)

    def merge(ptrs=None, E=2, n=1, cap=8):                  # ptrs: dst, dst offsets, results, planes, plane offsets, plane sizes
        q = list(ptrs or [p] * 6)
        return lib.FSEHIP_planes_merge_pred_dbatch(*q, SZ(n), UI(E), U64(cap), null)

    def compress(ptrs=None, E=2, n=1, cap=8, blocks=4, bsid=0, codec=0, codecs=null, policy=0, tol=0, align=0, w=ws, wb=big):
        q = list(ptrs or [p] * 8)                           # ptrs: dst, frame offsets, frame results, tensor results, src, source offsets, planes, plane offsets
        return lib.FSEHIP_tensor_compress_pred_dbatch(q[0], U64(64), q[1], q[2], q[3], q[4], q[5], SZ(n), UI(E), U64(cap), SZ(blocks), UI(bsid), CI(codec), codecs,
                                                      CI(policy), UI(tol), UI(align), q[6], q[7], w, wb, null)

    def decompress(ptrs=None, E=2, n=1, cap=8, blocks=4, w=ws, wb=big):
        q = list(ptrs or [p] * 8)                           # ptrs: dst, dst offsets, results, frames, frame offsets, planes, plane offsets, plane results
        return lib.FSEHIP_tensor_decompress_pred_dbatch(q[0], q[1], U64(cap), q[2], q[3], q[4], SZ(n), UI(E), SZ(blocks), q[5], U64(8), q[6], q[7], w, wb, null)

    def seg(ptrs=None, E=2, n=1, cap=8, nseg=None, seg_log=10, blocks=4, bsid=0, codec=0, codecs=null, policy=0, tol=0, align=0, w=ws, wb=big):
        q = list(ptrs or [p] * 10)                          # ptrs: .. of compress .., seg first (6), planes (7), plane offsets (8), seg offsets (9)
        return lib.FSEHIP_tensor_compress_seg_pred_dbatch(q[0], U64(64), q[1], q[2], q[3], q[4], q[5], SZ(n), UI(E), U64(cap), q[6], SZ(E if nseg is None else nseg),
                                                          UI(seg_log), SZ(blocks), UI(bsid), CI(codec), codecs, CI(policy), UI(tol), UI(align), q[7], q[8], q[9], w, wb, null)

    def unseg(ptrs=None, E=2, n=1, cap=8, nseg=None, seg_log=10, blocks=4, w=ws, wb=big):
        q = list(ptrs or [p] * 11)                          # ptrs: dst, dst offsets, results, frames, frame offsets, seg first, planes, seg offsets, seg results, plane offsets, plane sizes
        return lib.FSEHIP_tensor_decompress_seg_pred_dbatch(q[0], q[1], U64(cap), q[2], q[3], q[4], SZ(n), UI(E), q[5], SZ(E if nseg is None else nseg), UI(seg_log),
                                                            SZ(blocks), q[6], U64(8), q[7], q[8], q[9], q[10], w, wb, null)
    return dict(split=split, merge=merge, compress=compress, decompress=decompress, seg=seg, unseg=unseg)


NPTRS = dict(split=5, merge=6, compress=8, decompress=8, seg=10, unseg=11)


def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    assert "#define FSEHIP_PRED_RUN_LOG 10" in header and all(name + "(" in header for name in EXPORTS)
    a = (C.c_uint64 * 8)()
    room = (C.c_uint8 * 512)()
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    big = SZ(1 << 40)
    f = _calls(lib, a, room)
    assert len(f) == len(EXPORTS)
    for name, call in f.items():
        for E in (0, 3, 5, 6, 7, 16, 0xFFFFFFFF):
            assert call(E=E) == HIP_INVALID_VALUE, (name, E)
        for E in (1, 2, 4, 8):
            for k in range(NPTRS[name]):                    # every array, the planes buffer for E == 1 too; the destination of the frames may
                if name in ("compress", "seg") and k == 0:  # be null where nothing is to be written -- as for the calls these are named after
                    continue
                args = [p] * NPTRS[name]
                args[k] = null
                assert call(args, E) == HIP_INVALID_VALUE, (name, E, k)
            # 2^31 planes, a launch of 2^24 workgroups
            assert call(None, E, n=(1 << 31) // E) == HIP_INVALID_VALUE, (name, E)
        assert call(None, 2, cap=1 << 46) == HIP_INVALID_VALUE and call(None, 2, cap=32768 << 24) == HIP_INVALID_VALUE, name
    # the composites: a workspace that is null, too small or off its alignment; a promise of 2^31 blocks
    for name in ("compress", "decompress", "seg", "unseg"):
        assert f[name](w=null, wb=SZ(0)) == HIP_INVALID_VALUE and f[name](w=ws, wb=SZ(0)) == HIP_INVALID_VALUE, name
        assert f[name](w=VP(ws.value + 8)) == HIP_INVALID_VALUE and f[name](blocks=1 << 31) == HIP_INVALID_VALUE, name
    # the writers: a bad codec, block-size id, alignment, policy and tolerance
    for name in ("compress", "seg"):
        for kw in (dict(bsid=7), dict(codec=2), dict(codec=-1), dict(align=13), dict(codecs=p, policy=2), dict(codecs=p, policy=1, tol=1001)):
            assert f[name](**kw) == HIP_INVALID_VALUE, (name, kw)
    # the segmented pair: a segment below a block or above 2^30, 2^31 segments
    for name, extra in (("seg", dict(bsid=1)), ("unseg", {})):
        assert f[name](seg_log=9) == HIP_INVALID_VALUE and f[name](seg_log=31) == HIP_INVALID_VALUE and f[name](nseg=1 << 31) == HIP_INVALID_VALUE, name
    assert f["seg"](seg_log=10, bsid=1) == HIP_INVALID_VALUE, "a segment is a whole number of blocks"
    assert all(x == 0 for x in a) and not any(room), "nothing is written"


def test_the_old_calls_refuse_what_they_refused(lib):
    """deltaOp == 2 is no way in: the *_op_dbatch calls still take FSEHIP_DELTA_XOR and FSEHIP_DELTA_SUB alone"""
    a = (C.c_uint64 * 8)()
    p, null = C.cast(a, VP), VP(0)
    for op in (2, 3, 0xFFFFFFFF):
        for E in (1, 2, 4, 8):
            assert lib.FSEHIP_planes_split_op_dbatch(p, p, p, p, p, UI(op), p, SZ(1), UI(E), U64(8), null) == HIP_INVALID_VALUE
            assert lib.FSEHIP_planes_merge_op_dbatch(p, p, p, p, p, p, p, UI(op), SZ(1), UI(E), U64(8), null) == HIP_INVALID_VALUE
    assert all(x == 0 for x in a)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_python_surface():
    import finitestateentropy_amd
    from finitestateentropy_amd import api
    P = api.PredictedPlanes
    assert finitestateentropy_amd.PredictedPlanes is P and "PredictedPlanes" in finitestateentropy_amd.__all__
    assert P().codec == 0 and P(1).codec == 1 and P(api.AutoCodec(20)).codec == api.AutoCodec(20)
    assert P(1) == P(1) and P(1) != P(0) and P(0) != 0 and hash(P(1)) == hash(P(1)) and repr(P(api.AutoCodec(5))) == "PredictedPlanes(AutoCodec(5))"
    for bad in (2, -1, True, None, "fse", 0.5, api.SparsePlanes(0), P(0), api.SparsePlanes(api.AutoCodec(0))):
        with pytest.raises(ValueError):
            P(bad)
    with pytest.raises(ValueError):
        api.SparsePlanes(P(0))
    # the object: a class-level default, set on the instance
    assert api.CompressedTensors.predictor is None
    assert "predictor" not in vars(api.CompressedTensors([], [], [], None, 0, 5))
    # the pinned signatures
    assert list(inspect.signature(api.compress_tensors).parameters) == ["tensors", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.compress_tensors_segmented).parameters) == ["tensors", "segment_log", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.decompress_tensors).parameters) == ["obj", "base"]
    assert list(inspect.signature(api.CompressedTensors.__init__).parameters) == ["self", "groups", "dtypes", "shapes", "device", "codec", "block_size_id", "delta"]
    assert list(inspect.signature(api.decompress_tensor_windows).parameters) == ["obj", "windows", "base"]
    assert list(inspect.signature(api.patch_tensor_windows).parameters) == ["obj", "tensors", "windows", "base"]
    # the six low-level methods mirror the C calls: no base, no delta_op
    for name in EXPORTS:
        par = inspect.signature(getattr(api.FseHip, name[len("FSEHIP_"):])).parameters
        assert "base" not in par and "delta_op" not in par and "elem_bytes" in par, name
    for name in ("tensor_compress_pred_dbatch", "tensor_compress_seg_pred_dbatch"):
        par = inspect.signature(getattr(api.FseHip, name)).parameters
        assert par["codec"].default == 0 and par["codecs"].default is None and par["block_size_id"].default == 5


def test_python_refusals_and_the_empty_object_need_no_device(monkeypatch):
    from finitestateentropy_amd import api
    hip = api.FseHip.__new__(api.FseHip)                     # no library: whatever reaches it fails the test

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)
    hip.lib = NoLib()
    P = api.PredictedPlanes
    for codec in (P(0), P(1), P(api.AutoCodec(10))):
        for seg_log in (None, 16):
            obj = hip.compress_tensors_segmented([], seg_log, codec) if seg_log else hip.compress_tensors([], codec)
            assert obj.predictor == "prev" and vars(obj)["predictor"] == "prev" and obj.codec == codec and obj.delta is False and obj.groups == []
            assert obj.segment_log == seg_log and obj.sparse_permille is None
            assert hip.decompress_tensors(obj) == []
            with pytest.raises(ValueError):
                hip.decompress_tensor_windows(obj, [])
            with pytest.raises(ValueError):
                hip.patch_tensor_windows(obj, [], [])
    assert hip.compress_tensors([], 0).predictor is None
    # a base does not go with prediction, as a sequence or as a DeltaBase, with tensors or without
    for base in ([], [object()], api.DeltaBase([]), api.DeltaBase([object()], "xor")):
        with pytest.raises(ValueError):
            hip.compress_tensors([], P(0), base=base)
        with pytest.raises(ValueError):
            hip.compress_tensors_segmented([object()], 16, P(1), base=base)
    seg = hip.compress_tensors_segmented([], 16, P(0))
    with pytest.raises(ValueError):
        hip.decompress_tensors(seg, base=[])                 # no deltas: a base does not belong to the object
    seg.predictor = "next"
    with pytest.raises(ValueError):
        hip.decompress_tensors(seg)
    # the archive's meta JSON
    to_json, from_json = None, None
    for cell in api.FseHip.archive_tensors.__closure__ or ():
        v = cell.cell_contents
        if callable(v) and getattr(v, "__name__", "") == "_codec_to_json":
            to_json = v
    for cell in api.FseHip.open_archive.__closure__ or ():
        v = cell.cell_contents
        if callable(v) and getattr(v, "__name__", "") == "_codec_from_json":
            from_json = v
    assert to_json is not None and from_json is not None
    for codec, j in ((P(0), {"pred": 0}), (P(1), {"pred": 1}), (P(api.AutoCodec(7)), {"pred": {"auto": 7}})):
        assert to_json(codec) == j and from_json(j) == codec
    assert to_json(api.SparsePlanes(1, 300)) == {"sparse": 1, "permille": 300} and from_json(3) == 3


# ---------------------------------------------------------------------------------------------------------------- 4
def _frame_bytes(checker, raw, E):
    return [checker.frame_compress(np.ascontiguousarray(pl), 5, 0)[0] for pl in pc.planes_of(raw, E)]


def test_predicted_frames_of_sorted_indices_and_of_a_sine_field_against_the_plain_ones(checker):
    idx = np.sort(np.random.default_rng(1).choice(2 ** 22, 2 ** 18, replace=False)).astype(np.uint32)
    field = (np.sin(np.linspace(0, 40, 2 ** 18)) + 1e-4 * np.random.default_rng(2).standard_normal(2 ** 18)).astype(np.float32)
    for what, data, cap in (("sorted uint32 indices", idx, 0.5), ("fp32 sine field", field, 0.75)):
        raw = data.view(np.uint8)
        assert raw.size == 4 << 18
        z = ppc.forward(raw, 4)
        assert (ppc.inverse(z, 4) == raw).all()
        plain, pred = _frame_bytes(checker, raw, 4), _frame_bytes(checker, z, 4)
        print("%s, %d bytes, FSE, block-size id 5: plain planes %s = %d, predicted planes %s = %d (%.3f)" % (what, raw.size, plain, sum(plain), pred, sum(pred),
                                                                                                              sum(pred) / sum(plain)))
        assert 0 < sum(pred) <= cap * sum(plain)

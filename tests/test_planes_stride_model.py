"""Strided predicted planes without a device (include/fsehip.h, "strided predicted planes"): the numpy model of planes_stride_corpus.py is
the transform's definition on Python integers and a bijection for every stride 1 .. 8 and element size -- every size from 0 to 40 bytes
and around one and three runs -- stride 1 is the model of planes_pred_corpus.py, the chains restart with every run (a de-interleaved
identity, a constant per channel), the edge values as stride-neighbours in both directions across lane and run boundaries; the library
exports the six *_pred_stride_dbatch calls and refuses bad arguments, strides 0 and 9 among them, before any device call with nothing
written; the Python surface (PredictedPlanes(codec, stride), the predictor strings, the archive's meta JSON, the refusals) is as
specified; and the reason for the feature: on the oracle's FSE frames of five interleaved corpora the planes of the right stride are
smaller than the plain planes and than the stride-1 planes."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_pred_corpus as ppc
import planes_stride_corpus as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI, CI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint, C.c_int
EXPORTS = ("FSEHIP_planes_split_pred_stride_dbatch", "FSEHIP_planes_merge_pred_stride_dbatch", "FSEHIP_tensor_compress_pred_stride_dbatch",
           "FSEHIP_tensor_decompress_pred_stride_dbatch", "FSEHIP_tensor_compress_seg_pred_stride_dbatch", "FSEHIP_tensor_decompress_seg_pred_stride_dbatch")
R = sc.RUN


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


def _ints(raw, E):
    return [int.from_bytes(bytes(raw[k:k + E]), "little") for k in range(0, len(raw) - len(raw) % E, E)]


def _ref_forward(t, E, S):
    """the definition on Python integers"""
    W = 8 * E
    out = []
    for j, x in enumerate(t):
        d = (x - (0 if j % R < S else t[j - S])) % (1 << W)
        out.append(((d << 1) % (1 << W)) ^ ((1 << W) - 1 if d >> (W - 1) else 0))
    return out


def _ref_inverse(z, E, S):
    """t[j] = the sum of d[k] over k = j, j - S, .. while k >= R floor(j / R)"""
    W = 8 * E
    d = [(x >> 1) ^ ((1 << W) - 1 if x & 1 else 0) for x in z]
    return [sum(d[k] for k in range(j, j // R * R - 1, -S)) % (1 << W) for j in range(len(z))]


def model_sizes(E, S):
    """0 .. 40 bytes, and 1023, 1024, 1025, 1024 + S and 3072 + 5 elements, some with trailing bytes"""
    return list(range(41)) + [E * 1023 + 3 % E, E * 1024, E * 1025 + 1 % E, E * (1024 + S), E * 3077 + E - 1]


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("S", sc.STRIDES)
@pytest.mark.parametrize("E", pc.ELEMS)
def test_model_is_the_definition_and_a_bijection_at_every_size(E, S):
    rng = np.random.default_rng(100 * E + S)
    for n in model_sizes(E, S):
        for raw in (rng.integers(0, 256, n, dtype=np.uint8), (np.cumsum(rng.integers(0, 3, n)) & 0xFF).astype(np.uint8)):
            z = sc.forward(raw, E, S)
            assert z.dtype == np.uint8 and len(z) == n
            assert _ints(z, E) == _ref_forward(_ints(raw, E), E, S), (n, "forward")
            assert (z[n - n % E:] == raw[n - n % E:]).all(), "the trailing bytes pass unchanged"
            back = sc.inverse(z, E, S)
            assert (back == raw).all() and _ints(back, E) == _ref_inverse(_ints(z, E), E, S), (n, "inverse")
            assert (sc.forward(sc.inverse(raw, E, S), E, S) == raw).all(), "a bijection: every bit pattern is somebody's differences"
            if n // E < S:
                assert _ints(z, E) == _ref_forward(_ints(raw, E), E, 10 ** 6), "fewer than S elements: zigzag(t)"


@pytest.mark.parametrize("E", pc.ELEMS)
def test_stride_one_is_the_model_of_the_predicted_planes(E):
    rng = np.random.default_rng(7 + E)
    for n in model_sizes(E, 1):
        raw = rng.integers(0, 256, n, dtype=np.uint8)
        assert (sc.forward(raw, E, 1) == ppc.forward(raw, E)).all() and (sc.inverse(raw, E, 1) == ppc.inverse(raw, E)).all()


@pytest.mark.parametrize("S", sc.STRIDES)
@pytest.mark.parametrize("E", pc.ELEMS)
def test_chains_restart_with_every_run(E, S):
    """channel c of a tensor of lcm(S, 1024) elements (times two) against the definition on that channel alone: the channel's elements of
    run r are its own run there, whose first element is predicted by 0 -- which holds only where the phase of the chains is
    (j mod 1024) mod S and not j mod S; and a constant per channel leaves S elements per run"""
    m = 2 * (S * R // math.gcd(S, R))
    rng = np.random.default_rng(50 * E + S)
    z = rng.integers(0, 256, m * E, dtype=np.uint8)
    t = np.array(_ints(sc.inverse(z, E, S), E), dtype=object)
    d = [(x >> 1) ^ ((1 << 8 * E) - 1 if x & 1 else 0) for x in _ints(z, E)]
    j = np.arange(m)
    for c in range(S):
        for r in range(m // R):
            sel = np.nonzero((j // R == r) & ((j % R) % S == c))[0]
            want = np.cumsum(np.array([d[k] for k in sel], dtype=object)) % (1 << 8 * E)
            assert (t[sel] == want).all(), (c, r)
    raw = sc.channels(E, S, 4 * R + 7)
    zc = _ints(sc.forward(raw, E, S), E)
    t0 = _ints(raw, E)
    assert all((zc[k] == 0) == (k % R >= S) for k in range(len(zc))), "zero except the first S elements of every run"
    assert all(zc[k] == 2 * t0[k] for k in range(len(zc)) if k % R < S)
    assert (sc.inverse(sc.forward(raw, E, S), E, S) == raw).all()


@pytest.mark.parametrize("S", sc.STRIDES[1:])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_edge_values_as_stride_neighbours_in_both_directions(E, S):
    vals = sc.edge_values(E)
    W = 8 * E
    assert {0, 1, (1 << (W - 1)) - 1, 1 << (W - 1), (1 << W) - 1, (1 << (W - 8)) - 1 if E > 1 else 0, 1 << (W - 8) if E > 1 else 1} <= set(vals)
    assert E != 8 or {(1 << 32) - 1, 1 << 32} <= set(vals)
    for period in (16, R):
        raw = sc.across(E, S, period)
        t = _ints(raw, E)
        pairs = [(x, y) for x in vals for y in vals]
        assert all((y, x) in pairs for x, y in pairs), "both directions"
        for k, (x, y) in enumerate(pairs):
            b = period * (k + 1)
            assert t[b - S:b] == [x] * S and t[b:b + S] == [y] * S
        z = sc.forward(raw, E, S)
        assert _ints(z, E) == _ref_forward(t, E, S)
        back = sc.inverse(z, E, S)
        assert (back == raw).all() and _ints(back, E) == _ref_inverse(_ints(z, E), E, S)


# ---------------------------------------------------------------------------------------------------------------- the C calls
def _calls(lib, a, room):
    """name -> f(**changes): each of the six calls on one tensor with arguments nothing but the named change refuses"""
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    big = SZ(1 << 40)

    def split(ptrs=None, E=2, n=1, cap=8, stride=2):        # ptrs: planes, plane offsets, results, src, source offsets
        q = list(ptrs or [p] * 5)
        return lib.FSEHIP_planes_split_pred_stride_dbatch(*q, SZ(n), UI(E), U64(cap), UI(stride), null)

    def merge(ptrs=None, E=2, n=1, cap=8, stride=2):        # ptrs: dst, dst offsets, results, planes, plane offsets, plane sizes
        q = list(ptrs or [p] * 6)
        return lib.FSEHIP_planes_merge_pred_stride_dbatch(*q, SZ(n), UI(E), U64(cap), UI(stride), null)

    def compress(ptrs=None, E=2, n=1, cap=8, blocks=4, bsid=0, codec=0, codecs=null, policy=0, tol=0, align=0, w=ws, wb=big, stride=2):
        q = list(ptrs or [p] * 8)                           # ptrs: dst, frame offsets, frame results, tensor results, src, source offsets, planes, plane offsets
        return lib.FSEHIP_tensor_compress_pred_stride_dbatch(q[0], U64(64), q[1], q[2], q[3], q[4], q[5], SZ(n), UI(E), U64(cap), SZ(blocks), UI(bsid), CI(codec),
                                                             codecs, CI(policy), UI(tol), UI(align), q[6], q[7], w, wb, UI(stride), null)

    def decompress(ptrs=None, E=2, n=1, cap=8, blocks=4, w=ws, wb=big, stride=2):
        q = list(ptrs or [p] * 8)                           # ptrs: dst, dst offsets, results, frames, frame offsets, planes, plane offsets, plane results
        return lib.FSEHIP_tensor_decompress_pred_stride_dbatch(q[0], q[1], U64(cap), q[2], q[3], q[4], SZ(n), UI(E), SZ(blocks), q[5], U64(8), q[6], q[7], w, wb,
                                                               UI(stride), null)

    def seg(ptrs=None, E=2, n=1, cap=8, nseg=None, seg_log=10, blocks=4, bsid=0, codec=0, codecs=null, policy=0, tol=0, align=0, w=ws, wb=big, stride=2):
        q = list(ptrs or [p] * 10)                          # ptrs: .. of compress .., seg first (6), planes (7), plane offsets (8), seg offsets (9)
        return lib.FSEHIP_tensor_compress_seg_pred_stride_dbatch(q[0], U64(64), q[1], q[2], q[3], q[4], q[5], SZ(n), UI(E), U64(cap), q[6],
                                                                 SZ(E if nseg is None else nseg), UI(seg_log), SZ(blocks), UI(bsid), CI(codec), codecs, CI(policy),
                                                                 UI(tol), UI(align), q[7], q[8], q[9], w, wb, UI(stride), null)

    def unseg(ptrs=None, E=2, n=1, cap=8, nseg=None, seg_log=10, blocks=4, w=ws, wb=big, stride=2):
        q = list(ptrs or [p] * 11)                          # ptrs: dst, dst offsets, results, frames, frame offsets, seg first, planes, seg offsets, seg results, plane offsets, plane sizes
        return lib.FSEHIP_tensor_decompress_seg_pred_stride_dbatch(q[0], q[1], U64(cap), q[2], q[3], q[4], SZ(n), UI(E), q[5], SZ(E if nseg is None else nseg),
                                                                   UI(seg_log), SZ(blocks), q[6], U64(8), q[7], q[8], q[9], q[10], w, wb, UI(stride), null)
    return dict(split=split, merge=merge, compress=compress, decompress=decompress, seg=seg, unseg=unseg)


NPTRS = dict(split=5, merge=6, compress=8, decompress=8, seg=10, unseg=11)


def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    assert "#define FSEHIP_PRED_MAX_STRIDE 8" in header and all(name + "(" in header for name in EXPORTS)
    assert not any("pred_stride" in line and "workspaceSize" in line for line in header.splitlines()), "no workspace call of their own"
    a = (C.c_uint64 * 8)()
    room = (C.c_uint8 * 512)()
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    f = _calls(lib, a, room)
    assert len(f) == len(EXPORTS)
    for name, call in f.items():
        for stride in (0, 9, 16, 0xFFFFFFFF):               # with everything else in order -- and for every good stride, the other refusals
            assert call(stride=stride) == HIP_INVALID_VALUE, (name, stride)
        for stride in sc.STRIDES:
            for E in (0, 3, 5, 6, 7, 16, 0xFFFFFFFF):
                assert call(E=E, stride=stride) == HIP_INVALID_VALUE, (name, E, stride)
        for E in (1, 2, 4, 8):
            for stride in (1, 3, 8):
                for k in range(NPTRS[name]):                # every array, the planes buffer for E == 1 too; the destination of the frames may
                    if name in ("compress", "seg") and k == 0:   # be null where nothing is to be written -- as for the calls these are named after
                        continue
                    args = [p] * NPTRS[name]
                    args[k] = null
                    assert call(args, E, stride=stride) == HIP_INVALID_VALUE, (name, E, k)
                # 2^31 planes, a launch of 2^24 workgroups
                assert call(None, E, n=(1 << 31) // E, stride=stride) == HIP_INVALID_VALUE, (name, E)
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
    for name in ("seg", "unseg"):
        assert f[name](seg_log=9) == HIP_INVALID_VALUE and f[name](seg_log=31) == HIP_INVALID_VALUE and f[name](nseg=1 << 31) == HIP_INVALID_VALUE, name
    assert f["seg"](seg_log=10, bsid=1) == HIP_INVALID_VALUE, "a segment is a whole number of blocks"
    assert all(x == 0 for x in a) and not any(room), "nothing is written"


# ---------------------------------------------------------------------------------------------------------------- Python
def test_python_surface():
    from finitestateentropy_amd import api
    P = api.PredictedPlanes
    assert P().stride == 1 and P(1).stride == 1 and P(1, 3).stride == 3 and P(0, stride=8).stride == 8 and P(api.AutoCodec(20), 2).codec == api.AutoCodec(20)
    assert list(inspect.signature(P.__init__).parameters) == ["self", "codec", "stride"]
    for bad in (0, 9, -1, True, False, None, "3", 2.0, 1.5):
        with pytest.raises(ValueError):
            P(0, bad)
    assert P(1, 3) == P(1, 3) and P(1, 3) != P(1, 2) and P(1, 3) != P(1) and P(1, 1) == P(1) and P(0, 3) != P(1, 3)
    assert hash(P(1, 3)) == hash(P(1, 3)) and hash(P(1, 1)) == hash(P(1)) and len({P(1, s) for s in sc.STRIDES}) == 8
    assert repr(P(1)) == repr(P(1, 1)) == "PredictedPlanes(1)" and repr(P(0, 3)) == "PredictedPlanes(0, stride=3)"
    assert repr(P(api.AutoCodec(5), 2)) == "PredictedPlanes(AutoCodec(5), stride=2)"
    assert [P(0, s).predictor for s in sc.STRIDES] == ["prev", "prev2", "prev3", "prev4", "prev5", "prev6", "prev7", "prev8"]
    # the six low-level methods mirror the C calls: `stride` is required, no base, no delta_op
    for name in EXPORTS:
        par = inspect.signature(getattr(api.FseHip, name[len("FSEHIP_"):])).parameters
        assert "base" not in par and "delta_op" not in par and "elem_bytes" in par, name
        assert par["stride"].default is inspect.Parameter.empty, name
    for name in ("tensor_compress_pred_stride_dbatch", "tensor_compress_seg_pred_stride_dbatch"):
        par = inspect.signature(getattr(api.FseHip, name)).parameters
        assert par["codec"].default == 0 and par["codecs"].default is None and par["block_size_id"].default == 5


def test_python_refusals_and_the_empty_object_need_no_device():
    from finitestateentropy_amd import api
    hip = api.FseHip.__new__(api.FseHip)                     # no library: whatever reaches it fails the test

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)
    hip.lib = NoLib()
    P = api.PredictedPlanes
    for S in sc.STRIDES[1:]:
        name = "prev%d" % S
        for codec in (P(0, S), P(api.AutoCodec(10), S)):
            for seg_log in (None, 16):
                obj = hip.compress_tensors_segmented([], seg_log, codec) if seg_log else hip.compress_tensors([], codec)
                assert obj.predictor == name and vars(obj)["predictor"] == name and obj.codec == codec and obj.delta is False and obj.groups == []
                assert obj.segment_log == seg_log and obj.sparse_permille is None
                assert hip.decompress_tensors(obj) == []
                for call in (hip.decompress_tensor_windows, hip.decompress_tensor_windows_each):
                    with pytest.raises(ValueError):
                        call(obj, [])
                for call in (hip.patch_tensor_windows, hip.patch_tensor_windows_each):
                    with pytest.raises(ValueError):
                        call(obj, [], [])
        # a base does not go with prediction, as a sequence or as a DeltaBase, with tensors or without
        for base in ([], [object()], api.DeltaBase([]), api.DeltaBase([object()], "xor")):
            with pytest.raises(ValueError):
                hip.compress_tensors([], P(0, S), base=base)
            with pytest.raises(ValueError):
                hip.compress_tensors_segmented([object()], 16, P(1, S), base=base)
    assert hip.compress_tensors([], P(1, 1)).predictor == "prev"
    seg = hip.compress_tensors_segmented([], 16, P(0, 3))
    with pytest.raises(ValueError):
        hip.decompress_tensors(seg, base=[])                 # no deltas: a base does not belong to the object
    for unknown in ("prev0", "prev1", "prev9", "next", "prev10", "prev3 ", "PREV3", 3):
        seg.predictor = unknown
        with pytest.raises(ValueError):
            hip.decompress_tensors(seg)
    # a bad stride at the low-level methods: before the library is reached
    lead = dict(planes_split=2, planes_merge=4, tensor_compress=2, tensor_decompress=3)      # the arguments in front of elem_bytes and stride
    for name in EXPORTS:
        method = name[len("FSEHIP_"):]
        for bad in (0, 9, True, None, 2.0):
            with pytest.raises(ValueError):
                getattr(hip, method)(*[None] * next(v for k, v in lead.items() if method.startswith(k)), 2, bad, *([16] if "_seg_" in method else []))
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
    for codec, j in ((P(0), {"pred": 0}), (P(1, 1), {"pred": 1}), (P(0, 3), {"pred": 0, "stride": 3}), (P(1, 8), {"pred": 1, "stride": 8}),
                     (P(api.AutoCodec(7), 2), {"pred": {"auto": 7}, "stride": 2})):
        assert to_json(codec) == j and from_json(j) == codec
    with pytest.raises(ValueError):
        from_json({"pred": 0, "stride": 9})


# ---------------------------------------------------------------------------------------------------------------- the reason
def _frame_bytes(checker, raw, E):
    return sum(checker.frame_compress(np.ascontiguousarray(pl), 5, 0)[0] for pl in pc.planes_of(raw, E))


@pytest.mark.parametrize("name,E,S,gen", sc.CORPORA, ids=[c[0].replace(" ", "-") for c in sc.CORPORA])
def test_strided_frames_are_below_the_plain_and_the_stride_one_frames(checker, name, E, S, gen):
    """the oracle's FSE frames, block-size id 5, of the model's planes of 2^18 elements: conditions on the reference's output alone"""
    raw = gen()
    assert raw.dtype == np.uint8 and raw.size == E << 18
    z = sc.forward(raw, E, S)
    assert (sc.inverse(z, E, S) == raw).all()
    plain, one, strided = _frame_bytes(checker, raw, E), _frame_bytes(checker, sc.forward(raw, E, 1), E), _frame_bytes(checker, z, E)
    print("%s, %d bytes, FSE, block-size id 5: plain planes %d (%.3f), predicted planes %d (%.3f), stride %d %d (%.3f)"
          % (name, raw.size, plain, plain / raw.size, one, one / raw.size, S, strided, strided / raw.size))
    assert 0 < strided < plain and strided < one

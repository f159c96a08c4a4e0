"""Arithmetic tensor deltas without a device (include/fsehip.h, "arithmetic tensor deltas"): the numpy model of planes_sub_corpus.py is a
bijection -- exhaustively for bytes, over the edge values and random pairs for the wider elements -- an unchanged tensor is all zeros, the
trailing bytes go bytewise, swapping tensor and base gives other planes; the library exports the ten *_op_dbatch calls and refuses a bad
deltaOp, and what the XOR calls refuse, before any device call; the Python surface (DeltaBase, delta_op) is as specified and the pinned
signatures are unchanged; and the reason for the feature: the oracle's frames of the planes of zigzag(new - old) of a bf16 weight update take
less than 0.90 (FSE) and 0.95 (Huff0) of the frames of the planes of new XOR old."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_delta_corpus as pdc
import planes_sub_corpus as psc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI, CI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint, C.c_int
EXPORTS = ("FSEHIP_planes_split_op_dbatch", "FSEHIP_planes_merge_op_dbatch", "FSEHIP_planes_split_window_op_dbatch", "FSEHIP_tensor_compress_delta_op_dbatch",
           "FSEHIP_tensor_decompress_delta_op_dbatch", "FSEHIP_tensor_compress_mixed_op_dbatch", "FSEHIP_tensor_compress_seg_op_dbatch",
           "FSEHIP_tensor_decompress_seg_op_dbatch", "FSEHIP_tensor_decompress_window_op_dbatch", "FSEHIP_tensor_patch_window_op_dbatch")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


def _ref_zz(t, b, E):
    """the issue's definition on Python integers"""
    W = 8 * E
    d = (t - b) % (1 << W)
    return ((d << 1) % (1 << W)) ^ ((1 << W) - 1 if d >> (W - 1) else 0)


def _ints(raw, E):
    return [int.from_bytes(bytes(raw[k:k + E]), "little") for k in range(0, len(raw) - len(raw) % E, E)]


# ---------------------------------------------------------------------------------------------------------------- 1
def test_bytes_exhaustively():
    t, b = np.repeat(np.arange(256, dtype=np.uint8), 256), np.tile(np.arange(256, dtype=np.uint8), 256)
    z = psc.forward(t, b, 1)
    assert z.tolist() == [_ref_zz(int(x), int(y), 1) for x, y in zip(t, b)]
    assert (psc.inverse(z, b, 1) == t).all()
    for y in range(256):                                     # for every base: all 256 tensors give all 256 deltas
        assert len(set(z[b == y].tolist())) == 256
    assert not z[t == b].any() and z[t != b].all()


@pytest.mark.parametrize("E", (2, 4, 8))
def test_wide_elements_over_the_edge_set_and_random_pairs(E):
    t, b = psc.edge_pairs(E)
    vals = psc.edge_values(E)
    assert len(t) == 2 * len(vals) ** 2 * E and {0, 1, (1 << (8 * E)) - 1, 1 << (8 * E - 1), (1 << (8 * E - 8)) - 1, 1 << (8 * E - 8)} <= set(vals)
    assert E != 8 or {(1 << 32) - 1, 1 << 32} <= set(vals)
    assert _ints(t, E)[:4] == [0, 0, 0, 1] and _ints(b, E)[:4] == [0, 0, 1, 0], "0 - 1 beside 1 - 0"
    rng = np.random.default_rng(40 + E)
    rt, rb = rng.integers(0, 256, 4096 * E, dtype=np.uint8), rng.integers(0, 256, 4096 * E, dtype=np.uint8)
    wide = np.dtype("<u%d" % E)
    near = (rt.view(wide) + rng.integers(0, 5, 4096).astype(wide) - wide.type(2)).view(np.uint8)      # the element moves by -2 .. 2, carries and all
    for x, y in ((t, b), (rt, rb), (near, rt)):
        z = psc.forward(x, y, E)
        assert _ints(z, E) == [_ref_zz(p, q, E) for p, q in zip(_ints(x, E), _ints(y, E))]
        assert (psc.inverse(z, y, E) == x).all()
    # the most negative difference is its own negative: it maps to 2^W - 1, and back
    top = (1 << (8 * E - 1)).to_bytes(E, "little")
    z = psc.forward(np.frombuffer(top, np.uint8), np.zeros(E, np.uint8), E)
    assert bytes(z) == b"\xff" * E and bytes(psc.inverse(z, np.zeros(E, np.uint8), E)) == top


@pytest.mark.parametrize("E", pc.ELEMS)
def test_model_round_trips_unchanged_is_zero_trailing_bytes_and_asymmetry(E):
    sizes = pc.split_sizes(E, 256) + list(range(41))
    tensors, bases = pc.random_tensors(sizes, 3), pc.random_tensors(sizes, 4)
    out, written, P, res = psc.split_sub_model(tensors, bases, E)
    S = [int(x) for x in pc.offsets(tensors)]
    assert written.all() and res == sizes and len(P) == len(tensors) * E + 1 and P[-1] == S[-1]
    differ = 0
    for i, (raw, b) in enumerate(zip(tensors, bases)):
        planes = [out[P[i * E + p]:P[i * E + p + 1]] for p in range(E)]
        assert [len(x) for x in planes] == [pc.plane_size(len(raw), p, E) for p in range(E)]
        z = psc.forward(raw, b, E)
        assert all((planes[p] == z[p::E]).all() for p in range(E))
        assert (psc.merge_sub_one(planes, b, E) == raw).all()
        # the trailing n mod E bytes: the E == 1 form, each byte by itself
        tail = len(raw) % E
        if tail:
            assert z[-tail:].tolist() == [_ref_zz(int(x), int(y), 1) for x, y in zip(raw[-tail:], b[-tail:])]
        assert _ints(z, E) == [_ref_zz(p, q, E) for p, q in zip(_ints(raw, E), _ints(b, E))]
        # not symmetric: the planes of base - tensor are others (they would decode the tensor to something else)
        if len(raw) >= 8:
            swapped = psc.forward(b, raw, E)
            differ += int((swapped != z).any())
            assert (psc.inverse(swapped, b, E) != raw).any()
    assert differ == sum(1 for s in sizes if s >= 8)
    zeros, _, _, _ = psc.split_sub_model(tensors, tensors, E)
    assert not zeros.any(), "an unchanged tensor is all zeros, whatever it holds"
    # a capacity inside tensor 6: it and everything behind it collapse onto its start
    k = 6
    cap = S[k] + 1
    assert S[k + 1] > cap
    _, written, P, res = psc.split_sub_model(tensors, bases, E, cap)
    assert res[:k] == sizes[:k] and set(res[k:]) == {pc.GENERIC}
    assert P[k * E:] == [S[k]] * (len(P) - k * E) and not written[S[k]:].any() and written[:S[k]].all()


# ---------------------------------------------------------------------------------------------------------------- 2
def _calls(lib, a, room):
    """name -> f(op, **changes): each of the ten calls on one tensor with arguments nothing but the named change refuses -- every pointer the
    array `a`, workspaces and scratch on their alignment and "large enough" """
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    big = SZ(1 << 40)

    def split(op, ptrs=None, E=2, n=1, cap=8):              # ptrs: planes, plane offsets, results, src, base, source offsets
        q = list(ptrs or [p] * 6)
        return lib.FSEHIP_planes_split_op_dbatch(*q[:5], UI(op), q[5], SZ(n), UI(E), U64(cap), null)

    def merge(op, ptrs=None, E=2, n=1, cap=8):              # ptrs: dst, dst offsets, results, planes, plane offsets, plane sizes, base
        q = list(ptrs or [p] * 7)
        return lib.FSEHIP_planes_merge_op_dbatch(*q, UI(op), SZ(n), UI(E), U64(cap), null)

    def split_window(op, E=2, base=p):
        return lib.FSEHIP_planes_split_window_op_dbatch(p, p, p, p, base, UI(op), p, p, p, SZ(1), UI(E), UI(10), U64(8), U64(8), null)

    def compress(op, E=2, bsid=0, codec=0, align=0, src=p, base=p, planes=p, w=ws, wb=big):
        return lib.FSEHIP_tensor_compress_delta_op_dbatch(p, U64(64), p, p, p, src, base, UI(op), p, SZ(1), UI(E), U64(8), SZ(4), UI(bsid), CI(codec), UI(align),
                                                          planes, p, w, wb, null)

    def decompress(op, E=2, base=p, w=ws, wb=big):
        return lib.FSEHIP_tensor_decompress_delta_op_dbatch(p, p, U64(8), base, UI(op), p, p, p, SZ(1), UI(E), SZ(4), p, U64(8), p, p, w, wb, null)

    def mixed(op, E=2, base=p):
        return lib.FSEHIP_tensor_compress_mixed_op_dbatch(p, U64(64), p, p, p, p, base, UI(op), p, SZ(1), UI(E), U64(8), SZ(4), UI(0), p, CI(0), UI(0), UI(0), p, p,
                                                          ws, big, null)

    def seg(op, E=2, base=p):
        return lib.FSEHIP_tensor_compress_seg_op_dbatch(p, U64(64), p, p, p, p, base, UI(op), p, SZ(1), UI(E), U64(8), p, SZ(E), UI(10), SZ(4), UI(0), CI(0), null,
                                                        CI(0), UI(0), UI(0), p, p, p, ws, big, null)

    def unseg(op, E=2, base=p):
        return lib.FSEHIP_tensor_decompress_seg_op_dbatch(p, p, U64(8), base, UI(op), p, p, p, SZ(1), UI(E), p, SZ(E), UI(10), SZ(4), p, U64(8), p, p, p, p, ws, big, null)

    def window(op, E=2, base=p):
        return lib.FSEHIP_tensor_decompress_window_op_dbatch(p, p, U64(8), base, UI(op), p, p, p, p, p, SZ(1), UI(E), p, SZ(E), UI(10), p, SZ(E), SZ(4), p, U64(8), p, p, p,
                                                             p, p, ws, big, null)

    def patch(op, E=2, base=p):
        return lib.FSEHIP_tensor_patch_window_op_dbatch(p, U64(64), p, p, null, p, p, U64(64), p, p, null, p, base, UI(op), p, U64(8), p, SZ(1), UI(E), p, SZ(E), UI(10), p,
                                                        SZ(E), p, U64(8), SZ(4), UI(0), CI(0), null, CI(0), UI(0), UI(0), p, p, p, p, p, U64(64), p, p, ws, big, ws, big, null)
    return dict(split=split, merge=merge, split_window=split_window, compress=compress, decompress=decompress, mixed=mixed, seg=seg, unseg=unseg, window=window,
                patch=patch)


def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    a = (C.c_uint64 * 8)()
    room = (C.c_uint8 * 512)()
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    big = SZ(1 << 40)
    f = _calls(lib, a, room)
    assert len(f) == len(EXPORTS)
    # a deltaOp that is none: refused by every call, for every element size, with a base and (where it is nullable) without one
    for op in (2, 3, 0x7FFFFFFF, 0xFFFFFFFF):
        for name, call in f.items():
            for E in (1, 2, 4, 8):
                assert call(op, E=E) == HIP_INVALID_VALUE, (name, op, E)
        for name in ("split_window", "mixed", "seg", "unseg", "window", "patch"):
            assert f[name](op, base=null) == HIP_INVALID_VALUE, (name, op, "null base")
    # what test_planes_delta_model.py checks for the XOR calls, for both ops
    for op in (psc.XOR, psc.SUB):
        for E in (0, 3, 5, 6, 7, 16, 0xFFFFFFFF):
            for name, call in f.items():
                assert call(op, E=E) == HIP_INVALID_VALUE, (name, op, E)
        for E in (1, 2, 4, 8):
            for k in range(6):                               # every array of the split: planes and source for E == 1 too, and the base
                args = [p] * 6
                args[k] = null
                assert f["split"](op, args, E) == HIP_INVALID_VALUE, (op, E, k)
            for k in range(7):                               # every array of the merge, the base among them
                args = [p] * 7
                args[k] = null
                assert f["merge"](op, args, E) == HIP_INVALID_VALUE, (op, E, k)
            # the composites: a null base, a null planes buffer (E == 1 too), a null source
            assert f["compress"](op, E, base=null) == HIP_INVALID_VALUE, (op, E)
            assert f["compress"](op, E, planes=null) == HIP_INVALID_VALUE, (op, E)
            assert f["compress"](op, E, src=null) == HIP_INVALID_VALUE, (op, E)
            assert f["decompress"](op, E, base=null) == HIP_INVALID_VALUE, (op, E)
        # 2^31 planes, a launch of 2^24 workgroups
        for E in (1, 2, 8):
            assert f["split"](op, None, E, n=(1 << 31) // E) == HIP_INVALID_VALUE
            assert f["merge"](op, None, E, n=(1 << 31) // E) == HIP_INVALID_VALUE
        assert f["split"](op, None, 2, cap=1 << 46) == HIP_INVALID_VALUE
        assert f["merge"](op, None, 2, cap=32768 << 24) == HIP_INVALID_VALUE
        # the composites: a workspace that is too small, a bad codec / block-size id / alignment -- all before the first launch
        for bsid, codec, align in ((0, 0, 0), (7, 0, 0), (0, 2, 0), (0, 0, 13)):
            assert f["compress"](op, 2, bsid, codec, align, w=null, wb=SZ(0)) == HIP_INVALID_VALUE, (op, bsid, codec, align)
        for bsid, codec, align in ((7, 0, 0), (0, 2, 0), (0, 0, 13)):
            assert f["compress"](op, 2, bsid, codec, align) == HIP_INVALID_VALUE, (op, bsid, codec, align)
        assert f["decompress"](op, 2, w=null, wb=SZ(0)) == HIP_INVALID_VALUE
        assert f["compress"](op, 2, w=VP(ws.value + 8), wb=big) == HIP_INVALID_VALUE and f["decompress"](op, 2, w=VP(ws.value + 8), wb=big) == HIP_INVALID_VALUE
    assert all(x == 0 for x in a) and not any(room), "nothing is written"


# ---------------------------------------------------------------------------------------------------------------- 3
def test_python_surface():
    import finitestateentropy_amd
    from finitestateentropy_amd import api
    assert finitestateentropy_amd.DeltaBase is api.DeltaBase and "DeltaBase" in finitestateentropy_amd.__all__
    d = api.DeltaBase([1, 2, 3])
    assert d.op == "sub" and d.tensors == [1, 2, 3] and list(d) == [1, 2, 3] and len(d) == 3
    assert api.DeltaBase((), "xor").op == "xor" and api.DeltaBase(iter([4])).tensors == [4]
    for bad in ("add", "SUB", 1, None, b"sub"):
        with pytest.raises(ValueError):
            api.DeltaBase([], bad)
    assert api.DELTA_OPS == {"xor": 0, "sub": 1}
    # the object: a class-level default, set on the instance as segment_log is
    assert api.CompressedTensors.delta_op == "xor" and api.CompressedTensors.segment_log is None
    obj = api.CompressedTensors([], [], [], None, 0, 5, delta=True)
    assert obj.delta_op == "xor" and "delta_op" not in vars(obj) and obj.delta is True
    # the pinned signatures
    assert list(inspect.signature(api.compress_tensors).parameters) == ["tensors", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.decompress_tensors).parameters) == ["obj", "base"]
    assert list(inspect.signature(api.CompressedTensors.__init__).parameters) == ["self", "groups", "dtypes", "shapes", "device", "codec", "block_size_id", "delta"]
    assert list(inspect.signature(api.compress_tensors_segmented).parameters) == ["tensors", "segment_log", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.decompress_tensor_windows).parameters) == ["obj", "windows", "base"]
    assert list(inspect.signature(api.patch_tensor_windows).parameters) == ["obj", "tensors", "windows", "base"]
    # the low-level methods that take a base: a trailing keyword delta_op = 0
    for name in ("planes_split_xor_dbatch", "planes_merge_xor_dbatch", "planes_split_window_dbatch", "tensor_compress_delta_dbatch", "tensor_decompress_delta_dbatch",
                 "tensor_compress_mixed_dbatch", "tensor_compress_seg_dbatch", "tensor_decompress_seg_dbatch", "tensor_decompress_window_dbatch",
                 "tensor_patch_window_dbatch"):
        par = inspect.signature(getattr(api.FseHip, name)).parameters
        assert "base" in par and list(par)[-1] == "delta_op" and par["delta_op"].default == 0, name
    for name in ("planes_split_dbatch", "planes_merge_dbatch", "tensor_compress_dbatch", "tensor_decompress_dbatch"):
        assert "delta_op" not in inspect.signature(getattr(api.FseHip, name)).parameters, name


# ---------------------------------------------------------------------------------------------------------------- 4
def test_planes_of_a_bf16_update_minus_its_base_take_less_than_those_of_the_xor(checker):
    old, new = pdc.bf16_update_pair()
    assert old.size == new.size == 2 << 18 and (old != new).any()
    sub = psc.forward(new, old, 2)
    assert (psc.inverse(sub, old, 2) == new).all()

    def frames(raw, codec):
        return [checker.frame_compress(np.ascontiguousarray(pl), 5, codec)[0] for pl in pc.planes_of(raw, 2)]
    for codec, bound in ((0, 0.90), (1, 0.95)):
        x, s = frames(old ^ new, codec), frames(sub, codec)
        print("bf16 N(0, 0.02) + N(0, 2e-5), %d bytes, codec %d: planes of new XOR old %s = %d, planes of zigzag(new - old) %s = %d (%.3f)"
              % (new.size, codec, x, sum(x), s, sum(s), sum(s) / sum(x)))
        assert 0 < sum(s) < bound * sum(x)
    unchanged = frames(psc.forward(new, new, 2), 0)
    print("unchanged tensor: planes %s" % unchanged)
    assert sum(unchanged) < 200

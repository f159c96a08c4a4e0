"""Tensor deltas without a device (include/fsehip.h, "tensor deltas"): the numpy model of planes_delta_corpus.py round-trips; the library exports
the four XOR calls and refuses bad arguments -- the plain calls' and a null base -- before any device call; the Python pair takes `base`; and
the reason for the feature: the oracle's frames of the planes of `new XOR old` of a bf16 weight update take less than half of the frames of
the planes of `new`."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_delta_corpus as pdc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64 = C.c_size_t, C.c_void_p, C.c_uint64
EXPORTS = ("FSEHIP_planes_split_xor_dbatch", "FSEHIP_planes_merge_xor_dbatch", "FSEHIP_tensor_compress_delta_dbatch", "FSEHIP_tensor_decompress_delta_dbatch")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("E", pc.ELEMS)
def test_model_round_trips(E):
    sizes = pc.split_sizes(E, 256) + list(range(41))
    tensors, bases = pc.random_tensors(sizes, 3), pc.random_tensors(sizes, 4)
    out, written, P, res = pdc.split_xor_model(tensors, bases, E)
    S = [int(x) for x in pc.offsets(tensors)]
    assert written.all() and res == sizes and len(P) == len(tensors) * E + 1 and P[-1] == S[-1]
    for i, (raw, b) in enumerate(zip(tensors, bases)):
        assert P[i * E] == S[i]
        planes = [out[P[i * E + p]:P[i * E + p + 1]] for p in range(E)]
        assert [len(x) for x in planes] == [pc.plane_size(len(raw), p, E) for p in range(E)]
        assert all((planes[p] == (raw ^ b)[p::E]).all() for p in range(E))
        assert (pdc.merge_xor_one(planes, b, E) == raw).all()
        assert (pdc.merge_xor_one(planes, raw, E) == b).all()                       # XOR: either side is the other's base
        assert pc.merge_verdict([len(x) for x in planes], S[i + 1], S[i], E, S[-1]) == len(raw)
    # an unchanged tensor is all zeros, whatever it holds
    zeros, _, _, _ = pdc.split_xor_model(tensors, tensors, E)
    assert not zeros.any()
    # a capacity inside tensor 6: it and everything behind it collapse onto its start
    k = 6
    cap = S[k] + 1
    assert S[k + 1] > cap
    _, written, P, res = pdc.split_xor_model(tensors, bases, E, cap)
    assert res[:k] == sizes[:k] and set(res[k:]) == {pc.GENERIC}
    assert P[k * E:] == [S[k]] * (len(P) - k * E) and not written[S[k]:].any() and written[:S[k]].all()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    a = (C.c_uint64 * 8)()
    p = C.cast(a, VP)
    null = VP(0)
    room = (C.c_uint8 * 512)()
    ws = VP((C.addressof(room) + 255) & ~255)                # a workspace on its 256-byte alignment, "large enough": only what is named refuses the call
    big = 1 << 40
    s, m = lib.FSEHIP_planes_split_xor_dbatch, lib.FSEHIP_planes_merge_xor_dbatch
    tc, td = lib.FSEHIP_tensor_compress_delta_dbatch, lib.FSEHIP_tensor_decompress_delta_dbatch

    def split(ptrs, E):                     # ptrs: planes, plane offsets, results, src, base, source offsets
        return s(*ptrs, SZ(1), C.c_uint(E), U64(8), null)

    def merge(ptrs, E):                     # ptrs: dst, dst offsets, results, planes, plane offsets, plane sizes, base
        return m(*ptrs, SZ(1), C.c_uint(E), U64(8), null)

    def compress(E, bsid=0, codec=0, align=0, src=p, base=p, planes=p, ws=null, ws_bytes=0):
        return tc(p, U64(64), p, p, p, src, base, p, SZ(1), C.c_uint(E), U64(8), SZ(4), C.c_uint(bsid), C.c_int(codec), C.c_uint(align), planes, p, ws, SZ(ws_bytes), null)

    def decompress(E, base=p, ws=null, ws_bytes=0):
        return td(p, p, U64(8), base, p, p, p, SZ(1), C.c_uint(E), SZ(4), p, U64(8), p, p, ws, SZ(ws_bytes), null)

    # what test_planes_model.py checks for the plain calls
    for E in (0, 3, 5, 6, 7, 16, 0xFFFFFFFF):
        assert split([p] * 6, E) == HIP_INVALID_VALUE, E
        assert merge([p] * 7, E) == HIP_INVALID_VALUE, E
        assert compress(E) == HIP_INVALID_VALUE, E
        assert decompress(E) == HIP_INVALID_VALUE, E
    for E in (1, 2, 4, 8):
        for k in range(6):                                   # every array of the split: planes and source for E == 1 too, and the base
            args = [p] * 6
            args[k] = null
            assert split(args, E) == HIP_INVALID_VALUE, (E, k)
        for k in range(7):                                   # every array of the merge, the base among them
            args = [p] * 7
            args[k] = null
            assert merge(args, E) == HIP_INVALID_VALUE, (E, k)
        # the composites: a null base, a null planes buffer (E == 1 too), a null source
        assert compress(E, base=null, ws=ws, ws_bytes=big) == HIP_INVALID_VALUE, E
        assert compress(E, planes=null, ws=ws, ws_bytes=big) == HIP_INVALID_VALUE, E
        assert compress(E, src=null, ws=ws, ws_bytes=big) == HIP_INVALID_VALUE, E
        assert decompress(E, base=null, ws=ws, ws_bytes=big) == HIP_INVALID_VALUE, E
    # 2^31 planes, a launch of 2^24 workgroups
    for E in (1, 2, 8):
        assert s(p, p, p, p, p, p, SZ((1 << 31) // E), C.c_uint(E), U64(8), null) == HIP_INVALID_VALUE
        assert m(p, p, p, p, p, p, p, SZ((1 << 31) // E), C.c_uint(E), U64(8), null) == HIP_INVALID_VALUE
    assert s(p, p, p, p, p, p, SZ(1), C.c_uint(2), U64(1 << 46), null) == HIP_INVALID_VALUE
    assert m(p, p, p, p, p, p, p, SZ(1), C.c_uint(2), U64(32768 << 24), null) == HIP_INVALID_VALUE
    # the composites: a workspace that is too small, a bad codec / block-size id / alignment -- all before the first launch
    for bsid, codec, align in ((0, 0, 0), (7, 0, 0), (0, 2, 0), (0, 0, 13)):
        assert compress(2, bsid, codec, align) == HIP_INVALID_VALUE, (bsid, codec, align)
    assert decompress(2) == HIP_INVALID_VALUE
    assert compress(2, ws=VP(ws.value + 8), ws_bytes=big) == HIP_INVALID_VALUE and decompress(2, ws=VP(ws.value + 8), ws_bytes=big) == HIP_INVALID_VALUE
    assert all(x == 0 for x in a) and not any(room)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_python_pair_takes_a_base():
    from finitestateentropy_amd import api
    for f in (api.compress_tensors, api.FseHip.compress_tensors, api.decompress_tensors, api.FseHip.decompress_tensors):
        par = inspect.signature(f).parameters
        assert "base" in par and par["base"].default is None, f
    assert list(inspect.signature(api.compress_tensors).parameters) == ["tensors", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.decompress_tensors).parameters) == ["obj", "base"]
    for name in ("planes_split_xor_dbatch", "planes_merge_xor_dbatch", "tensor_compress_delta_dbatch", "tensor_decompress_delta_dbatch"):
        assert "base" in inspect.signature(getattr(api.FseHip, name)).parameters, name
    old_way = api.CompressedTensors([], [], [], None, 0, 5)
    assert old_way.delta is False and old_way.nbytes == 0
    assert api.CompressedTensors([], [], [], None, 0, 5, delta=True).delta is True


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("codec", [0, 1])
def test_planes_of_a_bf16_update_xor_its_base_take_less_than_half(checker, codec):
    old, new = pdc.bf16_update_pair()
    assert old.size == new.size == 2 << 18 and (old != new).any()

    def frames(raw):
        return [checker.frame_compress(np.ascontiguousarray(pl), 5, codec)[0] for pl in pc.planes_of(raw, 2)]
    plain, delta = frames(new), frames(old ^ new)
    print("bf16 N(0, 0.02) + N(0, 2e-5), %d bytes, codec %d: planes of the new tensor %s = %d, planes of new XOR old %s = %d (%.3f)"
          % (new.size, codec, plain, sum(plain), delta, sum(delta), sum(delta) / sum(plain)))
    assert 0 < sum(delta) < sum(plain) / 2
    unchanged = frames(new ^ new)
    print("unchanged tensor: planes %s" % unchanged)
    assert sum(unchanged) < 200

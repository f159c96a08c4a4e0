"""Sparse planes without a device (include/fsehip.h, "sparse planes"): the numpy model of planes_sparse_corpus.py is a bijection -- every size
0 .. 40, all-zero and all-non-zero units, non-zeros in the last partial mask byte only, both sides of both inequalities of the writer rule,
random units -- and refuses what the reader rule refuses; the library exports the seven calls and decides every argument error before any
device call, with nothing written; the Python surface (SparsePlanes, sparse_permille) is as specified and the pinned signatures are unchanged;
and the reason for the feature: the oracle's frames of the sparse contents of the planes of a bf16 weight update, against those of the
planes themselves."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_delta_corpus as pdc
import planes_sparse_corpus as sp
import planes_sub_corpus as psc
from planes_corpus import CORRUPT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI, CI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint, C.c_int
EXPORTS = ("FSEHIP_sparse_workspaceBound", "FSEHIP_sparse_pack_dbatch", "FSEHIP_sparse_expand_dbatch", "FSEHIP_tensor_compress_sparse_dbatch",
           "FSEHIP_tensor_decompress_sparse_dbatch", "FSEHIP_tensor_compress_seg_sparse_dbatch", "FSEHIP_tensor_decompress_seg_sparse_dbatch")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


def _round_trip(unit, permille):
    """pack, the form it took, expand: -> (content, sparse?)"""
    unit = np.asarray(unit, np.uint8)
    n, nnz, m = len(unit), int((unit != 0).sum()), sp.mask_bytes(len(unit))
    c = sp.pack_unit(unit, permille)
    sparse = nnz * 1000 <= n * permille and m + nnz < n
    assert len(c) == (m + nnz if sparse else n) and (sparse or (c == unit).all()) and len(c) <= n
    if sparse:
        bits = [(int(c[i >> 3]) >> (i & 7)) & 1 for i in range(8 * m)]      # LSB first, by the definition
        assert bits[:n] == [int(x != 0) for x in unit] and not any(bits[n:]) and (c[m:] == unit[unit != 0]).all()
    res, back = sp.expand_unit(c, n)
    assert res == n and (back == unit).all()
    return c, sparse


# ---------------------------------------------------------------------------------------------------------------- 1
def test_model_is_a_bijection_on_small_and_special_units():
    rng = np.random.default_rng(11)
    for n in range(41):
        for permille in (0, 1, 125, 500, 999, 1000):
            _round_trip(np.zeros(n, np.uint8), permille)
            _round_trip(rng.integers(1, 256, n, dtype=np.uint8), permille)
            for nnz in {0, 1, n // 8, n // 2, max(n - 1, 0)}:
                _round_trip(sp.with_density(n, min(nnz, n), 100 * n + nnz), permille)
    # all zero: sparse from two bytes on, at every permille; all non-zero: never
    assert [_round_trip(np.zeros(n, np.uint8), 0)[1] for n in (0, 1, 2, 8, 9)] == [False, False, True, True, True]
    assert not any(_round_trip(np.full(n, 3, np.uint8), 1000)[1] for n in (1, 8, 9, 64, 4099))
    # non-zeros only in the last, partial mask byte
    for n in (9, 17, 33, 39, 4099):
        u = np.zeros(n, np.uint8)
        u[8 * (n // 8):] = 255
        c, sparse = _round_trip(u, 1000)
        assert sparse and c[sp.mask_bytes(n) - 1] == (1 << (n % 8)) - 1 and not c[:sp.mask_bytes(n) - 1].any()


def test_both_sides_of_both_inequalities_of_the_writer_rule():
    # nnz * 1000 <= n * permille: n = 4000, permille 250 admits 1000 non-zeros and not 1001 (the second inequality holds for both)
    assert _round_trip(sp.with_density(4000, 1000, 1), 250)[1] and not _round_trip(sp.with_density(4000, 1001, 2), 250)[1]
    assert _round_trip(sp.with_density(4000, 1000, 1), 251)[1] and not _round_trip(sp.with_density(4000, 1000, 1), 249)[1]
    # m + nnz < n: n = 64, m = 8 admits 55 non-zeros and not 56 (equality), at a permille that admits both
    assert _round_trip(sp.with_density(64, 55, 3), 1000)[1] and not _round_trip(sp.with_density(64, 56, 4), 1000)[1]
    assert not _round_trip(sp.with_density(64, 57, 5), 1000)[1]
    # ... and with a partial mask byte: n = 65, m = 9
    assert _round_trip(sp.with_density(65, 55, 6), 1000)[1] and not _round_trip(sp.with_density(65, 56, 7), 1000)[1]
    assert sp.is_sparse(1 << 45, 1 << 44, 500) and not sp.is_sparse(1 << 45, (1 << 44) + 1, 500), "64-bit products"
    assert sp.flip_permille(4000, 1000, 4000, 1001) == 250 and sp.flip_permille(64, 8, 64, 8) is None


def test_random_units_round_trip_and_pack_model_lays_contents_back_to_back():
    rng = np.random.default_rng(12)
    units = [sp.with_density(int(n), int(rng.integers(0, n + 1)), 50 + k) for k, n in enumerate(rng.integers(1, 5000, 40))]
    for permille in (0, 300, 1000):
        contents, off = sp.pack_model(units, permille)
        assert off[0] == 0 and [b - a for a, b in zip(off[:-1], off[1:])] == [len(c) for c in contents] and off[-1] <= sum(len(u) for u in units)
        for u, c in zip(units, contents):
            res, back = sp.expand_unit(c, len(u))
            assert res == len(u) and (back == u).all()
    assert any(len(c) < len(u) for u, c in zip(units, sp.pack_model(units, 1000)[0])) and all(len(c) == len(u) or not u.any() for u, c in zip(units, sp.pack_model(units, 0)[0]))


def test_every_reader_refusal():
    unit = sp.with_density(77, 20, 9)
    unit[76] = 0
    cases = sp.damaged_contents(unit)
    assert [name for name, _, _ in cases] == ["longer than the unit", "shorter than the mask", "popcount one short", "popcount one over", "a padding bit",
                                              "a zero among the values"]
    for name, content, n in cases:
        assert sp.expand_unit(content, n) == (CORRUPT, None), name
    # an error of the frame reader passes through, in front of everything else
    assert sp.expand_unit(-3, 77) == (-3, None) and sp.expand_unit(-1, 0) == (-1, None)
    # c == n is dense whatever it holds: an all-zero content of the unit's size is the all-zero unit
    res, back = sp.expand_unit(np.zeros(77, np.uint8), 77)
    assert res == 77 and not back.any()
    # the smallest sparse content: a mask alone
    res, back = sp.expand_unit(np.zeros(10, np.uint8), 77)
    assert res == 77 and not back.any()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    lib.FSEHIP_sparse_workspaceBound.restype = SZ
    a = (C.c_uint64 * 8)()
    room = (C.c_uint8 * 512)()
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    big = SZ(1 << 40)

    # the bound: host arithmetic, a multiple of 256 that grows with both arguments; GENERIC where the launch cannot be made
    b0, b1, b2 = (lib.FSEHIP_sparse_workspaceBound(U64(c), SZ(n)) for c, n in ((0, 0), (1 << 20, 4), (1 << 30, 4096)))
    assert 0 < b0 <= b1 < b2 < (1 << 30) and b0 % 256 == b1 % 256 == b2 % 256 == 0
    for c, n in ((1 << 46, 1), (32768 << 24, 1), (8, 1 << 31), (8, 1 << 24)):
        assert lib.FSEHIP_sparse_workspaceBound(U64(c), SZ(n)) > (1 << 62), (c, n)

    def pack(ptrs=None, n=1, cap=8, permille=500, w=ws, wb=big):             # ptrs: contents, content offsets, units, unit offsets
        q = list(ptrs or [p] * 4)
        return lib.FSEHIP_sparse_pack_dbatch(*q, SZ(n), U64(cap), UI(permille), w, wb, null)

    def expand(ptrs=None, n=1, cap=8, w=ws, wb=big):                         # ptrs: units, unit results, unit offsets, contents, content offsets, content results
        q = list(ptrs or [p] * 6)
        return lib.FSEHIP_sparse_expand_dbatch(*q[:3], SZ(n), U64(cap), q[3], U64(8), q[4], q[5], w, wb, null)

    def compress(E=2, op=0, base=p, permille=500, bsid=0, codec=0, codecs=null, policy=0, tol=0, align=0, src=p, planes=p, contents=p, coff=p, w=ws, wb=big, n=1,
                 cap=8):
        return lib.FSEHIP_tensor_compress_sparse_dbatch(p, U64(64), p, p, p, src, base, UI(op), p, SZ(n), UI(E), U64(cap), SZ(4), UI(bsid), CI(codec), codecs, CI(policy),
                                                        UI(tol), UI(align), UI(permille), planes, p, contents, coff, w, wb, null)

    def compress_seg(E=2, op=0, base=p, permille=500, bsid=0, codec=0, codecs=null, policy=0, tol=0, align=0, src=p, planes=p, contents=p, coff=p, w=ws, wb=big, n=1,
                     cap=8, seg_log=10, first=p, so=p):
        return lib.FSEHIP_tensor_compress_seg_sparse_dbatch(p, U64(64), p, p, p, src, base, UI(op), p, SZ(n), UI(E), U64(cap), first, SZ(E), UI(seg_log), SZ(4), UI(bsid),
                                                            CI(codec), codecs, CI(policy), UI(tol), UI(align), UI(permille), planes, p, so, contents, coff, w, wb, null)

    def decompress(E=2, op=0, base=p, contents=p, coff=p, cres=p, planes=p, w=ws, wb=big, n=1, cap=8):
        return lib.FSEHIP_tensor_decompress_sparse_dbatch(p, p, U64(cap), base, UI(op), p, p, p, SZ(n), UI(E), SZ(4), contents, U64(8), coff, cres, planes, U64(8), p, p,
                                                          w, wb, null)

    def decompress_seg(E=2, op=0, base=p, contents=p, coff=p, cres=p, planes=p, w=ws, wb=big, n=1, cap=8, seg_log=10, first=p):
        return lib.FSEHIP_tensor_decompress_seg_sparse_dbatch(p, p, U64(cap), base, UI(op), p, p, p, SZ(n), UI(E), first, SZ(E), UI(seg_log), SZ(4), contents, U64(8),
                                                              coff, cres, planes, U64(8), p, p, p, p, w, wb, null)

    # pack and expand: every array, the threshold, the counts, the launch, the workspace
    for k in range(4):
        q = [p] * 4
        q[k] = null
        assert pack(q) == HIP_INVALID_VALUE, k
    for k in range(6):
        q = [p] * 6
        q[k] = null
        assert expand(q) == HIP_INVALID_VALUE, k
    for permille in (1001, 5000, 0xFFFFFFFF):
        assert pack(permille=permille) == HIP_INVALID_VALUE
    for call in (pack, expand):
        assert call(n=1 << 31) == HIP_INVALID_VALUE and call(cap=1 << 46) == HIP_INVALID_VALUE and call(cap=32768 << 24) == HIP_INVALID_VALUE
        assert call(w=null, wb=SZ(0)) == HIP_INVALID_VALUE and call(w=null) == HIP_INVALID_VALUE
        assert call(w=VP(ws.value + 8)) == HIP_INVALID_VALUE
        assert call(wb=SZ(lib.FSEHIP_sparse_workspaceBound(U64(8), SZ(1)) - 1)) == HIP_INVALID_VALUE
    # the composites
    writers, readers = (compress, compress_seg), (decompress, decompress_seg)
    for call in writers + readers:
        for E in (0, 3, 5, 16, 0xFFFFFFFF):
            assert call(E=E) == HIP_INVALID_VALUE, (call.__name__, E)
        for op in (2, 0xFFFFFFFF):
            assert call(op=op) == HIP_INVALID_VALUE and call(op=op, base=null) == HIP_INVALID_VALUE, (call.__name__, op)
        for E in (1, 2, 4, 8):
            assert call(E=E, contents=null) == HIP_INVALID_VALUE and call(E=E, coff=null) == HIP_INVALID_VALUE, (call.__name__, E)
            assert call(E=E, n=(1 << 31) // E) == HIP_INVALID_VALUE
        assert call(cap=1 << 46) == HIP_INVALID_VALUE
        assert call(w=null, wb=SZ(0)) == HIP_INVALID_VALUE and call(w=VP(ws.value + 8)) == HIP_INVALID_VALUE
        # the sparse head of the workspace alone is not enough: the writer's / the reader's follows it
        assert call(wb=SZ(lib.FSEHIP_sparse_workspaceBound(U64(8), SZ(2)))) == HIP_INVALID_VALUE
    for call in writers:
        for permille in (1001, 0xFFFFFFFF):
            assert call(permille=permille) == HIP_INVALID_VALUE, call.__name__
        for bsid, codec, align in ((7, 0, 0), (0, 2, 0), (0, 0, 13)):
            assert call(bsid=bsid, codec=codec, align=align) == HIP_INVALID_VALUE, (call.__name__, bsid, codec, align)
        assert call(codecs=p, policy=2) == HIP_INVALID_VALUE and call(codecs=p, policy=1, tol=1001) == HIP_INVALID_VALUE
        assert call(src=null) == HIP_INVALID_VALUE and call(planes=null) == HIP_INVALID_VALUE and call(E=1, planes=null) == HIP_INVALID_VALUE
    for call in readers:
        assert call(cres=null) == HIP_INVALID_VALUE and call(planes=null) == HIP_INVALID_VALUE
    for call in (compress_seg, decompress_seg):
        assert call(seg_log=9) == HIP_INVALID_VALUE and call(seg_log=31) == HIP_INVALID_VALUE and call(first=null) == HIP_INVALID_VALUE
    assert compress_seg(bsid=2, seg_log=11) == HIP_INVALID_VALUE and compress_seg(so=null) == HIP_INVALID_VALUE
    assert all(x == 0 for x in a) and not any(room), "nothing is written"


# ---------------------------------------------------------------------------------------------------------------- 3
def test_python_surface():
    import finitestateentropy_amd
    from finitestateentropy_amd import api
    assert finitestateentropy_amd.SparsePlanes is api.SparsePlanes and "SparsePlanes" in finitestateentropy_amd.__all__
    s = api.SparsePlanes()
    assert (s.codec, s.permille) == (0, 500) and s == api.SparsePlanes(0, 500) and s != api.SparsePlanes(1) and hash(s) == hash(api.SparsePlanes(0, 500))
    assert api.SparsePlanes(1).codec == 1 and api.SparsePlanes(1, 0).permille == 0 and api.SparsePlanes(permille=1000).permille == 1000
    auto = api.SparsePlanes(api.AutoCodec(50), 250)
    assert auto.codec == api.AutoCodec(50) and auto.permille == 250 and "AutoCodec(50)" in repr(auto)
    for bad in (2, -1, None, "fse", True, api.SparsePlanes(0)):
        with pytest.raises(ValueError):
            api.SparsePlanes(bad)
    for bad in (-1, 1001, 0.5, None, True):
        with pytest.raises(ValueError):
            api.SparsePlanes(0, bad)
    # the object: a class-level default, set on the instance as segment_log is
    assert api.CompressedTensors.sparse_permille is None
    obj = api.CompressedTensors([], [], [], None, 0, 5)
    assert obj.sparse_permille is None and "sparse_permille" not in vars(obj)
    # the pinned signatures
    assert list(inspect.signature(api.compress_tensors).parameters) == ["tensors", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.compress_tensors_segmented).parameters) == ["tensors", "segment_log", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.decompress_tensors).parameters) == ["obj", "base"]
    assert list(inspect.signature(api.CompressedTensors.__init__).parameters) == ["self", "groups", "dtypes", "shapes", "device", "codec", "block_size_id", "delta"]
    assert list(inspect.signature(api.decompress_tensor_windows).parameters) == ["obj", "windows", "base"]
    assert list(inspect.signature(api.patch_tensor_windows).parameters) == ["obj", "tensors", "windows", "base"]
    # the low-level methods mirror the seven C calls
    for name in ("sparse_workspace_bound", "sparse_pack_dbatch", "sparse_expand_dbatch", "tensor_compress_sparse_dbatch", "tensor_decompress_sparse_dbatch",
                 "tensor_compress_seg_sparse_dbatch", "tensor_decompress_seg_sparse_dbatch"):
        assert callable(getattr(api.FseHip, name)), name
    for name in ("tensor_compress_sparse_dbatch", "tensor_compress_seg_sparse_dbatch"):
        par = inspect.signature(getattr(api.FseHip, name)).parameters
        assert par["permille"].default == 500 and par["base"].default is None and par["delta_op"].default == 0 and "contents" in par, name
    # windows and patches of a sparse object: ValueError before any launch (nothing here has a device)
    seg = api.CompressedTensors([], [], [], None, api.SparsePlanes(1), 5)
    seg.segment_log, seg.sparse_permille = 18, 500
    hip = api.FseHip.__new__(api.FseHip)
    with pytest.raises(ValueError, match="sparse"):
        api.FseHip.decompress_tensor_windows(hip, seg, [])
    with pytest.raises(ValueError, match="sparse"):
        api.FseHip.patch_tensor_windows(hip, seg, [], [])
    # an empty call carries the threshold through without a device
    empty = api.FseHip.compress_tensors(hip, [], api.SparsePlanes(1, 300))
    assert empty.sparse_permille == 300 and empty.codec == api.SparsePlanes(1, 300) and empty.groups == []
    assert api.FseHip.compress_tensors(hip, [], 1).sparse_permille is None


# ---------------------------------------------------------------------------------------------------------------- 4
def table_sums(frame_size):
    """{(delta, codec): (dense sum, sparse sum)} with frame_size(content, codec) -> the frame's bytes; the symbols of the sparse contents"""
    old, new = pdc.bf16_update_pair()
    out, symbols = {}, {}
    for name, delta in (("xor", old ^ new), ("sub", psc.forward(new, old, 2))):
        planes = [np.ascontiguousarray(p) for p in pc.planes_of(delta, 2)]
        contents = [sp.pack_unit(p, 500) for p in planes]
        symbols[name] = [len(c) for c in contents]
        for codec in (0, 1):
            out[(name, codec)] = (sum(frame_size(p, codec) for p in planes), sum(frame_size(c, codec) for c in contents))
    return out, symbols


def test_size_table_of_the_bf16_update_pair(checker):
    got, symbols = table_sums(lambda content, codec: checker.frame_compress(content, 5, codec)[0])
    print(got, symbols)
    assert got == sp.TABLE
    assert symbols["xor"] == [115473, 33812], "0.28 of the 2 x 262,144 symbols"
    for name in ("xor", "sub"):
        (fd, fs), (hd, hs) = got[(name, 0)], got[(name, 1)]
        assert hs < 0.75 * hd and fs <= fd and hs <= 1.08 * fd, (name, hs / hd, fs / fd, hs / fd)

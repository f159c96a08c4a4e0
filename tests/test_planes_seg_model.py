"""Segmented planes without a device (include/fsehip.h, "segmented planes"): FSEHIP_planes_segmentFirst against the brute-force model of
planes_seg_corpus.py and its refusals; the reason the feature needs no new format -- with the oracle's frame writer the segment frames of a
plane hold the single frame's blocks byte for byte and cost eight bytes per additional frame; the block bound that stays sufficient; the
fold's verdict, one case per branch, with deliberately broken variants of the model told apart; and the new calls' argument checks, which
answer before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_dev_corpus as fdc
import planes_corpus as pc
import planes_seg_corpus as psc
from planes_corpus import CORRUPT, GENERIC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
ERR = (1 << 64) - 1
SZ, VP, U64 = C.c_size_t, C.c_void_p, C.c_uint64
EXPORTS = ("FSEHIP_planes_segmentFirst", "FSEHIP_planes_segments_dbatch", "FSEHIP_planes_fold_segments_dbatch", "FSEHIP_tensor_compress_seg_dbatch",
           "FSEHIP_tensor_decompress_seg_dbatch")
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    lib = C.CDLL(path)
    lib.FSEHIP_planes_segmentFirst.restype = SZ
    return lib


def _segment_first(lib, sizes, E, seg_log, fill=True):
    offs = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)
    out = np.full(len(sizes) * E + 2, 0xA5A5A5A5, dtype=np.uint64)
    r = lib.FSEHIP_planes_segmentFirst(out.ctypes.data_as(VP) if fill else VP(0), offs.ctypes.data_as(VP), SZ(len(sizes)), C.c_uint(E), C.c_uint(seg_log))
    assert int(out[-1]) == 0xA5A5A5A5, "one entry more than planes, no further"
    return int(r), [int(x) for x in out[:-1]]


@pytest.mark.parametrize("E", psc.ELEMS)
def test_segment_first_against_the_model(lib, E):
    rng = np.random.default_rng(20 + E)
    for seg_log in (10, 11, 14):
        s = 1 << seg_log
        sizes = psc.seg_sizes(E, seg_log) + [int(x) for x in rng.integers(0, 5 * E * s, 20)]
        planes = psc.plane_sizes(sizes, E)
        assert {0, 1, s - 1, s, s + 1, 2 * s, 2 * s + 1} <= set(planes)
        if E > 1:                                            # the planes of one tensor with different counts
            assert any(len({psc.seg_count(planes[i * E + p], seg_log) for p in range(E)}) > 1 for i in range(len(sizes)))
        want = psc.seg_first(sizes, E, seg_log)
        assert want[-1] == sum(max(1, -(-x // s)) for x in planes)
        r, got = _segment_first(lib, sizes, E, seg_log)
        assert r == want[-1] and got == want
        assert _segment_first(lib, sizes, E, seg_log, fill=False)[0] == want[-1], "the count alone"
        # the Python arithmetic is the same function
        from finitestateentropy_amd.api import FseHip
        assert [int(x) for x in FseHip.planes_segment_first(None, sizes, E, seg_log)] == want
    assert _segment_first(lib, [], E, 10) == (0, [0])


def test_segment_first_refusals(lib):
    assert _segment_first(lib, [5], 1, 10) == (1, [0, 1])
    for E in (0, 3, 16):
        offs = (U64 * 2)(0, 5)
        assert lib.FSEHIP_planes_segmentFirst(VP(0), offs, SZ(1), C.c_uint(E), C.c_uint(10)) == ERR, E
    offs = (U64 * 2)(0, 5)
    for seg_log in (0, 9, 31, 64):
        assert lib.FSEHIP_planes_segmentFirst(VP(0), offs, SZ(1), C.c_uint(2), C.c_uint(seg_log)) == ERR, seg_log
    # 2^31 segments or more: one tensor of 2^41 bytes at 1 KB segments is exactly 2^31; a byte less, one segment less
    big = (U64 * 2)(0, 1 << 41)
    assert lib.FSEHIP_planes_segmentFirst(VP(0), big, SZ(1), C.c_uint(1), C.c_uint(10)) == ERR
    big = (U64 * 2)(0, (1 << 41) - 1024)
    assert lib.FSEHIP_planes_segmentFirst(VP(0), big, SZ(1), C.c_uint(1), C.c_uint(10)) == (1 << 31) - 1
    from finitestateentropy_amd.api import FseHip
    for args in (([5], 3, 10), ([5], 2, 9), ([5], 2, 31), ([1 << 41], 1, 10), ([-1], 1, 10)):
        with pytest.raises((ValueError, TypeError)):
            FseHip.planes_segment_first(None, *args)


def _plane_frames(oracle, bsid, codec, seg_log):
    """the oracle's single frame of a plane of 150,001 bytes of bf16 N(0, 0.02) data (plane 1: sign and exponent; plane 0 with codec 1) and the
    frames of its segments"""
    key = (bsid, codec, seg_log)
    if key not in _CACHE:
        if "planes" not in _CACHE:
            _CACHE["planes"] = [np.ascontiguousarray(p) for p in pc.planes_of(pc.bf16_gaussian(150001, 7), 2)]
        plane = _CACHE["planes"][1 - codec]
        assert plane.size == 150001
        r, buf = oracle.frame_compress(plane, bsid, codec)
        whole = buf[:r].copy()
        parts = []
        for a in range(0, plane.size, 1 << seg_log):
            r, buf = oracle.frame_compress(plane[a:a + (1 << seg_log)], bsid, codec)
            parts.append(buf[:r].copy())
        _CACHE[key] = (plane, whole, parts)
    return _CACHE[key]


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("bsid,seg_kib", [(0, 1), (0, 4), (0, 32), (0, 64), (5, 32), (5, 64)])
def test_segment_frames_hold_the_single_frames_blocks(checker, bsid, seg_kib, codec):
    seg_log = 10 + seg_kib.bit_length() - 1
    assert 1 << seg_log == seg_kib << 10 and seg_log >= 10 + bsid
    plane, whole, parts = _plane_frames(checker, bsid, codec, seg_log)
    assert len(parts) == psc.seg_count(plane.size, seg_log) > 1
    assert sum(len(f) for f in parts) == len(whole) + 8 * (len(parts) - 1)
    assert all((f[:5] == whole[:5]).all() for f in parts), "the same five bytes of header"
    assert (np.concatenate([f[5:-3] for f in parts]) == whole[5:-3]).all(), "the block regions concatenate to the single frame's"
    back = np.concatenate([checker.frame_decompress(f, 1 << seg_log)[1][:min(1 << seg_log, plane.size - k * (1 << seg_log))] for k, f in enumerate(parts)])
    assert (back == plane).all()


@pytest.mark.parametrize("E", psc.ELEMS)
def test_block_bound_covers_the_segment_frames(lib, E):
    f = lib.FSEHIP_planes_blockBound
    f.restype = SZ
    rng = np.random.default_rng(50 + E)
    for bsid, seg_log in ((0, 10), (0, 11), (0, 13), (2, 12), (5, 15), (5, 16)):
        s = 1 << seg_log
        sizes = psc.seg_sizes(E, seg_log) + [int(x) for x in rng.integers(0, 4 * E * s, 12)]
        blocks = 0
        for size in psc.plane_sizes(sizes, E):
            for a in (range(0, size, s) if size else [0]):
                blocks += fdc.block_count(min(s, size - a), bsid)
        unsegmented = sum(fdc.block_count(x, bsid) for x in psc.plane_sizes(sizes, E))
        assert blocks == unsegmented, "full segments are whole blocks: not a block more than one frame per plane has"
        assert blocks <= f(SZ(sum(sizes)), SZ(len(sizes)), C.c_uint(E), C.c_uint(bsid))


def test_fold_verdict_one_case_per_branch_and_broken_models_told_apart():
    for seg_log in (10, 20):
        cases = psc.fold_cases(seg_log)
        for name, off, res, want in cases:
            assert len(off) == len(res) + 1
            assert psc.fold_verdict(off, res, seg_log) == want, name
        assert {w for _, _, _, w in cases} >= {GENERIC, CORRUPT, 0, -3, -2}
        for variant in psc.VARIANTS:
            differs = [name for name, off, res, want in cases if psc.fold_verdict(off, res, seg_log, variant) != want]
            assert differs, "no case tells the model with '%s' from the right one" % variant
    # the whole-array form: planes cut by segFirst, the entry behind a plane's last segment is its neighbour's and is not looked at
    s = 1 << 10
    first = [0, 2, 2, 3, 6]
    off = [0, s, s + 9, 5000, 5000 + s, 5000 + 2 * s, 9000]
    res = [s, 9, 77, s, s, -4]
    assert psc.fold_model(off, res, first, 10) == ([0, s + 9, s + 9, 5000], [s + 9, GENERIC, 77, -4])


def test_segments_model_refuses_only_the_tensor_whose_counts_are_wrong():
    E, seg_log = 2, 10
    sizes = [5000, 0, 4097, 2048]
    right = psc.seg_first(sizes, E, seg_log)
    assert right == [0, 3, 6, 7, 8, 11, 13, 14, 15]
    off, res = psc.segments_model(sizes, E, seg_log)
    assert res == sizes and off[:7] == [0, 1024, 2048, 2500, 3524, 4548, 5000] and off[-1] == sum(sizes)
    # tensor 2: plane 0 one segment short, plane 1 one too many -- every other plane's count is its own
    wrong = list(right)
    wrong[2 * E + 1] -= 1
    off2, res2 = psc.segments_model(sizes, E, seg_log, wrong)
    assert res2 == [5000, 0, GENERIC, 2048]
    a, b = right[2 * E], right[3 * E]
    assert off2[:a] == off[:a] and off2[b:] == off[b:] and off2[a:b] == [5000] * (b - a)
    # a capacity inside tensor 2: it and tensor 3 collapse onto its start, their counts stay
    off3, res3 = psc.segments_model(sizes, E, seg_log, capacity=5001)
    assert res3 == [5000, 0, GENERIC, GENERIC] and off3[:a] == off[:a] and off3[a:] == [5000] * (len(off) - a)


def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    a = (C.c_uint64 * 8)()
    p = C.cast(a, VP)
    null = VP(0)
    u, i = C.c_uint, C.c_int
    sg, fo = lib.FSEHIP_planes_segments_dbatch, lib.FSEHIP_planes_fold_segments_dbatch
    tc, td = lib.FSEHIP_tensor_compress_seg_dbatch, lib.FSEHIP_tensor_decompress_seg_dbatch

    def compress(E=2, seg_log=10, nseg=2, bsid=0, codec=0, codecs=null, policy=0, tol=0, align=0, planes=p, base=null, ws=null, first=p, so=p):
        return tc(p, U64(64), p, p, p, p, base, p, SZ(1), u(E), U64(8), first, SZ(nseg), u(seg_log), SZ(4), u(bsid), i(codec), codecs, i(policy), u(tol), u(align),
                  planes, p, so, ws, SZ(0), null)

    def decompress(E=2, seg_log=10, nseg=2, first=p, so=p):
        return td(p, p, U64(8), null, p, p, p, SZ(1), u(E), first, SZ(nseg), u(seg_log), SZ(4), p, U64(8), so, p, p, p, null, SZ(0), null)
    for E in (0, 3, 5, 16, 0xFFFFFFFF):
        assert sg(p, p, p, p, p, SZ(1), u(E), SZ(2), u(10), null) == HIP_INVALID_VALUE, E
        assert compress(E=E) == HIP_INVALID_VALUE and decompress(E=E) == HIP_INVALID_VALUE, E
    for seg_log in (0, 9, 31, 40):
        assert sg(p, p, p, p, p, SZ(1), u(2), SZ(2), u(seg_log), null) == HIP_INVALID_VALUE, seg_log
        assert fo(p, p, p, p, p, SZ(2), SZ(2), u(seg_log), null) == HIP_INVALID_VALUE, seg_log
        assert compress(seg_log=seg_log) == HIP_INVALID_VALUE and decompress(seg_log=seg_log) == HIP_INVALID_VALUE, seg_log
    for bsid in range(1, 7):                                 # a segment is a whole number of blocks: 10 + blockSizeId <= segLog
        assert compress(seg_log=9 + bsid, bsid=bsid) == HIP_INVALID_VALUE, bsid
    for nseg in (1 << 31, 1 << 40):
        assert sg(p, p, p, p, p, SZ(1), u(2), SZ(nseg), u(10), null) == HIP_INVALID_VALUE
        assert fo(p, p, p, p, p, SZ(2), SZ(nseg), u(10), null) == HIP_INVALID_VALUE
        assert compress(nseg=nseg) == HIP_INVALID_VALUE and decompress(nseg=nseg) == HIP_INVALID_VALUE
    assert fo(p, p, p, p, p, SZ(1 << 31), SZ(2), u(10), null) == HIP_INVALID_VALUE
    for k in range(5):
        args = [p] * 5
        args[k] = null
        assert sg(*args, SZ(1), u(2), SZ(2), u(10), null) == HIP_INVALID_VALUE, k
        assert fo(*args, SZ(2), SZ(2), u(10), null) == HIP_INVALID_VALUE, k
    # the composites: everything the steps check, in front of the first launch -- a too small workspace last of all
    assert compress(first=null) == compress(so=null) == decompress(first=null) == decompress(so=null) == HIP_INVALID_VALUE
    assert compress(bsid=7) == compress(codec=2) == compress(align=13) == HIP_INVALID_VALUE
    assert compress(codecs=p, policy=2) == compress(codecs=p, policy=1, tol=1001) == HIP_INVALID_VALUE
    assert compress(planes=null) == compress(E=1, planes=null, base=p) == HIP_INVALID_VALUE
    assert compress(ws=VP(128)) == HIP_INVALID_VALUE
    assert compress() == compress(codecs=p) == compress(E=1, planes=null) == decompress() == HIP_INVALID_VALUE, "a workspace of no bytes"
    assert all(x == 0 for x in a)

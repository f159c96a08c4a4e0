"""Byte planes of tensors without a device (include/fsehip.h, "byte planes of tensors"): the numpy model of planes_corpus.py round-trips and
its work mapping visits every (tile, tensor) intersection exactly once; the library exports the five calls, refuses bad arguments before
any device call, and its block bound is sufficient; and the reason for the feature -- the oracle's frames of the planes of bf16 data are
smaller than its frame of the raw bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_dev_corpus as fdc
import planes_corpus as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64 = C.c_size_t, C.c_void_p, C.c_uint64
EXPORTS = ("FSEHIP_planes_blockBound", "FSEHIP_planes_split_dbatch", "FSEHIP_planes_merge_dbatch", "FSEHIP_tensor_compress_dbatch",
           "FSEHIP_tensor_decompress_dbatch")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


@pytest.mark.parametrize("E", pc.ELEMS)
def test_model_round_trips(E):
    tensors = pc.random_tensors(pc.split_sizes(E, 256) + list(range(0, 41)), 3)
    out, written, P, res = pc.split_model(tensors, E)
    S = [int(x) for x in pc.offsets(tensors)]
    assert written.all() and res == [len(t) for t in tensors] and len(P) == len(tensors) * E + 1 and P[-1] == S[-1]
    for i, raw in enumerate(tensors):
        assert P[i * E] == S[i]
        planes = [out[P[i * E + p]:P[i * E + p + 1]] for p in range(E)]
        assert [len(x) for x in planes] == [pc.plane_size(len(raw), p, E) for p in range(E)]
        assert sum(len(x) for x in planes) == len(raw)
        assert (pc.merge_one(planes, E) == raw).all()
        assert pc.merge_verdict([len(x) for x in planes], S[i + 1], S[i], E, S[-1]) == len(raw)
    # a capacity inside tensor 6: it and everything behind it collapse onto its start
    k = 6
    cap = S[k] + 1
    assert S[k + 1] > cap
    _, written, P, res = pc.split_model(tensors, E, cap)
    assert res[:k] == [len(t) for t in tensors[:k]] and set(res[k:]) == {pc.GENERIC}
    assert P[k * E:] == [S[k]] * (len(P) - k * E) and not written[S[k]:].any() and written[:S[k]].all()


def test_merge_verdict_order():
    E = 4
    good = [3, 3, 2, 2]                                      # n = 10
    assert pc.merge_verdict(good, 110, 100, E, 110) == 10
    assert pc.merge_verdict(good, 111, 100, E, 110) == pc.GENERIC
    assert pc.merge_verdict([3, -3, 2, -4], 110, 100, E, 110) == -3
    assert pc.merge_verdict([3, -3, 2, -4], 111, 100, E, 110) == pc.GENERIC
    assert pc.merge_verdict([3, 2, 3, 2], 110, 100, E, 110) == pc.CORRUPT
    assert pc.merge_verdict([3, 2, 3, 2], 105, 100, E, 110) == pc.CORRUPT
    assert pc.merge_verdict(good, 109, 100, E, 110) == pc.TOO_SMALL
    assert pc.merge_verdict([0, 0, 0, 0], 100, 100, E, 110) == 0


def test_work_mapping_visits_every_intersection_once():
    rng = np.random.default_rng(11)
    T = 64
    for trial in range(60):
        kind = trial % 4
        n = int(rng.integers(0, 40))
        sizes = rng.integers(0, [1, 7, 3 * T, 9 * T][kind] + 1, n)
        S = [int(rng.integers(0, 3 * T)) if trial % 3 == 0 else 0]
        for s in sizes:
            S.append(S[-1] + int(s))
        cap = S[-1] + int(rng.integers(0, T))
        groups = -(-cap // T) + n
        want = sorted((i, t) for i in range(n) for t in range(cap // T + 1) if S[i] < S[i + 1] and t * T < S[i + 1] and (t + 1) * T > S[i])
        got = pc.work_map(S, groups, T)
        assert sorted((i, t) for _, i, t in got) == want, (trial, S)
        assert len({w for w, _, _ in got}) == len(got)


def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    a = (C.c_uint64 * 8)()
    p = C.cast(a, VP)
    null = VP(0)
    s = lib.FSEHIP_planes_split_dbatch
    m = lib.FSEHIP_planes_merge_dbatch
    for E in (0, 3, 5, 6, 7, 16, 0xFFFFFFFF):
        assert s(p, p, p, p, p, SZ(1), C.c_uint(E), U64(8), null) == HIP_INVALID_VALUE, E
        assert m(p, p, p, p, p, p, SZ(1), C.c_uint(E), U64(8), null) == HIP_INVALID_VALUE, E
        assert lib.FSEHIP_tensor_compress_dbatch(p, U64(64), p, p, p, p, p, SZ(1), C.c_uint(E), U64(8), SZ(4), C.c_uint(0), C.c_int(0), C.c_uint(0), p, p, null, SZ(0),
                                                 null) == HIP_INVALID_VALUE, E
        assert lib.FSEHIP_tensor_decompress_dbatch(p, p, U64(8), p, p, p, SZ(1), C.c_uint(E), SZ(4), p, U64(8), p, p, null, SZ(0), null) == HIP_INVALID_VALUE, E
    for E in (1, 2, 4, 8):
        for k in (1, 2, 4):                                  # plane offsets, results, source offsets
            args = [p, p, p, p, p]
            args[k] = null
            assert s(*args, SZ(1), C.c_uint(E), U64(8), null) == HIP_INVALID_VALUE, (E, k)
        for k in range(6):
            args = [p] * 6
            args[k] = null
            assert m(*args, SZ(1), C.c_uint(E), U64(8), null) == HIP_INVALID_VALUE, (E, k)
    for k in (0, 3):                                         # planes and source: needed from two bytes per element on
        args = [p, p, p, p, p]
        args[k] = null
        assert s(*args, SZ(1), C.c_uint(2), U64(8), null) == HIP_INVALID_VALUE, k
    # the composites: a workspace that is too small, a bad codec / block-size id / alignment -- all before the first launch
    tc = lib.FSEHIP_tensor_compress_dbatch
    for bsid, codec, align in ((0, 0, 0), (7, 0, 0), (0, 2, 0), (0, 0, 13)):
        assert tc(p, U64(64), p, p, p, p, p, SZ(1), C.c_uint(2), U64(8), SZ(4), C.c_uint(bsid), C.c_int(codec), C.c_uint(align), p, p, null, SZ(0),
                  null) == HIP_INVALID_VALUE, (bsid, codec, align)
    assert lib.FSEHIP_tensor_decompress_dbatch(p, p, U64(8), p, p, p, SZ(1), C.c_uint(2), SZ(4), p, U64(8), p, p, null, SZ(0), null) == HIP_INVALID_VALUE
    assert all(x == 0 for x in a)


def test_block_bound(lib):
    f = lib.FSEHIP_planes_blockBound
    f.restype = SZ
    err = (1 << 64) - 1
    for bsid in range(7):
        bs = 1024 << bsid
        for total, n, E in ((0, 0, 1), (0, 5, 8), (1, 1, 2), (bs, 1, 4), (bs + 1, 3, 2), (10 * bs - 1, 7, 8), ((1 << 30) + 5, 1024, 2)):
            assert f(SZ(total), SZ(n), C.c_uint(E), C.c_uint(bsid)) == -(-total // bs) + n * E, (bsid, total, n, E)
    assert f(SZ(100), SZ(1), C.c_uint(2), C.c_uint(7)) == err and f(SZ(100), SZ(1), C.c_uint(3), C.c_uint(0)) == err
    # sufficient: the blocks of all planes never exceed it
    rng = np.random.default_rng(5)
    for E in pc.ELEMS:
        sizes = [int(x) for x in rng.integers(0, 5000, 50)] + [1024 * E, 1024 * E + 1, 2048 * E - 1]
        blocks = sum(fdc.block_count(pc.plane_size(n, p, E), 0) for n in sizes for p in range(E))
        assert blocks <= f(SZ(sum(sizes)), SZ(len(sizes)), C.c_uint(E), C.c_uint(0))


@pytest.mark.parametrize("codec", [0, 1])
def test_planes_of_bf16_data_compress_better_than_the_raw_bytes(checker, codec):
    raw = pc.bf16_gaussian(1 << 18)
    whole, _ = checker.frame_compress(raw, 5, codec)
    per_plane = [checker.frame_compress(np.ascontiguousarray(p), 5, codec)[0] for p in pc.planes_of(raw, 2)]
    print("bf16 N(0, 0.02), %d bytes, codec %d: raw frame %d, planes %s = %d (%.3f of the raw frame)"
          % (raw.size, codec, whole, per_plane, sum(per_plane), sum(per_plane) / whole))
    assert 0 < sum(per_plane) < whole

"""The host arithmetic behind the packed frame writer (include/fsehip.h, FSEHIP_frame_compress_packed_dbatch): its capacity bound and its
workspace size -- and the two facts about the oracle's frames that the writer's contract rests on: laid out by the model of
frame_packed_corpus.py they stay within the bound, and the oracle's reader does not look behind a frame's end mark (so the offsets the
writer produces can be handed to a reader, padding and all).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import frame_dev_corpus as fdc
import frame_packed_corpus as fpc
from oracle.oracle import is_error

SZ = C.c_size_t


@pytest.fixture(scope="module")
def api():
    from finitestateentropy_amd.api import FseHip
    return FseHip()


@pytest.fixture(scope="module")
def oracle(restatement):
    return restatement


def test_packed_bound_is_the_formula(api):
    f = api.lib.FSEHIP_frame_packedBound
    f.restype = SZ
    batches = ([], [0], [0, 0, 0], [1], [1023, 1024, 1025], [0, 1, 15, 1024, 1025, 3077, 2500, 0, 1100 * 1024 + 7], [65536 * 3 + 1] * 5)
    for bsid in (0, 5, 6):
        for align_log in (0, 4, 12):
            for sizes in batches:
                total, n, blocks = sum(sizes), len(sizes), sum(fdc.block_count(x, bsid) for x in sizes)
                want = total + 8 * n + 5 * blocks + n * ((1 << align_log) - 1)
                assert int(f(SZ(total), SZ(n), SZ(blocks), C.c_uint(align_log))) == want == fpc.packed_bound(sizes, bsid, align_log), (bsid, align_log, sizes)
                assert api.frame_packed_bound(total, n, blocks, align_log) == want
    for align_log in (13, 64, 0xFFFFFFFF):
        assert is_error(int(f(SZ(1000), SZ(1), SZ(1), C.c_uint(align_log)))), align_log
    with pytest.raises(ValueError):
        api.frame_packed_bound(1000, 1, 1, 13)


def test_packed_workspace_size(api):
    w = api.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize
    fixed = api.lib.FSEHIP_frame_compress_dbatch_workspaceSize
    w.restype = SZ; fixed.restype = SZ
    frames = (0, 1, 2, 64, 65, 1000, 100000)
    blocks = (0, 1, 2, 1023, 1024, 1025, 40000, 300000)
    for bsid in (0, 5, 6):
        for codec in (0, 1):
            size = lambda nf, nb: int(w(SZ(nf), SZ(nb), C.c_uint(bsid), C.c_int(codec)))
            for nb in blocks:
                row = [size(nf, nb) for nf in frames]
                assert all(not is_error(x) for x in row) and row == sorted(row), (bsid, codec, nb, row)
            for nf in frames:
                col = [size(nf, nb) for nb in blocks]
                assert col == sorted(col), (bsid, codec, nf, col)
                for nb in blocks:
                    assert size(nf, nb) >= int(fixed(SZ(nf), SZ(nb), C.c_uint(bsid), C.c_int(codec))), (bsid, codec, nf, nb)
    assert is_error(int(w(SZ(1), SZ(1), C.c_uint(7), C.c_int(0)))) and is_error(int(w(SZ(1), SZ(1), C.c_uint(0), C.c_int(2))))


def test_model_offsets():
    sizes = [8, 17, -1, 0, 16, 100]                         # (-1: a frame that fails takes no room; no writer gives 0, the model takes it)
    assert fpc.packed_offsets(sizes, 0) == [0, 8, 25, 25, 25, 41, 141]
    assert fpc.packed_offsets(sizes, 4) == [0, 16, 48, 48, 48, 64, 176]
    assert fpc.packed_offsets(sizes, 4, 50) == [0, 16, 48, 48, 48, 50, 50]
    assert fpc.packed_results(sizes, 4) == sizes
    assert fpc.packed_results(sizes, 4, 50) == [8, 17, -1, 0, fpc.TOO_SMALL, fpc.TOO_SMALL]
    assert fpc.packed_results(sizes, 0, 24) == [8, fpc.TOO_SMALL, -1, 0, fpc.TOO_SMALL, fpc.TOO_SMALL]
    assert fpc.packed_offsets([], 12, 7) == [0]


@pytest.mark.parametrize("codec", [0, 1])
def test_oracle_frames_packed_stay_within_the_bound(api, oracle, codec):
    contents = [c for _, c in fdc.contents(oracle)]
    frames = fdc.frames(oracle, codec)
    sizes = [len(c) for c in contents]
    blocks = sum(fdc.block_count(n) for n in sizes)
    for align_log in (0, 4, 8, 12):
        off = fpc.packed_offsets([len(f) for f in frames], align_log)
        bound = api.frame_packed_bound(sum(sizes), len(sizes), blocks, align_log)
        assert bound == fpc.packed_bound(sizes, fdc.BSID, align_log)
        assert off[-1] <= bound, (codec, align_log, off[-1], bound)
        assert fpc.packed_results([len(f) for f in frames], align_log, bound) == [len(f) for f in frames]
        for i, f in enumerate(frames):                      # ... and frame by frame: a slot at the frame's own bound holds it
            assert off[i + 1] - off[i] <= fdc.bound(sizes[i]) + (1 << align_log) - 1, (codec, align_log, i)


@pytest.mark.parametrize("codec", [0, 1])
def test_oracle_reader_stops_at_the_end_mark(oracle, codec):
    """a frame followed by 1 to 255 bytes the writer never wrote (0xA5, as the tests fill them): the same result, the same bytes"""
    for (name, data), frame in zip(fdc.contents(oracle), fdc.frames(oracle, codec)):
        cap = len(data)
        r0, out0 = oracle.frame_decompress(frame, cap)
        assert r0 == len(data) and (out0[:r0] == data).all(), (name, codec)
        padded = np.concatenate([frame, np.full(255, 0xA5, np.uint8)])
        for pad in range(1, 256):
            r, out = oracle.frame_decompress(padded[:len(frame) + pad], cap)
            assert r == r0 and (out[:cap] == out0[:cap]).all(), (name, codec, pad)

"""The host arithmetic behind the device frame calls (include/fsehip.h, "frames on DEVICE buffers"): block counts, workspace sizes, the
binding's offset planner -- and that the oracle's frames of the test contents fit the slots the planner gives them.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import frame_dev_corpus as fdc
from oracle.oracle import is_error

SZ = C.c_size_t


@pytest.fixture(scope="module")
def api():
    from finitestateentropy_amd.api import FseHip
    return FseHip()


@pytest.fixture(scope="module")
def oracle(restatement):
    return restatement


def test_block_count(api):
    f = api.lib.FSEHIP_frame_blockCount
    f.restype = SZ
    for bsid in range(7):
        bs = 1024 << bsid
        for n in (0, 1, 1023, 1024, 1025, 65536 * 3 + 1):
            assert int(f(SZ(n), C.c_uint(bsid))) == -(-n // bs), (n, bsid)
            assert api.frame_block_count(n, bsid) == fdc.block_count(n, bsid)
    for bsid in (7, 8, 255):
        assert is_error(int(f(SZ(1000), C.c_uint(bsid)))), bsid


def test_workspace_sizes_are_monotone(api):
    w = api.lib.FSEHIP_frame_compress_dbatch_workspaceSize
    r = api.lib.FSEHIP_frame_decompress_dbatch_workspaceSize
    w.restype = SZ; r.restype = SZ
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
    assert is_error(int(w(SZ(1), SZ(1), C.c_uint(7), C.c_int(0)))) and is_error(int(w(SZ(1), SZ(1), C.c_uint(0), C.c_int(2))))
    size = lambda nf, nb: int(r(SZ(nf), SZ(nb)))
    for nb in blocks:
        row = [size(nf, nb) for nf in frames]
        assert row == sorted(row), (nb, row)
    for nf in frames:
        col = [size(nf, nb) for nb in blocks]
        assert col == sorted(col), (nf, col)


def test_planner_gives_every_frame_its_bound(api):
    api.lib.FSEHIP_frame_compressBound.restype = SZ
    sizes = [0, 1, 15, 1024, 1025, 3077, 2500, 0, 1100 * 1024 + 7]
    for bsid in (0, 2, 5, 6):
        off = api.frame_dbatch_plan(sizes, bsid)
        assert off.dtype == np.uint64 and len(off) == len(sizes) + 1 and off[0] == 0
        for i, n in enumerate(sizes):
            want = int(api.lib.FSEHIP_frame_compressBound(SZ(n), C.c_uint(bsid)))
            assert int(off[i + 1] - off[i]) == want == fdc.bound(n, bsid), (bsid, n)
    with pytest.raises(ValueError):
        api.frame_dbatch_plan(sizes, 7)


def test_oracle_frames_fit_the_bound(oracle):
    for codec in (0, 1):
        for (name, data), frame in zip(fdc.contents(oracle), fdc.frames(oracle, codec)):
            assert 8 <= len(frame) <= fdc.bound(len(data)), (name, codec, len(frame))
        forms = set()
        for frame in fdc.frames(oracle, codec):
            forms |= fdc.header_forms(frame)
        assert forms == {(t, full) for t in (0, 1, 2) for full in (False, True)}, (codec, forms)   # every block kind, full and partial
    for codec, want in ((0, 1724), (1, None)):               # the crafted frame of test_gpu_frame_device.py, as the oracle reads it
        ab, frame = fdc.crafted_short_block(oracle, codec)
        for cap in (1724, 2124):
            r, out = oracle.frame_decompress(frame, cap)
            if want is None:
                assert is_error(r) and (1 << 64) - r == 4, (codec, cap)          # corruption_detected
            else:
                assert r == want and (out[:r] == ab).all(), (codec, cap)

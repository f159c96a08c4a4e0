"""FSEHIP_frame_inspect (include/fsehip.h, "frames of UNKNOWN size") against a Python restatement and the oracle's reader, over intact,
truncated and bit-flipped frames (frame_inspect_corpus.py) -- and the fact the device plan rests on: with the content bound as its capacity
the reader decides what it decides with any larger one.  Host arithmetic only.  No GPU."""
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest
import torch

import frame_dev_corpus as fdc
import frame_inspect_corpus as fic
from oracle.oracle import err_code, is_error

SZ = C.c_size_t
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    from finitestateentropy_amd.api import FseHip
    return FseHip()


@pytest.fixture(scope="module")
def oracle(restatement):
    return restatement


def test_inspect_equals_the_restatement_and_the_bound_is_a_sufficient_capacity(api, oracle):
    corpus, want = fic.corpus(oracle), fic.inspected(oracle)
    bases = fic.bases(oracle)
    seen = Counter()
    for i, ((kind, b, f), (rw, iw)) in enumerate(zip(corpus, want)):
        rg, ig = api.frame_inspect(f)
        assert rg == rw and ig == iw, (i, kind, bases[b][0], len(f), ig, iw)
        bound, status = iw["content_bound"], iw["status"]
        r1, o1 = oracle.frame_decompress(f, bound)
        r2, o2 = oracle.frame_decompress(f, bound + 4096)
        assert r1 == r2, (i, kind, bases[b][0], len(f), bound, r1, r2)
        if not is_error(r1):
            assert (o1[:r1] == o2[:r1]).all(), (i, kind, bases[b][0])
        if status == fic.GENERIC:
            assert bound == 0 and iw["n_blocks"] == 0 and err_code(r1) == fic.GENERIC, (i, kind, r1)
        if status == 0 and not is_error(r1):
            assert r1 <= bound, (i, kind, r1, bound)
        seen["status %d" % status] += 1
        if status == 0:
            seen["status 0, fails in a block or at the checksum" if is_error(r1) else "status 0, succeeds"] += 1
        if kind == "cut" and status == fic.SRC_WRONG and err_code(r1) != fic.SRC_WRONG:
            assert is_error(r1), (i, r1)
            seen["truncated, an earlier block's error"] += 1
    print(len(corpus), "frames:", dict(seen))
    for key in ("status 0", "status 1", "status 3", "status 4", "status 0, succeeds", "status 0, fails in a block or at the checksum",
                "truncated, an earlier block's error"):
        assert seen[key] > 0, (key, dict(seen))
    assert sum(seen["status %d" % s] for s in (0, 1, 3, 4)) == len(corpus) > 15000


def test_intact_frames_announce_their_content(api, oracle):
    n = 0
    for name, f, data, bsid in fic.bases(oracle):
        r, info = api.frame_inspect(f)
        if bsid is None:
            continue
        assert info["status"] == 0 and r == info["content_bound"] == len(data), name
        assert info["n_blocks"] == fdc.block_count(len(data), bsid) and info["block_size_id"] == bsid and info["reserved"] == bytes(6), name
        assert info["checksum22"] == (oracle.xxh32(data) >> 5) & 0x3FFFFF, name
        n += 1
    assert n == 2 * len(fdc.contents(oracle)) + 4
    assert max(info["n_blocks"] for info in (api.frame_inspect(f)[1] for _, f, _, _ in fic.bases(oracle))) == 1101


def test_the_bound_is_a_capacity_not_a_size(api, oracle):
    """the crafted FSE frame: two blocks announce 1024 bytes each, the first regenerates 700"""
    ab, f = fdc.crafted_short_block(oracle, 0)
    r, info = api.frame_inspect(f)
    assert r == 2048 and info["n_blocks"] == 2 and info["status"] == 0
    ro, out = oracle.frame_decompress(f, 2048)
    assert ro == 1724 == len(ab) and (out[:ro] == ab).all()
    _, hf = fdc.crafted_short_block(oracle, 1)                # Huff0 payloads: the announced size is exact, the block fails
    r, info = api.frame_inspect(hf)
    assert r == 2048 and info["status"] == 0 and info["codec"] == 1
    assert err_code(oracle.frame_decompress(hf, 2048)[0]) == fic.CORRUPT


def test_inspect_without_an_info_record(api, oracle):
    f = api.lib.FSEHIP_frame_inspect
    f.restype = SZ
    for _, frame, _, _ in fic.bases(oracle)[:8]:
        a = np.ascontiguousarray(frame)
        assert int(f(None, a.ctypes.data_as(C.c_void_p), SZ(a.size))) == fic.inspect(frame)[0]
    assert int(f(None, None, SZ(0))) == (1 << 64) - fic.SRC_WRONG


def test_abi(api):
    from finitestateentropy_amd.api import FRAME_INFO_DTYPE, FrameInfo
    assert C.sizeof(FrameInfo) == 32 == FRAME_INFO_DTYPE.itemsize
    assert [(n, FRAME_INFO_DTYPE.fields[n][1]) for n in FRAME_INFO_DTYPE.names] == [(n, getattr(FrameInfo, n).offset) for n, _ in FrameInfo._fields_]
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    assert "uint8_t  reserved[6];" in header and "} FSEHIP_FrameInfo;" in header
    p = api.lib.FSEHIP_frame_plan_dbatch_workspaceSize
    r = api.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    p.restype = SZ; r.restype = SZ
    frames = (0, 1, 2, 64, 65, 1000, 1024, 1025, 100000)
    blocks = (0, 1, 2, 1023, 1024, 1025, 40000, 300000)
    row = [int(p(SZ(nf))) for nf in frames]
    assert row == sorted(row) and row[0] > 0
    for nb in blocks:
        row = [int(r(SZ(nf), SZ(nb))) for nf in frames]
        assert row == sorted(row), (nb, row)
    for nf in frames:
        col = [int(r(SZ(nf), SZ(nb))) for nb in blocks]
        assert col == sorted(col), (nf, col)


def test_planners_refuse_a_slot_alignment_above_4096(api):
    frames, off = torch.zeros(8, dtype=torch.uint8), np.array([0, 8], np.uint64)
    with pytest.raises(ValueError):
        api.frame_plan_dbatch(frames, off, align_log=13)
    with pytest.raises(ValueError):
        api.frame_decompress_packed_dbatch(frames, off, align_log=13)

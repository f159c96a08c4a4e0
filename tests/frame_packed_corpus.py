"""The model of the packed frame writer (FSEHIP_frame_compress_packed_dbatch, include/fsehip.h) shared by test_frame_packed_writer_plan.py
and test_gpu_frame_packed_writer.py: where frames of given sizes land for an alignment and a capacity, and what every frame's result is.
A frame's `size` here is what the oracle's writer returns for its content -- a positive size, or a negative value -c for error code c (a
frame that fails takes 0 bytes).  The batches are built once per session from frame_dev_corpus and never changed."""
import numpy as np

import frame_dev_corpus as fdc

GENERIC, TOO_SMALL = -1, -2
NO_CAP = (1 << 64) - 1
LONG_REPEATS = 171            # 12 small contents x 171 = 2052 frames: the scan over frames crosses two groups of 1024
_CACHE = {}


def packed_offsets(sizes, align_log, cap=NO_CAP):
    """d_dstOffsets: min(U[i], cap) with U the running sum of the sizes rounded up to 1 << align_log; len(sizes) + 1 python ints"""
    a = (1 << align_log) - 1
    out, u = [0], 0
    for s in sizes:
        u += (max(int(s), 0) + a) & ~a
        out.append(u)
    return [min(x, int(cap)) for x in out]


def packed_results(sizes, align_log, cap=NO_CAP):
    """d_results: the frame's own error, its size where its slot holds it, dstSize_tooSmall where the capacity cut the slot short"""
    off = packed_offsets(sizes, align_log, cap)
    return [int(s) if int(s) < 0 or off[i + 1] - off[i] >= int(s) else TOO_SMALL for i, s in enumerate(sizes)]


def packed_bound(sizes, bsid, align_log):
    """FSEHIP_frame_packedBound of contents of these sizes, restated: every frame at its FSEHIP_frame_compressBound, plus its padding"""
    return sum(fdc.bound(int(n), bsid) for n in sizes) + len(sizes) * ((1 << align_log) - 1)


def long_batch(oracle, codec):
    """the twelve small contents of frame_dev_corpus repeated LONG_REPEATS times: -> (contents, the oracle's frames)"""
    key = ("long", codec)
    if key not in _CACHE:
        contents = [c for _, c in fdc.contents(oracle)[:12]] * LONG_REPEATS
        frames = fdc.frames(oracle, codec)[:12] * LONG_REPEATS
        assert len(contents) > 2048
        _CACHE[key] = (contents, frames)
    return _CACHE[key]

"""The numpy model of the tensor deltas (include/fsehip.h, "tensor deltas") shared by test_planes_delta_model.py and test_gpu_planes_delta.py,
built on planes_corpus.py: the XOR split is the split of `tensor XOR base`, the XOR merge is the merge XORed with the base.  Plain Python,
never the library.  Tensors and bases are numpy uint8 arrays of equal sizes, pair by pair."""
import numpy as np

import planes_corpus as pc


def xor_all(tensors, bases):
    assert [len(t) for t in tensors] == [len(b) for b in bases]
    return [np.asarray(t, np.uint8) ^ np.asarray(b, np.uint8) for t, b in zip(tensors, bases)]


def split_xor_model(tensors, bases, E, capacity=None):
    """-> (planes buffer, written, plane offsets, tensor results) of FSEHIP_planes_split_xor_dbatch, as planes_corpus.split_model gives them"""
    return pc.split_model(xor_all(tensors, bases), E, capacity)


def merge_xor_one(planes, base, E):
    """the tensor whose delta against `base` these planes hold"""
    return pc.merge_one(planes, E) ^ np.asarray(base, np.uint8)


def bf16_bytes(x):
    """float32 values cut to their top 16 bits (bf16 by truncation), as bytes"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)


def bf16_update_pair(n=1 << 18, step=2e-5, sigma=0.02):
    """(old, new) of the issue: w = N(0, sigma) from default_rng(1), w2 = w + N(0, step) from default_rng(2), both float32, both cut to bf16 by
    truncation -- n elements, 2 n bytes each"""
    w = np.random.default_rng(1).normal(0, sigma, n).astype(np.float32)
    w2 = w + np.random.default_rng(2).normal(0, step, n).astype(np.float32)
    return bf16_bytes(w), bf16_bytes(w2)

"""The numpy model of the arithmetic tensor deltas (include/fsehip.h, "arithmetic tensor deltas") shared by test_planes_sub_model.py and
test_gpu_planes_sub.py, built on planes_corpus.py: the SUB split is the split of zigzag(tensor - base), the SUB merge is base + unzigzag of the
merge.  Elements are little-endian unsigned integers of E bytes counted from the tensor's start; the trailing n mod E bytes go with the
E == 1 form, each byte by itself.  Plain Python, never the library.  Tensors and bases are numpy uint8 arrays of equal sizes, pair by pair."""
import numpy as np

import planes_corpus as pc

XOR, SUB = 0, 1                # FSEHIP_DELTA_XOR, FSEHIP_DELTA_SUB
_U = {1: np.uint8, 2: np.dtype("<u2"), 4: np.dtype("<u4"), 8: np.dtype("<u8")}


def _zz(t, b, E):
    """arrays of E-byte unsigned integers -> zigzag((t - b) mod 2^W), in that width (numpy's unsigned arithmetic wraps)"""
    one = t.dtype.type(1)
    d = t - b
    z = (d << one) ^ (np.zeros_like(d) - (d >> t.dtype.type(8 * E - 1)))        # 0 - 1 wraps to 2^W - 1: the mask of a set top bit
    assert z.dtype == t.dtype
    return z


def _unzz(z, b, E):
    one = z.dtype.type(1)
    t = b + ((z >> one) ^ (np.zeros_like(z) - (z & one)))
    assert t.dtype == z.dtype
    return t


def _apply(f, x, y, E):
    x, y = np.ascontiguousarray(x, np.uint8), np.ascontiguousarray(y, np.uint8)
    assert x.shape == y.shape and x.ndim == 1
    whole = len(x) // E * E
    out = np.empty(len(x), np.uint8)
    with np.errstate(over="ignore"):
        out[:whole] = f(x[:whole].view(_U[E]), y[:whole].view(_U[E]), E).view(np.uint8)
        out[whole:] = f(x[whole:], y[whole:], 1)
    return out


def forward(t, b, E):
    """the bytes of zigzag(t - b), element by element"""
    return _apply(_zz, t, b, E)


def inverse(z, b, E):
    """the tensor whose delta against b is z"""
    return _apply(_unzz, z, b, E)


def sub_all(tensors, bases, E):
    assert [len(t) for t in tensors] == [len(b) for b in bases]
    return [forward(t, b, E) for t, b in zip(tensors, bases)]


def delta_all(tensors, bases, E, op):
    """what the planes of an *_op_dbatch call are the planes of"""
    return sub_all(tensors, bases, E) if op == SUB else [np.asarray(t, np.uint8) ^ np.asarray(b, np.uint8) for t, b in zip(tensors, bases)]


def split_sub_model(tensors, bases, E, capacity=None):
    """-> (planes buffer, written, plane offsets, tensor results) of FSEHIP_planes_split_op_dbatch with FSEHIP_DELTA_SUB"""
    return pc.split_model(sub_all(tensors, bases, E), E, capacity)


def merge_sub_one(planes, base, E):
    """the tensor whose SUB delta against `base` these planes hold"""
    return inverse(pc.merge_one(planes, E), base, E)


def edge_values(E):
    """the adversarial element values of the issue: 0, 1, 2^(W-1) - 1, 2^(W-1), 2^W - 1, 0x00FF.., 0x0100.., and for E == 8 the dword carry"""
    W = 8 * E
    v = [0, 1, (1 << (W - 1)) - 1, 1 << (W - 1), (1 << W) - 1, (1 << (W - 8)) - 1, 1 << (W - 8)]
    if E == 8:
        v += [(1 << 32) - 1, 1 << 32]
    return sorted(set(v))


def edge_pairs(E, repeat=1):
    """(t, b) as bytes: every pair over edge_values(E), each followed by the swapped pair -- neighbouring elements of a dword borrow in
    opposite directions (0 - 1 beside 1 - 0) -- the whole list `repeat` times"""
    vals = edge_values(E)
    t, b = [], []
    for x in vals:
        for y in vals:
            t += [x, y]
            b += [y, x]
    t, b = np.array(t * repeat, dtype=np.uint64), np.array(b * repeat, dtype=np.uint64)
    return t.astype(_U[E]).view(np.uint8).copy(), b.astype(_U[E]).view(np.uint8).copy()

"""The numpy model of "a transform per tensor" (include/fsehip.h) shared by test_planes_each_model.py and test_gpu_planes_each.py: it
defines no transform, it dispatches per tensor to the models there are -- the plain planes (planes_corpus.py), the predicted planes
(planes_pred_corpus.py), XOR and SUB against a base (planes_sub_corpus.py) -- with the ids of planes_estimate_corpus.py.  A tensor whose
transform byte is none of the four, or is XOR / SUB where there is no base, is refused: result GENERIC, its plane offsets those of its
size, none of its bytes written.  Plain Python, never the library.  Tensors are numpy uint8 arrays."""
import numpy as np

import planes_corpus as pc
import planes_pred_corpus as ppc
import planes_sub_corpus as psc
from planes_corpus import GENERIC
from planes_estimate_corpus import NAMES, PLAIN, PRED, SUB, XOR

IDS = (PLAIN, PRED, XOR, SUB)
assert IDS == (0, 1, 2, 3) and NAMES == ("plain", "pred", "xor", "sub")
PAIRS = [(a, b) for a in IDS for b in IDS]                 # the 16 ordered pairs of transforms


def accepted(tr, has_base):
    return tr in IDS and (tr < XOR or has_base)


def forward(t, b, E, tr):
    """the bytes whose plain planes the split writes for tensor t (base b) under transform tr"""
    t = np.ascontiguousarray(t, np.uint8)
    if tr == PLAIN:
        return t.copy()
    if tr == PRED:
        return ppc.forward(t, E)
    if tr == XOR:
        return t ^ np.asarray(b, np.uint8)
    assert tr == SUB
    return psc.forward(t, b, E)


def inverse(z, b, E, tr):
    """the tensor that forward() made z of"""
    z = np.ascontiguousarray(z, np.uint8)
    if tr == PLAIN:
        return z.copy()
    if tr == PRED:
        return ppc.inverse(z, E)
    if tr == XOR:
        return z ^ np.asarray(b, np.uint8)
    assert tr == SUB
    return psc.inverse(z, b, E)


def split_each_model(tensors, bases, E, transforms, capacity=None):
    """-> (planes buffer, written, plane offsets, tensor results) of FSEHIP_planes_split_each_dbatch; bases None: no base"""
    assert len(transforms) == len(tensors) and (bases is None or [len(b) for b in bases] == [len(t) for t in tensors])
    ok = [accepted(tr, bases is not None) for tr in transforms]
    z = [forward(t, None if bases is None else bases[i], E, transforms[i]) if ok[i] else np.asarray(t, np.uint8) for i, t in enumerate(tensors)]
    out, written, P, res = pc.split_model(z, E, capacity)
    S = [int(x) for x in pc.offsets(tensors)]
    for i in range(len(tensors)):
        if not ok[i]:
            if res[i] != GENERIC:                          # (behind the capacity its offsets have collapsed already)
                written[S[i]:S[i + 1]] = False
            res[i] = GENERIC
    return out, written, P, res


def merge_each_one(planes, base, E, tr):
    """the tensor whose planes under transform tr these are"""
    return inverse(pc.merge_one(planes, E), base, E, tr)


def cycle_all_pairs(n, lead=0):
    """n transform ids in which every ordered pair of the four occurs between neighbours: a walk over all 16 pairs (a de Bruijn sequence
    of order 2 over four letters, 0 0 1 0 2 0 3 1 1 2 1 3 2 2 3 3 and around), started `lead` entries in and repeated"""
    walk = [0, 0, 1, 0, 2, 0, 3, 1, 1, 2, 1, 3, 2, 2, 3, 3]
    assert sorted(set(zip(walk, walk[1:] + walk[:1]))) == sorted(PAIRS)
    return [walk[(lead + k) % 16] for k in range(n)]


def neighbour_pairs(transforms, lo=0, hi=None):
    """the ordered pairs (transforms[i], transforms[i + 1]) for lo <= i < i + 1 < hi"""
    hi = len(transforms) if hi is None else hi
    return set(zip(transforms[lo:hi - 1], transforms[lo + 1:hi]))

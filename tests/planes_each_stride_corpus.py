"""The numpy model of "strides in the estimate" and "a stride per tensor" (include/fsehip.h) shared by test_planes_each_stride_model.py and
test_gpu_planes_each_stride.py.  It defines no transform and no cost: it composes the per-tensor dispatch of planes_each_corpus.py, the
strided differences of planes_stride_corpus.py and the integer cost of planes_estimate_corpus.py -- a PRED tensor takes its stride, the
stride candidates of the estimate are the planes the strided split writes, the stride is chosen by the estimate's own hysteresis rule in
rising order.  Plain Python, never the library.  Tensors are numpy uint8 arrays."""
import numpy as np

import planes_corpus as pc
import planes_each_corpus as pe
import planes_estimate_corpus as pest
import planes_stride_corpus as psc
from planes_corpus import GENERIC
from planes_estimate_corpus import NO_CHOICE, ONES, PLAIN, PRED, SUB, XOR

MAX_STRIDE = psc.MAX_STRIDE
STRIDES = psc.STRIDES
NO_STRIDE = 0xFF                                    # d_strides of a refused tensor
PRED_BIT = 1 << PRED


def stride_ok(tr, st):
    return tr != PRED or 1 <= st <= MAX_STRIDE


def accepted(tr, st, has_base):
    return pe.accepted(tr, has_base) and stride_ok(tr, st)


def forward(t, b, E, tr, st=1):
    """the bytes whose plain planes the split writes for tensor t (base b) under transform tr, PRED at stride st"""
    return psc.forward(t, E, st) if tr == PRED else pe.forward(t, b, E, tr)


def inverse(z, b, E, tr, st=1):
    return psc.inverse(z, E, st) if tr == PRED else pe.inverse(z, b, E, tr)


def split_each_stride_model(tensors, bases, E, transforms, strides, capacity=None):
    """-> (planes buffer, written, plane offsets, tensor results) of FSEHIP_planes_split_each_stride_dbatch; strides None: stride 1 everywhere"""
    n = len(tensors)
    strides = [1] * n if strides is None else list(strides)
    assert len(transforms) == len(strides) == n
    ok = [accepted(tr, st, bases is not None) for tr, st in zip(transforms, strides)]
    z = [forward(t, None if bases is None else bases[i], E, transforms[i], strides[i]) if ok[i] else np.asarray(t, np.uint8) for i, t in enumerate(tensors)]
    out, written, P, res = pc.split_model(z, E, capacity)
    S = [int(x) for x in pc.offsets(tensors)]
    for i in range(n):
        if not ok[i]:
            if res[i] != GENERIC:                          # (behind the capacity its offsets have collapsed already)
                written[S[i]:S[i + 1]] = False
            res[i] = GENERIC
    return out, written, P, res


def merge_each_stride_one(planes, base, E, tr, st=1):
    return inverse(pc.merge_one(planes, E), base, E, tr, st)


# ---- the estimate over strides -------------------------------------------------------------------------------------------------------------
def stride_planes(t, E, S):
    """the planes that FSEHIP_planes_split_pred_stride_dbatch writes for tensor t at stride S"""
    buf, _, P, _ = psc.split_model([t], E, S)
    return [buf[P[p]:P[p + 1]] for p in range(E)]


def stride_mask(strides):
    m = 0
    for s in strides:
        assert 1 <= s <= MAX_STRIDE
        m |= 1 << (s - 1)
    return m


def choose_stride(est, smask, margin):
    """est: eight estimates, est[S - 1] (those outside smask are not looked at) -> the chosen stride"""
    best = None
    for s in STRIDES:
        if not (smask >> (s - 1)) & 1:
            continue
        if best is None or est[s - 1] * 1000 < est[best - 1] * (1000 - margin):
            best = s
    return best


def estimate_stride_model(tensors, E, mask, smask, bases=None, margin=50, capacity=None, offsets=None):
    """-> (plane_bits [n * 4 * E], est_bytes [n * 4], choice [n], results [n], stride_est [n * 8], strides [n]) of
    FSEHIP_planes_estimate_stride_dbatch, the 64-bit outputs as Python ints (ONES where the call writes all-ones)"""
    S = [int(x) for x in (pc.offsets(tensors) if offsets is None else offsets)]
    cap = max(S) if capacity is None else int(capacity)
    assert 0 < mask < 16 and 0 < smask < 256 and 0 <= margin <= 1000 and (smask == 1 or mask & PRED_BIT)
    bits, est, choice, res, sest, strides = [], [], [], [], [], []
    for i, t in enumerate(tensors):
        if S[i] > S[i + 1] or S[i + 1] > cap:
            bits += [ONES] * (4 * E); est += [ONES] * 4; choice.append(NO_CHOICE); res.append(GENERIC); sest += [ONES] * MAX_STRIDE; strides.append(NO_STRIDE)
            continue
        assert len(t) == S[i + 1] - S[i] < 1 << 32
        mine_s, planes_s = [ONES] * MAX_STRIDE, {}
        if mask & PRED_BIT:
            for s in STRIDES:
                if (smask >> (s - 1)) & 1:
                    planes_s[s] = stride_planes(t, E, s)
                    mine_s[s - 1] = pest.est_bytes(planes_s[s])
        best = choose_stride(mine_s, smask, margin) if mask & PRED_BIT else 1
        mine = []
        for c in range(4):
            if not (mask >> c) & 1:
                bits += [ONES] * E; mine.append(ONES)
                continue
            planes = planes_s[best] if c == PRED else pest.candidate_planes(t, None if bases is None else bases[i], E, c)
            bits += [pest.plane_bits(p) for p in planes]
            mine.append(pest.est_bytes(planes))
        est += mine
        choice.append(pest.choose(mine, mask, margin))
        res.append(len(t))
        sest += mine_s
        strides.append(best)
    return bits, est, choice, res, sest, strides


def settled(choice, strides):
    """what the CHOOSE composites leave in d_strides: 1 where an accepted tensor did not choose PRED"""
    return [st if ch == PRED or ch == NO_CHOICE else 1 for ch, st in zip(choice, strides)]


# ---- the corpora of the choice table: name -> (E, bytes, stride, transform) ------------------------------------------------------------------
def table(n=None):
    """the corpora of the table in fsehip.h's neighbourhood with the stride and the transform the rule must choose.  n: cut to the
    first n elements (a multiple of every channel count keeps the phase)"""
    def cut(a, E):
        return a if n is None else a[:n * E]
    rows = {"stereo": (2, psc.stereo(), 2, PRED), "rgb": (1, psc.rgb(), 3, PRED), "xyz": (4, psc.xyz(), 3, PRED), "boxes": (4, psc.boxes(), 4, PRED),
            "phasor": (4, psc.phasor(), 2, PRED), "bf16_gaussian": (2, pest.bf16_gaussian(), 1, PLAIN), "sorted_int64": (8, pest.sorted_int64(), 1, PRED),
            "sorted_int64 as E=4": (4, pest.sorted_int64(), 2, PRED), "position_ids": (4, pest.position_ids(), 1, PRED)}
    return {k: (E, cut(np.ascontiguousarray(a, np.uint8), E), s, tr) for k, (E, a, s, tr) in rows.items()}


def cycle_transforms_and_strides(n, lead=0):
    """n (transform, stride) pairs in which every ordered pair of the eleven kinds -- PLAIN, XOR, SUB and PRED at strides 1 .. 8 -- occurs
    between neighbours: kind k of 11 follows kind j for every (j, k), a walk of 121 steps over the complete digraph, repeated"""
    kinds = [(PLAIN, 1), (XOR, 1), (SUB, 1)] + [(PRED, s) for s in STRIDES]
    K = len(kinds)
    walk = []                                                  # an Euler circuit of the complete digraph with loops on K nodes (Hierholzer)
    nxt = [0] * K
    stack = [0]
    while stack:
        v = stack[-1]
        if nxt[v] < K:
            stack.append(nxt[v]); nxt[v] += 1
        else:
            walk.append(stack.pop())
    walk = walk[::-1][:-1]
    assert len(walk) == K * K and len(set(zip(walk, walk[1:] + walk[:1]))) == K * K
    seq = [kinds[walk[(lead + k) % len(walk)]] for k in range(n)]
    return [tr for tr, _ in seq], [st for _, st in seq]

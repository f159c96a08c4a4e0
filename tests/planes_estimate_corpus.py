"""The numpy model of the plane estimates (include/fsehip.h, "plane estimates") shared by test_planes_estimate_model.py and
test_gpu_planes_estimate.py, built on the split models of planes_corpus.py, planes_pred_corpus.py, planes_delta_corpus.py and
planes_sub_corpus.py: the planes of a candidate are the ones its split writes, their histograms are np.bincount, and the cost is the
header's integer arithmetic.  Pure integers and numpy, never the library.  Tensors and bases are numpy uint8 arrays."""
import math

import numpy as np

import planes_corpus as pc
import planes_delta_corpus as pdc
import planes_pred_corpus as ppc
import planes_sub_corpus as psc

PLAIN, PRED, XOR, SUB = 0, 1, 2, 3                  # FSEHIP_EST_*
NAMES = ("plain", "pred", "xor", "sub")
ONES = (1 << 64) - 1                                # what a slot that holds no estimate holds
GENERIC, SRCSIZE_WRONG = -1, -3
NO_CHOICE = 0xFF

T = [int(math.floor(256 * math.log2(1 + f / 256) + 0.5)) for f in range(256)]


def L(x):
    """256 floor(log2 x) + T[the eight bits below the leading one], x >= 1"""
    x = int(x)
    assert x >= 1
    e = x.bit_length() - 1
    f = (((x << (63 - e)) & ONES) >> 55) & 0xFF
    return 256 * e + T[f]


def bits256(counts):
    """the order-0 cost of a plane with these counts, in 1/256 bits"""
    counts = [int(c) for c in counts]
    n = sum(counts)
    return sum(c * (L(n) - L(c)) for c in counts if c > 0)


def plane_bits(plane):
    return bits256(np.bincount(np.asarray(plane, np.uint8), minlength=256))


def est_bytes(planes):
    """the estimate of a tensor under one candidate from its planes: per plane min(N, ceil(bits256 / 2048))"""
    return sum(min(len(p), (plane_bits(p) + 2047) >> 11) for p in planes)


def choose(est, mask, margin):
    """est: four estimates (those of candidates outside the mask are not looked at) -> the chosen id"""
    best = None
    for c in range(4):
        if not (mask >> c) & 1:
            continue
        if best is None or est[c] * 1000 < est[best] * (1000 - margin):
            best = c
    return best


def candidate_planes(t, b, E, c):
    """the planes that candidate c's split writes for tensor t (base b)"""
    if c == PLAIN:
        buf, _, P, _ = pc.split_model([t], E)
    elif c == PRED:
        buf, _, P, _ = ppc.split_pred_model([t], E)
    elif c == XOR:
        buf, _, P, _ = pdc.split_xor_model([t], [b], E)
    else:
        buf, _, P, _ = psc.split_sub_model([t], [b], E)
    return [buf[P[p]:P[p + 1]] for p in range(E)]


def estimate_model(tensors, E, mask, bases=None, margin=50, capacity=None, offsets=None):
    """-> (plane_bits [n * 4 * E], est_bytes [n * 4], choice [n], results [n]) of FSEHIP_planes_estimate_dbatch, the 64-bit outputs as
    Python ints (ONES where the call writes all-ones).  offsets: the source offsets where they are not those of `tensors` laid back to back
    (a slot that decreases: its tensor is then whatever `tensors` holds for it, and is refused)"""
    S = [int(x) for x in (pc.offsets(tensors) if offsets is None else offsets)]
    cap = max(S) if capacity is None else int(capacity)
    assert 0 < mask < 16 and 0 <= margin <= 1000
    bits, est, choice, res = [], [], [], []
    for i, t in enumerate(tensors):
        if S[i] > S[i + 1] or S[i + 1] > cap:
            bits += [ONES] * (4 * E); est += [ONES] * 4; choice.append(NO_CHOICE); res.append(GENERIC)
            continue
        assert len(t) == S[i + 1] - S[i] < 1 << 32
        mine = []
        for c in range(4):
            if not (mask >> c) & 1:
                bits += [ONES] * E; mine.append(ONES)
                continue
            planes = candidate_planes(t, None if bases is None else bases[i], E, c)
            assert [len(p) for p in planes] == [pc.plane_size(len(t), p, E) for p in range(E)]
            bits += [plane_bits(p) for p in planes]
            mine.append(est_bytes(planes))
        est += mine
        choice.append(choose(mine, mask, margin))
        res.append(len(t))
    return bits, est, choice, res


# ---- the corpora of the header's table (seeds fixed here)
def bf16_gaussian():
    """bf16 gaussian, 256 KiB"""
    return pc.bf16_gaussian(1 << 17)


def sorted_int64():
    """sorted int64 below 2^40, 256 KiB"""
    return np.sort(np.random.default_rng(15).integers(0, 1 << 40, 1 << 15).astype(np.uint64)).astype("<u8").view(np.uint8)


def position_ids():
    """position ids arange % 4096 as u32, 128 KiB"""
    return (np.arange(1 << 15, dtype=np.uint64) % 4096).astype("<u4").view(np.uint8)


def update_pair():
    """(tensor, base) = bf16_update_pair(1 << 17) in its order, 256 KiB each: the table's row takes the first of the pair as the tensor"""
    return pdc.bf16_update_pair(1 << 17)


def float_entropy_bits(plane):
    c = np.bincount(np.asarray(plane, np.uint8), minlength=256).astype(np.float64)
    c = c[c > 0]
    return float((c * (np.log2(c.sum()) - np.log2(c))).sum())

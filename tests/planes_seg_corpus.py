"""The numpy model of segmented planes (include/fsehip.h, "segmented planes") shared by test_planes_seg_model.py and test_gpu_planes_seg.py: how
many segments a plane has, where every segment lies in the planes buffer, which tensors a segFirst array refuses, and what the fold says of a
plane from its segments' offsets and results -- as plain Python, never the library.  Sizes and offsets are python ints, error results negative
ints (-c for error code c), as the binding shows them."""
import numpy as np

import planes_corpus as pc
from planes_corpus import CORRUPT, GENERIC

ELEMS = pc.ELEMS


def seg_count(size, seg_log):
    """segments of a plane of `size` bytes, by enumeration: the starts 0, seg, 2 seg, .. below size; an empty plane has one (empty) segment"""
    return max(1, len(range(0, int(size), 1 << seg_log)))


def plane_sizes(sizes, E):
    return [pc.plane_size(int(n), p, E) for n in sizes for p in range(E)]


def seg_first(sizes, E, seg_log):
    """segFirst of tensors of these byte sizes: the running sum of the planes' segment counts, one entry more than planes"""
    out = [0]
    for s in plane_sizes(sizes, E):
        out.append(out[-1] + seg_count(s, seg_log))
    return out


def split_offsets(sizes, E, capacity=None):
    """-> (plane offsets, tensor results) as FSEHIP_planes_split_dbatch leaves them for tensors of these sizes laid back to back from 0"""
    n = len(sizes)
    S = [0]
    for s in sizes:
        S.append(S[-1] + int(s))
    cap = S[-1] if capacity is None else int(capacity)
    bad_at = next((i for i in range(n) if S[i + 1] > cap), n)
    P, res = [], []
    for i in range(n):
        if i >= bad_at:
            P += [S[bad_at]] * E
            res.append(GENERIC)
            continue
        at = S[i]
        for p in range(E):
            P.append(at)
            at += pc.plane_size(int(sizes[i]), p, E)
        res.append(int(sizes[i]))
    P.append(S[bad_at])
    return P, res


def segments_model(sizes, E, seg_log, first=None, capacity=None):
    """-> (segment offsets, tensor results) of the split followed by FSEHIP_planes_segments_dbatch for tensors of these sizes laid back to back
    from 0.  `first`: the segFirst handed in (default: the right one); a tensor whose counts in it are not its own is refused: GENERIC, all
    its entries its start.  `capacity`: the split's -- tensors that end behind it are refused by the split and collapse onto the first one's start"""
    n = len(sizes)
    right = seg_first(sizes, E, seg_log)
    first = right if first is None else [int(x) for x in first]
    assert len(first) == n * E + 1
    P, res = split_offsets(sizes, E, capacity)
    seg = 1 << seg_log
    out = []
    for i in range(n):
        ok = all(first[j + 1] - first[j] == right[j + 1] - right[j] for j in range(i * E, (i + 1) * E))
        if not ok:
            res[i] = GENERIC
        for j in range(i * E, (i + 1) * E):
            for k in range(first[j + 1] - first[j]):
                out.append(min(P[j] + k * seg, P[j + 1]) if ok else P[i * E])
    out.append(P[n * E])
    assert len(out) == first[-1] + 1
    return out, res


def fold_verdict(off, res, seg_log, variant=None):
    """the fold's result for ONE plane from its segments' results `res` and their offsets `off` (one more than segments: the entry behind the last
    belongs to the next plane and is not looked at).  The order of include/fsehip.h.  `variant` names a deliberately broken model (the tests
    must tell each from the right one): "size_before_error" checks the sizes in front of the errors, "no_contiguity" drops the back-to-back
    check, "last_error" takes the last error instead of the first, "no_generic" sums an empty plane to 0, "last_may_be_empty" lets the last of
    several segments hold nothing"""
    seg, cnt = 1 << seg_log, len(res)
    if cnt == 0:
        return 0 if variant == "no_generic" else GENERIC

    def sizes_ok():
        for k, r in enumerate(res):
            if r < 0:
                continue
            if k < cnt - 1:
                if r != seg:
                    return False
            elif r > seg or (r == 0 and cnt != 1 and variant != "last_may_be_empty"):
                return False
        return True

    errors = [r for r in res if r < 0]
    if variant == "size_before_error" and not sizes_ok():
        return CORRUPT
    if errors:
        return errors[-1] if variant == "last_error" else errors[0]
    if not sizes_ok():
        return CORRUPT
    if variant != "no_contiguity" and any(off[k + 1] != off[k] + res[k] for k in range(cnt - 1)):
        return CORRUPT
    return sum(res)


VARIANTS = ("size_before_error", "no_contiguity", "last_error", "no_generic", "last_may_be_empty")


def fold_model(off, res, first, seg_log, variant=None):
    """-> (plane offsets, plane sizes) of FSEHIP_planes_fold_segments_dbatch over all planes"""
    po, ps = [], []
    for j in range(len(first) - 1):
        a, b = first[j], first[j + 1]
        po.append(off[a])
        ps.append(fold_verdict(off[a:b + 1], res[a:b], seg_log, variant))
    return po, ps


def fold_cases(seg_log):
    """[(name, offsets, results, expected)]: one case per branch of the verdict's ordering, and the pairs of branches whose order matters"""
    s = 1 << seg_log
    return [
        ("no segment", [40], [], GENERIC),
        ("one empty segment", [40, 40], [0], 0),
        ("one short segment", [40, 47], [7], 7),
        ("one full segment", [40, 40 + s], [s], s),
        ("three segments", [0, s, 2 * s, 2 * s + 5], [s, s, 5], 2 * s + 5),
        ("three full segments", [8, 8 + s, 8 + 2 * s, 8 + 3 * s], [s, s, s], 3 * s),
        ("first error wins", [0, s, 2 * s, 3 * s], [s, -3, -2], -3),
        ("an error in front of a short middle segment", [0, s, 2 * s, 3 * s], [s - 1, -2, 1], -2),
        ("a short middle segment", [0, s - 1, 2 * s - 1, 2 * s], [s - 1, s, 1], CORRUPT),
        ("a long last segment", [0, s, 2 * s + 1], [s, s + 1], CORRUPT),
        ("an empty last segment of two", [0, s, s], [s, 0], CORRUPT),
        ("a gap between full segments", [0, s + 16, 2 * s + 16], [s, 3], CORRUPT),
        ("segments that overlap", [0, s - 1, s + 4], [s, 5], CORRUPT),
    ]


def seg_sizes(E, seg_log):
    """tensor sizes in bytes that put plane sizes 0, 1, seg - 1, seg, seg + 1, 2 seg and 2 seg + 1 next to each other, sizes that are no multiple of E
    (the planes of one tensor then differ in their counts), and an empty tensor among the others"""
    s = 1 << seg_log
    return [E * s, 0, E * (s - 1), 1, E * (s + 1), E * s + 1, E * 2 * s, E * 2 * s + 1, E, 2 * E * s + E - 1, E * s - 1, 3]

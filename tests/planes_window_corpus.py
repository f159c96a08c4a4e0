"""The numpy model of windows of segmented tensors (include/fsehip.h, "windows of segmented tensors") shared by test_planes_window_model.py and
test_gpu_planes_window.py: which segment frames of a plane a window of elements selects, how many blocks they hold, which tensors the
selection refuses, where every selected frame's extent starts in the frames buffer, and what the fold says of a plane from its selected
segments' offsets and results -- as plain Python, never the library.  Sizes, offsets and windows are python ints, error results negative ints
(-c for error code c), as the binding shows them."""
import bisect

import planes_corpus as pc
import planes_seg_corpus as psc
from planes_corpus import CORRUPT, GENERIC

ELEMS = pc.ELEMS


def window_valid(n, a, b, E):
    """a window of elements [a, b) of a tensor of n bytes: whole elements only"""
    return 0 <= a <= b <= n // E


def selected(size, a, b, seg_log):
    """the segments of a plane of `size` bytes that hold a byte of [a, b), by enumeration over the plane's segments"""
    seg = 1 << seg_log
    return [k for k, at in enumerate(range(0, int(size), seg)) if any(True for e in range(max(a, at), min(b, at + seg, size)))]


def window_first(sizes, windows, E, seg_log, bsid=0):
    """-> (selFirst, blocks) of tensors of these byte sizes and windows: the running sum of the selected segments per plane, one entry more than
    planes, and the blocks those segments are coded in; None where a window is not valid"""
    seg, bs = 1 << seg_log, 1024 << bsid
    out, blocks = [0], 0
    for n, (a, b) in zip(sizes, windows):
        if not window_valid(int(n), a, b, E):
            return None
        for p in range(E):
            size = pc.plane_size(int(n), p, E)
            ks = selected(size, a, b, seg_log)
            out.append(out[-1] + len(ks))
            blocks += sum(len(range(0, min(seg, size - k * seg), bs)) for k in ks)
    return out, blocks


def accepted(sizes, windows, E, seg_log, seg_first, sel_first, nsel):
    """per tensor: a valid window, the window's count for each of its planes in sel_first, ending at or below nsel, and the counts its size implies
    in seg_first"""
    right = psc.seg_first(sizes, E, seg_log)
    out = []
    for i, (n, (a, b)) in enumerate(zip(sizes, windows)):
        ok = window_valid(int(n), a, b, E)
        if ok:
            cnt = len(selected(pc.plane_size(int(n), 0, E), a, b, seg_log))
            ok = all(sel_first[j + 1] - sel_first[j] == cnt for j in range(i * E, (i + 1) * E)) and sel_first[i * E] <= sel_first[(i + 1) * E] <= nsel
        ok = ok and all(seg_first[j + 1] - seg_first[j] == right[j + 1] - right[j] for j in range(i * E, (i + 1) * E))
        out.append(ok)
    return out


def select_model(F, sizes, windows, E, seg_log, seg_first=None, sel_first=None, nsel=None):
    """-> the nsel + 1 entries of FSEHIP_planes_select_window_dbatch.  F: all frames' offsets (nSegments + 1).  seg_first / sel_first: what is
    handed in (default: the right ones; they must be non-decreasing).  Entry r belongs to the last plane j with sel_first[j] <= r, the last
    entry to the plane of entry nsel - 1 and is the END of that frame; a refused tensor's entries are all F[seg_first[(i + 1) * E]]."""
    nseg = len(F) - 1
    seg_first = psc.seg_first(sizes, E, seg_log) if seg_first is None else [int(x) for x in seg_first]
    sel_first = window_first(sizes, windows, E, seg_log)[0] if sel_first is None else [int(x) for x in sel_first]
    nsel = sel_first[-1] if nsel is None else nsel
    nP = len(sizes) * E
    if nsel == 0 or nP == 0:
        return [F[0]] * (nsel + 1)
    assert sel_first == sorted(sel_first), "the plane of an entry is only defined for a non-decreasing selFirst"
    ok = accepted(sizes, windows, E, seg_log, seg_first, sel_first, nsel)
    of_plane = {}
    out = []
    for r in range(nsel + 1):
        at = min(r, nsel - 1)
        j = max(bisect.bisect_right(sel_first, at, 0, nP) - 1, 0)           # the last plane j < nP with sel_first[j] <= at
        i = j // E
        if not ok[i]:
            q = seg_first[(i + 1) * E]
        else:
            a, b = windows[i]
            if j not in of_plane:
                of_plane[j] = selected(pc.plane_size(int(sizes[i]), j % E, E), a, b, seg_log)
            ks = of_plane[j]
            k = min(max(at - sel_first[j], 0), max(len(ks) - 1, 0))
            q = seg_first[j] + (ks[k] if ks else a >> seg_log) + (1 if r == nsel else 0)
        out.append(F[min(q, nseg)])
    return out


VARIANTS = ("size_before_error", "no_contiguity", "last_error", "loose_last", "empty_before_refused", "offset_of_the_segment")


def fold_plane(off, res, a, b, size, seg_log, refused=False, variant=None):
    """-> (plane offset, plane size) of ONE plane of `size` bytes from the results `res` and offsets `off` (one more than results: the entry behind
    the last is the next plane's and is not looked at) of its selected segments, in the order of include/fsehip.h.  `variant` names a
    deliberately broken model (the tests must tell each from the right one): "size_before_error" checks the sizes in front of the errors,
    "no_contiguity" drops the back-to-back check, "last_error" takes the last error instead of the first, "loose_last" takes 1 .. seg bytes from
    the last selected segment as the fold of the full read does, "empty_before_refused" answers 0 for an empty window of a refused tensor,
    "offset_of_the_segment" forgets to move the offset from the first selected segment's start to the window's first byte"""
    seg = 1 << seg_log
    if variant == "empty_before_refused" and a == b:
        return 0, 0
    if refused:
        return 0, GENERIC
    if a == b:
        return 0, 0
    ks = selected(size, a, b, seg_log)
    assert len(res) == len(ks) and len(off) >= len(ks)

    def sizes_ok():
        for t, (k, r) in enumerate(zip(ks, res)):
            if r < 0:
                continue
            want = min(seg, size - k * seg)
            if variant == "loose_last" and t == len(ks) - 1:
                if not 1 <= r <= seg:
                    return False
            elif r != want:
                return False
        return True

    errors = [r for r in res if r < 0]
    if variant == "size_before_error" and not sizes_ok():
        return 0, CORRUPT
    if errors:
        return 0, errors[-1] if variant == "last_error" else errors[0]
    if not sizes_ok():
        return 0, CORRUPT
    if variant != "no_contiguity" and any(off[t + 1] != off[t] + res[t] for t in range(len(ks) - 1)):
        return 0, CORRUPT
    return off[0] + (0 if variant == "offset_of_the_segment" else a - ks[0] * seg), b - a


def fold_model(off, res, sizes, windows, E, seg_log, seg_first=None, sel_first=None, nsel=None, variant=None):
    """-> (plane offsets, plane sizes) of FSEHIP_planes_fold_window_dbatch over all planes"""
    seg_first = psc.seg_first(sizes, E, seg_log) if seg_first is None else [int(x) for x in seg_first]
    sel_first = window_first(sizes, windows, E, seg_log)[0] if sel_first is None else [int(x) for x in sel_first]
    nsel = sel_first[-1] if nsel is None else nsel
    ok = accepted(sizes, windows, E, seg_log, seg_first, sel_first, nsel)
    po, ps = [], []
    for j in range(len(sizes) * E):
        i = j // E
        a, b = windows[i]
        if not ok[i]:
            o, s = fold_plane([], [], a, b, 0, seg_log, True, variant)
        else:
            q0, q1 = sel_first[j], sel_first[j + 1]
            o, s = fold_plane(off[q0:q1 + 1], res[q0:q1], a, b, pc.plane_size(int(sizes[i]), j % E, E), seg_log, False, variant)
        po.append(o)
        ps.append(s)
    return po, ps


def fold_cases(seg_log):
    """[(name, size, a, b, refused, offsets, results, (expected offset, expected size))]: one case per branch of the verdict's ordering, and the pairs
    of branches whose order matters.  The plane has 3 seg + 5 bytes: segments of seg, seg, seg and 5 bytes."""
    s = 1 << seg_log
    size = 3 * s + 5
    return [
        ("a refused tensor", size, 3, 9, True, [40], [], (0, GENERIC)),
        ("a refused tensor with an empty window", size, 7, 7, True, [40], [], (0, GENERIC)),
        ("an empty window", size, 7, 7, False, [40], [], (0, 0)),
        ("inside the first segment", size, 3, 9, False, [40, 40 + s], [s], (43, 6)),
        ("inside a middle segment", size, s + 3, 2 * s, False, [40, 40 + s], [s], (43, s - 3)),
        ("across a boundary", size, s - 1, s + 1, False, [8, 8 + s, 8 + 2 * s], [s, s], (8 + s - 1, 2)),
        ("from a boundary to the end", size, 2 * s, size, False, [0, s, s + 5], [s, 5], (0, s + 5)),
        ("the last, short segment alone", size, 3 * s + 1, size, False, [16, 21], [5], (17, 4)),
        ("everything", size, 0, size, False, [0, s, 2 * s, 3 * s, 3 * s + 5], [s, s, s, 5], (0, size)),
        ("first error wins", size, 0, size, False, [0, s, 2 * s, 3 * s, 3 * s], [s, -3, -2, 5], (0, -3)),
        ("an error in front of a short segment", size, 0, 3 * s, False, [0, s - 1, 2 * s - 1, 2 * s - 1], [s - 1, s, -2], (0, -2)),
        ("a short middle segment", size, 0, 3 * s, False, [0, s, 2 * s - 1, 3 * s - 1], [s, s - 1, s], (0, CORRUPT)),
        ("a last segment that is not the plane's rest", size, 3 * s, size, False, [0, 4], [4], (0, CORRUPT)),
        ("a last segment longer than the plane's rest", size, s, size, False, [0, s, 2 * s, 2 * s + 6], [s, s, 6], (0, CORRUPT)),
        ("an empty segment", size, 1, 2, False, [0, 0], [0], (0, CORRUPT)),
        ("a gap between segments", size, 1, 2 * s, False, [0, s + 16, 2 * s + 16], [s, s], (0, CORRUPT)),
        ("segments that overlap", size, 1, 2 * s, False, [0, s - 1, 2 * s - 1], [s, s], (0, CORRUPT)),
    ]


def points(numel, seg_log):
    """the window ends that matter for a tensor of `numel` elements: 0, 1, k seg - 1, k seg, k seg + 1 for the first segments, the last
    boundary and the end"""
    s = 1 << seg_log
    cand = {0, 1, numel - 1, numel, (numel >> seg_log << seg_log) - 1, numel >> seg_log << seg_log}
    for k in (1, 2):
        cand |= {k * s - 1, k * s, k * s + 1}
    return sorted(x for x in cand if 0 <= x <= numel)


def boundary_windows(numel, seg_log):
    """every window (a, b), a <= b, between those points: empty ones, the whole tensor, windows inside one segment, windows that end on, one short
    of and one behind a segment boundary"""
    pts = points(numel, seg_log)
    return [(a, b) for a in pts for b in pts if a <= b]


def window_sizes(E, seg_log):
    """tensor sizes in bytes: 0, fewer than E, sizes that are no multiple of E (the planes of one tensor then differ in size and segment count), one
    segment exactly, a byte more, two segments and a bit, several segments"""
    s = 1 << seg_log
    return [E * s, 0, E - 1 if E > 1 else 0, E * (s - 1), 1, E * (s + 1), E * s + 1, E * 2 * s, E * 2 * s + 1, E, 2 * E * s + E - 1, E * s - 1, E * (3 * s + 5) + E // 2]

"""The numpy model of "windows of tensors with a transform per tensor" (include/fsehip.h) shared by test_planes_window_each_model.py and
test_gpu_planes_window_each.py: what FSEHIP_planes_merge_window_each_dbatch makes of the window [a, b) of a tensor's planes, built from the
inverses there are (planes_each_corpus.py, planes_pred_corpus.py) -- PLAIN, XOR and SUB slice the planes and invert; PRED inverts from the
start of the run that holds a, a - a % RUN, and slices -- and the corpus of the merge test with the shapes it has to contain.  Plain Python,
never the library.  Tensors are numpy uint8 arrays, windows are in elements."""
import numpy as np

import planes_corpus as pc
import planes_each_corpus as pe
import planes_pred_corpus as ppc
from planes_corpus import TILE
from planes_each_corpus import IDS, PLAIN, PRED, SUB, XOR

RUN = ppc.RUN
ENDS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048)       # and m - 1, m: what a and b are drawn from
FILL = 0xA5
MED = 2051                                                     # elements of the tensors that take every window: 12 ends, 78 windows


def ends(m):
    return sorted({x for x in ENDS + (m - 1, m) if 0 <= x <= m})


def window_set(m):
    """every window (a, b), a <= b, between the ends of a tensor of m elements"""
    pts = ends(m)
    return [(a, b) for a in pts for b in pts if a <= b]


def lead(tr, a, b):
    """the elements in front of the window that the merge reads and does not store"""
    return a % RUN if tr == PRED and a < b else 0


def whole_planes(t, base, E, tr):
    """the E planes of the whole tensor under transform tr, as the split writes them"""
    return pc.planes_of(pe.forward(t, base, E, tr), E)


def window_merge_model(planes, base_window, E, tr, a, b):
    """elements [a, b) of the tensor whose WHOLE planes under transform tr these are; base_window: bytes [a E, b E) of the base"""
    if tr == PRED:
        a0 = a - lead(tr, a, b)
        z = pc.merge_one([np.asarray(p[a0:b]) for p in planes], E)
        return ppc.inverse(z, E)[(a - a0) * E:]
    z = pc.merge_one([np.asarray(p[a:b]) for p in planes], E)
    return pe.inverse(z, base_window, E, tr)


def merge_verdict(tr, has_base, a, b, E, plane_sizes, plane_offsets, slot):
    """the result of one tensor of the merge-only call: the merge's rules (sizes that belong together, a slot that holds them), then the
    refusals of the window form"""
    if not pe.accepted(tr, has_base):
        return pc.GENERIC
    n = sum(plane_sizes)
    if list(plane_sizes) != [pc.plane_size(n, p, E) for p in range(E)]:
        return pc.CORRUPT
    if n > slot:
        return pc.TOO_SMALL
    if a > b or n % E or b - a != n // E:
        return pc.GENERIC
    if any(lead(tr, a, b) > po for po in plane_offsets):
        return pc.GENERIC
    return n


# ---------------------------------------------------------------------------------------------------------------- the corpus of the merge test
WALK = pe.cycle_all_pairs(16)


def _occurrence(k):
    """which of the four occurrences of its transform position k of the walk is"""
    return WALK[:k % 16].count(WALK[k % 16])


def merge_corpus(E, seed=0):
    """-> dict(tensors, bases, transforms, windows, D, tiny=(lo, hi)): tensors with a window each and the destination slots D (len + 1
    offsets; slot i holds its window and a gap of guard bytes behind it, the first slot lies 7 bytes in).
      two tensors of several tiles, sixty tiny ones (1 .. 40 elements) whose slots lie inside one tile, two more of several tiles, then 320
      tensors of MED elements: the transforms walk through all 16 ordered neighbour pairs, and among the 320 every
      transform meets every window of window_set(m) -- block k // 16 of the walk holds each transform four times, its occurrences take the
      windows 4 (k // 16) .. + 3."""
    rng = np.random.default_rng(100 * E + seed)
    big = 2 * TILE // E + 4096 + 7
    counts, windows = [], []
    for m, w in ((big, (1, big)), (big + 3, (1023, big + 2))):
        counts.append(m); windows.append(w)
    tiny_lo = len(counts)
    for k in range(60):
        m = 1 + (7 * k) % 40
        pts = ends(m)
        counts.append(m); windows.append((pts[k % len(pts)], m) if k % 3 else (pts[(k // 3) % len(pts)], pts[-1 - (k // 3) % 2]))
    windows = [(a, b) if a <= b else (b, a) for a, b in windows]
    tiny_hi = len(counts)
    for m, w in ((big + 1, (1025, big + 1)), (big + 2, (2047, big + 2))):
        counts.append(m); windows.append(w)
    for k in range(320):
        ws = window_set(MED)
        counts.append(MED); windows.append(ws[(4 * (k // 16) + _occurrence(k)) % len(ws)])
    n = len(counts)
    # the walk, turned so that the two tensors in front of the tiny ones are PRED and the four large ones take all four transforms
    transforms = pe.cycle_all_pairs(n, 8)                       # 1 1 2 1 3 2 2 3 3 0 0 1 0 2 0 3 ...
    for i, tr in zip((0, 1, tiny_hi, tiny_hi + 1), (PRED, SUB, XOR, PLAIN)):
        transforms[i] = tr
    first_med = tiny_hi + 2
    for k in range(320):
        transforms[first_med + k] = WALK[k % 16]
    sizes = [m * E + (i % E if i % 5 == 0 else 0) for i, m in enumerate(counts)]          # some with n mod E trailing bytes: never inside a window
    tensors = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    for i in range(0, n, 3):                                    # smooth ones, whose differences are small: sums that carry rarely
        x = (np.cumsum(rng.integers(-3, 4, counts[i])) + 1000).astype("<u8")
        tensors[i][:counts[i] * E] = np.ascontiguousarray(x.view(np.uint8).reshape(-1, 8)[:, :E]).reshape(-1)
    bases = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    D, at = [], 7
    for i, (a, b) in enumerate(windows):
        if i == tiny_lo:
            at = -(-at // TILE) * TILE + 5                      # the tiny slots start a tile
        D.append(at)
        at += E * (b - a) + 1 + (3 * i) % 17
    D.append(at)
    return dict(tensors=tensors, bases=bases, transforms=transforms, windows=windows, D=D, tiny=(tiny_lo, tiny_hi), first_med=first_med, counts=counts)


def shapes(c, E):
    """what the corpus holds, by name: the merge test needs every one of these to be True"""
    tr, w, D, m = c["transforms"], c["windows"], c["D"], c["counts"]
    lo, hi = c["tiny"]
    n = len(tr)
    med = range(c["first_med"], n)
    pred = [i for i in range(n) if tr[i] == PRED]
    return {
        "all 16 ordered neighbour pairs": pe.neighbour_pairs(tr) == set(pe.PAIRS),
        "every transform meets every window": {(tr[i], w[i]) for i in med} == {(t, x) for t in IDS for x in window_set(MED)},
        "a PRED window inside one run, off its start": any(0 < w[i][0] % RUN and w[i][0] // RUN == (w[i][1] - 1) // RUN and w[i][0] < w[i][1] for i in pred),
        "a PRED window across a run boundary, off a run start": any(0 < w[i][0] % RUN and w[i][0] // RUN < (w[i][1] - 1) // RUN for i in pred),
        "a PRED window with the largest lead": any(w[i][0] % RUN == RUN - 1 and w[i][0] < w[i][1] for i in pred),
        "a PRED lane that straddles the lead": any(0 < w[i][0] % 16 and w[i][1] - w[i][0] >= 16 for i in pred),
        "a window that ends at the last element": all(any(tr[i] == t and w[i][1] == m[i] and w[i][0] < w[i][1] for i in range(n)) for t in IDS),
        "an empty window off a run start": any(w[i][0] == w[i][1] and w[i][0] % RUN for i in pred),
        "a PRED tensor of fewer than 16 elements": any(m[i] < 16 and w[i][0] < w[i][1] for i in pred),
        "sixty tiny tensors inside one tile": hi - lo == 60 and D[lo] // TILE == (D[hi] - 1) // TILE and max(m[lo:hi]) <= 40,
        "all four transforms among the tiny ones": {tr[i] for i in range(lo, hi)} == set(IDS),
        "tensors of several tiles": all(any(tr[i] == t and E * (w[i][1] - w[i][0]) > 2 * TILE for i in range(n)) for t in IDS),
        "slots off every alignment": {D[i] % 16 for i in range(n) if w[i][1] - w[i][0] > 16} == set(range(16)),
        "guard bytes around every slot": D[0] > 0 and all(D[i + 1] - D[i] > E * (w[i][1] - w[i][0]) for i in range(n)),
    }

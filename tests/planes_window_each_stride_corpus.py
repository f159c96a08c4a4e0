"""The numpy model of "windows and patches of tensors with a stride per tensor" (include/fsehip.h) shared by
test_planes_window_each_stride_model.py, test_planes_patch_each_stride_model.py and the two GPU tests of the same names: what
FSEHIP_planes_merge_window_each_stride_dbatch makes of the window [a, b) of a tensor's planes -- PLAIN, XOR and SUB as
planes_window_each_corpus.py has them; PRED at stride S inverts from the start of the run that holds a (planes_stride_corpus.inverse) and
slices --, what FSEHIP_planes_split_window_each_stride_dbatch stages, the verdict rules with the stride's refusal, and the corpus of the merge
test with the shapes it has to contain.  Plain Python, never the library.  Tensors are numpy uint8 arrays, windows are in elements."""
import numpy as np

import planes_corpus as pc
import planes_each_corpus as pe
import planes_each_stride_corpus as pes
import planes_patch_corpus as ppc
import planes_stride_corpus as psc
import planes_window_corpus as pwc
import planes_window_each_corpus as pwe
from planes_corpus import GENERIC, TILE
from planes_each_corpus import IDS, PLAIN, PRED, SUB, XOR

RUN = pwe.RUN
FILL = pwe.FILL
MED = pwe.MED                                                  # 2051 elements: the tensors that take every window
STRIDES = tuple(range(2, psc.MAX_STRIDE + 1))                  # the strides that the stride-1 calls do not know
lead = pwe.lead                                                # a % RUN for a PRED tensor with a < b, whatever its stride


def ends(m, S=1):
    """what a and b are drawn from: the ends of planes_window_each_corpus.py and the two sides of the chain heads of the first two runs"""
    more = (S - 1, S, S + 1, RUN + S - 1, RUN + S, RUN + S + 1) if S > 1 else ()
    return sorted({x for x in pwe.ENDS + more + (m - 1, m) if 0 <= x <= m})


def window_set(m, S=1):
    pts = ends(m, S)
    return [(a, b) for a in pts for b in pts if a <= b]


def whole_planes(t, base, E, tr, st=1):
    """the E planes of the whole tensor under transform tr, PRED at stride st, as the split writes them"""
    return pc.planes_of(pes.forward(t, base, E, tr, st), E)


def window_merge_model(planes, base_window, E, tr, st, a, b):
    """elements [a, b) of the tensor whose WHOLE planes under transform tr (PRED at stride st) these are: for PRED invert from the start of the
    run that holds a -- there every chain starts -- then slice"""
    if tr == PRED:
        a0 = a - lead(tr, a, b)
        z = pc.merge_one([np.asarray(p[a0:b]) for p in planes], E)
        return psc.inverse(z, E, st)[(a - a0) * E:]
    return pwe.window_merge_model(planes, base_window, E, tr, a, b)


def merge_verdict(tr, st, has_base, a, b, E, plane_sizes, plane_offsets, slot):
    """the result of one tensor of the merge-only call: a refused transform or, for PRED alone, a refused stride byte; then the rules of
    planes_window_each_corpus.py"""
    if not pes.accepted(tr, st, has_base):
        return GENERIC
    return pwe.merge_verdict(tr, has_base, a, b, E, plane_sizes, plane_offsets, slot)


# ---- the patch's stage
def segment_slices(t, base, E, tr, st, a, b, seg_log):
    """segments k0 .. k1 of every plane of transform(WHOLE tensor): what the patch has to stage for the window [a, b)"""
    at, m = ppc.sub_range(len(t), a, b, E, seg_log)
    k0 = at // E
    return [np.asarray(p[k0:k0 + pc.plane_size(m, j, E)]) for j, p in enumerate(whole_planes(t, base, E, tr, st))]


def sub_planes(t, base, E, tr, st, a, b, seg_log):
    """the planes of transform(sub-tensor): what the kernel computes -- runs, chains and chunks counted from the sub-tensor's start"""
    at, m = ppc.sub_range(len(t), a, b, E, seg_log)
    return pc.planes_of(pes.forward(t[at:at + m], None if base is None else base[at:at + m], E, tr, st), E)


def stage_model(tensors, windows, E, seg_log, transforms, strides, bases=None, stage_off=None):
    """-> (stage bytes, written mask, staged plane offsets, results) of FSEHIP_planes_split_window_each_stride_dbatch for tensors laid back to
    back from 0: planes_patch_each_corpus.stage_each_model with one more cause of rule 1, the stride byte of a PRED tensor"""
    sizes = [len(t) for t in tensors]
    ok_win = [pwc.window_valid(n, a, b, E) for n, (a, b) in zip(sizes, windows)]
    right = ppc.stage_offsets(sizes, [w if ok else (0, 0) for w, ok in zip(windows, ok_win)], E, seg_log)
    T = right if stage_off is None else [int(x) for x in stage_off]
    cap = T[-1]
    out, written = np.zeros(cap, np.uint8), np.zeros(cap, bool)
    P, res = [], []
    for i, raw in enumerate(tensors):
        a, b = windows[i]
        m = ppc.sub_range(sizes[i], a, b, E, seg_log)[1] if ok_win[i] else 0
        ok = ok_win[i] and T[i] <= T[i + 1] <= cap and T[i + 1] - T[i] == m and pes.accepted(transforms[i], strides[i], bases is not None)
        if not ok:
            P += [min(T[i], cap)] * E
            res.append(GENERIC)
            continue
        pos = T[i]
        for pl in segment_slices(raw, None if bases is None else bases[i], E, transforms[i], strides[i], a, b, seg_log):
            P.append(pos)
            out[pos:pos + len(pl)] = pl
            written[pos:pos + len(pl)] = True
            pos += len(pl)
        assert pos == T[i + 1]
        res.append(m)
    P.append(min(T[-1], cap))
    return out, written, P, res


# ---------------------------------------------------------------------------------------------------------------- the corpus of the merge test
def _smooth(rng, m, E, S):
    """m elements of S interleaved slow walks around levels of their own: differences at stride S are small, those at stride 1 are not"""
    x = (np.cumsum(rng.integers(-3, 4, m)) + 1000 + 5000 * (np.arange(m) % S)).astype("<u8")
    return np.ascontiguousarray(x.view(np.uint8).reshape(-1, 8)[:, :E]).reshape(-1)


def merge_corpus(E, seed=0):
    """-> dict(tensors, bases, transforms, strides, windows, D, counts, tiny=(lo, hi), walk=(lo, hi), first_med): tensors with a window each and
    the destination slots D (len + 1 offsets; slot i holds its window and a gap of guard bytes behind it, the first slot lies 7 bytes in).
      two PRED tensors of several tiles at strides 4 (divides 16) and 3 (does not), sixty tiny ones (1 .. 40 elements) whose slots lie inside
      one tile, two more of several tiles (PRED at stride 7, PLAIN), 32 tensors of MED elements whose transforms walk twice through all 16
      ordered neighbour pairs -- their stride bytes are 0 and 0xFF in turn where the transform is not PRED --, then for every stride 2 .. 8 one
      PRED tensor of MED elements per window of window_set(MED, S)."""
    rng = np.random.default_rng(300 * E + seed)
    big = 2 * TILE // E + 4096 + 7
    counts, windows, transforms, strides = [], [], [], []

    def add(m, w, tr, st):
        counts.append(m); windows.append(w); transforms.append(tr); strides.append(st)
    add(big, (1, big), PRED, 4)
    add(big + 3, (1023, big + 2), PRED, 3)
    tiny_lo = len(counts)
    cyc = pe.cycle_all_pairs(60, 8)
    for k in range(60):
        m = 1 + (7 * k) % 40
        pts = pwe.ends(m)
        a, b = (pts[k % len(pts)], m) if k % 3 else (pts[(k // 3) % len(pts)], pts[-1 - (k // 3) % 2])
        add(m, (min(a, b), max(a, b)), cyc[k], STRIDES[k % 7] if cyc[k] == PRED else (0, 0xFF, 1, 9)[k % 4])
    tiny_hi = len(counts)
    add(big + 1, (1025, big + 1), PRED, 7)
    add(big + 2, (2047, big + 2), PLAIN, 0xFF)
    walk_lo = len(counts)
    walk = pe.cycle_all_pairs(33)
    ws = window_set(MED)
    for k, tr in enumerate(walk):
        add(MED, ws[(5 * k + 1) % len(ws)], tr, STRIDES[k % 7] if tr == PRED else (0, 0xFF)[k % 2])
    walk_hi = len(counts)
    first_med = len(counts)
    for S in STRIDES:
        for w in window_set(MED, S):
            add(MED, w, PRED, S)
    n = len(counts)
    sizes = [m * E + (i % E if i % 5 == 0 else 0) for i, m in enumerate(counts)]          # some with n mod E trailing bytes: never inside a window
    tensors = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    for i in range(0, n, 3):                                    # smooth ones, whose differences are small: sums that carry rarely
        tensors[i][:counts[i] * E] = _smooth(rng, counts[i], E, strides[i] if transforms[i] == PRED else 1)
    bases = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    D, at = [], 7
    for i, (a, b) in enumerate(windows):
        if i == tiny_lo:
            at = -(-at // TILE) * TILE + 5                      # the tiny slots start a tile
        D.append(at)
        at += E * (b - a) + 1 + (3 * i) % 17
    D.append(at)
    return dict(tensors=tensors, bases=bases, transforms=transforms, strides=strides, windows=windows, D=D, counts=counts, tiny=(tiny_lo, tiny_hi), walk=(walk_lo, walk_hi),
                first_med=first_med)


def shapes(c, E):
    """what the corpus holds, by name: the merge test needs every one of these to be True"""
    tr, st, w, D, m = c["transforms"], c["strides"], c["windows"], c["D"], c["counts"]
    lo, hi = c["tiny"]
    n = len(tr)
    med = range(c["first_med"], n)
    pred = [i for i in range(n) if tr[i] == PRED and st[i] in STRIDES and w[i][0] < w[i][1]]
    L = {i: w[i][0] % RUN for i in pred}
    return {
        "every stride meets every window between its ends": {(st[i], w[i]) for i in med if tr[i] == PRED} == {(S, x) for S in STRIDES for x in window_set(MED, S)},
        "the ends of the issue": all(set(ends(MED, S)) == {0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, MED - 1, MED, S - 1, S, S + 1, RUN + S - 1, RUN + S, RUN + S + 1}
                                     for S in STRIDES),
        "a lead below S": all(any(st[i] == S and 0 < L[i] < S for i in pred) for S in STRIDES),
        "a lead that is no multiple of S": all(any(st[i] == S and L[i] % S for i in pred) for S in STRIDES),
        "the largest lead": all(any(st[i] == S and L[i] == RUN - 1 for i in pred) for S in STRIDES),
        "a window inside one chunk of 16, off the chunk's start": all(any(st[i] == S and w[i][0] % 16 and w[i][0] // 16 == (w[i][1] - 1) // 16 and L[i] for i in pred)
                                                                      for S in STRIDES),
        "a full chunk that straddles the lead": all(any(st[i] == S and L[i] % 16 and w[i][1] - w[i][0] >= 32 for i in pred) for S in STRIDES),
        "a window shorter than S": all(any(st[i] == S and w[i][1] - w[i][0] < S and L[i] for i in pred) for S in STRIDES),
        "an empty window off a run start": all(any(tr[i] == PRED and st[i] == S and w[i][0] == w[i][1] and w[i][0] % RUN for i in med) for S in STRIDES),
        "a PRED tensor of fewer than 16 elements": any(m[i] < 16 for i in pred),
        "a non-PRED tensor whose stride byte is 0, and one whose is 0xFF": all(any(tr[i] != PRED and st[i] == x and w[i][0] < w[i][1] for i in range(n)) for x in (0, 0xFF)),
        "all 16 ordered neighbour pairs": pe.neighbour_pairs(tr, *c["walk"]) == set(pe.PAIRS),
        "sixty tiny tensors inside one tile": hi - lo == 60 and D[lo] // TILE == (D[hi] - 1) // TILE and max(m[lo:hi]) <= 40,
        "all four transforms among the tiny ones": {tr[i] for i in range(lo, hi)} == set(IDS),
        "tensors of several tiles, at a stride that divides 16 and at one that does not":
            all(any(st[i] == S and E * (w[i][1] - w[i][0]) > 2 * TILE for i in pred) for S in (4, 3, 7)),
        "slots off every alignment": {D[i] % 16 for i in pred if w[i][1] - w[i][0] > 16} == set(range(16)),
        "guard bytes around every slot": D[0] > 0 and all(D[i + 1] - D[i] > E * (w[i][1] - w[i][0]) for i in range(n)),
    }

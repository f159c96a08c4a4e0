"""The numpy model of "patching tensors with a transform per tensor" (include/fsehip.h) shared by test_planes_patch_each_model.py and
test_gpu_planes_patch_each.py: what FSEHIP_planes_split_window_each_dbatch stages -- segments k0 .. k1 of the planes of transform(WHOLE tensor),
which the model test shows to be the planes of transform(sub-tensor) -- and the corpus of the split test with the shapes it has to contain.
Built on the models there are (planes_each_corpus.py, planes_patch_corpus.py, planes_window_each_corpus.py); plain Python, never the library.
Tensors are numpy uint8 arrays, windows are in elements."""
import numpy as np

import planes_corpus as pc
import planes_each_corpus as pe
import planes_patch_corpus as ppc
import planes_window_corpus as pwc
import planes_window_each_corpus as pwe
from planes_corpus import GENERIC, TILE
from planes_each_corpus import IDS, PLAIN, PRED

RUN = pwe.RUN
FILL = pwe.FILL
LEAD = 7                                                       # T[0] of the corpus: guard bytes in front of the stage


def segment_slices(t, base, E, tr, a, b, seg_log):
    """segments k0 .. k1 of every plane of transform(WHOLE tensor): what the patch has to stage for the window [a, b)"""
    at, m = ppc.sub_range(len(t), a, b, E, seg_log)
    k0 = at // E
    return [np.asarray(p[k0:k0 + pc.plane_size(m, j, E)]) for j, p in enumerate(pwe.whole_planes(t, base, E, tr))]


def sub_planes(t, base, E, tr, a, b, seg_log):
    """the planes of transform(sub-tensor): what the kernel computes -- runs and chunks counted from the sub-tensor's start"""
    at, m = ppc.sub_range(len(t), a, b, E, seg_log)
    return pc.planes_of(pe.forward(t[at:at + m], None if base is None else base[at:at + m], E, tr), E)


def stage_each_model(tensors, windows, E, seg_log, transforms, bases=None, stage_off=None, stage_cap=None, capacity=None):
    """-> (stage bytes, written mask, staged plane offsets, results) of FSEHIP_planes_split_window_each_dbatch for tensors laid back to back
    from 0: planes_patch_corpus.stage_model with the transform read per tensor and one more cause of rule 1 -- a transform that is none of the
    four, or XOR / SUB without a base.  stage_off: the T handed in (default: the right one from 0)"""
    sizes = [len(t) for t in tensors]
    S = [int(x) for x in pc.offsets(tensors)]
    ok_win = [pwc.window_valid(n, a, b, E) for n, (a, b) in zip(sizes, windows)]
    right = ppc.stage_offsets(sizes, [w if ok else (0, 0) for w, ok in zip(windows, ok_win)], E, seg_log)
    T = right if stage_off is None else [int(x) for x in stage_off]
    cap = T[-1] if stage_cap is None else int(stage_cap)
    capacity = S[-1] if capacity is None else int(capacity)
    out, written = np.zeros(cap, np.uint8), np.zeros(cap, bool)
    P, res = [], []
    for i, raw in enumerate(tensors):
        a, b = windows[i]
        ok = ok_win[i] and S[i + 1] <= capacity
        m = ppc.sub_range(sizes[i], a, b, E, seg_log)[1] if ok else 0
        ok = ok and T[i] <= T[i + 1] <= cap and T[i + 1] - T[i] == m and pe.accepted(transforms[i], bases is not None)
        if not ok:
            P += [min(T[i], cap)] * E
            res.append(GENERIC)
            continue
        pos = T[i]
        for pl in segment_slices(raw, None if bases is None else bases[i], E, transforms[i], a, b, seg_log):
            P.append(pos)
            out[pos:pos + len(pl)] = pl
            written[pos:pos + len(pl)] = True
            pos += len(pl)
        assert pos == T[i + 1]
        res.append(m)
    P.append(min(T[-1], cap))
    return out, written, P, res


# ---------------------------------------------------------------------------------------------------------------- the corpus of the split test
def split_corpus(E, seg_log=10, seed=0):
    """-> dict(tensors, bases, transforms, windows, T, tiny=(lo, hi), first_med, counts): the merge corpus of planes_window_each_corpus.py -- two
    tensors of several tiles, sixty tiny ones, two more of several tiles, 320 tensors of MED elements in which every transform meets every
    window between the ends and the transforms walk through all 16 ordered neighbour pairs -- with one PLAIN filler in front of the tiny ones,
    sized so that all sixty are staged inside one tile, and the stage offsets T from LEAD on"""
    c = pwe.merge_corpus(E, seed)
    lo, hi = c["tiny"]
    sizes = [len(t) for t in c["tensors"]]
    T = ppc.stage_offsets(sizes, c["windows"], E, seg_log)
    fill = (5 - (LEAD + T[lo])) % TILE                          # the tiny ones start 5 bytes into a tile of the stage
    fill += TILE if fill < 64 else 0
    rng = np.random.default_rng(900 + E + seed)
    ins = dict(tensors=rng.integers(0, 256, fill, dtype=np.uint8), bases=rng.integers(0, 256, fill, dtype=np.uint8), transforms=PLAIN, windows=(0, fill // E),
               counts=fill // E)
    out = {k: list(c[k][:lo]) + [ins[k]] + list(c[k][lo:]) for k in ins}
    sizes = [len(t) for t in out["tensors"]]
    out["T"] = [LEAD + x for x in ppc.stage_offsets(sizes, out["windows"], E, seg_log)]
    out["tiny"], out["first_med"] = (lo + 1, hi + 1), c["first_med"] + 1
    return out


def shapes(c, E, seg_log=10):
    """what the corpus holds, by name: the split test needs every one of these to be True"""
    tr, w, T, m, ts = c["transforms"], c["windows"], c["T"], c["counts"], c["tensors"]
    lo, hi = c["tiny"]
    n = len(tr)
    med = range(c["first_med"], n)
    pred = [i for i in range(n) if tr[i] == PRED]
    staged = [T[i + 1] - T[i] for i in range(n)]
    return {
        "all 16 ordered neighbour pairs": pe.neighbour_pairs(tr) == set(pe.PAIRS),
        "every transform meets every window": {(tr[i], w[i]) for i in med} == {(t, x) for t in IDS for x in pwe.window_set(pwe.MED)},
        "the ends of the issue": set(pwe.ends(pwe.MED)) == {0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, pwe.MED - 1, pwe.MED},
        "a window that ends at the last element of a tensor with a partial element behind it":
            all(any(tr[i] == t and w[i][1] == m[i] and w[i][0] < w[i][1] and len(ts[i]) % E for i in range(n)) for t in IDS) if E > 1 else True,
        "empty windows": all(any(tr[i] == t and w[i][0] == w[i][1] for i in range(n)) for t in IDS),
        "a PRED window that starts inside a run": any(w[i][0] % RUN and w[i][0] < w[i][1] for i in pred),
        "a PRED sub-tensor that starts behind the tensor's start": any((w[i][0] >> seg_log) > 0 and w[i][0] < w[i][1] for i in pred),
        "a PRED tensor of fewer than 16 elements": any(m[i] < 16 and w[i][0] < w[i][1] for i in pred),
        "sixty tiny tensors inside one tile of the stage": hi - lo == 60 and T[lo] // TILE == (T[hi] - 1) // TILE and max(m[lo:hi]) <= 40,
        "all four transforms among the tiny ones": {tr[i] for i in range(lo, hi)} == set(IDS),
        "staged tensors of several tiles": all(any(tr[i] == t and staged[i] > 2 * TILE for i in range(n)) for t in IDS),
        "stage slots off every alignment": {T[i] % 16 for i in range(n) if staged[i] > 16 * E} == set(range(16)),
        "guard bytes in front of the stage": T[0] == LEAD,
    }

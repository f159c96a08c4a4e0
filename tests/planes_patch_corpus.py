"""The numpy model of patching segmented tensors (include/fsehip.h, "patching segmented tensors") shared by test_planes_patch_model.py and
test_gpu_planes_patch.py: which bytes of a tensor its selected segments cover and where they are staged, which frames of the object a window
selects, what the splice makes of an old and a new batch of frames -- offsets, results, codecs, where every frame's bytes come from, the
verdict per tensor in the order of the header -- and which workgroup of the gather copies which piece, by brute force.  Plain Python built on
planes_seg_corpus.py and planes_window_corpus.py, never the library.  Sizes, offsets and windows are python ints, error results negative."""
import numpy as np

import planes_corpus as pc
import planes_seg_corpus as psc
import planes_window_corpus as pwc
from planes_corpus import CORRUPT, GENERIC, TILE, TOO_SMALL

ELEMS = pc.ELEMS


def sub_range(n, a, b, E, seg_log):
    """-> (at, m): the bytes [at, at + m) of a tensor of n bytes that the segments holding the elements [a, b) cover, by enumeration over the
    tensor's bytes: byte x belongs to segment (x // E) >> seg_log of its plane"""
    ks = pwc.selected(pc.plane_size(n, 0, E), a, b, seg_log)
    if not ks:
        return (a >> seg_log << seg_log) * E, 0
    inside = [x for x in (ks[0] * E << seg_log, min(n, (ks[-1] + 1) * E << seg_log))]
    assert all(((x // E) >> seg_log) in ks for x in range(inside[0], inside[1], max(1, (inside[1] - inside[0]) // 97)))
    assert inside[0] == 0 or ((inside[0] - 1) // E) >> seg_log not in ks
    assert inside[1] == n or (inside[1] // E) >> seg_log not in ks
    return inside[0], inside[1] - inside[0]


def stage_offsets(sizes, windows, E, seg_log):
    """T: the running sum of the staged bytes per tensor"""
    out = [0]
    for n, (a, b) in zip(sizes, windows):
        out.append(out[-1] + sub_range(int(n), a, b, E, seg_log)[1])
    return out


def stage_model(tensors, windows, E, seg_log, bases=None, stage_off=None, stage_cap=None, capacity=None):
    """-> (stage bytes, written mask, staged plane offsets, results) of FSEHIP_planes_split_window_dbatch for tensors laid back to back from 0.
    stage_off: the T handed in (default: the right one); a tensor whose pair does not hold exactly its staged bytes below stage_cap, whose
    window is not valid or which ends behind `capacity` is refused: GENERIC, all its entries min(T[i], stage_cap)"""
    sizes = [len(t) for t in tensors]
    S = [int(x) for x in pc.offsets(tensors)]
    ok_win = [pwc.window_valid(n, a, b, E) for n, (a, b) in zip(sizes, windows)]
    right = stage_offsets(sizes, [w if ok else (0, 0) for w, ok in zip(windows, ok_win)], E, seg_log)
    T = right if stage_off is None else [int(x) for x in stage_off]
    cap = T[-1] if stage_cap is None else int(stage_cap)
    capacity = S[-1] if capacity is None else int(capacity)
    out, written = np.zeros(cap, np.uint8), np.zeros(cap, bool)
    P, res = [], []
    for i, raw in enumerate(tensors):
        a, b = windows[i]
        ok = ok_win[i] and S[i + 1] <= capacity
        at, m = sub_range(sizes[i], a, b, E, seg_log) if ok else (0, 0)
        ok = ok and T[i] <= T[i + 1] <= cap and T[i + 1] - T[i] == m
        if not ok:
            P += [min(T[i], cap)] * E
            res.append(GENERIC)
            continue
        sub = np.asarray(raw[at:at + m], np.uint8)
        if bases is not None:
            sub = sub ^ np.asarray(bases[i][at:at + m], np.uint8)
        pos = T[i]
        for pl in pc.planes_of(sub, E):
            P.append(pos)
            out[pos:pos + len(pl)] = pl
            written[pos:pos + len(pl)] = True
            pos += len(pl)
        assert pos == T[i + 1]
        res.append(m)
    P.append(min(T[-1], cap))
    return out, written, P, res


def selected_frames(sizes, windows, E, seg_log):
    """the frames q of the object that valid windows select, in the order of the selected frames r"""
    first = psc.seg_first(sizes, E, seg_log)
    out = []
    for i, (n, (a, b)) in enumerate(zip(sizes, windows)):
        for p in range(E):
            out += [first[i * E + p] + k for k in pwc.selected(pc.plane_size(int(n), p, E), a, b, seg_log)]
    return out


def extent_ok(F, R, q, cap):
    return 0 <= F[q] <= F[q + 1] <= cap and 0 <= R[q] <= F[q + 1] - F[q]


def splice_model(F, R, NF, NR, sizes, windows, E, seg_log, frames_cap, new_cap, out_cap, C=None, NC=None, seg_first=None, sel_first=None, nsel=None, stage_res=None):
    """-> dict(off, res, src, codecs, tres, fits) of FSEHIP_planes_splice_dbatch.  F, R (C): the object's frame offsets, results (codecs); NF, NR
    (NC): the new frames'.  src[q] = ("new", r) or ("old", q) or None (no byte).  The verdict per tensor in the header's order: the window and
    the split's result, the counts, the old extents, the writer's results"""
    nseg = len(R)
    right = psc.seg_first(sizes, E, seg_log)
    seg_first = right if seg_first is None else [int(x) for x in seg_first]
    sel_first = pwc.window_first(sizes, windows, E, seg_log)[0] if sel_first is None else [int(x) for x in sel_first]
    nsel = sel_first[-1] if nsel is None else nsel
    acc = pwc.accepted(sizes, windows, E, seg_log, seg_first, sel_first, nsel)
    ext, res, src, cod, tres = [None] * nseg, [None] * nseg, [None] * nseg, [None] * nseg, []
    owner = {}
    for i, n in enumerate(sizes):
        verdict = 0
        a, b = windows[i]
        planes = range(i * E, (i + 1) * E)
        if stage_res is not None and stage_res[i] < 0:
            verdict = stage_res[i]
        elif not acc[i] or any(seg_first[j] > seg_first[j + 1] or seg_first[j + 1] > nseg for j in planes):
            verdict = GENERIC
        elif any(not extent_ok(F, R, q, frames_cap) for q in range(seg_first[i * E], seg_first[(i + 1) * E])):
            verdict = CORRUPT
        else:
            for j in planes:
                ks = pwc.selected(pc.plane_size(int(n), j % E, E), a, b, seg_log)
                rs = range(sel_first[j], sel_first[j] + len(ks))
                errs = [NR[r] for r in rs if NR[r] < 0]
                verdict = errs[0] if errs else CORRUPT if any(not extent_ok(NF, NR, r, new_cap) for r in rs) else 0
                if verdict:
                    break
                for t, k in enumerate(ks):
                    owner[seg_first[j] + k] = sel_first[j] + t
        if verdict:
            for j in planes:
                for q in range(max(seg_first[j], 0), min(seg_first[j + 1], nseg)):
                    owner.pop(q, None)
        tres.append(verdict if verdict else int(n))
    for q in range(nseg):
        if q in owner:
            r = owner[q]
            ext[q], res[q], src[q], cod[q] = NF[r + 1] - NF[r], NR[r], ("new", r), None if C is None else NC[r]
        else:
            inside = 0 <= F[q] <= F[q + 1] <= frames_cap
            ext[q] = F[q + 1] - F[q] if inside else 0
            res[q] = R[q] if inside and (R[q] < 0 or R[q] <= ext[q]) else GENERIC
            src[q] = ("old", q) if res[q] > 0 else None
            cod[q] = None if C is None else C[q]
    off = [0]
    for e in ext:
        off.append(off[-1] + e)
    fits = off[-1] <= out_cap
    if not fits:
        tres = [TOO_SMALL] * len(sizes)
    return dict(off=off, res=res, src=src, codecs=None if C is None else cod, tres=tres, fits=fits)


def splice_bytes(model, frames, new_frames, F, NF, out_cap, fill):
    """the output buffer of the model: every frame's real bytes at its new offset, the fill everywhere else"""
    out = np.full(out_cap, fill, np.uint8)
    if not model["fits"]:
        return out
    for q, s in enumerate(model["src"]):
        r = model["res"][q]
        if s is None or r <= 0:
            continue
        at = NF[s[1]] if s[0] == "new" else F[s[1]]
        out[model["off"][q]:model["off"][q] + r] = (new_frames if s[0] == "new" else frames)[at:at + r]
    return out


def gather_pieces(off, lens, n_groups, T=TILE):
    """by brute force: the (frame q, tile t) intersections of frames of `lens` real bytes at off[q] with tiles of T bytes -- as the set of
    (w, q, first byte, end) with w = q + t, the workgroup the mapping gives it"""
    out = set()
    for q, n in enumerate(lens):
        if n <= 0:
            continue
        for t in range(off[q] // T, (off[q] + n - 1) // T + 1):
            assert q + t < n_groups
            out.add((q + t, q, max(off[q], t * T), min(off[q] + n, (t + 1) * T)))
    return out


def gather_map(off, lens, n_groups, T=TILE):
    """the same from the kernel's side: workgroup w looks its frame up by the plane kernels' work mapping over the NEW offsets and clips the
    frame's real bytes to its tile"""
    nseg = len(lens)
    out = set()
    total = off[nseg]
    for w in range(n_groups):
        if nseg == 0 or w > total // T + nseg or off[0] // T > w:
            continue
        lo, hi = 0, nseg - 1
        while lo < hi:
            mid = lo + ((hi - lo + 1) >> 1)
            if off[mid] // T + mid <= w:
                lo = mid
            else:
                hi = mid - 1
        q, t = lo, w - lo
        b0, b1 = max(t * T, off[q]), min((t + 1) * T, off[q] + max(lens[q], 0))
        if b0 < b1:
            out.add((w, q, b0, b1))
    return out

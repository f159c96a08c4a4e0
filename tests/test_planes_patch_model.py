"""Patching segmented tensors without a device (include/fsehip.h, "patching segmented tensors"): the defining identity with the oracle's frame
writer -- the frames of the selected segments of `new` put in the place of those of `old` ARE the segmented frames of `new`, offsets
included, at both alignments; the staged sub-tensor, whose planes are the selected segments of the tensor's planes and which has exactly the
window's count of segments per plane; the gather's work mapping over the new frame offsets against brute force; the host arithmetic of the
binding; and the new calls' argument checks, which answer before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_packed_corpus as fpc
import planes_corpus as pc
import planes_patch_corpus as ppc
import planes_seg_corpus as psc
import planes_window_corpus as pwc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
ERR = (1 << 64) - 1
SZ, VP, U64 = C.c_size_t, C.c_void_p, C.c_uint64
EXPORTS = ("FSEHIP_planes_split_window_dbatch", "FSEHIP_planes_spliceScratchBound", "FSEHIP_planes_splice_dbatch", "FSEHIP_tensor_patch_window_dbatch")
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


def _planes():
    """old and new: the sign / exponent plane of 150,001 bf16 N(0, 0.02) elements, and the same with the bytes [40,000, 90,001) drawn again"""
    if "planes" not in _CACHE:
        old = np.ascontiguousarray(pc.planes_of(pc.bf16_gaussian(150001, 7), 2)[1])
        new = old.copy()
        new[40000:90001] = pc.planes_of(pc.bf16_gaussian(150001, 8), 2)[1][40000:90001]
        _CACHE["planes"] = (old, new, (40000, 90001))
    return _CACHE["planes"]


def _segment_frames(oracle, which, bsid, codec, seg_log):
    key = (which, bsid, codec, seg_log)
    if key not in _CACHE:
        plane = _planes()[which]
        out = []
        for a in range(0, plane.size, 1 << seg_log):
            r, buf = oracle.frame_compress(plane[a:a + (1 << seg_log)], bsid, codec)
            out.append(buf[:r].copy())
        _CACHE[key] = out
    return _CACHE[key]


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("bsid,seg_kib", [(0, 1), (0, 4), (0, 32), (0, 64), (5, 32), (5, 64)])
def test_the_selected_frames_of_new_in_place_of_those_of_old_are_the_frames_of_new(checker, bsid, seg_kib, codec):
    seg_log = 10 + seg_kib.bit_length() - 1
    old, new, (a, b) = _planes()
    assert old.size == 150001 and (old[:a] == new[:a]).all() and (old[b:] == new[b:]).all() and not (old[a:b] == new[a:b]).all()
    fo, fn = _segment_frames(checker, 0, bsid, codec, seg_log), _segment_frames(checker, 1, bsid, codec, seg_log)
    sel = ppc.selected_frames([old.size], [(a, b)], 1, seg_log)
    assert sel == list(range(a >> seg_log, ((b - 1) >> seg_log) + 1)) and 0 < len(sel) < len(fo) == len(fn) == psc.seg_count(old.size, seg_log)
    assert any(len(fo[q]) != len(fn[q]) for q in sel), "the patch moves the frames behind it"
    for align_log in (0, 6):
        F, NF = fpc.packed_offsets([len(f) for f in fo], align_log), fpc.packed_offsets([len(fn[q]) for q in sel], align_log)
        frames, fresh = np.full(F[-1], 0xEE, np.uint8), np.full(NF[-1], 0xDD, np.uint8)
        for q, f in enumerate(fo):
            frames[F[q]:F[q] + len(f)] = f
        for r, q in enumerate(sel):
            fresh[NF[r]:NF[r] + len(fn[q])] = fn[q]
        m = ppc.splice_model(F, [len(f) for f in fo], NF, [len(fn[q]) for q in sel], [old.size], [(a, b)], 1, seg_log, F[-1], NF[-1], F[-1] + NF[-1])
        want = fpc.packed_offsets([len(f) for f in fn], align_log)
        assert m["off"] == want and m["res"] == [len(f) for f in fn] and m["tres"] == [old.size] and m["fits"]
        assert m["src"] == [("new", sel.index(q)) if q in sel else ("old", q) for q in range(len(fo))]
        out = ppc.splice_bytes(m, frames, fresh, F, NF, want[-1] + 16, 0xA5)
        for q, f in enumerate(fn):
            assert (out[want[q]:want[q] + len(f)] == f).all(), q
            assert (out[want[q] + len(f):want[q + 1]] == 0xA5).all(), "padding inside an extent is not written"
        assert (out[want[-1]:] == 0xA5).all()
        # a byte short: nothing is written, the offsets are whole
        short = ppc.splice_model(F, [len(f) for f in fo], NF, [len(fn[q]) for q in sel], [old.size], [(a, b)], 1, seg_log, F[-1], NF[-1], want[-1] - 1)
        assert short["off"] == want and short["tres"] == [pc.TOO_SMALL] and not short["fits"]


def _patch_sizes(E, seg_log):
    """tensor sizes in bytes: multiples of E and not, whole elements that end on a segment boundary with and without a partial element behind
    them, less than a segment, several segments"""
    s = 1 << seg_log
    return [E * 3 * s, E * 3 * s + E - 1, E * 3 * s + 1, E * (2 * s + 5) + E // 2, E * s - 1, E * (s - 1), E + 1, E * (4 * s + 1), E * 2 * s + E - 1]


@pytest.mark.parametrize("seg_log", [10, 11])
@pytest.mark.parametrize("E", ppc.ELEMS)
def test_the_planes_of_the_staged_sub_tensor_are_the_selected_segments(E, seg_log):
    s = 1 << seg_log
    sizes = _patch_sizes(E, seg_log)
    tensors = pc.random_tensors(sizes, 40 + E + seg_log)
    assert any((n // E) % s == 0 and n % E == 0 for n in sizes) and (E == 1 or any((n // E) % s == 0 and n % E for n in sizes))
    ends = set()
    for raw, n in zip(tensors, sizes):
        planes = pc.planes_of(raw, E)
        for a, b in pwc.boundary_windows(n // E, seg_log):
            ks = pwc.selected(len(planes[0]), a, b, seg_log)
            at, m = ppc.sub_range(n, a, b, E, seg_log)
            assert at % E == 0 and (m == 0) == (a == b)
            if a == b:
                continue
            ends.add((b == n // E, (n // E) % s == 0, n % E != 0))
            assert ks == list(range(a >> seg_log, ((b - 1) >> seg_log) + 1))
            sub = pc.planes_of(raw[at:at + m], E)
            for p in range(E):
                # every plane of the tensor has these segments, and the sub-tensor's plane is exactly their bytes, a partial last element included
                assert pwc.selected(len(planes[p]), a, b, seg_log) == ks
                assert (sub[p] == planes[p][ks[0] * s:(ks[-1] + 1) * s]).all() and len(sub[p]) == pc.plane_size(m, p, E)
                assert psc.seg_count(len(sub[p]), seg_log) == len(ks), "exactly cnt segments per plane: the segments kernel runs over the stage with selFirst"
    assert {(True, True, False), (True, False, False), (False, False, False)} <= ends and (E == 1 or {(True, True, True), (True, False, True)} <= ends)
    # ... so the segment offsets of the stage, with the stage offsets as the tensors' and selFirst as segFirst, are those of the selected segments
    windows = [pwc.boundary_windows(n // E, seg_log)[(7 * i + 3) % len(pwc.boundary_windows(n // E, seg_log))] for i, n in enumerate(sizes)]
    windows[0], windows[1] = (s - 1, 2 * s + 1), (3 * s - 1, 3 * s)
    T = ppc.stage_offsets(sizes, windows, E, seg_log)
    staged = [T[i + 1] - T[i] for i in range(len(sizes))]
    sel, _ = pwc.window_first(sizes, windows, E, seg_log)
    counts = [sel[j + 1] - sel[j] for j in range(len(sizes) * E)]
    for i, m in enumerate(staged):
        if windows[i][0] < windows[i][1]:
            assert [psc.seg_count(pc.plane_size(m, p, E), seg_log) for p in range(E)] == counts[i * E:(i + 1) * E]
    from finitestateentropy_amd.api import FseHip
    assert [int(x) for x in FseHip.planes_stage_offsets(None, sizes, windows, E, seg_log)] == T
    _, written, P, res = ppc.stage_model(tensors, windows, E, seg_log)
    assert res == staged and written.all() and P[-1] == T[-1]


def test_stage_offsets_refusals():
    from finitestateentropy_amd.api import FseHip
    for args in (([8], [(0, 5)], 2, 10), ([8], [(3, 2)], 2, 10), ([8], [(0, 1)], 3, 10), ([8], [(0, 1)], 2, 9), ([8], [(0, 1), (0, 1)], 2, 10), ([-1], [(0, 0)], 1, 10)):
        with pytest.raises((ValueError, TypeError)):
            FseHip.planes_stage_offsets(None, *args)


def test_the_gathers_work_mapping_against_brute_force():
    T = ppc.TILE
    rng = np.random.default_rng(77)
    layouts = []
    # many empty and tiny frames in one tile, frames that end on, one short of and one behind a tile boundary, a frame over several tiles
    lens = [0] * 40 + [8] * 300 + [0, 1, 0, 0, 15, 16, 17] + [T - 8 * 300 - 49, 1, T - 1, T, T + 1, 0, 3 * T + 5, 0, 0, 9]
    layouts.append((lens, [n + (5 if q % 11 == 3 else 0) for q, n in enumerate(lens)]))           # some extents padded
    lens = [int(x) for x in rng.integers(0, 40, 3000)]
    layouts.append((lens, [(n + 63) & ~63 for n in lens]))                                            # slots aligned to 64
    lens = [int(x) for x in rng.integers(0, 3 * T, 40)]
    layouts.append((lens, lens))
    layouts.append(([0] * 500, [0] * 500))
    layouts.append(([-1, 5, -2, 0], [0, 8, 0, 0]))                                                    # frames with an error take and move nothing
    for lens, exts in layouts:
        off = [0]
        for e in exts:
            off.append(off[-1] + e)
        for cap in (off[-1], off[-1] + 2 * T + 1):
            groups = (cap + T - 1) // T + len(lens)
            want = ppc.gather_pieces(off, lens, groups)
            got = ppc.gather_map(off, lens, groups)
            assert got == want
            covered = sorted((b0, b1) for _, _, b0, b1 in got)
            assert sum(b1 - b0 for b0, b1 in covered) == sum(max(n, 0) for n in lens) and all(x[1] <= y[0] for x, y in zip(covered, covered[1:]))
            assert len({w for w, _, _, _ in got}) == len(got), "one workgroup per piece"
    # the same search as the plane kernels' mapping
    off = [0, 5, 5, T - 1, T + 9, 4 * T]
    assert {(w, q) for w, q, _, _ in ppc.gather_map(off, [5, 0, T - 6, 10, 3 * T - 9], 20)} == {(w, i) for w, i, _ in pc.work_map(off, 20)}


def test_splice_model_refuses_a_tensor_whole():
    E, seg_log = 2, 10
    s = 1 << seg_log
    sizes = [E * 3 * s, E * 2 * s, E * (s + 1)]
    windows = [(s, s + 1), (0, 2 * s), (5, 5)]
    first, (sel, _) = psc.seg_first(sizes, E, seg_log), pwc.window_first(sizes, windows, E, seg_log)
    assert first == [0, 3, 6, 8, 10, 12, 14] and sel == [0, 1, 2, 4, 6, 6, 6]
    R = [20 + q for q in range(14)]
    F = fpc.packed_offsets(R, 0)
    NR = [50 + r for r in range(6)]
    NF = fpc.packed_offsets(NR, 0)
    args = (sizes, windows, E, seg_log, F[-1], NF[-1], 10 ** 6)
    good = ppc.splice_model(F, R, NF, NR, *args)
    assert good["tres"] == sizes and [x[0] for x in good["src"]] == ["old", "new", "old", "old", "new", "old"] + ["new"] * 4 + ["old"] * 4
    assert good["res"][1] == 50 and good["res"][4] == 51 and good["res"][6:10] == [52, 53, 54, 55] and good["off"][-1] == sum(good["res"])
    # a writer's error: the first in plane and segment order, the tensor keeps all its frames, the others are patched
    bad = list(NR)
    bad[3], bad[4] = -7, -9
    m = ppc.splice_model(F, R, NF, bad, *args)
    assert m["tres"] == [sizes[0], -7, sizes[2]] and m["src"][6:10] == [("old", q) for q in range(6, 10)] and m["src"][:6] == good["src"][:6]
    # an old extent that does not hold its frame, selected or not
    for q in (7, 9):
        short = list(R)
        short[q] = F[q + 1] - F[q] + 1
        m = ppc.splice_model(F, short, NF, NR, *args)
        assert m["tres"] == [sizes[0], pc.CORRUPT, sizes[2]] and m["res"][q] == pc.GENERIC and m["src"][q] is None and m["src"][6] == ("old", 6)
    # the old extents come in front of the writer's errors, the window and the counts in front of both
    m = ppc.splice_model(F, short, NF, bad, *args)
    assert m["tres"][1] == pc.CORRUPT
    wrong = list(sel)
    wrong[3] -= 1
    m = ppc.splice_model(F, short, NF, bad, *args, sel_first=wrong)
    assert m["tres"] == [sizes[0], pc.GENERIC, sizes[2]] and m["src"][:6] == good["src"][:6]
    m = ppc.splice_model(F, R, NF, NR, *args, stage_res=[sizes[0], -1, 0])
    assert m["tres"] == [sizes[0], -1, sizes[2]]


def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    assert not hasattr(lib, "FSEHIP_tensor_patch_window_dbatch_workspaceSize") and not hasattr(lib, "FSEHIP_planes_splice_dbatch_workspaceSize")
    bound = lib.FSEHIP_planes_spliceScratchBound
    bound.restype = SZ
    assert bound(SZ(3), C.c_uint(3), SZ(10)) == ERR and bound(SZ(1 << 31), C.c_uint(1), SZ(10)) == ERR and bound(SZ(1), C.c_uint(1), SZ(1 << 31)) == ERR
    small, more = bound(SZ(0), C.c_uint(1), SZ(0)), bound(SZ(100), C.c_uint(8), SZ(5000))
    assert 0 < small < more < (1 << 20) and small % 256 == 0 and more >= 100 * 8 * 8 + 5000 * 8
    # a non-null address that is never dereferenced: every refusal is decided on the host
    p = VP(256)
    split = lib.FSEHIP_planes_split_window_dbatch

    def split_args(E=2, seg_log=10, n=1, cap=U64(64), poff=p, stage=p):
        return (stage, poff, p, p, VP(0), p, p, p, SZ(n), C.c_uint(E), C.c_uint(seg_log), U64(64), cap, VP(0))
    for kw in (dict(E=3), dict(seg_log=9), dict(seg_log=31), dict(n=1 << 30), dict(cap=U64(1 << 46)), dict(poff=VP(0)), dict(stage=VP(0))):
        assert split(*split_args(**kw)) == HIP_INVALID_VALUE, kw
    splice = lib.FSEHIP_planes_splice_dbatch

    def splice_args(E=2, seg_log=10, nseg=4, nsel=2, out_cap=U64(64), codecs=(VP(0), VP(0), VP(0)), scratch=p, scratch_bytes=1 << 20, new=p, foff=p):
        return (p, out_cap, p, p, codecs[0], p, p, U64(64), foff, p, codecs[1], new, U64(64), p, p, codecs[2], VP(0), p, p, SZ(1), C.c_uint(E), p, SZ(nseg),
                C.c_uint(seg_log), p, SZ(nsel), scratch, SZ(scratch_bytes), VP(0))
    for kw in (dict(E=5), dict(seg_log=9), dict(nsel=5), dict(nseg=1 << 31), dict(out_cap=U64(1 << 46)), dict(codecs=(p, VP(0), VP(0))), dict(codecs=(p, p, VP(0))),
               dict(codecs=(VP(0), VP(0), p)), dict(scratch=VP(0)), dict(scratch=VP(264)), dict(scratch_bytes=255), dict(new=VP(0)), dict(foff=VP(0))):
        assert splice(*splice_args(**kw)) == HIP_INVALID_VALUE, kw
    patch = lib.FSEHIP_tensor_patch_window_dbatch

    def patch_args(E=2, seg_log=10, nsel=2, bsid=0, codec=0, align=0, blocks=4, ws=p, ws_bytes=1 << 30, stage_cap=U64(64), toff=p, scratch_bytes=1 << 20):
        return (p, U64(64), p, p, VP(0), p, p, U64(64), p, p, VP(0), p, VP(0), p, U64(64), p, SZ(1), C.c_uint(E), p, SZ(4), C.c_uint(seg_log), p, SZ(nsel), toff,
                stage_cap, SZ(blocks), C.c_uint(bsid), C.c_int(codec), VP(0), C.c_int(0), C.c_uint(0), C.c_uint(align), p, p, p, p, p, U64(64), p, p, p, SZ(scratch_bytes),
                ws, SZ(ws_bytes), VP(0))
    for kw in (dict(E=3), dict(seg_log=9), dict(seg_log=10, bsid=1), dict(bsid=7), dict(codec=2), dict(align=13), dict(blocks=1 << 31), dict(ws=VP(264)), dict(ws_bytes=16),
               dict(nsel=5), dict(stage_cap=U64(1 << 46)), dict(toff=VP(0)), dict(scratch_bytes=255)):
        assert patch(*patch_args(**kw)) == HIP_INVALID_VALUE, kw

"""Windows of segmented tensors without a device (include/fsehip.h, "windows of segmented tensors"): FSEHIP_planes_windowFirst against the
brute-force model of planes_window_corpus.py, its exact block count and its refusals; the premise the feature stands on -- with the oracle's
frame reader an extent that starts at a segment's frame and runs on over the frames behind it reads as that frame alone; the models of the
selection and of the fold, one case per branch of the fold, with deliberately broken variants of the model told apart; and the new calls'
argument checks, which answer before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

import planes_corpus as pc
import planes_seg_corpus as psc
import planes_window_corpus as pwc
from planes_corpus import CORRUPT, GENERIC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
ERR = (1 << 64) - 1
SZ, VP, U64 = C.c_size_t, C.c_void_p, C.c_uint64
EXPORTS = ("FSEHIP_planes_windowFirst", "FSEHIP_planes_select_window_dbatch", "FSEHIP_planes_fold_window_dbatch", "FSEHIP_tensor_decompress_window_dbatch")
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    lib = C.CDLL(path)
    lib.FSEHIP_planes_windowFirst.restype = SZ
    return lib


def _window_first(lib, sizes, windows, E, seg_log, bsid=0, fill=True):
    offs = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)
    win = np.asarray([x for w in windows for x in w] + [0xA5], dtype=np.uint64)
    out = np.full(len(sizes) * E + 2, 0xA5A5A5A5, dtype=np.uint64)
    blocks = SZ(0xA5A5)
    r = lib.FSEHIP_planes_windowFirst(out.ctypes.data_as(VP) if fill else VP(0), C.byref(blocks) if fill else VP(0), offs.ctypes.data_as(VP), win.ctypes.data_as(VP),
                                      SZ(len(sizes)), C.c_uint(E), C.c_uint(seg_log), C.c_uint(bsid))
    assert int(out[-1]) == 0xA5A5A5A5, "one entry more than planes, no further"
    return int(r), [int(x) for x in out[:-1]], int(blocks.value)


def _spread(sizes, E, seg_log, rng):
    """one window per tensor, drawn from the boundary windows of each, so that every kind appears over a few rounds"""
    out = []
    for n in sizes:
        cand = pwc.boundary_windows(int(n) // E, seg_log)
        out.append(cand[int(rng.integers(0, len(cand)))])
    return out


@pytest.mark.parametrize("E", pwc.ELEMS)
def test_window_first_against_the_model(lib, E):
    from finitestateentropy_amd.api import FseHip
    rng = np.random.default_rng(70 + E)
    for seg_log in (10, 11, 14):
        s = 1 << seg_log
        sizes = pwc.window_sizes(E, seg_log) + [int(x) for x in rng.integers(0, 5 * E * s, 12)]
        planes = psc.plane_sizes(sizes, E)
        assert 0 in sizes and (E == 1 or (any(0 < n < E for n in sizes) and any(n > E and n % E for n in sizes)))
        if E > 1:                                            # the planes of one tensor with different sizes and different counts
            assert any(len({psc.seg_count(planes[i * E + p], seg_log) for p in range(E)}) > 1 for i in range(len(sizes)))
        seen = set()
        for bsid in (0, seg_log - 10):
            for rnd in range(40):
                windows = _spread(sizes, E, seg_log, rng) if rnd else [(0, n // E) for n in sizes]
                want, blocks = pwc.window_first(sizes, windows, E, seg_log, bsid)
                r, got, gblocks = _window_first(lib, sizes, windows, E, seg_log, bsid)
                assert r == want[-1] and got == want and gblocks == blocks, (seg_log, bsid, rnd)
                assert _window_first(lib, sizes, windows, E, seg_log, bsid, fill=False)[0] == want[-1], "the count alone"
                pfirst, pblocks = FseHip.planes_window_first(None, sizes, windows, E, seg_log, bsid)
                assert [int(x) for x in pfirst] == want and pblocks == blocks, "the Python arithmetic is the same function"
                if not rnd:                                  # every whole element: every segment of every plane that holds one, and all their blocks but
                    full = psc.seg_first(sizes, E, seg_log)   # those of the planes' bytes of a partial last element
                    assert all(w - v <= f - e for v, w, e, f in zip(want, want[1:], full, full[1:]))
                    assert [w - v for v, w in zip(want, want[1:])] == [-(-(n // E) // s) for n in sizes for _ in range(E)]
                for (a, b), n in zip(windows, sizes):
                    seen |= {"empty"} if a == b else {"whole"} if (a, b) == (0, n // E) and n >= E else set()
                    if a < b and a >> seg_log == (b - 1) >> seg_log and (a, b) != (0, n // E):
                        seen.add("inside one segment")
                    for x, name in ((a, "a"), (b, "b")):
                        if x and x % s == 0:
                            seen.add(name + " on a boundary")
                        if x % s == s - 1:
                            seen.add(name + " one short of a boundary")
                        if x > s and x % s == 1:
                            seen.add(name + " one behind a boundary")
        assert seen == {"empty", "whole", "inside one segment"} | {x + y for x in "ab" for y in (" on a boundary", " one short of a boundary", " one behind a boundary")}
    assert _window_first(lib, [], [], E, 10) == (0, [0], 0)


def test_window_first_counts_exactly_the_blocks_of_the_selected_segments(lib):
    # a plane of 5000 bytes (E = 1) at 2 KB segments and 1 KB blocks: segments of 2, 2 and 1 blocks (the last holds 904 bytes)
    for window, segments, blocks in (((0, 5000), 3, 5), ((0, 2048), 1, 2), ((2047, 2049), 2, 4), ((4096, 4097), 1, 1), ((2048, 5000), 2, 3), ((77, 77), 0, 0)):
        assert pwc.window_first([5000], [window], 1, 11, 0) == ([0, segments], blocks)
        assert _window_first(lib, [5000], [window], 1, 11, 0) == (segments, [0, segments], blocks)
    # E = 2, 4097 bytes: plane 0 has 2049 bytes (two segments), plane 1 2048 (one); only elements 0 .. 2047 are addressable, all in segment 0
    assert _window_first(lib, [4097], [(0, 2048)], 2, 11, 0) == (2, [0, 1, 2], 4)
    assert _window_first(lib, [4097], [(0, 2048)], 2, 11, 1) == (2, [0, 1, 2], 2)
    assert _window_first(lib, [4097], [(0, 2049)], 2, 11, 0)[0] == ERR, "the partial last element is not addressable"


def test_window_first_refusals(lib):
    from finitestateentropy_amd.api import FseHip
    ok = ([10], [(1, 3)])
    assert _window_first(lib, *ok, 2, 10) == (2, [0, 1, 2], 2)
    for E in (0, 3, 16):
        offs, win = (U64 * 2)(0, 10), (U64 * 2)(1, 3)
        assert lib.FSEHIP_planes_windowFirst(VP(0), VP(0), offs, win, SZ(1), C.c_uint(E), C.c_uint(10), C.c_uint(0)) == ERR, E
    offs, win = (U64 * 2)(0, 10), (U64 * 2)(1, 3)
    for seg_log, bsid in ((0, 0), (9, 0), (31, 0), (64, 0), (10, 1), (15, 6), (20, 7)):
        assert lib.FSEHIP_planes_windowFirst(VP(0), VP(0), offs, win, SZ(1), C.c_uint(2), C.c_uint(seg_log), C.c_uint(bsid)) == ERR, (seg_log, bsid)
    assert lib.FSEHIP_planes_windowFirst(VP(0), VP(0), offs, win, SZ(1), C.c_uint(2), C.c_uint(16), C.c_uint(6)) == 2
    for window in ((3, 1), (0, 6), (6, 6), (5, 1 << 63), ((1 << 64) - 1, (1 << 64) - 1)):                         # a > b, b > floor(n / E)
        win = (U64 * 2)(*window)
        assert lib.FSEHIP_planes_windowFirst(VP(0), VP(0), offs, win, SZ(1), C.c_uint(2), C.c_uint(10), C.c_uint(0)) == ERR, window
    assert lib.FSEHIP_planes_windowFirst(VP(0), VP(0), offs, (U64 * 2)(5, 5), SZ(1), C.c_uint(2), C.c_uint(10), C.c_uint(0)) == 0
    assert lib.FSEHIP_planes_windowFirst(VP(0), VP(0), VP(0), win, SZ(1), C.c_uint(2), C.c_uint(10), C.c_uint(0)) == ERR
    assert lib.FSEHIP_planes_windowFirst(VP(0), VP(0), offs, VP(0), SZ(1), C.c_uint(2), C.c_uint(10), C.c_uint(0)) == ERR
    # 2^31 selected frames or more: one tensor of 2^41 bytes at 1 KB segments is exactly 2^31; a segment less, one frame less
    big = (U64 * 2)(0, 1 << 41)
    assert lib.FSEHIP_planes_windowFirst(VP(0), VP(0), big, (U64 * 2)(0, 1 << 41), SZ(1), C.c_uint(1), C.c_uint(10), C.c_uint(0)) == ERR
    assert lib.FSEHIP_planes_windowFirst(VP(0), VP(0), big, (U64 * 2)(1024, 1 << 41), SZ(1), C.c_uint(1), C.c_uint(10), C.c_uint(0)) == (1 << 31) - 1
    for args in (([10], [(1, 3)], 3, 10), ([10], [(1, 3)], 2, 9), ([10], [(1, 3)], 2, 31), ([10], [(1, 3)], 2, 10, 1), ([10], [(1, 3)], 2, 20, 7), ([10], [(3, 1)], 2, 10),
                 ([10], [(0, 6)], 2, 10), ([10], [(-1, 2)], 2, 10), ([10], [], 2, 10), ([1 << 41], [(0, 1 << 41)], 1, 10, 0)):
        with pytest.raises((ValueError, TypeError)):
            FseHip.planes_window_first(None, *args)


def _segment_frames(oracle, codec, seg_log):
    """the oracle's frames of the segments of a plane of 150,001 bytes of bf16 N(0, 0.02) data (plane 1: sign and exponent; plane 0 with codec 1)"""
    key = (codec, seg_log)
    if key not in _CACHE:
        if "planes" not in _CACHE:
            _CACHE["planes"] = [np.ascontiguousarray(p) for p in pc.planes_of(pc.bf16_gaussian(150001, 7), 2)]
        plane = _CACHE["planes"][1 - codec]
        assert plane.size == 150001
        parts = []
        for a in range(0, plane.size, 1 << seg_log):
            r, buf = oracle.frame_compress(plane[a:a + (1 << seg_log)], 0, codec)
            parts.append(buf[:r].copy())
        _CACHE[key] = (plane, parts)
    return _CACHE[key]


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("seg_log", [13, 15])
def test_an_extent_with_trailing_frames_reads_as_its_first_frame(checker, seg_log, codec):
    s = 1 << seg_log
    plane, parts = _segment_frames(checker, codec, seg_log)
    assert len(parts) == psc.seg_count(plane.size, seg_log) > 4
    for k in range(len(parts)):
        want = plane[k * s:(k + 1) * s]
        alone = checker.frame_decompress(parts[k], s)
        rest = checker.frame_decompress(np.concatenate(parts[k:]), s)
        assert alone[0] == rest[0] == len(want), k
        assert (alone[1][:len(want)] == want).all() and (rest[1][:len(want)] == want).all(), k
        assert (rest[1][len(want):] == 0).all(), "nothing of the frames behind it is regenerated"
    # ... with padding in front of the next frame too, as between packed frames
    gap = np.concatenate([parts[1], np.full(13, 0xEE, np.uint8), parts[3]])
    r, out = checker.frame_decompress(gap, s)
    assert r == s and (out[:s] == plane[s:2 * s]).all()


def _laid_out(sizes, E, seg_log):
    """frame offsets of frames of invented sizes (8 bytes and a few more per segment), one per segment of every plane"""
    first = psc.seg_first(sizes, E, seg_log)
    F = [0]
    for q in range(first[-1]):
        F.append(F[-1] + 8 + (q * 7) % 23)
    return first, F


def test_select_model_picks_the_frames_of_the_window_and_refuses_only_the_tensor_whose_counts_are_wrong():
    E, seg_log = 2, 10
    s = 1 << seg_log
    sizes = [E * (3 * s + 5), 0, E * 2 * s + 1, E * s]
    windows = [(s - 1, 2 * s + 1), (0, 0), (0, 2 * s), (7, 7)]
    first, F = _laid_out(sizes, E, seg_log)
    assert first == [0, 4, 8, 9, 10, 13, 15, 16, 17]
    sel, blocks = pwc.window_first(sizes, windows, E, seg_log)
    assert sel == [0, 3, 6, 6, 6, 8, 10, 10, 10] and blocks == 10
    got = pwc.select_model(F, sizes, windows, E, seg_log)
    frames = [0, 1, 2, 4, 5, 6, 10, 11, 13, 14]
    assert got == [F[q] for q in frames] + [F[15]] and got == sorted(got)
    # extent r holds selected frame r at its start and runs over the unselected frames to the next selected one
    assert [got[r + 1] - got[r] >= F[q + 1] - F[q] for r, q in enumerate(frames)] == [True] * 10
    # tensor 2 with one frame too few in selFirst for its plane 0, one too many for plane 1: it alone is refused
    wrong = list(sel)
    wrong[2 * E + 1] -= 1
    bad = pwc.select_model(F, sizes, windows, E, seg_log, sel_first=wrong)
    assert pwc.accepted(sizes, windows, E, seg_log, first, wrong, 10) == [True, True, False, True]
    assert bad[:6] == got[:6] and bad[6:] == [F[first[3 * E]]] * 5 and bad == sorted(bad)
    # a wrong count in segFirst does the same, and so does a window behind the tensor's last whole element
    wrong = list(first)
    wrong[2 * E + 1] += 1
    assert pwc.select_model(F, sizes, windows, E, seg_log, seg_first=wrong)[6:] == [F[first[3 * E]]] * 5
    late = list(windows)
    late[2] = (1, 2 * s + 1)
    assert pwc.select_model(F, sizes, late, E, seg_log, sel_first=sel)[6:] == [F[first[3 * E]]] * 5
    # the refused tensor in front: the accepted ones behind it keep their frames
    wrong = [0, 2] + [x for x in sel[2:]]
    bad = pwc.select_model(F, sizes, windows, E, seg_log, sel_first=wrong)
    assert bad[:6] == [F[first[E]]] * 6 and bad[6:] == got[6:]
    # nothing selected
    assert pwc.select_model(F, sizes, [(0, 0), (0, 0), (5, 5), (s, s)], E, seg_log) == [F[0]]


def test_fold_verdict_one_case_per_branch_and_broken_models_told_apart():
    for seg_log in (10, 20):
        cases = pwc.fold_cases(seg_log)
        for name, size, a, b, refused, off, res, want in cases:
            assert len(off) == len(res) + 1
            assert pwc.fold_plane(off, res, a, b, size, seg_log, refused) == want, name
        assert {w[1] for *_, w in cases} >= {GENERIC, CORRUPT, 0, -3, -2}
        for variant in pwc.VARIANTS:
            differs = [name for name, size, a, b, refused, off, res, want in cases if pwc.fold_plane(off, res, a, b, size, seg_log, refused, variant) != want]
            assert differs, "no case tells the model with '%s' from the right one" % variant
    # the whole-array form: planes cut by selFirst; a refused tensor's planes are GENERIC whatever their segments say
    E, seg_log, s = 2, 10, 1024
    sizes = [E * (2 * s + 9), E * s, 3]
    windows = [(s - 2, 2 * s + 9), (4, 4), (0, 1)]
    sel, _ = pwc.window_first(sizes, windows, E, seg_log)
    assert sel == [0, 3, 6, 6, 6, 7, 8]
    off = [0, s, 2 * s, 5000, 5000 + s, 5000 + 2 * s, 9000, 9002, 9003]
    res = [s, s, 9, s, -4, 9, 2, 1]
    assert pwc.fold_model(off, res, sizes, windows, E, seg_log) == ([s - 2, 0, 0, 0, 9000, 9002], [s + 11, -4, 0, 0, 1, 1])
    wrong = list(sel)
    wrong[1] -= 1
    assert pwc.fold_model(off, res, sizes, windows, E, seg_log, sel_first=wrong)[1] == [GENERIC, GENERIC, 0, 0, 1, 1]
    assert pwc.fold_model(off, res, sizes, windows, E, seg_log, nsel=7)[1] == [s + 11, -4, 0, 0, GENERIC, GENERIC], "a selection that ends behind nSelected"


def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    a = (C.c_uint64 * 8)()
    p = C.cast(a, VP)
    null = VP(0)
    u = C.c_uint
    se, fo, td = lib.FSEHIP_planes_select_window_dbatch, lib.FSEHIP_planes_fold_window_dbatch, lib.FSEHIP_tensor_decompress_window_dbatch

    def select(ptrs=None, n=1, E=2, nseg=4, nsel=2, seg_log=10):
        return se(*(ptrs or [p] * 6), SZ(n), u(E), SZ(nseg), SZ(nsel), u(seg_log), null)

    def fold(ptrs=None, n=1, E=2, nsel=2, seg_log=10):
        return fo(*(ptrs or [p] * 8), SZ(n), u(E), SZ(nsel), u(seg_log), null)

    def window(E=2, seg_log=10, n=1, nseg=4, nsel=2, blocks=4, cap=8, base=null, ws=null, wsize=0, **nulls):
        names = ("dst", "doff", "res", "frames", "foff", "soff", "win", "sf", "wf", "planes", "sfo", "so", "sres", "poff", "psz")
        assert set(nulls) <= set(names)
        q = {k: null if k in nulls else p for k in names}
        return td(q["dst"], q["doff"], U64(cap), base, q["res"], q["frames"], q["foff"], q["soff"], q["win"], SZ(n), u(E), q["sf"], SZ(nseg), u(seg_log), q["wf"], SZ(nsel),
                  SZ(blocks), q["planes"], U64(8), q["sfo"], q["so"], q["sres"], q["poff"], q["psz"], ws, SZ(wsize), null), names
    for E in (0, 3, 5, 16, 0xFFFFFFFF):
        assert select(E=E) == fold(E=E) == window(E=E)[0] == HIP_INVALID_VALUE, E
    for seg_log in (0, 9, 31, 40):
        assert select(seg_log=seg_log) == fold(seg_log=seg_log) == window(seg_log=seg_log)[0] == HIP_INVALID_VALUE, seg_log
    for big in (1 << 31, 1 << 40):
        assert select(nseg=big) == select(nseg=big, nsel=big) == window(nseg=big)[0] == window(nseg=big, nsel=big)[0] == HIP_INVALID_VALUE
        assert fold(nsel=big) == HIP_INVALID_VALUE
        assert window(blocks=big)[0] == HIP_INVALID_VALUE
    assert select(n=1 << 30) == fold(n=1 << 30) == window(n=1 << 30)[0] == HIP_INVALID_VALUE, "2^31 planes"
    assert select(nseg=4, nsel=5) == window(nseg=4, nsel=5)[0] == HIP_INVALID_VALUE, "more selected frames than frames"
    for k in range(6):
        assert select([null if x == k else p for x in range(6)]) == HIP_INVALID_VALUE, k
    for k in range(8):
        assert fold([null if x == k else p for x in range(8)]) == HIP_INVALID_VALUE, k
    # the composite: everything the steps check, in front of the first launch -- a too small workspace last of all
    for name in window()[1]:
        assert window(**{name: True})[0] == HIP_INVALID_VALUE, name
    assert window(cap=1 << 46)[0] == window(cap=1 << 40)[0] == HIP_INVALID_VALUE, "a capacity the merge cannot launch for"
    assert window(ws=VP(128), wsize=1 << 30)[0] == HIP_INVALID_VALUE, "a misaligned workspace"
    assert window()[0] == window(base=p)[0] == window(nsel=0)[0] == HIP_INVALID_VALUE, "a workspace of no bytes"
    need = lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    need.restype = SZ
    assert need(SZ(2), SZ(4)) > 1
    assert window(ws=VP(256), wsize=need(SZ(2), SZ(4)) - 1)[0] == HIP_INVALID_VALUE, "a workspace one byte short"
    assert all(x == 0 for x in a)

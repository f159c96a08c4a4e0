"""The device building blocks without a device: the numpy models of tests/devtest_models.py against hand-written cases; the two test-only
libraries (tests/device/devtest.hip, the DPP and the shuffle build) load and list exactly the operations of the models' table; every refusal
of FSEHIP_devtest_run comes back as hipErrorInvalidValue with nothing launched (there is no device here to launch on); and the host side of
pl_size / pl_start against Python integers for sizes up to 2^63."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import devtest_lib as dl
import devtest_models as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32, M64 = dm.M32, dm.M64


@pytest.fixture(scope="module", params=dl.KINDS)
def lib(request):
    return dl.load(request.param)


# ---------------------------------------------------------------------------------------------------------------- the models
def _wave(fn):
    return np.array([[fn(l) for l in range(64)]], dtype=np.uint64)


def test_scans_by_hand():
    ones = _wave(lambda l: 1)
    assert dm.scan_incl(ones, 64, "add").tolist() == [list(range(1, 65))]
    assert dm.scan_incl(ones, 8, "add").tolist() == [[l % 8 + 1 for l in range(64)]]
    assert dm.scan_excl(ones, 16).tolist() == [[l % 16 for l in range(64)]]
    top = _wave(lambda l: M32)
    assert dm.scan_incl(top, 32, "add").tolist() == [[(M32 * (l % 32 + 1)) & M32 for l in range(64)]], "sums wrap"
    assert dm.reduce(top, 64, "add").tolist() == [[(64 * M32) & M32] * 64]
    lanes = _wave(lambda l: l)
    assert dm.scan_incl(lanes, 16, "max").tolist() == [list(range(64))]
    assert dm.scan_incl(lanes, 16, "min").tolist() == [[l & ~15 for l in range(64)]]
    assert dm.reduce(lanes, 32, "max").tolist() == [[31] * 32 + [63] * 32]
    assert dm.group_last(lanes, 8).tolist() == [[l | 7 for l in range(64)]]
    assert dm.lane_xor(lanes, 16).tolist() == [[l ^ 16 for l in range(64)]]
    # 64 bits: the carry out of the low half in lane 1, the wrap of the whole sum in the last lane
    v = _wave(lambda l: 0xFFFFFFFF)
    assert dm.scan_incl(v, 64, "add", 64)[0, :3].tolist() == [0xFFFFFFFF, 0x1FFFFFFFE, 0x2FFFFFFFD]
    v = _wave(lambda l: 1 << 63)
    assert dm.scan_incl(v, 8, "add", 64)[0, :4].tolist() == [1 << 63, 0, 1 << 63, 0]
    assert dm.scan_excl(v, 8, 64)[0, :4].tolist() == [0, 1 << 63, 0, 1 << 63]


def test_signed_max_any_suffix_min_bytesum_by_hand():
    v = np.array([[0x80000000, 0xFFFFFFFF] * 32], dtype=np.uint32)
    assert dm.wave_max_i32(v).tolist() == [[0xFFFFFFFF] * 64], "-1 is above INT_MIN"
    v[0, 5] = 0
    assert dm.wave_max_i32(v).tolist() == [[0] * 64]
    p = np.zeros((1, 64), dtype=np.uint32)
    p[0, 17] = 1
    assert dm.group_any(p, 8).tolist() == [[1 if 16 <= l < 24 else 0 for l in range(64)]]
    assert dm.group_any(p, 64).tolist() == [[1] * 64]
    lanes = _wave(lambda l: l)
    assert dm.suffix_min_excl(lanes, 8).tolist() == [[M32 if l % 8 == 7 else l + 1 for l in range(64)]]
    fall = _wave(lambda l: 100 - l)
    assert dm.suffix_min_excl(fall, 16).tolist() == [[M32 if l % 16 == 15 else 100 - (l | 15) for l in range(64)]]
    assert dm.bytesum(np.array([0x01020304, 0xFFFFFFFF, 0], dtype=np.uint32)).tolist() == [10, 1020, 0]


def test_zigzag_by_hand():
    for E in dm.ELEMS:
        top = (1 << (8 * E)) - 1
        assert [dm.zz_int(t, 0, E) for t in (0, top, 1, top - 1, 2)] == [0, 1, 2, 3, 4]
        assert dm.zz_int(1 << (8 * E - 1), 0, E) == top, "the most negative difference takes the last code"
        assert dm.zz_int(0, 1, E) == 1 and dm.zz_int(5, 7, E) == 3 and dm.zz_int(7, 5, E) == 4
        rng = np.random.default_rng(E)
        t, b = [rng.integers(0, 256, 8 * 50, dtype=np.uint8).view("<u%d" % E) for _ in range(2)]
        z = dm.zz(t, b, E)
        assert z.tolist() == [dm.zz_int(int(x), int(y), E) for x, y in zip(t, b)]
        assert dm.unzz(z, b, E).tolist() == t.tolist() and [dm.unzz_int(int(x), int(y), E) for x, y in zip(z, b)] == t.tolist()
    w = np.array([[5, 0, 0xFF, 0x80] * 4], dtype=np.uint8)
    b = np.array([[7, 1, 0, 0] * 4], dtype=np.uint8)
    assert dm.sub4(w, b, 1, False).tolist() == [[3, 1, 1, 0xFF] * 4]
    assert dm.sub4(dm.sub4(w, b, 1, False), b, 1, True).tolist() == w.tolist()
    assert dm.sub4(w, b, 2, False).view("<u2")[0, :2].tolist() == [dm.zz_int(0x0005, 0x0107, 2), dm.zz_int(0x80FF, 0, 2)]


def test_interleave_prefix_carry_rotate_by_hand():
    chunk = np.arange(32, dtype=np.uint8).reshape(1, 32)
    assert dm.deinterleave(chunk, 2).tolist() == [[list(range(0, 32, 2)), list(range(1, 32, 2))]]
    assert dm.interleave(dm.deinterleave(chunk, 2), 2).tolist() == chunk.tolist()
    assert dm.deinterleave(np.arange(64, dtype=np.uint8).reshape(1, 64), 4)[0, 3].tolist() == list(range(3, 64, 4))
    ff = np.full((1, 16), 0xFF, dtype=np.uint8)
    words, total = dm.prefix(ff, 1)
    assert words.tolist() == [[(0xFF * (k + 1)) & 0xFF for k in range(16)]] and total.tolist() == [0xF0]
    words, total = dm.prefix(np.full((1, 32), 0xFF, dtype=np.uint8), 2)
    assert words.view("<u2").tolist() == [[(0xFFFF * (k + 1)) & 0xFFFF for k in range(16)]] and total.tolist() == [0xFFF0]
    assert dm.carry(ff, [2], 1).tolist() == [[1] * 16]
    assert dm.carry(np.zeros((1, 32), dtype=np.uint8), [0x1FF], 2).view("<u2").tolist() == [[0x1FF] * 16]
    assert dm.add_lanes(np.array([0x00FF00FF], dtype=np.uint32), np.array([0x00010001], dtype=np.uint32), 1).tolist() == [0]
    assert dm.add_lanes(np.array([0x00FF00FF], dtype=np.uint32), np.array([0x00010001], dtype=np.uint32), 2).tolist() == [0x01000100]
    assert dm.rotate(np.array([[10, 11, 12]]), [2], 3).tolist() == [[12, 10, 11]]
    buf = np.arange(100, dtype=np.uint8)
    assert dm.prev(buf, 40, 2, 1, False).tolist() == list(range(38, 70)) and dm.prev(buf, 40, 2, 1, True).tolist() == [0, 0] + list(range(40, 70))
    assert dm.prev(buf, 40, 1, 3, False).tolist() == list(range(37, 53)) and dm.prev(buf, 40, 1, 3, True).tolist() == [0] * 3 + list(range(40, 53))


def test_index_models_by_hand():
    assert [dm.pl_size(10, p, 4) for p in range(4)] == [3, 3, 2, 2] and [dm.pl_start(10, p, 4) for p in range(4)] == [0, 3, 6, 8]
    assert dm.pl_size(0, 0, 2) == 0 and dm.pl_size(1, 1, 2) == 0
    # a tensor of 10 bytes at flat 32766, E = 4: elements start at 32766, 32770, 32774 -- one in tile 0, two in tile 1
    assert dm.share_range(32766, 10, 0, 32768, 4) == (0, 1) and dm.share_range(32766, 10, 32768, 32768, 4) == (1, 3)
    assert dm.share_range(32767, 2, 32768, 32768, 4) is None, "the tile holds bytes of the tensor and no element's first byte"
    assert dm.last_le([3, 3, 5, 9], 4) == 1 and dm.last_le([3, 3, 5, 9], 2) == 0 and dm.last_le([3, 3, 5, 9], 99) == 3
    S = [0, 0, 100, 3 * 32768]                               # floor(S / T) + i = 0, 1, 2, 6
    assert [dm.find(S, w, 15) for w in range(8)] == [0, 1, 2, 2, 2, 2, 3, 3]
    assert dm.find([32768], 0, 15) is None


def test_bit_model_by_hand():
    # 0b1_01_1: the mark, then "01", then "1" -- read from the top
    m = dm.BitModel([0b1011])
    assert m.status is None and m.P == 3 and m.used == 61 and m.at == 0 and m.win == 0b1011
    assert m.read(2) == 0b01 and m.read(1) == 1 and m.used == 64 and m.reload() == dm.COMPLETED
    assert m.read(1) is None and m.reload() == dm.OVERFLOW
    assert dm.BitModel([]).status == "srcSize_wrong" and dm.BitModel([5, 0]).status == "corruption_detected" and dm.BitModel([1] * 7 + [0]).status == "GENERIC"
    assert dm.init_return(dm.BitModel([5, 0])) == (1 << 64) - 4 and dm.init_return(dm.BitModel([5, 1])) == 2
    s = list(range(1, 13))                                   # 12 bytes: the window is bytes 4 .. 11, the mark is bit 3 of byte 11 (12 = 0b1100)
    m = dm.BitModel(s)
    assert m.at == 4 and m.used == 5 and m.win == int.from_bytes(bytes(s[4:]), "little")
    assert m.read(3) == 0b100 and m.read(8) == 11 and m.read(0) == 0
    assert m.reload() == dm.UNFINISHED and (m.at, m.used) == (2, 0) and m.read(8) == 10
    m.read(24)
    assert m.reload() == dm.END_OF_BUFFER and (m.at, m.used) == (0, 16), "clamped at the stream's start"
    assert m.read(8) == 6
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    for name, code in dm.ERRORS.items():
        assert int(re.search(r"FSEHIP_error_%s\s*=\s*(\d+)" % name, header).group(1)) == code
    cells = [(1 << 24) | (65 << 16) | 2, 0, (2 << 24) | (66 << 16) | 0, (0 << 24) | (67 << 16) | 1]
    rows = dm.fse_steps([0b10110110, 0b1], cells, 0, 3)      # bits from the top: 1 0 1 1 0 1 1 0
    assert [r[:2] for r in rows] == [(65, 3), (67, 1), (0, 0)]


# ---------------------------------------------------------------------------------------------------------------- the libraries
def test_both_libraries_list_the_models_table(lib):
    assert dl.listing(lib) == dm.table()


def test_the_two_builds_are_the_two_forms():
    assert dl.load("dpp").FSEHIP_devtest_dpp() == 1 and dl.load("shfl").FSEHIP_devtest_dpp() == 0


def test_list_truncates_and_terminates(lib):
    need = lib.FSEHIP_devtest_list(None, 0)
    buf = C.create_string_buffer(b"\xAA" * 64, 64)
    assert lib.FSEHIP_devtest_list(buf, 16) == need
    assert buf.raw[15] == 0 and buf.raw[16:] == b"\xAA" * 48 and len(buf.value) == 15


def test_every_refusal_launches_nothing(lib):
    """Each call differs from an acceptable one in one argument.  An accepted call would have to launch, which cannot succeed without a device
    and would come back with another error than hipErrorInvalidValue."""
    IN, OUT = 0x10000, 0x20000                               # never dereferenced
    def run(name=b"group_scan_incl", a=64, b=0, n=256, d_in=IN, in_bytes=None, d_out=OUT, out_bytes=None, threads=64, words=(1, 1)):
        in_bytes = n * 4 * words[0] if in_bytes is None else in_bytes
        out_bytes = n * 4 * words[1] if out_bytes is None else out_bytes
        return lib.FSEHIP_devtest_run(name, a, b, n, d_in, in_bytes, d_out, out_bytes, threads, None)
    bad = dl.HIP_INVALID_VALUE
    assert run(name=None) == bad and run(name=b"") == bad and run(name=b"group_scan") == bad and run(name=b"group_scan_incl ") == bad
    for a, b in ((4, 0), (128, 0), (0, 0), (63, 0), (-1, 0), (64, 3), (64, -1)):
        assert run(a=a, b=b) == bad, (a, b)
    for threads in (0, 1, 32, 63, 65, 128, 255, 257, 512, 1024):
        assert run(threads=threads, n=1024) == bad, threads
    for n in (0, 1, 63, 65, 255):
        assert run(n=n) == bad and run(n=n, threads=256) == bad, n
    assert run(n=64 << 24) == bad, "more blocks than a grid of the tests ever has"
    assert run(in_bytes=1023) == bad and run(in_bytes=1025) == bad and run(in_bytes=0) == bad
    assert run(out_bytes=1023) == bad and run(out_bytes=1025) == bad and run(out_bytes=0) == bad
    assert run(d_in=None) == bad and run(d_out=None) == bad and run(d_in=IN + 4) == bad and run(d_out=OUT + 2) == bad
    # every operation: a template argument it does not have, and buffers of another operation's sizes
    for (name, a, b), words in dm.table().items():
        a0 = 1 if a == -1 else a
        if name == "pl_find" or name == "pl_last_le":
            continue
        assert run(name=name.encode(), a=a0, b=b + 100, words=words) == bad, name
        assert run(name=name.encode(), a=a0, b=b, words=(words[0], words[1] + 1)) == bad, name
        if a != -1:
            assert run(name=name.encode(), a=a + 1000, b=b, words=words) == bad, name
        if name not in ("pp_prev", "ps_prev"):                # (these take a payload of any size behind their records)
            assert run(name=name.encode(), a=a0, b=b, words=words, in_bytes=256 * 4 * words[0] + 4) == bad, name
        assert run(name=name.encode(), a=a0, b=b, words=words, in_bytes=256 * 4 * words[0] - 4) == bad, name
    # the run-time arguments
    for d in (0, 3, 5, 64, 48):
        assert run(name=b"lane_xor_any", a=d) == bad, d
    assert run(name=b"fse_step", a=2, words=dm.table()[("fse_step", -1, 0)]) == bad
    # pl_find / pl_last_le: the payload holds exactly a keys
    for name, words in ((b"pl_find", (2, 4)), (b"pl_last_le", (2, 2))):
        assert run(name=name, a=5, words=words, in_bytes=256 * 8 + 5 * 8 - 8) == bad and run(name=name, a=5, words=words, in_bytes=256 * 8 + 5 * 8 + 8) == bad
        assert run(name=name, a=1 << 20, words=words, in_bytes=256 * 8 + (8 << 20)) == bad
        assert run(name=name, a=5, b=1, words=words, in_bytes=256 * 8 + 40) == bad
    assert run(name=b"pl_last_le", a=0, words=(2, 2)) == bad, "pl_last_le needs one key at least"
    assert run(in_bytes=1 << 31, n=1 << 29, out_bytes=1 << 31) == bad


def test_pl_size_and_start_on_the_host(lib):
    assert lib.FSEHIP_devtest_tile() == 32768
    rng = np.random.default_rng(7)
    sizes = list(range(0, 70)) + [255, 256, 257, 32767, 32768, 32769, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 5,
                                  (1 << 53) + 1, (1 << 63) - 9, (1 << 63) - 1, 1 << 63]
    sizes += [int(x) for x in rng.integers(0, 1 << 63, 200, dtype=np.uint64)]
    for E in dm.ELEMS:
        for n in sizes:
            got = [int(lib.FSEHIP_devtest_pl_size(n, p, E)) for p in range(E)]
            starts = [int(lib.FSEHIP_devtest_pl_start(n, p, E)) for p in range(E)]
            assert got == [dm.pl_size(n, p, E) for p in range(E)], (n, E)
            assert sum(got) == n and starts == [sum(got[:p]) for p in range(E)], (n, E)
            if n < M32:
                assert lib.FSEHIP_devtest_pl_size(n, n, E) == 0 and lib.FSEHIP_devtest_pl_size(n, n + 1, E) == 0, "a plane index at or behind the size: empty"

"""The device building blocks on the GPU, one by one: every helper that tests/device/devtest.hip wraps (the DPP scans, reductions and lane
exchanges of dev_common.h and wave_glue.h, wb_scan_excl / wb_bytesum, the SWAR arithmetic, byte shuffles, work mapping and tile shares of
planes_dev.h, the LIFO bit reader) against the models of tests/devtest_models.py, in both builds of the library (the DPP forms the product
uses, and the shuffle forms of -DFSEHIP_NO_DPP_SCANS), in blocks of 64 and of 256 threads.  Every comparison is exact integer equality.

pl_share: the alignment property (alignAddr + eb alignStride is a multiple of 16 unless the head was clamped) is asserted wherever such a
boundary exists, i.e. where alignAddr is a multiple of alignStride; the callers pass alignStride = E only for such addresses (planes.hip), and
for the others the remaining properties (order, whole elements, head and tail shorter than a chunk, disjoint cover) are asserted all the same."""
import functools

import numpy as np
import pytest

import devtest_lib as dl
import devtest_models as dm

pytestmark = pytest.mark.gpu
M32, M64 = dm.M32, dm.M64
GOLD = 0x9E3779B9
GOLD64 = 0x9E3779B97F4A7C15
BLOCKS = (64, 256)
TABLE = dm.table()


@pytest.fixture(scope="module", params=dl.KINDS)
def lib(request):
    return dl.load(request.param)


def _check(lib, name, a, b, records, expected, payload=None, mask=None, what=""):
    """runs (name, a, b) over the records in blocks of 64 and of 256 and compares all stored dwords (those under `mask`) with `expected`"""
    words = TABLE[(name, -1 if (name, -1, b) in TABLE else a, b)]
    records = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, words[0])
    expected = np.ascontiguousarray(expected, dtype=np.uint32).reshape(-1, words[1])
    assert len(records) == len(expected) and len(records) >= 2 * 256, "two blocks at least"
    got = None
    for threads in BLOCKS:
        got = dl.run(lib, name, a, b, records, words[1], threads, payload)
        g, e = (got, expected) if mask is None else (got & mask, expected & mask)
        if not np.array_equal(g, e):
            r, c = np.argwhere(g != e)[0]
            raise AssertionError("%s<%d, %d> %s, blocks of %d: item %d (lane %d) word %d: got %#x, expected %#x; %d of %d items differ; record %s"
                                 % (name, a, b, what, threads, r, r % 64, c, g[r, c], e[r, c], (g != e).any(axis=1).sum(), len(g), [hex(x) for x in records[r][:10]]))
    return got


def _pad_waves(w):
    """(k, 64) -> the waves of whole blocks of 256, two blocks at least"""
    w = np.asarray(w)
    k = max(-(-len(w) // 4) * 4, 8)
    return np.concatenate([w, np.zeros((k - len(w), 64), dtype=w.dtype)])


# ---------------------------------------------------------------------------------------------------------------- cross-lane inputs
@functools.lru_cache(maxsize=None)
def waves32(ident):
    """the waves of 32-bit operands for an operation whose identity is `ident`"""
    rng = np.random.default_rng(1000 + (ident & 0xFF))
    lanes = np.arange(64, dtype=np.uint64)
    w = [np.zeros(64, np.uint64), np.full(64, M32, np.uint64), lanes]
    for r in range(64):                                      # one-hot: one recognisable value, the identity elsewhere
        v = np.full(64, ident, np.uint64); v[r] = (GOLD + r) & M32; w.append(v)
    for r in range(64):                                      # ... and its complement: the identity in lane r only
        v = (GOLD + lanes) & M32; v[r] = ident; w.append(v)
    for r in range(64):                                      # one 0 among all ones
        v = np.full(64, M32, np.uint64); v[r] = 0; w.append(v)
    for W in (8, 16, 32):                                    # neighbouring groups differ: a leak across a border shows
        even = (lanes // W) % 2 == 0
        w.append(np.where(even, M32, lanes)); w.append(np.where(even, lanes, M32)); w.append(np.where(even, 0, GOLD - lanes))
    w.append(np.array([0x80000000, 0xFFFFFFFF, 0, 0x7FFFFFFF] * 16, np.uint64))          # INT_MIN, -1, 0, INT_MAX
    w.append(np.where(lanes % 3 == 0, 0x80000000, 0xFFFFFFFF - lanes))                   # all negative
    w.append(0x80000000 + ((lanes * 37) % 64))
    w += list(rng.integers(0, 1 << 32, (200, 64), dtype=np.uint64))
    return _pad_waves(np.array(w, dtype=np.uint64).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def waves64():
    rng = np.random.default_rng(64)
    lanes = np.arange(64, dtype=np.uint64)
    w = [np.zeros(64, np.uint64), np.full(64, M64, np.uint64), lanes, np.full(64, 0xFFFFFFFF, np.uint64), np.full(64, 0xFFFFFFFF00000001, np.uint64),
         np.full(64, 1 << 63, np.uint64), np.full(64, 0x80000000, np.uint64)]
    for r in range(64):
        v = np.zeros(64, np.uint64); v[r] = np.uint64((GOLD64 + r) & M64); w.append(v)
    for r in range(64):                                      # the low halves sum to 2^32 exactly in lane r + 1: the carry starts there (r = 63: nowhere)
        v = np.full(64, 0xFFFFFFFF00000000, np.uint64); v[0] += np.uint64(0xFFFFFFFF - r); v[1:r + 2] += np.uint64(1); w.append(v)
    for W in (8, 16, 32):
        even = (lanes // W) % 2 == 0
        w.append(np.where(even, np.uint64(M64), lanes)); w.append(np.where(even, lanes << np.uint64(32), np.uint64(0xFFFFFFFF)))
    w += list(rng.integers(0, 1 << 64, (100, 64), dtype=np.uint64))                      # the running sum passes 2^64
    w += list(rng.integers(0, 1 << 32, (60, 64), dtype=np.uint64))                       # the low halves carry, in ever other lanes
    w += list(rng.integers(0, 1 << 33, (40, 64), dtype=np.uint64) << np.uint64(24))
    return _pad_waves(np.array(w, dtype=np.uint64))


def _rec32(w):
    return np.asarray(w, dtype=np.uint32).reshape(-1, 1)


@pytest.mark.parametrize("W", dm.WIDTHS)
def test_group_scans_and_reductions(lib, W):
    for b, op in enumerate(dm.OPS):
        w = waves32(dm.IDENT[op])
        _check(lib, "group_scan_incl", W, b, _rec32(w), dm.scan_incl(w, W, op), what=op)
        _check(lib, "group_reduce", W, b, _rec32(w), dm.reduce(w, W, op), what=op)
    w = waves32(0)
    _check(lib, "group_last", W, 0, _rec32(w), dm.group_last(w, W))
    _check(lib, "wg_sum", W, 0, _rec32(w), dm.reduce(w, W, "add"))
    _check(lib, "wg_max", W, 0, _rec32(w), dm.reduce(w, W, "max"))
    _check(lib, "wg_min", W, 0, _rec32(waves32(M32)), dm.reduce(waves32(M32), W, "min"))
    _check(lib, "wg_scan_excl", W, 0, _rec32(w), dm.scan_excl(w, W))


@pytest.mark.parametrize("W", dm.WIDTHS)
def test_group_scans_of_64_bits(lib, W):
    w = waves64()
    rec = dl.u64_words(w.reshape(-1))
    _check(lib, "group_scan_incl_add64", W, 0, rec, dl.u64_words(dm.scan_incl(w, W, "add", 64).reshape(-1)))
    _check(lib, "group_last64", W, 0, rec, dl.u64_words(dm.group_last(w, W, 64).reshape(-1)))
    _check(lib, "wg_sum64", W, 0, rec, dl.u64_words(dm.reduce(w, W, "add", 64).reshape(-1)))
    _check(lib, "wg_scan_excl64", W, 0, rec, dl.u64_words(dm.scan_excl(w, W, 64).reshape(-1)))


def test_lane_exchanges(lib):
    w = waves32(0)
    for d in (1, 2, 4, 8, 16, 32):
        _check(lib, "lane_xor", d, 0, _rec32(w), dm.lane_xor(w, d))
        _check(lib, "lane_xor_any", d, 0, _rec32(w), dm.lane_xor(w, d))


def test_wave_reductions(lib):
    w = waves32(0)
    _check(lib, "wave_max_u32", 0, 0, _rec32(w), dm.reduce(w, 64, "max"))
    _check(lib, "wave_max_i32", 0, 0, _rec32(w), dm.wave_max_i32(w))
    got = _check(lib, "wb_scan_excl", 0, 0, _rec32(w), np.stack([dm.scan_excl(w, 64).reshape(-1), dm.reduce(w, 64, "add").reshape(-1)], axis=1))
    assert got.shape[1] == 2
    v = np.concatenate([w.reshape(-1), np.arange(65536, dtype=np.uint32) * 0x00010001, np.arange(65536, dtype=np.uint32) << 8])
    v = v[:len(v) // 256 * 256]
    _check(lib, "wb_bytesum", 0, 0, _rec32(v), dm.bytesum(v))


@pytest.mark.parametrize("W", dm.WIDTHS)
def test_group_any(lib, W):
    p = np.zeros((68, 64), dtype=np.uint32)                  # every single lane, none, all, and a value that is no 0 / 1
    for r in range(64):
        p[r, r] = 1
    p[65] = 1
    p[66, 13] = 0x80000000
    p[67, ::W] = 2
    p = _pad_waves(p)
    _check(lib, "wg_any", W, 0, _rec32(p), dm.group_any(p, W))


@pytest.mark.parametrize("W", dm.WIDTHS)
def test_group_suffix_min(lib, W):
    lanes = np.arange(64, dtype=np.uint64)
    w = [3 * lanes + 5, 1000 - lanes, np.full(64, 7, np.uint64), np.full(64, M32, np.uint64), np.zeros(64, np.uint64)]
    for r in range(64):                                      # the minimum at every position
        v = 100 + lanes; v[r] = 1; w.append(v)
    for r in range(64):
        v = 100 + (63 - lanes); v[r] = 1; w.append(v)
    w = _pad_waves(np.concatenate([np.array(w, dtype=np.uint64).astype(np.uint32), waves32(M32)]))
    exp = dm.suffix_min_excl(w, W)
    assert (exp[:, W - 1::W] == M32).all(), "the last lane of each group"
    _check(lib, "wg_suffix_min_excl", W, 0, _rec32(w), exp)


# ---------------------------------------------------------------------------------------------------------------- SWAR arithmetic
@functools.lru_cache(maxsize=None)
def bytes_e1():
    """4 byte positions x 4 fills of the other three bytes x all 65,536 (x, y): the dwords w and b, (16, 65536) each"""
    rng = np.random.default_rng(11)
    x, y = np.divmod(np.arange(65536, dtype=np.uint32), 256)
    ws, bs = [], []
    for pos in range(4):
        keep = np.uint32(~(0xFF << (8 * pos)) & M32)
        for fw, fb in ((0, 0), (M32, M32), (0x80808080, 0x7F7F7F7F), (None, None)):
            fw = rng.integers(0, 1 << 32, 65536, dtype=np.uint32) if fw is None else np.uint32(fw)
            fb = rng.integers(0, 1 << 32, 65536, dtype=np.uint32) if fb is None else np.uint32(fb)
            ws.append((fw & keep) | (x << np.uint32(8 * pos))); bs.append((fb & keep) | (y << np.uint32(8 * pos)))
    return np.array(ws, dtype=np.uint32), np.array(bs, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def halves_e2():
    """both halves x the other half at its extremes x 13 y x all 65,536 differences: the dwords w and b"""
    rng = np.random.default_rng(12)
    d = np.arange(65536, dtype=np.uint32)
    ws, bs = [], []
    for y in [0, 1, 0x7FFF, 0x8000, 0xFFFF] + [int(v) for v in rng.integers(0, 65536, 8)]:
        t = (d + np.uint32(y)) & np.uint32(0xFFFF)
        for ow, ob in ((0, 0xFFFF), (0xFFFF, 0xFFFF)):        # the other half borrows (0 - 0xFFFF) and carries (0xFFFF + 0xFFFF) as hard as it can
            ws.append(t | np.uint32(ow << 16)); bs.append(np.full(65536, y | (ob << 16), np.uint32))
            ws.append((t << np.uint32(16)) | np.uint32(ow)); bs.append(np.full(65536, (y << 16) | ob, np.uint32))
    return np.array(ws, dtype=np.uint32).reshape(-1), np.array(bs, dtype=np.uint32).reshape(-1)


@functools.lru_cache(maxsize=None)
def pairs_wide(E):
    """E = 4, 8: the cross product of the six edge values, 100,000 random pairs and (E = 8) pairs whose low dwords borrow"""
    rng = np.random.default_rng(13 + E)
    w = 8 * E
    edge = [0, 1, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << w) - 1, (1 << w) - 2]
    t, b = [x for x in edge for _ in edge], [y for _ in edge for y in edge]
    if E == 8:
        hi = rng.integers(0, 1 << 32, (2, 2000), dtype=np.uint64)
        lo = np.sort(rng.integers(0, 1 << 32, (2, 2000), dtype=np.uint64), axis=0)       # t's low dword <= b's
        t += [int(v) for v in (hi[0] << np.uint64(32)) | lo[0]] + [5 << 32, 1 << 32]
        b += [int(v) for v in (hi[1] << np.uint64(32)) | lo[1]] + [(4 << 32) | M32, 1]
    t += [int(v) for v in rng.integers(0, 1 << w, 100000, dtype=np.uint64)]
    b += [int(v) for v in rng.integers(0, 1 << w, 100000, dtype=np.uint64)]
    k = len(t) // 1024 * 1024                                # whole dword quadruples, whole blocks (the cut takes random pairs)
    return np.array(t[:k], dtype=np.uint64), np.array(b[:k], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def sub4_cases(E):
    """(w, b) as bytes (n, 16) and the model's forward result"""
    if E == 1:
        w, b = (x.reshape(-1) for x in bytes_e1())
    elif E == 2:
        w, b = halves_e2()
    else:
        t, y = pairs_wide(E)
        w, b = t.astype("<u%d" % E).view(np.uint32), y.astype("<u%d" % E).view(np.uint32)
    w, b = w.reshape(-1, 4).view(np.uint8), b.reshape(-1, 4).view(np.uint8)
    return w, b, dm.sub4(w, b, E, False)


def _chunks(x):
    return np.ascontiguousarray(x).view(np.uint32).reshape(len(x), -1)


@pytest.mark.parametrize("E", dm.ELEMS)
def test_sub_and_zigzag_on_dwords(lib, E):
    w, b, z = sub4_cases(E)
    rec = np.concatenate([_chunks(w), _chunks(b)], axis=1)
    got = _check(lib, "pl_sub4", E, 0, rec, _chunks(z), what="forward")
    back = _check(lib, "pl_sub4", E, 1, np.concatenate([got, _chunks(b)], axis=1), _chunks(w), what="the inverse of the forward result")
    assert np.array_equal(back, _chunks(w))
    # every bit pattern is somebody's zigzag: the inverse on the raw operands too
    _check(lib, "pl_sub4", E, 1, rec, _chunks(dm.sub4(w, b, E, True)), what="inverse")


@pytest.mark.parametrize("E", dm.ELEMS)
def test_zigzag_of_elements(lib, E):
    """pl_zz / pl_unzz on numbers below 2^(8 E), and pl_sub4's forward value is pl_zz's on every element"""
    w, b, z = sub4_cases(E)
    t, y, zz = (dm.elems(x, E).reshape(-1).astype(np.uint64) for x in (w, b, z))
    if E == 1:                                               # (the 65,536 pairs once, not in every position)
        t, y, zz = t[:4 * 65536:4], y[:4 * 65536:4], zz[:4 * 65536:4]
    if E == 2:                                               # (the low halves of the five fixed y: all differences against each)
        t, y, zz = (x.reshape(13, 4, 65536, 2)[:5, 0, :, 0].reshape(-1) for x in (t, y, zz))
    k = len(t) // 256 * 256
    t, y, zz = t[:k], y[:k], zz[:k]
    rec = np.concatenate([dl.u64_words(t), dl.u64_words(y)], axis=1)
    _check(lib, "pl_zz", E, 0, rec, dl.u64_words(zz))
    _check(lib, "pl_unzz", E, 0, np.concatenate([dl.u64_words(zz), dl.u64_words(y)], axis=1), dl.u64_words(t))
    _check(lib, "pl_unzz", E, 0, rec, dl.u64_words(dm.unzz(t, y, E)))


def test_packed_additions(lib):
    w, b = (x.reshape(-1) for x in bytes_e1())
    _check(lib, "pp_add8x4", 0, 0, np.stack([w, b], axis=1), dm.add_lanes(w, b, 1))
    w, b = halves_e2()
    _check(lib, "pp_add16x2", 0, 0, np.stack([w, b], axis=1), dm.add_lanes(w, b, 2))


@functools.lru_cache(maxsize=None)
def prefix_chunks(E):
    rng = np.random.default_rng(20 + E)
    c = [np.full(16 * E, 0xFF, np.uint8), np.full(16 * E, 0x80, np.uint8), np.tile(np.array([0x80, 0x7F], np.uint8), 8 * E),
         np.tile(np.array([0x7F, 0x80], np.uint8), 8 * E), np.full(16 * E, 0x01, np.uint8), np.zeros(16 * E, np.uint8)]
    for k in range(16):                                      # one element of all ones; one 0xFF byte, at each place
        v = np.zeros(16 * E, np.uint8); v[k * E:(k + 1) * E] = 0xFF; c.append(v)
    for k in range(16 * E):
        v = np.zeros(16 * E, np.uint8); v[k] = 0xFF; c.append(v)
        v = np.full(16 * E, 0xFF, np.uint8); v[k] = 0; c.append(v)
    c = np.array(c, dtype=np.uint8)
    r = rng.integers(0, 256, (100000, 16 * E), dtype=np.uint8)
    r[:20000] |= 0x80                                        # carries almost everywhere
    c = np.concatenate([c, r])
    return c[:len(c) // 256 * 256]


@pytest.mark.parametrize("E", dm.ELEMS)
def test_prefix_sums_of_a_chunk(lib, E):
    c = prefix_chunks(E)
    words, total = dm.prefix(c, E)
    assert np.array_equal(total, dm.elems(words, E)[:, -1].astype(np.uint64)), "the total is the last prefix sum"
    _check(lib, "pp_prefix", E, 0, _chunks(c), np.concatenate([_chunks(words), dl.u64_words(total)], axis=1))


@pytest.mark.parametrize("E", dm.ELEMS)
def test_carry_into_a_chunk(lib, E):
    rng = np.random.default_rng(30 + E)
    w = 8 * E
    edge = [0, 1, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << w) - 1, (1 << w) - 2]
    if E == 1:                                               # 256 carries x 256 values in each byte of a dword, random bytes around it
        cv, val = np.divmod(np.arange(65536), 256)
        chunk = rng.integers(0, 256, (4, 65536, 16), dtype=np.uint8)
        for pos in range(4):
            chunk[pos, :, 5 * pos] = val                     # (dword pos, byte pos)
        chunk, c = chunk.reshape(-1, 16), np.tile(cv, 4).astype(np.uint64)
    elif E == 2:                                             # 65,536 carries; the six edges and a random element in both halves of a dword
        c = np.arange(65536, dtype=np.uint64)
        el = np.array([(edge + [0])[k % 7] for k in range(16)], dtype=np.uint16)
        chunk = np.tile(el, (65536, 1))
        chunk[:, 6::7] = rng.integers(0, 65536, (65536, 2), dtype=np.uint16)
        assert {(k % 7, k % 2) for k in range(16)} >= {(i, h) for i in range(6) for h in (0, 1)}
        chunk = chunk.view(np.uint8)
    else:
        c = np.array([x for x in edge for _ in edge] + [int(v) for v in rng.integers(0, 1 << w, 20444, dtype=np.uint64)], dtype=np.uint64)
        chunk = rng.integers(0, 1 << w, (len(c), 16), dtype=np.uint64)
        chunk[:36, :] = np.array([y for _ in edge for y in edge], dtype=np.uint64).reshape(36, 1)          # every edge plus every edge
        chunk = chunk.astype("<u%d" % E).view(np.uint8)
        if E == 4:                                           # the carry is taken mod 2^32
            c[1000:2000] |= np.uint64(0xABCD) << np.uint64(48)
    k = len(c) // 256 * 256
    chunk, c = chunk[:k], c[:k]
    _check(lib, "pp_carry", E, 0, np.concatenate([_chunks(chunk), dl.u64_words(c)], axis=1), _chunks(dm.carry(chunk, c, E)))


def test_carry_bits_above_the_element_are_dropped(lib):
    """pp_carry<1> and <2> take the carry mod 2^8 / 2^16"""
    rng = np.random.default_rng(33)
    for E in (1, 2):
        chunk = rng.integers(0, 256, (512, 16 * E), dtype=np.uint8)
        c = rng.integers(0, 1 << 64, 512, dtype=np.uint64)
        _check(lib, "pp_carry", E, 0, np.concatenate([_chunks(chunk), dl.u64_words(c)], axis=1), _chunks(dm.carry(chunk, c, E)))


@pytest.mark.parametrize("E", dm.ELEMS)
def test_byte_shuffles(lib, E):
    rng = np.random.default_rng(40 + E)
    c = np.concatenate([np.arange(16 * E, dtype=np.uint8).reshape(1, -1), 255 - np.arange(16 * E, dtype=np.uint8).reshape(1, -1),
                        rng.integers(0, 256, (1022, 16 * E), dtype=np.uint8)])
    planes = dm.deinterleave(c, E)
    assert planes[0, E - 1].tolist() == list(range(E - 1, 16 * E, E)), "byte k holds k: every byte names where it came from"
    got = _check(lib, "pl_deinterleave", E, 0, _chunks(c), _chunks(planes.reshape(len(c), -1)))
    back = _check(lib, "pl_interleave", E, 0, got, _chunks(c), what="of the deinterleaved chunk")
    assert np.array_equal(back, _chunks(c))
    # and the other way round: c as E planes
    z = dm.interleave(c, E)
    got = _check(lib, "pl_interleave", E, 0, _chunks(c), _chunks(z))
    _check(lib, "pl_deinterleave", E, 0, got, _chunks(c), what="of the interleaved planes")


def _prev_case(E, S, run_start):
    """payload byte k holds k mod 251; chunks at every offset 0 .. 15 from a 16-byte boundary.  With run_start the first one lies at the very start
    of the payload, behind the records (no word of which is 0): what is in front of a chunk must not reach the result"""
    n = 512
    payload = (np.arange(16 * 8 + 64 + 16 + 64) % 251).astype(np.uint8)
    front = 0 if run_start else 64
    offs = np.array([front + 16 * ((k // 16) % 4) + k % 16 for k in range(n)], dtype=np.uint32)
    if run_start:
        offs[64:80] = np.arange(16)
        offs[0] = 0
    rec = (offs + 4 * n).astype(np.uint32)
    exp = np.array([dm.prev(payload, int(o), E, S, run_start) for o in offs], dtype=np.uint8)
    return rec.reshape(-1, 1), payload, _chunks(exp)


@pytest.mark.parametrize("E", dm.ELEMS)
def test_predecessors_of_a_chunk(lib, E):
    for rs in (0, 1):
        rec, payload, exp = _prev_case(E, 1, bool(rs))
        _check(lib, "pp_prev", E, rs, rec, exp, payload=payload, what="runStart %d" % rs)
        for S in dm.STRIDES:
            rec, payload, exp = _prev_case(E, S, bool(rs))
            _check(lib, "ps_prev", E, S + 16 * rs, rec, exp, payload=payload, what="stride %d runStart %d" % (S, rs))


def test_a_chunk_outside_the_payload_is_refused_by_the_kernel(lib):
    """the wrapper's own bounds check (it keeps a wrong offset of a test from reading outside the buffer): such a record stores the refusal mark"""
    n = 512
    payload = np.arange(256, dtype=np.uint8)
    rec = np.full((n, 1), 4 * n + 64, dtype=np.uint32)
    rec[0] = 4 * n + 256 - 15                                # the chunk ends behind the buffer
    rec[1] = 4 * n                                           # no run start, and nothing in front inside the payload
    rec[2] = 0
    got = dl.run(lib, "pp_prev", 1, 0, rec, 4, 64, payload)
    assert (got[:3] == 0xBAD0BAD0).all() and np.array_equal(got[3].view(np.uint8), payload[63:79])


@pytest.mark.parametrize("E", dm.ELEMS)
def test_registers_of_a_chunk(lib, E):
    rng = np.random.default_rng(50 + E)
    c = np.concatenate([np.arange(16 * E, dtype=np.uint8).reshape(1, -1), np.full((1, 16 * E), 0xFF, np.uint8), rng.integers(0, 256, (510, 16 * E), dtype=np.uint8)])
    el = dm.elems(c, E).astype(np.uint64)
    mask = np.tile(np.array([(1 << min(8 * E, 32)) - 1, M32 if E == 8 else 0], dtype=np.uint32), 16)       # (above the element: not kept clean)
    x = _check(lib, "ps_unpack", E, 0, _chunks(c), dl.u64_words(el), mask=mask)
    back = _check(lib, "ps_pack", E, 0, x, _chunks(c), what="of the unpacked chunk")
    assert np.array_equal(back, _chunks(c))
    # garbage above the element (and, below 8 bytes, above the register): dropped
    dirty = el | (rng.integers(0, 1 << 64, el.shape, dtype=np.uint64) << np.uint64(8 * E)) if E < 8 else el
    _check(lib, "ps_pack", E, 0, dl.u64_words(dirty), _chunks(c), what="with bits above the element")


@pytest.mark.parametrize("S", dm.STRIDES)
def test_rotation_by_a_lane_dependent_amount(lib, S):
    rng = np.random.default_rng(60 + S)
    lanes = np.arange(512, dtype=np.uint64) % 64
    for T in (4, 8):
        v = 16 * lanes.reshape(-1, 1) + np.arange(S, dtype=np.uint64)
        r = (lanes % S).astype(np.uint32)                    # every (S, r) pair in every wave
        assert set(r[:64].tolist()) == set(range(S))
        v2 = rng.integers(0, 1 << (8 * T), (512, S), dtype=np.uint64)
        r2 = rng.integers(0, S, 512, dtype=np.uint32)
        vv, rr = np.concatenate([v, v2]), np.concatenate([r, r2])
        rec = np.concatenate([dl.u64_words(vv), rr.reshape(-1, 1)], axis=1)
        _check(lib, "ps_rotate", S, T, rec, dl.u64_words(dm.rotate(vv, rr, S)), what="T of %d bytes" % T)


# ---------------------------------------------------------------------------------------------------------------- index logic
_share_range = functools.lru_cache(maxsize=None)(dm.share_range)


def _fill(items, least=512):
    """the list repeated up to whole blocks of 256, `least` items at least"""
    want = max(least, -(-len(items) // 256) * 256)
    return (items * -(-want // len(items)))[:want]


def test_plane_sizes_and_starts_on_the_device(lib):
    sizes = list(range(0, 40)) + [32767, 32768, 32769, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 63) - 9, (1 << 63) - 1, 1 << 63]
    rec = [(n, p, E) for E in dm.ELEMS for n in sizes for p in range(E)]
    rec += rec[:-len(rec) % 256]
    r = np.array([[n & M32, n >> 32, p, E] for n, p, E in rec], dtype=np.uint32)
    _check(lib, "pl_size", 0, 0, r, dl.u64_words(np.array([dm.pl_size(n, p, E) for n, p, E in rec], dtype=np.uint64)))
    _check(lib, "pl_start", 0, 0, r, dl.u64_words(np.array([dm.pl_start(n, p, E) for n, p, E in rec], dtype=np.uint64)))


@pytest.mark.parametrize("E", dm.ELEMS)
def test_share_of_a_tile(lib, E):
    T = int(lib.FSEHIP_devtest_tile())
    assert T == 32768
    cases = []                                               # (s0, n, lo, alignAddr, alignStride)
    tensors = [(3 * T + r, n) for r in (0, 1, 15, 16, T - 1) for n in sorted({1, E - 1, E, 15 * E, 16 * E, 16 * E + 1, T - 1, T, T + E + 1, 3 * T + 5} - {0})]
    for s0, n in tensors:
        for lo in range(s0 // T * T, s0 + n, T):             # every tile the tensor touches
            for addr in range(16):
                for stride in sorted({0, 1, E}):
                    cases.append((s0, n, lo, addr + (7 << 40), stride))
    pad = -len(cases) % 256
    rows = cases + cases[:pad]
    rec = np.array([[s0 & M32, s0 >> 32, n & M32, n >> 32, lo & M32, lo >> 32, a & M32, a >> 32, st] for s0, n, lo, a, st in rows], dtype=np.uint32)
    got = None
    for threads in BLOCKS:
        g = dl.words_u64(dl.run(lib, "pl_share", E, 0, rec, 10, threads))
        assert got is None or np.array_equal(g, got)
        got = g
    cover = {}
    for (s0, n, lo, addr, stride), (e0, eb, et, e1, nch) in zip(cases, got.tolist()):
        tag = (s0, n, lo, addr & 15, stride, e0, eb, et, e1, nch)
        rng_ = _share_range(s0, n, lo, T, E)
        assert (e0, e1) == rng_ if rng_ else e0 == e1, tag
        assert e0 <= eb <= et <= e1 and et - eb == 16 * nch, tag
        assert et == eb or et * E <= n, ("a chunk holds whole elements only", tag)
        assert eb - e0 <= 15 and min(e1, n // E) - et < 16, ("head and tail are shorter than a chunk", tag)
        clamped = eb == e1
        if stride and addr % stride == 0 and not clamped:
            assert (addr + eb * stride) % 16 == 0, ("the chunks start on a 16-byte boundary", tag)
            assert all((addr + e * stride) % 16 for e in range(e0, eb)), ("... the first one", tag)
        if stride == 0:
            assert eb == e0, tag
        cover.setdefault((s0, n, addr, stride), []).append((e0, e1))
    for (s0, n, addr, stride), parts in cover.items():
        parts = sorted(p for p in parts if p[0] != p[1])
        assert parts[0][0] == 0 and parts[-1][1] == -(-n // E) and all(a[1] == b[0] for a, b in zip(parts, parts[1:])), (s0, n, parts)


def test_work_mapping(lib):
    T, TL = 32768, 15
    rng = np.random.default_rng(70)
    arrays = [[0, 0, 100, 100, 5 * T + 7, 5 * T + 9, 5 * T + 9, 6 * T, 9 * T + 1],             # empty tensors, many tiles, a shared tile
              [0], [T], [3 * T + 1, 3 * T + 1], [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, T - 1, T, T + 1], [0, 40 * T]]
    arrays.append(sorted(int(v) for v in rng.integers(0, 64 * T, 100)))
    for S in arrays:
        top = (S[-1] >> TL) + len(S) + 3
        w = list(range(top + 1)) + [1 << 31, 1 << 32, (1 << 63) + 5, M64]
        w = _fill(w)
        exp = [dm.find(S, q, TL) for q in w]
        e = np.array([[0, M64] if i is None else [1, i] for i in exp], dtype=np.uint64)
        _check(lib, "pl_find", len(S), 0, dl.u64_words(np.array(w, dtype=np.uint64)), dl.u64_words(e), payload=np.array(S, dtype=np.uint64), what=str(S[:9]))
    _check(lib, "pl_find", 0, 0, dl.u64_words(np.arange(512, dtype=np.uint64)), dl.u64_words(np.tile(np.array([0, M64], dtype=np.uint64), (512, 1))),
           payload=np.zeros(0, dtype=np.uint64), what="no tensor")
    # keys that do not decrease, with runs of equal ones: every key, its neighbours and the ends
    for keys in ([7], [3, 3, 5, 9], [0, 0, 0], sorted(int(v) for v in rng.integers(0, 1000, 37)), sorted(int(v) for v in rng.integers(0, 1 << 64, 64, dtype=np.uint64))):
        q = sorted({(k + d) & M64 for k in keys for d in (-1, 0, 1)} | {0, M64})
        q = _fill(q)
        _check(lib, "pl_last_le", len(keys), 0, dl.u64_words(np.array(q, dtype=np.uint64)), dl.u64_words(np.array([dm.last_le(keys, x) for x in q], dtype=np.uint64)),
               payload=np.array(keys, dtype=np.uint64), what=str(keys[:9]))
    # arrays that are not monotone: whatever comes back is an index below the count
    for nT in (1, 2, 7, 64, 100):
        for k in range(4):
            S = rng.integers(0, 1 << (16 + 12 * k), nT, dtype=np.uint64)
            w = rng.integers(0, 1 << (4 + 12 * k), 512, dtype=np.uint64)
            for threads in BLOCKS:
                got = dl.words_u64(dl.run(lib, "pl_find", nT, 0, dl.u64_words(w), 4, threads, S))
                assert ((got[:, 0] == 0) | (got[:, 1] < nT)).all() and (got[:, 0] <= 1).all()
                assert (got[got[:, 0] == 0][:, 1] == M64).all()
                got = dl.words_u64(dl.run(lib, "pl_last_le", nT, 0, dl.u64_words(w), 2, threads, S))
                assert (got[:, 0] < nT).all()


# ---------------------------------------------------------------------------------------------------------------- bit reader
OPC = {"read": 0, "fast": 1, "reload": 2}


@functools.lru_cache(maxsize=None)
def bit_scripts():
    """[(stream, steps, the statuses a reload of the script must meet or None)]"""
    rng = np.random.default_rng(80)
    out = []
    mix = [("read", 0), ("read", 1), ("fast", 1), ("reload", 0), ("read", 15), ("reload", 0), ("read", 16), ("reload", 0), ("read", 24), ("reload", 0),
           ("fast", 24), ("reload", 0), ("fast", 7), ("read", 0), ("reload", 0), ("read", 24), ("read", 24), ("reload", 0), ("read", 16), ("reload", 0)]
    for n in range(1, 25):
        for last in (0x01, 0x80, 0xFF, 0x00):
            s = rng.integers(0, 256, n, dtype=np.uint8); s[-1] = last
            out.append((s, mix, None))
    for lo, hi in ((1, 13), (13, 20), (20, 25)):             # read_fast of 1 .. 24 bits
        s = rng.integers(0, 256, 24, dtype=np.uint8); s[-1] |= 0x80
        out.append((s, [st for nb in range(lo, hi) for st in (("fast", nb), ("reload", 0))], None))
        s = rng.integers(0, 256, 24, dtype=np.uint8); s[-1] = 0x01
        out.append((s, [st for nb in range(lo, hi) for st in (("read", nb), ("reload", 0))], None))
    r16 = rng.integers(1, 256, 24, dtype=np.uint8)
    # reload in each of its states
    out.append((r16[:16], [("read", 24)] * 3 + [("reload", 0)], [dm.OVERFLOW]))                              # more than 64 bits used
    out.append((r16, [("read", 16), ("reload", 0)], [dm.UNFINISHED]))                                        # 8 bytes left at least
    out.append((r16[:12], [("read", 16), ("reload", 0)], [dm.UNFINISHED]))                                   # fewer left, enough of them
    out.append((r16[:10], [("read", 24), ("read", 8), ("reload", 0)], [dm.END_OF_BUFFER]))                   # fewer left, clamped
    out.append((r16[:8], [("read", 16), ("reload", 0)], [dm.END_OF_BUFFER]))                                 # nothing left, bits left
    s = r16[:8].copy(); s[-1] = 0x80
    out.append((s, [("read", 24), ("read", 24), ("read", 15), ("reload", 0)], [dm.COMPLETED]))               # nothing left, 64 bits used exactly
    out.append((r16[:3], [("read", 5), ("reload", 0)], [dm.END_OF_BUFFER]))
    s = r16.copy(); s[-1] = 0x80                                                                             # 191 bits, drained
    out.append((s, [("read", 16), ("reload", 0)] * 11 + [("read", 15), ("reload", 0)], [dm.UNFINISHED] * 2 + [None] * 9 + [dm.COMPLETED]))
    return out


def test_bit_reader(lib):
    scripts = bit_scripts()
    IN, OUT = TABLE[("bitreader", 0, 0)]
    rec, exp, mask = np.zeros((512, IN), np.uint32), np.zeros((512, OUT), np.uint32), np.zeros((512, OUT), np.uint32)
    assert len(scripts) <= 512
    for k in range(512):
        stream, steps, want = scripts[k % len(scripts)]
        raw = np.zeros(dm.BR_STREAM, np.uint8); raw[:len(stream)] = stream
        rec[k, 0], rec[k, 1] = len(stream), len(steps)
        rec[k, 2:2 + dm.BR_STREAM // 4] = raw.view(np.uint32)
        rec[k, 2 + dm.BR_STREAM // 4:2 + dm.BR_STREAM // 4 + len(steps)] = [OPC[op] | (nb << 8) for op, nb in steps]
        m, rows = dm.run_script([int(x) for x in stream], steps)
        ret = dm.init_return(m)
        exp[k, 0], exp[k, 1] = ret & M32, ret >> 32
        mask[k, :2] = M32
        seen = []
        for j, (v, at, used, win) in enumerate(rows):
            if j == 0:
                exp[k, 2:6] = [at, used, win & M32, win >> 32]; mask[k, 2:6] = M32
                continue
            o = 6 + 5 * (j - 1)
            exp[k, o:o + 5] = [0 if v is None else v, at, used, win & M32, win >> 32]
            mask[k, o:o + 5] = [0 if v is None else M32, M32, M32, M32, M32]
            if steps[j - 1][0] == "reload":
                seen.append(v)
        if want is not None:
            assert len(seen) == len(want) and all(w is None or w == s for w, s in zip(want, seen)), (k, seen, want)
    _check(lib, "bitreader", 0, 0, rec, exp, mask=mask)


def test_fse_step(lib):
    IN, OUT = TABLE[("fse_step", -1, 0)]
    for fast in (0, 1):
        rng = np.random.default_rng(90 + fast)
        rec, exp = np.zeros((512, IN), np.uint32), np.zeros((512, OUT), np.uint32)
        for k in range(512):
            n = (4, 8, 9, 24)[k % 4]
            steps = 8 if n == 4 else 16
            stream = rng.integers(0, 256, n, dtype=np.uint8); stream[-1] |= 0x80 >> (k % 8)
            nb = rng.integers(1 if fast else 0, 4, dm.FS_CELLS)
            cells = [(int(b) << 24) | (int(rng.integers(0, 256)) << 16) | int(rng.integers(0, dm.FS_CELLS - (1 << int(b)) + 1)) for b in nb]
            state = int(rng.integers(0, dm.FS_CELLS))
            raw = np.zeros(dm.BR_STREAM, np.uint8); raw[:n] = stream
            rec[k, :3] = [n, steps, state]
            rec[k, 3:3 + dm.BR_STREAM // 4] = raw.view(np.uint32)
            rec[k, 3 + dm.BR_STREAM // 4:] = cells
            exp[k, 0] = n
            for j, row in enumerate(dm.fse_steps([int(x) for x in stream], cells, state, steps)):
                exp[k, 2 + 5 * j:7 + 5 * j] = row
        _check(lib, "fse_step", fast, 0, rec, exp, what="fast %d" % fast)

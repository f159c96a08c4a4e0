"""k_huf_encode on streams of UNEQUAL size and on tables that are not the block's own -- every route of the kernel, told from the reference's output:
fixed tables (lengths 1..12, flat 8 bits, a third of the symbols without a code), blocks written quarter by quarter (stream k is segment k of
(n + 3) / 4 bytes) so that the stream sizes are known in advance, and a predictor that restates launch_huf_encode / k_huf_encode's choices (image
min(cap + 16, 30720) rounded up to 16; region a quarter of it rounded down to 16; region limit 8 * region - 64 bits; single pass only for regions of
1024 bytes or more; two passes through LDS, in two halves, or with global atomics) and asserts how often each route is met.  Results and bytes are
the compiled reference's throughout."""
import itertools

import numpy as np
import pytest
import torch

from oracle.oracle import huf_compress_bound, is_error

pytestmark = pytest.mark.gpu

IMG_MAX = 30720


# ------------------------------------------------------------------------------------------------------------------------------
#  tables
# ------------------------------------------------------------------------------------------------------------------------------
class Table:
    """a fixed code table and, where HUF_writeCTable gives it a header that the reference's HUF_readDTableX1 / X2 accept, that header: the blocks coded
    with it are then decoded on the device as well (run_4x)"""

    def __init__(self, ref, celt, msv, log):
        self.celt, self.msv, self.log = celt, msv, log
        self.nb = ((celt >> 16) & 0xFF).astype(np.int64)
        self.by_len = {int(L): np.nonzero(self.nb[:msv + 1] == L)[0].astype(np.uint8) for L in np.unique(self.nb[:msv + 1])}
        celt.setflags(write=False)
        h, hdr = ref.huf_write_ctable(256, celt, msv, log)
        self.header = None if is_error(h) else hdr[:h].copy()
        self.reads_x1 = self.header is not None and ref.huf_read_dtable_x1(self.header, 12)[0] == h
        self.reads_x2 = self.header is not None and ref.huf_read_dtable_x2(self.header, 12)[0] == h
        self.dtables = None

    def covers(self, block):
        """every symbol of the block has a code"""
        return bool((self.nb[block] > 0).all())

    def device_tables(self, hip):
        """the X1 and X2 decoding tables, built on the device from the header, once"""
        if self.dtables is None:
            row = torch.from_numpy(np.pad(self.header, (0, 8))[None, :].copy()).cuda()
            dt1, q1 = hip.huf_read_dtable_x1_batch(row, len(self.header), max_table_log=12)
            dt2, q2 = hip.huf_read_dtable_x2_batch(row, len(self.header), max_table_log=12)
            assert int(q1[0]) == len(self.header) and (not self.reads_x2 or int(q2[0]) == len(self.header))
            self.dtables = (dt1.contiguous(), dt2.contiguous())
        return self.dtables


@pytest.fixture(scope="module")
def tables(ref):
    """fib: a Fibonacci histogram limited to 12 (thirteen symbols: lengths 1..12, two symbols of 12 bits); flat: 256 symbols of 8 bits; holes: every third symbol
    without a code.  BIT_addBitsFast wants a clean value (lib/bitstream.h:208-217), so the entries of length 0 carry value 0, not the running
    number HUF_buildCTable leaves there."""
    fib = np.zeros(256, np.uint32)
    a, b = 1, 2
    for s in range(13):
        fib[s] = a
        a, b = b, a + b
    log, celt = ref.huf_build_ctable(fib, 12, 12)
    t_fib = Table(ref, celt, 12, log)
    assert log == 12 and sorted(t_fib.by_len) == list(range(1, 13)) and len(t_fib.by_len[12]) == 2
    assert t_fib.reads_x1 and t_fib.reads_x2, "the header of the Fibonacci table must read back: its blocks are decoded too"
    log, celt = ref.huf_build_ctable(np.full(256, 7, np.uint32), 255, 11)
    t_flat = Table(ref, celt, 255, log)
    assert log == 8 and list(t_flat.by_len) == [8] and t_flat.header is None      # (256 equal weights: HUF_writeCTable has no form for them, GENERIC)
    holes = np.array([0 if s % 3 == 2 else 1 + (s * 37) % 50 + (3000 if s < 4 else 0) for s in range(256)], np.uint32)
    log, celt = ref.huf_build_ctable(holes, 255, 11)
    celt = np.where((celt >> 16) & 0xFF, celt, 0).astype(np.uint32)
    t_holes = Table(ref, celt, 255, log)
    assert len(t_holes.by_len[0]) == 85 and min(L for L in t_holes.by_len if L) <= 3
    return {"fib": t_fib, "flat": t_flat, "holes": t_holes}


def segment(table, q, length, rng):
    """q symbols of one code length"""
    return rng.choice(table.by_len[length], q)


def segment_of_bits(table, q, bits, rng):
    """q symbols whose codes total `bits` bits: two neighbouring lengths, shuffled"""
    a, r = divmod(bits, q)
    assert 1 <= a and (a + 1 <= 12 or r == 0), (q, bits)
    seg = np.concatenate([rng.choice(table.by_len[a], q - r), rng.choice(table.by_len[a + 1], r) if r else np.zeros(0, np.uint8)])
    rng.shuffle(seg)
    return seg.astype(np.uint8)


def quarters(n):
    q = (n + 3) // 4
    return [q, q, q, n - 3 * q]


def block_of(table, n, lengths, rng):
    return np.concatenate([segment(table, q, L, rng) for q, L in zip(quarters(n), lengths)]).astype(np.uint8)


def stream_bits(table, block):
    n = len(block)
    q = (n + 3) // 4
    return [int(table.nb[block[k * q:min((k + 1) * q, n)]].sum()) for k in range(4)]


# ------------------------------------------------------------------------------------------------------------------------------
#  the route predictor
# ------------------------------------------------------------------------------------------------------------------------------
def image_bytes(cap):
    return (min(cap + 16, IMG_MAX) + 15) & ~15


def route(cap, r, out, bits, dst_addr):
    """the route k_huf_encode must take for a 4-stream block: from the reference's result `r` and bytes `out` (jump table, total), the capacity and the
    address of the destination row; `bits` (the code bits per stream, from the table and the source) only settle a stream that ends within a byte of
    its region's limit.  Returns (route, number of regions that overflow in the single-pass attempt)"""
    if r == 0:
        return "fail", 0
    img = image_bytes(cap)
    region = (img // 4) & ~15
    sizes = [int(out[0]) | int(out[1]) << 8, int(out[2]) | int(out[3]) << 8, int(out[4]) | int(out[5]) << 8]
    sizes.append(r - 6 - sum(sizes))
    assert all(s == (b + 8) >> 3 for s, b in zip(sizes, bits)), (sizes, bits)
    over = 0
    if region >= 1024:
        for s, b in zip(sizes, bits):
            assert 8 * (s - 1) <= b <= 8 * s - 1
            over += b > 8 * region - 64
        if over == 0:
            return "single", 0
    lead = dst_addr & 3
    if ((lead + r + 3) >> 2) * 4 <= img:
        return "lds", over
    start2 = 6 + sizes[0] + sizes[1]
    if start2 + 8 <= img and (r - start2) + 8 <= img:
        return "halves", over
    return "global", over


ROUND_TRIPS = {}        # test -> blocks decoded back to their source (counted from the reference's results)


def run_4x(hip, ref, table, blocks, cap, what, counts=None):
    """blocks of one size through HUF_compress4X_usingCTable_batch with one shared table; everything against the reference; returns the routes.
    Where the table's header reads back (in the reference) and every symbol of a block has a code, what the device wrote is decoded by the device's
    4X1 and 4X2 decoders and must be the source"""
    n = len(blocks[0])
    src = torch.from_numpy(np.stack(blocks)).cuda()
    ct = torch.from_numpy(table.celt.view(np.int32).copy()).cuda()[None, :]
    dst, res = hip.huf_compress4x_using_ctable_batch(src, ct, dst_capacity=cap, shared_table=True)
    dst_h, res_h = dst.cpu().numpy(), res.cpu().numpy()
    routes = []
    for b, blk in enumerate(blocks):
        r, out = ref.huf_compress4x_using_ctable(blk, table.celt, cap)
        assert not is_error(r) and res_h[b] == r, (what, b, res_h[b], r)
        if r:
            assert (dst_h[b][:r] == out[:r]).all(), (what, b, r, np.nonzero(dst_h[b][:r] != out[:r])[0][:8])
        routes.append(route(cap, r, out, stream_bits(table, blk), dst.data_ptr() + b * dst.stride(0)))
    back = [b for b, (rt, _) in enumerate(routes) if rt != "fail" and table.reads_x1 and table.covers(blocks[b])]
    if back:
        dt1, dt2 = table.device_tables(hip)
        idx = torch.tensor(back, device="cuda")
        comp, sizes = dst[idx].contiguous(), res[idx].contiguous()
        for dt, name, built in ((dt1, "huf_decompress4x1_using_dtable_batch", True), (dt2, "huf_decompress4x2_using_dtable_batch", table.reads_x2)):
            if not built:
                continue
            got, dres = getattr(hip, name)(comp, sizes, dt, n, max_table_log=12, shared_table=True)
            assert bool((dres == n).all()) and torch.equal(got[:, :n], src[idx]), (what, name, dres.cpu().numpy()[:8])
        key = what if isinstance(what, str) else what[0]
        ROUND_TRIPS[key] = ROUND_TRIPS.get(key, 0) + len(back)
    if counts is not None:
        for rt, _ in routes:
            counts[rt] = counts.get(rt, 0) + 1
    return routes, dst, res


def subsets_blocks(table, n, long_len, short_len, rng, tail_only=False):
    """one block per subset of the four streams made long (all 16), the rest short.  tail_only: the long symbols fill only the part of a segment that
    is emitted AFTER its first 4096 symbols (the segment's front), the rest of a long segment has 4-bit symbols"""
    blocks = []
    for mask in range(16):
        segs = []
        for k, q in enumerate(quarters(n)):
            if not (mask >> k) & 1:
                segs.append(segment(table, q, short_len, rng))
            elif tail_only:
                segs.append(np.concatenate([segment(table, q - 4096, long_len, rng), segment(table, 4096, 4, rng)]))
            else:
                segs.append(segment(table, q, long_len, rng))
        blocks.append(np.concatenate(segs).astype(np.uint8))
    return blocks


def test_some_regions_overflow_small_shape(hip, ref, tables):
    """n = 4000, capacity 4200: the image is 4224 bytes, a region 1056, its limit 1048.  Every subset of the streams made long, the rest at one bit per
    symbol: with 1000 x 12 bits = 1500 bytes per long stream, and -- because three such streams no longer fit the capacity, where the reference
    returns 0 -- with 1000 x 10 bits = 1250 bytes as well.  Wherever some but not all regions overflow, the single-pass attempt is abandoned with
    its regions partly written and the block goes through the two-pass path with everything still in LDS."""
    ROUND_TRIPS.pop("subsets", None)
    assert image_bytes(4200) == 4224 and (4224 // 4) & ~15 == 1056
    rng = np.random.default_rng(41)
    t = tables["fib"]
    counts = {}
    for long_len, least in ((12, 10), (10, 14)):
        blocks = subsets_blocks(t, 4000, long_len, 1, rng)
        routes, _, _ = run_4x(hip, ref, t, blocks, 4200, ("subsets", long_len), counts)
        partial = sum(rt == "lds" and 0 < over < 4 for rt, over in routes)
        assert partial >= least, (long_len, partial, routes)
        assert routes[0] == ("single", 0) and routes[15][0] == "fail"
    assert counts["single"] >= 2 and counts["fail"] >= 6, counts
    assert ROUND_TRIPS["subsets"] >= 11 + 15, ROUND_TRIPS                     # every block the reference does not give up on was decoded


def test_overflow_in_a_later_tile(hip, ref, tables):
    """n = 32768, default capacity: regions of 7680 bytes.  All subsets again; the long streams are 8192 x 12 bits (12288 bytes: more than two of
    them exceed the capacity), 8192 x 9 bits (9216 bytes), and, third batch, 4096 symbols of 4 bits emitted first and 4096 of 12 bits behind them:
    2048 + 6144 bytes, so the region overflows only in the stream's second tile.  Four such streams total more than the image: two halves."""
    ROUND_TRIPS.pop("later tile", None)
    cap = huf_compress_bound(32768)
    assert image_bytes(cap) == IMG_MAX and (IMG_MAX // 4) & ~15 == 7680 and 2048 < 7672 < 2048 + 6144
    rng = np.random.default_rng(42)
    t = tables["fib"]
    for long_len, tail_only, least, last in ((12, False, 10, ("fail", 0)), (9, False, 14, ("fail", 0)), (12, True, 14, ("halves", 4))):
        blocks = subsets_blocks(t, 32768, long_len, 1, rng, tail_only)
        routes, _, _ = run_4x(hip, ref, t, blocks, cap, ("later tile", long_len, tail_only))
        partial = sum(rt == "lds" and 0 < over < 4 for rt, over in routes)
        assert partial >= least, (long_len, tail_only, partial, routes)
        assert routes[0] == ("single", 0) and routes[15] == last, (routes[0], routes[15])
    assert ROUND_TRIPS["later tile"] >= 11 + 15 + 16, ROUND_TRIPS


def test_whole_rows_of_twelve_bit_codes(hip, ref, tables):
    """sixteen 12-bit codes per lane = four 48-bit chunks, the stated limit of or_bits: n = 4 * 1024 and 4 * 1024 + 3 through the 4X form, the 1X batch
    form (four waves per block) and the single-block 1X call (one wave)"""
    ROUND_TRIPS.pop("12-bit rows", None)
    rng = np.random.default_rng(43)
    t = tables["fib"]
    for n in (4096, 4099):
        blocks = [segment(t, n, 12, rng).astype(np.uint8) for _ in range(3)]
        routes, _, _ = run_4x(hip, ref, t, blocks, 8000, ("12-bit rows", n))
        assert all(rt == ("single", 0) for rt in routes), routes
        assert ROUND_TRIPS["12-bit rows"] >= 3
        src = torch.from_numpy(np.stack(blocks)).cuda()
        ct = torch.from_numpy(t.celt.view(np.int32).copy()).cuda()[None, :]
        dst, res = hip.huf_compress1x_using_ctable_batch(src, ct, dst_capacity=8000, shared_table=True)
        dst_h, res_h = dst.cpu().numpy(), res.cpu().numpy()
        for b, blk in enumerate(blocks):
            r, out = ref.huf_compress1x_using_ctable(blk, t.celt, 8000)
            assert r == (12 * n + 8) >> 3 and res_h[b] == r and (dst_h[b][:r] == out[:r]).all(), (n, b, res_h[b], r)
            rg, og = hip.huf_compress1x_using_ctable(blk, t.celt, 8000)
            assert rg == r and (og[:r] == out[:r]).all(), (n, b, "single-block call")


def test_flat_table_fills_every_region_alike(hip, ref, tables):
    """the flat 8-bit table: four equal streams that just fit their regions (4096 bytes: one pass), and four that all overflow them (32 KiB: the total
    exceeds the image as well, so two halves) -- the equal-streams ends of the routes above"""
    rng = np.random.default_rng(48)
    t = tables["flat"]
    for n, want in ((4096, ("single", 0)), (32768, ("halves", 4))):
        blocks = [rng.integers(0, 256, n).astype(np.uint8) for _ in range(3)]
        routes, _, _ = run_4x(hip, ref, t, blocks, huf_compress_bound(n), ("flat", n))
        assert routes == [want] * 3, routes


def test_symbols_without_a_code(hip, ref, tables):
    """HUF_CElt entries of length 0 in runs and singly, a whole row of them, a whole stream of them (the stream is then just the end mark), 4X and 1X"""
    rng = np.random.default_rng(44)
    t = tables["holes"]
    coded = np.concatenate([t.by_len[L] for L in t.by_len if L])
    none = t.by_len[0]
    blocks = []
    for n in (16384, 16387, 5000):
        q = (n + 3) // 4
        x = rng.choice(coded, n).astype(np.uint8)
        x[rng.choice(n, n // 9, replace=False)] = rng.choice(none, n // 9)                       # singly
        for _ in range(12):                                                                     # runs
            at, ln = int(rng.integers(0, n - 40)), int(rng.integers(2, 40))
            x[at:at + ln] = rng.choice(none, ln)
        blocks.append(x.copy())
        y = x.copy(); y[q:2 * q] = rng.choice(none, q)                                          # stream 1: nothing but the end mark
        blocks.append(y)
        z = x.copy(); z[3 * q:] = rng.choice(none, n - 3 * q)                                    # the last stream likewise
        z[100:100 + min(2100, q - 200)] = rng.choice(none, min(2100, q - 200))                   # and more than two rows of stream 0 in one piece
        blocks.append(z)
    for n in (16384, 16387, 5000):
        group = [b for b in blocks if len(b) == n]
        routes, _, _ = run_4x(hip, ref, t, group, 2 * n, ("no code", n))                         # (most of this table's codes are longer than 8 bits)
        assert all(rt != "fail" for rt, _ in routes), routes
        r1, out1 = ref.huf_compress4x_using_ctable(group[1], t.celt, 2 * n)
        assert r1 > 0 and (int(out1[2]) | int(out1[3]) << 8) == 1, "stream 1 is the end mark alone"
        src = torch.from_numpy(np.stack(group)).cuda()
        ct = torch.from_numpy(t.celt.view(np.int32).copy()).cuda()[None, :]
        dst, res = hip.huf_compress1x_using_ctable_batch(src, ct, dst_capacity=2 * n, shared_table=True)
        dst_h, res_h = dst.cpu().numpy(), res.cpu().numpy()
        for b, blk in enumerate(group):
            r, out = ref.huf_compress1x_using_ctable(blk, t.celt, 2 * n)
            assert r > 0 and res_h[b] == r and (dst_h[b][:r] == out[:r]).all(), (n, b, res_h[b], r)
    only = rng.choice(none, 4096).astype(np.uint8)                                               # nothing has a code: four end marks
    routes, dst, res = run_4x(hip, ref, t, [only], huf_compress_bound(4096), "no code at all")
    assert int(res.cpu().numpy()[0]) == 6 + 4


def first_failing_stream(ref, table, block, cap):
    """which stream the reference's HUF_compress4X_usingCTable gives up at, from the reference alone: its own 1X call on every segment with the room
    that is left (lib/huf_compress.c:564-601); None when all four fit"""
    n = len(block)
    q = (n + 3) // 4
    op = 6
    for k in range(4):
        room = cap - op
        r, _ = ref.huf_compress1x_using_ctable(block[k * q:min((k + 1) * q, n)], table.celt, room) if room > 0 else (0, None)
        if r == 0:
            return k
        op += r
    return None


def test_capacity_failure_at_every_stream(hip, ref, tables):
    """streams of four distinct sizes in all 24 orders; around the smallest capacity that lets stream k through (BIT_closeCStream's rule, once per
    stream): -1, 0, +1, +8, +9.  One launch per capacity over all 24 blocks; results, and bytes where there are any, of the reference"""
    ROUND_TRIPS.pop("capacity", None)
    rng = np.random.default_rng(45)
    t = tables["fib"]
    n = 4096
    blocks = [block_of(t, n, perm, rng) for perm in itertools.permutations((1, 4, 8, 12))]
    caps = set()
    for blk in blocks:
        op = 6
        for bits in stream_bits(t, blk):
            edge = op + ((bits + 1) >> 3) + 9                      # the smallest capacity at which this stream passes
            caps |= {edge + d for d in (-1, 0, 1, 8, 9)}
            op += (bits + 8) >> 3
    position = {0: 0, 1: 0, 2: 0, 3: 0, None: 0}
    for cap in sorted(caps):
        routes, _, res = run_4x(hip, ref, t, blocks, cap, ("capacity", cap))
        for blk, (rt, _) in zip(blocks, routes):
            k = first_failing_stream(ref, t, blk, cap)
            assert (k is None) == (rt != "fail"), (cap, k, rt)
            position[k] += 1
    assert min(position.values()) >= 24, position
    assert ROUND_TRIPS["capacity"] == position[None] >= 30, (ROUND_TRIPS, position)


def test_halves_against_global_atomics(hip, ref, tables):
    """40 KiB and 48 KiB blocks, a capacity far above the image: the two-halves route needs start[2] + 8 <= image and total - start[2] + 8 <= image.
    Blocks on both sides of both bounds (exactly at it, one byte over), their rows at all four byte alignments (an odd row stride)"""
    ROUND_TRIPS.pop("halves", None)
    rng = np.random.default_rng(46)
    t = tables["fib"]
    cap = 65536 + 1 - (hip.guard & 1)                              # capacity + the binding's guard bytes: an odd row stride
    for n in (40960, 49152):
        q = n // 4
        kinds = []
        for s01, s23 in ((IMG_MAX - 8 - 6, 9000), (IMG_MAX - 8 - 6 + 1, 9000), (9000, IMG_MAX - 8), (9000, IMG_MAX - 8 + 1)):
            sizes = (s01 // 2, s01 - s01 // 2, s23 // 2, s23 - s23 // 2)
            kinds.append([8 * s - 4 for s in sizes])                # bits per stream: the stream then takes s bytes with its end mark
        blocks = [np.concatenate([segment_of_bits(t, q, b, rng) for b in kinds[row // 4]]) for row in range(16)]
        routes, dst, _ = run_4x(hip, ref, t, blocks, cap, ("halves", n))
        assert dst.stride(0) % 2 == 1
        assert [rt for rt, _ in routes] == ["halves"] * 4 + ["global"] * 4 + ["halves"] * 4 + ["global"] * 4, routes
        assert {(dst.data_ptr() + r * dst.stride(0)) & 3 for r in range(4)} == {0, 1, 2, 3}
    assert ROUND_TRIPS["halves"] == 32, ROUND_TRIPS


def test_foreign_tables_and_round_trip(hip, ref):
    """64 blocks of 4097 bytes from three generators, block b coded with the table of block (b + 1) % 64 (every table gives every symbol a code), 4X and
    1X against the reference; and what the device wrote decoded by the device's 4X1 and 4X2 decoders wherever the table's header reads back"""
    from oracle.oracle import Oracle
    orc = Oracle()
    rng = np.random.default_rng(47)
    n, nb = 4097, 64
    blocks = []
    for b in range(nb):
        if b % 3 == 0:
            blocks.append(orc.probagen_batch((20, 50, 5)[b % 9 // 3], 1, n, 900 + b)[0])
        elif b % 3 == 1:
            blocks.append(rng.integers(0, 8 << (b % 5), n).astype(np.uint8))
        else:
            blocks.append(np.minimum(rng.geometric(0.02 + 0.01 * (b % 7), n) - 1, 255).astype(np.uint8))
    tabs, hdrs = [], []
    for b in range(nb):
        cnt = np.bincount(blocks[b], minlength=256).astype(np.uint32) + 1
        log, celt = ref.huf_build_ctable(cnt, 255, 11)
        h, hdr = ref.huf_write_ctable(256, celt, 255, log)
        assert not is_error(log) and not is_error(h) and ((celt >> 16) & 0xFF).min() >= 1
        tabs.append(celt); hdrs.append(hdr[:h].copy())
    foreign = [tabs[(b + 1) % nb] for b in range(nb)]
    src = torch.from_numpy(np.stack(blocks)).cuda()
    ct = torch.from_numpy(np.stack(foreign).view(np.int32)).cuda()
    cap = huf_compress_bound(n)
    d4, r4 = hip.huf_compress4x_using_ctable_batch(src, ct)
    d1, r1 = hip.huf_compress1x_using_ctable_batch(src, ct)
    d4_h, r4_h, d1_h, r1_h = d4.cpu().numpy(), r4.cpu().numpy(), d1.cpu().numpy(), r1.cpu().numpy()
    for b in range(nb):
        r, out = ref.huf_compress4x_using_ctable(blocks[b], foreign[b], cap)
        assert r4_h[b] == r and (d4_h[b][:r] == out[:r]).all(), ("4X", b, r4_h[b], r)
        r, out = ref.huf_compress1x_using_ctable(blocks[b], foreign[b], cap)
        assert r1_h[b] == r and (d1_h[b][:r] == out[:r]).all(), ("1X", b, r1_h[b], r)
    # round trip on the device
    hbuf = np.zeros((nb, 256), np.uint8)
    for b in range(nb):
        h = hdrs[(b + 1) % nb]
        hbuf[b, :len(h)] = h
    hsz = torch.tensor([len(hdrs[(b + 1) % nb]) for b in range(nb)], dtype=torch.int64, device="cuda")
    d_h = torch.from_numpy(hbuf).cuda()
    dt1, q1 = hip.huf_read_dtable_x1_batch(d_h, hsz, max_table_log=12)
    dt2, q2 = hip.huf_read_dtable_x2_batch(d_h, hsz, max_table_log=12)
    q1_h, q2_h = q1.cpu().numpy(), q2.cpu().numpy()
    coded = [b for b in range(nb) if ref.huf_compress4x_using_ctable(blocks[b], foreign[b], cap)[0] > 0]
    for reader, q_h, dt, fn in ((ref.huf_read_dtable_x1, q1_h, dt1, hip.huf_decompress4x1_using_dtable_batch),
                                (ref.huf_read_dtable_x2, q2_h, dt2, hip.huf_decompress4x2_using_dtable_batch)):
        good = []                                                                # blocks that qualify, by the reference alone
        for b in range(nb):
            e = reader(hdrs[(b + 1) % nb], 12)[0]
            assert q_h[b] == (e if not is_error(e) else e - (1 << 64)), (fn.__name__, b, q_h[b], e)
            if not is_error(e) and b in coded:
                good.append(b)
        assert len(good) >= 30, (fn.__name__, len(good))
        ok = torch.tensor(good, device="cuda")
        out, res = fn(d4[ok].contiguous(), r4[ok].contiguous(), dt[ok].contiguous(), n, max_table_log=12)
        assert bool((res == n).all()) and torch.equal(out[:, :n], src[ok]), fn.__name__

"""A corpus that lands on every route and hand-over of the 16-bit-symbol coder (csrc/fse_u16.hip, csrc/fse_u16_decode.hip) on purpose, each
block labelled with what it reaches.  The labels come from the route model (scripts/sim/u16_codec_sim.py), never from the device.
tests/test_u16_corpus.py checks on the CPU that every label is reached, that the model computes what the compiled reference computes and that
the corpus tells the listed broken rule sets from the kernels' own; tests/test_gpu_u16_paths.py runs the corpus on the device against the
compiled reference.  Everything is seeded and built from the reference's own parts (FSE_buildCTableU16, FSE_compressU16_usingCTable,
FSE_compressU16, FSE_readNCount); headers of hand-made tables come from `_write_ncount` below, checked against the reference's writer
wherever that one applies.

How the decoder's boundaries are hit exactly: with a table in which every symbol costs a fixed number of bits the payload holds exactly
sum(costs) + tableLog bits in front of the end mark, so the unread bits B after the state read are the sum of the costs:
  * flat<k>: 2^k symbols of count 1 at table log k (k = 5 .. 8): k bits each (833 = 7 * 119, 832 = 8 * 104, 112 = 7 * 16);
  * nb12: table log 12, 256 (or 286) symbols of count 1 and one unused symbol with the rest of the table: 12 bits each, 48 an iteration;
  * mix11 (table log 11; counts 1 / 2 -> 11 / 10 bits) and mix12 (table log 12; counts 1 / 2 / 4 -> 12 / 11 / 10 bits) where a value is
    no multiple of one cost: 113 = 3 * 11 + 8 * 10 = 3 * 12 + 7 * 11, and 65 = 5 * 11 + 10 behind a long phase of 64 twelve-bit symbols
    (833 = 768 + 65).
Not reachable, with reasons: `UNREACHABLE` (the model's list and what building the corpus added).
"""
import importlib.util
import os

import numpy as np

from oracle.oracle import fse_compress_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXSV = 286


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", "sim", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sim = _load("u16_codec_sim")
ferr, is_err = sim.ferr, sim.is_err


# ------------------------------------------------------------------------------------------------------------------------------ NCount writer
def _write_ncount(norm, max_sv, tl, cap=None):
    """The NCount header (format: SURVEY A.2, written by lib/fse_compress.c:193-284) for any table log and alphabet -- the reference's writer is
    the byte coder's object and refuses table log 13.  With `cap` below FSE_NCountWriteBound it is the careful writer: dstSize_tooSmall (as the
    reference's size_t) when a 16-bit flush or the last two bytes would start beyond cap - 2.  Checked against the reference's bytes and
    verdicts by tests/test_u16_corpus.py and tests/test_gpu_u16.py."""
    out = bytearray()
    bit_stream, bit_count = tl - 5, 4
    remaining, threshold, nb = (1 << tl) + 1, 1 << tl, tl + 1
    sym, prev0, alphabet = 0, False, max_sv + 1
    careful = cap is not None and cap < ((((max_sv + 1) * tl) >> 3) + 3 if max_sv else 512)
    refused = False
    flushes = 0

    def flush16():
        nonlocal bit_stream, bit_count, refused, flushes
        flushes += 1
        if careful and len(out) > cap - 2:
            refused = True
        out.append(bit_stream & 0xFF); out.append((bit_stream >> 8) & 0xFF)
        bit_stream >>= 16; bit_count -= 16
    while sym < alphabet and remaining > 1:
        if prev0:
            start = sym
            while sym < alphabet and norm[sym] == 0:
                sym += 1
            assert sym < alphabet
            while sym >= start + 24:
                start += 24
                bit_stream += 0xFFFF << bit_count
                bit_count += 16; flush16()
            while sym >= start + 3:
                start += 3
                bit_stream += 3 << bit_count; bit_count += 2
            bit_stream += (sym - start) << bit_count; bit_count += 2
            if bit_count > 16:
                flush16()
        count = int(norm[sym]); sym += 1
        mx = (2 * threshold - 1) - remaining
        remaining -= abs(count)
        count += 1
        if count >= threshold:
            count += mx
        bit_stream += count << bit_count
        bit_count += nb - (1 if count < mx else 0)
        prev0 = count == 1
        assert remaining >= 1
        while remaining < threshold:
            nb -= 1; threshold >>= 1
        if bit_count > 16:
            flush16()
    assert remaining == 1
    refused = refused or (careful and len(out) > cap - 2)
    # wg_write_ncount (csrc/wave_glue.h) states the same verdict in closed form, from the header's bits: the position of the last flush
    assert not careful or refused == (2 * ((16 * flushes + bit_count - 1) >> 4) > cap - 2), (max_sv, tl, cap)
    if refused:
        return ferr("dstSize_tooSmall")
    out.append(bit_stream & 0xFF); out.append((bit_stream >> 8) & 0xFF)
    return np.frombuffer(bytes(out[:len(out) - 2 + (bit_count + 7) // 8]), dtype=np.uint8).copy()


# ------------------------------------------------------------------------------------------------------------------------------ labels
D_LABELS = (["d:csize_lt_2", "d:header_error", "d:tablelog_above_13", "d:nothing_behind_header",
             "d:builder_tl_le_11", "d:builder_tl_12", "d:builder_tl_13", "d:init_fails_no_bulk", "d:never_bulk_B_lt_113", "d:never_bulk_no_group"] +
            ["d:start_%d" % v for v in (833, 832, 113, 112)] + ["d:after_long_%d" % v for v in (833, 832, 113, 112)] +
            ["d:after_fin_113", "d:after_fin_112", "d:long_phase_leaves_65", "d:nb12_B832_no_long", "d:long_then_finishing"] +
            ["d:groups_%d" % g for g in (0, 1, 15, 16, 17)] +
            ["d:iteration_of_48_bits", "d:zero_bit_iterations_64plus"] +
            ["d:inA_%d" % k for k in range(4)] + ["d:last_word_bytes_%d" % k for k in range(4)] +
            ["d:c0_spread", "d:refills_0", "d:refills_1", "d:refills_8plus_ring_wraps_twice",
             "d:window_crosses_ring_end_at_phase_start", "d:refill_read_crosses_ring_end"] +
            ["d:iters_lt_32", "d:iters_32", "d:iters_64", "d:iters_65", "d:iters_300plus"] +
            ["d:out_row_mod8_%d" % k for k in (0, 2, 4, 6)] +
            ["d:cap_eq_n", "d:cap_n_minus_1", "d:cap_n_minus_5", "d:cap_above_n"] + ["d:cap_%d" % c for c in range(1, 6)] +
            ["d:cap_mod4_%d_above_16_groups" % k for k in (1, 2, 3)] +
            ["d:exit_clean", "d:exit_destination_full", "d:exit_reader_overrun", "d:exit_state_not_0"] +
            ["d:damaged_truncated", "d:damaged_last_zero", "d:damaged_last_random", "d:damaged_bitflip", "d:damaged_garbage", "d:damaged_header"])
C_LABELS = (["c:n_le_1", "c:err_maxsv_too_large", "c:err_tablelog_too_large", "c:err_symbol_above_limit", "c:one_symbol",
             "c:header_refused", "c:header_careful_fits", "c:tl_le_11", "c:tl_12_wide_launch", "c:n16384_tl11", "c:n16385_tl12", "c:request_13_clamped"] +
            ["c:count_head_%d" % k for k in range(8)] + ["c:count_tail_%d" % k for k in range(8)] +
            ["c:count_nvec_%d" % k for k in (192, 193, 256, 449)] + ["c:count_prefetch", "c:count_no_prefetch", "c:count_single_vectors"] +
            ["c:route_lane_short", "c:route_lane_skewed", "c:route_wave", "c:n_2047", "c:n_2048", "c:skew_at_63_64", "c:skew_at_63_64_plus_1",
             "c:wave_bail_word_in_front_of_row"] + ["c:wave_short_header_row_mod4_%d" % k for k in range(4)] +
            ["c:wave_bail_lane_under_8_bits", "c:lane_with_exactly_8_bits", "c:under_8_bits_by_search", "c:under_8_bits_by_arrangement",
             "c:warm_clamped_64", "c:warm_between", "c:warm_clamped_2048", "c:start_exact", "c:start_speculated", "c:lanes_without_symbols",
             "c:repair_rounds_0", "c:repair_rounds_1", "c:repair_rounds_2plus",
             "c:wave_room_le_8", "c:wave_room_edge_refused", "c:wave_room_edge_fits"] +
            ["c:sink_lead_%d" % k for k in range(64)] +
            ["c:sink_first_byte_shared", "c:sink_first_byte_own", "c:sink_piece_aligned", "c:sink_piece_copy_out", "c:sink_lane_without_piece"] +
            ["c:lane_n_mod4_%d" % k for k in range(4)] +
            ["c:lane_room_le_8", "c:lane_clamped_at_room_minus_8", "c:lane_room_edge_refused", "c:lane_room_edge_fits", "c:lane_result_0_not_compressible"])
LABELS = D_LABELS + C_LABELS
UNREACHABLE = dict(sim.UNREACHABLE)
UNREACHABLE.update({
    "d:after_long_113_table_log_le_11": "a long phase of 64 symbols takes at most 704 bits at table log 11 and starts from 833 or more: it leaves 129 "
                                        "or more.  113 / 112 behind a long phase exist in the table-log-12 class only (mix12)",
    "c:wave_result_0_not_compressible": "the wave kernel takes n >= 2048: at most 12 bits a symbol and a header under 512 bytes stay below "
                                        "2 (n - 1) bytes, so its `no compression` verdict cannot come out 0; the lane kernel's can (short blocks)",
})
SEARCH = {}
DAMAGE_STATS = {}
BATCH_CAPS = (20001, 67)          # capacities of the device runs that decode the whole corpus in one call: everything fits / 16 groups


def _rs(*key):
    seed = 54321
    for k in key:
        seed = (seed * 1000003 + int(k)) % ((1 << 31) - 1)
    return np.random.RandomState(seed)


# ------------------------------------------------------------------------------------------------------------------------------ decode blocks
class DBlock:
    """a compressed block (header + payload): `caps` the capacities it is decoded with alone, `in_off` / `out_off` its compressed row's address
    modulo 64 and its output row's modulo 8 when it is decoded alone"""

    def __init__(self, ref, name, comp, n, src=None, caps=None, in_off=0, out_off=0, kind="", bits=None):
        self.name, self.n, self.src, self.kind = name, n, src, kind
        self.bits = bits                                # fixed-cost tables: the sum of the symbols' costs (what B after the state read must be)
        self.comp = np.ascontiguousarray(comp, dtype=np.uint8)
        self.caps = [n] if caps is None else list(caps)
        self.in_off, self.out_off = in_off, out_off
        self.parsed = ref.fse_read_ncount(self.comp, MAXSV) if len(self.comp) >= 2 else None
        self._sims = {}

    @property
    def defined(self):
        """the reference is defined: no header that parses with nothing behind it (it would dereference a null stream pointer)"""
        return self.parsed is None or is_err(self.parsed[0]) or self.parsed[2] > sim.U16_MAXTL or self.parsed[0] < len(self.comp)

    def sim(self, cap, in_addr=None, out_addr=None, mut=None):
        key = (cap, self.in_off if in_addr is None else in_addr & 63, self.out_off if out_addr is None else out_addr & 7, mut)
        if key not in self._sims:
            self._sims[key] = sim.decode(self.comp, cap, self.parsed, key[1], key[2], mut)
        return self._sims[key]

    def labels(self, in_addr=None, out_addr=None):
        out = set()
        n = self.n
        for cap in self.caps:
            s = self.sim(cap, in_addr, out_addr)
            out |= s["labels"]
            if self.kind.startswith("damaged_"):
                out.add("d:" + self.kind)
                continue
            if self.kind in ("parse", "tl13"):
                continue
            if cap == n: out.add("d:cap_eq_n")
            if cap == n - 1: out.add("d:cap_n_minus_1")
            if cap == n - 5: out.add("d:cap_n_minus_5")
            if cap > n: out.add("d:cap_above_n")
            if 1 <= cap <= 5 and n > 100: out.add("d:cap_%d" % cap)
            if cap < n and cap >= 64 and (cap // 4) % 16 == 0 and cap % 4: out.add("d:cap_mod4_%d_above_16_groups" % (cap % 4))
            if self.kind == "mix12" and s["B0"] == 832 and s["nLong"] == 0 and cap >= n: out.add("d:nb12_B832_no_long")
        return out


def table_block(ref, name, norm, tl, src, **kw):
    """header by the writer above, table and payload by FSE_buildCTableU16 / FSE_compressU16_usingCTable"""
    norm = np.asarray(norm, np.int16)
    msv = len(norm) - 1
    hdr = _write_ncount(norm, msv, tl)
    e, ct = ref.fse_build_ctable_u16(norm, msv, tl)
    assert not is_err(e), name
    src = np.asarray(src, np.uint16)
    cs, payload = ref.fse_compress_u16_using_ctable(src, ct, 2 * len(src) + 1024)
    assert not is_err(cs) and cs > 0, name
    return DBlock(ref, name, np.concatenate([hdr, payload[:cs]]), len(src), src, **kw)


def flat_block(ref, name, k, n, seed=1, **kw):
    src = _rs(k, n, seed).randint(0, 1 << k, n)
    return table_block(ref, name, np.ones(1 << k, np.int16), k, src, kind="flat%d" % k, bits=k * n, **kw)


def nb12_block(ref, name, n, used=256, seed=1, **kw):
    norm = np.array([1] * used + [4096 - used], np.int16)
    return table_block(ref, name, norm, 12, _rs(12, n, seed).randint(0, used, n), kind="nb12", bits=12 * n, **kw)


MIX11 = np.array([1] * 100 + [2] * 50 + [66] + [18] * 99, np.int16)                  # 2048: symbols 0..99 cost 11 bits, 100..149 cost 10
MIX12 = np.array([1] * 100 + [2] * 50 + [4] * 20 + [116] + [37] * 100, np.int16)     # 4096: 0..99 cost 12, 100..149 cost 11, 150..169 cost 10


def mix_block(ref, name, tl, costs, **kw):
    """`costs`: bits per symbol in decoding order"""
    norm = MIX11 if tl == 11 else MIX12
    assert int(norm.sum()) == 1 << tl
    rs = _rs(tl, len(costs), sum(costs))
    pick = {tl: (0, 100), tl - 1: (100, 150), tl - 2: (150, 170)}
    src = [rs.randint(*pick[c]) for c in costs]
    return table_block(ref, name, norm, tl, src, kind="mix%d" % tl, bits=sum(costs), **kw)


def u16_data(kind, n, seed):
    rs = _rs(n, seed, len(kind))
    if kind == "flat":
        return rs.randint(0, MAXSV + 1, n).astype(np.uint16)
    if kind == "geo":
        return np.minimum(rs.geometric(0.05, n) - 1, MAXSV).astype(np.uint16)
    if kind == "small":
        return (rs.randint(0, 5, n) * 70).astype(np.uint16)
    if kind == "two":
        return rs.randint(0, 2, n).astype(np.uint16)
    if kind == "rare":                                  # one dominant symbol, a few stragglers
        a = np.full(n, 7, np.uint16)
        idx = rs.randint(0, n, max(n // 300, 1))
        a[idx] = rs.randint(0, MAXSV + 1, idx.size)
        return a
    if kind.startswith("dom"):                          # "dom<k>_<permille>": symbol 0 with that probability, k others evenly
        k, pm = (int(v) for v in kind[3:].split("_"))
        a = rs.randint(1, k + 1, n).astype(np.uint16)
        a[rs.random_sample(n) < pm / 1000.0] = 0
        return a
    raise ValueError(kind)


def data_block(ref, name, kind, n, tl=0, seed=1, **kw):
    """the reference's own stream for the data (FSE_compressU16)"""
    src = u16_data(kind, n, seed)
    cs, out = ref.fse_compress_u16(src, 0, tl)
    assert not is_err(cs) and cs > 1, (name, cs)
    return DBlock(ref, name, out[:cs], n, src, kind="data", **kw)


def tl13_block(ref, name, n, seed=1, **kw):
    """a stream of table log 13, which the reference's compressor never writes: its own counts for the data scaled up to 13 bits"""
    src = u16_data("geo", n, seed)
    cs, out = ref.fse_compress_u16(src, 0, 12)
    h, msv, tl, norm = ref.fse_read_ncount(out[:cs], MAXSV)
    norm13 = (np.abs(norm[:msv + 1].astype(np.int64)) << (13 - tl)).astype(np.int16)      # (a counter of -1 is one cell)
    b = table_block(ref, name, norm13, 13, src, **kw)
    b.kind = "tl13"
    return b


DAMAGE = ("truncated", "last_zero", "last_random", "bitflip", "garbage", "header")


def damaged(ref, blk, how, seed):
    rs = _rs(len(blk.comp), seed, DAMAGE.index(how))
    c = blk.comp.copy()
    h = blk.parsed[0]
    if how == "truncated":
        c = c[:int(rs.randint(h + 1, len(c)))]
    elif how == "last_zero":
        c[-1] = 0
    elif how == "last_random":
        c[-1] = int(rs.randint(0, 256))
    elif how == "bitflip":
        for _ in range(1 + seed % 3):
            c[int(rs.randint(h, len(c)))] ^= 1 << int(rs.randint(0, 8))
    elif how == "garbage":
        c[h:] = rs.randint(0, 256, len(c) - h)
    elif how == "header":
        c[int(rs.randint(0, h))] ^= 1 << int(rs.randint(0, 8))
    return DBlock(ref, "%s_%s_%d" % (blk.name, how, seed), c, blk.n, None, [blk.n, blk.n + 7], blk.in_off, blk.out_off, "damaged_" + how)


def build_decode(ref):
    """-> the decode-side blocks in corpus order"""
    B = []
    offs = [0, 0]

    def place():                                        # compressed rows: every residue modulo 4, a spread modulo 64; output rows: 0 2 4 6 modulo 8
        offs[0] = (offs[0] + 13) & 63
        offs[1] = (offs[1] + 2) & 7
        return dict(in_off=offs[0], out_off=offs[1])

    def add(b):
        B.append(b)
        return b
    # ---- parse refusals
    add(DBlock(ref, "parse_size_0", np.zeros(0, np.uint8), 10, kind="parse", **place()))
    add(DBlock(ref, "parse_size_1", np.array([0x35], np.uint8), 10, kind="parse", **place()))
    good = flat_block(ref, "flat5_seed", 5, 40)
    h = good.parsed[0]
    bad = good.comp.copy(); bad[:h] = 0xFF                                # a header that does not parse
    add(DBlock(ref, "parse_header_error", bad, 40, kind="parse", **place()))
    add(DBlock(ref, "parse_no_payload", good.comp[:h], 40, kind="parse", **place()))
    n14 = np.array([1] * 200 + [(1 << 14) - 200], np.int16)
    add(DBlock(ref, "parse_tl14", np.concatenate([_write_ncount(n14, 200, 14), np.array([1, 2, 3, 0x81], np.uint8)]), 40, kind="parse", **place()))
    # ---- the phase rules on their values (start), flat tables
    for k, n in ((7, 119), (8, 104), (7, 16), (8, 14), (5, 22), (5, 23), (6, 139), (6, 138), (7, 120), (7, 118), (8, 105), (8, 103)):
        add(flat_block(ref, "flat%d_n%d" % (k, n), k, n, caps=[n, n + 64], **place()))
    c113, c112 = [11] * 3 + [10] * 8, [11] * 2 + [10] * 9
    for inA in range(4):                                # payload at every address modulo 4 (mix11's header is 263 bytes... whatever it is: in_off is the row's)
        for tag, tailc in (("113", c113), ("112", c112)):
            add(mix_block(ref, "mix11_start_%s_a%d" % (tag, inA), 11, tailc, caps=[11, 64], in_off=17 * inA, out_off=2 * inA))
    c833, c832 = [11] * 3 + [10] * 80, [11] * 2 + [10] * 81
    for tag, tailc in (("833", c833), ("832", c832)):
        add(mix_block(ref, "mix11_start_" + tag, 11, tailc, caps=[len(tailc), 200], **place()))
        add(mix_block(ref, "mix11_after_long_" + tag, 11, [11] * 64 + tailc, caps=[64 + len(tailc), 400], **place()))
    for tag, tailc in (("113", c113), ("112", c112)):
        add(mix_block(ref, "mix11_after_fin_" + tag, 11, [11, 10] * 2 + tailc, caps=[15, 64], **place()))
    # ---- table log 12: the same, and what only twelve-bit symbols reach
    d113, d112 = [12] * 3 + [11] * 7, [12] * 2 + [11] * 8
    d833, d832 = [12] * 63 + [11] * 7, [12] * 62 + [11] * 8
    for tag, tailc in (("113", d113), ("112", d112), ("833", d833), ("832", d832)):
        add(mix_block(ref, "mix12_start_" + tag, 12, tailc, caps=[len(tailc), 200], **place()))
    add(mix_block(ref, "mix12_leaves_65", 12, [12] * 64 + [11] * 5 + [10], caps=[70, 100], **place()))
    for tag, tailc in (("113", d113), ("112", d112)):
        add(mix_block(ref, "mix12_after_long_" + tag, 12, [12] * 64 + tailc, caps=[64 + len(tailc), 200], **place()))
        add(mix_block(ref, "mix12_after_fin_" + tag, 12, [12, 11] * 2 + tailc, caps=[14, 64], **place()))
    for tag, tailc in (("833", d833), ("832", d832)):
        add(mix_block(ref, "mix12_after_long_" + tag, 12, [12] * 64 + tailc, caps=[64 + len(tailc), 300], **place()))
    for n in (70, 200, 1400):
        add(nb12_block(ref, "nb12_n%d" % n, n, caps=[n, n - 1, n + 3], **place()))
    add(nb12_block(ref, "nb12_286_n600", 600, used=286, **place()))
    # ---- room in the destination: plenty of bits, few groups; the literal tail's capacities
    n = 1500
    add(flat_block(ref, "flat7_roomy", 7, n, caps=[0, 1, 2, 3, 4, 5, 7, 60, 63, 64, 65, 66, 67, 68, 71, 128, 129, 130, 131, 4 * 48 + 1,
                                                  n, n - 1, n - 5, n + 1, n + 40], **place()))
    add(nb12_block(ref, "nb12_roomy", 900, caps=[3, 4, 63, 64, 65, 68, 899, 900, 905], **place()))
    # ---- state ring: total iterations under 32, 32, 64, 65, 300 and more -- by search over the sizes of a flat table
    want = {"lt32": None, 32: None, 64: None, 65: None}
    for n in range(30, 330):
        b = flat_block(ref, "flat8_n%d" % n, 8, n)
        it = b.sim(n)["iters"]
        key = it if it in want else ("lt32" if 0 < it < 32 and want["lt32"] is None and n >= 60 else None)
        if key is not None and want[key] is None:
            want[key] = b
    SEARCH["iters"] = {str(k): (v.name if v else None) for k, v in want.items()}
    for v in want.values():
        if v is not None:
            v.__dict__.update(place())
            add(v)
    # ---- input ring: payloads that are never refilled, refilled once, many times; the partial last word; the ring's end
    for n in range(150, 158):
        add(flat_block(ref, "flat8_ring_n%d" % n, 8, n, in_off=(5 * n) & 63, out_off=(2 * n) & 7))
    for n in range(225, 233):
        add(flat_block(ref, "flat8_ring_n%d" % n, 8, n, in_off=(7 * n) & 63, out_off=(2 * n) & 7))
    for n, k in ((1300, 8), (1900, 6), (2000, 7)):
        add(flat_block(ref, "flat%d_long_n%d" % (k, n), k, n, **place()))
    # ---- real streams by table log (the reference's compressor), capacity around the size
    for j, (kind, n, tl) in enumerate((("geo", 300, 0), ("geo", 2100, 0), ("flat", 2050, 0), ("small", 1000, 6), ("flat", 1700, 9), ("geo", 2000, 10),
                                       ("rare", 2100, 0), ("dom6_900", 2000, 0), ("geo", 9000, 0), ("small", 60, 0), ("two", 90, 5), ("geo", 17, 0))):
        add(data_block(ref, "data_%s_n%d_%d" % (kind, n, j), kind, n, tl, seed=j, caps=[n, n - 1, n - 5, n + 1], **place()))
    add(data_block(ref, "data_tl12_n16385", "geo", 16385, 0, seed=3, **place()))
    add(data_block(ref, "data_tl12_n20000", "flat", 20000, 0, seed=4, caps=[20000, 19999], **place()))
    # a dominant symbol: cells of nbBits 0, iterations that take no bits at all, and the end game with a state that is not back at 0
    big = add(data_block(ref, "data_dominant_n20000", "dom3_999", 20000, 0, seed=5, caps=[20000, 19999, 19998, 19997, 19996, 20001], **place()))
    add(data_block(ref, "data_big11_n20000", "geo", 20000, 11, seed=7, **place()))
    add(data_block(ref, "data_dominant_n6000", "dom2_998", 6000, 0, seed=6, caps=[6000, 5999, 5998], **place()))
    add(tl13_block(ref, "tl13_n3000", 3000, seed=1, caps=[3000, 2999, 3009], **place()))
    add(tl13_block(ref, "tl13_n150", 150, seed=2, **place()))
    # ---- a block that never enters the bulk: too few bits; initOk false comes with the damaged ones (last byte zero)
    add(flat_block(ref, "flat5_n8", 5, 8, **place()))
    add(flat_block(ref, "flat6_n3", 6, 3, **place()))
    add(mix_block(ref, "mix12_n4", 12, [12, 11, 10, 12], **place()))
    # ---- damaged streams: generated by seed, the undefined ones (a header that parses with nothing behind it) dropped here
    by = {b.name: b for b in B}
    gen = kept = 0
    for base in ("data_geo_n2100_1", "flat7_roomy", "nb12_n1400", "data_dominant_n6000", "tl13_n150", "data_small_n60_9", "mix11_after_long_833"):
        for how in DAMAGE:
            for seed in range(3):
                d = damaged(ref, by[base], how, seed)
                gen += 1
                if d.defined and len(d.comp) >= 2:
                    kept += 1
                    add(d)
    DAMAGE_STATS.update(generated=gen, kept=kept)
    assert big.n == 20000
    return B


def decode_company(blocks):
    """workgroups of mixed fate: orderings (lists of blocks, one workgroup's range each) for the 4 KiB launch (33 blocks) and the 8 KiB launch
    (18 blocks).  Each holds blocks of the other class, a header that fails, a header with nothing behind it, a table-log-13 block, blocks
    that never enter the bulk, one 20,000-symbol block among blocks of under 200 symbols, and four consecutive slots on a multiple of 4 (one
    service wave's blocks) none of which is the launch's."""
    by = {b.name: b for b in blocks}
    zero = next(b.name for b in blocks if b.kind == "damaged_last_zero" and b.sim(b.n)["cls"] == 11)
    trunc = next(b.name for b in blocks if b.kind == "damaged_truncated" and b.sim(b.n)["cls"] == 11)
    small11 = ["flat7_n119", "flat8_n104", "flat7_n16", "mix11_start_113_a1", "flat5_n8", zero, "flat6_n139", "mix11_after_fin_112", "flat8_ring_n150",
               "data_small_n60_9", trunc, "flat6_n3", "data_two_n90_10", "mix11_start_833", "data_geo_n17_11", "flat5_n22"]
    small12 = ["mix12_start_113", "mix12_leaves_65", "nb12_n70", "mix12_after_fin_113", "mix12_start_833", "mix12_after_long_112", "nb12_n200", "mix12_n4"]
    odd = ["parse_header_error", "parse_no_payload", "tl13_n150", "parse_tl14"]
    wg11 = ["data_big11_n20000"] + small11[:3] + small12[:4] + small11[3:8] + odd + small11[8:] + small12[4:] + ["flat7_n120", "flat7_n118", "parse_size_1", "flat8_n105"]
    wg11_b = small11[:4] + odd + small11[4:12] + small12[:4] + small11[12:] + ["data_big11_n20000"] + small12[4:] + ["flat7_n120", "flat7_n118", "flat8_n105", "parse_size_1"]
    wg12 = ["data_tl12_n20000"] + small12[:3] + small11[:4] + small12[3:] + odd + ["nb12_n1400"]
    wg12_b = small12[:4] + ["flat7_n119", "tl13_n150", "parse_no_payload", "flat5_n8"] + small12[4:] + ["parse_header_error", "data_tl12_n20000", "nb12_n1400", "parse_tl14", "mix12_start_112", "mix12_start_832"]
    out = {"wg11_a": (11, wg11), "wg11_b": (11, wg11_b), "wg12_a": (12, wg12), "wg12_b": (12, wg12_b)}
    return {k: (cls, [by[n] for n in names]) for k, (cls, names) in out.items()}


# ------------------------------------------------------------------------------------------------------------------------------ compress blocks
class CBlock:
    """a source block of FSE_compressU16: `caps` (None = FSE_compressBound) the capacities it is compressed with alone, `src_off` / `dst_off` its
    source row's address modulo 16 and its destination row's modulo 64 when it is compressed alone"""

    def __init__(self, ref, name, src, msv=0, tl=0, caps=(None,), src_off=0, dst_off=0, kind=""):
        self.name, self.msv, self.tl, self.kind = name, msv, tl, kind
        self.src = np.ascontiguousarray(src, dtype=np.uint16)
        self.n = len(self.src)
        self.src_off, self.dst_off = src_off, dst_off
        self.bound = fse_compress_bound(2 * self.n)
        self.facts = None
        self._sims = {}
        n = self.n
        if n > 1 and (msv or MAXSV) <= MAXSV and (tl or 12) <= 13 and int(self.src.max()) <= (msv or MAXSV) and int(np.bincount(self.src).max()) < n:
            r, out = ref.fse_compress_u16(self.src, msv, tl, cap=self.bound)         # (room for everything: the reference is defined)
            assert not is_err(r), (name, r)
            h, m2, tl2, norm = ref.fse_read_ncount(out, MAXSV)                      # (also where the result is 0: the bytes are written)
            assert not is_err(h), name
            e, ct = ref.fse_build_ctable_u16(norm[:m2 + 1], m2, tl2)
            assert not is_err(e), name
            self.facts = dict(norm=norm[:m2 + 1].copy(), msv=m2, tl=tl2, header=out[:h].tobytes(), ct=ct)
            # the payload by FSE_compressU16_usingCTable on that table is the one-shot call's
            cs, pay = ref.fse_compress_u16_using_ctable(self.src, ct, self.bound)
            assert r == 0 or (cs == r - h and bytes(pay[:cs]) == bytes(out[h:r])), name
        self.caps = [self.resolve(c) for c in caps]

    def resolve(self, c):
        """capacities are written relative to the block: None = the bound, ("hdr", d) = header size + d, ("fit", d) = header + 8 + (total >> 3) + d"""
        if c is None:
            return self.bound
        if isinstance(c, tuple):
            hdr = len(self.facts["header"])
            if c[0] == "hdr":
                return hdr + c[1]
            total = self.sim(self.bound)["total"]
            return hdr + 8 + (total >> 3) + c[1]
        return c

    def hdr_verdict(self, cap):
        f = self.facts
        v = _write_ncount(f["norm"], f["msv"], f["tl"], cap)
        return v if isinstance(v, int) else len(v)

    def sim(self, cap, src_addr=None, dst_addr=None, mut=None):
        key = (cap, self.src_off if src_addr is None else src_addr & 15, self.dst_off if dst_addr is None else dst_addr & 63, mut)
        if key not in self._sims:
            self._sims[key] = sim.compress(self.src, self.msv, self.tl, cap, self.facts, 1024 + key[1], 1024 + key[2], self.hdr_verdict, mut)
        return self._sims[key]

    def ref_defined(self, cap):
        """FSE_compressU16 is defined: the header does not fit at all, or more than 8 bytes are left behind it"""
        if self.facts is None:
            return True
        hdr = len(self.facts["header"])
        return cap < hdr or cap > hdr + 8

    def labels(self, src_addr=None, dst_addr=None):
        out = set()
        for cap in self.caps:
            s = self.sim(cap, src_addr, dst_addr)
            out |= s["labels"]
            if "c:wave_bail_lane_under_8_bits" in s["labels"] and self.kind in ("search", "arranged"):
                out.add("c:under_8_bits_by_" + ("search" if self.kind == "search" else "arrangement"))
        return out


def skew_search(ref):
    """4,096 symbols, a dominant one and one or three rare ones: blocks whose normalised top counter is exactly 63/64 of the table (not skewed) and
    63/64 + 1 (skewed), at table logs 8 and 9"""
    found = {}
    for tl in (8, 9):
        ts = 1 << tl
        for rare in (1, 3):
            for dom in range(4096 - 90, 4096 - 40):
                rs = _rs(tl, rare, dom)
                src = np.zeros(4096, np.uint16)
                idx = rs.permutation(4096)[:4096 - dom]
                src[idx] = 1 + (np.arange(len(idx)) % rare)
                r, out = ref.fse_compress_u16(src, 0, tl)
                if is_err(r) or r <= 1:
                    continue
                _, m2, tl2, norm = ref.fse_read_ncount(out, MAXSV)
                if tl2 != tl:
                    continue
                top1 = int(norm[:m2 + 1].max())
                for tag, v in (("at", 63 * ts // 64), ("plus1", 63 * ts // 64 + 1)):
                    if top1 == v and (tl, tag) not in found:
                        found[(tl, tag)] = (rare, dom, src)
    return found


def build_compress(ref):
    B = []
    offs = [0, 0]

    def place():
        offs[0] = (offs[0] + 6) & 15
        offs[1] = (offs[1] + 21) & 63
        return dict(src_off=offs[0], dst_off=offs[1])

    def add(b):
        B.append(b)
        return b
    geo = lambda n, s=1: u16_data("geo", n, s)
    # ---- early outs and argument errors
    add(CBlock(ref, "n0", np.zeros(0, np.uint16), **place()))
    add(CBlock(ref, "n1", np.array([9], np.uint16), **place()))
    add(CBlock(ref, "msv_287", geo(300), msv=287, **place()))
    add(CBlock(ref, "tl_14", geo(300), tl=14, **place()))
    add(CBlock(ref, "symbol_above", geo(3000), msv=3, **place()))
    add(CBlock(ref, "one_symbol", np.full(2500, 123, np.uint16), **place()))
    add(CBlock(ref, "one_symbol_short", np.full(2, 5, np.uint16), **place()))
    # ---- header refusals and the careful writer
    add(CBlock(ref, "hdr_small_room", geo(3000, 2), caps=[0, 1, 3, ("hdr", -1), ("hdr", 0), ("hdr", 8), ("hdr", 9), ("hdr", 30)], **place()))
    add(CBlock(ref, "hdr_small_room_flat", u16_data("flat", 2500, 2), caps=[5, 100, ("hdr", -2), ("hdr", -1), ("hdr", 4), ("hdr", 9), ("hdr", 60)], **place()))
    # ---- table-log class: 16,384 / 16,385 symbols, a request of 13
    add(CBlock(ref, "geo_n16384", geo(16384, 3), **place()))
    add(CBlock(ref, "geo_n16385", geo(16385, 3), **place()))
    add(CBlock(ref, "flat_n16385", u16_data("flat", 16385, 4), **place()))
    add(CBlock(ref, "geo_n20000_tl13", geo(20000, 5), tl=13, **place()))
    add(CBlock(ref, "geo_n5000_tl13", geo(5000, 5), tl=13, **place()))
    # ---- counting loop: head 0..7 (source row at every address modulo 16 in steps of 2), nvec at 192, 193, 256, 449, tail 0..7
    for k in range(8):
        head = ((-2 * k) & 15) >> 1
        for nvec, tail in ((192, k), (193, 7 - k), (256, (k + 3) & 7), (449, (k + 5) & 7))[k % 2::2] + ((5, k),):
            n = head + 8 * nvec + tail
            add(CBlock(ref, "count_h%d_v%d_t%d" % (head, nvec, tail), geo(n, k), src_off=2 * k, dst_off=(11 * k + nvec) & 63))
    # ---- encoder route: 2,047 / 2,048 symbols; the skew limit by search
    add(CBlock(ref, "geo_n2047", geo(2047, 6), **place()))
    add(CBlock(ref, "geo_n2048", geo(2048, 6), **place()))
    add(CBlock(ref, "geo_n2049", geo(2049, 6), **place()))
    found = skew_search(ref)
    SEARCH["skew"] = {"tl%d_%s" % k: (v[0], v[1]) for k, v in sorted(found.items())}
    for (tl, tag), (rare, dom, src) in sorted(found.items()):
        add(CBlock(ref, "skew_tl%d_%s_r%d_d%d" % (tl, tag, rare, dom), src, tl=tl, kind="search", **place()))
    # a lane with fewer than 8 bits although the table is not skewed, by arrangement: a long run of the dominant symbol inside a mixed block
    arr = u16_data("small", 4096, 9)
    arr[:] = np.where(_rs(4096, 77).random_sample(4096) < 0.94, 0, arr + 1)       # (a share between 0.917 -- 8 bits in 64 symbols -- and 63/64)
    arr[1000:1400] = 0
    add(CBlock(ref, "arranged_run", arr, kind="arranged", **place()))
    # the other side of that rule: a block the wave kernel keeps although one lane has exactly 8 bits (seeds kept from a search over 80 seeds a share)
    for pm, seed in ((820, 1), (840, 10)):
        add(CBlock(ref, "eight_bits_dom4_%d_s%d" % (pm, seed), u16_data("dom4_%d" % pm, 2048, seed), kind="eight", **place()))
    # ---- the aligned word in front of the row: two-symbol blocks, header of 2 bytes (table log 5 asked for) and of 3 (default), rows at 0..3 mod 4
    for n in (2048, 4096):
        for a in range(4):
            add(CBlock(ref, "two_n%d_tl5_a%d" % (n, a), u16_data("two", n, a), tl=5, src_off=2 * a, dst_off=20 + a))
            add(CBlock(ref, "two_n%d_def_a%d" % (n, a), u16_data("two", n, a), src_off=4 * a, dst_off=40 + a))
    # ---- inside the wave kernel: warm-up clamps, repair rounds, lanes without symbols
    add(CBlock(ref, "flat_n2100", u16_data("flat", 2100, 7), **place()))                      # many symbols: warm-up 64
    add(CBlock(ref, "small_n2300", u16_data("small", 2300, 7), **place()))                    # 5 symbols at table log 9: in between
    add(CBlock(ref, "three_n8300", u16_data("dom2_600", 8300, 7), **place()))                 # 3 symbols at table log 11: 2048
    add(CBlock(ref, "slow_n8300", u16_data("dom2_950", 8300, 8), **place()))                  # slowly mixing: repair rounds
    add(CBlock(ref, "slow_n4200", u16_data("dom3_930", 4200, 8), **place()))
    add(CBlock(ref, "rare_n5000", u16_data("rare", 5000, 8), **place()))
    # ---- capacity verdicts of both encoders
    for name, src in (("geo_n2600", geo(2600, 9)), ("geo_n900", geo(900, 9)), ("geo_n901", geo(901, 9)), ("geo_n902", geo(902, 9)), ("geo_n903", geo(903, 9))):
        add(CBlock(ref, name + "_room", src, caps=[None, ("hdr", 4), ("hdr", 9), ("hdr", 12), ("fit", -3), ("fit", -1), ("fit", 0), ("fit", 1), ("fit", 2), ("fit", 9)], **place()))
    for n in (2, 3, 4, 5, 6, 9, 14, 40):                                                     # short blocks: `no compression`
        add(CBlock(ref, "flat_n%d" % n, u16_data("flat", n, n), **place()))
    # ---- U16Sink: the payload address at every value modulo 64 (the header's size is the block's: the row's address makes up for it)
    base = geo(2048, 10)
    hdr = len(CBlock(ref, "sink_probe", base).facts["header"])
    for lead in range(64):
        add(CBlock(ref, "sink_lead_%d" % lead, base, src_off=(2 * lead) & 15, dst_off=(lead - hdr) & 63))
    return B


def build(ref):
    """-> (decode blocks, compress blocks)"""
    return build_decode(ref), build_compress(ref)


def corpus_labels(dblocks, cblocks, daddr=None, caddr=None):
    """every label the corpus reaches when each block runs alone; daddr / caddr: name -> (row address in, row address out) as a device run placed
    them (default: the blocks' own offsets)"""
    lab = set()
    c0 = set()
    for b in dblocks:
        ia, oa = daddr[b.name] if daddr else (None, None)
        lab |= b.labels(ia, oa)
        c0 |= {s["c0"] for s in (b.sim(cap, ia, oa) for cap in b.caps) if s["everBulk"]}
    if len(c0) >= 8:                                    # (the payload's aligned base is a multiple of 4: 16 values exist)
        lab.add("d:c0_spread")
    for b in cblocks:
        sa, da = caddr[b.name] if caddr else (None, None)
        lab |= b.labels(sa, da)
    return lab


# ------------------------------------------------------------------------------------------------------------------------------ device rows
def device_bytes(torch, rows, off, stride_pad=1, guard=0, fill=0):
    """byte rows on the device in one buffer: row stride max(len) + guard + stride_pad (made odd), the first row `off` bytes above a
    256-byte boundary -> (2-D uint8 view over the rows WITH their guard bytes, row stride)"""
    w = max(max((len(r) for r in rows), default=1), 1) + guard + stride_pad
    w |= 1
    buf = torch.full((len(rows) * w + 1024,), fill, dtype=torch.uint8, device="cuda")
    base = (-buf.data_ptr()) % 256 + off
    view = buf[base:base + len(rows) * w].view(len(rows), w)
    host = np.full((len(rows), w), fill, np.uint8)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.frombuffer(bytes(r), np.uint8) if not isinstance(r, np.ndarray) else r
    view.copy_(torch.from_numpy(host))
    return view, w


def device_u16(torch, rows, off, width=None, fill=0):
    """rows of 16-bit symbols on the device: an odd number of symbols per row stride (rows on every 2-byte phase of a 16-byte line), the first
    row `off` bytes (even) above a 256-byte boundary -> 2-D int16 view"""
    assert off % 2 == 0
    w = (max(max((len(r) for r in rows), default=1), 1) if width is None else width) | 1
    buf = torch.full((len(rows) * w + 512,), fill, dtype=torch.int16, device="cuda")
    base = ((-buf.data_ptr()) % 256 + off) // 2
    view = buf[base:base + len(rows) * w].view(len(rows), w)
    host = np.full((len(rows), w), fill, np.int16)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.asarray(r, np.uint16).view(np.int16)
    view.copy_(torch.from_numpy(host))
    return view

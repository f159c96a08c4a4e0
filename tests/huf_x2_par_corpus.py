"""Blocks with double-symbol (X2) tables for the stream-parallel Huff0 decoder (k_huf_decode_par<HPAR_DATA_LARGE, true>, csrc/huf_decode_par.hip;
model: derive_x2 / simulate_block(accept_x2=True) in scripts/sim/huf_par_sim.py).  Every table comes from the COMPILED REFERENCE
(HUF_buildCTable -> HUF_writeCTable -> HUF_readDTableX2), every payload from its HUF_compress4X / 1X_usingCTable; seeds and constructions are
fixed, so building twice gives the same bytes.  Every entry carries its labels (LABELS lists what the corpus must reach).

  valid tables    every table log 1 .. 12 read at limit = table log (geometric histograms: logs 1 .. 4 cannot come from HUF_compress2), logs 1, 5
                  and 8 again at limit 12 (a 1-bit code owns 2048 cells: next to the n < ts rule), real blocks P 2 / 14 / 80, and the shapes of
                  the walk: dst_size % 4 != 0, a stream of exactly HPAR_MIN_BITS bits and one bit less, a longest stream between 4513 and 8480
                  bytes (one piece here, two with a single-symbol table), one above 8480 (two pieces), a stretch of 1-bit codes that spills
                  HPAR_KEEP; forms 4 and 1; a batch that shares one table.  The tests run all of it at max_table_log 12 and 11 (the 4 KiB slot;
                  a table of log 12 is then the literal kernel's tableLog_tooLarge).
  damaged tables  one cell changed so that ONE rule of X2_CLAUSES breaks first, at cell 0, a cell 64k, a cell 64k + 17 and the last cell where
                  the rule allows it (a run boundary or a one-symbol cell cannot sit just anywhere), on a table filled above its code's own log
                  (P14, log 11 read at 12), one at its own log, and one of 32 cells.  The length field stays 1 or 2, so the reference stays
                  inside its buffers.  The cell is chosen among those the reference's walk looks up: for EVERY damaged-table entry the
                  reference's (result, bytes) differ from (dst_size, block) -- a kernel that vouched for the table would return the block.
                  Each damage goes with its valid payload; the 64k ones also with a corrupted payload.
  benign          junk in descriptor bytes 0 and 3 (maxTableLog as found, reserved): still accepted.
  CPU only        a length field of 0 and of 3 (the literal kernel clamps the advance, huf_decode.hip:416-417, and so differs from the reference
                  by design) and the constant table, every cell {s, 0 bits, 1 symbol}: one run fills the table and only n < ts declines it.  A
                  kernel without that rule would derive a code of zero bits and never terminate -- on shared machines -- so these never enter
                  a device batch (`cpu_only`).
  damaged payloads  on valid tables: a flipped bit inside lane 0's range, one in a middle lane, the payload one byte short, dst_size - 1.
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("huf_par_sim", os.path.join(ROOT, "scripts", "sim", "huf_par_sim.py"))
hsim = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(hsim)

W12 = 1 + (1 << 12)
TOO_LARGE = (1 << 64) - 5                                               # tableLog_tooLarge (lib/error_public.h)
CLAUSES = tuple(hsim.X2_CLAUSES)
POSITIONS = ("cell0", "at64k", "at64k17", "last")
LABELS = (["log_%d" % t for t in range(1, 13)] + ["log_%d_at_12" % t for t in (1, 5, 8)] + ["real_p2", "real_p14", "real_p80"] +
          ["form_1", "form_4", "dst_not_mult4", "min_bits_at", "min_bits_under", "one_piece_two_on_x1", "two_pieces", "spill",
           "repair_rounds", "over_max_repair", "cells_under_64", "filled_above_own_log", "slot_4k", "limit11_too_large", "shared_table", "benign_descriptor",
           "len_0", "len_3", "constant_table", "pl_lane0", "pl_middle", "pl_short", "pl_dst_minus_1"] +
          ["declined_" + c for c in CLAUSES] + ["damage_" + p for p in POSITIONS])


class X2Entry:
    def __init__(self, name, blk, form, dst_size, payload, dt, labels=(), kind="valid", clause=None, cpu_only=False):
        self.name, self.blk, self.form, self.dst_size, self.payload, self.kind, self.clause, self.cpu_only = name, blk, form, dst_size, payload, kind, clause, cpu_only
        self.dt = np.ascontiguousarray(dt[:W12], dtype=np.uint32)
        self.labels = list(labels)
        self.table_log = (int(self.dt[0]) >> 16) & 0xFF

    def simulate(self, mut=None, decode=True, max_table_log=12):
        return hsim.simulate_block(self.payload, self.dt, self.dst_size, self.form, max_table_log=max_table_log, decode=decode, mut=mut, accept_x2=True)

    def reference(self, ref, max_table_log=12):
        """(result, bytes) of HUF_decompress4X / 1X_usingDTable; the batch calls check the table log against max_table_log first"""
        if self.table_log > max_table_log:
            return TOO_LARGE, np.zeros(0, np.uint8)
        f = ref.huf_decompress1x_using_dtable if self.form == 1 else ref.huf_decompress4x_using_dtable
        return f(self.payload, self.dt, self.dst_size)


# ---------------------------------------------------------------------------------------------------------------------------- tables and payloads
def geometric(t):
    """counts whose Huffman code has the lengths 1, 2, .., t - 1, t, t: table log t"""
    return np.array([1, 1] + [1 << k for k in range(1, t)], np.uint32)


def draw(count, size, seed):
    """a block of `size` symbols with the histogram's proportions (every symbol of the histogram has a code)"""
    rs = np.random.RandomState(seed)
    p = np.asarray(count, np.float64)
    return rs.choice(len(count), size, p=p / p.sum()).astype(np.uint8)


def tables(ref, count, limit, L):
    """(CTable, double-symbol DTable read at maxTableLog L, table log of the code)"""
    count = np.asarray(count, np.uint32)
    msv = len(count) - 1
    tl, celt = ref.huf_build_ctable(count, msv, limit)
    assert 0 < tl <= 12, tl
    h, hdr = ref.huf_write_ctable(256, celt, msv, tl)
    assert 0 < h < 256, h
    r, dt = ref.huf_read_dtable_x2(hdr[:h], L)
    assert r == h, (r, h)
    return celt, dt, tl


def hist(blk):
    return np.bincount(blk, minlength=int(blk.max()) + 1).astype(np.uint32)


def compress(ref, blk, celt, form):
    r, s = (ref.huf_compress1x_using_ctable if form == 1 else ref.huf_compress4x_using_ctable)(blk, celt)
    assert 0 < r < (1 << 32), r
    return s[:r].copy()


def stream_bits(payload):
    """unread bits under the end mark of a one-stream payload (bitstream.h:285-290)"""
    return 8 * (len(payload) - 1) + int(payload[-1]).bit_length() - 1


def valid_entries(ref, orc):
    out = []

    def add(name, blk, form, celt, dt, labels):
        out.append(X2Entry(name, blk, form, len(blk), compress(ref, blk, celt, form), dt, labels))

    # every table log at limit = table log; 1, 5 and 8 again filled at 12.  Sizes: every stream holds HPAR_MIN_BITS bits (geometric codes: ~2 bits
    # per symbol; log 1: one bit), in both forms
    for t in range(1, 13):
        cnt = geometric(t)
        blk = draw(cnt, 40000 if t == 1 else 12000 + 16 * t + (t % 4), 100 + t)
        celt, dt, tl = tables(ref, cnt, t, t)
        assert tl == t, (t, tl)
        for f in (4, 1):
            add("log%d_f%d" % (t, f), blk if f == 4 else np.ascontiguousarray(blk[:len(blk) // 2 + 1]), f, celt, dt,
                ["log_%d" % t] + (["cells_under_64"] if t < 6 else []))
        if t in (1, 5, 8):
            celt, dt, _ = tables(ref, cnt, t, 12)
            f = 1 if t % 2 else 4
            add("log%d_at12_f%d" % (t, f), blk, f, celt, dt, ["log_%d_at_12" % t, "filled_above_own_log"])
    # a stretch of 1-bit codes in ONE stream of 8 KiB: every lane's share is 1024 symbols, beyond HPAR_KEEP's 160 (pass 2 decodes again)
    cnt = geometric(1)
    celt, dt, _ = tables(ref, cnt, 1, 1)
    add("spill_log1_f1", draw(cnt, 65536, 7), 1, celt, dt, ["spill"])
    cnt = geometric(3)
    celt, dt, _ = tables(ref, cnt, 3, 12)
    add("spill_log3_at12_f4", draw(cnt, 65536, 8), 4, celt, dt, ["spill"])
    # real blocks, the limit of HUF_buildCTable also the table's maxTableLog
    real = {}
    for P, size, limit in ((2, 65536, 12), (14, 32768, 11), (80, 32768, 11), (14, 45000, 12), (14, 10001, 11), (14, 11000, 11)):
        blk = np.ascontiguousarray(orc.probagen_batch(P, 1, size, 500 + P)[0])
        celt, dt, tl = tables(ref, hist(blk), limit, limit)
        real[(P, size)] = (blk, celt, dt)
    for P in (2, 14, 80):
        blk, celt, dt = real[(P, 65536 if P == 2 else 32768)]
        for form in (4, 1):
            add("p%d_f%d" % (P, form), blk, form, celt, dt, ["real_p%d" % P])
    blk, celt, dt = real[(14, 45000)]
    add("p14_45000_f4", blk, 4, celt, dt, ["one_piece_two_on_x1"])                # streams of ~6 KB
    blk, celt, dt = real[(14, 11000)]
    add("p14_11000_f1", blk, 1, celt, dt, ["one_piece_two_on_x1"])
    blk, celt, dt = real[(14, 10001)]
    add("p14_10001_f4", blk, 4, celt, dt, ["dst_not_mult4"])
    add("p14_10003_f4", np.ascontiguousarray(real[(14, 11000)][0][:10003]), 4, real[(14, 11000)][1], real[(14, 11000)][2], ["dst_not_mult4"])
    # one stream of exactly HPAR_MIN_BITS bits, and of one bit less: the shortest prefixes of a P14 block that give them
    blk, celt, dt = real[(14, 32768)]
    want = {hsim.MIN_BITS: "min_bits_at", hsim.MIN_BITS - 1: "min_bits_under"}
    for off in range(0, 30000, 1000):                                   # (a code takes several bits: not every start hits the two counts)
        for n in range(800, 1400):
            bits = stream_bits(compress(ref, blk[off:off + n], celt, 1))
            if bits in want:
                add("%s_f1" % want[bits], np.ascontiguousarray(blk[off:off + n]), 1, celt, dt, [want.pop(bits)])
            if bits > hsim.MIN_BITS:
                break
        if not want:
            break
    assert not want, want
    # streams that need repair rounds (the constructions of tests/repair_corpus.py: runs of a two-bit symbol inside a skewed background), so
    # that the rounds and bad links of the device's record say something; seeds 21 and 5 exceed HPAR_MAX_REPAIR behind a single-symbol table, and
    # with the larger pieces of this launch seed 5 still does and is handed over
    import repair_corpus as rc
    for form, seed in ((1, 26), (1, 60), (4, 6), (4, 261), (1, 21), (4, 5)):
        blk = rc.huf_bytes(orc, rc.huf_random(seed))
        celt, dt, _ = tables(ref, hist(blk), 11, 12 if seed % 2 else 11)
        add("zrun_s%d_f%d" % (seed, form), blk, form, celt, dt, [])
    return out


def shared_batch(ref, orc):
    """five blocks of one source behind ONE table (the histogram of all five): the batch calls' shared_table form"""
    blks = [np.ascontiguousarray(b) for b in orc.probagen_batch(14, 5, 9000, 900)]
    celt, dt, _ = tables(ref, hist(np.concatenate(blks)), 11, 12)
    return [X2Entry("shared_%d" % i, b, 4, len(b), compress(ref, b, celt, 4), dt, ["shared_table"]) for i, b in enumerate(blks)]


# ---------------------------------------------------------------------------------------------------------------------------- damaged tables
def _fields(w):
    return w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF, w >> 24


def _cell(s1, s2, nb, ln):
    return int(s1) | int(s2) << 8 | int(nb) << 16 | int(ln) << 24


def _nbs(cells, dtLog):
    """bits of every first symbol of a VALID table (255: absent), from its run"""
    s1 = cells & 0xFF
    n = np.bincount(s1, minlength=256)
    return np.where(n > 0, dtLog - np.log2(np.maximum(n, 1)).astype(np.int64), 255)


# damage kind -> (the rule it must break first, f(cells, i, nbs, dtLog) -> the new word of cell i or None where the cell does not allow it)
def _d_first_symbol(c, i, nbs, L):                                      # another first symbol inside a run: its symbol gets a second run
    s1 = c & 0xFF
    if i == 0 or i == len(c) - 1 or not (s1[i - 1] == s1[i] == s1[i + 1]):
        return None
    other = int(s1[(i + len(c) // 2) % len(c)])
    return None if other == s1[i] else (int(c[i]) & ~0xFF) | other


def _d_boundary(c, i, nbs, L):                                          # the run in front takes this run's first cell
    s1 = c & 0xFF
    return None if i == 0 or s1[i] == s1[i - 1] else (int(c[i]) & ~0xFF) | int(s1[i - 1])


def _d_bits1_plus(c, i, nbs, L):
    a, b, nb, ln = _fields(int(c[i]))
    return _cell(a, b, nb + 1, 1) if ln == 1 else None


def _d_bits2_minus(c, i, nbs, L):
    a, b, nb, ln = _fields(int(c[i]))
    return _cell(a, b, nb - 1, 2) if ln == 2 else None


def _d_len_2to1(c, i, nbs, L):
    a, b, nb, ln = _fields(int(c[i]))
    return _cell(a, b, nb, 1) if ln == 2 else None


def _d_len_1to2(c, i, nbs, L):                                          # (a one-symbol cell's second byte is 0: symbol 0 follows, or is absent)
    a, b, nb, ln = _fields(int(c[i]))
    return _cell(a, b, nb, 2) if ln == 1 and nbs[b] != 255 else None


def _d_absent_second(c, i, nbs, L):
    a, b, nb, ln = _fields(int(c[i]))
    absent = int(np.nonzero(nbs == 255)[0][-1])
    return _cell(a, absent, nb, 2) if ln == 2 else None


def _d_beyond_log(c, i, nbs, L):                                        # the one-symbol cell takes the symbol that really follows, whose code does not fit
    a, b, nb, ln = _fields(int(c[i]))
    if ln != 1:
        return None
    follow = int(c[(i << nb) & (len(c) - 1)]) & 0xFF
    return _cell(a, follow, nb + int(nbs[follow]), 2) if nb + nbs[follow] > L else None


def _d_swap_second(c, i, nbs, L):                                       # another second symbol of the same length
    a, b, nb, ln = _fields(int(c[i]))
    if ln != 2:
        return None
    same = [s for s in np.nonzero(nbs == nbs[b])[0] if s != b]
    return _cell(a, same[(i // 7) % len(same)], nb, 2) if same else None


def _single(c, i):
    s1 = c & 0xFF
    return 0 < i and s1[i - 1] != s1[i] and (i == len(c) - 1 or s1[i + 1] != s1[i])


def _d_relabel_run(c, i, nbs, L):                                       # a longest code's only cell takes the cell of another longest code, two cells down:
    if i < 3 or not (_single(c, i) and _single(c, i - 2)) or (int(c[i]) ^ int(c[i - 2])) >> 8:      # two runs of that symbol, and nothing else wrong
        return None
    return int(c[i - 2])


def _d_copy_next(c, i, nbs, L):                                         # a longest code's only cell becomes a copy of the one-symbol cell behind it, the first
    if i < 1 or i + 2 >= len(c) or not _single(c, i) or _single(c, i + 1) or int(c[i + 1]) >> 24 != 1:      # of a longer run (short codes come last): a run of n + 1
        return None
    return int(c[i + 1])


# The last two break ONLY their rule (the single-field damages of the same rules also break a rule behind it): a version of the derivation
# without the rule accepts them.  They are tried at every cell, not at the four positions.
ANYWHERE = ("relabel_run", "copy_next")
DAMAGES = (("first_symbol", "runs", _d_first_symbol), ("relabel_run", "runs", _d_relabel_run), ("copy_next", "pow2_aligned", _d_copy_next), ("boundary", "pow2_aligned", _d_boundary), ("bits1_plus", "len1_bits", _d_bits1_plus),
           ("len_2to1", "len1_bits", _d_len_2to1), ("absent_second", "second_present", _d_absent_second), ("bits2_minus", "len2_bits", _d_bits2_minus),
           ("len_1to2", "len2_bits", _d_len_1to2), ("beyond_log", "nbtot_le_log", _d_beyond_log), ("swap_second", "second_follows", _d_swap_second))


def _candidates(pos, ts, rs):
    if pos == "cell0":
        return [0]
    if pos == "last":
        return [ts - 1]
    off = 0 if pos == "at64k" else 17
    if ts < 64:
        return [off] if 0 < off < ts - 1 else []
    return [int(v) for v in rs.permutation(np.arange(off if off else 64, ts - 1, 64))]


def damaged_entries(ref, base, tag, positions=POSITIONS, corrupt_at=("at64k",), tries=48):
    """base: a valid X2Entry whose block visits the table widely.  One entry per damage kind and position where a cell exists that (a) the kind
    applies to, (b) breaks the kind's rule first and (c) the reference's walk looks up, so that its outcome is not (dst_size, block)."""
    out = []
    L = base.table_log
    ts = 1 << L
    cells = base.dt[1:1 + ts].astype(np.int64)
    nbs = _nbs(cells, L)
    bad_pl = base.payload.copy()
    bad_pl[len(bad_pl) // 2] ^= 0x08
    for k, (kind, clause, fn) in enumerate(DAMAGES):
        for pos in (("any",) if kind in ANYWHERE else positions):
            rs = np.random.RandomState(1000 * k + len(pos) + L)
            n_try = 0
            for i in (range(ts - 1, 0, -1) if pos == "any" else _candidates(pos, ts, rs)):
                w = fn(cells, i, nbs, L)
                if w is None:
                    continue
                dt = base.dt.copy()
                dt[1 + i] = w
                if hsim.derive_x2(dt)[:2] != (False, clause):
                    continue
                e = X2Entry("%s_%s_%s_c%d" % (tag, kind, pos, i), base.blk, base.form, base.dst_size, base.payload, dt,
                            ["declined_" + clause] + ["damage_" + pos] * (pos != "any"), "damaged_table", clause)
                r, o = e.reference(ref)
                n_try += 1
                if r != base.dst_size or not np.array_equal(o[:r], base.blk):
                    out.append(e)
                    if pos in corrupt_at:
                        out.append(X2Entry(e.name + "_badpl", base.blk, base.form, base.dst_size, bad_pl, dt, e.labels, "damaged_table", clause))
                    break
                if n_try >= tries:
                    break
    return out


def plant_first_cell(ref, blk, limit, L, form):
    """the block with runs of its longest-coded symbol (the table's FIRST cell: long codes come first, :524-537) planted in every quarter, so
    that the reference looks up cell 0 -- the last cell, all ones, is the most frequent symbol's and needs no help; returns the valid entry
    built from the planted block"""
    blk = blk.copy()
    seen = []
    for _ in range(12):                                                 # (the histogram moves with the planted bytes: until it settles)
        celt, dt, tl = tables(ref, hist(blk), limit, L)
        first = int(dt[1]) & 0xFF
        if first in seen:
            break
        seen.append(first)
        for q in range(4):
            p = (len(blk) // 4) * q + 1000 + 8 * len(seen)
            blk[p:p + 3] = first
    assert int(dt[1]) & 0xFF == first
    return X2Entry("base_L%d_f%d" % (L, form), blk, form, len(blk), compress(ref, blk, celt, form), dt, ["real_p14"] + (["filled_above_own_log"] if tl < L else []))


def special_entries(ref, base):
    """benign descriptor junk, and the CPU-only tables"""
    out = []
    dt = base.dt.copy()
    dt[0] = (int(dt[0]) & 0x00FFFF00) | 0xC3000005                      # maxTableLog as found = 5, reserved = 0xC3: nobody reads them while decoding
    out.append(X2Entry("benign_descriptor", base.blk, base.form, base.dst_size, base.payload, dt, ["benign_descriptor"], "benign"))
    ts = 1 << base.table_log
    for ln in (0, 3):
        dt = base.dt.copy()
        i = 64 * 3 + 17
        dt[1 + i] = (int(dt[1 + i]) & 0x00FFFFFF) | ln << 24
        out.append(X2Entry("len_%d" % ln, base.blk, base.form, base.dst_size, base.payload, dt, ["len_%d" % ln, "declined_len_1_or_2"],
                           "cpu_only", "len_1_or_2", cpu_only=True))
    dt = base.dt.copy()
    dt[1:1 + ts] = _cell(int(base.blk[0]), 0, 0, 1)
    out.append(X2Entry("constant_table", base.blk, base.form, base.dst_size, base.payload, dt, ["constant_table", "declined_n_lt_ts"],
                       "cpu_only", "n_lt_ts", cpu_only=True))
    return out


def payload_damages(e):
    """a flipped bit inside lane 0's range of the first stream, one in a middle lane, the payload one byte short, dst_size - 1"""
    L = len(e.payload) if e.form == 1 else int(e.payload[0]) | int(e.payload[1]) << 8
    first = 6 * (e.form == 4)

    def flip(frac):                                                     # a stream is read from its last byte down: lane 0 owns the top
        p = e.payload.copy()
        p[first + int((L - 2) * (1.0 - frac))] ^= 0x10
        return p
    mk = lambda tag, lab, pl, ds: X2Entry("%s_%s" % (e.name, tag), e.blk, e.form, ds, pl, e.dt, [lab], "damaged_payload")
    return [mk("lane0", "pl_lane0", flip(0.004), e.dst_size), mk("middle", "pl_middle", flip(0.5), e.dst_size),
            mk("short", "pl_short", e.payload[:-1].copy(), e.dst_size), mk("dstm1", "pl_dst_minus_1", e.payload, e.dst_size - 1)]


def build(ref, orc):
    valid = valid_entries(ref, orc)
    p14 = np.ascontiguousarray(orc.probagen_batch(14, 1, 20000, 514)[0])
    bases = [plant_first_cell(ref, p14, 11, 12, 4), plant_first_cell(ref, p14, 11, 11, 1)]
    small = next(e for e in valid if e.name == "log5_f4")
    out = valid + bases + shared_batch(ref, orc)
    out += damaged_entries(ref, bases[0], "d12")
    out += damaged_entries(ref, bases[1], "d11", positions=("at64k17", "last"), corrupt_at=())
    out += damaged_entries(ref, small, "d5", corrupt_at=())
    out += special_entries(ref, bases[0])
    for e in (bases[0], bases[1]):
        out += payload_damages(e)
    for e in out:
        e.labels += ["form_%d" % e.form]
        e.dt.setflags(write=False)
        e.payload.setflags(write=False)
    assert len(out) <= 150, len(out)
    assert len({e.name for e in out}) == len(out)
    return out


def labels(e, rec, rec11):
    """the entry's own labels plus what the model's walk reached at max_table_log 12 (rec) and 11 (rec11)"""
    lab = list(e.labels)
    pieces = [p for st in rec["streams"] for p in st["pieces"]]
    lab += ["repair_rounds"] * (rec["parallel"] and rec["rounds"] > 0) + ["over_max_repair"] * any(p.get("fail") == "rounds" for p in pieces)
    if rec["parallel"]:
        pcs = [len(st["pieces"]) for st in rec["streams"]]
        lab += ["two_pieces"] * (max(pcs) == 2)
        lab += ["spill"] * any(p["spill"] for st in rec["streams"] for p in st["pieces"]) if "spill" not in lab else []
    elif "spill" in lab:
        lab.remove("spill")
    if "one_piece_two_on_x1" in lab:                                    # the claim, checked: one piece at 2120 dwords, two at 1128
        big = max(st["pieces"][0]["nd"] for st in rec["streams"]) if rec["parallel"] else 0
        if not (rec["parallel"] and all(len(st["pieces"]) == 1 for st in rec["streams"]) and hsim.PDW < big <= hsim.PDW_X2):
            lab.remove("one_piece_two_on_x1")
    if e.kind == "valid":
        if e.table_log > 11:
            lab += ["limit11_too_large"] * (rec11["reason"] == "block")
        else:
            lab += ["slot_4k"] * bool(rec11["parallel"])
    return lab

"""A corpus that lands on every hand-over of the batched FSE decoder (k_fse_decode, csrc/fse_decode.hip) on purpose, each block labelled
with what it reaches.  The labels come from the schedule model (scripts/sim/fse_decode_sim.py), never from the device.
tests/test_fse_decode_corpus.py checks on the CPU that every label is reached, that the model computes what the reference computes and that
the corpus tells every broken variant of the model from the kernel's rules; tests/test_gpu_fse_decode_paths.py runs the corpus through the
device against the reference and compares the device's phase counters with the model's.

How the boundaries are hit exactly.  A block of n symbols coded with a table in which every symbol costs a fixed number of bits leaves
exactly sum(cost of symbols 0 .. n-3) unread bits after the two state reads, and every symbol decoded takes its own cost:
  * raw tables (FSE_buildCTable_raw(nb), caller path only -- they have no header): nb bits per symbol; nb = 1 reaches every value and takes
    the cell-by-cell staging of tables under 16 cells; nb = 12 is the worst case the 48*(N-1) term exists for (780 must not take a long
    phase, 792 must, its 16th iteration starting at 72);
  * flat headers (2^k symbols of normalised count 1 at table log k, k in 5..8): k bits per symbol, both paths;
  * "mix11" (table log 11: 100 symbols of count 1 = 11 bits each, 50 of count 2 = 10 bits each, the rest of the table in symbols the data
    never uses): 113 = 3*11 + 8*10 and 112 = 2*11 + 9*10, and a long phase of 64 eleven-bit symbols takes 704 bits -- the only way to sit on
    113 / 112 AFTER a long phase (a fixed cost c would need c >= 10.5 and c | 113), and the way the one-shot path reaches the prime 113.

Labels (`LABELS`; "c:" = caller tables, FSE_decompress_usingDTable; "o:" = one-shot, FSE_decompress; both where no prefix is listed):
  start_785/784/113/112      the start decision of the bit-reversed loop sits on the value (161 / 160 / 65 / 64 too: the values the broken
                             variants N-1 -> N and 65 -> 64 move the rules to)
  after_long_785/784/113/112 the decision after a long phase; after_fin_113/112 the decision after a finishing phase
  nb12_780_no_long, nb12_792_long   the raw table of 12 bits per symbol
  groups_<g>                 plenty of bits (>= 785) and dstCapacity // 4 == g, g in 0 1 2 3 15 16 17
  groups_drop_after_long     the groups fall below 16 after k >= 1 long phases with >= 785 bits left; finishing phases run on until < 2
  cap_eq_size, cap_size_m1, cap_size_m5, cap_1 .. cap_5, exit_*   the literal tail's four ways out
  rev_log_5 .. rev_log_12    bit-reversed tables from real headers by table log (12: no cell of nbBits 0; its 4096 cells take the two
                             passes of the staging: two_pass_4096)
  plain_oneshot, plain_caller_decline   table log 12 with a cell of nbBits 0: the PLAIN class / declined by launch 2, taken by launch 3
  plain_at_127, plain_at_128 the plain loop's start rule (r.at >= 128) on both sides
  plain_q_120, plain_q_124   its continuation rule (q >= 124) on both sides.  q = 4*((B + 8*inA) >> 5) - 8 is a multiple of 4, so 123 does
                             not exist: 120 is the value next below.
  log_1, log_2, log_3        caller tables under 16 cells: the cell-by-cell staging
  bad_table_*                caller tables the staging pass refuses to vouch for (a low bit OR-ed into newState where the state stays inside
                             the table): cell-by-cell, quads, two-pass and plain staging; no bulk phase, the reference's bytes
  inA_0..3, straddle_0..3, c0_variety, refills_0 / _1 / _100plus, iters_48 / _64 / _66 / _300plus, ring_wrap   the input and state rings
Not reachable, and why:
  * the plain-cell loop WITHOUT NB0 (fse_bulk_phase<false>): both launchers send only tables with a cell of nbBits 0 to that loop (the
    one-shot PLAIN class is "a counter above half the table", which makes such a cell; the caller path's third launch takes exactly the
    declined tables), so the flag is set whenever the loop runs;
  * plain_q_123 (see above).
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", "sim", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dsim = _load("fse_decode_sim")

BOUNDARY = (["start_%d" % v for v in (785, 784, 113, 112)] + ["after_long_%d" % v for v in (785, 784, 113, 112)] +
            ["after_fin_113", "after_fin_112"])
LABELS = (["c:" + b for b in BOUNDARY] + ["o:" + b for b in BOUNDARY] +
          ["c:start_161", "c:start_160", "c:start_65", "c:start_64", "o:start_161", "o:start_160", "nb12_780_no_long", "nb12_792_long"] +
          ["groups_%d" % g for g in (0, 1, 2, 3, 15, 16, 17)] + ["groups_drop_after_long", "cap_eq_size", "cap_size_m1", "cap_size_m5"] +
          ["cap_%d" % c for c in range(1, 6)] + ["exit_state1_last", "exit_state2_last", "exit_tooSmall_1", "exit_tooSmall_2"] +
          ["rev_log_%d" % k for k in range(5, 13)] + ["two_pass_4096", "plain_oneshot", "plain_caller_decline", "plain_at_127", "plain_at_128",
                                                      "plain_q_120", "plain_q_124", "log_1", "log_2", "log_3"] +
          ["bad_table_cellwise", "bad_table_quads", "bad_table_two_pass", "bad_table_plain"] +
          ["inA_%d" % k for k in range(4)] + ["straddle_%d" % k for k in range(4)] +
          ["c0_variety", "refills_0", "refills_1", "refills_100plus", "iters_48", "iters_64", "iters_66", "iters_300plus", "ring_wrap"] +
          ["damaged_truncated", "damaged_bitflip", "damaged_zero_tail"])
UNREACHABLE = {"plain_without_NB0": "both launchers send only tables with a cell of nbBits 0 to the plain-cell loop",
               "plain_q_123": "q is a multiple of 4; 120 is the value next below 124"}
SEARCH = {}                       # what the candidate search for the plain loop's rules found (filled by build())
BATCH_CAPS = (33000, 67)          # capacities of the runs that decode the whole corpus in one call (one capacity per call): everything fits / 16 groups


class Block:
    """payload + reference-layout DTable (+ the header the one-shot path reads the table from); `caps`: the capacities it is decoded with
    alone; `off`: its row's address modulo 64 when it is decoded alone"""

    def __init__(self, name, payload, dt, n, caps=None, header=None, off=0, kind="", src=None):
        self.name, self.n, self.off, self.kind = name, n, off, kind
        self.payload = np.ascontiguousarray(payload, dtype=np.uint8)
        self.dt = np.ascontiguousarray(dt, dtype=np.uint32)
        self.header = None if header is None else np.ascontiguousarray(header, dtype=np.uint8)
        self.caps = [n] if caps is None else list(caps)
        self.table = dsim.DTable(self.dt)
        self.src = src
        self._sims = {}

    @property
    def routes(self):
        return ("caller", "oneshot") if self.header is not None else ("caller",)

    @property
    def loop(self):
        return self.table.loop()

    def oneshot_bytes(self):
        return np.concatenate([self.header, self.payload])

    def payload_addr(self, route, row_addr):
        return (row_addr + (len(self.header) if route == "oneshot" else 0)) & 63

    def sim(self, cap, route="caller", row_addr=None, mut=None):
        addr = self.payload_addr(route, self.off if row_addr is None else row_addr)
        key = (cap, addr, mut)
        if key not in self._sims:
            self._sims[key] = dsim.simulate(self.payload, self.table, cap, addr, mut=mut)
        return self._sims[key]


# ------------------------------------------------------------------------------------------------------------------------------ builders
def _rs(*key):
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k)) % ((1 << 31) - 1)
    return np.random.RandomState(seed)


def raw_block(orc, name, nb, n, caps=None, off=0, seed=1):
    _, ct = orc.fse_build_ctable_raw(nb)
    _, dt = orc.fse_build_dtable_raw(nb)
    src = _rs(nb, n, seed).randint(0, min(256, 1 << nb), n).astype(np.uint8)
    r, out = orc.fse_compress_using_ctable(src, ct)
    assert 0 < r < (1 << 63), (name, r)
    return Block(name, out[:r], dt, n, caps, None, off, "raw%d" % nb, src)


def norm_block(orc, name, norm, msv, tl, src, caps=None, off=0, kind="norm", header=True):
    norm = np.asarray(norm, dtype=np.int16)
    r, ct = orc.fse_build_ctable(norm, msv, tl)
    assert r == 0, (name, r)
    r, dt = orc.fse_build_dtable(norm, msv, tl)
    assert r == 0, (name, r)
    h, hdr = orc.fse_write_ncount(512, norm, msv, tl) if header else (0, None)      # (table logs under 5 have no header format)
    assert not header or 0 < h < 512, (name, h)
    r, out = orc.fse_compress_using_ctable(src, ct)
    assert 0 < r < (1 << 63), (name, r)
    return Block(name, out[:r], dt, len(src), caps, hdr[:h] if header else None, off, kind, src)


def flat_block(orc, name, k, n, caps=None, off=0, seed=1):
    """2^k symbols of normalised count 1 at table log k: every symbol costs k bits"""
    src = _rs(k, n, seed).randint(0, 1 << k, n).astype(np.uint8)
    return norm_block(orc, name, np.ones(1 << k, np.int16), (1 << k) - 1, k, src, caps, off, "flat%d" % k)


MIX11_NORM = np.array([1] * 100 + [2] * 50 + [66] + [18] * 99, np.int16)        # sums to 2048; symbols 0..99 cost 11 bits, 100..149 cost 10


def mix11_block(orc, name, costs, caps=None, off=0):
    """`costs`: 11 / 10 per symbol, in decoding order (two more symbols are appended: the last two cost nothing)"""
    assert int(MIX11_NORM.sum()) == 2048
    rs = _rs(len(costs), sum(costs))
    src = np.array([rs.randint(0, 100) if c == 11 else rs.randint(100, 150) for c in list(costs) + [11, 10]], np.uint8)
    return norm_block(orc, name, MIX11_NORM, 249, 11, src, caps, off, "mix11")


def data_bytes(orc, spec):
    kind = spec[0]
    if kind == "proba":
        return orc.probagen_batch(spec[1], 1, spec[2], spec[3])[0]
    if kind == "uniform":                              # k symbols evenly
        return _rs(spec[1], spec[2], spec[3]).randint(0, spec[1], spec[2]).astype(np.uint8)
    if kind == "dominant":                             # symbol 0 with probability p, k others evenly
        _, p, k, size, seed = spec
        rs = _rs(k, size, seed)
        out = rs.randint(1, k + 1, size).astype(np.uint8)
        out[rs.random_sample(size) < p] = 0
        return out
    raise ValueError(kind)


def data_block(orc, name, spec, tl, caps=None, off=0):
    """the reference's own table for the data at table log `tl` (FSE_normalizeCount, FSE_buildCTable / DTable, FSE_writeNCount)"""
    src = data_bytes(orc, spec)
    mx, msv, cnt = orc.hist_count(src)
    r, norm = orc.fse_normalize_count(tl, cnt, len(src), msv)
    assert r == tl, (name, r)
    return norm_block(orc, name, norm[:msv + 1], msv, tl, src, caps, off, "data%d" % tl)


def bad_table(blk, name):
    """the block with a table the staging pass must refuse to vouch for: bit 0 set in newState of every third cell with nbBits >= 1 and
    newState + (1 << nbBits) < tableSize -- every reachable state stays inside the table, which is what the reference itself needs"""
    dt = blk.dt.copy()
    ts = 1 << blk.table.tl
    k = 0
    for i in range(ts):
        nb, ns = int(dt[1 + i]) >> 24, int(dt[1 + i]) & 0xFFFF
        if nb >= 1 and ns + (1 << nb) < ts:
            if k % 3 == 0:
                dt[1 + i] |= 1
            k += 1
    assert k > 0, name
    b = Block(name, blk.payload, dt, blk.n, [blk.n + 64, blk.n // 2], None, blk.off, "bad")
    assert b.table.bad and all(n < ts for n in b.table.ns) and b.table.fast == blk.table.fast
    return b


def damaged(blk, name, how):
    p = blk.payload.copy()
    if how == "truncated":
        p = p[:len(p) * 2 // 3]
        if p[-1] == 0:
            p[-1] = 1                                  # (a zero last byte is its own case)
    elif how == "bitflip":
        p[len(p) // 2] ^= 0x10
    elif how == "zero_tail":
        p[-1] = 0
    return Block(name, p, blk.dt, blk.n, [blk.n], blk.header, blk.off, "damaged_" + how)


# ------------------------------------------------------------------------------------------------------------------------------ the corpus
def build(orc):
    """-> (blocks, company): the blocks in corpus order; company: name -> (max_table_log, [block, ...]) workgroups of the caller path"""
    B = []
    add = B.append
    off = [0]

    def nxt():                                          # row addresses: every residue modulo 4, many modulo 64
        off[0] = (off[0] + 13) & 63
        return off[0]

    # ---- the bit-reversed loop's rules on their values: raw tables of 1 bit per symbol (start; after a long phase of 64 bits; after a
    #      finishing phase of 8), of 5 and of 12
    for n in (787, 786, 115, 114, 67, 66, 163, 162):
        add(raw_block(orc, "raw1_start_%d" % (n - 2), 1, n, off=nxt()))
    for n in (851, 850, 123, 122, 915, 914):
        add(raw_block(orc, "raw1_n%d" % n, 1, n, off=nxt()))
    for inA in range(4):                               # 113 - 8*inA .. 112 after a phase, payload at every address modulo 4
        for n in (123, 122, 121, 120, 119, 118, 117, 116, 851, 850, 849, 848):
            add(raw_block(orc, "raw1_n%d_a%d" % (n, inA), 1, n, off=16 * inA + inA, seed=2 + inA))
    for inA in (1, 2, 3):                              # just under a start rule by less than 8*inA bits
        for n in (114, 106, 786, 770):
            add(raw_block(orc, "raw1_under_n%d_a%d" % (n, inA), 1, n, off=32 + inA, seed=7))
    for n in (159, 158, 34, 35, 15, 14, 287, 273, 209, 700, 1300):
        add(raw_block(orc, "raw5_n%d" % n, 5, n, off=nxt()))
    for n in (5, 67, 68, 131, 132, 400):
        add(raw_block(orc, "raw12_n%d" % n, 12, n, off=nxt()))
    for nb, sizes in ((2, (10, 60, 400, 1200)), (3, (9, 45, 300, 900)), (1, (3, 4, 5, 9, 2500))):
        for n in sizes:
            add(raw_block(orc, "raw%d_n%d" % (nb, n), nb, n, off=nxt()))
    # ---- the same from flat headers: both paths
    for k, sizes in ((5, (159, 158, 34, 35, 223, 222, 600)), (6, (130, 131, 132, 133, 300)), (7, (114, 115, 25, 24, 18, 19, 178, 179, 82, 83, 20, 21, 500)),
                     (8, (100, 101, 164, 165, 16, 400))):
        for n in sizes:
            add(flat_block(orc, "flat%d_n%d" % (k, n), k, n, off=nxt()))
    # ---- mixed costs: 113 and 112 at the start, after a long phase and after a finishing phase, both paths
    c113, c112 = [11] * 3 + [10] * 8, [11] * 2 + [10] * 9
    for tag, tailc in (("113", c113), ("112", c112)):
        add(mix11_block(orc, "mix11_start_" + tag, tailc, off=nxt()))
        add(mix11_block(orc, "mix11_after_long_" + tag, [11] * 64 + tailc, off=nxt()))
        add(mix11_block(orc, "mix11_after_2long_" + tag, [11] * 64 + [11] * 40 + [10] * 24 + tailc, off=nxt()))
        add(mix11_block(orc, "mix11_after_fin_" + tag, [11, 10] * 4 + tailc, off=nxt()))
        add(mix11_block(orc, "mix11_after_long_fin_" + tag, [11] * 64 + [10] * 8 + tailc, off=nxt()))
    # ---- room in the destination: plenty of bits, few groups
    roomy = 2000
    caps = [0, 1, 2, 3, 4, 5, 8, 11, 12, 15, 60, 63, 64, 67, 68, 71, 4 * 37, 4 * 63 + 1, 4 * 48 + 3, 4 * 64, 4 * 66, 4 * 130 + 2,
            roomy, roomy - 1, roomy - 2, roomy - 5, roomy - 6, roomy + 3]
    add(raw_block(orc, "raw5_roomy", 5, roomy, caps=caps, off=nxt()))
    add(flat_block(orc, "flat7_roomy", 7, 1500, caps=[0, 3, 4, 7, 8, 12, 61, 64, 70, 4 * 21, 4 * 34 + 1, 1500, 1499, 1498, 1495, 1494], off=nxt()))
    # ---- real tables by table log, both paths; capacity around the size
    for tl in range(5, 13):
        for j, (P, size) in enumerate(((20, 3000), (50, 1777), (80, 3999))):
            if tl < 8:                                  # (few symbols: the normalisation must fit the small table)
                spec = (("uniform", 1 << (tl - 2), size, 7), ("uniform", 3, size, 8), ("dominant", 0.6, 1 << (tl - 3), size, 9))[j]
            else:
                spec = ("proba", P, size, 11 * tl + j)
            add(data_block(orc, "data_tl%d_%d" % (tl, j), spec, tl, caps=[size, size - 1, size - 5, size + 1] if j == 0 else None, off=nxt()))
    # ---- input ring: payloads of about 170 bytes (never refilled), of about 230 (once), at every (S + inA) & 3
    for n in range(268, 276):
        add(raw_block(orc, "raw5_ring_n%d" % n, 5, n, off=nxt()))
    for n in range(368, 372):
        add(raw_block(orc, "raw5_ring_n%d" % n, 5, n, off=nxt()))
    # ---- table log 12 with a cell of nbBits 0: the plain-cell loop.  Its two rules' values come from a search over a fixed candidate list
    cands = [data_block(orc, "plain_n%d" % n, ("dominant", 0.75, 8, n, 5), 12, off=0) for n in range(640, 900, 2)]
    want = {"plain_at_127": None, "plain_at_128": None, "plain_q_120": None, "plain_q_124": None}
    for c in cands:
        assert c.loop == "plain", c.name
        d = c.sim(c.n)["decisions"]
        if d and d[0]["at"] in (127, 128) and want["plain_at_%d" % d[0]["at"]] is None:
            want["plain_at_%d" % d[0]["at"]] = c
        if len(d) > 1 and d[1]["q"] in (120, 124) and want["plain_q_%d" % d[1]["q"]] is None:
            want["plain_q_%d" % d[1]["q"]] = c
    for c in dict.fromkeys(v for v in want.values() if v is not None):
        add(c)
    SEARCH["found"] = {k: (v.name if v is not None else None) for k, v in want.items()}
    SEARCH["at_reached"] = sorted({c.sim(c.n)["decisions"][0]["at"] for c in cands})
    SEARCH["q_reached"] = sorted({d["q"] for c in cands for d in c.sim(c.n)["decisions"][1:2]})
    add(data_block(orc, "plain_3000", ("dominant", 0.8, 12, 3000, 3), 12, caps=[3000, 2999, 64, 3], off=nxt()))
    add(data_block(orc, "plain_3900_a3", ("dominant", 0.6, 30, 3900, 4), 12, off=3))
    # ---- tables the staging pass refuses to vouch for (caller path only)
    by = {b.name: b for b in B}
    # (the table builders start at table log 5: a table of 8 cells is written out by hand -- symbol 0 in four cells of 1 bit, symbols 1 and 2
    #  in two cells of 2 bits each -- and decodes a stream of random bytes, as any complete table does)
    cells = [(0, 1, 0), (1, 2, 0), (0, 1, 2), (2, 2, 0), (0, 1, 4), (1, 2, 4), (0, 1, 6), (2, 2, 4)]
    dt3 = np.array([3 | (1 << 16)] + [ns | (sy << 16) | (nb << 24) for sy, nb, ns in cells], np.uint32)
    stream = _rs(3, 3, 3).randint(0, 256, 300).astype(np.uint8)
    stream[-1] |= 0x40
    hand = Block("hand_tl3", stream, dt3, 2600, [2600, 700], None, nxt(), "hand")
    assert not hand.table.bad
    add(hand)
    add(bad_table(hand, "bad_tl3"))
    add(bad_table(by["data_tl9_0"], "bad_tl9"))
    add(bad_table(by["data_tl11_2"], "bad_tl11"))
    add(bad_table(by["data_tl12_0"], "bad_tl12"))
    add(bad_table(by["plain_3000"], "bad_tl12_plain"))
    # ---- damaged streams
    for base in ("data_tl11_0", "data_tl9_1", "data_tl12_1", "raw5_n700", "plain_3000"):
        for how in ("truncated", "bitflip", "zero_tail"):
            add(damaged(by[base], "%s_%s" % (base, how), how))
    # ---- the few large ones: 32 KB blocks (hundreds of phases, more than 100 refills), and the one-shot path's last size bin
    add(data_block(orc, "big11", ("proba", 20, 32768, 901), 11, off=5))
    add(data_block(orc, "big12", ("proba", 14, 32768, 902), 12, off=9))
    for j, tl in enumerate((11, 11, 12)):
        add(data_block(orc, "last_bin_%d" % j, ("uniform", 250, 32768, 910 + j), tl, off=nxt()))
    for j in range(5):                                 # compressed sizes of 2 .. 4 KiB: the one-shot path's second size bin
        add(data_block(orc, "bin1_%d" % j, ("uniform", 128, 2900 + 150 * j, 920 + j), 11, off=nxt()))
    by = {b.name: b for b in B}

    # ---- company: workgroups of the caller path in block order (slot g -> decoder wave g // ppw).  Blocks that finish after 0, 1, 2, ..
    #      phases, damaged streams among them, share a wave with one 32 KB block and ride along as zombies for hundreds of rounds.
    small11 = ["raw1_start_785", "raw1_start_113", "raw1_start_112", "raw5_n287", "data_tl11_0_truncated", "raw5_n15", "mix11_after_long_113",
               "data_tl9_1_bitflip", "flat7_n178", "data_tl11_0_zero_tail", "raw1_n5", "data_tl5_0", "raw5_n700_bitflip", "flat5_n223", "raw2_n400"]
    tail11 = ["raw5_n1300", "raw1_n2500", "flat8_n400", "data_tl10_1", "raw5_n273", "raw3_n9", "data_tl9_1_truncated", "mix11_start_112",
              "data_tl8_2", "raw5_n209", "flat6_n300", "raw1_n4", "data_tl7_1", "raw5_n700_zero_tail", "data_tl6_0", "raw5_n34"]
    company = {
        # slot 0 and slot 17 (the first slots of the two decoder waves) enter the bulk: both waves' rounds are counted
        "wg11_a": (11, [by[n] for n in ["data_tl11_1"] + small11 + ["big11"] + tail11]),
        # slot 17 never enters the bulk (5 symbols): wave 1 runs its rounds, but the counter it adds is that lane pair's -- zero
        "wg11_b": (11, [by[n] for n in ["data_tl11_1"] + small11 + ["big11", "raw1_n5"] + tail11[1:]]),
        # maxTableLog 12: the 4 KiB class's launch finds none of its tables here and returns; the 8 KiB class takes 18 slots a workgroup,
        # declines the two tables with a cell of nbBits 0 and leaves them to the plain-cell launch
        "wg12": (12, [by[n] for n in ["raw12_n68", "raw12_n5", "data_tl12_1_bitflip", "raw12_n400", "data_tl12_1_truncated", "raw12_n131",
                                      "data_tl12_1_zero_tail", "raw12_n67", "big12",
                                      "data_tl12_2", "plain_3000", "data_tl12_1", "raw12_n400", "plain_3900_a3", "data_tl12_0", "raw12_n68",
                                      "raw12_n132", "raw12_n67"]]),
    }
    assert len(company["wg11_a"][1]) == 33 and len(company["wg11_b"][1]) == 33 and len(company["wg12"][1]) == 18
    return B, company


# ------------------------------------------------------------------------------------------------------------------------------ labels
def labels(blk):
    """the labels one block reaches when it is decoded alone at its own capacities and row address, per route"""
    out = set()
    t = blk.table
    for route in blk.routes:
        pre = "c:" if route == "caller" else "o:"
        for cap in blk.caps:
            s = blk.sim(cap, route)
            plenty = cap >= blk.n
            for d in s["decisions"]:
                if s["loop"] == "rev" and plenty:
                    out.add("%s%s_%d" % (pre, d["kind"], d["B"]))
                if s["loop"] == "rev" and d["kind"] == "start" and d["B"] >= 785 and blk.kind.startswith(("raw", "flat")):
                    out.add("groups_%d" % d["groups"])
                if s["loop"] == "plain" and d["kind"] == "start" and plenty:
                    out.add("plain_at_%d" % d["at"])
                if s["loop"] == "plain" and d["kind"] == "after_long" and plenty:
                    out.add("plain_q_%d" % d["q"])
            dl = [d for d in s["decisions"] if d["kind"] == "after_long" and d["B"] >= 785 and d["groups"] < 16]
            if dl and s["nFin"] >= 1 and s["decisions"][-1]["groups"] < 2:
                out.add("groups_drop_after_long")
            if blk.kind == "raw12" and plenty and s["decisions"]:
                if s["decisions"][0]["B"] == 780 and s["nLong"] == 0:
                    out.add("nb12_780_no_long")
                if s["decisions"][0]["B"] == 792 and s["nLong"] == 1 and s["heads"][15] == 72:
                    out.add("nb12_792_long")
            if not blk.kind.startswith(("damaged", "bad")):
                if cap == blk.n: out.add("cap_eq_size")
                if cap == blk.n - 1: out.add("cap_size_m1")
                if cap == blk.n - 5: out.add("cap_size_m5")
                if 1 <= cap <= 5 and blk.n > 100: out.add("cap_%d" % cap)
                out.add("exit_" + s["exit"])
            if s["everBulk"]:
                out.add("inA_%d" % s["inA"]); out.add("straddle_%d" % s["straddle"])
                if s["refills"] == 0 and len(blk.payload) >= 150: out.add("refills_0")
                if s["refills"] == 1: out.add("refills_1")
                if s["refills"] > 100: out.add("refills_100plus")
                if s["iters"] in (48, 64, 66): out.add("iters_%d" % s["iters"])
                if s["iters"] >= 300: out.add("iters_300plus")
                if s["wraps"]: out.add("ring_wrap")
                if s["loop"] == "rev" and blk.kind.startswith("data") and plenty:
                    out.add("rev_log_%d" % t.tl)
                    if t.tl == 12 and route == "caller": out.add("two_pass_4096")
                if s["loop"] == "plain" and plenty:
                    out.add("plain_oneshot" if route == "oneshot" else "plain_caller_decline")
                if route == "caller" and t.tl <= 3: out.add("log_%d" % t.tl)
            if blk.kind == "bad":
                assert not s["everBulk"]
                out.add("bad_table_plain" if s["loop"] == "plain" else "bad_table_two_pass" if t.tl == 12 else
                        "bad_table_quads" if t.tl >= 4 else "bad_table_cellwise")
            if blk.kind.startswith("damaged_"):
                out.add(blk.kind)
    return out


def oneshot_bins(blocks):
    """compressed-size bins (csize >> FSE_DBIN_LOG, the last one open-ended) of the blocks that carry a header, per decoder class"""
    bins = {}
    for b in blocks:
        if b.header is None:
            continue
        cls = "plain" if b.loop == "plain" else "rev12" if b.table.tl > dsim.FSE_DEC_FAST_MAXLOG else "rev11"
        k = min((len(b.header) + len(b.payload)) >> dsim.FSE_DBIN_LOG, 15)
        bins.setdefault(cls, {}).setdefault(k, []).append(b)
    return bins


# ------------------------------------------------------------------------------------------------------------------------------ device batches
def device_rows(torch, rows, stride_pad, off):
    """byte rows on the device with a row stride of max(len) + stride_pad and the first row `off` bytes above a 256-byte boundary
    -> (2-D tensor view, sizes tensor, row addresses modulo 64)"""
    w = max(max(len(r) for r in rows), 1) + stride_pad
    host = np.zeros((len(rows), w), np.uint8)
    for i, r in enumerate(rows):
        host[i, :len(r)] = r
    buf = torch.zeros(len(rows) * w + 512, dtype=torch.uint8, device="cuda")
    base = (-buf.data_ptr()) % 256 + off
    view = buf[base:base + len(rows) * w].view(len(rows), w)
    view.copy_(torch.from_numpy(host))
    sizes = torch.tensor([len(r) for r in rows], dtype=torch.int64, device="cuda")
    addrs = [(view.data_ptr() + i * w) & 63 for i in range(len(rows))]
    return view, sizes, addrs


def device_tables(torch, blocks, mtl):
    dt = np.zeros((len(blocks), 1 + (1 << mtl)), np.uint32)
    for i, b in enumerate(blocks):
        dt[i, :len(b.dt)] = b.dt
    return torch.from_numpy(dt).cuda()

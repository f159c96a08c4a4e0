"""Schedule model of k_fse_decode (csrc/fse_decode.hip): which phases one block takes and what the kernel hands back to its literal tail.

The kernel is exact only if a chain of hand-overs is exact: long phases of FSE_CHECK_EVERY iterations, finishing phases of FSE_FINISH_EVERY
(bit-reversed loop only), the literal tail (fse_tail), and the reader state (ptr, bitsConsumed) rebuilt from two bit cursors when the bulk
ends.  Each hand-over is one inequality in k_fse_decode; this file restates them, one line each, in `simulate()`:

    bit-reversed loop  start       Bstart >= 65 + 48*(N-1) and groups0 >= N          N = 16 (long), N = 2 (finishing)
                       after       Bp     >= 65 + 48*(N-1) and grp     >= N          Bp = unread bits of the payload proper (8*inA taken out)
    plain-cell loop    start       r.at   >= 24 + 6*16 + 8 and groups0 >= 16
                       after       q      >= 24 + 6*16 + 4 and grp     >= 16         q = 4*((B + 8*inA) >> 5) - 8: a multiple of 4
    hand-back          Bh = unread bits at the head of the last iteration taken (plain loop: B now); at = ((Bh + 7) >> 3) - 8;
                       used = 8*(at + 8) - B

The model takes one block -- payload bytes, a reference-layout DTable (u32 words: header {u16 tableLog; u16 fastMode}, cells {u16 newState;
u8 symbol; u8 nbBits}, lib/fse.h:565-575), dstCapacity, the payload's address modulo 64, and which loop runs -- and walks it serially as the
reference does: BIT_initDStream, the two FSE_initDState, the four-symbol loop (lib/fse_decompress.c:201-218) and the end game (:222-235), the
reader a literal restatement of lib/bitstream.h:272-448 (csrc/bitreader.h).  The bulk iterations are decoded the way the kernel decodes them,
by absolute bit position and without a reader; everything after the hand-back runs from the REBUILT reader state, so a wrong hand-over shows
in the result or the bytes as it would on the device.  `mut` names a deliberately broken variant (MUTANTS) for tests/test_fse_decode_corpus.py.

What it returns (a dict): result (the reference's size_t), out (bytes), everBulk, nLong, nFin, iters = 16*nLong + 2*nFin, decisions (one
record per phase decision: kind, the deciding value of B -- r.at / q for the plain loop -- and the groups left, and what was decided),
tailIters (iterations of the four-symbol loop left to fse_tail), exit (which end-game exit), handback = (at, used) or None, heads (B at every
loop head), wraps (iters > FSE_DEC_RING: the state ring wraps), and the input ring's facts: inA, c0, validLo0, refills (64-byte chunks
until validLo <= 0), straddle = (S + inA) & 3 (non-zero: the topmost dword of the initial fill is assembled from bytes).
"""
import numpy as np

# the kernel's constants, by name (tests/test_fse_decode_corpus.py parses the #defines of fse_decode.hip and internal.h and compares)
FSE_CHECK_EVERY = 16
FSE_FINISH_EVERY = 2
FSE_DEC_RING = 64
FSE_IN_RING = 256
FSE_IN_CHUNK = 64
FSE_FLUSH_MIN = 32
FSE_DBIN_LOG = 11
FSE_DEC_FAST_MAXLOG = 11
FSE_DEC_WAVES = 2            # decoder waves per workgroup: slot g of a workgroup of G goes to wave g // ceil(G / FSE_DEC_WAVES)

M64 = (1 << 64) - 1
ERR = {"GENERIC": 1, "dstSize_tooSmall": 2, "srcSize_wrong": 3, "corruption_detected": 4, "tableLog_tooLarge": 5}


def ferr(name):
    return (1 << 64) - ERR[name]


MUTANTS = {
    "head_64": "a loop head needs 64 unread bits, not 65",
    "head_66": "a loop head needs 66 unread bits, not 65",
    "per_iter_47": "an iteration is taken to need 47 bits at most, not 48",
    "n_not_minus_1": "a phase of N iterations asks for 65 + 48*N bits, not 65 + 48*(N-1)",
    "fin_on_aligned_B": "the finishing rule after a phase is evaluated on B with the 8*inA bits of the aligned base left in",
    "long_on_aligned_B": "the long rule after a phase is evaluated on B with the 8*inA bits of the aligned base left in",
    "groups_plus_1": "one output group too many is counted",
    "groups_minus_1": "one output group too few is counted",
    "gt_long_bits": "the long rule's bits are compared with > instead of >=",
    "gt_fin_bits": "the finishing rule's bits are compared with > instead of >=",
    "gt_long_groups": "the long rule's groups are compared with > instead of >=",
    "gt_fin_groups": "the finishing rule's groups are compared with > instead of >=",
    "phead_at_phase_head": "Phead is taken at the head of the phase, not at the head of its last iteration",
    "plain_start_no_8": "the plain loop's start rule drops its +8",
    "plain_after_no_4": "the plain loop's continuation rule drops its +4",
    "gt_plain_start": "the plain loop's start rule is compared with > instead of >=",
    "gt_plain_after": "the plain loop's continuation rule is compared with > instead of >=",
    "gt_plain_groups": "the plain loop's groups are compared with > instead of >=",
    "start_on_aligned_B": "the start rules are evaluated on B with the 8*inA bits of the aligned base left in",
    "groups_from_olimit": "the groups are counted up to omax - 3: (dstCapacity - 3) / 4",
    "handback_floor": "the rebuilt ptr rounds the bits at the last loop head down to bytes, not up",
}


class DTable:
    """a reference-layout DTable taken apart"""

    def __init__(self, dt):
        dt = np.ascontiguousarray(dt, dtype=np.uint32)
        self.tl = int(dt[0]) & 0xFFFF
        self.fast = (int(dt[0]) >> 16) != 0
        ts = 1 << self.tl
        cells = dt[1:1 + ts]
        self.ns = (cells & 0xFFFF).astype(np.int64).tolist()
        self.sym = ((cells >> 16) & 0xFF).astype(np.int64).tolist()
        self.nb = (cells >> 24).astype(np.int64).tolist()
        # what the staging pass checks while the table passes through (FSE_buildDTable's guarantees, lib/fse_decompress.c:113-124)
        self.bad = any((n >> self.tl) != 0 or b > self.tl or (n & ((1 << min(b, 15)) - 1)) != 0 for n, b in zip(self.ns, self.nb))
        self.nb0 = any(b == 0 for b in self.nb)

    def loop(self):
        """the loop the launchers send this table to: tableLog 12 with a cell of nbBits 0 is the plain-cell loop's"""
        return "plain" if self.tl > FSE_DEC_FAST_MAXLOG and self.nb0 else "rev"


class Reader:
    """csrc/bitreader.h, itself lib/bitstream.h:272-448"""
    UNFINISHED, END_OF_BUFFER, COMPLETED, OVERFLOW = 0, 1, 2, 3

    def __init__(self, payload):
        self.n = len(payload)
        self.V = int.from_bytes(bytes(payload), "little")
        self.at, self.used, self.win = 0, 0, 0

    def _load(self):
        self.win = (self.V >> (8 * self.at)) & M64

    def init(self, payload):
        n = self.n
        if n < 1:
            return ferr("srcSize_wrong")
        last = int(payload[n - 1])
        if n >= 8:
            self.at = n - 8
            self._load()
            if last == 0:
                return ferr("GENERIC")
            self.used = 8 - (last.bit_length() - 1)
        else:
            self.at = 0
            self._load()
            if last == 0:
                return ferr("corruption_detected")
            self.used = 8 - (last.bit_length() - 1) + (8 - n) * 8
        return n

    def read(self, nb):
        v = (self.win >> ((64 - self.used - nb) & 63)) & ((1 << nb) - 1)
        self.used += nb
        return v

    def read_fast(self, nb):
        v = ((((self.win << (self.used & 63)) & M64) >> ((64 - nb) & 63))) & 0xFFFFFFFF
        self.used += nb
        return v

    def reload(self):
        if self.used > 64:
            return self.OVERFLOW
        if self.at >= 8:
            self.at -= self.used >> 3
            self.used &= 7
            self._load()
            return self.UNFINISHED
        if self.at == 0:
            return self.END_OF_BUFFER if self.used < 64 else self.COMPLETED
        nbytes, res = self.used >> 3, self.UNFINISHED
        if self.at < nbytes:
            nbytes, res = self.at, self.END_OF_BUFFER
        self.at -= nbytes
        self.used -= nbytes * 8
        self._load()
        return res

    def unread(self):
        return 8 * (self.at + 8) - self.used


def simulate(payload, dt, cap, addr=0, loop=None, mut=None):
    assert mut is None or mut in MUTANTS, mut
    t = dt if isinstance(dt, DTable) else DTable(dt)
    loop = t.loop() if loop is None else loop
    rev = loop == "rev"
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    S = len(payload)
    inA = addr & 3
    rec = dict(loop=loop, everBulk=False, nLong=0, nFin=0, iters=0, decisions=[], tailIters=0, exit=None, handback=None, heads=[],
               wraps=False, inA=inA, c0=None, validLo0=None, refills=0, straddle=(S + inA) & 3, result=None, out=b"", bad=t.bad)
    r = Reader(payload)
    e = r.init(payload)
    if e > (1 << 64) - 9:
        rec["result"] = e
        return rec
    ns, sym, nbs, fast = t.ns, t.sym, t.nb, t.fast
    s1 = r.read(t.tl); r.reload()
    s2 = r.read(t.tl); r.reload()
    out = bytearray()
    omax = cap

    # ---- the kernel's rules (k_fse_decode, "bulk eligibility" and the two round loops) ----
    head = 64 if mut == "head_64" else 66 if mut == "head_66" else 65
    per = 47 if mut == "per_iter_47" else 48
    less = 0 if mut == "n_not_minus_1" else 1

    def need(N):
        return head + per * (N - less)

    def bits_ok(B, N):
        strict = mut == ("gt_long_bits" if N == FSE_CHECK_EVERY else "gt_fin_bits")
        return B > need(N) if strict else B >= need(N)

    def groups_ok(g, N):
        strict = mut == ("gt_long_groups" if N == FSE_CHECK_EVERY else "gt_fin_groups")
        return g > N if strict else g >= N

    bulk_ok = not t.bad
    Bstart = r.unread() if bulk_ok else 0
    groups0 = (omax - 3 + 3) // 4 + (1 if mut == "groups_plus_1" else -1 if mut == "groups_minus_1" else 0)
    if mut == "groups_from_olimit":
        groups0 = max(omax - 3, 0) // 4
    Brule = Bstart + 8 * inA if mut == "start_on_aligned_B" and bulk_ok else Bstart
    pg = (lambda g: g > FSE_CHECK_EVERY) if mut == "gt_plain_groups" else (lambda g: g >= FSE_CHECK_EVERY)
    dec = rec["decisions"]
    if rev:
        can = bulk_ok and bits_ok(Brule, FSE_CHECK_EVERY) and groups_ok(groups0, FSE_CHECK_EVERY)
        can2 = bulk_ok and bits_ok(Brule, FSE_FINISH_EVERY) and groups_ok(groups0, FSE_FINISH_EVERY)
        if bulk_ok:
            dec.append(dict(kind="start", B=Bstart, groups=groups0, long=can, fin=can2))
    else:
        lim = 24 + 6 * FSE_CHECK_EVERY + (0 if mut == "plain_start_no_8" else 8)
        can = bulk_ok and (r.at > lim if mut == "gt_plain_start" else r.at >= lim) and pg(groups0)
        can2 = False
        if bulk_ok:
            dec.append(dict(kind="start", at=r.at, B=Bstart, groups=groups0, long=can, fin=False))
    ever = can or can2
    rec["everBulk"] = ever
    B = Bstart
    Bhead = B
    grp = groups0
    V = r.V
    state = [s1, s2]

    def phase(N):
        """N iterations of lib/fse_decompress.c:201-218 by absolute bit position; returns B at the head of the phase and of its last iteration"""
        nonlocal B
        first = B
        last = B
        for it in range(N):
            last = B
            rec["heads"].append(B)
            for k in (0, 1, 0, 1):
                st = state[k]
                nb = nbs[st]
                out.append(sym[st])
                B -= nb
                bits = ((V >> B) if B >= 0 else (V << -B)) & ((1 << nb) - 1)
                state[k] = ns[st] + bits
        return first, last

    if ever:
        Ba = B + 8 * inA                                       # unread bits counted from the aligned base
        q = 4 * (Ba >> 5) - 8
        c0 = (0 - (addr - inA)) & (FSE_IN_CHUNK - 1)
        vlo = ((q + 8 - 112 - c0) & ~(FSE_IN_CHUNK - 1)) + c0
        rec["c0"], rec["validLo0"] = c0, vlo
        rec["refills"] = (vlo + FSE_IN_CHUNK - 1) // FSE_IN_CHUNK if vlo > 0 else 0
        iters = 0
        if rev:
            while can:
                first, last = phase(FSE_CHECK_EVERY)
                Bhead = first if mut == "phead_at_phase_head" else last
                iters += FSE_CHECK_EVERY; grp -= FSE_CHECK_EVERY; rec["nLong"] += 1
                BL = B + 8 * inA if mut == "long_on_aligned_B" else B
                BF = B + 8 * inA if mut == "fin_on_aligned_B" else B
                canN = bits_ok(BL, FSE_CHECK_EVERY) and groups_ok(grp, FSE_CHECK_EVERY)
                more = canN or (bits_ok(BF, FSE_FINISH_EVERY) and groups_ok(grp, FSE_FINISH_EVERY))
                dec.append(dict(kind="after_long", B=B, groups=grp, long=canN, fin=more and not canN))
                can = canN
            BF = B + 8 * inA if mut == "fin_on_aligned_B" else B
            # (the first finishing decision repeats the start rule's, or the one just recorded after the last long phase)
            can2 = bulk_ok and bits_ok(BF, FSE_FINISH_EVERY) and groups_ok(grp, FSE_FINISH_EVERY)
            while can2:
                first, last = phase(FSE_FINISH_EVERY)
                Bhead = first if mut == "phead_at_phase_head" else last
                iters += FSE_FINISH_EVERY; grp -= FSE_FINISH_EVERY; rec["nFin"] += 1
                BF = B + 8 * inA if mut == "fin_on_aligned_B" else B
                can2 = bits_ok(BF, FSE_FINISH_EVERY) and groups_ok(grp, FSE_FINISH_EVERY)
                dec.append(dict(kind="after_fin", B=B, groups=grp, long=False, fin=can2))
        else:
            lim = 24 + 6 * FSE_CHECK_EVERY + (0 if mut == "plain_after_no_4" else 4)
            while can:
                phase(FSE_CHECK_EVERY)
                iters += FSE_CHECK_EVERY; grp -= FSE_CHECK_EVERY; rec["nLong"] += 1
                q = 4 * ((B + 8 * inA) >> 5) - 8
                can = (q > lim if mut == "gt_plain_after" else q >= lim) and pg(grp)
                dec.append(dict(kind="after_long", q=q, B=B, groups=grp, long=can, fin=False))
            Bhead = B
        rec["iters"] = iters
        rec["wraps"] = iters > FSE_DEC_RING
        if iters:
            # ---- hand-back: the reference's (ptr, bitsConsumed) from the cursor at the head of the last iteration and the cursor now
            at = ((Bhead + (0 if mut == "handback_floor" else 7)) >> 3) - 8
            used = 8 * (at + 8) - B
            rec["handback"] = (at, used)
            if at < 0 or at + 8 > S or used < 0:               # (a broken variant only: the kernel would read outside the payload)
                rec["result"] = "invalid hand-back"
                rec["out"] = bytes(out)
                return rec
            r.at, r.used = at, used
            r._load()
    s1, s2 = state

    # ---- fse_tail: the remaining iterations of :201-218 from the reader, then the end game :222-235 ----
    def step(st):
        nb = nbs[st]
        out.append(sym[st])
        low = r.read_fast(nb) if fast else r.read(nb)
        return ns[st] + low

    def ok_state(st):
        return 0 <= st < len(ns)

    op = len(out)
    result = None
    while True:
        rec["heads"].append(r.unread())
        stt = r.reload()
        if not (stt == Reader.UNFINISHED and op < omax - 3):
            break
        rec["tailIters"] += 1
        s1 = step(s1); s2 = step(s2); s1 = step(s1); s2 = step(s2)
        op += 4
    while True:
        if op > omax - 2:
            result, rec["exit"] = ferr("dstSize_tooSmall"), "tooSmall_1"
            break
        s1 = step(s1); op += 1
        if r.reload() == Reader.OVERFLOW:
            s2 = step(s2); op += 1
            result, rec["exit"] = op, "state2_last"
            break
        if op > omax - 2:
            result, rec["exit"] = ferr("dstSize_tooSmall"), "tooSmall_2"
            break
        s2 = step(s2); op += 1
        if r.reload() == Reader.OVERFLOW:
            s1 = step(s1); op += 1
            result, rec["exit"] = op, "state1_last"
            break
        assert ok_state(s1) and ok_state(s2)
    rec["result"] = result
    rec["out"] = bytes(out[:op])
    return rec


def view(rec):
    """what a broken variant must change to be told from the kernel's: a phase count, the rebuilt reader state, the result or a byte"""
    return (rec["nLong"], rec["nFin"], rec["handback"], rec["result"], rec["out"])


def wave_rounds(recs, G, key):
    """Rounds a workgroup's TIMED counters record for `key` ('nLong' -> g_decTiming[2], 'nFin' -> [10]), summed over its decoder waves.  Rounds
    are wave-uniform among the lane pairs inside the bulk branch, and every chain that can run does run, so a wave runs as many rounds as its
    slowest block; the counter a wave adds is lane 0's, i.e. that of the wave's first slot, which counts rounds only if its own block ever
    entered the bulk (the branch `(lane >> 1) < ppw && everBulk` keeps the other pairs out altogether)."""
    ppw = (G + FSE_DEC_WAVES - 1) // FSE_DEC_WAVES
    total = 0
    for w in range(FSE_DEC_WAVES):
        mine = recs[:G][w * ppw:(w + 1) * ppw]
        if mine and mine[0] is not None and mine[0]["everBulk"]:
            total += max(m[key] for m in mine if m is not None and m["everBulk"])
    return total

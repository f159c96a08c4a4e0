"""Route model of the 16-bit-symbol coder (csrc/fse_u16.hip, csrc/fse_u16_decode.hip): which DECISIONS one block meets on its way
through k_u16_cprep / k_u16_encode_wave / k_u16_encode and k_u16_dparse / k_u16_dprep / k_u16_decode_lds / k_u16_decode.

It restates the kernels' rules -- every `if` that sends a block one way or the other, one line each -- and none of their data movement.
It is fed by the compiled reference's outputs only (the normalised counts FSE_readNCount reads back from a header, the table
FSE_buildCTableU16 builds from them, the bytes FSE_compressU16 / FSE_compressU16_usingCTable write) and by the addresses the caller
chooses; nothing from the device goes into it.  tests/u16_corpus.py labels its blocks with what `compress()` and `decode()` return,
tests/test_u16_corpus.py pins the model against the reference (results, bytes, symbols) and against deliberately broken rule sets
(MUTANTS), tests/test_gpu_u16_paths.py runs the labelled blocks on the device.

compress(src, ...) -> dict: result (the reference's size_t), out (header + payload bytes where a stream is written), labels, and the facts
    behind the labels: tl, hdr, route ("lane" / "wave" / None), warm, present, rounds (repair rounds of the wave kernel), total (payload
    bits), lead (payload address modulo 64).
decode(comp, cap, ...) -> dict: result, out (the symbols written, also in front of an error), labels, and nLong, nFin, iters, handover =
    (at, used, state) of the reader the literal tail starts from (None without bulk), B0, inA, c0, validLo0, refills, exit.

What the model cannot reach, and why (UNREACHABLE):
  * the S >= 2^28 guard of k_u16_decode_lds (a 256 MiB stream is no seconds-long test) and the n >= 2^27 guard of k_u16_encode_wave;
  * a normaliser refusal inside FSE_compressU16: k_u16_cprep hands wg_normalize the table log wg_optimal_tablelog just raised to
    wg_min_tablelog, the one thing the normaliser checks;
  * the skewed-table route with many distinct symbols: every present symbol keeps one cell, so with p present symbols the top counter is
    at most 2^tl - (p - 1), and top1 * 64 > 63 << tl needs p - 1 < 2^tl / 64 (p <= 64 at table log 12);
  * whether the decoder lane really WAITS on the state ring or an input refill: that is timing between waves.  The model arranges the
    condition (64 and more iterations in a row that take no bits; refills) and cannot say that a wait happened.
"""
import numpy as np

U16_MAXSV = 286
U16_MAXTL = 13
U16_DEFTL = 12
FSE_MAX_TL = 12
FSE_MIN_TL = 5
U16_WAVE_MIN = 2048
U16_LINE = 32
U16_RING = 64
U16D_PHASE = 16
U16D_RING = 64
U16D_IN_RING = 256
U16D_IN_MIRROR = 16
U16D_IN_CHUNK = 64
U16D_FLUSH_MIN = 32
U16D_LDS = 160 * 1024
U16D_CTL_BYTES = 48

M64 = (1 << 64) - 1
ERR = {"GENERIC": 1, "dstSize_tooSmall": 2, "srcSize_wrong": 3, "corruption_detected": 4, "tableLog_tooLarge": 5,
       "maxSymbolValue_tooLarge": 6, "maxSymbolValue_tooSmall": 7}


def ferr(name):
    return (1 << 64) - ERR[name]


def is_err(r):
    return r > (1 << 64) - 64


MUTANTS = {
    "long_832": "a long phase runs from 832 unread bits, not 833",
    "fin_112": "a finishing phase runs from 112 unread bits, not 113",
    "groups_gt_16": "a long phase needs more than 16 groups, not 16",
    "wave_min_le": "the lane kernel takes n <= 2048, not n < 2048",
    "skew_ge": "a table is skewed from top1 * 64 >= 63 << tl on",
    "bits_le_8": "the wave kernel bails out when a lane has 8 bits or fewer, not fewer than 8",
    "tl_edge": "the table log by source size is taken from highbit(n), not highbit(n - 1)",
}

UNREACHABLE = {
    "d:S_ge_2pow28": "k_u16_decode_lds takes no bulk phase for a payload of 256 MiB or more: no seconds-long test holds such a stream",
    "c:n_ge_2pow27": "k_u16_encode_wave leaves blocks of 2^27 symbols and more to the lane kernel: 256 MiB of source",
    "c:normalizer_refuses": "FSE_compressU16 normalises at the table log FSE_optimalTableLog has just raised to FSE_minTableLog, the only thing "
                            "the normaliser checks",
    "c:skewed_many_symbols": "every present symbol keeps one cell: with p present symbols top1 <= 2^tl - (p - 1), so a skewed table needs "
                             "p - 1 < 2^tl / 64",
    "d:ring_wait_observed": "whether the decoder lane waits on the state ring or on a refill is timing between waves; the corpus arranges the "
                            "condition, nothing exports that a wait happened",
}


def hibit(v):
    return int(v).bit_length() - 1


# ---------------------------------------------------------------------------------------------------------------------- the bit reader
class Reader:
    """csrc/bitreader.h (lib/bitstream.h:272-448) on a Python integer"""
    UNFINISHED, END_OF_BUFFER, COMPLETED, OVERFLOW = 0, 1, 2, 3

    def __init__(self, payload):
        self.n = len(payload)
        self.V = int.from_bytes(bytes(payload), "little")
        self.last = int(payload[-1]) if self.n else 0
        self.at, self.used, self.win = 0, 0, 0

    def load(self):
        self.win = (self.V >> (8 * self.at)) & M64

    def init(self):
        n = self.n
        if n < 1:
            return False
        if n >= 8:
            self.at = n - 8
            self.load()
            if self.last == 0:
                return False
            self.used = 8 - hibit(self.last)
        else:
            self.at = 0
            self.load()
            if self.last == 0:
                return False
            self.used = 8 - hibit(self.last) + (8 - n) * 8
        return True

    def read(self, nb):
        v = (self.win >> ((64 - self.used - nb) & 63)) & ((1 << nb) - 1)
        self.used += nb
        return v

    def reload(self):
        if self.used > 64:
            return self.OVERFLOW
        if self.at >= 8:
            self.at -= self.used >> 3
            self.used &= 7
            self.load()
            return self.UNFINISHED
        if self.at == 0:
            return self.END_OF_BUFFER if self.used < 64 else self.COMPLETED
        nbytes, res = self.used >> 3, self.UNFINISHED
        if self.at < nbytes:
            nbytes, res = self.at, self.END_OF_BUFFER
        self.at -= nbytes
        self.used -= nbytes * 8
        self.load()
        return res


# ---------------------------------------------------------------------------------------------------------------------- tables
_DT_CACHE = {}


def build_dtable(norm, msv, tl):
    """FSE_buildDTable (lib/fse_decompress.c:71-126) for any alphabet -> (newState, nbBits, symbol) per cell, as lists"""
    key = (tl, msv, np.asarray(norm[:msv + 1], np.int16).tobytes())
    if key in _DT_CACHE:
        return _DT_CACHE[key]
    ts = 1 << tl
    mask, step = ts - 1, (ts >> 1) + (ts >> 3) + 3
    sym = [0] * ts
    nxt = [0] * (msv + 1)
    high = ts - 1
    for s in range(msv + 1):
        if norm[s] == -1:
            sym[high] = s
            high -= 1
            nxt[s] = 1
        else:
            nxt[s] = int(norm[s])
    pos = 0
    for s in range(msv + 1):
        for _ in range(max(int(norm[s]), 0)):
            sym[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    assert pos == 0
    ns, nb = [0] * ts, [0] * ts
    for u in range(ts):
        v = nxt[sym[u]]
        nxt[sym[u]] = v + 1
        nb[u] = tl - hibit(v)
        ns[u] = (v << nb[u]) - ts
    _DT_CACHE[key] = (ns, nb, sym)
    return _DT_CACHE[key]


class CTable:
    """the reference's FSE_CTable for 16-bit symbols taken apart (lib/fse_compress.c:66-169 as instantiated by lib/fseU16.c): u16 tableLog,
    u16 maxSymbolValue, the state table, then {int deltaFindState; u32 deltaNbBits} per symbol"""

    def __init__(self, ct):
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        h = ct.view(np.uint16)
        self.tl, self.msv = int(h[0]), int(h[1])
        ts = 1 << self.tl
        self.ts = ts
        self.st = h[2:2 + ts].astype(np.int64).tolist()
        tt = ct[1 + (ts >> 1 if self.tl else 1):][:2 * (self.msv + 1)]
        self.dfs = tt[0::2].view(np.int32).astype(np.int64).tolist()
        self.dnb = tt[1::2].astype(np.int64).tolist()
        self.present = sum(1 for d in self.dnb if d != ((self.tl + 1) << 16) - ts)

    def run(self, x, syms):
        """FSE_encodeSymbol over `syms` (emission order) from state x -> (end state, bits)"""
        st, dfs, dnb = self.st, self.dfs, self.dnb
        bits = 0
        for s in syms:
            nb = (x + dnb[s]) >> 16
            bits += nb
            x = st[(x >> nb) + dfs[s]]
        return x, bits


# ---------------------------------------------------------------------------------------------------------------------- header writer rule
def optimal_tablelog(request, n, msv, mut=None):
    """wg_optimal_tablelog(request, n, maxSV, 2, 12, 12) (lib/fse_compress.c:316-342)"""
    tl = request if request else U16_DEFTL
    by_src = (hibit(n if mut == "tl_edge" else n - 1) - 2) & 0xFFFFFFFF       # (unsigned: 2 .. 4 symbols wrap and keep the request)
    tl = min(by_src, tl)
    need = min(hibit(n) + 1, hibit(msv) + 2)
    tl = max(need, tl)
    tl = max(tl, FSE_MIN_TL)
    return min(tl, FSE_MAX_TL)


# ---------------------------------------------------------------------------------------------------------------------- compress side
def count_labels(n, src_addr):
    """the loops of FSE_countU16 in k_u16_cprep: head, prefetched groups of four vectors per lane, single vectors, tail"""
    out = set()
    head = min(((-src_addr) & 15) >> 1, n)
    nvec = (n - head) >> 3
    tail = n - head - (nvec << 3)
    out.add("c:count_head_%d" % head)
    out.add("c:count_tail_%d" % tail)
    if nvec in (192, 193, 256, 449):
        out.add("c:count_nvec_%d" % nvec)
    pre = single = False
    for lane in range(64):
        i = lane
        if i + 192 < nvec:
            pre = True
            while True:
                j = i + 256
                more = j + 192 < nvec
                i = j
                if not more:
                    break
        if i < nvec:
            single = True
    out.add("c:count_prefetch" if pre else "c:count_no_prefetch")
    if single:
        out.add("c:count_single_vectors")
    return out


def compress(src, msv_req, tl_req, cap, facts, src_addr=0, dst_addr=0, hdr_verdict=None, mut=None):
    """FSE_compressU16 as the device routes it.  `facts`: None, or what the reference says of this block's table: dict(norm, msv, tl,
    header (bytes), ct (FSE_buildCTableU16's words)); `hdr_verdict(cap) -> header size or error` is the header writer's verdict at a capacity
    below the header's bound (tests/u16_corpus.py: the careful writer restated, checked there against the reference's)."""
    src = np.asarray(src, dtype=np.uint16)
    n = len(src)
    L = set()
    R = {"labels": L, "out": b"", "route": None, "rounds": None, "tl": None, "hdr": None, "lead": None, "total": None, "warm": None}

    def done(result, label):
        L.add(label)
        R["result"] = result
        return R
    if n <= 1:
        return done(n, "c:n_le_1")
    msv = msv_req or U16_MAXSV
    tlr = tl_req or U16_DEFTL
    if msv > U16_MAXSV:
        return done(ferr("maxSymbolValue_tooLarge"), "c:err_maxsv_too_large")
    if tlr > U16_MAXTL:
        return done(ferr("tableLog_tooLarge"), "c:err_tablelog_too_large")
    L |= count_labels(n, src_addr)
    if int(src.max()) > msv:
        return done(ferr("maxSymbolValue_tooSmall"), "c:err_symbol_above_limit")
    cnt = np.bincount(src)
    if int(cnt.max()) == n:
        return done(1, "c:one_symbol")
    top = len(cnt) - 1
    tl = optimal_tablelog(tlr, n, top, mut)
    R["tl"] = tl
    L.add("c:tl_le_11" if tl <= 11 else "c:tl_12_wide_launch")
    if n == 16384 and not tl_req:
        L.add("c:n16384_tl%d" % tl)
    if n == 16385 and not tl_req:
        L.add("c:n16385_tl%d" % tl)
    if tlr == 13 and tl == 12:
        L.add("c:request_13_clamped")
    if mut == "tl_edge" and facts["tl"] != tl:
        return done(None, "c:mutant_table_log_differs")
    assert facts is not None and facts["tl"] == tl and facts["msv"] == top, (facts and facts["tl"], tl, top)
    header = bytes(facts["header"])
    hdr = len(header)
    bound = (((top + 1) * tl) >> 3) + 3 if top else 512
    if cap < bound:
        v = hdr_verdict(cap)
        if is_err(v):
            return done(v, "c:header_refused")
        assert v == hdr
        L.add("c:header_careful_fits")
    R["hdr"] = hdr
    ct = CTable(facts["ct"])
    assert ct.tl == tl
    ts = 1 << tl
    norm = facts["norm"]
    top1 = int(max(norm[:top + 1]))
    skew = top1 * 64 >= (63 << tl) if mut == "skew_ge" else top1 * 64 > (63 << tl)
    if top1 * 64 == (63 << tl):
        L.add("c:skew_at_63_64")
    if top1 * 64 == (63 << tl) + 64:
        L.add("c:skew_at_63_64_plus_1")
    syms = src[::-1].astype(np.int64).tolist()                      # emission order: the last symbol first
    route = "wave"
    if skew:
        route = "lane"
        L.add("c:route_lane_skewed")
    short = n <= U16_WAVE_MIN if mut == "wave_min_le" else n < U16_WAVE_MIN
    if short:
        route = "lane"
        L.add("c:route_lane_short")
    if n == 2047 or n == 2048:
        L.add("c:n_%d" % n)
    payload_addr = dst_addr + hdr
    if route == "wave" and (payload_addr & ~3) < dst_addr:
        route = "lane"
        L.add("c:wave_bail_word_in_front_of_row")
    elif route == "wave" and hdr <= 3:
        L.add("c:wave_short_header_row_mod4_%d" % (dst_addr & 3))
    # the exact chain: bits per symbol and the state in front of every symbol
    st, dfs, dnb = ct.st, ct.dfs, ct.dnb
    x = ts
    xs, nbs = [0] * n, [0] * n
    acc, pos = 0, 0
    for j, s in enumerate(syms):
        xs[j] = x
        nb = (x + dnb[s]) >> 16
        nbs[j] = nb
        acc |= (x & ((1 << nb) - 1)) << pos
        pos += nb
        x = st[(x >> nb) + dfs[s]]
    acc |= (x & (ts - 1)) << pos
    pos += tl
    acc |= 1 << pos
    pos += 1
    total = pos
    R["total"] = total
    stream = acc.to_bytes((total + 7) >> 3, "little")
    capp = cap - hdr
    if route == "wave":
        present = ct.present
        warm = (4 << tl) // (present if present else 1)
        L.add("c:warm_clamped_64" if warm < 64 else "c:warm_clamped_2048" if warm > 2048 else "c:warm_between")
        warm = 64 if warm < 64 else 2048 if warm > 2048 else warm
        R["warm"], R["present"] = warm, present
        C = (n + 63) // 64
        j0 = [min(l * C, n) for l in range(64)]
        j1 = [min((l + 1) * C, n) for l in range(64)]
        mine = [j0[l] < j1[l] for l in range(64)]
        last_lane = (n - 1) // C
        if last_lane < 63:
            L.add("c:lanes_without_symbols")
        start, end, bits = [ts] * 64, [ts] * 64, [0] * 64
        for l in range(64):
            if not mine[l]:
                continue
            x = ts
            if j0[l] > warm:
                x, _ = ct.run(x, syms[j0[l] - warm:j0[l]])
                L.add("c:start_speculated")
            else:
                x, _ = ct.run(x, syms[0:j0[l]])
                L.add("c:start_exact")
            start[l] = x
            end[l], bits[l] = ct.run(x, syms[j0[l]:j1[l]])
        rounds = 0
        while True:
            prev = [ts] + end[:63]
            bad = [mine[l] and l > 0 and start[l] != prev[l] for l in range(64)]
            if not any(bad):
                break
            rounds += 1
            for l in range(64):
                if bad[l]:
                    start[l] = prev[l]
                    end[l], bits[l] = ct.run(start[l], syms[j0[l]:j1[l]])
        assert all(start[l] == xs[j0[l]] for l in range(64) if mine[l])
        R["rounds"] = rounds
        L.add("c:repair_rounds_0" if rounds == 0 else "c:repair_rounds_1" if rounds == 1 else "c:repair_rounds_2plus")
        few = [mine[l] and (bits[l] <= 8 if mut == "bits_le_8" else bits[l] < 8) for l in range(64)]
        if any(mine[l] and bits[l] == 8 for l in range(64)):
            L.add("c:lane_with_exactly_8_bits")
        if any(few):
            route = "lane"
            L.add("c:wave_bail_lane_under_8_bits")
        else:
            bits[last_lane] += tl + 1
            excl = [sum(bits[:l]) for l in range(64)]
            assert excl[63] + bits[63] == total
            if capp <= 8:
                L.add("c:wave_room_le_8")
            elif (total >> 3) == capp - 8:
                L.add("c:wave_room_edge_refused")
            elif (total >> 3) == capp - 9:
                L.add("c:wave_room_edge_fits")
            cs = ((total + 7) >> 3) if capp > 8 and (total >> 3) < capp - 8 else 0
            if cs:
                lead = payload_addr & (U16_RING - 1)
                R["lead"] = lead
                L.add("c:sink_lead_%d" % lead)
                for l in range(64):
                    if not mine[l]:
                        continue
                    if l > 0:
                        L.add("c:sink_first_byte_shared" if excl[l] & 7 else "c:sink_first_byte_own")
                    off0 = lead + (excl[l] >> 3)
                    woff, done_, nacc = off0 & ~3, off0, 8 * (off0 & 3) + (excl[l] & 7)
                    pieces = 0
                    seq = nbs[j0[l]:j1[l]]
                    for k, nb in enumerate(seq):
                        nacc += nb
                        if nacc >= 32:
                            woff += 4
                        nacc &= 31
                        if (k & 7) == 7 or k == len(seq) - 1:                   # line()
                            Lo = done_ & ~(U16_LINE - 1)
                            if woff >= Lo + U16_LINE:
                                L.add("c:sink_piece_aligned" if done_ == Lo else "c:sink_piece_copy_out")
                                done_ = Lo + U16_LINE
                                pieces += 1
                    if not pieces:
                        L.add("c:sink_lane_without_piece")
            R["route"] = "wave"
            R["out"] = header + (stream if cs else b"")
            s = hdr + cs
            if s >= 2 * (n - 1):
                L.add("c:wave_result_0_not_compressible")
            L.add("c:route_wave")
            R["result"] = 0 if s >= 2 * (n - 1) else s
            return R
    # the lane kernel
    R["route"] = "lane"
    L.add("c:lane_n_mod4_%d" % (n & 3))
    cs = 0
    if capp <= 8:
        L.add("c:lane_room_le_8")
    else:
        lim = capp - 8
        p = min(total >> 3, lim)
        if p >= lim:
            L.add("c:lane_clamped_at_room_minus_8")
            if (total >> 3) == lim:
                L.add("c:lane_room_edge_refused")
        else:
            cs = (total + 7) >> 3
            if (total >> 3) == lim - 1:
                L.add("c:lane_room_edge_fits")
    R["out"] = header + (stream if cs else b"")
    s = hdr + cs
    if s >= 2 * (n - 1):
        L.add("c:lane_result_0_not_compressible")
    R["result"] = 0 if s >= 2 * (n - 1) else s
    return R


# ---------------------------------------------------------------------------------------------------------------------- decompress side
def launch_geometry(log):
    """u16d_launch: blocks per workgroup of the 4 KiB (table logs up to 11) and the 8 KiB (table log 12) instance"""
    slot = U16D_RING * 8 + U16D_IN_RING + U16D_IN_MIRROR
    srv = 5 if log >= 12 else 9
    return min((U16D_LDS - 16) // ((2 << log) + slot + U16D_CTL_BYTES), 4 * srv)


def decode(comp, cap, parsed, in_addr=0, out_addr=0, mut=None):
    """FSE_decompressU16 as the device routes it.  `parsed` = (result, maxSymbolValue, tableLog, counts) of the reference's FSE_readNCount on
    `comp` with a limit of 286 (None when comp is shorter than 2 bytes)."""
    comp = bytes(comp)
    L = set()
    R = {"labels": L, "out": [], "nLong": 0, "nFin": 0, "iters": 0, "handover": None, "everBulk": False, "exit": None, "B0": None,
         "inA": None, "c0": None, "validLo0": None, "refills": None, "cls": None}

    def done(result, label):
        L.add(label)
        R["result"] = result
        return R
    if len(comp) < 2:
        return done(ferr("srcSize_wrong"), "d:csize_lt_2")
    h, msv, tl, norm = parsed
    if is_err(h):
        return done(h, "d:header_error")
    if tl > U16_MAXTL:
        return done(ferr("tableLog_tooLarge"), "d:tablelog_above_13")
    if h >= len(comp):
        return done(ferr("srcSize_wrong"), "d:nothing_behind_header")
    cls = 11 if tl <= 11 else tl
    R["cls"] = cls
    L.add("d:builder_tl_le_11" if tl <= 11 else "d:builder_tl_%d" % tl)
    ns, nb, sym = build_dtable(norm, msv, tl)
    payload = comp[h:]
    S = len(payload)
    r = Reader(payload)
    init_ok = r.init()
    state = r.read(tl)
    r.reload()
    out = R["out"]
    V = r.V
    if cls <= 12:                                                           # k_u16_decode_lds
        pa = in_addr + h
        inA = pa & 3
        B0 = 8 * (r.at + 8) - r.used if init_ok and S < (1 << 28) else 0
        R["B0"], R["inA"] = B0, inA
        if not init_ok:
            L.add("d:init_fails_no_bulk")
        grp = min(cap // 4, 1 << 30)
        LONG = 832 if mut == "long_832" else 65 + 48 * U16D_PHASE
        FIN = 112 if mut == "fin_112" else 65 + 48

        def rules(B, g):
            return (B >= LONG and (g > U16D_PHASE if mut == "groups_gt_16" else g >= U16D_PHASE)), (B >= FIN and g >= 1)
        can, can1 = rules(B0, grp)
        if init_ok:
            for v in (833, 832, 113, 112):
                if B0 == v and cap >= 4 * U16D_PHASE:
                    L.add("d:start_%d" % v)
            if B0 >= 833 and grp in (0, 1, 15, 16, 17):
                L.add("d:groups_%d" % grp)
        ever = can or can1
        R["everBulk"] = ever
        B = B0
        iters = 0
        if ever:
            Bq = B0 + 8 * inA
            q = 4 * (Bq >> 5) - 8
            c0 = (-(pa - inA)) & (U16D_IN_CHUNK - 1)
            valid = (((q + 8 - 112 - c0) & ~(U16D_IN_CHUNK - 1)) + c0)
            R["c0"], R["validLo0"] = c0, valid
            L.add("d:inA_%d" % inA)
            L.add("d:last_word_bytes_%d" % ((S + inA) & 3))
            need_lo = None
            zero_run = best_zero = 0

            def phase(niter):
                nonlocal B, state, iters, need_lo, zero_run, best_zero
                qq = 4 * ((B + 8 * inA) >> 5) - 8
                if (qq & (U16D_IN_RING - 4)) >= U16D_IN_RING - 8:
                    L.add("d:window_crosses_ring_end_at_phase_start")
                need_lo = max(qq - (6 * niter + 8 if niter > 1 else 16), 0)
                for _ in range(niter):
                    qi = 4 * ((B + 8 * inA) >> 5) - 8
                    if ((qi - 8) & (U16D_IN_RING - 4)) == U16D_IN_RING - 4:
                        L.add("d:refill_read_crosses_ring_end")
                    used = 0
                    for _k in range(4):
                        k = nb[state]
                        out.append(sym[state])
                        state = ns[state] + ((V >> (B - used - k)) & ((1 << k) - 1))
                        used += k
                    B -= used
                    if used == 48:
                        L.add("d:iteration_of_48_bits")
                    if used == 0:
                        zero_run += 1
                        best_zero = max(best_zero, zero_run)
                    else:
                        zero_run = 0
                iters += niter
            while can:
                phase(U16D_PHASE)
                grp -= U16D_PHASE
                R["nLong"] += 1
                can, can1 = rules(B, grp)
                for v in (833, 832, 113, 112):
                    if B == v and grp >= U16D_PHASE:
                        L.add("d:after_long_%d" % v)
                if B == 65:
                    L.add("d:long_phase_leaves_65")
            while can1:
                phase(1)
                grp -= 1
                R["nFin"] += 1
                _, can1 = rules(B, grp)
                for v in (113, 112):
                    if B == v and grp >= 1:
                        L.add("d:after_fin_%d" % v)
            if best_zero >= 64:
                L.add("d:zero_bit_iterations_64plus")
            # refills the decoder cannot do without: 64-byte chunks until validLo is at or below the lowest byte the last phase reads
            req = max((valid - need_lo + U16D_IN_CHUNK - 1) // U16D_IN_CHUNK, 0) if valid > 0 else 0
            R["refills"] = req
            if valid <= 0 and S >= 150:
                L.add("d:refills_0")
            if req == 1 and valid <= U16D_IN_CHUNK:
                L.add("d:refills_1")
            if req >= 8:
                L.add("d:refills_8plus_ring_wraps_twice")
            if iters < 32 or iters >= 300 or iters in (32, 64, 65):
                L.add("d:iters_lt_32" if iters < 32 else "d:iters_300plus" if iters >= 300 else "d:iters_%d" % iters)
            L.add("d:out_row_mod8_%d" % (out_addr & 7))
            if R["nLong"] and R["nFin"]:
                L.add("d:long_then_finishing")
        elif init_ok:
            L.add("d:never_bulk_B_lt_113" if B0 < 113 else "d:never_bulk_no_group")
        R["iters"] = iters
        if iters:                                                           # the reader rebuilt at this position
            r.at = ((B + 7) >> 3) - 8
            r.used = 8 * (r.at + 8) - B
            r.load()
            R["handover"] = (r.at, r.used, state)
    # the literal tail (k_u16_decode: all of it): fseU16.c:288-298
    op = len(out)
    while True:
        st_ = r.reload()
        if not (st_ < Reader.COMPLETED and op < cap):
            break
        out.append(sym[state])
        state = ns[state] + r.read(nb[state])
        op += 1
    if not (r.at == 0 and r.used == 64):
        R["exit"] = "reader_overrun" if r.used > 64 else "destination_full"
        result = ferr("corruption_detected")
    else:
        while state and op < cap:
            out.append(sym[state])
            state = ns[state] + r.read(nb[state])
            op += 1
        R["exit"] = "state_not_0" if state else "clean"
        result = ferr("corruption_detected") if state else op
    L.add("d:exit_" + R["exit"])
    R["result"] = result
    return R


def view(s):
    """what a mutant of the decode rules must change to be caught"""
    return (s["nLong"], s["nFin"], s["handover"], s["result"], tuple(s["out"]), tuple(sorted(s["labels"])))

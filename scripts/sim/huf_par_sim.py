"""Lane-exact CPU model of k_huf_decode_par (csrc/huf_decode_par.hip), single- and double-symbol tables, 4X and 1X.

What it copies from the kernel: the block checks that decide serial or parallel (the jump table, stream lengths, the end mark, HPAR_MIN_BITS per
stream -- and, on the one-shot path, k_huf_dprep's rule on the shortest stream, huf_prep.hip), the cursor geometry (Cend, Cstart, T0), the
pieces of PDW dwords, the warm-up formula, every lane's S_j / E_j and symbol count, the repair rounds up to the hand-over at HPAR_MAX_REPAIR,
the spill of a lane with more than HPAR_KEEP iterations and the piece verdict.  What it reports per block: serial or parallel (and why),
per stream and piece the rounds, bad links and spills, the HPAR_STATS record (rounds and bad links summed over the streams) and, for a
parallel block, the bytes it regenerates.  The code table is the reference's HUF_readDTableX1 (u32 words, lib/huf_decompress.c:118-185) or,
with `accept_x2` (the HUF_decompress4X / 1X_usingDTable batches), its HUF_readDTableX2 (:460-640): `derive_x2` restates, cell for cell, how the
X2 instantiation derives single-symbol cells from a double-symbol table and every rule by which it declines one (X2_CLAUSES).

Both budgets of the product take every parallel block with the 4.5 KiB class (HPAR_ALL_SMALL, HPAR_USE_TINY 0: internal.h), so the piece
size is that class's; a block with a double-symbol table is taken by the X2 launch, an instantiation of the large class (HPAR_DATA_LARGE:
pieces of 2120 dwords).  `mut` names a deliberately broken variant (MUTANTS) for tests/test_repair_corpus.py and
tests/test_huf_x2_par_model.py.
"""
import numpy as np

LANES = 64
WARM = 128                  # HPAR_WARM
MAX_REPAIR = 8              # HPAR_MAX_REPAIR
KEEP = 40                   # HPAR_KEEP (iterations of four symbols)
MIN_BITS = 4096             # HPAR_MIN_BITS
DATA_SMALL = 4608           # HPAR_DATA_SMALL
PDW = DATA_SMALL // 4 - 24  # dwords of a piece
DATA_LARGE = 8192 + 384     # HPAR_DATA_LARGE: the X2 launch
PDW_X2 = DATA_LARGE // 4 - 24

# the rules a double-symbol table must keep to be decoded through derived single-symbol cells, in the order derive_x2 reports them
X2_CLAUSES = {
    "runs": "the cells that begin with one symbol form ONE run",
    "pow2_aligned": "a run's length is a power of two and the run starts on a multiple of it",
    "n_lt_ts": "a run is shorter than the table (n < ts: no code of zero bits)",
    "len_1_or_2": "a cell's length field is 1 or 2",
    "len1_bits": "a one-symbol cell consumes the bits of its symbol",
    "second_present": "the second symbol of a two-symbol cell begins some cell",
    "len2_bits": "a two-symbol cell consumes the bits of its two symbols together",
    "nbtot_le_log": "a two-symbol cell consumes at most tableLog bits",
    "second_follows": "the second symbol is the first symbol of what follows the first code",
}

MUTANTS = {
    "trust_S_after_round0": "a lane repaired in round 1 is trusted: links are not checked again",
    "verdict_ignores_endC": "the last piece's verdict does not ask that it end on the stream's first bit",
    "verdict_ignores_count": "the last piece's verdict does not count the symbols",
    "next_piece_nominal": "a piece after the first starts at the nominal end of the one before, not where its last lane ended",
    "max_repair_9": "the block is handed to the serial decoder after nine repair rounds, not eight",
    "min_bits_le": "a stream of exactly HPAR_MIN_BITS bits goes to the serial decoder",
    "warm_unclamped": "the warm-up is not clamped to 48 .. 192 bits",
    "no_pieces": "a stream is never cut into pieces",
    "x2_small_pieces": "a block with a double-symbol table is cut into the lean launch's pieces of 1128 dwords",
    "x2_len_from_cell": "the derived single-symbol cell takes the double-symbol cell's nbBits, not the length of its first symbol's run",
}
MUTANTS.update({"x2_no_" + k: "double-symbol tables, rule dropped: " + v for k, v in X2_CLAUSES.items()})


def hibit(v):
    return int(v).bit_length() - 1


class Stream:
    """cursor tables of one stream: nxt[C] = C + nbBits of the code at cursor C, sym[C] its byte (bits below the stream's first bit read 0)"""

    def __init__(self, data, cells, dtLog):
        L = len(data)
        Sd = (L + 3) // 4
        buf = np.zeros(4 * Sd, np.uint8)
        buf[:L] = data
        r = np.unpackbits(buf, bitorder="little")[::-1].astype(np.int64)   # r[C] = the C-th bit consumed from the top
        r = np.concatenate([r, np.zeros(dtLog + 64, np.int64)])
        N = 32 * Sd + 64
        peek = np.zeros(N, np.int64)
        for t in range(dtLog):
            peek = (peek << 1) | r[t:t + N]
        nb = (cells >> 8).astype(np.int64)
        self.nxt = (np.arange(N) + nb[peek]).tolist()
        self.sym = (cells & 0xFF)[peek].astype(np.uint8)
        self.N = N

    def run(self, C, limit):
        """hpar_run: decode from C to the first boundary at or beyond limit; returns (C, symbols)"""
        n, nxt, N = 0, self.nxt, self.N
        while C < limit:
            C = nxt[C] if C < N else C + 1      # (beyond the table: past every real cursor, only garbage lanes get here)
            n += 1
        return C, n

    def decode(self, C, count):
        out = np.zeros(count, np.uint8)
        for i in range(count):
            out[i] = self.sym[C]
            C = self.nxt[C]
        return out


def derive_x2(dt, mut=None):
    """huf_decode_par.hip:347-421 on the reference's double-symbol DTable (u32 words, cell = s1 | s2 << 8 | nbBits << 16 | length << 24):
    (accept, the first rule of X2_CLAUSES the table breaks or None, the single-symbol cells s1 | len(s1) << 8 in table order or None)"""
    dt = np.asarray(dt, dtype=np.uint32)
    dtLog = (int(dt[0]) >> 16) & 0xFF
    ts = 1 << dtLog
    c = dt[1:1 + ts].astype(np.int64)
    s1, s2, nbTot, ln = c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF, c >> 24
    drop = mut[6:] if mut and mut.startswith("x2_no_") else None
    # runs at their boundaries: a count per first symbol, where its (last) run starts and where the run in front of a boundary ended
    starts = np.nonzero(np.concatenate([[True], s1[1:] != s1[:-1]]))[0]
    cnt = np.bincount(s1[starts], minlength=256)
    lo, hi = np.zeros(256, np.int64), np.zeros(256, np.int64)
    lo[s1[starts]] = starts                                             # (several runs of one symbol: the last one's, as stores in index order leave it)
    hi[s1[starts]] = np.concatenate([starts[1:] - 1, [ts - 1]])
    n = hi - lo + 1
    nbs = np.full(256, 0xFF, np.int64)
    present = cnt > 0
    for name, broken in (("runs", present & (cnt != 1)),
                         ("pow2_aligned", present & (((n & (n - 1)) != 0) | ((lo & (n - 1)) != 0))),
                         ("n_lt_ts", present & (n >= ts))):
        if name != drop and broken.any():
            return False, name, None
    for sy in np.nonzero(present)[0]:
        nbs[sy] = dtLog - hibit(max(int(n[sy]), 1))
    n1, n2 = nbs[s1], nbs[s2]
    one, two = ln == 1, ln == 2
    for name, broken in (("len_1_or_2", ~(one | two)), ("len1_bits", one & (nbTot != n1)), ("second_present", two & (n2 == 0xFF)),
                         ("len2_bits", two & (nbTot != n1 + n2)), ("nbtot_le_log", two & (nbTot > dtLog))):
        if name != drop and broken.any():
            return False, name, None
    j = (np.arange(ts, dtype=np.int64) << np.minimum(n1, 32)) & (ts - 1)    # what follows the first code, zero-extended
    if drop != "second_follows" and (two & (s1[j] != s2)).any():
        return False, "second_follows", None
    return True, None, s1 | ((nbTot if mut == "x2_len_from_cell" else n1) << 8)


def simulate_block(payload, dt, dst_size, streams=4, oneshot=False, max_table_log=12, decode=True, mut=None, accept_x2=False):
    """payload: the block without its header (jump table + streams, or the one stream of 1X); dt: the reference's DTable (u32 words);
    accept_x2: the call is HUF_decompress4X / 1X_usingDTable's batch, which takes double-symbol tables (never the one-shot path)"""
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    dt = np.asarray(dt, dtype=np.uint32)
    desc = int(dt[0])
    dtLog, tableType = (desc >> 16) & 0xFF, (desc >> 8) & 0xFF
    cSize = len(payload)
    rec = dict(parallel=False, reason=None, entered=False, rounds=0, bad=0, streams=[], out=None)
    ldsLog = 12 if max_table_log > 11 else 11
    nS = 1 if streams == 1 else 4
    seg = (dst_size + 3) // 4 if nS == 4 else dst_size
    jump = 6 if nS == 4 else 0
    lens = [0, 0, 0, 0]
    if nS == 4 and cSize >= 10:
        lens[:3] = [int(payload[0]) | int(payload[1]) << 8, int(payload[2]) | int(payload[3]) << 8, int(payload[4]) | int(payload[5]) << 8]
    if oneshot:                                                          # k_huf_dprep (huf_prep.hip:754-762): the shortest stream decides
        used = 6 + sum(lens[:3])
        if not (nS == 4 and cSize >= 10 and dst_size >= 64 and used < cSize and 8 * min(lens[:3] + [cSize - used]) >= MIN_BITS + 8):
            rec["reason"] = "prep"
            return rec
    x2 = tableType == 1 and accept_x2 and not oneshot
    ok = (tableType == 0 or x2) and 1 <= dtLog <= ldsLog and dtLog <= max_table_log and 10 <= cSize < (1 << 28) and 64 <= dst_size < (1 << 28)
    if ok and nS == 4:
        used = 6 + sum(lens[:3])
        if used > cSize:
            ok = False
        else:
            lens[3] = cSize - used
        if 3 * seg >= dst_size:
            ok = False
    if ok and nS == 1:
        lens[0] = cSize
    T0 = [0] * 4
    if ok:
        p = jump
        for q in range(nS):
            L = lens[q]
            last = int(payload[p + L - 1]) if L else 0
            if L < 8 or last == 0:
                ok = False
            else:
                T0[q] = 8 * (L - 1) + hibit(last)
            if T0[q] < MIN_BITS or (mut == "min_bits_le" and T0[q] <= MIN_BITS):
                ok = False
            p += L
    if not ok:
        rec["reason"] = "block"
        return rec
    if x2:
        acc, rec["clause"], cells = derive_x2(dt, mut)
        if not acc:
            rec["reason"] = "table"
            return rec
        if ((cells >> 8) < 1).any():                                     # (only a mutant gets here: a code of zero bits pins every cursor)
            rec.update(entered=True, reason="hang")
            return rec
    else:
        cells = dt[1:1 + (1 << dtLog) // 2].view(np.uint16)[:1 << dtLog].astype(np.int64)
        nbc = cells >> 8
        if ((nbc < 1) | (nbc > dtLog)).any():
            rec["reason"] = "table"
            return rec
    rec["entered"] = True
    pdw = PDW_X2 if x2 and mut != "x2_small_pieces" else PDW
    out = np.zeros(dst_size, np.uint8) if decode else None
    p = jump
    good = True
    max_rep = 9 if mut == "max_repair_9" else MAX_REPAIR
    for q in range(nS):
        L = lens[q]
        S_ = Stream(payload[p:p + L], cells, dtLog)
        Sd = (L + 3) // 4
        want = dst_size if nS == 1 else (seg if q < 3 else dst_size - 3 * seg)
        Cend = 32 * Sd
        Cstart = Cend - T0[q]
        outBase = 0
        warm = WARM + WARM // 2 if T0[q] > 6 * want else (24 * T0[q]) // (want if want else 1)
        if mut != "warm_unclamped":
            warm = min(max(warm, 48), WARM + WARM // 2)
        srec = dict(T0=T0[q], want=want, warm=warm, pieces=[])
        rec["streams"].append(srec)
        while good and Cstart < Cend:
            mTop = (Cstart - 1) >> 5
            rest = Sd - mTop
            nPc = 1 if mut == "no_pieces" else (rest + pdw - 1) // pdw
            nd = rest if nPc <= 1 else (rest + nPc - 1) // nPc
            lastPiece = mTop + nd == Sd
            C0 = Cstart
            CendL = Cend if lastPiece else 32 * (mTop + nd)
            Tp = CendL - C0
            stepA = (Tp + 63) // 64
            S, E, n = [0] * LANES, [0] * LANES, [0] * LANES
            for j in range(LANES):
                aLo = min(j * stepA, Tp)
                if j == 0:
                    S[j] = C0
                else:
                    S[j], _ = S_.run(C0 + aLo - warm if aLo > warm else C0, C0 + aLo)
            cHi = [C0 + min((j + 1) * stepA, Tp) for j in range(LANES)]
            todo = [True] * LANES
            spill = [False] * LANES
            prec = dict(nd=nd, last=lastPiece, rounds=0, bad=[], spill=False, reruns=[0] * LANES)
            for rnd in range(10 ** 6):
                for j in range(LANES):
                    if todo[j]:
                        E[j], n[j] = S_.run(S[j], cHi[j])
                        spill[j] = n[j] > 4 * KEEP
                        if rnd:
                            prec["reruns"][j] += 1
                bad = [j > 0 and S[j] != E[j - 1] for j in range(LANES)]
                if mut == "trust_S_after_round0" and rnd >= 1:
                    bad = [False] * LANES
                if not any(bad):
                    break
                if rnd == max_rep:
                    good = False
                    prec["fail"] = "rounds"
                    break
                rec["rounds"] += 1
                rec["bad"] += sum(bad)
                prec["rounds"] += 1
                prec["bad"].append(sum(bad))
                todo = bad
                S = [E[j - 1] if bad[j] else S[j] for j in range(LANES)]
            srec["pieces"].append(prec)
            if not good:
                break
            prec["spill"] = any(spill)
            total, endC = sum(n), E[LANES - 1]
            if lastPiece:
                fail = (outBase + total != want and mut != "verdict_ignores_count") or (endC != CendL and mut != "verdict_ignores_endC")
            else:
                fail = outBase + total >= want
            if fail:
                good = False
                prec["fail"] = "verdict"
                break
            if decode:
                pos = q * seg + outBase
                for j in range(LANES):
                    k = min(n[j], max(want - (pos - q * seg), 0))     # (a mutant may claim more symbols than the segment holds)
                    if k:
                        out[pos:pos + k] = S_.decode(S[j], k)
                    pos += n[j]
            outBase += total
            Cstart = CendL if (mut == "next_piece_nominal" and not lastPiece) else endC
        if not good:
            break
        p += L
    rec["parallel"] = good
    if not good:
        rec["reason"] = "repair"
    elif decode:
        rec["out"] = out
    return rec

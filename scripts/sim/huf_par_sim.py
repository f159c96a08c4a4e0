"""Lane-exact CPU model of k_huf_decode_par (csrc/huf_decode_par.hip), single-symbol tables, 4X and 1X.

What it copies from the kernel: the block checks that decide serial or parallel (the jump table, stream lengths, the end mark, HPAR_MIN_BITS per
stream -- and, on the one-shot path, k_huf_dprep's rule on the shortest stream, huf_prep.hip), the cursor geometry (Cend, Cstart, T0), the
pieces of PDW dwords, the warm-up formula, every lane's S_j / E_j and symbol count, the repair rounds up to the hand-over at HPAR_MAX_REPAIR,
the spill of a lane with more than HPAR_KEEP iterations and the piece verdict.  What it reports per block: serial or parallel (and why),
per stream and piece the rounds, bad links and spills, the HPAR_STATS record (rounds and bad links summed over the streams) and, for a
parallel block, the bytes it regenerates.  The code table is the reference's HUF_readDTableX1 (u32 words, lib/huf_decompress.c:118-185).

Both budgets of the product take every parallel block with the 4.5 KiB class (HPAR_ALL_SMALL, HPAR_USE_TINY 0: internal.h), so the piece
size is that class's.  `mut` names a deliberately broken variant (MUTANTS) for tests/test_repair_corpus.py.
"""
import numpy as np

LANES = 64
WARM = 128                  # HPAR_WARM
MAX_REPAIR = 8              # HPAR_MAX_REPAIR
KEEP = 40                   # HPAR_KEEP (iterations of four symbols)
MIN_BITS = 4096             # HPAR_MIN_BITS
DATA_SMALL = 4608           # HPAR_DATA_SMALL
PDW = DATA_SMALL // 4 - 24  # dwords of a piece

MUTANTS = {
    "trust_S_after_round0": "a lane repaired in round 1 is trusted: links are not checked again",
    "verdict_ignores_endC": "the last piece's verdict does not ask that it end on the stream's first bit",
    "verdict_ignores_count": "the last piece's verdict does not count the symbols",
    "next_piece_nominal": "a piece after the first starts at the nominal end of the one before, not where its last lane ended",
    "max_repair_9": "the block is handed to the serial decoder after nine repair rounds, not eight",
    "min_bits_le": "a stream of exactly HPAR_MIN_BITS bits goes to the serial decoder",
    "warm_unclamped": "the warm-up is not clamped to 48 .. 192 bits",
    "no_pieces": "a stream is never cut into pieces",
}


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


def simulate_block(payload, dt, dst_size, streams=4, oneshot=False, max_table_log=12, decode=True, mut=None):
    """payload: the block without its header (jump table + streams, or the one stream of 1X); dt: the reference's DTable (u32 words)"""
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
    ok = tableType == 0 and 1 <= dtLog <= ldsLog and dtLog <= max_table_log and 10 <= cSize < (1 << 28) and 64 <= dst_size < (1 << 28)
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
    cells = dt[1:1 + (1 << dtLog) // 2].view(np.uint16)[:1 << dtLog].astype(np.int64)
    nbc = cells >> 8
    if ((nbc < 1) | (nbc > dtLog)).any():
        rec["reason"] = "table"
        return rec
    rec["entered"] = True
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
            nPc = 1 if mut == "no_pieces" else (rest + PDW - 1) // PDW
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

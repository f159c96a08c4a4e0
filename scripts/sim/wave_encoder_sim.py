"""Lane-exact CPU model of k_fse_encode_wave (csrc/fse_encode_wave.hip) on the caller-table path (a.list == nullptr, a.meta == nullptr).

What it copies from the kernel, line for line: the block set-up (m, C with its two roundings, delta from the source address, lastLane,
the super-ranges sLo / sMid / sHi), the warm-up length with its 64 / 4096 clamps, the `1 << tl` warm-up start and the exact start when
sLo <= 2 + warm, the checkpoint spacing (every, total, none when C & 63), the counting pass, the verify / kept-sample / repair loop of a
wave of two blocks in batch order (WV_SAMPLE_CACHE, WV_CK_MERGE with its shift by d), the hand-over to the ranges, the verdict and the
sub-byte rule that sends a block to the serial writer.  What it reports per wave: rounds, nBad0, firstBad (the FSE_ENC_TIMING record);
per block: every lane's branch, the hand-over (both states at every range bound, every range's bits), the compressed size and the bytes
pass 2 writes from the hand-over.

It is the instrument for pricing repair policies: a kernel change that moves the cut or a branch changes this file and the
corpus labels (tests/repair_corpus.py) with it; tests/test_gpu_repair_paths.py checks it against the device.

`mut` names a deliberately broken variant (MUTANTS): tests/test_repair_corpus.py checks that the corpus tells each from the kernel.
"""
import numpy as np

LANES = 32                 # WV_LANES
WARM_FACTOR = 2            # FSE_WV_WARM_FACTOR
WARM_MIN, WARM_MAX = 64, 4096
CK_MAX = 8                 # WV_CK_MAX
M32 = 0xFFFFFFFF

MUTANTS = {
    "swap_forgets_cmid": "a kept sample taken back keeps the newer run's mid state",
    "swap_forgets_lo": "a kept sample taken back keeps the newer run's bitsLo",
    "merge_no_shift_lo": "a re-run that merges before its midpoint does not shift bitsLo by d",
    "merge_no_shift_slots": "a merge does not shift the later checkpoints' bit counts",
    "merge_late": "a merge at checkpoint i takes its shift from checkpoint i + 1's record",
    "no_delta": "the cut ignores the source address",
    "small_like_large": "blocks below 4 KiB are cut like large ones",
    "last_lane_no_delta": "lastLane ignores delta",
    "no_exact_start": "no lane starts exactly, every one warms up from 1 << tl",
    "no_warm_clamp": "the warm-up is not clamped to 64 .. 4096",
    "no_sample_cache": "no kept sample (WV_SAMPLE_CACHE 0)",
    "thin_le8": "the sub-byte rule tests bits <= 8",
}


def ctable_fields(ct):
    """the kernel's view of a reference CTable (u32 words, lib/fse.h:295): tableLog, max symbol, stateTable, deltaFindState, deltaNbBits"""
    ct = np.asarray(ct, dtype=np.uint32)
    h0 = int(ct[0])
    tl, msv = h0 & 0xFFFF, min(h0 >> 16, 255)
    if tl == 0:
        return tl, msv, None, None, None
    T = 1 << tl
    st = ct[1:1 + T // 2].view(np.uint16).astype(np.int64)
    tt = ct[1 + T // 2:1 + T // 2 + 2 * (msv + 1)].reshape(-1, 2)
    return tl, msv, st, tt[:, 0].view(np.int32).astype(np.int64), tt[:, 1].astype(np.int64)


def cut(n, addr, mut=None):
    """the ranges in emission order (fse_encode_wave.hip:367-376): m, C, delta, lastLane and range t = [j0, j1) of every lane (n = 0: off)"""
    m = n - 2 if n else 0
    C = (m + LANES - 1) // LANES
    big = m >= 4096 or (mut == "small_like_large" and m > 0)
    C = (C + 63) & ~63 if big else (C + 1) & ~1
    C = C if C else 2
    delta = ((-(addr + n - 2)) & 62) if (m >= 4096 and mut != "no_delta") else 0
    dl = 0 if mut == "last_lane_no_delta" else delta
    lastLane = min((m + dl - 1) // C, LANES - 1) if m else 0
    bounds = []
    for hl in range(LANES):
        lo0 = 2 + hl * C - delta if hl else 2
        hi0 = 2 + (hl + 1) * C - delta
        bounds.append((min(lo0, n), n if (hl == LANES - 1 or hi0 > n) else hi0))
    return m, C, delta, lastLane, bounds


class Block:
    """one block's set-up (fse_encode_wave.hip:301-412) and its lanes' state"""

    def __init__(self, src, ct, addr, max_tl=11, cap=None, mut=None):
        src = np.ascontiguousarray(src, dtype=np.uint8)
        self.src, self.n, self.mut = src, int(src.size), mut
        n = self.n
        self.cap = (512 + n + (n >> 7) + 4 + 8) if cap is None else int(cap)
        self.tl, self.msv, st, dfs, dnb = ctable_fields(ct)
        self.result = None                       # set when the block is finished before the counting pass
        self.on = True
        if self.tl > max_tl:
            self.result, self.on = "tableLog_tooLarge", False
        elif n <= 2 or self.cap <= 8:
            self.result, self.on = 0, False
        elif self.tl == 0:
            self.result, self.on = 1, False
        tl = self.tl
        present = 0
        if self.on:
            T = 1 << tl
            present = int(np.count_nonzero(dnb != ((tl + 1) << 16) - T))
            # FSE_encodeSymbol as one flat table: tr[s * 2T + x] = nbBits << 16 | next state, x in [T, 2T)
            x = np.arange(T, 2 * T, dtype=np.int64)
            nb = (x[None, :] + dnb[:, None]) >> 16
            nxt = st[np.clip((x[None, :] >> nb) + dfs[:, None], 0, T - 1)]
            tr = np.zeros((self.msv + 1, 2 * T), dtype=np.int64)
            tr[:, T:] = (nb << 16) | nxt
            self.tr, self.T2 = tr.ravel().tolist(), 2 * T
            syms = src[::-1].astype(np.int64) * (2 * T)                    # symbol at distance j from the end, pre-scaled
            self.sy = [syms[0::2].tolist(), syms[1::2].tolist()]           # chain c walks the j of parity c
            ns = (dnb + (1 << 15)) >> 16                                   # FSE_initCState2, lib/fse.h:503-512
            self.init = [int(st[(((ns[s] << 16) - dnb[s]) >> ns[s]) + dfs[s]]) for s in range(self.msv + 1)]
        self.present = present
        warm = (WARM_FACTOR << tl) // (present if present else 1)
        warm = (warm + 63) & ~63
        if mut != "no_warm_clamp":
            warm = min(max(warm, WARM_MIN), WARM_MAX)
        self.warm = warm
        self.addr = int(addr)
        self.m, self.C, self.delta, self.lastLane, self.bounds = cut(n if self.on else 0, self.addr, mut)
        C = self.C
        self.every = (2 * C // 64 + CK_MAX - 1) // CK_MAX or 1
        if C & 63:
            self.every = 0x7FFFFFFF
        self.total = (2 * C // 64) // self.every

    # ---- FSE_encodeSymbol with its bits (BIT_addBits: the low nbBits of the state), both chains by j (even: A), j in [ja, jb)
    def emit_range(self, xa, xb, ja, jb):
        acc, pos, tr, sy = 0, 0, self.tr, self.sy
        for j in range(ja, jb):
            if j & 1:
                v = tr[sy[1][j >> 1] + xb]
                nb = v >> 16
                acc |= (xb & ((1 << nb) - 1)) << pos
                xb = v & 0xFFFF
            else:
                v = tr[sy[0][j >> 1] + xa]
                nb = v >> 16
                acc |= (xa & ((1 << nb) - 1)) << pos
                xa = v & 0xFFFF
            pos += nb
        return acc, pos, xa, xb

    # ---- FSE_encodeSymbol over chain c, j in [ja, jb) (ja even)
    def walk(self, c, x, ja, jb):
        bits, tr, T2 = 0, self.tr, self.T2
        for o in self.sy[c][ja // 2:(jb - c + 1) // 2]:
            v = tr[o + x]
            x = v & 0xFFFF
            bits += v >> 16
        return x, bits


class Lane:
    __slots__ = ("blk", "hl", "cc", "kk", "sLo", "sMid", "sHi", "mineC", "exact", "cstart", "cmid", "cend", "bitsLo", "bitsTot",
                 "o", "r", "slot", "idx", "left", "d", "merged", "takes", "reruns")


def _chain(L, c, x, ja, jb, bits, mode):
    """wv_chain (fse_encode_wave.hip:182-224): mode 0 none, 1 record, 2 merge; returns (x, bits); L.merged / L.d on a merge"""
    B = L.blk
    if mode == 0:
        xx, b = B.walk(c, x, ja, jb)
        return xx, bits + b
    ngroups = (jb - ja) // 64 if jb > ja else 0
    g = L.left - 1                                         # the group (of this call) after which the next checkpoint falls
    pos = ja
    while g < ngroups:
        end = ja + 64 * (g + 1)
        x, b = B.walk(c, x, pos, end)
        bits += b
        pos = end
        L.left = B.every
        if mode == 2 and L.idx < CK_MAX:
            ox, oy = L.slot[L.idx]
            if ox == x:
                late = B.mut == "merge_late" and L.idx + 1 < CK_MAX
                d = bits - (L.slot[L.idx + 1][1] if late else oy)
                if B.mut != "merge_no_shift_slots":
                    for i in range(L.idx, min(B.total, CK_MAX)):
                        L.slot[i] = (L.slot[i][0], L.slot[i][1] + d)
                L.d, L.merged = d, True
                return x, bits
        if L.idx < CK_MAX:
            L.slot[L.idx] = (x, bits)
        L.idx += 1
        g += B.every
    L.left = g - ngroups + 1
    x, b = B.walk(c, x, pos, jb)
    return x, bits + b


def _lanes(B):
    out = []
    for hl in range(LANES):
        L = Lane()
        L.blk, L.hl, L.cc, L.kk = B, hl, hl & 1, hl >> 1
        C, d, n, kk = B.C, B.delta, B.n, hl >> 1
        sLo0 = 2 + 2 * kk * C - d if kk else 2
        sMid0, sHi0 = 2 + (2 * kk + 1) * C - d, 2 + (2 * kk + 2) * C - d
        L.sLo, L.sMid = min(sLo0, n), min(sMid0, n)
        L.sHi = n if (2 * kk + 2 >= LANES or sHi0 > n) else sHi0
        L.mineC = B.on and L.sLo < n
        L.exact = False
        L.cstart = L.cmid = L.cend = L.bitsLo = L.bitsTot = 0
        L.slot, L.idx, L.left, L.d, L.merged = [(None, 0)] * CK_MAX, 0, B.every, 0, False
        L.takes, L.reruns = [], []                         # takes: the lane's re-runs so far at each kept sample taken back
        out.append(L)
    return out


def _count(L):
    """warm-up + pass 1 (fse_encode_wave.hip:394-413)"""
    B = L.blk
    if not L.mineC:
        return
    cc = L.cc
    if L.sLo <= 2 + B.warm and B.mut != "no_exact_start":
        L.exact = True
        x, _ = _chain(L, cc, B.init[int(B.src[B.n - 1 - cc])], 2, L.sLo, 0, 0)
    else:                                                    # (sLo - warm > 2 here; the no_exact_start mutant clamps at j = 2)
        x, _ = _chain(L, cc, 1 << B.tl, max(L.sLo - B.warm, 2), L.sLo, 0, 0)
    L.cstart = x
    L.idx, L.left = 0, B.every
    x, nbits = _chain(L, cc, x, L.sLo, L.sMid, 0, 1)
    L.cmid, L.bitsLo = x, nbits
    x, nbits = _chain(L, cc, x, L.sMid, L.sHi, nbits, 1)
    L.cend, L.bitsTot = x, nbits


def simulate_wave(blocks):
    """the verify / repair loop of one wave (fse_encode_wave.hip:425-461) over its one or two blocks (lanes 0-31, 32-63)"""
    lanes = []
    for B in blocks:
        ls = _lanes(B)
        for L in ls:
            _count(L)
            L.o = [M32 + 1, 0, 0, 0, 0]                     # oStart, oEnd, oMid, oLo, oTot (no state is 0xFFFFFFFF)
            L.r = [L.cend, L.cmid, L.bitsLo, L.bitsTot]      # the run the checkpoints describe
        lanes += ls
    cache = not any(B.mut == "no_sample_cache" for B in blocks)
    rounds, nBad0, firstBad = 0, 0, 99
    while True:
        while True:
            prevEnd = [lanes[i - 2].cend if i >= 2 else lanes[i].cend for i in range(len(lanes))]
            bad = [L.mineC and L.kk > 0 and L.cstart != prevEnd[i] for i, L in enumerate(lanes)]
            hit = [cache and bad[i] and L.o[0] == prevEnd[i] for i, L in enumerate(lanes)]
            if not any(hit):
                break
            for i, L in enumerate(lanes):
                if hit[i]:
                    mut = L.blk.mut
                    cur = [L.cstart, L.cend, L.cmid, L.bitsLo, L.bitsTot]
                    old = L.o
                    if mut == "swap_forgets_cmid":
                        old = old[:2] + [L.cmid] + old[3:]
                    if mut == "swap_forgets_lo":
                        old = old[:3] + [L.bitsLo] + old[4:]
                    L.cstart, L.cend, L.cmid, L.bitsLo, L.bitsTot = old
                    L.o = cur
                    L.takes.append(len(L.reruns))
        if not any(bad):
            break
        if rounds == 0:
            nBad0 = sum(bad)
            firstBad = bad.index(True)
        for i, L in enumerate(lanes):
            if not bad[i]:
                continue
            L.o = [L.cstart, L.cend, L.cmid, L.bitsLo, L.bitsTot]
            L.cstart = prevEnd[i]
            L.cend, L.cmid, L.bitsLo, L.bitsTot = L.r
            x, nbits = L.cstart, 0
            L.merged, L.idx, L.left = False, 0, L.blk.every
            midDone = False
            where = None
            for piece, (lo, hi) in enumerate(((L.sLo, L.sMid), (L.sMid, L.sHi))):
                x, nbits = _chain(L, L.cc, x, lo, hi, nbits, 2)
                if L.merged:
                    where = ("merge", piece, L.idx)
                    break
                if piece == 0:
                    L.cmid, L.bitsLo, midDone = x, nbits, True
            if L.merged:
                if not midDone and L.blk.mut != "merge_no_shift_lo":
                    L.bitsLo += L.d
                L.bitsTot += L.d
            else:
                L.cend, L.bitsTot = x, nbits
                where = ("end",)
            L.reruns.append(where)
            L.r = [L.cend, L.cmid, L.bitsLo, L.bitsTot]
        rounds += 1
    res = []
    for w, B in enumerate(blocks):
        res.append(_finish(B, lanes[w * LANES:(w + 1) * LANES]))
    return dict(rounds=rounds, nBad0=nBad0, firstBad=firstBad, blocks=res)


def _finish(B, ls):
    """hand-over to the ranges, prefix sum, verdict, sub-byte rule (fse_encode_wave.hip:463-501)"""
    start, bits = [], []
    for hl in range(LANES):
        a, b = ls[hl & ~1], ls[(hl & ~1) + 1]
        if hl & 1:
            start.append((a.cmid, b.cmid)); bits.append((a.bitsTot - a.bitsLo) + (b.bitsTot - b.bitsLo))
        else:
            start.append((a.cstart, b.cstart)); bits.append(a.bitsLo + b.bitsLo)
    out = dict(n=B.n, tl=B.tl, on=B.on, C=B.C, delta=B.delta, m=B.m, warm=B.warm, every=B.every, total=B.total,
               lastLane=B.lastLane, lanes=[], result=B.result, thin=0, start=None, bits=None)
    if not B.on:
        return out
    mine = [B.bounds[t][0] < B.n for t in range(LANES)]
    out["start"] = [s if mine[t] else None for t, s in enumerate(start)]
    out["bits"] = [bt if mine[t] else 0 for t, bt in enumerate(bits)]
    body = sum(out["bits"])
    total = body + 2 * B.tl + 1
    whole = total >> 3
    csize = 0 if whole >= B.cap - 8 else (total + 7) >> 3
    out["result"] = csize
    thr = 9 if B.mut == "thin_le8" else 8
    if csize:
        out["thin"] = sum(1 for t in range(LANES) if mine[t] and t < B.lastLane and out["bits"][t] < thr)
    for L in ls:
        out["lanes"].append(dict(empty=not L.mineC, exact=L.exact, takes=list(L.takes), reruns=list(L.reruns)))
    out["bytes"] = _emit(B, out) if csize else None
    return out


def _emit(B, out):
    """pass 2 (fse_encode_wave.hip:503-530): range t's bits from its two start states at the prefix sum of the counts before it, the final
    states and the end mark behind lastLane's (fse_compress.c:608-610), neighbours' shared bytes OR-ed; the block's csize bytes"""
    acc, excl, mask = 0, 0, (1 << B.tl) - 1
    for t in range(LANES):
        j0, j1 = B.bounds[t]
        if j0 >= B.n:
            continue
        xa, xb = out["start"][t]
        v, nb, xa, xb = B.emit_range(xa, xb, j0, j1)
        if t == B.lastLane:
            c2, c1 = (xb, xa) if B.n & 1 else (xa, xb)
            v |= ((c2 & mask) | (c1 & mask) << B.tl | 1 << 2 * B.tl) << nb
        acc |= v << excl
        excl += out["bits"][t]
    return acc.to_bytes(out["result"] + 8, "little")[:out["result"]]


def simulate_batch(blocks):
    """caller-table batch: blocks 2w and 2w + 1 share wave w (batch order); returns one record per wave"""
    return [simulate_wave(blocks[i:i + 2]) for i in range(0, len(blocks), 2)]


def serial_truth(B):
    """both chains walked once from the exact start over the whole block: the states at every range bound and every range's bits"""
    if not B.on:
        return None
    n = B.n
    xa, xb = B.init[int(B.src[n - 1])], B.init[int(B.src[n - 2])]
    start, bits = [], []
    for t in range(LANES):
        j0, j1 = B.bounds[t]
        if j0 >= n:
            start.append(None); bits.append(0); continue
        start.append((xa, xb))
        xa, ba = B.walk(0, xa, j0, j1)
        xb, bb = B.walk(1, xb, j0, j1)
        bits.append(ba + bb)
    return start, bits

// fse_wave_build.h -- wave-cooperative core of FSE_buildCTable / FSE_buildDTable (one 64-lane wave per table).
//
// Both reference builders (lib/fse_compress.c:96-133, lib/fse_decompress.c:86-124) do the same two serial walks:
//   1. "spread": visit table cells u = 0, step, 2*step, ... (mod tableSize), skipping cells above highThreshold, and hand
//      them out to the symbols in symbol order, normalizedCounter[s] cells each; the low-probability symbols (-1) take the
//      cells above highThreshold;
//   2. "rank": walk the cells in ascending u and number the cells of every symbol 0, 1, 2, ... in that order
//      (CTable: stateTable[cumul[s] + rank] = tableSize + u;  DTable: nextState = symbolNext[s] + rank).
// Restated without the loop-carried dependencies:
//   1. step is odd, so m -> (m * step) mod tableSize is a bijection and the serial walk visits m = 0, 1, 2, ... in
//      order; the k-th *kept* visit (u <= highThreshold) gets the symbol whose cumulative count range contains k.  Every
//      symbol marks the first k of its range with itself (one byte; 0 = no mark: only the smallest symbol in use can be 0, its
//      mark sits at k = 0, and a running maximum that starts at 0 names it just the same); each lane takes a contiguous range
//      of m, a wave prefix sum of the kept visits gives its first k, and the symbol of a visit is the running maximum of the
//      marks up to its k (a wave prefix maximum carries it across lanes).
//   2. rank(u) = number of cells u' < u with the same symbol.  Lane l owns the contiguous cells [l*C, (l+1)*C);
//      a byte matrix cnt[symbol][lane] counts the symbols per lane range (LDS atomic add with return = the rank inside
//      the range), a per-symbol running sum over groups of 4 lanes gives the ranks of everything before the range.
//      The matrix holds WB_WIN symbols; larger alphabets take one rank / sum / emit pass per window of symbols.
// The result is handed to `emit(u, symbol, rank, payload(symbol))` once per cell, lane l emitting its own range in
// ascending u; `payload` is a per-symbol LDS lookup of the caller's that is gathered together with the core's own.
#pragma once
#include "dev_common.h"

#define WB_MAXSYM 256
// The rank matrix covers a window of WB_WIN symbols at a time (alphabets up to 64 symbols: one pass; measured per 100k blocks,
// compress + decompress build: window 128 -> 64: Proba14 1.88 -> 1.64 ms, tableLog 12 4.48 -> 3.55 ms, Proba02 3.24 -> 3.72 ms; the LDS footprint
// decides how many table builds a CU runs at once, and these builds are latency-bound).
#ifndef WB_WIN
#define WB_WIN 64u
#endif
#define WB_TSTEP(ts) (((ts) >> 1) + ((ts) >> 3) + 3)     // lib/fse.h:683

#ifdef FSE_WB_TIMING         // development aid: phase cycle accounting of the last table build of each workgroup
__device__ unsigned long long g_wbTiming[4096 * 8];
#define WBT(k) TT[k] = __builtin_readcyclecounter();
#else
#define WBT(k)
#endif
// LDS of one wave, tableSize = 1 << tl <= capTs.  Two pairs of arrays share their bytes, each pair being used in phases that a
// barrier separates: the spread's marks and the rank matrix (the marks are dead once the spread is done), the cells' symbols and
// the running sums (every lane holds the symbols of its own cells in registers from the first rank pass on).  The local ranks
// never go to LDS: they stay in the lane's registers from the rank pass to the emit pass.
struct WaveBuildLds {
    s16* nrm;                // [256] normalized counters, zero beyond maxSV (input)
    u16* cumP;               // [257] (unused by the core; callers may use it -- only a carve `withCum` has it)
    u8*  symP;               // [256] symbols in use (counter != 0), ascending
    u8*  symTab;             // [wb_si(capTs)] symbol of every cell (output of the spread), index through wb_si(); shares its bytes with coarse
    u8*  marks;              // [wb_si(capTs)] scratch of the spread, index through wb_si(); shares its bytes with cnt
    u32* cnt;                // [WB_WIN * 16] byte matrix cnt[symbol - window base][lane]
    u16* coarse;             // [WB_WIN * 16] per symbol of the window: cells before lane group j (4 lanes per group)
};
// marks[] / symTab[] are indexed through wb_si(): every row of 32 cells is followed by 4 bytes of padding.  Lane l
// works on cells [l*C, (l+1)*C) (C = 32 at tableLog 11), so without the padding the 64 lanes of one LDS instruction
// would sit 64 (or 32) bytes apart -- on 2 (4) of the 32 banks; with it they are 17 (9) dwords apart: conflict-free.
__host__ __device__ inline u32 wb_si(u32 u) { return u + ((u >> 5) << 2); }
// A/B aid: unused LDS per build, i.e. fewer waves per CU (how much do the builders live on residency?)
#ifndef WB_EXTRA_LDS
#define WB_EXTRA_LDS 0u
#endif
// (both variable-size parts are rounded up to 16 bytes, so that everything behind them stays aligned whatever capTs and WB_WIN are)
__host__ __device__ inline size_t wb_up16(size_t n) { return (n + 15) & ~(size_t)15; }
__host__ __device__ inline size_t wb_part_a(u32 capTs) { const size_t m = wb_si(capTs); return wb_up16(m > WB_WIN * 64 ? m : WB_WIN * 64); }   // cnt | marks
__host__ __device__ inline size_t wb_part_b(u32 capTs) { const size_t t = wb_si(capTs); return wb_up16(t > WB_WIN * 32 ? t : WB_WIN * 32); }   // symTab | coarse
// `withCum`: the carve has cumP (the CTable builders use it; k_fse_dbuild does not).  At tableLog 11: 7,168 bytes without, 7,696 with
// (22 / 21 builds per CU by LDS; the 32-cell kernels' registers allow 24 and more), at tableLog 12: 9,984 / 10,512 (16 / 15; the
// 64-cell kernels' registers allow 16)
__host__ __device__ inline size_t wave_build_lds_bytes(u32 capTs, bool withCum) { return wb_part_a(capTs) + wb_part_b(capTs) + 512 + 256 + (withCum ? 528 : 0) + WB_EXTRA_LDS; }
DEV WaveBuildLds wave_build_carve(u8* base, u32 capTs, bool withCum)
{
    WaveBuildLds w;
    w.cnt = (u32*)base; w.marks = base; base += wb_part_a(capTs);         // 16-byte aligned parts first
    w.coarse = (u16*)base; w.symTab = base; base += wb_part_b(capTs);
    w.nrm = (s16*)base; base += 512;
    w.symP = base; base += 256;
    w.cumP = withCum ? (u16*)base : nullptr;
    return w;
}
// cells per lane a builder instantiation keeps in registers: 32 where no table of the launch has more than 2048 cells, else 64
__host__ __device__ inline bool wb_small(u32 capTs) { return capTs <= 2048u; }

DEV u32 wb_bytesum(u32 v) { return __builtin_amdgcn_sad_u8(v, 0u, 0u); }
DEV u32 wb_scan_excl(u32 v, u32 lane, u32* total)         // exclusive prefix sum over the 64 lanes
{
#if FSEHIP_DPP_SCANS
    const u32 incl = group_scan_incl<64, ScanAdd>(v, lane);
    *total = group_last<64>(incl, lane);
#else
    u32 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const u32 o = (u32)__shfl_up((int)incl, off, WAVE); if ((int)lane >= off) incl += o; }
    *total = (u32)__shfl((int)incl, 63, WAVE);
#endif
    return incl - v;
}

// an empty asm that "changes" v: what is computed from v per group cannot be hoisted out of the window loop (the compiler would
// otherwise keep the symbols, addresses and masks of all 64 cells live at once: 256 VGPRs)
DEV void wb_opaque(u32& v) { asm volatile("" : "+v"(v)); }
#define WB_MAXC ((1u << FSEHIP_FSE_MAX_TABLELOG) >> 6)                   // cells per lane at the largest table (64)

// All 64 lanes of one wave call this with uniform arguments; w.nrm holds the counters.  Uses __syncthreads(), so the
// workgroup must be exactly this wave.  Returns the fastMode flag of FSE_buildDTable (no counter >= tableSize/2).
// MAXC = the cells per lane the instantiation has registers for (the symbols and local ranks of a lane's cells, four to a register):
// the CALLER guarantees 1 << tl <= 64 * MAXC (the kernels check it, uniformly, before they get here).
template <u32 MAXC, class Payload, class Emit>
DEV bool wave_spread_rank(const WaveBuildLds& w, u32 maxSV, u32 tl, u32 lane, Payload&& payload, Emit&& emit)
{
#ifdef FSE_WB_TIMING
    unsigned long long TT[8];
#endif
    WBT(0)
    const u32 ts = 1u << tl, mask = ts - 1, step = WB_TSTEP(ts);
    const u32 C = ts >= 64 ? ts >> 6 : 1;                                 // cells (and visits) per lane
    const bool act = lane * C < ts;
    const u32 m0 = lane * C;
    static_assert(MAXC % 8 == 0 && MAXC <= WB_MAXC, "cells per lane: whole groups of eight, at most the largest table's");
    u8* const marks = w.marks;                                            // [ts] scratch of the spread (cnt[] is not in use yet)
    // ---- per symbol: lane l looks after symbols 4l .. 4l+3
    int n[4];
    {   const uint2 raw = *(const uint2*)(w.nrm + 4 * lane);
        n[0] = (s16)(raw.x & 0xFFFFu); n[1] = (s16)(raw.x >> 16); n[2] = (s16)(raw.y & 0xFFFFu); n[3] = (s16)(raw.y >> 16);
    }
    u32 lanePos = 0, laneLow = 0, laneAny = 0; bool big = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (4 * lane + i > maxSV) n[i] = 0;
        lanePos += n[i] > 0 ? (u32)n[i] : 0u; laneLow += n[i] == -1; laneAny += n[i] != 0;
        big |= n[i] >= (int)(ts >> 1);
    }
    // one packed scan: positive counts (<= 4096: 13 bits) | low-probability symbols (9 bits) | symbols in use (9 bits)
    u32 totals;
    const u32 base3 = wb_scan_excl(lanePos | (laneLow << 13) | (laneAny << 22), lane, &totals);
    u32 posBase = base3 & 0x1FFFu, lowBase = (base3 >> 13) & 0x1FFu, anyBase = base3 >> 22;
    const u32 nLow = (totals >> 13) & 0x1FFu, nAny = totals >> 22;
    const int high = (int)ts - 1 - (int)nLow;                             // highThreshold (-1: every cell is a low-probability one)
    // clear the spread marks
    if (act) { if (C >= 4) for (u32 i = 0; i < C; i += 4) *(u32*)(marks + wb_si(m0 + i)) = 0; else for (u32 i = 0; i < C; ++i) marks[wb_si(m0 + i)] = 0; }
    __syncthreads();
    WBT(1)
    // symbols in use (for the per-symbol pass below); low-probability symbols take the top cells; every symbol with a
    // positive count marks the first of its kept visits with itself
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (n[i] != 0) w.symP[anyBase++] = (u8)(4 * lane + i);
        if (n[i] > 0) { marks[wb_si(posBase)] = (u8)(4 * lane + i); posBase += (u32)n[i]; }
        else if (n[i] == -1) { w.symTab[wb_si(ts - 1 - lowBase)] = (u8)(4 * lane + i); ++lowBase; }
    }
    // ---- spread: lane l visits m in [l*C, (l+1)*C); the k-th kept visit belongs to the symbol of the last mark at or
    //      before k, i.e. a running maximum over the marks (symbols ascend with k)
    u32 nv = 0;
    if (act) { u32 u = (m0 * step) & mask; for (u32 i = 0; i < C; ++i) { nv += (int)u <= high; u = (u + step) & mask; } }
    u32 totalKept;
    const u32 k0 = wb_scan_excl(nv, lane, &totalKept);
    __syncthreads();
    WBT(2)
    // (eight marks at a time so that the LDS round trips overlap; indices are clamped, unused values are ignored)
    u32 localMax = 0;
    for (u32 i = 0; i < nv; i += 8) {
        u32 v[8];
#pragma unroll
        for (u32 j = 0; j < 8; ++j) { const u32 idx = k0 + i + j; v[j] = marks[wb_si(idx < ts ? idx : ts - 1)]; }
#pragma unroll
        for (u32 j = 0; j < 8; ++j) if (i + j < nv) localMax = v[j] > localMax ? v[j] : localMax;
    }
    u32 run = localMax;                                                   // inclusive prefix maximum over the lanes ...
#if FSEHIP_DPP_SCANS
    run = group_scan_incl<64, ScanMax>(run, lane);
    run = dpp_mov<0x138, 0xF, true>(0u, run);                            // ... made exclusive: wave_shr:1, lane 0 gets 0
#else
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const u32 o = (u32)__shfl_up((int)run, off, WAVE); if ((int)lane >= off) run = o > run ? o : run; }
    run = (u32)__shfl_up((int)run, 1, WAVE);                             // ... made exclusive
    if (lane == 0) run = 0;
#endif
    if (act && nv) {
        u32 u = (m0 * step) & mask, k = k0;
        u32 i = 0;
        for (; i + 8 <= C; i += 8) {
            u32 uu[8], v[8]; bool keep[8];
#pragma unroll
            for (u32 j = 0; j < 8; ++j) {
                uu[j] = u; keep[j] = (int)u <= high;
                v[j] = marks[wb_si(k < ts ? k : ts - 1)];
                k += keep[j]; u = (u + step) & mask;
            }
#pragma unroll
            for (u32 j = 0; j < 8; ++j) if (keep[j]) { run = v[j] > run ? v[j] : run; w.symTab[wb_si(uu[j])] = (u8)run; }
        }
        for (; i < C; ++i) {
            if ((int)u <= high) { const u32 v = marks[wb_si(k)]; ++k; run = v > run ? v : run; w.symTab[wb_si(u)] = (u8)run; }
            u = (u + step) & mask;
        }
    }
    __syncthreads();
    WBT(3)

    // ---- the symbols of my cells, four to a register (sym[c >> 2] byte c & 3 = symbol of cell m0 + c), and their ranks inside
    //      my range, packed the same way (a rank is < C <= 64).  Cells go in groups of eight; C is 1, 2 or 4 (one partial group)
    //      or a multiple of 8.  The loops over the groups are unrolled so that the arrays stay in registers.
    const u32 nj = C < 8 ? C : 8;                                         // cells per group
    u32 sym[MAXC / 4], lr[MAXC / 4];
#pragma unroll
    for (u32 q = 0; q < MAXC / 4; ++q) { sym[q] = 0; lr[q] = 0; }
    if (act) {
        if (C >= 8) {
#pragma unroll
            for (u32 g = 0; g < MAXC / 8; ++g)
                if (8 * g < C) {
                    const u32* const syp = (const u32*)(w.symTab + wb_si(m0 + 8 * g));   // 8 cells of one row: two aligned dwords
                    sym[2 * g] = syp[0]; sym[2 * g + 1] = syp[1];
                }
        } else {
#pragma unroll
            for (u32 j = 0; j < 4; ++j) if (j < C) sym[0] |= (u32)w.symTab[wb_si(m0 + j)] << (8 * j);
        }
    }
    // ---- per window of WB_WIN symbols: rank inside the lane range, running sums over the lane groups, emit.
    const u32 sh8 = 8 * (lane & 3u), grp = lane >> 2;
    const u32 belowMask = (1u << sh8) - 1u;
    const bool single = maxSV < WB_WIN;                                   // uniform: one window, nothing to predicate
    for (u32 base = 0; base <= maxSV; base += WB_WIN) {
        {   const u32 rows = (maxSV + 1 - base) < WB_WIN ? (maxSV + 1 - base) : WB_WIN;
            for (u32 i = 4 * lane; i < rows * 16; i += 256) *(uint4*)(w.cnt + i) = make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        // rank inside the lane range: LDS atomics return the previous count, in program order.  Eight cells at a time so
        // that the LDS round trips overlap.  A cell of a later window keeps the rank an earlier window gave it.
        if (act) {
#pragma unroll
            for (u32 g = 0; g < MAXC / 8; ++g) {
                if (8 * g >= C) break;                                    // uniform
                wb_opaque(sym[2 * g]); wb_opaque(sym[2 * g + 1]);
                u32 old[8]; bool in[8];
#pragma unroll
                for (u32 j = 0; j < 8; ++j) {
                    const u32 s = ((sym[2 * g + (j >> 2)] >> (8 * (j & 3))) & 0xFFu) - base;
                    in[j] = j < nj && (single || s < WB_WIN);
                    old[j] = 0;
                    if (in[j]) old[j] = atomicAdd(&w.cnt[s * 16 + grp], 1u << sh8);
                }
#pragma unroll
                for (u32 h = 0; h < 2; ++h) {
                    u32 r = lr[2 * g + h];
#pragma unroll
                    for (u32 k = 0; k < 4; ++k) {
                        const u32 j = 4 * h + k;
                        if (in[j]) r = (r & ~(0xFFu << (8 * k))) | (((old[j] >> sh8) & 0xFFu) << (8 * k));
                    }
                    lr[2 * g + h] = r;
                }
            }
        }
        __syncthreads();
        WBT(4)
        // per symbol in use (lane l: the l-th, l+64-th, ... of them): running sum over the 16 lane groups
        for (u32 j = lane; j < nAny; j += 64) {
            const u32 s = (u32)w.symP[j] - base;
            if (!single && s >= WB_WIN) continue;
            const uint4* const row = (const uint4*)(w.cnt + s * 16);
            const uint4 c0 = row[0], c1 = row[1], c2 = row[2], c3 = row[3];
            u32 r[16];
            u32 acc = 0;
#define WB_ACC(k, v) r[k] = acc; acc += wb_bytesum(v);
            WB_ACC(0, c0.x) WB_ACC(1, c0.y) WB_ACC(2, c0.z) WB_ACC(3, c0.w) WB_ACC(4, c1.x) WB_ACC(5, c1.y) WB_ACC(6, c1.z) WB_ACC(7, c1.w)
            WB_ACC(8, c2.x) WB_ACC(9, c2.y) WB_ACC(10, c2.z) WB_ACC(11, c2.w) WB_ACC(12, c3.x) WB_ACC(13, c3.y) WB_ACC(14, c3.z) WB_ACC(15, c3.w)
#undef WB_ACC
            uint4* const out = (uint4*)(w.coarse + s * 16);
            out[0] = make_uint4(r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16));
            out[1] = make_uint4(r[8] | (r[9] << 16), r[10] | (r[11] << 16), r[12] | (r[13] << 16), r[14] | (r[15] << 16));
        }
        __syncthreads();
        WBT(5)
        // emit: everything a cell needs is gathered for eight cells before the first one is emitted
        if (act) {
#pragma unroll
            for (u32 g = 0; g < MAXC / 8; ++g) {
                if (8 * g >= C) break;                                    // uniform
                wb_opaque(sym[2 * g]); wb_opaque(sym[2 * g + 1]);
                u32 mg = m0 + 8 * g; wb_opaque(mg);
                u32 sf[8], co[8], cn[8], pl[8]; bool in[8];
#pragma unroll
                for (u32 j = 0; j < 8; ++j) {
                    sf[j] = (sym[2 * g + (j >> 2)] >> (8 * (j & 3))) & 0xFFu;
                    const u32 sw = sf[j] - base;
                    in[j] = j < nj && (single || sw < WB_WIN);
                    const u32 row = in[j] ? sw : 0u;
                    co[j] = w.coarse[row * 16 + grp]; cn[j] = w.cnt[row * 16 + grp]; pl[j] = payload(sf[j]);
                }
#pragma unroll
                for (u32 j = 0; j < 8; ++j) {
                    const u32 local = (lr[2 * g + (j >> 2)] >> (8 * (j & 3))) & 0xFFu;
                    if (in[j]) emit(mg + j, sf[j], local + co[j] + wb_bytesum(cn[j] & belowMask), pl[j]);
                }
            }
        }
        __syncthreads();
    }
    WBT(6)
#ifdef FSE_WB_TIMING
    if (lane == 0 && blockIdx.x < 4096) for (int q = 0; q < 6; ++q) g_wbTiming[8 * blockIdx.x + q] = TT[q + 1] - TT[q];
#endif
    return !__any(big);
}

// devtest.hip -- TEST ONLY, never linked into libfsehip.so: every device building block of dev_common.h, wave_glue.h, planes_dev.h, bitreader.h
// and wb_scan_excl / wb_bytesum of fse_wave_build.h behind a trivial kernel, so that tests/test_gpu_devtest.py can put each of them against a
// numpy model of its definition (tests/devtest_models.py).  The product headers are included as they are.  Built twice by csrc/Makefile:
// libfsehip_devtest.so (the DPP forms) and libfsehip_devtest_shfl.so (-DFSEHIP_NO_DPP_SCANS, the shuffle forms).
//
// One thread per work item.  Item t reads its record of Op::IN dwords at in + 4 IN t and stores Op::OUT dwords at out + 4 OUT t; some operations
// read a payload that follows the n records.  Blocks hold 64 or 256 threads and n is a multiple of the block: every wave is full and in uniform
// control flow, which is the helpers' precondition.  Whatever a record holds, a kernel reads and writes inside the two buffers only: indices
// that come from a record are checked first, and a refused record stores DT_REFUSED in its outputs.
#include "planes_dev.h"
#include "wave_glue.h"
#include "bitreader.h"
#include "fse_wave_build.h"
#include <string.h>
#include <stdio.h>

#define DT_REFUSED 0xBAD0BAD0u
#define DT_BR_STREAM 32          // bytes of a bit reader record's stream field
#define DT_BR_STEPS 64           // steps of a bit reader script
#define DT_FS_CELLS 32           // cells of an fse_step record's table
#define DT_FS_STEPS 32

namespace {
struct DtCtx { u64 a; const u8* in; size_t inBytes; size_t n; };   // a: the run-time argument; in: the whole input buffer (records, then payload)
DEV u64 dt_ld64(const u32* p) { return (u64)p[0] | ((u64)p[1] << 32); }
DEV void dt_st64(u32* p, u64 v) { p[0] = (u32)v; p[1] = (u32)(v >> 32); }

// ---- cross-lane ----
template <int W, class Op> struct DGroupScan { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { o[0] = group_scan_incl<W, Op>(i[0], lane & (u32)(W - 1)); } };
template <int W> struct DGroupLast { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { o[0] = group_last<W>(i[0], lane); } };
template <int W, class Op> struct DGroupReduce { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { o[0] = group_reduce<W, Op>(i[0], lane); } };
template <int W> struct DGroupScan64 { enum { IN = 2, OUT = 2 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { dt_st64(o, group_scan_incl_add64<W>(dt_ld64(i), lane & (u32)(W - 1))); } };
template <int W> struct DGroupLast64 { enum { IN = 2, OUT = 2 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { dt_st64(o, group_last64<W>(dt_ld64(i), lane)); } };
template <int D> struct DLaneXor { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { o[0] = lane_xor<D>(i[0], lane); } };
struct DLaneXorAny {
    enum { IN = 1, OUT = 1 };
    static bool ok(u64 d) { return d == 1 || d == 2 || d == 4 || d == 8 || d == 16 || d == 32; }
    DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx& c) { o[0] = lane_xor_any(i[0], (u32)c.a, lane); }
};
struct DWaveMaxU32 { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { o[0] = wave_max_u32(i[0]); } };
struct DWaveMaxI32 { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { o[0] = (u32)wave_max_i32((int)i[0]); } };
template <int W> struct DWgSum { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { o[0] = wg_sum<W>(i[0]); } };
template <int W> struct DWgSum64 { enum { IN = 2, OUT = 2 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { dt_st64(o, wg_sum64<W>(dt_ld64(i))); } };
template <int W> struct DWgMax { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { o[0] = wg_max<W>(i[0]); } };
template <int W> struct DWgMin { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { o[0] = wg_min<W>(i[0]); } };
template <int W> struct DWgAny { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { o[0] = wg_any<W>(i[0] != 0, lane) ? 1u : 0u; } };
template <int W> struct DWgScanExcl { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { o[0] = wg_scan_excl<W>(i[0], lane); } };
template <int W> struct DWgScanExcl64 { enum { IN = 2, OUT = 2 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { dt_st64(o, wg_scan_excl64<W>(dt_ld64(i), lane)); } };
template <int W> struct DWgSuffixMin { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { o[0] = wg_suffix_min_excl<W>(i[0], lane); } };
struct DWbScanExcl { enum { IN = 1, OUT = 2 }; DEV static void run(const u32* i, u32* o, u32 lane, const DtCtx&) { u32 total; o[0] = wb_scan_excl(i[0], lane, &total); o[1] = total; } };
struct DWbByteSum { enum { IN = 1, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { o[0] = wb_bytesum(i[0]); } };

// ---- plane arithmetic ----
template <int E> struct DPlZz { enum { IN = 4, OUT = 2 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { dt_st64(o, pl_zz<E>(dt_ld64(i), dt_ld64(i + 2))); } };
template <int E> struct DPlUnzz { enum { IN = 4, OUT = 2 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { dt_st64(o, pl_unzz<E>(dt_ld64(i), dt_ld64(i + 2))); } };
template <int E, bool INV> struct DPlSub4 {                  // w[4], b[4] -> w[4]
    enum { IN = 8, OUT = 4 };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx&)
    {
        u32 w[4], b[4];
        for (int k = 0; k < 4; ++k) { w[k] = i[k]; b[k] = i[4 + k]; }
        pl_sub4<E, INV>(w, b);
        for (int k = 0; k < 4; ++k) o[k] = w[k];
    }
};
template <int E> struct DPlDeinterleave {                    // w[4 E] -> o[E][4]
    enum { IN = 4 * E, OUT = 4 * E };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx&)
    {
        u32 w[4 * E], p[E][4];
        for (int k = 0; k < 4 * E; ++k) w[k] = i[k];
        pl_deinterleave<E>(w, p);
        for (int k = 0; k < 4 * E; ++k) o[k] = p[k / 4][k % 4];
    }
};
template <int E> struct DPlInterleave {                      // o[E][4] -> w[4 E]
    enum { IN = 4 * E, OUT = 4 * E };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx&)
    {
        u32 w[4 * E], p[E][4];
        for (int k = 0; k < 4 * E; ++k) p[k / 4][k % 4] = i[k];
        pl_interleave<E>(w, p);
        for (int k = 0; k < 4 * E; ++k) o[k] = w[k];
    }
};
// the chunk of 16 E bytes at byte `off` of the input buffer (off: the record), which lies in the payload; the bytes in front of it that the helper
// reads (FRONT of them, none where the chunk starts a run) lie in the payload too
template <int BYTES, int FRONT> DEV bool dt_chunk_ok(u64 off, bool runStart, const DtCtx& c)
{
    const u64 payload = (u64)c.n * 4;
    return off >= payload + (runStart ? 0 : FRONT) && off + BYTES <= c.inBytes;
}
template <int E, bool RS> struct DPpPrev {
    enum { IN = 1, OUT = 4 * E, PAYLOAD = 1 };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx& c)
    {
        u32 w[4 * E], pv[4 * E];
        if (!dt_chunk_ok<16 * E, E>(i[0], RS, c)) { for (int k = 0; k < 4 * E; ++k) o[k] = DT_REFUSED; return; }
        __builtin_memcpy(w, c.in + i[0], 16 * E);
        pp_prev<E>(pv, w, c.in + i[0], RS);
        for (int k = 0; k < 4 * E; ++k) o[k] = pv[k];
    }
};
template <int E, int S, bool RS> struct DPsPrev {
    enum { IN = 1, OUT = 4 * E, PAYLOAD = 1 };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx& c)
    {
        u32 w[4 * E], pv[4 * E];
        if (!dt_chunk_ok<16 * E, 4 * ((S * E + 3) / 4)>(i[0], RS, c)) { for (int k = 0; k < 4 * E; ++k) o[k] = DT_REFUSED; return; }
        __builtin_memcpy(w, c.in + i[0], 16 * E);
        ps_prev<E, S>(pv, w, c.in + i[0], RS);
        for (int k = 0; k < 4 * E; ++k) o[k] = pv[k];
    }
};
struct DPpAdd16x2 { enum { IN = 2, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { o[0] = pp_add16x2(i[0], i[1]); } };
struct DPpAdd8x4 { enum { IN = 2, OUT = 1 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { o[0] = pp_add8x4(i[0], i[1]); } };
template <int E> struct DPpPrefix {                          // w[4 E] -> w[4 E], total
    enum { IN = 4 * E, OUT = 4 * E + 2 };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx&)
    {
        u32 w[4 * E];
        for (int k = 0; k < 4 * E; ++k) w[k] = i[k];
        const u64 total = pp_prefix<E>(w);
        for (int k = 0; k < 4 * E; ++k) o[k] = w[k];
        dt_st64(o + 4 * E, total);
    }
};
template <int E> struct DPpCarry {                           // w[4 E], c -> w[4 E]
    enum { IN = 4 * E + 2, OUT = 4 * E };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx&)
    {
        u32 w[4 * E];
        for (int k = 0; k < 4 * E; ++k) w[k] = i[k];
        pp_carry<E>(w, dt_ld64(i + 4 * E));
        for (int k = 0; k < 4 * E; ++k) o[k] = w[k];
    }
};
template <int E> struct DPsUnpack {                          // w[4 E] -> x[16], each as 64 bits
    enum { IN = 4 * E, OUT = 32 };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx&)
    {
        u32 w[4 * E]; ps_t<E> x[16];
        for (int k = 0; k < 4 * E; ++k) w[k] = i[k];
        ps_unpack<E>(x, w);
        for (int q = 0; q < 16; ++q) dt_st64(o + 2 * q, (u64)x[q]);
    }
};
template <int E> struct DPsPack {                            // x[16], each as 64 bits (E < 8: the low 32 are the register) -> w[4 E]
    enum { IN = 32, OUT = 4 * E };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx&)
    {
        u32 w[4 * E]; ps_t<E> x[16];
        for (int q = 0; q < 16; ++q) x[q] = (ps_t<E>)dt_ld64(i + 2 * q);
        ps_pack<E>(w, x);
        for (int k = 0; k < 4 * E; ++k) o[k] = w[k];
    }
};
template <int S, class T> struct DPsRotate {                 // v[S] (each as 64 bits), r -> v[S]
    enum { IN = 2 * S + 1, OUT = 2 * S };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx&)
    {
        T v[S];
        for (int k = 0; k < S; ++k) v[k] = (T)dt_ld64(i + 2 * k);
        ps_rotate<S, T>(v, i[2 * S]);
        for (int k = 0; k < S; ++k) dt_st64(o + 2 * k, (u64)v[k]);
    }
};

// ---- index logic ----
struct DPlSize { enum { IN = 4, OUT = 2 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { dt_st64(o, i[3] ? pl_size(dt_ld64(i), i[2], i[3]) : 0); } };
struct DPlStart { enum { IN = 4, OUT = 2 }; DEV static void run(const u32* i, u32* o, u32, const DtCtx&) { dt_st64(o, i[3] ? pl_start(dt_ld64(i), i[2], i[3]) : 0); } };
template <int E> struct DPlShare {                           // s0, n, lo, alignAddr (64 bits each), alignStride -> e0, eb, et, e1, nch
    enum { IN = 9, OUT = 10 };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx&)
    {
        const PlShare r = pl_share<E>(dt_ld64(i), dt_ld64(i + 2), dt_ld64(i + 4), dt_ld64(i + 6), i[8]);
        dt_st64(o, r.e0); dt_st64(o + 2, r.eb); dt_st64(o + 4, r.et); dt_st64(o + 6, r.e1); dt_st64(o + 8, r.nch);
    }
};
// payload: a = nT offsets (keys) of 64 bits; the record is the work item w (the query q) -> found, index
struct DPlFind {
    enum { IN = 2, OUT = 4, PAYLOAD = 1 };
    static bool ok(u64 nT) { return nT < ((u64)1 << 20); }
    static size_t payload(u64 nT) { return (size_t)nT * 8; }
    DEV static void run(const u32* i, u32* o, u32, const DtCtx& c)
    {
        size_t at = ~(size_t)0;
        const bool found = pl_find((const u64*)(c.in + c.n * 8), (size_t)c.a, dt_ld64(i), at);
        dt_st64(o, found ? 1 : 0); dt_st64(o + 2, found ? (u64)at : ~(u64)0);
    }
};
struct DPlLastLe {
    enum { IN = 2, OUT = 2, PAYLOAD = 1 };
    static bool ok(u64 nT) { return nT >= 1 && nT < ((u64)1 << 20); }              // (n >= 1 is the helper's precondition)
    static size_t payload(u64 nT) { return (size_t)nT * 8; }
    DEV static void run(const u32* i, u32* o, u32, const DtCtx& c)
    {
        const u64* K = (const u64*)(c.in + c.n * 8);
        dt_st64(o, (u64)pl_last_le((size_t)c.a, dt_ld64(i), [K](size_t j) { return K[j]; }));
    }
};

// ---- bit reader ----
// record: n (bytes of the stream, <= DT_BR_STREAM), steps (<= DT_BR_STEPS), the stream, the steps as op | nb << 8 (op 0: read, 1: read_fast,
// 2: reload; nb <= 32).  out: init's return (64 bits), then at, used, win (64 bits) after init and, after every step, its value or status and
// the same four words
DEV void dt_br_state(u32* o, const BitReader& r) { o[0] = (u32)r.at; o[1] = r.used; dt_st64(o + 2, r.win); }
struct DBitReader {
    enum { IN = 2 + DT_BR_STREAM / 4 + DT_BR_STEPS, OUT = 6 + 5 * DT_BR_STEPS };
    DEV static void run(const u32* i, u32* o, u32, const DtCtx&)
    {
        for (int k = 0; k < OUT; ++k) o[k] = 0;
        const u32 n = i[0], steps = i[1];
        if (n > DT_BR_STREAM || steps > DT_BR_STEPS) { o[0] = DT_REFUSED; return; }
        BitReader r;
        dt_st64(o, (u64)r.init((const u8*)(i + 2), n));
        dt_br_state(o + 2, r);
        for (u32 s = 0; s < steps; ++s) {
            const u32 st = i[2 + DT_BR_STREAM / 4 + s], op = st & 0xFFu, nb = st >> 8;
            u32* q = o + 6 + 5 * s;
            if (op > 2 || nb > 32) { q[0] = DT_REFUSED; continue; }
            q[0] = op == 0 ? r.read(nb) : op == 1 ? r.read_fast(nb) : (u32)r.reload();
            dt_br_state(q + 1, r);
        }
    }
};
// record: n, steps (<= DT_FS_STEPS), the first state, the stream, DT_FS_CELLS cells.  a: fast.  out: init's return, then per step the symbol,
// the new state, reload's status behind it, at and used.  A state outside the cells ends the script
struct DFseStep {
    enum { IN = 3 + DT_BR_STREAM / 4 + DT_FS_CELLS, OUT = 2 + 5 * DT_FS_STEPS };
    static bool ok(u64 fast) { return fast <= 1; }
    DEV static void run(const u32* i, u32* o, u32, const DtCtx& c)
    {
        for (int k = 0; k < OUT; ++k) o[k] = 0;
        const u32 n = i[0], steps = i[1];
        u32 state = i[2];
        if (n > DT_BR_STREAM || steps > DT_FS_STEPS) { o[0] = DT_REFUSED; return; }
        BitReader r;
        dt_st64(o, (u64)r.init((const u8*)(i + 3), n));
        const u32* cells = i + 3 + DT_BR_STREAM / 4;
        for (u32 s = 0; s < steps; ++s) {
            u32* q = o + 2 + 5 * s;
            if (state >= DT_FS_CELLS) { q[0] = DT_REFUSED; break; }
            q[0] = fse_step(state, r, cells, c.a != 0);
            q[1] = state;
            q[2] = (u32)r.reload(); q[3] = (u32)r.at; q[4] = r.used;
        }
    }
};

template <class Op> __global__ void k_devtest(const u32* in, u32* out, DtCtx c)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;                // (the grid holds exactly n threads)
    Op::run(in + t * Op::IN, out + t * Op::OUT, wg_lane(), c);
}

// what an operation adds to the plain form: a check of the run-time argument, a payload behind the records
template <class Op, class = void> struct DtOk { static bool ok(u64) { return true; } };
template <class Op> struct DtOk<Op, decltype((void)Op::ok(0))> { static bool ok(u64 a) { return Op::ok(a); } };
template <class Op, class = void> struct DtPayload { static bool fits(size_t extra, u64) { return extra == 0; } };
template <class Op> struct DtPayload<Op, decltype((void)Op::PAYLOAD)> { static bool fits(size_t, u64) { return true; } };       // any size: the kernel checks its offsets
template <> struct DtPayload<DPlFind, void> { static bool fits(size_t extra, u64 a) { return extra == DPlFind::payload(a); } };
template <> struct DtPayload<DPlLastLe, void> { static bool fits(size_t extra, u64 a) { return extra == DPlLastLe::payload(a); } };

struct DtCall { u64 a; size_t n; const void* in; size_t inBytes; void* out; size_t outBytes; unsigned threads; hipStream_t stream; };
template <class Op> int dt_go(const DtCall& q)
{
    if (!DtOk<Op>::ok(q.a)) return (int)hipErrorInvalidValue;
    if (q.n == 0 || q.n % q.threads || q.n / q.threads >= ((size_t)1 << 24)) return (int)hipErrorInvalidValue;
    const size_t rec = q.n * Op::IN * 4;
    if (q.inBytes < rec || q.inBytes >= ((size_t)1 << 31) || !DtPayload<Op>::fits(q.inBytes - rec, q.a) || q.outBytes != q.n * Op::OUT * 4) return (int)hipErrorInvalidValue;
    if (!q.in || !q.out || ((uintptr_t)q.in & 15u) || ((uintptr_t)q.out & 3u)) return (int)hipErrorInvalidValue;
    const DtCtx c = { q.a, (const u8*)q.in, q.inBytes, q.n };
    k_devtest<Op><<<(unsigned)(q.n / q.threads), q.threads, 0, q.stream>>>((const u32*)q.in, (u32*)q.out, c);
    return (int)hipGetLastError();
}

// the operations: X(name, a, b, the wrapper).  a and b are the template arguments; DT_RT: a is a run-time argument that the wrapper checks
#define DT_RT (-1)
#define DT_FOR_W(X, name, T) X(name, 8, 0, T<8>) X(name, 16, 0, T<16>) X(name, 32, 0, T<32>) X(name, 64, 0, T<64>)
#define DT_FOR_W_OP1(X, name, T, W) X(name, W, 0, T<W, ScanAdd>) X(name, W, 1, T<W, ScanMax>) X(name, W, 2, T<W, ScanMin>)
#define DT_FOR_W_OP(X, name, T) DT_FOR_W_OP1(X, name, T, 8) DT_FOR_W_OP1(X, name, T, 16) DT_FOR_W_OP1(X, name, T, 32) DT_FOR_W_OP1(X, name, T, 64)
#define DT_FOR_E(X, name, T) X(name, 1, 0, T<1>) X(name, 2, 0, T<2>) X(name, 4, 0, T<4>) X(name, 8, 0, T<8>)
#define DT_FOR_E_BOOL(X, name, T) X(name, 1, 0, T<1, false>) X(name, 1, 1, T<1, true>) X(name, 2, 0, T<2, false>) X(name, 2, 1, T<2, true>) \
    X(name, 4, 0, T<4, false>) X(name, 4, 1, T<4, true>) X(name, 8, 0, T<8, false>) X(name, 8, 1, T<8, true>)
// ps_prev: a = E, b = S + 16 runStart
#define DT_PS_PREV1(X, E, S) X("ps_prev", E, S, DPsPrev<E, S, false>) X("ps_prev", E, S + 16, DPsPrev<E, S, true>)
#define DT_PS_PREV(X, E) DT_PS_PREV1(X, E, 2) DT_PS_PREV1(X, E, 3) DT_PS_PREV1(X, E, 4) DT_PS_PREV1(X, E, 5) DT_PS_PREV1(X, E, 6) DT_PS_PREV1(X, E, 7) DT_PS_PREV1(X, E, 8)
// ps_rotate: a = S, b = bytes of T
#define DT_PS_ROT1(X, S) X("ps_rotate", S, 4, DPsRotate<S, u32>) X("ps_rotate", S, 8, DPsRotate<S, u64>)
#define DT_OPS(X) \
    DT_FOR_W_OP(X, "group_scan_incl", DGroupScan) DT_FOR_W(X, "group_last", DGroupLast) DT_FOR_W_OP(X, "group_reduce", DGroupReduce) \
    DT_FOR_W(X, "group_scan_incl_add64", DGroupScan64) DT_FOR_W(X, "group_last64", DGroupLast64) \
    X("lane_xor", 1, 0, DLaneXor<1>) X("lane_xor", 2, 0, DLaneXor<2>) X("lane_xor", 4, 0, DLaneXor<4>) X("lane_xor", 8, 0, DLaneXor<8>) \
    X("lane_xor", 16, 0, DLaneXor<16>) X("lane_xor", 32, 0, DLaneXor<32>) X("lane_xor_any", DT_RT, 0, DLaneXorAny) \
    X("wave_max_u32", 0, 0, DWaveMaxU32) X("wave_max_i32", 0, 0, DWaveMaxI32) \
    DT_FOR_W(X, "wg_sum", DWgSum) DT_FOR_W(X, "wg_sum64", DWgSum64) DT_FOR_W(X, "wg_max", DWgMax) DT_FOR_W(X, "wg_min", DWgMin) \
    DT_FOR_W(X, "wg_any", DWgAny) DT_FOR_W(X, "wg_scan_excl", DWgScanExcl) DT_FOR_W(X, "wg_scan_excl64", DWgScanExcl64) \
    DT_FOR_W(X, "wg_suffix_min_excl", DWgSuffixMin) X("wb_scan_excl", 0, 0, DWbScanExcl) X("wb_bytesum", 0, 0, DWbByteSum) \
    DT_FOR_E(X, "pl_zz", DPlZz) DT_FOR_E(X, "pl_unzz", DPlUnzz) DT_FOR_E_BOOL(X, "pl_sub4", DPlSub4) \
    DT_FOR_E(X, "pl_deinterleave", DPlDeinterleave) DT_FOR_E(X, "pl_interleave", DPlInterleave) DT_FOR_E_BOOL(X, "pp_prev", DPpPrev) \
    X("pp_add16x2", 0, 0, DPpAdd16x2) X("pp_add8x4", 0, 0, DPpAdd8x4) DT_FOR_E(X, "pp_prefix", DPpPrefix) DT_FOR_E(X, "pp_carry", DPpCarry) \
    DT_PS_PREV(X, 1) DT_PS_PREV(X, 2) DT_PS_PREV(X, 4) DT_PS_PREV(X, 8) DT_FOR_E(X, "ps_unpack", DPsUnpack) DT_FOR_E(X, "ps_pack", DPsPack) \
    DT_PS_ROT1(X, 2) DT_PS_ROT1(X, 3) DT_PS_ROT1(X, 4) DT_PS_ROT1(X, 5) DT_PS_ROT1(X, 6) DT_PS_ROT1(X, 7) DT_PS_ROT1(X, 8) \
    X("pl_size", 0, 0, DPlSize) X("pl_start", 0, 0, DPlStart) DT_FOR_E(X, "pl_share", DPlShare) \
    X("pl_find", DT_RT, 0, DPlFind) X("pl_last_le", DT_RT, 0, DPlLastLe) X("bitreader", 0, 0, DBitReader) X("fse_step", DT_RT, 0, DFseStep)
}   // namespace

extern "C" {
// Runs operation `name` with the template arguments a and b (0 where it has none; for lane_xor_any, pl_find, pl_last_le and fse_step a is the
// run-time argument) on n work items in blocks of threadsPerBlock threads.  hipErrorInvalidValue, with nothing launched: an unknown name, an
// (a, b) that is not instantiated, n no positive multiple of threadsPerBlock, threadsPerBlock other than 64 or 256, buffers that are null,
// misaligned or not of the operation's sizes.  Asynchronous on `stream`.
FSEHIP_API int FSEHIP_devtest_run(const char* name, long long a, long long b, size_t n, const void* d_in, size_t inBytes, void* d_out, size_t outBytes,
                                  unsigned threadsPerBlock, void* stream)
{
    if (!name || (threadsPerBlock != 64 && threadsPerBlock != 256)) return (int)hipErrorInvalidValue;
    const DtCall q = { (u64)a, n, d_in, inBytes, d_out, outBytes, threadsPerBlock, (hipStream_t)stream };
#define DT_X(NAME, A, B, ...) if (!strcmp(name, NAME) && (A == DT_RT ? a >= 0 : a == A) && b == B) return dt_go<__VA_ARGS__>(q);
    DT_OPS(DT_X)
#undef DT_X
    return (int)hipErrorInvalidValue;
}
// The operations as lines "name a b in out\n" (a = -1: a run-time argument; in, out: dwords per work item) into buf, as far as cap allows, always
// terminated; returns the length of the whole list.
FSEHIP_API size_t FSEHIP_devtest_list(char* buf, size_t cap)
{
    size_t len = 0;
    char line[96];
#define DT_X(NAME, A, B, ...) { const int m = snprintf(line, sizeof line, "%s %d %d %d %d\n", NAME, (int)A, (int)B, (int)__VA_ARGS__::IN, (int)__VA_ARGS__::OUT); \
        for (int k = 0; k < m; ++k, ++len) if (buf && len + 1 < cap) buf[len] = line[k]; }
    DT_OPS(DT_X)
#undef DT_X
    if (buf && cap) buf[len + 1 < cap ? len : cap - 1] = 0;
    return len;
}
// 1: the DPP forms, 0: the shuffle forms (-DFSEHIP_NO_DPP_SCANS)
FSEHIP_API int FSEHIP_devtest_dpp(void) { return FSEHIP_DPP_SCANS; }
// pl_size and pl_start on the host (0 for E == 0)
FSEHIP_API uint64_t FSEHIP_devtest_pl_size(uint64_t n, unsigned p, unsigned E) { return E ? pl_size(n, p, E) : 0; }
FSEHIP_API uint64_t FSEHIP_devtest_pl_start(uint64_t n, unsigned p, unsigned E) { return E ? pl_start(n, p, E) : 0; }
FSEHIP_API uint64_t FSEHIP_devtest_tile(void) { return PLANES_TILE; }
}

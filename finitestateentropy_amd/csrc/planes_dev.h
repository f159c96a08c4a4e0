// planes_dev.h -- what the plane files (planes.hip: byte planes of tensors and their delta forms; planes_seg.hip; planes_win.hip; planes_patch.hip) share: the byte
// shuffle, the delta ops (XOR, subtract and zigzag), the register forms of the predicted planes (planes_pred.hip) and of the strided ones (planes_stride.hip), the arms of the per-tensor kernels (planes_each.hip, planes_each_stride.hip), the plane arithmetic, the search behind every work mapping, a workgroup's share of a tensor, the merge's verdict, the fold of a
// plane's segment results, the dispatch over the element size and the argument checks of the C calls.  Device helpers are inlined into the
// kernels of the file that includes this; nothing here is a kernel.
#pragma once
#include "internal.h"
#include <type_traits>

namespace {
#define PL_THREADS 256
#define HDEV __host__ __device__ __forceinline__
#define PL_TILE_LOG 15
static_assert(PLANES_TILE == ((u64)1 << PL_TILE_LOG), "tile size");
inline unsigned grid_for(size_t n) { return (unsigned)((n + PL_THREADS - 1) / PL_THREADS); }

// bytes 0..3 of the result picked from the eight bytes hi:lo by the selector's bytes (0..3: of lo, 4..7: of hi) -- v_perm_b32
DEV u32 pl_perm(u32 hi, u32 lo, u32 sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
// w: 16 elements of E bytes (4 E dwords) -> o[p]: byte p of each of them (4 dwords).  One round takes the even and the odd bytes of a dword pair
// apart; the even half then holds planes 0, 2, .. interleaved E / 2 wide, the odd half planes 1, 3, ..
template <int E> DEV void pl_deinterleave(const u32* w, u32 (*o)[4], int p0 = 0, int step = 1)
{
    if constexpr (E == 1) { for (int k = 0; k < 4; ++k) o[p0][k] = w[k]; }
    else {
        u32 ev[2 * E], od[2 * E];
#pragma unroll
        for (int j = 0; j < 2 * E; ++j) { ev[j] = pl_perm(w[2 * j + 1], w[2 * j], 0x06040200u); od[j] = pl_perm(w[2 * j + 1], w[2 * j], 0x07050301u); }
        pl_deinterleave<E / 2>(ev, o, p0, 2 * step);
        pl_deinterleave<E / 2>(od, o, p0 + step, 2 * step);
    }
}
// ... and back: the planes' dwords zipped bytewise, round by round
template <int E> DEV void pl_interleave(u32* w, const u32 (*o)[4], int p0 = 0, int step = 1)
{
    if constexpr (E == 1) { for (int k = 0; k < 4; ++k) w[k] = o[p0][k]; }
    else {
        u32 ev[2 * E], od[2 * E];
        pl_interleave<E / 2>(ev, o, p0, 2 * step);
        pl_interleave<E / 2>(od, o, p0 + step, 2 * step);
#pragma unroll
        for (int j = 0; j < 2 * E; ++j) { w[2 * j] = pl_perm(od[j], ev[j], 0x05010400u); w[2 * j + 1] = pl_perm(od[j], ev[j], 0x07030602u); }
    }
}

// size of plane p of a tensor of n bytes, and where it starts inside the tensor (the sizes of the planes in front of it)
HDEV u64 pl_size(u64 n, u32 p, u32 E) { return n > p ? (n - p + E - 1) / E : 0; }
HDEV u64 pl_start(u64 n, u32 p, u32 E) { const u64 r = n % E; return (u64)p * (n / E) + (p < r ? p : r); }

// ---- the delta ops (fsehip.h, "arithmetic tensor deltas") ----
// what the data kernels do with the base: nothing (it is never read), XOR, or SUB -- zigzag(tensor - base) on the elements' bit patterns
enum { PL_NONE = 0, PL_XOR = 1, PL_SUB = 2 };
// the template argument for a nullable base and a deltaOp of the C calls (bad_op has let it through)
inline int pl_op(const void* base, unsigned deltaOp) { return !base ? PL_NONE : deltaOp == FSEHIP_DELTA_SUB ? PL_SUB : PL_XOR; }
inline bool bad_op(unsigned deltaOp) { return deltaOp > FSEHIP_DELTA_SUB; }

// One element of E bytes as a number below 2^(8 E): z = zigzag((t - b) mod 2^W), and t from z and b.  The bytewise head and tail of the
// SUB kernels, and what the dword forms below must agree with bit for bit
template <int E> DEV u64 pl_zz(u64 t, u64 b)
{
    constexpr u64 M = E == 8 ? ~(u64)0 : (((u64)1 << (8 * (E & 7))) - 1);
    const u64 d = (t - b) & M;
    return ((d << 1) & M) ^ (((d >> (8 * E - 1)) & 1) ? M : 0);
}
template <int E> DEV u64 pl_unzz(u64 z, u64 b)
{
    constexpr u64 M = E == 8 ? ~(u64)0 : (((u64)1 << (8 * (E & 7))) - 1);
    const u64 d = (z >> 1) ^ ((z & 1) ? M : 0);
    return (b + d) & M;
}
// The same on the dwords of a chunk, which hold whole elements: w[0 .. 4) = zigzag(w - b), or (INV) w = b + unzigzag(w).
//   E == 1: four bytes per dword, SWAR -- the top bit of every byte is taken out of the subtraction (addition) and put back by XOR, so no
//           borrow (carry) crosses a byte; the sign byte masks are (bit * 0xFF)
//   E == 2: two elements per dword, the packed 16-bit forms (v_pk_sub_u16 / v_pk_add_u16, v_pk_lshlrev_b16, v_pk_ashrrev_i16)
//   E == 4: plain 32-bit
//   E == 8: the dword pair w[2 k], w[2 k + 1] as one 64-bit number (v_sub_co / v_subb, the shift over 64 bits)
typedef unsigned short pl_u16x2 __attribute__((ext_vector_type(2)));
typedef short pl_i16x2 __attribute__((ext_vector_type(2)));
template <int E, bool INV> DEV void pl_sub4(u32* w, const u32* b)
{
    constexpr u32 H = 0x80808080u, L = 0x7F7F7F7Fu, ONE = 0x01010101u;
    if constexpr (E == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (!INV) {
                const u32 d = ((w[k] | H) - (b[k] & L)) ^ ((w[k] ^ ~b[k]) & H);
                w[k] = ((d & L) << 1) ^ (((d >> 7) & ONE) * 0xFFu);
            } else {
                const u32 d = ((w[k] >> 1) & L) ^ ((w[k] & ONE) * 0xFFu);
                w[k] = ((b[k] & L) + (d & L)) ^ ((b[k] ^ d) & H);
            }
        }
    } else if constexpr (E == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pl_u16x2 x, y;
            __builtin_memcpy(&x, &w[k], 4); __builtin_memcpy(&y, &b[k], 4);
            if constexpr (!INV) {
                const pl_u16x2 d = x - y;
                x = (d << 1) ^ (pl_u16x2)((pl_i16x2)d >> 15);
            } else {
                const pl_u16x2 d = (x >> 1) ^ (pl_u16x2)(-(pl_i16x2)(x & (unsigned short)1));
                x = y + d;
            }
            __builtin_memcpy(&w[k], &x, 4);
        }
    } else if constexpr (E == 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (!INV) { const u32 d = w[k] - b[k]; w[k] = (d << 1) ^ (u32)((int)d >> 31); }
            else { const u32 d = (w[k] >> 1) ^ (0u - (w[k] & 1u)); w[k] = b[k] + d; }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const u64 x = (u64)w[2 * k] | ((u64)w[2 * k + 1] << 32), y = (u64)b[2 * k] | ((u64)b[2 * k + 1] << 32);
            const u64 r = INV ? pl_unzz<8>(x, y) : pl_zz<8>(x, y);
            w[2 * k] = (u32)r; w[2 * k + 1] = (u32)(r >> 32);
        }
    }
}
// w = op(w, the 16 bytes at `from`): the base stream of the delta forms, any alignment, combined into its words as it arrives
template <int E, int OP, bool INV> DEV void pl_base16(u32* w, const u8* from)
{
    u32 t[4];
    __builtin_memcpy(t, from, 16);
    if constexpr (OP == PL_XOR) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] ^= t[k];
    } else pl_sub4<E, INV>(w, t);
}
// element e of the tensor at sb (n bytes, base bb) as the SUB kernels' head and tail take it, a thread per element: its bytes into the
// planes at pb, or back from them into db.  The partial last element of a tensor whose size is no multiple of E goes byte by byte, E == 1 form
template <int E> DEV void pl_sub_elem_split(u8* pb, const u8* sb, const u8* bb, u64 n, u64 e)
{
    const u64 k0 = e * E;
    if (k0 + E <= n) {
        u64 t = 0, b = 0;
#pragma unroll
        for (int p = 0; p < E; ++p) { t |= (u64)sb[k0 + p] << (8 * p); b |= (u64)bb[k0 + p] << (8 * p); }
        const u64 z = pl_zz<E>(t, b);
#pragma unroll
        for (int p = 0; p < E; ++p) pb[pl_start(n, p, E) + e] = (u8)(z >> (8 * p));
    } else {
        for (u64 k = k0; k < n; ++k) pb[pl_start(n, (u32)(k - k0), E) + e] = (u8)pl_zz<1>(sb[k], bb[k]);
    }
}
template <int E, class PlaneAt> DEV void pl_sub_elem_merge(u8* db, const u8* bb, u64 n, u64 e, PlaneAt planeAt)
{
    const u64 k0 = e * E;
    if (k0 + E <= n) {
        u64 z = 0, b = 0;
#pragma unroll
        for (int p = 0; p < E; ++p) { z |= (u64)planeAt(p)[e] << (8 * p); b |= (u64)bb[k0 + p] << (8 * p); }      // (in place: these loads, then the stores)
        const u64 t = pl_unzz<E>(z, b);
#pragma unroll
        for (int p = 0; p < E; ++p) db[k0 + p] = (u8)(t >> (8 * p));
    } else {
        for (u64 k = k0; k < n; ++k) db[k] = (u8)pl_unzz<1>(planeAt((u32)(k - k0))[e], bb[k]);
    }
}

// ---- predicted planes (planes_pred.hip; fsehip.h, "predicted planes") ----
// z[j] = zigzag(t[j] - t[j - 1]) inside runs of PP_RUN elements whose first element is predicted by 0; the inverse sums a run back.  The
// dword forms work, as pl_sub4 does, on a lane's chunk of 16 whole elements (4 E dwords), and no carry crosses an element
#define PP_RUN ((u64)1 << FSEHIP_PRED_RUN_LOG)
static_assert(PP_RUN == 16 * WAVE && PLANES_TILE % (8 * PP_RUN) == 0, "a run is one round of one wave, and a tile holds whole runs of every element size");
// pv = the chunk w moved up by one element: every element's predecessor.  The first one's is the E bytes in front of `at` (where the
// chunk lies in the source), or 0 where the chunk starts a run -- nothing in front of it is read then
template <int E> DEV void pp_prev(u32* pv, const u32* w, const u8* at, bool runStart)
{
    u32 f[2] = { 0, 0 };
    if (!runStart) __builtin_memcpy(f, at - E, E);
    if constexpr (E >= 4) {
        constexpr int FD = E / 4;
#pragma unroll
        for (int j = 0; j < 4 * E; ++j) pv[j] = j < FD ? f[j] : w[j - FD];
    } else {
        pv[0] = __builtin_amdgcn_alignbyte(w[0], f[0] << (32 - 8 * E), 4 - E);
#pragma unroll
        for (int j = 1; j < 4 * E; ++j) pv[j] = __builtin_amdgcn_alignbyte(w[j], w[j - 1], 4 - E);
    }
}
// x + y on the two 16-bit halves (v_pk_add_u16), and on the four bytes (the top bits kept out of the addition, as in pl_sub4)
DEV u32 pp_add16x2(u32 x, u32 y)
{
    pl_u16x2 a, b;
    __builtin_memcpy(&a, &x, 4); __builtin_memcpy(&b, &y, 4);
    a += b;
    __builtin_memcpy(&x, &a, 4);
    return x;
}
DEV u32 pp_add8x4(u32 x, u32 y) { return ((x & 0x7F7F7F7Fu) + (y & 0x7F7F7F7Fu)) ^ ((x ^ y) & 0x80808080u); }
// the chunk's differences d -> their inclusive prefix sums mod 2^(8 E), in place; returns the last one, the chunk's total
//   E == 1: the even and the odd bytes of a dword as two 16-bit fields each -- four bytes and a carry stay below 2^16 -- summed there
//   E == 2: the upper half takes the lower one by a shift; the running total is added to both halves at once
template <int E> DEV u64 pp_prefix(u32* w)
{
    if constexpr (E == 1) {
        u32 c = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32 ev = w[k] & 0x00FF00FFu, od = (w[k] >> 8) & 0x00FF00FFu;
            const u32 evp = ev + (ev << 16), odp = od + (od << 16);
            const u32 e2 = evp + (odp << 16) + c * 0x00010001u, o2 = evp + odp + c * 0x00010001u;
            w[k] = (e2 & 0x00FF00FFu) | ((o2 & 0x00FF00FFu) << 8);
            c = w[k] >> 24;
        }
        return c;
    } else if constexpr (E == 2) {
        u32 c = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            w[k] = pp_add16x2(w[k] + (w[k] << 16), c * 0x00010001u);
            c = w[k] >> 16;
        }
        return c;
    } else if constexpr (E == 4) {
#pragma unroll
        for (int k = 1; k < 16; ++k) w[k] += w[k - 1];
        return w[15];
    } else {
        u64 acc = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            acc += (u64)w[2 * k] | ((u64)w[2 * k + 1] << 32);
            w[2 * k] = (u32)acc; w[2 * k + 1] = (u32)(acc >> 32);
        }
        return acc;
    }
}
// every element of the chunk plus c, mod 2^(8 E): the lane's carry-in
template <int E> DEV void pp_carry(u32* w, u64 c)
{
#pragma unroll
    for (int k = 0; k < 4 * E; ++k) {
        if constexpr (E == 1) w[k] = pp_add8x4(w[k], ((u32)c & 0xFFu) * 0x01010101u);
        else if constexpr (E == 2) w[k] = pp_add16x2(w[k], ((u32)c & 0xFFFFu) * 0x00010001u);
        else if constexpr (E == 4) w[k] += (u32)c;
        else if ((k & 1) == 0) {
            const u64 x = ((u64)w[k] | ((u64)w[k + 1] << 32)) + c;
            w[k] = (u32)x; w[k + 1] = (u32)(x >> 32);
        }
    }
}
// element e of the tensor at sb (n bytes) a thread per element, the split's head and tail: its difference into the planes at pb.  The
// partial last element of a tensor passes unchanged
template <int E> DEV void pp_elem_split(u8* pb, const u8* sb, u64 n, u64 e)
{
    const u64 k0 = e * E;
    if (k0 + E <= n) {
        u64 t = 0, b = 0;
#pragma unroll
        for (int p = 0; p < E; ++p) t |= (u64)sb[k0 + p] << (8 * p);
        if (e & (PP_RUN - 1)) {
#pragma unroll
            for (int p = 0; p < E; ++p) b |= (u64)sb[k0 - E + p] << (8 * p);
        }
        const u64 z = pl_zz<E>(t, b);
#pragma unroll
        for (int p = 0; p < E; ++p) pb[pl_start(n, p, E) + e] = (u8)(z >> (8 * p));
    } else {
        for (u64 k = k0; k < n; ++k) pb[pl_start(n, (u32)(k - k0), E) + e] = sb[k];
    }
}

// the largest j < n with key(j) <= q, for n >= 1 and a key that does not decrease; 0 where there is none.  The result is an index below n
// whatever the keys hold: a caller that reads its keys from an array it does not trust indexes with the result, never with a key
template <class Key> DEV size_t pl_last_le(size_t n, u64 q, Key key)
{
    size_t lo = 0, hi = n - 1;
    while (lo < hi) { const size_t mid = lo + ((hi - lo + 1) >> 1); if (key(mid) <= q) lo = mid; else hi = mid - 1; }
    return lo;
}
// the work mapping: the largest i < nT with floor(S[i] / T) + i <= w (false: there is none)
DEV bool pl_find(const u64* S, size_t nT, u64 w, size_t& i)
{
    if (nT == 0 || (S[0] >> PL_TILE_LOG) > w) return false;
    i = pl_last_le(nT, w, [S](size_t j) { return (S[j] >> PL_TILE_LOG) + j; });
    return true;
}
// A workgroup's share of a tensor of n bytes at flat position s0, tile [lo, lo + T): the elements [e0, e1) whose first byte lies in the tile
// and inside the tensor, cut into a bytewise head [e0, eb), `nch` chunks of 16 WHOLE elements from eb on, and a bytewise tail [et, e1).
// `first` = the address that the chunks are aligned by, as a number: element e0 lies `first` bytes behind a 16-byte boundary of it
struct PlShare { u64 e0, eb, et, e1, nch; };
template <int E> DEV PlShare pl_share(u64 s0, u64 n, u64 lo, u64 alignAddr, u32 alignStride)
{
    PlShare r;
    const u64 hi = lo + PLANES_TILE;
    const u64 a = lo > s0 ? lo - s0 : 0, b = (hi < s0 + n ? hi : s0 + n) - s0;
    r.e0 = (a + E - 1) / E; r.e1 = (b + E - 1) / E;
    // elements up to the 16-byte boundary of alignAddr + e * alignStride (alignStride 1: plane 0 of the split; E: the merge's tensor, where its start allows it)
    u64 head = alignStride ? ((0 - (alignAddr + r.e0 * alignStride)) & 15u) / alignStride : 0;
    if (head > r.e1 - r.e0) head = r.e1 - r.e0;
    r.eb = r.e0 + head;
    const u64 whole = n / E < r.e1 ? n / E : r.e1;                  // (the last element of the tensor may be partial)
    r.nch = whole > r.eb ? (whole - r.eb) >> 4 : 0;
    r.et = r.eb + 16 * r.nch;
    return r;
}

// the result of tensor i of the merge (fsehip.h: the five rules in their order)
DEV size_t pm_verdict(const u64* D, const size_t* PS, size_t i, u32 E, u64 dstCapacity)
{
    const u64 d0 = D[i], d1 = D[i + 1];
    if (d1 > dstCapacity) return FERR(GENERIC);
    u64 n = 0;
    for (u32 p = 0; p < E; ++p) { const size_t z = PS[i * E + p]; if (is_err(z)) return z; n += z; }
    for (u32 p = 0; p < E; ++p) if ((u64)PS[i * E + p] != pl_size(n, p, E)) return FERR(corruption_detected);
    if (n > (d1 > d0 ? d1 - d0 : 0)) return FERR(dstSize_tooSmall);
    return (size_t)n;
}

// ---- strided predicted planes (planes_stride.hip, planes_each_stride.hip; fsehip.h, "strided predicted planes") ----
// pv = the chunk w moved up by S elements: every element's predecessor.  Those of the first S are the S E bytes in front of `at` (where
// the chunk lies in the source), or 0 where the chunk starts a run -- nothing in front of it is read then.  The bytes in front are loaded
// as whole dwords, up to 3 bytes more than needed: a chunk that starts no run lies at least 16 elements inside its tensor, S E + 3 <= 16 E
template <int E, int S> DEV void ps_prev(u32* pv, const u32* w, const u8* at, bool runStart)
{
    constexpr int FD = (S * E + 3) / 4, OFF = 4 * FD - S * E;
    u32 x[FD + 4 * E];
#pragma unroll
    for (int j = 0; j < FD; ++j) x[j] = 0;
    if (!runStart) __builtin_memcpy(x, at - 4 * FD, 4 * FD);
#pragma unroll
    for (int j = 0; j < 4 * E; ++j) x[FD + j] = w[j];
#pragma unroll
    for (int j = 0; j < 4 * E; ++j) {
        if constexpr (OFF != 0) pv[j] = __builtin_amdgcn_alignbyte(x[j + 1], x[j], OFF);
        else pv[j] = x[j];
    }
}
// element e of the tensor at sb (n bytes) a thread per element, the split's head and tail (pp_elem_split with the predecessor S back)
template <int E, int S> DEV void ps_elem_split(u8* pb, const u8* sb, u64 n, u64 e)
{
    const u64 k0 = e * E;
    if (k0 + E <= n) {
        u64 t = 0, b = 0;
#pragma unroll
        for (int p = 0; p < E; ++p) t |= (u64)sb[k0 + p] << (8 * p);
        if ((e & (PP_RUN - 1)) >= (u64)S) {
#pragma unroll
            for (int p = 0; p < E; ++p) b |= (u64)sb[k0 - S * E + p] << (8 * p);
        }
        const u64 z = pl_zz<E>(t, b);
#pragma unroll
        for (int p = 0; p < E; ++p) pb[pl_start(n, p, E) + e] = (u8)(z >> (8 * p));
    } else {
        for (u64 k = k0; k < n; ++k) pb[pl_start(n, (u32)(k - k0), E) + e] = sb[k];
    }
}

// the merge's arithmetic: an element per register, sums mod 2^32 (2^64 for E == 8).  For E < 4 the bits above the element are not kept
// clean -- they never reach a bit below them -- and ps_pack drops them
template <int E> using ps_t = std::conditional_t<E == 8, u64, u32>;
template <int E> DEV void ps_unpack(ps_t<E>* x, const u32* w)
{
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if constexpr (E == 1) x[q] = w[q / 4] >> (8 * (q % 4));
        else if constexpr (E == 2) x[q] = w[q / 2] >> (16 * (q % 2));
        else if constexpr (E == 4) x[q] = w[q];
        else x[q] = (u64)w[2 * q] | ((u64)w[2 * q + 1] << 32);
    }
}
template <int E> DEV void ps_pack(u32* w, const ps_t<E>* x)
{
#pragma unroll
    for (int k = 0; k < 4 * E; ++k) {
        if constexpr (E == 1) w[k] = (x[4 * k] & 0xFFu) | ((x[4 * k + 1] & 0xFFu) << 8) | ((x[4 * k + 2] & 0xFFu) << 16) | (x[4 * k + 3] << 24);
        else if constexpr (E == 2) w[k] = (x[2 * k] & 0xFFFFu) | (x[2 * k + 1] << 16);
        else if constexpr (E == 4) w[k] = x[k];
        else w[k] = (u32)(x[k / 2] >> (32 * (k % 2)));
    }
}
// v[k] = v[(k + r) mod S] for a lane-dependent r < S: one round of selects per bit of r, static register indices throughout
template <int S, class T> DEV void ps_rotate(T* v, u32 r)
{
#pragma unroll
    for (int b = 1; b < S; b <<= 1) {
        T t[S];
#pragma unroll
        for (int k = 0; k < S; ++k) t[k] = (r & (u32)b) ? v[(k + b) % S] : v[k];
#pragma unroll
        for (int k = 0; k < S; ++k) v[k] = t[k];
    }
}
// A workgroup's share of the split of the tensor at sb (n bytes at flat position s0, planes at pb) at stride S: the body of
// k_planes_split_pred_stride and of the strided PRED arms of k_planes_split_each_stride
template <int E, int S> DEV void ps_split(u8* pb, const u8* sb, u64 s0, u64 n, u64 lo, u32 tid)
{
    const PlShare h = pl_share<E>(s0, n, lo, 0, 1);               // chunks at multiples of 16 elements of the tensor
    for (u64 c = tid; c < h.nch; c += PL_THREADS) {
        const u64 e = h.eb + 16 * c;
        u32 wv[4 * E], pv[4 * E], o[E][4];
#pragma unroll
        for (int k = 0; k < E; ++k) __builtin_memcpy(&wv[4 * k], sb + e * E + 16 * k, 16);
        ps_prev<E, S>(pv, wv, sb + e * E, (e & (PP_RUN - 1)) == 0);
#pragma unroll
        for (int k = 0; k < E; ++k) pl_sub4<E, false>(&wv[4 * k], &pv[4 * k]);
        pl_deinterleave<E>(wv, o);
#pragma unroll
        for (int p = 0; p < E; ++p) __builtin_memcpy(pb + pl_start(n, p, E) + e, o[p], 16);
    }
    const u64 nHead = h.eb - h.e0, nTail = h.e1 - h.et;
    for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) ps_elem_split<E, S>(pb, sb, n, j < nHead ? h.e0 + j : h.et + (j - nHead));
}
// The runs of tile t of the merge of the tensor at db (n bytes, plane p at planes + P[p]) at stride S: the body of
// k_planes_merge_pred_stride and of the strided PRED arms of k_planes_merge_each_stride.  All 64 lanes of a wave take every scan.  WIN (the
// window form, as in pe_merge): db, n and t are those of the virtual tensor, whose planes start L bytes in front of P[p] and whose first L
// elements are summed into their chains but not stored (n is a multiple of E there).  The virtual tensor starts on a run, so r0 and rEnd,
// which depend on the lane only, are the tensor's own
template <int E, int S, bool WIN = false> DEV void ps_merge(u8* db, const u8* planes, const u64* P, u64 n, u64 t, u64 L = 0)
{
    typedef ps_t<E> T;
    constexpr u32 RUNS = (u32)(PLANES_TILE / E / PP_RUN);         // whole runs of a tile
    constexpr bool ROT = 16 % S != 0;                             // the chain of a register depends on the lane
    const u64 m = n / E;
    const u32 lane = threadIdx.x % WAVE;
    const u32 r0 = ROT ? (16 * lane) % S : 0;                     // register q of this lane lies in chain (r0 + q) mod S
    const u32 rEnd = ROT ? (S - (r0 + 16) % S) % S : 0;           // chain a's last element is register 16 - S + (a + rEnd) mod S
    const u8* pp[E];
#pragma unroll
    for (int p = 0; p < E; ++p) pp[p] = planes + P[p];
    if constexpr (WIN) {
#pragma unroll
        for (int p = 0; p < E; ++p) pp[p] -= L;
    }
    for (u32 r = threadIdx.x / WAVE; r < RUNS; r += PL_THREADS / WAVE) {
        const u64 e0 = t * (PLANES_TILE / E) + r * PP_RUN, e = e0 + 16 * lane;
        if (e0 * E >= n) break;                                   // (uniform over the wave: the run lies behind the tensor)
        const bool full = e + 16 <= m;
        T x[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) x[q] = 0;
        if (full) {
            u32 wv[4 * E], o[E][4];
            const u32 zero[4] = { 0, 0, 0, 0 };
#pragma unroll
            for (int p = 0; p < E; ++p) __builtin_memcpy(o[p], pp[p] + e, 16);
            pl_interleave<E>(wv, o);
#pragma unroll
            for (int k = 0; k < E; ++k) pl_sub4<E, true>(&wv[4 * k], zero);
            ps_unpack<E>(x, wv);
#pragma unroll
            for (int q = S; q < 16; ++q) x[q] += x[q - S];
        }
        T c[S];                                                   // chain by chain, what the lanes in front of this one add up to: all 64 lanes scan
#pragma unroll
        for (int k = 0; k < S; ++k) c[k] = x[16 - S + k];
        if constexpr (ROT) ps_rotate<S>(c, rEnd);
#pragma unroll
        for (int k = 0; k < S; ++k) {
            if constexpr (E == 8) c[k] = group_scan_incl_add64<64>(c[k], lane) - c[k];
            else c[k] = group_scan_incl<64, ScanAdd>(c[k], lane) - c[k];
        }
        if constexpr (ROT) ps_rotate<S>(c, r0);                   // c[k]: the carry-in of the registers q with q mod S == k
        if (full) {
            u32 wv[4 * E];
#pragma unroll
            for (int q = 0; q < 16; ++q) x[q] += c[q % S];
            ps_pack<E>(wv, x);
            bool whole = true;
            if constexpr (WIN) whole = e >= L;
            if (whole) {
#pragma unroll
                for (int k = 0; k < E; ++k) __builtin_memcpy(db + e * E + 16 * k, &wv[4 * k], 16);
            } else {
                if constexpr (WIN) {                              // the chunk that straddles the lead: its elements from L on, one by one
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if (e + j >= L) __builtin_memcpy(db + (e + j) * E, (const u8*)wv + j * E, E);
                }
            }
        } else if (e * E < n) {                                   // the tensor's last chunk: fewer than 16 whole elements, then n mod E bytes
            u64 acc[S];
#pragma unroll
            for (int k = 0; k < S; ++k) acc[k] = c[k];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const u64 j = e + q;
                if (j < m) {
                    u64 z = 0;
#pragma unroll
                    for (int p = 0; p < E; ++p) z |= (u64)pp[p][j] << (8 * p);
                    acc[q % S] = pl_unzz<E>(z, acc[q % S]);
                    if (!WIN || j >= L) {                         // (the lead: summed, not stored)
#pragma unroll
                        for (int p = 0; p < E; ++p) db[j * E + p] = (u8)(acc[q % S] >> (8 * p));
                    }
                }
            }
            if constexpr (!WIN)
                for (u64 k = m * E; k < n; ++k) db[k] = planes[P[k - m * E] + m];
        }
    }
}
// the dispatch over a stride above 1: f(std::integral_constant<int, S>) for 2 <= S <= FSEHIP_PRED_MAX_STRIDE (bad_stride has let it through; on
// the device: the stride byte of an accepted tensor).  A switch, so that every body has its S as a constant and static register indices
template <class F> HDEV void ps_for_stride(unsigned S, F f)
{
    switch (S) {
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 6: f(std::integral_constant<int, 6>()); break;
    case 7: f(std::integral_constant<int, 7>()); break;
    default: f(std::integral_constant<int, 8>()); break;
    }
}
static_assert(FSEHIP_PRED_MAX_STRIDE == 8, "the strides the kernels are instantiated for");
HDEV bool bad_stride(unsigned stride) { return stride == 0 || stride > FSEHIP_PRED_MAX_STRIDE; }

// ---- a transform per tensor (planes_each.hip, planes_each_stride.hip; fsehip.h, "a transform per tensor") ----
DEV bool pe_ok(u32 tr, const void* base) { return tr <= FSEHIP_EST_SUB && (tr < FSEHIP_EST_XOR || base); }
// the stride of tensor i under transform tr (1 for every transform that has none: its stride byte is not read), and whether the pair is accepted
DEV u32 pes_stride(u32 tr, const u8* ST, size_t i) { return tr == FSEHIP_EST_PRED ? ST[i] : 1u; }
DEV bool pes_ok(u32 tr, u32 st, const void* base) { return pe_ok(tr, base) && !bad_stride(st); }
// The window rules of tensor i, whose transform is tr and whose verdict is n bytes, and its lead L in elements (at every stride: a run is
// PP_RUN elements counted from the tensor's start).  An empty window has none
DEV bool pe_win_ok(const u64* W, const u64* PO, size_t i, u32 E, u32 tr, u64 n, u64& L)
{
    const u64 a = W[2 * i], b = W[2 * i + 1];
    L = tr == FSEHIP_EST_PRED && n ? a & (PP_RUN - 1) : 0;
    if (a > b || n % E || b - a != n / E) return false;
    for (u32 p = 0; p < E; ++p) if (L > PO[i * E + p]) return false;
    return true;
}
// a workgroup's share of the tensor at sb (n bytes at flat position s0, base bb, planes at pb) under transform TR
template <int E, int TR> DEV void pe_split(u8* pb, const u8* sb, const u8* bb, u64 s0, u64 n, u64 lo, u32 tid)
{
    const PlShare h = pl_share<E>(s0, n, lo, 0, 1);               // chunks at multiples of 16 elements of the tensor
    for (u64 c = tid; c < h.nch; c += PL_THREADS) {
        const u64 e = h.eb + 16 * c;
        u32 wv[4 * E], o[E][4];
#pragma unroll
        for (int k = 0; k < E; ++k) __builtin_memcpy(&wv[4 * k], sb + e * E + 16 * k, 16);
        if constexpr (TR == FSEHIP_EST_PRED) {
            u32 pv[4 * E];
            pp_prev<E>(pv, wv, sb + e * E, (e & (PP_RUN - 1)) == 0);
#pragma unroll
            for (int k = 0; k < E; ++k) pl_sub4<E, false>(&wv[4 * k], &pv[4 * k]);
        } else if constexpr (TR != FSEHIP_EST_PLAIN) {
#pragma unroll
            for (int k = 0; k < E; ++k) pl_base16<E, TR == FSEHIP_EST_SUB ? PL_SUB : PL_XOR, false>(&wv[4 * k], bb + e * E + 16 * k);
        }
        pl_deinterleave<E>(wv, o);
#pragma unroll
        for (int p = 0; p < E; ++p) __builtin_memcpy(pb + pl_start(n, p, E) + e, o[p], 16);
    }
    // head and tail, an element per thread; the partial last element of the tensor byte by byte
    const u64 nHead = h.eb - h.e0, nTail = h.e1 - h.et;
    for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) {
        const u64 e = j < nHead ? h.e0 + j : h.et + (j - nHead);
        if constexpr (TR == FSEHIP_EST_PRED) pp_elem_split<E>(pb, sb, n, e);
        else if constexpr (TR == FSEHIP_EST_SUB) pl_sub_elem_split<E>(pb, sb, bb, n, e);
        else {
#pragma unroll
            for (int p = 0; p < E; ++p) {
                const u64 k = e * E + p;
                if (k < n) {
                    u8 v = sb[k];
                    if constexpr (TR == FSEHIP_EST_XOR) v ^= bb[k];
                    pb[pl_start(n, p, E) + e] = v;
                }
            }
        }
    }
}
// the runs of tile t of the tensor at db (n bytes, base bb, plane p at planes + P[p]) under transform TR.  WIN: db, n and t are those of the
// virtual tensor, whose planes start L bytes in front of P[p] and whose first L elements are not stored (n is a multiple of E there)
template <int E, int TR, bool WIN = false> DEV void pe_merge(u8* db, const u8* bb, const u8* planes, const u64* P, u64 n, u64 t, u64 L = 0)
{
    constexpr u32 RUNS = (u32)(PLANES_TILE / E / PP_RUN);         // whole runs of a tile
    const u64 m = n / E;
    const u32 lane = threadIdx.x % WAVE;
    const u8* pp[E];
#pragma unroll
    for (int p = 0; p < E; ++p) pp[p] = planes + P[p];
    if constexpr (WIN) {
#pragma unroll
        for (int p = 0; p < E; ++p) pp[p] -= L;
    }
    for (u32 r = threadIdx.x / WAVE; r < RUNS; r += PL_THREADS / WAVE) {
        const u64 e0 = t * (PLANES_TILE / E) + r * PP_RUN, e = e0 + 16 * lane;
        if (e0 * E >= n) break;                                   // (uniform over the wave: the run lies behind the tensor)
        const bool full = e + 16 <= m;
        u32 wv[4 * E];
        if constexpr (TR == FSEHIP_EST_PRED) {
            u64 total = 0;
            if (full) {
                u32 o[E][4];
                const u32 zero[4] = { 0, 0, 0, 0 };
#pragma unroll
                for (int p = 0; p < E; ++p) __builtin_memcpy(o[p], pp[p] + e, 16);
                pl_interleave<E>(wv, o);
#pragma unroll
                for (int k = 0; k < E; ++k) pl_sub4<E, true>(&wv[4 * k], zero);
                total = pp_prefix<E>(wv);
            }
            u64 carry;                                            // what the lanes in front of this one add up to: all 64 lanes scan
            if constexpr (E == 8) carry = group_scan_incl_add64<64>(total, lane) - total;
            else carry = group_scan_incl<64, ScanAdd>((u32)total, lane) - (u32)total;
            if (full) {
                pp_carry<E>(wv, carry);
                bool whole = true;
                if constexpr (WIN) whole = e >= L;
                if (whole) {
#pragma unroll
                    for (int k = 0; k < E; ++k) __builtin_memcpy(db + e * E + 16 * k, &wv[4 * k], 16);
                } else {
                    if constexpr (WIN) {                          // the chunk that straddles the lead: its elements from L on, one by one
#pragma unroll
                        for (int j = 0; j < 16; ++j)
                            if (e + j >= L) __builtin_memcpy(db + (e + j) * E, (const u8*)wv + j * E, E);
                    }
                }
            } else if (e * E < n) {                               // the tensor's last chunk: fewer than 16 whole elements, then n mod E bytes
                u64 acc = carry;
                for (u64 j = e; j < m; ++j) {
                    u64 z = 0;
#pragma unroll
                    for (int p = 0; p < E; ++p) z |= (u64)pp[p][j] << (8 * p);
                    acc = pl_unzz<E>(z, acc);
                    if (WIN && j < L) continue;                   // (the lead: summed, not stored)
#pragma unroll
                    for (int p = 0; p < E; ++p) db[j * E + p] = (u8)(acc >> (8 * p));
                }
                if constexpr (!WIN)
                    for (u64 k = m * E; k < n; ++k) db[k] = planes[P[k - m * E] + m];
            }
        } else if (full) {
            u32 o[E][4];
#pragma unroll
            for (int p = 0; p < E; ++p) __builtin_memcpy(o[p], pp[p] + e, 16);
            pl_interleave<E>(wv, o);
            if constexpr (TR != FSEHIP_EST_PLAIN) {
#pragma unroll
                for (int k = 0; k < E; ++k)                       // (in place: these loads, then the stores below)
                    pl_base16<E, TR == FSEHIP_EST_SUB ? PL_SUB : PL_XOR, true>(&wv[4 * k], bb + e * E + 16 * k);
            }
#pragma unroll
            for (int k = 0; k < E; ++k) __builtin_memcpy(db + e * E + 16 * k, &wv[4 * k], 16);
        } else if (e * E < n) {                                   // the tensor's last chunk, an element at a time (in place: its loads, then its stores)
            if constexpr (TR == FSEHIP_EST_SUB) {
                for (u64 j = e; j * E < n; ++j) pl_sub_elem_merge<E>(db, bb, n, j, [&](u32 p) { return planes + P[p]; });
            } else {
                for (u64 j = e; j * E < n; ++j) {
                    for (u64 k = j * E; k < n && k < (j + 1) * E; ++k) {
                        u8 v = planes[P[k - j * E] + j];
                        if constexpr (TR == FSEHIP_EST_XOR) v ^= bb[k];
                        db[k] = v;
                    }
                }
            }
        }
    }
}

// ---- segmented planes (planes_seg.hip; fsehip.h, "segmented planes") ----
// segments of a plane of `size` bytes at seg = 1 << segLog: every plane has at least one
__host__ __device__ inline u64 ps_count(u64 size, u32 segLog) { const u64 c = (size + (((u64)1 << segLog) - 1)) >> segLog; return c ? c : 1; }
// tensor i is accepted iff each of its E planes has in segFirst the count its size in S implies
DEV bool ps_tensor_ok(const u64* S, const u64* SF, size_t i, u32 E, u32 segLog)
{
    const u64 s0 = S[i], s1 = S[i + 1], n = s1 > s0 ? s1 - s0 : 0;
    bool ok = true;
    for (u32 p = 0; p < E; ++p) ok = ok && SF[i * E + p + 1] - SF[i * E + p] == ps_count(pl_size(n, p, E), segLog);
    return ok;
}
// What the two folds (k_planes_fold, k_planes_fold_window) share: one wave over the results res[0 .. cnt) of a plane's segments, which were
// written at off[0 .. cnt).  firstErr = the smallest index that holds an error (none: 0xFFFFFFFF); bad = a good segment whose size the
// caller's rule sizeOk(k, r) refuses, or that does not end where the next one starts; sum = the bytes of the good ones.  Every check is per
// segment, the reductions stand behind the loop, where all lanes are active again: all lanes return the same
struct PsFold { u32 firstErr, bad; u64 sum; };
template <class Rule> DEV PsFold ps_fold(const u64* off, const size_t* res, u64 cnt, u32 lane, Rule sizeOk)
{
    PsFold f = { 0xFFFFFFFFu, 0, 0 };
    for (u64 k = lane; k < cnt; k += WAVE) {
        const size_t r = res[k];
        if (is_err(r)) { if ((u32)k < f.firstErr) f.firstErr = (u32)k; continue; }
        if (!sizeOk(k, (u64)r)) f.bad = 1;
        if (k + 1 < cnt && off[k + 1] != off[k] + r) f.bad = 1;                        // ... and they lie back to back
        f.sum += r;
    }
    f.firstErr = group_reduce<64, ScanMin>(f.firstErr, lane);
    f.bad = group_reduce<64, ScanMax>(f.bad, lane);
    f.sum = group_last64<64>(group_scan_incl_add64<64>(f.sum, lane), lane);
    return f;
}

// ---- windows of segmented tensors (planes_win.hip; fsehip.h, "windows of segmented tensors") ----
// the window [a, b) of tensor i in elements, the segments k0 .. k0 + cnt - 1 of each of its planes that hold it (cnt 0: an empty window), and
// whether the tensor is accepted: a valid window, cnt in selFirst for each of its planes, ending at or below nSel, and ps_tensor_ok.  For an
// accepted tensor WF[i * E + p] + cnt <= nSel for every plane p, and segment k0 + cnt - 1 exists in every plane
// (the segments k0 .. k0 + cnt - 1 of a plane that hold the elements [a, b) of a valid window, cnt 0 for an empty or a refused one: pw_range,
// the host's arithmetic too)
struct PwRange { u64 k0, cnt; };
HDEV PwRange pw_range(u64 a, u64 b, bool valid, u32 segLog) { const u64 k0 = a >> segLog; return { k0, valid && a < b ? ((b - 1) >> segLog) - k0 + 1 : 0 }; }
struct PwWin { u64 a, b, k0, cnt; bool ok; };
DEV PwWin pw_window(const u64* S, const u64* W, const u64* SF, const u64* WF, size_t i, u32 E, u32 segLog, size_t nSel)
{
    const u64 s0 = S[i], s1 = S[i + 1], n = s1 > s0 ? s1 - s0 : 0;
    PwWin w;
    w.a = W[2 * i]; w.b = W[2 * i + 1];
    w.ok = w.a <= w.b && w.b <= n / E;
    const PwRange r = pw_range(w.a, w.b, w.ok, segLog);
    w.k0 = r.k0; w.cnt = r.cnt;
    for (u32 p = 0; p < E; ++p) w.ok = w.ok && WF[i * E + p + 1] - WF[i * E + p] == w.cnt;
    w.ok = w.ok && WF[i * E] <= WF[(i + 1) * E] && WF[(i + 1) * E] <= nSel && ps_tensor_ok(S, SF, i, E, segLog);
    return w;
}

// ---- patching segmented tensors (planes_patch.hip; fsehip.h, "patching segmented tensors") ----
// the bytes [at, at + m) of a tensor of n bytes that its selected segments k0 .. k0 + cnt - 1 cover: at is a multiple of E, so the planes of
// this sub-tensor are those segments of the tensor's planes (the host's arithmetic too)
struct PpSub { u64 at, m; };
HDEV PpSub pp_sub(u64 n, u64 k0, u64 cnt, u32 E, u32 segLog)
{
    const u64 at = (k0 << segLog) * E, full = (cnt << segLog) * E;
    return { at, cnt && at < n ? (n - at < full ? n - at : full) : 0 };
}
// what tensor i stages: the bytes [at, at + m) of it, accepted iff its slot in S lies below the capacity, its window is valid and its pair
// of stage offsets holds exactly those m bytes below the stage's capacity
struct PpStage { u64 at, m; bool ok; };
DEV PpStage pp_stage(const u64* S, const u64* W, const u64* T, size_t i, u32 E, u32 segLog, u64 capacity, u64 stageCapacity)
{
    const u64 s0 = S[i], s1 = S[i + 1], n = s1 > s0 ? s1 - s0 : 0, a = W[2 * i], b = W[2 * i + 1], t0 = T[i], t1 = T[i + 1];
    const bool valid = s0 <= s1 && s1 <= capacity && a <= b && b <= n / E;
    const PwRange r = pw_range(a, b, valid, segLog);
    const PpSub sub = pp_sub(n, r.k0, r.cnt, E, segLog);
    return { sub.at, sub.m, valid && t0 <= t1 && t1 <= stageCapacity && t1 - t0 == sub.m };
}
// frame q of a packed batch lies inside its buffer and holds its result: 0 <= F[q] <= F[q + 1] <= capacity, R[q] <= F[q + 1] - F[q]
DEV bool pp_extent_ok(const u64* F, const size_t* R, size_t q, u64 capacity)
{
    const u64 f0 = F[q], f1 = F[q + 1];
    const size_t r = R[q];
    return f0 <= f1 && f1 <= capacity && !is_err(r) && (u64)r <= f1 - f0;
}

// ---- the launches and the argument checks of the C calls ----
// the one dispatch over the element size: f(std::integral_constant<int, E>) for the E that bad_elem lets through
template <class F> inline void pl_for_elem(unsigned E, F f)
{
    if (E == 1) f(std::integral_constant<int, 1>());
    else if (E == 2) f(std::integral_constant<int, 2>());
    else if (E == 4) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, 8>());
}

inline bool bad_elem(unsigned E) { return E != 1 && E != 2 && E != 4 && E != 8; }
inline bool bad_seg(unsigned segLog, unsigned blockSizeId) { return segLog < 10 + blockSizeId || segLog > 30; }
// ceil(capacity / T) + nTensors workgroups of PL_THREADS threads in one launch
inline bool bad_grid(u64 capacity, size_t nTensors) { return capacity >= ((u64)1 << 46) || (capacity >> PL_TILE_LOG) + 1 + nTensors >= ((u64)1 << 24); }
inline unsigned tile_grid(u64 capacity, size_t nTensors) { return (unsigned)(((capacity + PLANES_TILE - 1) >> PL_TILE_LOG) + nTensors); }
// fewer than 2^31 planes, and fewer than 2^31 segment (or selected) frames
inline bool bad_tensors(size_t nTensors, unsigned E) { return nTensors >= ((size_t)1 << 31) / E; }
inline bool bad_counts(size_t nTensors, unsigned E, size_t nFrames) { return bad_tensors(nTensors, E) || nFrames >= ((size_t)1 << 31); }
// what a composite hands on to the packed writer (one codec, or a codec per frame where w.d_codecs is given) and to the packed reader, for
// nFrames frames: the checks those calls make themselves, here in front of the composite's first launch
inline bool bad_writer(const PlWriter& w, size_t nFrames)
{
    if (w.blockSizeId > 6 || w.slotAlignLog > 12 || ((uintptr_t)w.d_workspace & 255u) || w.maxTotalBlocks >= ((size_t)1 << 31)) return true;
    if (!w.d_codecs)
        return (w.codec != 0 && w.codec != 1) || w.workspaceBytes < FSEHIP_frame_compress_packed_dbatch_workspaceSize(nFrames, w.maxTotalBlocks, w.blockSizeId, w.codec);
    if ((w.policy != FSEHIP_CODECS_GIVEN && w.policy != FSEHIP_CODECS_CHOOSE) || (w.policy == FSEHIP_CODECS_CHOOSE && w.tolerancePermille > 1000)) return true;
    return w.workspaceBytes < FSEHIP_frame_mixedWorkspaceBound(nFrames, w.maxTotalBlocks, w.blockSizeId, w.policy);
}
inline bool bad_reader(const void* d_workspace, size_t workspaceBytes, size_t nFrames, size_t maxTotalBlocks)
{
    return ((uintptr_t)d_workspace & 255u) || maxTotalBlocks >= ((size_t)1 << 31) || workspaceBytes < FSEHIP_frame_decompress_packed_dbatch_workspaceSize(nFrames, maxTotalBlocks);
}
}   // namespace

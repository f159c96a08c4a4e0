// planes_estimate.hip -- PLANE ESTIMATES (fsehip.h, "plane estimates"): from ONE read of the tensors (and of their bases), per tensor and
// candidate transform -- plain planes, predicted planes, planes of tensor XOR base, planes of zigzag(tensor - base) -- the order-0 cost of
// every plane in integers, an estimated size and a choice.  No plane buffer, no coder: what planes.hip and planes_pred.hip would STORE is
// counted into histograms instead.  Kernel launches only.
//
//   FSEHIP_planes_estimate_dbatch : k_est_zero (the counters of the workspace) -> k_est_count (a workgroup per (tile, tensor): LDS histograms
//                                   per candidate and plane, flushed into the tensor's counters) -> k_est_finish (a wave per tensor: the cost
//                                   of every plane, the estimates, the choice, the result)
//   FSEHIP_planes_estimate_stride_dbatch : k_est_zero -> k_est_count (the candidates beside PRED) -> k_est_count_stride (PRED at every
//                                   requested stride 1 .. 8) -> k_est_finish_stride (the stride choice in front of the transform choice):
//                                   "strides in the estimate", below the kernels of the first call
//
// THE COUNT is k_planes_split_pred's frame (planes_pred.hip): the flat ragged mapping, chunks of 16 whole elements per lane counted from the
// TENSOR's start (so a run starts only where a chunk does, and a chunk's dwords hold whole elements for the subtraction), head and tail an
// element per thread.  Which tile a byte is counted in does not matter to a histogram; which plane it belongs to is the split's rule, byte
// k of the tensor to plane k mod E, the trailing n mod E bytes in their E == 1 forms.  A lane loads its chunk once (and the base's chunk
// where XOR or SUB is asked for) and derives every requested candidate from those registers with the splits' own helpers (planes_dev.h:
// pp_prev, pl_sub4, pl_deinterleave); the candidate set is an argument that is uniform over the launch, so a candidate that is not asked
// for costs neither a load nor a branch taken.  LDS: 4 candidates x E planes x 256 bins of 8 / E columns of 32 bits -- 32 KB for every E.
//
// THE HOT BIN.  The high planes of a delta are almost all zeros (tensor == base: all of them), so every byte of every lane would go to ONE
// LDS word, 64 lanes deep and 16 times per chunk and plane.  k_hist spreads a hot row over 16 columns (hist.hip); 32 histograms have
// room for 8 / E of them (EstCols below), which takes the edge off a plane that is only mostly one value.  For a plane that is one value
// (EST_HOT, measured: EXPERIMENTS.md):
//   1  a lane whose 16 bytes of a plane are one value adds 16 once;
//   2  (the default) and where every active lane of the wave says so of the same value, one lane adds 16 x the number of lanes.
// Both are exact: the same counts, in fewer additions.  EST_HOT 0 is the plain form, kept for the A/B.
//
// THE FLUSH: a tile's non-zero bins go to the tensor's counters in the workspace by global 32-bit atomic adds -- integers, so the order
// does not matter and a replayed graph gives the same numbers.  A counter holds at most the bytes of a plane: tensors of 2^32 bytes and
// more are refused (srcSize_wrong).  The call zeroes the counters itself, by a launch, every time.
//
// THE FINISH: a wave per tensor walks its requested (candidate, plane) histograms: 4 bins per lane, L() by count-leading-zeros and the
// table T, c (L(N) - L(c)) summed over the wave (dev_common.h's 64-bit scan: all 64 lanes, every branch in front of it is uniform), then
// min(N, ceil(bits256 / 2048)) per plane, their sum per candidate and the choice.
#include "planes_dev.h"

namespace {
#ifndef EST_HOT
#define EST_HOT 2
#endif
#ifndef EST_SPREAD
#define EST_SPREAD 8
#endif
#define EST_CANDS 4u
// COLUMNS: a bin is EST_COLS<E> words, lane l adds to word l mod EST_COLS -- the lanes of one LDS instruction that meet in a bin (the few
// exponent values of a bf16 plane, the zeros of a delta plane that is only mostly zero) queue up at that many words instead of one.  As
// many as keep the histograms at 32 KB for every element size: 8 / E
template <int E> struct EstCols { static constexpr u32 LOG = EST_SPREAD >= 8 * E ? 3 : EST_SPREAD >= 4 * E ? 2 : EST_SPREAD >= 2 * E ? 1 : 0, N = 1u << LOG; };
#define EST_MAX ((u64)1 << 32)                                    // a tensor of this many bytes could wrap a 32-bit counter
enum { EST_M_PLAIN = 1u << FSEHIP_EST_PLAIN, EST_M_PRED = 1u << FSEHIP_EST_PRED, EST_M_XOR = 1u << FSEHIP_EST_XOR, EST_M_SUB = 1u << FSEHIP_EST_SUB,
       EST_M_BASE = EST_M_XOR | EST_M_SUB, EST_M_ALL = 15u };

// T[f] = floor(256 log2(1 + f / 256) + 0.5) (fsehip.h, "plane estimates"; the nearest half is 8e-4 away: the rounding is not in doubt)
__device__ const u16 EST_T[256] = {
      0,   1,   3,   4,   6,   7,   9,  10,  11,  13,  14,  16,  17,  18,  20,  21,
     22,  24,  25,  26,  28,  29,  30,  32,  33,  34,  36,  37,  38,  40,  41,  42,
     44,  45,  46,  47,  49,  50,  51,  52,  54,  55,  56,  57,  59,  60,  61,  62,
     63,  65,  66,  67,  68,  69,  71,  72,  73,  74,  75,  77,  78,  79,  80,  81,
     82,  84,  85,  86,  87,  88,  89,  90,  92,  93,  94,  95,  96,  97,  98,  99,
    100, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 116, 117,
    118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 130, 131, 132, 133,
    134, 135, 136, 137, 138, 139, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149,
    150, 151, 152, 153, 154, 155, 155, 156, 157, 158, 159, 160, 161, 162, 163, 164,
    165, 166, 167, 168, 169, 169, 170, 171, 172, 173, 174, 175, 176, 177, 178, 178,
    179, 180, 181, 182, 183, 184, 185, 185, 186, 187, 188, 189, 190, 191, 192, 192,
    193, 194, 195, 196, 197, 198, 198, 199, 200, 201, 202, 203, 203, 204, 205, 206,
    207, 208, 208, 209, 210, 211, 212, 212, 213, 214, 215, 216, 216, 217, 218, 219,
    220, 220, 221, 222, 223, 224, 224, 225, 226, 227, 228, 228, 229, 230, 231, 231,
    232, 233, 234, 234, 235, 236, 237, 238, 238, 239, 240, 241, 241, 242, 243, 244,
    244, 245, 246, 247, 247, 248, 249, 249, 250, 251, 252, 252, 253, 254, 255, 255,
};
// L(x) = 256 floor(log2 x) + T[the eight bits below the leading one], x >= 1 (0 -> 0: never used, N == 0 has no counts)
DEV u32 est_L(u64 x)
{
    if (x == 0) return 0;
    const u32 e = 63u - (u32)__builtin_clzll(x);
    return 256u * e + EST_T[((x << (63u - e)) >> 55) & 0xFFu];
}

HDEV u32 est_rank(u32 mask, u32 c) { return (u32)__builtin_popcount(mask & ((1u << c) - 1u)); }

// the counters of the workspace, zeroed by a launch (16 bytes per thread and step: the workspace is 256-byte aligned and a multiple of 256)
__global__ __launch_bounds__(PL_THREADS) void k_est_zero(uint4* p, u64 n16)
{
    for (u64 k = (u64)blockIdx.x * PL_THREADS + threadIdx.x; k < n16; k += (u64)gridDim.x * PL_THREADS) p[k] = make_uint4(0, 0, 0, 0);
}

// the 16 bytes o[0 .. 4) of one plane of a lane's chunk into the histogram hp (256 counters in LDS)
template <u32 CL> DEV void est_count16(u32* hp, const u32* o, u32 col)
{
#if EST_HOT >= 1
    const bool same = o[0] == o[1] && o[1] == o[2] && o[2] == o[3] && o[0] == (o[0] & 0xFFu) * 0x01010101u;
#if EST_HOT >= 2
    const u64 act = __ballot(1);
    if (__ballot(same) == act) {                                  // (uniform over the wave's active lanes)
        const u32 v0 = (u32)__builtin_amdgcn_readfirstlane((int)o[0]);
        if (__ballot(o[0] == v0) == act) {
            if (o[0] == v0 && __builtin_amdgcn_mbcnt_hi((u32)(act >> 32), __builtin_amdgcn_mbcnt_lo((u32)act, 0)) == 0)
                atomicAdd(&hp[(v0 & 0xFFu) << CL], 16u * (u32)__builtin_popcountll(act));
            return;
        }
    }
#endif
    if (same) { atomicAdd(&hp[((o[0] & 0xFFu) << CL) | col], 16u); return; }
#endif
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        atomicAdd(&hp[((o[k] & 0xFFu) << CL) | col], 1u);
        atomicAdd(&hp[(((o[k] >> 8) & 0xFFu) << CL) | col], 1u);
        atomicAdd(&hp[(((o[k] >> 16) & 0xFFu) << CL) | col], 1u);
        atomicAdd(&hp[((o[k] >> 24) << CL) | col], 1u);
    }
}
// the planes of a chunk's 4 E dwords (one candidate's) into that candidate's E histograms
template <int E> DEV void est_count_chunk(u32* hc, const u32* t, u32 col)
{
    u32 o[E][4];
    pl_deinterleave<E>(t, o);
#pragma unroll
    for (int p = 0; p < E; ++p) est_count16<EstCols<E>::LOG>(hc + ((256 * p) << EstCols<E>::LOG), o[p], col);
}
// byte p of the element value z into plane p's histogram
template <int E> DEV void est_count_elem(u32* hc, u64 z)
{
#pragma unroll
    for (int p = 0; p < E; ++p) atomicAdd(&hc[(256 * p + (u32)((z >> (8 * p)) & 0xFFu)) << EstCols<E>::LOG], 1u);
}
// element e of the tensor at sb (n bytes, base bb) a thread per element, head and tail: every requested candidate's bytes of it, as
// pp_elem_split, pl_sub_elem_split and the bytewise loop of k_planes_split place them.  The partial last element goes byte by byte: unchanged
// (plain, predicted), XORed, or in the E == 1 form of the subtraction
template <int E> DEV void est_elem(u32* hist, u32 mask, const u8* sb, const u8* bb, u64 n, u64 e)
{
    constexpr u32 CL = EstCols<E>::LOG, HC = (E * 256) << CL;      // (head and tail: column 0)
    const u64 k0 = e * E;
    if (k0 + E <= n) {
        u64 t = 0, b = 0, pr = 0;
#pragma unroll
        for (int p = 0; p < E; ++p) t |= (u64)sb[k0 + p] << (8 * p);
        if (mask & EST_M_BASE) {
#pragma unroll
            for (int p = 0; p < E; ++p) b |= (u64)bb[k0 + p] << (8 * p);
        }
        if ((mask & EST_M_PRED) && (e & (PP_RUN - 1))) {
#pragma unroll
            for (int p = 0; p < E; ++p) pr |= (u64)sb[k0 - E + p] << (8 * p);
        }
        if (mask & EST_M_PLAIN) est_count_elem<E>(hist + FSEHIP_EST_PLAIN * HC, t);
        if (mask & EST_M_PRED) est_count_elem<E>(hist + FSEHIP_EST_PRED * HC, pl_zz<E>(t, pr));
        if (mask & EST_M_XOR) est_count_elem<E>(hist + FSEHIP_EST_XOR * HC, t ^ b);
        if (mask & EST_M_SUB) est_count_elem<E>(hist + FSEHIP_EST_SUB * HC, pl_zz<E>(t, b));
    } else {
        for (u64 k = k0; k < n; ++k) {
            const u32 at = 256u * (u32)(k - k0), v = sb[k], b = (mask & EST_M_BASE) ? bb[k] : 0u;
            if (mask & EST_M_PLAIN) atomicAdd(&hist[FSEHIP_EST_PLAIN * HC + ((at + v) << CL)], 1u);
            if (mask & EST_M_PRED) atomicAdd(&hist[FSEHIP_EST_PRED * HC + ((at + v) << CL)], 1u);
            if (mask & EST_M_XOR) atomicAdd(&hist[FSEHIP_EST_XOR * HC + ((at + (v ^ b)) << CL)], 1u);
            if (mask & EST_M_SUB) atomicAdd(&hist[FSEHIP_EST_SUB * HC + ((at + (u32)pl_zz<1>(v, b)) << CL)], 1u);
        }
    }
}

// counters: per tensor popcount(mask) x E x 256 words, the requested candidates in rising id.  `mask` is uniform over the launch
template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_est_count(u32* counters, const u8* src, const u8* base, const u64* S, size_t nT, u64 capacity, u32 mask)
{
    constexpr u32 CL = EstCols<E>::LOG, HC = (E * 256) << CL;      // words per candidate
    __shared__ __attribute__((aligned(16))) u32 hist[EST_CANDS * HC];
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(S, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 s0 = S[i], s1 = S[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(s0 < s1) || s1 > capacity || s1 - s0 >= EST_MAX || lo >= s1 || lo + PLANES_TILE <= s0) return;
    const u64 n = s1 - s0;
    const u32 tid = threadIdx.x, col = tid & (EstCols<E>::N - 1u);
    const u8* const sb = src + s0;
    const u8* const bb = (mask & EST_M_BASE) ? base + s0 : nullptr;
    for (u32 c = 0; c < EST_CANDS; ++c) {
        if (!((mask >> c) & 1u)) continue;
        for (u32 k = tid; k < HC / 4; k += PL_THREADS) ((uint4*)(hist + c * HC))[k] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    const PlShare h = pl_share<E>(s0, n, lo, 0, 1);               // chunks at multiples of 16 elements of the tensor
    for (u64 c = tid; c < h.nch; c += PL_THREADS) {
        const u64 e = h.eb + 16 * c;
        u32 wv[4 * E], bv[4 * E], t[4 * E];
#pragma unroll
        for (int k = 0; k < E; ++k) __builtin_memcpy(&wv[4 * k], sb + e * E + 16 * k, 16);
        if (mask & EST_M_BASE) {
#pragma unroll
            for (int k = 0; k < E; ++k) __builtin_memcpy(&bv[4 * k], bb + e * E + 16 * k, 16);
        } else {
#pragma unroll
            for (int j = 0; j < 4 * E; ++j) bv[j] = 0;
        }
        if (mask & EST_M_PLAIN) est_count_chunk<E>(hist + FSEHIP_EST_PLAIN * HC, wv, col);
        if (mask & EST_M_PRED) {
            u32 pv[4 * E];
            pp_prev<E>(pv, wv, sb + e * E, (e & (PP_RUN - 1)) == 0);
#pragma unroll
            for (int j = 0; j < 4 * E; ++j) t[j] = wv[j];
#pragma unroll
            for (int k = 0; k < E; ++k) pl_sub4<E, false>(&t[4 * k], &pv[4 * k]);
            est_count_chunk<E>(hist + FSEHIP_EST_PRED * HC, t, col);
        }
        if (mask & EST_M_XOR) {
#pragma unroll
            for (int j = 0; j < 4 * E; ++j) t[j] = wv[j] ^ bv[j];
            est_count_chunk<E>(hist + FSEHIP_EST_XOR * HC, t, col);
        }
        if (mask & EST_M_SUB) {
#pragma unroll
            for (int j = 0; j < 4 * E; ++j) t[j] = wv[j];
#pragma unroll
            for (int k = 0; k < E; ++k) pl_sub4<E, false>(&t[4 * k], &bv[4 * k]);
            est_count_chunk<E>(hist + FSEHIP_EST_SUB * HC, t, col);
        }
    }
    const u64 nHead = h.eb - h.e0, nTail = h.e1 - h.et;
    for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) est_elem<E>(hist, mask, sb, bb, n, j < nHead ? h.e0 + j : h.et + (j - nHead));
    __syncthreads();
    // the flush: this tile's non-zero bins into the tensor's counters
    const u32 nReq = (u32)__builtin_popcount(mask);
    u32* const ct = counters + (u64)i * nReq * (E * 256);
    for (u32 c = 0; c < EST_CANDS; ++c) {
        if (!((mask >> c) & 1u)) continue;
        u32* const cc = ct + est_rank(mask, c) * (E * 256);
        for (u32 k = tid; k < E * 256; k += PL_THREADS) {
            u32 v = 0;
#pragma unroll
            for (u32 j = 0; j < EstCols<E>::N; ++j) v += hist[c * HC + (k << CL) + j];
            if (v) atomicAdd(&cc[k], v);
        }
    }
}

// bits256 of the plane of N bytes whose counters are cp[0 .. 256): four bins per lane, all 64 lanes in the scan; the same on every lane
DEV u64 est_plane_bits(const u32* cp, u64 N, u32 lane)
{
    const u32 LN = est_L(N);
    u64 part = 0;
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        const u32 cnt = cp[lane + WAVE * k];
        if (cnt) part += (u64)cnt * (LN - est_L(cnt));
    }
    return group_last64<64>(group_scan_incl_add64<64>(part, lane), lane);
}
// A wave per tensor.  Every branch in front of a scan depends on the tensor and the mask alone: all 64 lanes take it together
__global__ __launch_bounds__(WAVE) void k_est_finish(u64* planeBits, u64* estBytes, u8* choice, size_t* results, const u32* counters, const u64* S, size_t nT, u32 E,
                                                     u64 capacity, u32 mask, u32 margin)
{
    const size_t i = blockIdx.x;
    const u32 lane = threadIdx.x;
    const u64 s0 = S[i], s1 = S[i + 1];
    const bool inside = s0 <= s1 && s1 <= capacity, ok = inside && s1 - s0 < EST_MAX;
    const u64 n = ok ? s1 - s0 : 0;
    const u32 nReq = (u32)__builtin_popcount(mask);
    u64 est[EST_CANDS];
    for (u32 c = 0; c < EST_CANDS; ++c) {
        const bool req = ok && ((mask >> c) & 1u);
        u64 sum = req ? 0 : ~(u64)0;
        for (u32 p = 0; p < E; ++p) {
            u64 bits = ~(u64)0;
            if (req) {
                const u32* const cp = counters + (((u64)i * nReq + est_rank(mask, c)) * E + p) * 256;
                const u64 N = pl_size(n, p, E);
                bits = est_plane_bits(cp, N, lane);
                const u64 b = (bits + 2047) >> 11;
                sum += b < N ? b : N;
            }
            if (lane == 0) planeBits[((u64)i * EST_CANDS + c) * E + p] = bits;
        }
        est[c] = sum;
        if (lane == 0) estBytes[(u64)i * EST_CANDS + c] = sum;
    }
    if (lane != 0) return;
    u32 best = 0xFFu;
    if (ok) {
        for (u32 c = 0; c < EST_CANDS; ++c) {
            if (!((mask >> c) & 1u)) continue;
            if (best == 0xFFu || est[c] * 1000 < est[best] * (1000 - margin)) best = c;
        }
    }
    choice[i] = (u8)best;
    results[i] = ok ? (size_t)n : inside ? FERR(srcSize_wrong) : FERR(GENERIC);
}

// ---- strides in the estimate (fsehip.h, "strides in the estimate") ---------------------------------------------------------------------------
// k_est_count_stride is k_est_count for the PRED candidate at every requested stride 1 .. 8: the same frame, the same columns and hot-bin
// paths, one histogram set of E planes per REQUESTED stride in dynamic LDS -- 8 KB each for every E, so four strides take the 32 KB of
// k_est_count and all eight 64 KB.  A lane loads its chunk once and the 8 elements in front of it (zeros where the chunk starts a run: the
// chain heads of every stride), and every stride's predecessors are those 24 elements moved in registers (est_prev), as ps_prev moves
// them.  The stride set is an argument that is uniform over the launch: a stride that is not asked for costs neither a load nor a branch
// taken.  PLAIN, XOR and SUB are counted by k_est_count in a launch of its own (EXPERIMENTS.md: why not in this one).
#define EST_STRIDES ((u32)FSEHIP_PRED_MAX_STRIDE)
// y: the 8 elements in front of a chunk (2 E dwords), then the chunk (4 E dwords) -> pv: the chunk's predecessors at stride S
template <int E, int S> DEV void est_prev(u32* pv, const u32* y)
{
    constexpr int B = (8 - S) * E, D = B / 4, OFF = B % 4;
#pragma unroll
    for (int j = 0; j < 4 * E; ++j) {
        if constexpr (OFF != 0) pv[j] = __builtin_amdgcn_alignbyte(y[D + j + 1], y[D + j], OFF);
        else pv[j] = y[D + j];
    }
}
// the strides S .. 8 of a chunk, each into the histograms of its rank among the requested ones
template <int E, int S> DEV void est_stride_chunks(u32* hist, u32 smask, const u32* y, u32 col)
{
    constexpr u32 HC = (E * 256) << EstCols<E>::LOG;
    if (smask & (1u << (S - 1))) {
        u32 pv[4 * E], t[4 * E];
        est_prev<E, S>(pv, y);
#pragma unroll
        for (int j = 0; j < 4 * E; ++j) t[j] = y[2 * E + j];
#pragma unroll
        for (int k = 0; k < E; ++k) pl_sub4<E, false>(&t[4 * k], &pv[4 * k]);
        est_count_chunk<E>(hist + est_rank(smask, S - 1) * HC, t, col);
    }
    if constexpr (S < (int)EST_STRIDES) est_stride_chunks<E, S + 1>(hist, smask, y, col);
}
// element e of the tensor at sb (n bytes) a thread per element, head and tail: every requested stride's bytes of it, as ps_elem_split places them
template <int E> DEV void est_stride_elem(u32* hist, u32 smask, const u8* sb, u64 n, u64 e)
{
    constexpr u32 CL = EstCols<E>::LOG, HC = (E * 256) << CL;      // (head and tail: column 0)
    const u64 k0 = e * E;
    u64 t = 0;
    if (k0 + E <= n) {
#pragma unroll
        for (int p = 0; p < E; ++p) t |= (u64)sb[k0 + p] << (8 * p);
    }
    u32 r = 0;
    for (u32 s = 1; s <= EST_STRIDES; ++s) {
        if (!((smask >> (s - 1)) & 1u)) continue;
        u32* const hc = hist + r++ * HC;
        if (k0 + E <= n) {
            u64 pr = 0;
            if ((e & (PP_RUN - 1)) >= s) {
#pragma unroll
                for (int p = 0; p < E; ++p) pr |= (u64)sb[k0 - (u64)s * E + p] << (8 * p);
            }
            est_count_elem<E>(hc, pl_zz<E>(t, pr));
        } else {
            for (u64 k = k0; k < n; ++k) atomicAdd(&hc[(256u * (u32)(k - k0) + sb[k]) << CL], 1u);
        }
    }
}

// counters: per tensor popcount(smask) x E x 256 words, the requested strides in rising order.  `smask` is uniform over the launch
template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_est_count_stride(u32* counters, const u8* src, const u64* S, size_t nT, u64 capacity, u32 smask)
{
    constexpr u32 CL = EstCols<E>::LOG, HC = (E * 256) << CL;      // words per stride: 8 KB
    extern __shared__ __attribute__((aligned(16))) u32 shist[];   // popcount(smask) x HC words
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(S, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 s0 = S[i], s1 = S[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(s0 < s1) || s1 > capacity || s1 - s0 >= EST_MAX || lo >= s1 || lo + PLANES_TILE <= s0) return;
    const u64 n = s1 - s0;
    const u32 tid = threadIdx.x, col = tid & (EstCols<E>::N - 1u), nReq = (u32)__builtin_popcount(smask);
    const u8* const sb = src + s0;
    for (u32 k = tid; k < nReq * (HC / 4); k += PL_THREADS) ((uint4*)shist)[k] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const PlShare h = pl_share<E>(s0, n, lo, 0, 1);               // chunks at multiples of 16 elements of the tensor
    for (u64 c = tid; c < h.nch; c += PL_THREADS) {
        const u64 e = h.eb + 16 * c;
        u32 y[6 * E];
#pragma unroll
        for (int j = 0; j < 2 * E; ++j) y[j] = 0;
        if (e & (PP_RUN - 1)) __builtin_memcpy(y, sb + e * E - 8 * E, 8 * E);      // (no run starts here: at least 16 elements lie in front)
#pragma unroll
        for (int k = 0; k < E; ++k) __builtin_memcpy(&y[2 * E + 4 * k], sb + e * E + 16 * k, 16);
        est_stride_chunks<E, 1>(shist, smask, y, col);
    }
    const u64 nHead = h.eb - h.e0, nTail = h.e1 - h.et;
    for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) est_stride_elem<E>(shist, smask, sb, n, j < nHead ? h.e0 + j : h.et + (j - nHead));
    __syncthreads();
    u32* const ct = counters + (u64)i * nReq * (E * 256);          // the flush: this tile's non-zero bins into the tensor's counters
    for (u32 k = tid; k < nReq * (E * 256); k += PL_THREADS) {
        u32 v = 0;
#pragma unroll
        for (u32 j = 0; j < EstCols<E>::N; ++j) v += shist[(k << CL) + j];
        if (v) atomicAdd(&ct[k], v);
    }
}

// k_est_finish with the stride choice in front of the transform choice.  cA: the counters of k_est_count for mask & ~PRED; cB: those of
// k_est_count_stride (PRED requested: nS = popcount(smask) sets per tensor, else none).  The PRED slots hold the numbers of the chosen
// stride.  Every branch in front of a scan depends on the tensor, the masks and numbers that are the same on every lane
__global__ __launch_bounds__(WAVE) void k_est_finish_stride(u64* planeBits, u64* estBytes, u8* choice, size_t* results, u64* strideEst, u8* strides, const u32* cA,
                                                            const u32* cB, const u64* S, size_t nT, u32 E, u64 capacity, u32 mask, u32 smask, u32 margin, u32 settle)
{
    const size_t i = blockIdx.x;
    const u32 lane = threadIdx.x;
    const u64 s0 = S[i], s1 = S[i + 1];
    const bool inside = s0 <= s1 && s1 <= capacity, ok = inside && s1 - s0 < EST_MAX;
    const u64 n = ok ? s1 - s0 : 0;
    const u32 maskA = mask & ~(u32)EST_M_PRED, nA = (u32)__builtin_popcount(maskA), nS = (mask & EST_M_PRED) ? (u32)__builtin_popcount(smask) : 0;
    const u32* const tB = cB + (u64)i * nS * E * 256;
    u32 bs = 0xFFu;                                               // the best stride so far, as its bit number
    u64 estBs = 0;
    for (u32 s = 0; s < EST_STRIDES; ++s) {
        const bool req = ok && nS && ((smask >> s) & 1u);
        u64 sum = req ? 0 : ~(u64)0;
        if (req) {
            for (u32 p = 0; p < E; ++p) {
                const u64 N = pl_size(n, p, E), b = (est_plane_bits(tB + (est_rank(smask, s) * E + p) * 256, N, lane) + 2047) >> 11;
                sum += b < N ? b : N;
            }
            if (bs == 0xFFu || sum * 1000 < estBs * (1000 - margin)) { bs = s; estBs = sum; }
        }
        if (lane == 0 && strideEst) strideEst[(u64)i * EST_STRIDES + s] = sum;
    }
    u64 est[EST_CANDS];
    for (u32 c = 0; c < EST_CANDS; ++c) {
        const bool req = ok && ((mask >> c) & 1u);
        u64 sum = req ? 0 : ~(u64)0;
        for (u32 p = 0; p < E; ++p) {
            u64 bits = ~(u64)0;
            if (req) {
                const u32* const cp = c == FSEHIP_EST_PRED ? tB + (est_rank(smask, bs) * E + p) * 256 : cA + (((u64)i * nA + est_rank(maskA, c)) * E + p) * 256;
                const u64 N = pl_size(n, p, E);
                bits = est_plane_bits(cp, N, lane);
                const u64 b = (bits + 2047) >> 11;
                sum += b < N ? b : N;
            }
            if (lane == 0) planeBits[((u64)i * EST_CANDS + c) * E + p] = bits;
        }
        est[c] = sum;
        if (lane == 0) estBytes[(u64)i * EST_CANDS + c] = sum;
    }
    if (lane != 0) return;
    u32 best = 0xFFu;
    if (ok) {
        for (u32 c = 0; c < EST_CANDS; ++c) {
            if (!((mask >> c) & 1u)) continue;
            if (best == 0xFFu || est[c] * 1000 < est[best] * (1000 - margin)) best = c;
        }
    }
    choice[i] = (u8)best;
    strides[i] = !ok ? (u8)0xFF : (bs == 0xFFu || (settle && best != FSEHIP_EST_PRED)) ? (u8)1 : (u8)(bs + 1);
    results[i] = ok ? (size_t)n : inside ? FERR(srcSize_wrong) : FERR(GENERIC);
}

inline size_t r256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool bad_mask(unsigned mask) { return mask == 0 || (mask & ~EST_M_ALL); }
inline bool bad_estimate(size_t nTensors, unsigned E, unsigned mask) { return bad_elem(E) || bad_mask(mask) || nTensors >= ((size_t)1 << 24); }
// the counters: per tensor and requested candidate E histograms of 256 words
inline size_t est_workspace(size_t nTensors, unsigned E, unsigned mask) { return r256(nTensors * (size_t)__builtin_popcount(mask) * E * 1024); }
}   // namespace

extern "C" size_t FSEHIP_planes_estimate_workspaceBound(size_t nTensors, unsigned elemBytes, unsigned candidateMask)
{
    if (bad_estimate(nTensors, elemBytes, candidateMask)) return FSEHIP_ERROR(GENERIC);
    return est_workspace(nTensors, elemBytes, candidateMask);
}

extern "C" int FSEHIP_planes_estimate_dbatch(uint64_t* d_planeBits, uint64_t* d_estBytes, uint8_t* d_choice, size_t* d_results, const void* d_src, const void* d_base,
                                             const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity, unsigned candidateMask,
                                             unsigned marginPermille, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (!d_planeBits || !d_estBytes || !d_choice || !d_results || !d_src || !d_srcOffsets || bad_estimate(nTensors, elemBytes, candidateMask) ||
        bad_grid(capacity, nTensors) || ((candidateMask & EST_M_BASE) && !d_base) || marginPermille > 1000)
        return (int)hipErrorInvalidValue;
    const size_t need = est_workspace(nTensors, elemBytes, candidateMask);
    if ((need && !d_workspace) || ((uintptr_t)d_workspace & 255u) || workspaceBytes < need) return (int)hipErrorInvalidValue;
    if (nTensors == 0) return (int)hipSuccess;
    const hipStream_t s = (hipStream_t)stream;
    const u64* const S = (const u64*)d_srcOffsets;
    const u64 n16 = need / 16;
    const u64 zb = (n16 + PL_THREADS - 1) / PL_THREADS;
    hipLaunchKernelGGL(k_est_zero, dim3((unsigned)(zb < 65536 ? zb : 65536)), dim3(PL_THREADS), 0, s, (uint4*)d_workspace, n16);
    if (capacity) {
        const dim3 g(tile_grid(capacity, nTensors)), b(PL_THREADS);
        pl_for_elem(elemBytes, [&](auto eb) {
            hipLaunchKernelGGL((k_est_count<decltype(eb)::value>), g, b, 0, s, (u32*)d_workspace, (const u8*)d_src, (const u8*)d_base, S, nTensors, (u64)capacity,
                               (u32)candidateMask);
        });
    }
    hipLaunchKernelGGL(k_est_finish, dim3((unsigned)nTensors), dim3(WAVE), 0, s, (u64*)d_planeBits, (u64*)d_estBytes, d_choice, d_results, (const u32*)d_workspace, S,
                       nTensors, (u32)elemBytes, (u64)capacity, (u32)candidateMask, (u32)marginPermille);
    return (int)hipGetLastError();
}

// ---- strides in the estimate: the C calls ----
namespace {
// a stride set of 0 or beyond stride 8, or more than stride 1 where PRED is no candidate
inline bool bad_smask(unsigned mask, unsigned smask) { return smask == 0 || (smask & ~0xFFu) || (smask != 1 && !(mask & EST_M_PRED)); }
inline unsigned est_stride_sets(unsigned mask, unsigned smask) { return (mask & EST_M_PRED) ? (unsigned)__builtin_popcount(smask) : 0; }
// the counters of k_est_count for the candidates beside PRED, then those of k_est_count_stride: per tensor and requested stride E histograms
inline size_t est_stride_workspace(size_t nTensors, unsigned E, unsigned mask, unsigned smask)
{
    return r256(nTensors * (size_t)(__builtin_popcount(mask & ~(unsigned)EST_M_PRED) + est_stride_sets(mask, smask)) * E * 1024);
}
}   // namespace

extern "C" size_t FSEHIP_planes_estimate_stride_workspaceBound(size_t nTensors, unsigned elemBytes, unsigned candidateMask, unsigned strideMask)
{
    if (bad_estimate(nTensors, elemBytes, candidateMask) || bad_smask(candidateMask, strideMask)) return FSEHIP_ERROR(GENERIC);
    return est_stride_workspace(nTensors, elemBytes, candidateMask, strideMask);
}

int planes_estimate_stride(uint64_t* d_planeBits, uint64_t* d_estBytes, uint8_t* d_choice, size_t* d_results, uint64_t* d_strideEstBytes, uint8_t* d_strides,
                           const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                           unsigned candidateMask, unsigned marginPermille, void* d_workspace, size_t workspaceBytes, unsigned strideMask, bool settle, void* stream)
{
    if (!d_planeBits || !d_estBytes || !d_choice || !d_results || !d_strides || !d_src || !d_srcOffsets || bad_estimate(nTensors, elemBytes, candidateMask) ||
        bad_smask(candidateMask, strideMask) || bad_grid(capacity, nTensors) || ((candidateMask & EST_M_BASE) && !d_base) || marginPermille > 1000)
        return (int)hipErrorInvalidValue;
    const size_t need = est_stride_workspace(nTensors, elemBytes, candidateMask, strideMask);
    if ((need && !d_workspace) || ((uintptr_t)d_workspace & 255u) || workspaceBytes < need) return (int)hipErrorInvalidValue;
    if (nTensors == 0) return (int)hipSuccess;
    const hipStream_t s = (hipStream_t)stream;
    const u64* const S = (const u64*)d_srcOffsets;
    const unsigned maskA = candidateMask & ~(unsigned)EST_M_PRED, nS = est_stride_sets(candidateMask, strideMask);
    u32* const cA = (u32*)d_workspace;
    u32* const cB = cA + nTensors * (size_t)__builtin_popcount(maskA) * elemBytes * 256;
    const u64 n16 = need / 16;
    const u64 zb = (n16 + PL_THREADS - 1) / PL_THREADS;
    hipLaunchKernelGGL(k_est_zero, dim3((unsigned)(zb < 65536 ? zb : 65536)), dim3(PL_THREADS), 0, s, (uint4*)d_workspace, n16);
    if (capacity) {
        const dim3 g(tile_grid(capacity, nTensors)), b(PL_THREADS);
        pl_for_elem(elemBytes, [&](auto eb) {
            constexpr int E = decltype(eb)::value;
            if (maskA) hipLaunchKernelGGL((k_est_count<E>), g, b, 0, s, cA, (const u8*)d_src, (const u8*)d_base, S, nTensors, (u64)capacity, (u32)maskA);
            if (nS) hipLaunchKernelGGL((k_est_count_stride<E>), g, b, nS * (((E * 256u) << EstCols<E>::LOG) * 4u), s, cB, (const u8*)d_src, S, nTensors, (u64)capacity, (u32)strideMask);
        });
    }
    hipLaunchKernelGGL(k_est_finish_stride, dim3((unsigned)nTensors), dim3(WAVE), 0, s, (u64*)d_planeBits, (u64*)d_estBytes, d_choice, d_results, (u64*)d_strideEstBytes,
                       d_strides, (const u32*)cA, (const u32*)cB, S, nTensors, (u32)elemBytes, (u64)capacity, (u32)candidateMask, (u32)strideMask, (u32)marginPermille,
                       (u32)settle);
    return (int)hipGetLastError();
}

extern "C" int FSEHIP_planes_estimate_stride_dbatch(uint64_t* d_planeBits, uint64_t* d_estBytes, uint8_t* d_choice, size_t* d_results, uint64_t* d_strideEstBytes,
                                                    uint8_t* d_strides, const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors,
                                                    unsigned elemBytes, uint64_t capacity, unsigned candidateMask, unsigned marginPermille, void* d_workspace,
                                                    size_t workspaceBytes, unsigned strideMask, void* stream)
{
    return planes_estimate_stride(d_planeBits, d_estBytes, d_choice, d_results, d_strideEstBytes, d_strides, d_src, d_base, d_srcOffsets, nTensors, elemBytes, capacity,
                                  candidateMask, marginPermille, d_workspace, workspaceBytes, strideMask, false, stream);
}

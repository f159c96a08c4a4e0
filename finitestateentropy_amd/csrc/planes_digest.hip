// planes_digest.hip -- TENSOR DIGESTS AND CHECKED DELTAS (fsehip.h, "tensor digests and checked deltas"): a 64-bit digest of every tensor of
// a flat buffer at the memory rate, and a gate that turns "the base is not the one the delta was made against" into frames the readers
// refuse.  A delta's frames are intact whatever base the receiver holds; only a digest of the base can tell a stale one, and one serial XXH32
// chain per tensor (k_xxh32 of frame_dev.hip, about 1.5 GB/s) would take most of a second over a GiB.
//
//   FSEHIP_tensor_digest_dbatch : k_dg_layout (per tensor its size behind its tile digests) -> k_dg_tiles (a wave per tile: 64 lane streams,
//                                 folded to the tile digest) -> k_dg_top (a lane quad per tensor and seed over the tensor's tile digests and
//                                 size: digest and result)
//   FSEHIP_tensor_gate_dbatch   : k_dg_gate (a thread per frame offset and per tensor)
//
// The digest (normative in fsehip.h).  A tensor of n bytes is cut into TILES of T = 32 KB from its first byte, a tile of L bytes into 16-byte
// pieces q = 0 .. ceil(L / 16) - 1 (only the last may be short).  Lane l owns the pieces q mod 64 == l; h[l] = XXH32(its pieces in rising q,
// S0) -- a round of the wave is one coalesced 1 KB read, each lane one 16-byte load, and a lane runs the four accumulators of ITS stream, so
// no lane waits for another before the fold.  The tile digest is XXH32 of the 64 h[l] (256 bytes) with S0 and with S1, the tensor digest
// XXH32 with S0 and S1 over its tile digests followed by the eight bytes of n.  Nothing depends on where the tensor lies.
//
// Work mapping (the ragged one of planes.hip): ceil(capacity / T) + nTensors work items, item w takes tile k = w - first(u) of the tensor u
// that pl_find gives it, first(u) = floor(S[u] / T) + u; idle where k >= nt(u).  Tile k of tensor u writes its eight bytes to SLOT
// first(u) + u + k of the workspace and the tensor's size goes to slot first(u) + u + nt(u): a tensor has one slot more than work items, so
// tile digests and size lie back to back as the one byte range that k_dg_top hashes.  For a tensor with S[u] <= S[u + 1] <= capacity
// floor(S[u] / T) + nt(u) <= ceil(capacity / T), so every slot it names is below G + nTensors; a tensor that fails that test names none.
#include "planes_dev.h"

namespace {
#define DG_P1 2654435761u
#define DG_P2 2246822519u
#define DG_P3 3266489917u
#define DG_P4 668265263u
#define DG_P5 374761393u
#define DG_S0 0u
#define DG_S1 0x9E3779B1u
#define DG_WAVES (PL_THREADS / WAVE)                             // work items per workgroup of k_dg_tiles: a wave each, none waits for another
#define DG_ROUNDS ((u32)(PLANES_TILE / (16 * WAVE)))              // 32 rounds of 1 KB in a full tile
#define DG_BATCH 8                                               // rounds loaded ahead of the chain: 8 x 16 bytes per lane in flight
static_assert(DG_ROUNDS % DG_BATCH == 0, "whole batches");

DEV u32 dg_rotl(u32 x, u32 r) { return __builtin_rotateleft32(x, r); }
DEV u32 dg_round(u32 v, u32 x) { return dg_rotl(v + x * DG_P2, 13) * DG_P1; }
DEV u32 dg_avalanche(u32 h) { h ^= h >> 15; h *= DG_P2; h ^= h >> 13; h *= DG_P3; h ^= h >> 16; return h; }
struct DgAcc { u32 v[4]; };
DEV DgAcc dg_init(u32 seed) { return { { seed + DG_P1 + DG_P2, seed + DG_P2, seed, seed - DG_P1 } }; }
DEV void dg_stripe(DgAcc& a, const u32* w) { a.v[0] = dg_round(a.v[0], w[0]); a.v[1] = dg_round(a.v[1], w[1]); a.v[2] = dg_round(a.v[2], w[2]); a.v[3] = dg_round(a.v[3], w[3]); }
DEV u32 dg_merge(const DgAcc& a) { return dg_rotl(a.v[0], 1) + dg_rotl(a.v[1], 7) + dg_rotl(a.v[2], 12) + dg_rotl(a.v[3], 18); }

// tensor u of the batch: accepted iff S[u] <= S[u + 1] <= capacity
struct DgTensor { bool ok; u64 s0, n, nt, slot0; };
DEV DgTensor dg_tensor(const u64* S, size_t u, u64 capacity)
{
    const u64 s0 = S[u], s1 = S[u + 1];
    DgTensor t;
    t.ok = s0 <= s1 && s1 <= capacity;
    t.s0 = s0; t.n = t.ok ? s1 - s0 : 0;
    t.nt = (t.n + PLANES_TILE - 1) >> PL_TILE_LOG;
    t.slot0 = (s0 >> PL_TILE_LOG) + 2 * (u64)u;                  // first(u) + u
    return t;
}

// per tensor its size into the slot behind its tile digests
__global__ void k_dg_layout(u64* slots, const u64* S, size_t nT, u64 capacity, u64 nSlots)
{
    const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nT) return;
    const DgTensor t = dg_tensor(S, u, capacity);
    if (t.ok && t.slot0 + t.nt < nSlots) slots[t.slot0 + t.nt] = t.n;   // (holds for every accepted tensor: see the head of the file)
}

// A wave per work item.  Full tile: DG_ROUNDS rounds, the 16-byte loads of DG_BATCH rounds in flight while the rounds of the batch before run
// through the four accumulators (everything unrolled: both batches are registers).  Partial tile: a loop over its rounds, whole pieces as
// above, the one short piece -- the tile's last -- bytewise into the tail of its lane's stream.  Then the 64 -> 1 fold by cross-lane reads:
// a lane quad per seed -- lane j of a quad runs accumulator j over the 16 stripes of H, with S1 where (lane & 4) and S0 elsewhere (the quads
// behind the first two run along, so that every lane is there to be read); lanes 0 and 4 hold lo and hi.
__global__ __launch_bounds__(PL_THREADS) void k_dg_tiles(u32* slots, const u8* src, const u64* S, size_t nT, u64 capacity, u64 G, u64 nSlots)
{
    const u32 lane = threadIdx.x % WAVE;
    const u64 w = (u64)blockIdx.x * DG_WAVES + threadIdx.x / WAVE;
    size_t u;
    if (w >= G || !pl_find(S, nT, w, u)) return;                  // (uniform over the wave, like every return below)
    const DgTensor t = dg_tensor(S, u, capacity);
    const u64 f = (t.s0 >> PL_TILE_LOG) + u;
    if (!t.ok || w < f) return;
    const u64 k = w - f, slot = t.slot0 + k;
    if (k >= t.nt || slot >= nSlots) return;
    const u64 at = k << PL_TILE_LOG;
    const u32 L = t.n - at < PLANES_TILE ? (u32)(t.n - at) : (u32)PLANES_TILE;
    const u8* const p = src + t.s0 + at + 16u * lane;
    DgAcc a = dg_init(DG_S0);
    u32 h;
    if (L == (u32)PLANES_TILE) {
        u32 buf[2][DG_BATCH][4];
#pragma unroll
        for (int j = 0; j < DG_BATCH; ++j) __builtin_memcpy(buf[0][j], p + 1024 * j, 16);
#pragma unroll
        for (int b = 0; b < (int)(DG_ROUNDS / DG_BATCH); ++b) {
            if (b + 1 < (int)(DG_ROUNDS / DG_BATCH)) {
#pragma unroll
                for (int j = 0; j < DG_BATCH; ++j) __builtin_memcpy(buf[(b + 1) & 1][j], p + 1024 * (DG_BATCH * (b + 1) + j), 16);
            }
#pragma unroll
            for (int j = 0; j < DG_BATCH; ++j) dg_stripe(a, buf[b & 1][j]);
        }
        h = dg_merge(a) + 16u * DG_ROUNDS;
    } else {
        u32 len = 0, rem = 0, tw[4] = { 0, 0, 0, 0 };
        for (u32 off = 16u * lane; off < L; off += 16u * WAVE) {
            const u8* const q = p + (off - 16u * lane);
            if (off + 16 <= L) { u32 x[4]; __builtin_memcpy(x, q, 16); dg_stripe(a, x); len += 16; }
            else {
                rem = L - off;
#pragma unroll
                for (u32 j = 0; j < 15; ++j)
                    if (j < rem) tw[j >> 2] |= (u32)q[j] << (8 * (j & 3));
            }
        }
        h = (len ? dg_merge(a) : DG_S0 + DG_P5) + len + rem;
#pragma unroll
        for (u32 j = 0; j < 3; ++j)
            if (4 * j + 4 <= rem) h = dg_rotl(h + tw[j] * DG_P3, 17) * DG_P4;
#pragma unroll
        for (u32 j = 0; j < 15; ++j)
            if (j >= (rem & ~3u) && j < rem) h = dg_rotl(h + ((tw[j >> 2] >> (8 * (j & 3))) & 0xFFu) * DG_P5, 11) * DG_P1;
    }
    h = dg_avalanche(h);
    // the fold: XXH32 of h[0 .. 63] as 256 bytes -- stripe s is h[4 s .. 4 s + 3], accumulator j takes h[4 s + j]
    const u32 j = lane & 3u, seed = (lane & 4u) ? DG_S1 : DG_S0;
    u32 v = j == 0 ? seed + DG_P1 + DG_P2 : j == 1 ? seed + DG_P2 : j == 2 ? seed : seed - DG_P1;
#pragma unroll
    for (u32 s = 0; s < 16; ++s) v = dg_round(v, (u32)__builtin_amdgcn_ds_bpermute((int)(4 * (4 * s + j)), (int)h));
    u32 d = dg_rotl(v, j == 0 ? 1u : j == 1 ? 7u : j == 2 ? 12u : 18u);
    d += lane_xor<1>(d, lane);
    d += lane_xor<2>(d, lane);
    d = dg_avalanche(d + 256u);
    if (lane == 0 || lane == 4) slots[2 * slot + (lane >> 2)] = d;
}

// The top level: a LANE QUAD per (tensor, seed), one accumulator per lane, over the tensor's slots -- its tile digests and its size, 8 nt + 8
// bytes -- both seeds in one launch.  The chain, its ring of loads ahead of it and its eight-wide middle loop are k_xxh32's (frame_dev.hip:
// a serial chain of about 1.5 GB/s, the known cost of a single giant tensor) -- A TWIN: a fix to either goes into both; it is a copy and
// not a shared helper because frame_dev.hip's device code was to stay byte for byte.  The slots are 8-byte aligned, so the tail is no
// bytes or two words.  The ring is entered from 127 tiles on (8 nt + 8 >= 1024 bytes), its refill loop from 255.  Lane 0 of the
// quad stores its half of the digest, the S0 quad the result too; a refused tensor gets 0 and GENERIC.
__global__ __launch_bounds__(WAVE) void k_dg_top(u32* digests, size_t* results, const u8* slots, const u64* S, size_t nT, u64 capacity, u64 nSlots)
{
    const size_t t = (size_t)blockIdx.x * WAVE + threadIdx.x, i = t >> 2, u = i >> 1;
    const u32 q = (u32)t & 3u, lane = threadIdx.x, seed = (i & 1) ? DG_S1 : DG_S0;
    const bool on = u < nT;                                       // (a quad beyond the tensors runs along with len 0: the wave stays whole for the lane exchange)
    DgTensor x = { false, 0, 0, 0, 0 };
    if (on) x = dg_tensor(S, u, capacity);
    const bool ok = on && x.ok && x.slot0 + x.nt < nSlots;
    const u64 len = ok ? 8 * x.nt + 8 : 0;
    const u8* const base = slots + (ok ? 8 * x.slot0 : 0);
    const u32* p = reinterpret_cast<const u32*>(base) + q;
    u32 v = q == 0 ? seed + DG_P1 + DG_P2 : q == 1 ? seed + DG_P2 : q == 2 ? seed : seed - DG_P1;
    u64 stripes = len >> 4;
    constexpr int NB = 4, NS = 16;                                // a ring of NB batches of NS stripes loaded ahead of the chain
    if (stripes >= (u64)(NB * NS)) {
        u32 buf[NB][NS];
        const u32* pl = p;
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int j = 0; j < NS; ++j) buf[k][j] = pl[4 * (k * NS + j)];
        pl += 4 * NB * NS;
        u64 left = stripes / NS - NB;                             // batches not loaded yet
        while (left >= (u64)NB) {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
#pragma unroll
                for (int j = 0; j < NS; ++j) v = dg_round(v, buf[k][j]);
#pragma unroll
                for (int j = 0; j < NS; ++j) buf[k][j] = pl[4 * (k * NS + j)];
                __builtin_amdgcn_sched_barrier(0);                // (keeps the refill here, as in k_xxh32)
            }
            pl += 4 * NB * NS; left -= NB;
        }
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int j = 0; j < NS; ++j) v = dg_round(v, buf[k][j]);
        stripes = left * NS + stripes % NS; p = pl;
    }
    while (stripes >= 8) {                                        // (the leftover of a long chain and the whole of a mid-size one: eight loads at a time)
        const u32 x0 = p[0], x1 = p[4], x2 = p[8], x3 = p[12], x4 = p[16], x5 = p[20], x6 = p[24], x7 = p[28];
        v = dg_round(v, x0); v = dg_round(v, x1); v = dg_round(v, x2); v = dg_round(v, x3); v = dg_round(v, x4); v = dg_round(v, x5); v = dg_round(v, x6); v = dg_round(v, x7);
        p += 32; stripes -= 8;
    }
    while (stripes) { v = dg_round(v, *p); p += 4; --stripes; }
    u32 h = dg_rotl(v, q == 0 ? 1u : q == 1 ? 7u : q == 2 ? 12u : 18u);
    h += lane_xor<1>(h, lane);
    h += lane_xor<2>(h, lane);
    if (!on || q != 0) return;
    if (len < 16) h = seed + DG_P5;
    h += (u32)len;
    if (len & 8) {                                                // (len is a multiple of 8)
        const u32* const r = reinterpret_cast<const u32*>(base + (len & ~(u64)15));
        h = dg_rotl(h + r[0] * DG_P3, 17) * DG_P4;
        h = dg_rotl(h + r[1] * DG_P3, 17) * DG_P4;
    }
    digests[2 * u + (i & 1)] = ok ? dg_avalanche(h) : 0;
    if (!(i & 1)) results[u] = ok ? (size_t)x.n : FERR(GENERIC);
}

// One thread per entry q <= nFrames of the gated offsets, and per tensor for its result.  The tensor that owns frame q is q / E without
// SF, else the largest i with SF[i E] <= q (values clamped to nFrames: the search of k_planes_select), where q lies below its end; a
// frame nobody owns and the last entry pass through.  Every index into F is clamped to nFrames.
DEV u64 dg_clamp(u64 x, u64 hi) { return x < hi ? x : hi; }
DEV bool dg_pass(const u64* D, const size_t* DR, const u64* X, size_t i) { return !is_err(DR[i]) && D[i] == X[i]; }
__global__ void k_dg_gate(u64* Gt, size_t* GR, const u64* F, size_t nF, const u64* SF, u32 E, const u64* D, const size_t* DR, const u64* X, size_t nT)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nT) { const size_t r = DR[q]; GR[q] = dg_pass(D, DR, X, q) || is_err(r) ? r : FERR(corruption_detected); }
    if (q > nF) return;
    u64 g = F[q];
    if (q < nF && nT) {
        const size_t i = SF ? pl_last_le(nT, q, [SF, E, nF](size_t m) { return dg_clamp(SF[m * E], nF); }) : q / E;
        const u64 b = SF ? dg_clamp(SF[i * E], nF) : (u64)i * E, e = SF ? dg_clamp(SF[(i + 1) * E], nF) : (u64)(i + 1) * E;
        if (i < nT && b <= q && q < e && !dg_pass(D, DR, X, i)) g = F[e];
    }
    Gt[q] = g;
}

inline size_t r256(size_t x) { return (x + 255) & ~(size_t)255; }
// the workspace: the slots, G + nTensors of eight bytes
inline size_t dg_workspace(u64 capacity, size_t nTensors) { return r256((tile_grid(capacity, nTensors) + nTensors) * 8); }
inline bool bad_digest(u64 capacity, size_t nTensors) { return nTensors >= ((size_t)1 << 31) || bad_grid(capacity, nTensors); }
}   // namespace

extern "C" size_t FSEHIP_tensor_digest_workspaceBound(uint64_t capacity, size_t nTensors)
{
    if (bad_digest(capacity, nTensors)) return FSEHIP_ERROR(GENERIC);
    return dg_workspace(capacity, nTensors);
}

extern "C" int FSEHIP_tensor_digest_dbatch(uint64_t* d_digests, size_t* d_results, const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, uint64_t capacity,
                                           void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (!d_digests || !d_results || !d_src || !d_srcOffsets || bad_digest(capacity, nTensors) || !d_workspace || ((uintptr_t)d_workspace & 255u) ||
        workspaceBytes < dg_workspace(capacity, nTensors))
        return (int)hipErrorInvalidValue;
    if (nTensors == 0) return (int)hipSuccess;
    u64* const slots = (u64*)d_workspace;
    const u64 G = tile_grid(capacity, nTensors), nSlots = G + nTensors;
    const u64* const S = (const u64*)d_srcOffsets;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dg_layout, dim3(grid_for(nTensors)), dim3(PL_THREADS), 0, s, slots, S, nTensors, (u64)capacity, nSlots);
    hipLaunchKernelGGL(k_dg_tiles, dim3((unsigned)((G + DG_WAVES - 1) / DG_WAVES)), dim3(PL_THREADS), 0, s, (u32*)slots, (const u8*)d_src, S, nTensors, (u64)capacity, G, nSlots);
    hipLaunchKernelGGL(k_dg_top, dim3((unsigned)((8 * nTensors + WAVE - 1) / WAVE)), dim3(WAVE), 0, s, (u32*)d_digests, d_results, (const u8*)slots, S, nTensors, (u64)capacity, nSlots);
    return (int)hipGetLastError();
}

extern "C" int FSEHIP_tensor_gate_dbatch(uint64_t* d_gatedOffsets, size_t* d_gateResults, const uint64_t* d_frameOffsets, size_t nFrames, const uint64_t* d_frameFirst,
                                         unsigned elemBytes, const uint64_t* d_digests, const size_t* d_digestResults, const uint64_t* d_expected, size_t nTensors,
                                         void* stream)
{
    if (bad_elem(elemBytes) || !d_gatedOffsets || !d_gateResults || !d_frameOffsets || !d_digests || !d_digestResults || !d_expected || bad_counts(nTensors, elemBytes, nFrames) ||
        (!d_frameFirst && nFrames != nTensors * elemBytes))
        return (int)hipErrorInvalidValue;
    const size_t n = nFrames + 1 > nTensors ? nFrames + 1 : nTensors;
    hipLaunchKernelGGL(k_dg_gate, dim3(grid_for(n)), dim3(PL_THREADS), 0, (hipStream_t)stream, (u64*)d_gatedOffsets, d_gateResults, (const u64*)d_frameOffsets, nFrames,
                       (const u64*)d_frameFirst, (u32)elemBytes, (const u64*)d_digests, d_digestResults, (const u64*)d_expected, nTensors);
    return (int)hipGetLastError();
}

// frame_dev.hip -- the .fse frame (frame.hip; reference: programs/fileio.c:266-285 format, :286-432 writer, :462-626 reader) on DEVICE
// buffers: many contents -> many frames and back, kernel launches on the caller's stream and nothing else (no read-back, no
// synchronisation, no allocation, no memset / copy nodes: the calls can be captured into a HIP graph).
//
//   FSEHIP_XXH32_batch            : XXH32 of n byte ranges of one buffer, one lane quad per range
//   FSEHIP_frame_compress_dbatch  : k_fw_counts -> scan -> k_fw_blocks (every block of every content: where it starts, whose it is)
//                                   -> ONE call of the one-shot block coder over that offsets view (BlockView::offsets; results 0 / 1 /
//                                   size / error as the frame writer switches on them, frame.hip:160-177) -> k_fw_lens -> scan (record
//                                   positions; a frame's own = the difference to its first block's) -> k_xxh32 (trailers)
//                                   -> k_fw_verdict (per frame: result, magic, trailer) -> k_fw_assemble (per block: header + record)
//   FSEHIP_frame_compress_packed_dbatch: the same up to the record positions (fw_encode, shared with FSEHIP_frame_compress_dbatch) -> k_fw_sizes
//                                   (per frame: its result without a capacity; the size rounded up to the slot alignment) -> scan of those
//                                   -> k_fr_clamp: the destination offsets, an OUTPUT -> k_fw_place (per frame: does it fit its slot; magic,
//                                   trailer) -> k_fw_assemble over the offsets just produced
//   FSEHIP_frame_compress_packed_mixed_dbatch: the packed writer with a codec PER FRAME.  GIVEN: k_fm_route (per block, its size for its frame's
//                                   coder and 0 for the other) -> both one-shot coders over (offset, size) views of the same blocks and slots
//                                   -> k_fm_lens (per block: the owner's result, the record's length) -> scan -> k_fm_sizes.  CHOOSE: both coders
//                                   over every block into slots of their own -> k_fw_lens and scan for each -> k_fm_choose (per frame: both
//                                   sizes, the rule, the codec -- an OUTPUT).  Then, for both: scan, k_fr_clamp -> k_fm_place -> k_fm_assemble
//                                   (magic and records by the frame's codec)
//   FSEHIP_frame_decompress_dbatch: k_fr_count (header walk per frame) -> scan -> k_fr_clear + k_fr_fill (the block table) -> the one-shot
//                                   FSE and Huff0 decoders over (offset, size) views of the compressed blocks, writing every block in
//                                   place at the position its predecessors ANNOUNCE -> k_fr_expand (raw / RLE blocks) -> k_fr_settle (per
//                                   frame: the reader's walk over results, frame.hip:325-341; repairs a frame in which a block
//                                   regenerated less than announced) -> k_xxh32 -> k_fr_final
//   FSEHIP_frame_plan_dbatch      : k_fr_plan (the same header walk, summing what the blocks announce) -> scan of the aligned bounds, scan of
//                                   the block counts -> k_fr_clamp: destination offsets and the exact block total of frames of unknown size
//   FSEHIP_frame_decompress_packed_dbatch: k_fr_plan in place of k_fr_count, the two scans, k_fr_clamp -- then the reader from k_fr_clear on
//                                   over the offsets just produced (fr_decode, shared with FSEHIP_frame_decompress_dbatch)
// A caller's promise `maxTotalBlocks` sizes every per-block launch; what lies beyond the real block count is a block of size 0.
#include "internal.h"
#include "ncount_reader.h"
#include "bitreader.h"

namespace {
const u32 MAGIC_FSE = 0x183E2309u, MAGIC_HUF = 0x183E3309u;      // fileio.c:121-122
const unsigned MAX_BSID = 6;
enum { BT_COMPRESSED = 0, BT_RAW = 1, BT_RLE = 2, BT_CRC = 3 };  // fileio.c:137
#define FD_THREADS 256
#define FD_PER_WG 1024
#define FD_NONE 0xFFFFFFFFu
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline unsigned grid_for(size_t n) { return (unsigned)((n + FD_THREADS - 1) / FD_THREADS); }

// =====================================================================================================
//  XXH32 (public algorithm; fileio.c:303,339,408 streams it over the content).  A serial chain per item -- four accumulators, each
//  rotl(v + x * P2, 13) * P1 over its own dword of every 16-byte stripe -- so the parallel axis is the items.  A LANE QUAD per item, one
//  accumulator per lane.  Both shapes were compiled and their ISA read: a round is v_mad_u64_u32 -> v_alignbit_b32 -> v_mul_lo_u32, two
//  of the three quarter-rate.  With the four chains interleaved in one lane a stripe is 12 VALU instructions (8 quarter-rate) whatever the
//  number of live lanes -- a wave is issue-bound at about 144 cycles per stripe even for a single item; with a quad per item it is 3
//  instructions per stripe, the dependent chain itself, at the price of four times the waves and a two-step cross-lane sum at the end.
//  Measured (scripts/framedevbench.py): 0.24 GB/s per item in one lane, 1.5 GB/s in a quad with its loads far enough ahead (below) --
//  1024 items of 1 MiB in 0.69 instead of 4.3 ms.  A batch only loses to the one-lane form once quads fill every SIMD of the device
//  (beyond ~16k items), where the call runs at the memory rate either way.  Items start at any alignment (unaligned dword loads).
//  k_dg_top of planes_digest.hip is a TWIN of this chain (ring and middle loop, two seeds in one launch): a fix here goes there too.
// =====================================================================================================
#define XP1 2654435761u
#define XP2 2246822519u
#define XP3 3266489917u
#define XP4 668265263u
#define XP5 374761393u
DEV u32 xrotl(u32 x, u32 r) { return __builtin_rotateleft32(x, r); }
DEV u32 xround(u32 v, u32 x) { return xrotl(v + x * XP2, 13) * XP1; }
DEV u32 xld32(const u8* p) { u32 v; __builtin_memcpy(&v, p, 4); return v; }
// item i = data[starts[i], starts[i] + lens[i])  (lens == nullptr: up to starts[i + 1]); lanes 4i .. 4i+3 of the grid
__global__ __launch_bounds__(64) void k_xxh32(u32* hashes, const u8* data, const u64* starts, const u64* lens, size_t n, u32 seed)
{
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    const size_t i = t >> 2;
    const u32 q = (u32)t & 3u, lane = threadIdx.x;
    const bool on = i < n;                                        // (a quad beyond the items runs along with len 0: the wave stays whole for the lane exchange)
    const u64 at = on ? starts[i] : 0, len = on ? (lens ? lens[i] : starts[i + 1] - at) : 0;
    u32 v = q == 0 ? seed + XP1 + XP2 : q == 1 ? seed + XP2 : q == 2 ? seed : seed - XP1;
    const u8* p = data + at + 4u * q;
    u64 stripes = len >> 4;
    // Long items: a ring of XNB batches of XNS stripes (1 KB per lane) loaded ahead of the chain.  A batch's rounds take about 0.2 us, a load
    // from memory several times that: with the loads only one batch ahead the lone quad of a large item waits for memory, not for its chain.
    constexpr int XNB = 4, XNS = 16;
    if (stripes >= (u64)(XNB * XNS)) {
        u32 buf[XNB][XNS];
        const u8* pl = p;
#pragma unroll
        for (int k = 0; k < XNB; ++k)
#pragma unroll
            for (int j = 0; j < XNS; ++j) buf[k][j] = xld32(pl + 16 * (k * XNS + j));
        pl += 16 * XNB * XNS;
        u64 left = stripes / XNS - XNB;                           // batches not loaded yet
        while (left >= (u64)XNB) {
#pragma unroll
            for (int k = 0; k < XNB; ++k) {
#pragma unroll
                for (int j = 0; j < XNS; ++j) v = xround(v, buf[k][j]);
#pragma unroll
                for (int j = 0; j < XNS; ++j) buf[k][j] = xld32(pl + 16 * (k * XNS + j));
                __builtin_amdgcn_sched_barrier(0);                // (keeps the refill here: the scheduler otherwise sinks all loads behind the last batch)
            }
            pl += 16 * XNB * XNS; left -= XNB;
        }
#pragma unroll
        for (int k = 0; k < XNB; ++k)
#pragma unroll
            for (int j = 0; j < XNS; ++j) v = xround(v, buf[k][j]);
        stripes = left * XNS + stripes % XNS; p = pl;
    }
    while (stripes >= 8) {
        const u32 x0 = xld32(p), x1 = xld32(p + 16), x2 = xld32(p + 32), x3 = xld32(p + 48), x4 = xld32(p + 64), x5 = xld32(p + 80), x6 = xld32(p + 96), x7 = xld32(p + 112);
        v = xround(v, x0); v = xround(v, x1); v = xround(v, x2); v = xround(v, x3); v = xround(v, x4); v = xround(v, x5); v = xround(v, x6); v = xround(v, x7);
        p += 128; stripes -= 8;
    }
    while (stripes) { v = xround(v, xld32(p)); p += 16; --stripes; }
    u32 h = xrotl(v, q == 0 ? 1u : q == 1 ? 7u : q == 2 ? 12u : 18u);
    h += lane_xor<1>(h, lane);
    h += lane_xor<2>(h, lane);                                    // rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18) in every lane of the quad
    if (!on || q != 0) return;
    if (len < 16) h = seed + XP5;
    h += (u32)len;
    const u8* r = data + at + (len & ~(u64)15);
    const u8* const end = data + at + len;
    while (r + 4 <= end) { h = xrotl(h + xld32(r) * XP3, 17) * XP4; r += 4; }
    while (r < end) { h = xrotl(h + (u32)(*r) * XP5, 11) * XP1; ++r; }
    h ^= h >> 15; h *= XP2; h ^= h >> 13; h *= XP3; h ^= h >> 16;
    hashes[i] = h;
}

// =====================================================================================================
//  exclusive scan of n u64 in place, the total behind them (a[n]): sums of FD_PER_WG entries per workgroup, one workgroup over the sums,
//  then the entries again (the pattern of compact.hip)
// =====================================================================================================
DEV u64 fd_wg_scan(u64 v, u64* sh, u32 tid)                       // inclusive, over the FD_THREADS threads of a workgroup
{
    const u32 lane = tid & 63u, w = tid >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const u64 o = __shfl_up(v, off, WAVE); if ((int)lane >= off) v += o; }
    if (lane == 63) sh[w] = v;
    __syncthreads();
    u64 base = 0;
    for (u32 k = 0; k < w; ++k) base += sh[k];
    __syncthreads();
    return v + base;
}
__global__ __launch_bounds__(FD_THREADS) void k_scan_sums(const u64* a, size_t n, u64* partials)
{
    __shared__ u64 sh[4];
    const u32 tid = threadIdx.x;
    const size_t b0 = (size_t)blockIdx.x * FD_PER_WG;
    u64 sum = 0;
    for (u32 k = 0; k < FD_PER_WG / FD_THREADS; ++k) { const size_t b = b0 + tid + (size_t)k * FD_THREADS; if (b < n) sum += a[b]; }
    const u64 incl = fd_wg_scan(sum, sh, tid);
    if (tid == FD_THREADS - 1) partials[blockIdx.x] = incl;
}
__global__ __launch_bounds__(FD_THREADS) void k_scan_groups(u64* partials, u32 nGroups)
{
    __shared__ u64 sh[4];
    __shared__ u64 carry;
    const u32 tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (u32 g0 = 0; g0 < nGroups; g0 += FD_THREADS) {
        const u32 g = g0 + tid;
        const u64 v = g < nGroups ? partials[g] : 0;
        const u64 incl = fd_wg_scan(v, sh, tid);
        const u64 c = carry;
        if (g < nGroups) partials[g] = c + incl - v;
        __syncthreads();
        if (tid == FD_THREADS - 1) carry = c + incl;
        __syncthreads();
    }
    if (tid == 0) partials[nGroups] = carry;
}
__global__ __launch_bounds__(FD_THREADS) void k_scan_apply(u64* a, size_t n, const u64* partials, u32 nGroups)
{
    __shared__ u64 sh[4];
    __shared__ u64 carry;
    const u32 tid = threadIdx.x;
    const size_t b0 = (size_t)blockIdx.x * FD_PER_WG;
    if (tid == 0) carry = partials[blockIdx.x];
    __syncthreads();
    for (u32 k = 0; k < FD_PER_WG / FD_THREADS; ++k) {
        const size_t b = b0 + tid + (size_t)k * FD_THREADS;
        const u64 v = b < n ? a[b] : 0;
        const u64 incl = fd_wg_scan(v, sh, tid);
        const u64 c = carry;
        if (b < n) a[b] = c + incl - v;
        __syncthreads();
        if (tid == FD_THREADS - 1) carry = c + incl;
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid == 0) a[n] = partials[nGroups];
}
inline size_t scan_partials(size_t n) { return (n + FD_PER_WG - 1) / FD_PER_WG + 2; }           // u64 words of scratch
}   // namespace
// (declared in internal.h: planes_patch.hip scans its frame extents with it)
size_t exscan_partials(size_t n) { return scan_partials(n); }
hipError_t launch_exscan(u64* a, size_t n, u64* partials, hipStream_t s)
{
    const u32 nGroups = (u32)((n + FD_PER_WG - 1) / FD_PER_WG);
    if (n == 0) { hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(FD_THREADS), 0, s, a, 0u); return hipGetLastError(); }      // a[0] = 0
    hipLaunchKernelGGL(k_scan_sums, dim3(nGroups), dim3(FD_THREADS), 0, s, (const u64*)a, n, partials);
    hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(FD_THREADS), 0, s, partials, nGroups);
    hipLaunchKernelGGL(k_scan_apply, dim3(nGroups), dim3(FD_THREADS), 0, s, a, n, (const u64*)partials, nGroups);
    return hipGetLastError();
}
namespace {

// `len` bytes from s to d, any alignments, by the FD_THREADS threads of a workgroup: up to the next 16-byte boundary of d bytewise, 16-byte
// pieces (unaligned loads, aligned stores), the rest bytewise.  fill >= 0: that byte repeated instead.
DEV void fd_copy(u8* d, const u8* s, size_t len, u32 tid, int fill)
{
    const u32 f4 = (u32)(fill & 0xFF) * 0x01010101u;
    size_t head = (size_t)((0 - (uintptr_t)d) & 15u);
    if (head > len) head = len;
    if (tid < head) d[tid] = fill >= 0 ? (u8)fill : s[tid];
    const size_t body = (len - head) & ~(size_t)15;
    for (size_t off = head + 16 * (size_t)tid; off < head + body; off += 16 * FD_THREADS) {
        uint4 v = make_uint4(f4, f4, f4, f4);
        if (fill < 0) __builtin_memcpy(&v, s + off, 16);
        *(uint4*)(d + off) = v;
    }
    const size_t done = head + body;
    if (done + tid < len) d[done + tid] = fill >= 0 ? (u8)fill : s[done + tid];
}

// =====================================================================================================
//  writer
// =====================================================================================================
__global__ void k_fw_counts(u64* first, const u64* srcOff, size_t nFrames, u32 bsLog)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    const u64 n = srcOff[f + 1] - srcOff[f];
    first[f] = (n + ((u64)1 << bsLog) - 1) >> bsLog;
}
// block g (0 .. maxBlocks inclusive: the coder's offsets view has one entry more than blocks): where it starts in d_src and whose it is.
// Contents lie back to back, so a content's last block ends where the next content's first one starts; blocks beyond the real count
// start (and end) at the end of the last content.
__global__ void k_fw_blocks(u64* blkOff, u32* blkFrame, const u64* first, const u64* srcOff, size_t nFrames, size_t maxBlocks, u32 bsLog)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > maxBlocks) return;
    u32 frame = FD_NONE; u64 off = srcOff[nFrames];
    if (g < first[nFrames]) {
        size_t lo = 0, hi = nFrames - 1;                         // the smallest f with first[f + 1] > g
        while (lo < hi) { const size_t mid = (lo + hi) >> 1; if (first[mid + 1] > g) hi = mid; else lo = mid + 1; }
        frame = (u32)lo; off = srcOff[lo] + ((g - first[lo]) << bsLog);
    }
    blkOff[g] = off;
    if (g < maxBlocks) blkFrame[g] = frame;
}
// bytes of block g's record in its frame: header (1, or 3 for a block shorter than the block size) + raw block | RLE byte | 2 + compressed
__global__ void k_fw_lens(u64* pos, const size_t* cres, const u64* blkOff, const u32* blkFrame, size_t maxBlocks, u32 bsLog)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= maxBlocks) return;
    u64 len = 0;
    const size_t r = cres[g];
    if (blkFrame[g] != FD_NONE && !is_err(r)) {
        const u64 n = blkOff[g + 1] - blkOff[g];
        len = (n == ((u64)1 << bsLog) ? 1u : 3u) + (r == 0 ? n : r == 1 ? 1u : 2u + (u64)r);
    }
    pos[g] = len;
}
// what FSEHIP_frame_compress returns for content f at a capacity of FSEHIP_frame_compressBound (frame.hip:132-133,167,177): the frame's size, a
// block coder's error, or GENERIC for a frame beyond the caller's promise
DEV size_t fw_result(u64 b0, u64 b1, const u64* pos, const size_t* cres, size_t maxBlocks)
{
    if (b1 > b0 && b1 > maxBlocks) return FERR(GENERIC);                                       // beyond the caller's promise
    for (u64 g = b0; g < b1; ++g) if (is_err(cres[g])) return cres[g];                         // fileio.c:341
    return (size_t)(5 + (b1 > b0 ? pos[b1] - pos[b0] : 0) + 3);
}
// magic and block-size id in front of a frame of `size` bytes, the end mark behind its records
DEV void fw_ends(u8* out, u64 size, u32 hash, u32 bsid, int codec)
{
    const u32 magic = codec == 1 ? MAGIC_HUF : MAGIC_FSE;
    out[0] = (u8)magic; out[1] = (u8)(magic >> 8); out[2] = (u8)(magic >> 16); out[3] = (u8)(magic >> 24); out[4] = (u8)bsid;
    const u32 checksum = (hash >> 5) & ((1u << 22) - 1);                                        // fileio.c:408-416
    out[size - 3] = (u8)((checksum >> 16) + (BT_CRC << 6)); out[size - 2] = (u8)(checksum >> 8); out[size - 1] = (u8)checksum;
}
// per frame: the result of FSEHIP_frame_compress for this content (frame.hip:132-133,167,177); a good frame gets its magic and trailer here
__global__ void k_fw_verdict(u8* dst, const u64* dstOff, size_t* results, const u64* srcOff, const u64* first, const u64* pos, const size_t* cres,
                             const u32* hashes, size_t nFrames, size_t maxBlocks, u32 bsid, int codec)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    const u64 n = srcOff[f + 1] - srcOff[f], cap = dstOff[f + 1] - dstOff[f];
    const u64 b0 = first[f], b1 = first[f + 1];
    if (cap < 5 + n + 5 * (b1 - b0) + 3) { results[f] = FERR(dstSize_tooSmall); return; }      // FSEHIP_frame_compressBound
    const size_t r = fw_result(b0, b1, pos, cres, maxBlocks);
    if (!is_err(r)) fw_ends(dst + dstOff[f], r, hashes[f], bsid, codec);
    results[f] = r;
}
// the packed writer, per frame: k_fw_verdict's result without the capacity test into fsize, and what the frame takes of the destination -- its
// size rounded up to the slot alignment, 0 for a frame that fails -- into slots (scanned in place afterwards: the destination offsets)
__global__ void k_fw_sizes(size_t* fsize, u64* slots, const u64* first, const u64* pos, const size_t* cres, size_t nFrames, size_t maxBlocks, u32 alignLog)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    const size_t r = fw_result(first[f], first[f + 1], pos, cres, maxBlocks);
    fsize[f] = r;
    const u64 a = ((u64)1 << alignLog) - 1;
    slots[f] = is_err(r) ? 0 : ((u64)r + a) & ~a;
}
// ... and behind the scan and the clamp: a frame whose slot holds it gets its size, magic and trailer (dst == nullptr: the size alone), one
// whose slot the capacity cut short dstSize_tooSmall
__global__ void k_fw_place(u8* dst, const u64* dstOff, size_t* results, const size_t* fsize, const u32* hashes, size_t nFrames, u32 bsid, int codec)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    size_t r = fsize[f];
    if (!is_err(r)) {
        if (dstOff[f + 1] - dstOff[f] < (u64)r) r = FERR(dstSize_tooSmall);
        else if (dst) fw_ends(dst + dstOff[f], r, hashes[f], bsid, codec);
    }
    results[f] = r;
}
// one workgroup per block: its header and record at its place in its frame (frame.hip:163-174)
__global__ __launch_bounds__(FD_THREADS) void k_fw_assemble(u8* dst, const u64* dstOff, const size_t* results, const u8* src, const u64* blkOff, const u32* blkFrame,
                                                            const u64* first, const u64* pos, const size_t* cres, const u8* slots, size_t slotStride, u32 bsLog)
{
    const size_t g = blockIdx.x;
    const u32 f = blkFrame[g];
    if (f == FD_NONE || is_err(results[f])) return;              // uniform
    const u32 tid = threadIdx.x;
    const u64 n = blkOff[g + 1] - blkOff[g];
    const size_t r = cres[g];
    const u32 bt = r == 0 ? BT_RAW : r == 1 ? BT_RLE : BT_COMPRESSED;
    const bool full = n == ((u64)1 << bsLog);
    u8* out = dst + dstOff[f] + 5 + (pos[g] - pos[first[f]]);
    const u32 hdr = (full ? 1u : 3u) + (bt == BT_COMPRESSED ? 2u : 0u);
    if (tid == 0) {
        u32 o = 0;
        if (full) out[o++] = (u8)((bt << 6) + 0x20);
        else { out[o++] = (u8)(bt << 6); out[o++] = (u8)(n >> 8); out[o++] = (u8)n; }
        if (bt == BT_COMPRESSED) { out[o++] = (u8)(r >> 8); out[o++] = (u8)r; }
        else if (bt == BT_RLE) out[o] = src[blkOff[g]];
    }
    if (bt == BT_RAW) fd_copy(out + hdr, src + blkOff[g], (size_t)n, tid, -1);
    else if (bt == BT_COMPRESSED) fd_copy(out + hdr, slots + g * slotStride, r, tid, -1);
}

// ---- the mixed packed writer: a codec per frame (0 = FSE, 1 = Huff0), given by the caller or chosen by size ----
// GIVEN, per block: its size in the size array of its frame's coder, 0 in the other's -- a block of size 0 is "not compressible" to both
// coders after the histogram (k_fse_cprep, k_huf_cprep: result 0, nothing written to its slot), so both can share one slot array.  A
// frame whose codec byte is neither has no coder: 0 in both.
__global__ void k_fm_route(size_t* szF, size_t* szH, const u64* blkOff, const u32* blkFrame, const u8* codecs, size_t maxBlocks)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= maxBlocks) return;
    const u32 f = blkFrame[g];
    const size_t n = (size_t)(blkOff[g + 1] - blkOff[g]);
    const u32 c = f == FD_NONE ? 2u : codecs[f];
    szF[g] = c == 0 ? n : 0; szH[g] = c == 1 ? n : 0;
}
// GIVEN, behind the two coders: cres[g] (the FSE coder's) becomes the result of the block's owner, pos[g] the length of its record (k_fw_lens)
__global__ void k_fm_lens(u64* pos, size_t* cres, const size_t* cresH, const u64* blkOff, const u32* blkFrame, const u8* codecs, size_t maxBlocks, u32 bsLog)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= maxBlocks) return;
    u64 len = 0;
    const u32 f = blkFrame[g];
    if (f != FD_NONE) {
        size_t r = cres[g];
        if (codecs[f] == 1) { r = cresH[g]; cres[g] = r; }
        if (!is_err(r)) {
            const u64 n = blkOff[g + 1] - blkOff[g];
            len = (n == ((u64)1 << bsLog) ? 1u : 3u) + (r == 0 ? n : r == 1 ? 1u : 2u + (u64)r);
        }
    }
    pos[g] = len;
}
// GIVEN: k_fw_sizes, and GENERIC for a frame whose codec byte names no coder
__global__ void k_fm_sizes(size_t* fsize, u64* slots, const u64* first, const u64* pos, const size_t* cres, const u8* codecs, size_t nFrames, size_t maxBlocks, u32 alignLog)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    const size_t r = codecs[f] > 1 ? FERR(GENERIC) : fw_result(first[f], first[f + 1], pos, cres, maxBlocks);
    fsize[f] = r;
    const u64 a = ((u64)1 << alignLog) - 1;
    slots[f] = is_err(r) ? 0 : ((u64)r + a) & ~a;
}
// what one coder left of every block: record positions (scanned), results, slots
struct FmSet { const u64* pos; const size_t* cres; const u8* slots; };
// CHOOSE, per frame: F and H, the sizes of its FSE and its Huff0 frame (fw_result); Huff0 iff H * 1000 <= F * (1000 + tol); an error on
// one side takes the other, on both sides codec 0 and F's error.  The codec is an OUTPUT; fsize and slots as k_fw_sizes leaves them.
__global__ void k_fm_choose(u8* codecs, size_t* fsize, u64* slots, const u64* first, FmSet F, FmSet H, size_t nFrames, size_t maxBlocks, u32 tol, u32 alignLog)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    const size_t rF = fw_result(first[f], first[f + 1], F.pos, F.cres, maxBlocks), rH = fw_result(first[f], first[f + 1], H.pos, H.cres, maxBlocks);
    bool huf;
    if (is_err(rH)) huf = false;
    else if (is_err(rF)) huf = true;
    else huf = (u64)rH * 1000u <= (u64)rF * (u64)(1000u + tol);
    const size_t r = huf ? rH : rF;
    codecs[f] = huf ? 1 : 0;
    fsize[f] = r;
    const u64 a = ((u64)1 << alignLog) - 1;
    slots[f] = is_err(r) ? 0 : ((u64)r + a) & ~a;
}
// k_fw_place with the magic of the frame's own codec
__global__ void k_fm_place(u8* dst, const u64* dstOff, size_t* results, const size_t* fsize, const u32* hashes, const u8* codecs, size_t nFrames, u32 bsid)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    size_t r = fsize[f];
    if (!is_err(r)) {
        if (dstOff[f + 1] - dstOff[f] < (u64)r) r = FERR(dstSize_tooSmall);
        else if (dst) fw_ends(dst + dstOff[f], r, hashes[f], bsid, (int)codecs[f]);
    }
    results[f] = r;
}
// k_fw_assemble with the block's record taken from the set of its frame's codec (GIVEN: both sets are the one there is)
__global__ __launch_bounds__(FD_THREADS) void k_fm_assemble(u8* dst, const u64* dstOff, const size_t* results, const u8* src, const u64* blkOff, const u32* blkFrame,
                                                            const u64* first, FmSet F, FmSet H, const u8* codecs, size_t slotStride, u32 bsLog)
{
    const size_t g = blockIdx.x;
    const u32 f = blkFrame[g];
    if (f == FD_NONE || is_err(results[f])) return;              // uniform
    const FmSet S = codecs[f] == 1 ? H : F;
    const u32 tid = threadIdx.x;
    const u64 n = blkOff[g + 1] - blkOff[g];
    const size_t r = S.cres[g];
    const u32 bt = r == 0 ? BT_RAW : r == 1 ? BT_RLE : BT_COMPRESSED;
    const bool full = n == ((u64)1 << bsLog);
    u8* out = dst + dstOff[f] + 5 + (S.pos[g] - S.pos[first[f]]);
    const u32 hdr = (full ? 1u : 3u) + (bt == BT_COMPRESSED ? 2u : 0u);
    if (tid == 0) {
        u32 o = 0;
        if (full) out[o++] = (u8)((bt << 6) + 0x20);
        else { out[o++] = (u8)(bt << 6); out[o++] = (u8)(n >> 8); out[o++] = (u8)n; }
        if (bt == BT_COMPRESSED) { out[o++] = (u8)(r >> 8); out[o++] = (u8)r; }
        else if (bt == BT_RLE) out[o] = src[blkOff[g]];
    }
    if (bt == BT_RAW) fd_copy(out + hdr, src + blkOff[g], (size_t)n, tid, -1);
    else if (bt == BT_COMPRESSED) fd_copy(out + hdr, S.slots + g * slotStride, r, tid, -1);
}

struct FwLayout { size_t first, hashes, blkOff, blkFrame, cres, pos, partials, slots, codec, fsize, total, slotStride, codecBytes; };
// packed: the packed writer's layout -- the fixed-slot one with the frames' results behind it
FwLayout fw_layout(size_t nFrames, size_t maxBlocks, unsigned bsid, int codec, bool packed = false)
{
    FwLayout L; size_t p = 0;
    auto carve = [&](size_t bytes) { const size_t r = p; p += up256(bytes); return r; };
    const size_t bs = (size_t)1024 << bsid;
    L.slotStride = (FSEHIP_FSE_COMPRESSBOUND(bs) + 15) & ~(size_t)15;             // FSE_compressBound(inputBlockSize), fileio.c:340
    L.codecBytes = codec == 1 ? FSEHIP_HUF_compress_batch_workspaceSize(maxBlocks) : FSEHIP_FSE_compress_batch_workspaceSize(maxBlocks, FSEHIP_FSE_DEFAULT_TABLELOG);
    L.first = carve((nFrames + 1) * 8); L.hashes = carve(nFrames * 4);
    L.blkOff = carve((maxBlocks + 1) * 8); L.blkFrame = carve(maxBlocks * 4); L.cres = carve(maxBlocks * 8); L.pos = carve((maxBlocks + 1) * 8);
    L.partials = carve(scan_partials(nFrames > maxBlocks ? nFrames : maxBlocks) * 8);
    L.slots = carve(maxBlocks * L.slotStride); L.codec = carve(L.codecBytes);
    L.fsize = packed ? carve((nFrames + 1) * 8) : 0;
    L.total = p;
    return L;
}

// The mixed writer's layout: the packed writer's with the larger of the two coder workspaces (the coders run one after the other, as the
// reader's do), and behind it the Huff0 coder's results, then GIVEN: the two size arrays; CHOOSE: the Huff0 coder's record positions and slots.
struct FmLayout { FwLayout w; size_t szF, szH, cres2, pos2, slots2, total; };
FmLayout fm_layout(size_t nFrames, size_t maxBlocks, unsigned bsid, int policy)
{
    FmLayout L;
    const FwLayout a = fw_layout(nFrames, maxBlocks, bsid, 0, true), b = fw_layout(nFrames, maxBlocks, bsid, 1, true);
    L.w = a.codecBytes >= b.codecBytes ? a : b;
    size_t p = L.w.total;
    auto carve = [&](size_t bytes) { const size_t r = p; p += up256(bytes); return r; };
    L.cres2 = carve(maxBlocks * 8);
    L.szF = L.szH = L.pos2 = L.slots2 = 0;
    if (policy == FSEHIP_CODECS_GIVEN) { L.szF = carve(maxBlocks * 8); L.szH = carve(maxBlocks * 8); }
    else { L.pos2 = carve((maxBlocks + 1) * 8); L.slots2 = carve(maxBlocks * L.w.slotStride); }
    L.total = p;
    return L;
}

// =====================================================================================================
//  reader
// =====================================================================================================
struct FrFrame { size_t hard; size_t soft; u32 crc; u32 codec; u32 bsLog; u32 pad; };
// what frame_decompress_impl decides before it looks at a block (frame.hip:184-189): nothing else is reported for such a frame
DEV size_t fr_head(const u8* in, size_t srcSize, u32& codec, u32& bsLog)
{
    codec = 0; bsLog = 10;
    if (srcSize < 5 + 3) return FERR(srcSize_wrong);
    const u32 magic = ld32(in);
    if (magic == MAGIC_FSE) codec = 0; else if (magic == MAGIC_HUF) codec = 1; else return FERR(GENERIC);       // fileio.c:484-499
    if (in[4] > MAX_BSID) return FERR(GENERIC);                                                              // :502-504
    bsLog = 10 + in[4];
    return 0;
}
// the header walk (frame.hip:199-217): onBlock(type, rSize, cSize, at) for every block in front of the first structural problem or the end
// mark; returns the structural error (0: none).  Serial by format -- every header says where the next one is -- and inside [in, in + srcSize).
template <class F>
DEV size_t fr_walk(const u8* in, size_t srcSize, size_t bs, u32& crc, F onBlock)
{
    size_t ip = 5;
    crc = 0;
    for (;;) {
        if (ip >= srcSize) return FERR(srcSize_wrong);
        const u32 b0 = in[ip++];
        const u32 bt = b0 >> 6;
        size_t rSize = bs, cSize;
        if (bt == BT_CRC) {
            if (ip + 2 > srcSize) return FERR(srcSize_wrong);
            crc = in[ip + 1] + ((u32)in[ip] << 8) + ((b0 & 0x3Fu) << 16);
            return 0;
        }
        if (!(b0 & 0x20u)) { if (ip + 2 > srcSize) return FERR(srcSize_wrong); rSize = ((size_t)in[ip] << 8) + in[ip + 1]; ip += 2; }
        if (bt == BT_COMPRESSED) { if (ip + 2 > srcSize) return FERR(srcSize_wrong); cSize = ((size_t)in[ip] << 8) + in[ip + 1]; ip += 2; }
        else cSize = bt == BT_RAW ? rSize : 1;
        if (ip + cSize > srcSize) return FERR(srcSize_wrong);
        if (rSize > bs) return FERR(corruption_detected);        // the reference's buffers hold blockSize bytes (fileio.c:509-510; frame.hip:212-214)
        onBlock(bt, rSize, cSize, ip);
        ip += cSize;
    }
}
__global__ void k_fr_count(FrFrame* frames, u64* first, const u8* src, const u64* frameOff, size_t nFrames)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    const u8* const in = src + frameOff[f];
    const size_t srcSize = (size_t)(frameOff[f + 1] - frameOff[f]);
    FrFrame m; m.soft = 0; m.crc = 0; m.pad = 0;
    m.hard = fr_head(in, srcSize, m.codec, m.bsLog);
    u64 n = 0;
    if (!m.hard) m.soft = fr_walk(in, srcSize, (size_t)1 << m.bsLog, m.crc, [&](u32, size_t, size_t, size_t) { ++n; });
    frames[f] = m;
    first[f] = n;
}
// k_fr_count for frames whose regenerated sizes nobody knows: the same walk, which also sums what the blocks ANNOUNCE -- the frame's
// content bound (fsehip.h: a capacity with which the reader decides what it decides with any larger one, not the content size), rounded
// up to the slot alignment in slots[f] -- and tells what it saw (infos, may be null; frames may be null: the plan alone keeps no FrFrame).
__global__ void k_fr_plan(FrFrame* frames, u64* first, u64* slots, FSEHIP_FrameInfo* infos, const u8* src, const u64* frameOff, size_t nFrames, u32 alignLog)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    const u8* const in = src + frameOff[f];
    const size_t srcSize = (size_t)(frameOff[f + 1] - frameOff[f]);
    FrFrame m; m.soft = 0; m.crc = 0; m.pad = 0;
    m.hard = fr_head(in, srcSize, m.codec, m.bsLog);
    u64 n = 0, bound = 0;
    if (!m.hard) m.soft = fr_walk(in, srcSize, (size_t)1 << m.bsLog, m.crc, [&](u32, size_t rSize, size_t, size_t) { ++n; bound += rSize; });
    if (frames) frames[f] = m;
    first[f] = n;
    const u64 a = ((u64)1 << alignLog) - 1;
    slots[f] = (bound + a) & ~a;
    if (infos) {
        FSEHIP_FrameInfo fi;
        fi.contentBound = bound; fi.nBlocks = n;
        fi.status = (u32)(0 - (m.hard ? m.hard : m.soft));
        fi.checksum22 = m.crc;
        fi.codec = m.hard ? 0 : (u8)m.codec; fi.blockSizeId = m.hard ? 0 : (u8)(m.bsLog - 10);
        for (int k = 0; k < 6; ++k) fi.reserved[k] = 0;
        infos[f] = fi;
    }
}
// off[i] = min(off[i], cap), i < n: the slots behind the capacity become empty, the one across it short
__global__ void k_fr_clamp(u64* off, size_t n, u64 cap)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && off[i] > cap) off[i] = cap;
}
// The block table, one entry per promised block:
//   at / csize : the record's bytes in d_frames;  dpos : where the block lands in d_dst if every block before it regenerates what it announces;
//   kind       : type | inPlace << 2 (dpos + rSize fits the frame's slot: decoded / expanded there at once) | codec << 3, or FD_NONE: no block
//   fseCs / fseCap, hufCs / hufDs : the (size, capacity) the FSE and the Huff0 decoder see for this entry -- 0 where the block is not theirs
struct FrTable { u64* at; u64* dpos; u32* csize; u32* rsize; u32* kind; size_t* fseCs; size_t* fseCap; size_t* hufCs; size_t* hufDs; size_t* fseRes; size_t* hufRes; };
__global__ void k_fr_clear(FrTable t, size_t maxBlocks)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= maxBlocks) return;
    t.at[g] = 0; t.dpos[g] = 0; t.kind[g] = FD_NONE; t.fseCs[g] = 0; t.fseCap[g] = 0; t.hufCs[g] = 0; t.hufDs[g] = 0;
}
DEV bool fr_dead(const FrFrame& m, const u64* first, size_t f, size_t maxBlocks) { return first[f + 1] > first[f] && first[f + 1] > maxBlocks; }
__global__ void k_fr_fill(FrTable t, const FrFrame* frames, const u64* first, const u8* src, const u64* frameOff, const u64* dstOff, size_t nFrames, size_t maxBlocks)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    const FrFrame m = frames[f];
    if (m.hard || fr_dead(m, first, f, maxBlocks)) return;
    const u64 fo = frameOff[f], dOff = dstOff[f], cap = dstOff[f + 1] - dOff;
    u64 g = first[f], A = 0;
    u32 crc;
    (void)fr_walk(src + fo, (size_t)(frameOff[f + 1] - fo), (size_t)1 << m.bsLog, crc, [&](u32 bt, size_t rSize, size_t cSize, size_t at) {
        const bool inPlace = A + rSize <= cap;
        t.at[g] = fo + at; t.dpos[g] = dOff + (inPlace ? A : 0); t.csize[g] = (u32)cSize; t.rsize[g] = (u32)rSize;
        t.kind[g] = bt | (inPlace ? 4u : 0u) | (m.codec << 3);
        if (bt == BT_COMPRESSED && inPlace) {
            if (m.codec == 0) { t.fseCs[g] = cSize; t.fseCap[g] = rSize; }      // FSE_decompress(dst, announced size as capacity), fileio.c:570
            else { t.hufCs[g] = cSize; t.hufDs[g] = rSize; }                    // HUF_decompress(dst, announced size = exact size)
        }
        A += rSize; ++g;
    });
}
// raw and RLE blocks that fit at their announced place, one workgroup per block
__global__ __launch_bounds__(FD_THREADS) void k_fr_expand(u8* dst, FrTable t, const u8* src)
{
    const size_t g = blockIdx.x;
    const u32 k = t.kind[g];
    if (k == FD_NONE || !(k & 4u)) return;
    const u32 bt = k & 3u;
    if (bt == BT_RAW) fd_copy(dst + t.dpos[g], src + t.at[g], t.rsize[g], threadIdx.x, -1);
    else if (bt == BT_RLE) fd_copy(dst + t.dpos[g], nullptr, t.rsize[g], threadIdx.x, (int)src[t.at[g]]);
}
// FSE_decompress (lib/fse_decompress.c:255-283) by ONE lane, tables in LDS: for the blocks of a frame that the batch decoder could not
// place (k_fr_settle).  Literal: FSE_readNCount (ncount_reader.h), FSE_buildDTable (:71-126), FSE_decompress_usingDTable (:178-243).
DEV size_t fse_decompress_lane(u8* out, size_t cap, const u8* in, size_t cSize, u32* cells, u16* symNext, s16* norm)
{
    u32 tl = 0, maxSV = 255;
    const size_t h = ncount_read<1>(norm, &maxSV, &tl, in, cSize);
    if (is_err(h)) return h;
    if (tl > FSEHIP_FSE_MAX_TABLELOG) return FERR(tableLog_tooLarge);
    const u32 ts = 1u << tl, mask = ts - 1;
    u32 high = ts - 1;
    bool fast = true;
    for (u32 s = 0; s <= maxSV; ++s) {
        if (norm[s] == -1) { cells[high--] = s << 16; symNext[s] = 1; }
        else { if (norm[s] >= (s16)(1 << (tl - 1))) fast = false; symNext[s] = (u16)norm[s]; }
    }
    {   const u32 step = (ts >> 1) + (ts >> 3) + 3;
        u32 position = 0;
        for (u32 s = 0; s <= maxSV; ++s)
            for (int i = 0; i < norm[s]; ++i) {
                cells[position] = s << 16;
                position = (position + step) & mask;
                while (position > high) position = (position + step) & mask;
            }
        if (position != 0) return FERR(GENERIC);
    }
    for (u32 u = 0; u < ts; ++u) {
        const u32 sym = (cells[u] >> 16) & 0xFFu;
        const u32 next = symNext[sym]++;
        const u32 nb = tl - hibit32(next);
        cells[u] = (((next << nb) - ts) & 0xFFFFu) | (sym << 16) | (nb << 24);
    }
    BitReader r;
    {   const size_t e = r.init(in + h, cSize - h); if (is_err(e)) return e; }
    u32 s1 = r.read(tl); r.reload();
    u32 s2 = r.read(tl); r.reload();
    long op = 0; const long omax = (long)cap;
    for (;;) {                                                   // :201-218
        const int st = r.reload();
        if (!((st == BR_UNFINISHED) & (op < omax - 3))) break;
        out[op] = (u8)fse_step(s1, r, cells, fast); out[op + 1] = (u8)fse_step(s2, r, cells, fast);
        out[op + 2] = (u8)fse_step(s1, r, cells, fast); out[op + 3] = (u8)fse_step(s2, r, cells, fast);
        op += 4;
    }
    for (;;) {                                                   // :222-235
        if (op > omax - 2) return FERR(dstSize_tooSmall);
        out[op++] = (u8)fse_step(s1, r, cells, fast);
        if (r.reload() == BR_OVERFLOW) { out[op++] = (u8)fse_step(s2, r, cells, fast); return (size_t)op; }
        if (op > omax - 2) return FERR(dstSize_tooSmall);
        out[op++] = (u8)fse_step(s2, r, cells, fast);
        if (r.reload() == BR_OVERFLOW) { out[op++] = (u8)fse_step(s1, r, cells, fast); return (size_t)op; }
    }
}
// Per frame, by one lane: the reader's walk over the block results (frame.hip:325-338) -- per block dstSize_tooSmall before its decoding
// error, blocks back to back by what they really regenerated, then the structural error.  A Huff0 block regenerates its announced size or
// fails; an FSE block may regenerate LESS (its announced size is only a capacity).  From such a block on the frame takes the slow way:
// every later block is moved down from its announced place -- or, if it did not fit there, regenerated now at its real place (raw / RLE
// from the frame; FSE by fse_decompress_lane).  Moves go downwards in block order, so nothing still needed is overwritten.
__global__ __launch_bounds__(64) void k_fr_settle(u8* dst, FrTable t, const FrFrame* frames, const u64* first, const u8* src, const u64* dstOff,
                                                  size_t* verdict, u64* olen, size_t nFrames, size_t maxBlocks)
{
    __shared__ u32 cells[1 << FSEHIP_FSE_MAX_TABLELOG];
    __shared__ u16 symNext[256];
    __shared__ s16 norm[256];
    const size_t f = blockIdx.x;
    if (threadIdx.x != 0) return;
    const FrFrame m = frames[f];
    olen[f] = 0;
    if (m.hard) { verdict[f] = m.hard; return; }
    if (fr_dead(m, first, f, maxBlocks)) { verdict[f] = FERR(GENERIC); return; }              // beyond the caller's promise
    const u64 cap = dstOff[f + 1] - dstOff[f];
    u8* const base = dst + dstOff[f];
    u64 o = 0, A = 0;
    size_t res = 0;
    for (u64 g = first[f]; g < first[f + 1]; ++g) {
        const u32 k = t.kind[g], bt = k & 3u;
        const bool inPlace = (k & 4u) != 0;
        const size_t rSize = t.rsize[g];
        if (o + rSize > cap) { res = FERR(dstSize_tooSmall); break; }
        if (bt == BT_COMPRESSED) {
            size_t r;
            if (inPlace) r = m.codec ? t.hufRes[g] : t.fseRes[g];
            else if (m.codec) r = FERR(GENERIC);                 // (not reached: a Huff0 frame has o == A, and A + rSize > cap was reported above)
            else r = fse_decompress_lane(base + o, rSize, src + t.at[g], t.csize[g], cells, symNext, norm);
            if (is_err(r)) { res = r; break; }                   // fileio.c:571-572
            if (inPlace && o != A) for (size_t i = 0; i < r; ++i) base[o + i] = base[A + i];
            o += r;
        } else {
            if (!inPlace || o != A) {
                const u8* const in = src + t.at[g];
                if (bt == BT_RAW) for (size_t i = 0; i < rSize; ++i) base[o + i] = in[i];
                else { const u8 v = in[0]; for (size_t i = 0; i < rSize; ++i) base[o + i] = v; }
            }
            o += rSize;
        }
        A += rSize;
    }
    if (!res) res = m.soft;
    verdict[f] = res;
    if (!res) olen[f] = o;
}
__global__ void k_fr_final(size_t* results, const size_t* verdict, const u64* olen, const u32* hashes, const FrFrame* frames, size_t nFrames)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nFrames) return;
    size_t r = verdict[f];
    if (!r) r = ((hashes[f] >> 5) & ((1u << 22) - 1)) != frames[f].crc ? FERR(corruption_detected) : (size_t)olen[f];    // fileio.c:604-607
    results[f] = r;
}

// the decoders go over the table in chunks of FR_CHUNK entries (their workspaces: 13 KB and 8 KB per entry)
#define FR_CHUNK ((size_t)32768)
struct FrLayout { size_t frames, first, hashes, verdict, olen, at, dpos, csize, rsize, kind, fseCs, fseCap, hufCs, hufDs, fseRes, hufRes, partials, codec, total, codecBytes; };
FrLayout fr_layout(size_t nFrames, size_t maxBlocks)
{
    FrLayout L; size_t p = 0;
    auto carve = [&](size_t bytes) { const size_t r = p; p += up256(bytes); return r; };
    const size_t chunk = maxBlocks < FR_CHUNK ? maxBlocks : FR_CHUNK;
    const size_t a = FSEHIP_FSE_decompress_batch_workspaceSize(chunk, FSEHIP_FSE_MAX_TABLELOG), b = FSEHIP_HUF_decompress_batch_workspaceSize(chunk);
    L.codecBytes = a > b ? a : b;
    L.frames = carve(nFrames * sizeof(FrFrame)); L.first = carve((nFrames + 1) * 8); L.hashes = carve(nFrames * 4); L.verdict = carve(nFrames * 8); L.olen = carve(nFrames * 8);
    L.at = carve(maxBlocks * 8); L.dpos = carve(maxBlocks * 8); L.csize = carve(maxBlocks * 4); L.rsize = carve(maxBlocks * 4); L.kind = carve(maxBlocks * 4);
    L.fseCs = carve(maxBlocks * 8); L.fseCap = carve(maxBlocks * 8); L.hufCs = carve(maxBlocks * 8); L.hufDs = carve(maxBlocks * 8);
    L.fseRes = carve(maxBlocks * 8); L.hufRes = carve(maxBlocks * 8);
    L.partials = carve(scan_partials(nFrames) * 8);
    L.codec = carve(L.codecBytes);
    L.total = p;
    return L;
}
struct FpLayout { size_t first, partials, total; };
FpLayout fp_layout(size_t nFrames)
{
    FpLayout L; size_t p = 0;
    auto carve = [&](size_t bytes) { const size_t r = p; p += up256(bytes); return r; };
    L.first = carve((nFrames + 1) * 8); L.partials = carve(scan_partials(nFrames) * 8);
    L.total = p;
    return L;
}
}   // namespace

#define CKE(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
#define CKI(x) do { const int e_ = (x); if (e_ != 0) return e_; } while (0)

hipError_t launch_xxh32(u32* hashes, const u8* data, const u64* starts, const u64* lens, size_t nItems, u32 seed, hipStream_t s)
{
    if (nItems == 0) return hipSuccess;
    hipLaunchKernelGGL(k_xxh32, dim3((unsigned)((nItems + 15) / 16)), dim3(64), 0, s, hashes, data, starts, lens, nItems, seed);
    return hipGetLastError();
}

extern "C" int FSEHIP_XXH32_batch(uint32_t* d_hashes, const void* d_data, const uint64_t* d_offsets, size_t nItems, uint32_t seed, void* stream)
{
    return (int)launch_xxh32(d_hashes, (const u8*)d_data, (const u64*)d_offsets, nullptr, nItems, seed, (hipStream_t)stream);
}

extern "C" size_t FSEHIP_frame_blockCount(size_t srcSize, unsigned blockSizeId)
{
    if (blockSizeId > MAX_BSID) return FSEHIP_ERROR(GENERIC);
    const size_t bs = (size_t)1024 << blockSizeId;
    return srcSize / bs + (srcSize % bs ? 1 : 0);
}

extern "C" size_t FSEHIP_frame_compress_dbatch_workspaceSize(size_t nFrames, size_t maxTotalBlocks, unsigned blockSizeId, int codec)
{
    if (blockSizeId > MAX_BSID || (codec != 0 && codec != 1)) return FSEHIP_ERROR(GENERIC);
    return fw_layout(nFrames, maxTotalBlocks, blockSizeId, codec).total;
}

// the writer's first steps: block counts and their scan (`first`), the trailers' hashes, where every block starts and whose it is -- in the workspace
static int fw_blocks(const u8* src, const u64* srcOff, size_t nFrames, size_t nb, u32 bsLog, u8* ws, const FwLayout& L, hipStream_t s)
{
    u64* const first = (u64*)(ws + L.first);
    hipLaunchKernelGGL(k_fw_counts, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, first, srcOff, nFrames, bsLog);
    CKE(launch_exscan(first, nFrames, (u64*)(ws + L.partials), s));
    CKE(launch_xxh32((u32*)(ws + L.hashes), src, srcOff, nullptr, nFrames, 0, s));
    if (nb) hipLaunchKernelGGL(k_fw_blocks, dim3(grid_for(nb + 1)), dim3(FD_THREADS), 0, s, (u64*)(ws + L.blkOff), (u32*)(ws + L.blkFrame), (const u64*)first, srcOff, nFrames, nb, bsLog);
    return (int)hipGetLastError();
}
// every block of the view in one call of the one-shot coder (frame.hip:118-119: default table logs, alphabet 255, slot = capacity)
static int fw_code(int codec, u8* slots, size_t* cres, const BlockView& v, size_t nb, u8* ws, const FwLayout& L, hipStream_t s)
{
    if (codec == 1) return huf_compress_view(4, slots, L.slotStride, L.slotStride, cres, v, 255, FSEHIP_HUF_TABLELOG_DEFAULT, nb, ws + L.codec, L.codecBytes, s);
    return fse_compress_view(slots, L.slotStride, L.slotStride, cres, v, 255, FSEHIP_FSE_DEFAULT_TABLELOG, nb, ws + L.codec, L.codecBytes, s);
}
// the writer up to the record positions: fw_blocks, every block of every content through the one-shot coder into its workspace slot
// (`cres`), the records' lengths and their scan (`pos`) -- all in the workspace
static int fw_encode(const u8* src, const u64* srcOff, size_t nFrames, size_t nb, u32 bsLog, int codec, u8* ws, const FwLayout& L, hipStream_t s)
{
    u64* const blkOff = (u64*)(ws + L.blkOff);
    size_t* const cres = (size_t*)(ws + L.cres); u64* const pos = (u64*)(ws + L.pos);
    CKI(fw_blocks(src, srcOff, nFrames, nb, bsLog, ws, L, s));
    if (nb) {
        BlockView v; v.base = src; v.stride = 0; v.sizes = nullptr; v.uniform = 0; v.offsets = blkOff;
        CKI(fw_code(codec, ws + L.slots, cres, v, nb, ws, L, s));
        hipLaunchKernelGGL(k_fw_lens, dim3(grid_for(nb)), dim3(FD_THREADS), 0, s, pos, (const size_t*)cres, (const u64*)blkOff, (const u32*)(ws + L.blkFrame), nb, bsLog);
        CKE(launch_exscan(pos, nb, (u64*)(ws + L.partials), s));
    }
    return (int)hipGetLastError();
}
// ... and behind the frames' verdicts: every block's header and record at its place
static int fw_assemble(u8* dst, const u64* dstOff, const size_t* results, const u8* src, size_t nb, u32 bsLog, u8* ws, const FwLayout& L, hipStream_t s)
{
    if (nb) hipLaunchKernelGGL(k_fw_assemble, dim3((unsigned)nb), dim3(FD_THREADS), 0, s, dst, dstOff, results, src, (const u64*)(ws + L.blkOff), (const u32*)(ws + L.blkFrame),
                               (const u64*)(ws + L.first), (const u64*)(ws + L.pos), (const size_t*)(ws + L.cres), (const u8*)(ws + L.slots), L.slotStride, bsLog);
    return (int)hipGetLastError();
}

extern "C" int FSEHIP_frame_compress_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_src, const uint64_t* d_srcOffsets,
                                            size_t nFrames, size_t maxTotalBlocks, unsigned blockSizeId, int codec,
                                            void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (blockSizeId > MAX_BSID || (codec != 0 && codec != 1)) return (int)hipErrorInvalidValue;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (nFrames == 0) return 0;
    if (maxTotalBlocks >= ((size_t)1 << 31) || nFrames >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;       // (launch grids, 32-bit frame indices)
    const FwLayout L = fw_layout(nFrames, maxTotalBlocks, blockSizeId, codec);
    if (workspaceBytes < L.total) return (int)hipErrorInvalidValue;
    u8* const ws = (u8*)d_workspace;
    const u64* const srcOff = (const u64*)d_srcOffsets; const u64* const dstOff = (const u64*)d_dstOffsets;
    const u32 bsLog = 10 + blockSizeId;
    const size_t nb = maxTotalBlocks;
    CKI(fw_encode((const u8*)d_src, srcOff, nFrames, nb, bsLog, codec, ws, L, s));
    hipLaunchKernelGGL(k_fw_verdict, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, (u8*)d_dst, dstOff, d_results, srcOff, (const u64*)(ws + L.first), (const u64*)(ws + L.pos),
                       (const size_t*)(ws + L.cres), (const u32*)(ws + L.hashes), nFrames, nb, blockSizeId, codec);
    return fw_assemble((u8*)d_dst, dstOff, (const size_t*)d_results, (const u8*)d_src, nb, bsLog, ws, L, s);
}

extern "C" size_t FSEHIP_frame_packedBound(size_t totalSrcBytes, size_t nFrames, size_t totalBlocks, unsigned slotAlignLog)
{
    if (slotAlignLog > 12) return FSEHIP_ERROR(GENERIC);
    return totalSrcBytes + 8 * nFrames + 5 * totalBlocks + nFrames * (((size_t)1 << slotAlignLog) - 1);
}

extern "C" size_t FSEHIP_frame_compress_packed_dbatch_workspaceSize(size_t nFrames, size_t maxTotalBlocks, unsigned blockSizeId, int codec)
{
    if (blockSizeId > MAX_BSID || (codec != 0 && codec != 1)) return FSEHIP_ERROR(GENERIC);
    return fw_layout(nFrames, maxTotalBlocks, blockSizeId, codec, true).total;
}

extern "C" int FSEHIP_frame_compress_packed_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_dstOffsets, size_t* d_results, const void* d_src,
                                                   const uint64_t* d_srcOffsets, size_t nFrames, size_t maxTotalBlocks, unsigned blockSizeId, int codec,
                                                   unsigned slotAlignLog, void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (blockSizeId > MAX_BSID || (codec != 0 && codec != 1) || slotAlignLog > 12) return (int)hipErrorInvalidValue;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (maxTotalBlocks >= ((size_t)1 << 31) || nFrames >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const FwLayout L = fw_layout(nFrames, maxTotalBlocks, blockSizeId, codec, true);
    if (workspaceBytes < L.total) return (int)hipErrorInvalidValue;
    u8* const ws = (u8*)d_workspace;
    const u64* const srcOff = (const u64*)d_srcOffsets; u64* const dstOff = (u64*)d_dstOffsets;
    size_t* const fsize = (size_t*)(ws + L.fsize);
    const u32 bsLog = 10 + blockSizeId;
    const size_t nb = maxTotalBlocks;
    if (nFrames) {
        CKI(fw_encode((const u8*)d_src, srcOff, nFrames, nb, bsLog, codec, ws, L, s));
        hipLaunchKernelGGL(k_fw_sizes, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, fsize, dstOff, (const u64*)(ws + L.first), (const u64*)(ws + L.pos),
                           (const size_t*)(ws + L.cres), nFrames, nb, (u32)slotAlignLog);
    }
    CKE(launch_exscan(dstOff, nFrames, (u64*)(ws + L.partials), s));
    hipLaunchKernelGGL(k_fr_clamp, dim3(grid_for(nFrames + 1)), dim3(FD_THREADS), 0, s, dstOff, nFrames + 1, (u64)dstCapacity);
    CKE(hipGetLastError());
    if (nFrames == 0) return 0;
    hipLaunchKernelGGL(k_fw_place, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, (u8*)d_dst, (const u64*)dstOff, d_results, (const size_t*)fsize,
                       (const u32*)(ws + L.hashes), nFrames, blockSizeId, codec);
    if (!d_dst) return (int)hipGetLastError();               // the sizing query: offsets and results, no frame
    return fw_assemble((u8*)d_dst, (const u64*)dstOff, (const size_t*)d_results, (const u8*)d_src, nb, bsLog, ws, L, s);
}

extern "C" size_t FSEHIP_frame_mixedWorkspaceBound(size_t nFrames, size_t maxTotalBlocks, unsigned blockSizeId, int policy)
{
    if (blockSizeId > MAX_BSID || (policy != FSEHIP_CODECS_GIVEN && policy != FSEHIP_CODECS_CHOOSE)) return FSEHIP_ERROR(GENERIC);
    return fm_layout(nFrames, maxTotalBlocks, blockSizeId, policy).total;
}

extern "C" int FSEHIP_frame_compress_packed_mixed_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_dstOffsets, size_t* d_results, const void* d_src,
                                                         const uint64_t* d_srcOffsets, size_t nFrames, size_t maxTotalBlocks, unsigned blockSizeId,
                                                         uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog,
                                                         void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const bool choose = policy == FSEHIP_CODECS_CHOOSE;
    if (blockSizeId > MAX_BSID || (!choose && policy != FSEHIP_CODECS_GIVEN) || slotAlignLog > 12 || !d_codecs) return (int)hipErrorInvalidValue;
    if (choose && tolerancePermille > 1000) return (int)hipErrorInvalidValue;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (maxTotalBlocks >= ((size_t)1 << 31) || nFrames >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const FmLayout M = fm_layout(nFrames, maxTotalBlocks, blockSizeId, policy);
    if (workspaceBytes < M.total) return (int)hipErrorInvalidValue;
    const FwLayout& L = M.w;
    u8* const ws = (u8*)d_workspace;
    const u8* const src = (const u8*)d_src;
    const u64* const srcOff = (const u64*)d_srcOffsets; u64* const dstOff = (u64*)d_dstOffsets;
    const u64* const first = (const u64*)(ws + L.first); const u64* const blkOff = (const u64*)(ws + L.blkOff); const u32* const blkFrame = (const u32*)(ws + L.blkFrame);
    size_t* const cres = (size_t*)(ws + L.cres); size_t* const cres2 = (size_t*)(ws + M.cres2);
    u64* const pos = (u64*)(ws + L.pos); u64* const partials = (u64*)(ws + L.partials);
    size_t* const fsize = (size_t*)(ws + L.fsize);
    const u32 bsLog = 10 + blockSizeId;
    const size_t nb = maxTotalBlocks;
    FmSet F, H;
    F.pos = pos; F.cres = cres; F.slots = ws + L.slots;
    H = F;
    if (choose) { H.pos = (const u64*)(ws + M.pos2); H.cres = cres2; H.slots = ws + M.slots2; }
    if (nFrames) {
        CKI(fw_blocks(src, srcOff, nFrames, nb, bsLog, ws, L, s));
        BlockView v; v.base = src; v.stride = 0; v.sizes = nullptr; v.uniform = 0; v.offsets = blkOff;
        if (nb && !choose) {
            size_t* const szF = (size_t*)(ws + M.szF); size_t* const szH = (size_t*)(ws + M.szH);
            hipLaunchKernelGGL(k_fm_route, dim3(grid_for(nb)), dim3(FD_THREADS), 0, s, szF, szH, blkOff, blkFrame, (const u8*)d_codecs, nb);
            CKE(hipGetLastError());
            v.sizes = szF; CKI(fw_code(0, ws + L.slots, cres, v, nb, ws, L, s));
            v.sizes = szH; CKI(fw_code(1, ws + L.slots, cres2, v, nb, ws, L, s));
            hipLaunchKernelGGL(k_fm_lens, dim3(grid_for(nb)), dim3(FD_THREADS), 0, s, pos, cres, (const size_t*)cres2, blkOff, blkFrame, (const u8*)d_codecs, nb, bsLog);
            CKE(launch_exscan(pos, nb, partials, s));
        } else if (nb) {
            u64* const pos2 = (u64*)(ws + M.pos2);
            CKI(fw_code(0, ws + L.slots, cres, v, nb, ws, L, s));
            CKI(fw_code(1, ws + M.slots2, cres2, v, nb, ws, L, s));
            hipLaunchKernelGGL(k_fw_lens, dim3(grid_for(nb)), dim3(FD_THREADS), 0, s, pos, (const size_t*)cres, blkOff, blkFrame, nb, bsLog);
            CKE(launch_exscan(pos, nb, partials, s));
            hipLaunchKernelGGL(k_fw_lens, dim3(grid_for(nb)), dim3(FD_THREADS), 0, s, pos2, (const size_t*)cres2, blkOff, blkFrame, nb, bsLog);
            CKE(launch_exscan(pos2, nb, partials, s));
        }
        if (choose) hipLaunchKernelGGL(k_fm_choose, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, (u8*)d_codecs, fsize, dstOff, first, F, H, nFrames, nb,
                                       (u32)tolerancePermille, (u32)slotAlignLog);
        else hipLaunchKernelGGL(k_fm_sizes, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, fsize, dstOff, first, (const u64*)pos, (const size_t*)cres, (const u8*)d_codecs,
                                nFrames, nb, (u32)slotAlignLog);
    }
    CKE(launch_exscan(dstOff, nFrames, partials, s));
    hipLaunchKernelGGL(k_fr_clamp, dim3(grid_for(nFrames + 1)), dim3(FD_THREADS), 0, s, dstOff, nFrames + 1, (u64)dstCapacity);
    CKE(hipGetLastError());
    if (nFrames == 0) return 0;
    hipLaunchKernelGGL(k_fm_place, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, (u8*)d_dst, (const u64*)dstOff, d_results, (const size_t*)fsize,
                       (const u32*)(ws + L.hashes), (const u8*)d_codecs, nFrames, blockSizeId);
    if (d_dst && nb) hipLaunchKernelGGL(k_fm_assemble, dim3((unsigned)nb), dim3(FD_THREADS), 0, s, (u8*)d_dst, (const u64*)dstOff, (const size_t*)d_results, src, blkOff, blkFrame,
                                        first, F, H, (const u8*)d_codecs, L.slotStride, bsLog);
    return (int)hipGetLastError();
}

extern "C" size_t FSEHIP_frame_decompress_dbatch_workspaceSize(size_t nFrames, size_t maxTotalBlocks) { return fr_layout(nFrames, maxTotalBlocks).total; }

// the reader behind its header walk and first scan: `frames` and `first` (scanned) are in the workspace, dstOff in device memory
static int fr_decode(void* d_dst, const u64* dstOff, size_t* d_results, const u8* src, const u64* frameOff, size_t nFrames, size_t nb, u8* ws, const FrLayout& L, hipStream_t s)
{
    FrFrame* const frames = (FrFrame*)(ws + L.frames); u64* const first = (u64*)(ws + L.first); u32* const hashes = (u32*)(ws + L.hashes);
    size_t* const verdict = (size_t*)(ws + L.verdict); u64* const olen = (u64*)(ws + L.olen);
    FrTable t;
    t.at = (u64*)(ws + L.at); t.dpos = (u64*)(ws + L.dpos); t.csize = (u32*)(ws + L.csize); t.rsize = (u32*)(ws + L.rsize); t.kind = (u32*)(ws + L.kind);
    t.fseCs = (size_t*)(ws + L.fseCs); t.fseCap = (size_t*)(ws + L.fseCap); t.hufCs = (size_t*)(ws + L.hufCs); t.hufDs = (size_t*)(ws + L.hufDs);
    t.fseRes = (size_t*)(ws + L.fseRes); t.hufRes = (size_t*)(ws + L.hufRes);
    if (nb) {
        hipLaunchKernelGGL(k_fr_clear, dim3(grid_for(nb)), dim3(FD_THREADS), 0, s, t, nb);
        hipLaunchKernelGGL(k_fr_fill, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, t, (const FrFrame*)frames, (const u64*)first, src, frameOff, dstOff, nFrames, nb);
        CKE(hipGetLastError());
        // compressed blocks where they lie, (offset, size) pairs; destinations by offset.  An entry that is not the decoder's has size 0 and
        // capacity 0: an error result nobody reads, nothing written.
        for (size_t b0 = 0; b0 < nb; b0 += FR_CHUNK) {
            const size_t n = nb - b0 < FR_CHUNK ? nb - b0 : FR_CHUNK;
            BlockView v; v.base = src; v.stride = 0; v.uniform = 0; v.offsets = t.at + b0;
            v.sizes = t.fseCs + b0;
            CKI(fse_decompress_view(d_dst, t.dpos + b0, t.fseCap + b0, t.fseRes + b0, v, FSEHIP_FSE_MAX_TABLELOG, n, ws + L.codec, L.codecBytes, s));
            v.sizes = t.hufCs + b0;
            CKI(huf_decompress_view(d_dst, t.dpos + b0, t.hufDs + b0, t.hufRes + b0, v, n, ws + L.codec, L.codecBytes, s));
        }
        hipLaunchKernelGGL(k_fr_expand, dim3((unsigned)nb), dim3(FD_THREADS), 0, s, (u8*)d_dst, t, src);
    }
    hipLaunchKernelGGL(k_fr_settle, dim3((unsigned)nFrames), dim3(64), 0, s, (u8*)d_dst, t, (const FrFrame*)frames, (const u64*)first, src, dstOff, verdict, olen, nFrames, nb);
    CKE(hipGetLastError());
    CKE(launch_xxh32(hashes, (const u8*)d_dst, dstOff, (const u64*)olen, nFrames, 0, s));
    hipLaunchKernelGGL(k_fr_final, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, d_results, (const size_t*)verdict, (const u64*)olen, (const u32*)hashes,
                       (const FrFrame*)frames, nFrames);
    return (int)hipGetLastError();
}

extern "C" int FSEHIP_frame_decompress_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets,
                                              size_t nFrames, size_t maxTotalBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (nFrames == 0) return 0;
    if (maxTotalBlocks >= ((size_t)1 << 31) || nFrames >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const FrLayout L = fr_layout(nFrames, maxTotalBlocks);
    if (workspaceBytes < L.total) return (int)hipErrorInvalidValue;
    u8* const ws = (u8*)d_workspace;
    FrFrame* const frames = (FrFrame*)(ws + L.frames); u64* const first = (u64*)(ws + L.first); u64* const partials = (u64*)(ws + L.partials);
    const u8* const src = (const u8*)d_frames;
    const u64* const frameOff = (const u64*)d_frameOffsets;

    hipLaunchKernelGGL(k_fr_count, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, frames, first, src, frameOff, nFrames);
    CKE(launch_exscan(first, nFrames, partials, s));
    return fr_decode(d_dst, (const u64*)d_dstOffsets, d_results, src, frameOff, nFrames, maxTotalBlocks, ws, L, s);
}

// k_fr_plan, the scan of the slots (in place in dstOff: nFrames + 1 entries) and of the block counts, the clamp
static int fr_plan(FrFrame* frames, u64* first, u64* dstOff, FSEHIP_FrameInfo* infos, const u8* src, const u64* frameOff, size_t nFrames, u64 dstCapacity,
                   unsigned alignLog, u64* partials, hipStream_t s)
{
    if (nFrames) hipLaunchKernelGGL(k_fr_plan, dim3(grid_for(nFrames)), dim3(FD_THREADS), 0, s, frames, first, dstOff, infos, src, frameOff, nFrames, (u32)alignLog);
    CKE(launch_exscan(dstOff, nFrames, partials, s));
    CKE(launch_exscan(first, nFrames, partials, s));
    hipLaunchKernelGGL(k_fr_clamp, dim3(grid_for(nFrames + 1)), dim3(FD_THREADS), 0, s, dstOff, nFrames + 1, dstCapacity);
    return (int)hipGetLastError();
}

extern "C" size_t FSEHIP_frame_plan_dbatch_workspaceSize(size_t nFrames) { return fp_layout(nFrames).total; }

extern "C" int FSEHIP_frame_plan_dbatch(uint64_t* d_dstOffsets, uint64_t* d_blockFirst, FSEHIP_FrameInfo* d_infos, const void* d_frames, const uint64_t* d_frameOffsets,
                                        size_t nFrames, uint64_t dstCapacity, unsigned slotAlignLog, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (slotAlignLog > 12 || ((uintptr_t)d_workspace & 255u) || nFrames >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const FpLayout L = fp_layout(nFrames);
    if (workspaceBytes < L.total) return (int)hipErrorInvalidValue;
    u8* const ws = (u8*)d_workspace;
    u64* const first = d_blockFirst ? (u64*)d_blockFirst : (u64*)(ws + L.first);
    return fr_plan(nullptr, first, (u64*)d_dstOffsets, d_infos, (const u8*)d_frames, (const u64*)d_frameOffsets, nFrames, dstCapacity, slotAlignLog,
                   (u64*)(ws + L.partials), (hipStream_t)stream);
}

extern "C" size_t FSEHIP_frame_decompress_packed_dbatch_workspaceSize(size_t nFrames, size_t maxTotalBlocks) { return fr_layout(nFrames, maxTotalBlocks).total; }

extern "C" int FSEHIP_frame_decompress_packed_dbatch(void* d_dst, size_t dstCapacity, uint64_t* d_dstOffsets, size_t* d_results, const void* d_frames,
                                                     const uint64_t* d_frameOffsets, size_t nFrames, size_t maxTotalBlocks, unsigned slotAlignLog,
                                                     void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (slotAlignLog > 12 || ((uintptr_t)d_workspace & 255u)) return (int)hipErrorInvalidValue;
    if (maxTotalBlocks >= ((size_t)1 << 31) || nFrames >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const FrLayout L = fr_layout(nFrames, maxTotalBlocks);
    if (workspaceBytes < L.total) return (int)hipErrorInvalidValue;
    u8* const ws = (u8*)d_workspace;
    const u8* const src = (const u8*)d_frames;
    const u64* const frameOff = (const u64*)d_frameOffsets;
    CKI(fr_plan((FrFrame*)(ws + L.frames), (u64*)(ws + L.first), (u64*)d_dstOffsets, nullptr, src, frameOff, nFrames, (u64)dstCapacity, slotAlignLog,
                (u64*)(ws + L.partials), s));
    if (nFrames == 0) return 0;
    return fr_decode(d_dst, (const u64*)d_dstOffsets, d_results, src, frameOff, nFrames, maxTotalBlocks, ws, L, s);
}

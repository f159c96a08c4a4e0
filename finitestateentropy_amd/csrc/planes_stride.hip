// planes_stride.hip -- STRIDED PREDICTED PLANES (fsehip.h, "strided predicted planes"): the planes of z[j] = zigzag(t[j] - t[j - S]), the
// predecessor S elements back -- the same channel of interleaved data (stereo samples, RGB pixels, xyz coordinates, boxes, complex pairs) --
// and taken as 0 for the first S elements of every RUN of 1024 elements.  Runs are those of planes_pred.hip, counted from the tensor's start
// whatever S is; the chain an element belongs to is ((j mod 1024) mod S) and starts again with every run.  No frame byte differs: ordinary
// .fse frames of the planes of z, the caller carries the stride as it carries the predictor.  Kernel launches only.
//
//   FSEHIP_planes_split_pred_stride_dbatch          : k_planes_offsets (planes.hip) -> k_planes_split_pred_stride
//   FSEHIP_planes_merge_pred_stride_dbatch          : k_planes_verdicts (planes.hip) -> k_planes_merge_pred_stride
//   FSEHIP_tensor_compress_pred_stride_dbatch       : the strided split -> the packed (mixed) writer           (planes_compress of planes.hip)
//   FSEHIP_tensor_compress_seg_pred_stride_dbatch   : the strided split -> the segments kernel -> the writer   (the same)
//   FSEHIP_tensor_decompress_pred_stride_dbatch     : the packed reader into the planes buffer -> the strided merge
//   FSEHIP_tensor_decompress_seg_pred_stride_dbatch : the packed reader -> the fold (planes_seg.hip) -> the strided merge
// stride == 1 launches the kernels of planes_pred.hip: the six _pred_ calls are these with stride 1.
//
// THE SPLIT is k_planes_split_pred with the predecessors S elements back: the chunk moved up by S elements in registers behind the S
// elements in front of it (ps_prev), which are 0 where the chunk starts a run -- a run starts only where a chunk does and S <= 16, so the
// S chain heads of a run are the first S elements of one chunk.  The source is only read; no scan, no workspace.
//
// THE MERGE keeps the frame of k_planes_merge_pred -- tiles relative to the tensor, one run per round of one wave, 16 elements per lane,
// whole tensor-side lines stored -- and sums S interleaved chains where that kernel sums one.  In registers and DPP only:
//   1. the lane's 16 differences one per register (ps_unpack), x[q] += x[q - S] for q = S .. 15: every chain summed inside the lane;
//   2. the lane's total of chain a is one of its last S registers, which one depends on the lane where 16 mod S != 0: element q of lane L
//      lies in chain (16 L + q) mod S.  ps_rotate brings the totals into chain order (a barrel of selects; the identity for S = 2, 4, 8);
//   3. S inclusive wave scans (dev_common.h, the DPP path) of those totals, every lane of the wave in every scan;
//   4. the exclusive results rotated back to register order and added: element q takes the carry of register q mod S.
// A lane behind the last whole element contributes zeros; the lane that holds the tensor's last, partial chunk goes element by element
// behind the scans with S running sums and copies the n mod E trailing bytes.  No LDS, no workspace, nothing crosses a wave.
#include "planes_dev.h"

namespace {
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

template <int E, int S>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split_pred_stride(u8* planes, const u8* src, const u64* SO, size_t nT, u64 capacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(SO, nT, w, i)) return;                           // (uniform, like every return below)
    const u64 s0 = SO[i], s1 = SO[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(s0 < s1) || s1 > capacity || lo >= s1 || lo + PLANES_TILE <= s0) return;
    const u64 n = s1 - s0;
    const u32 tid = threadIdx.x;
    const u8* const sb = src + s0;
    u8* const pb = planes + s0;
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

template <int E, int S>
__global__ __launch_bounds__(PL_THREADS) void k_planes_merge_pred_stride(u8* dst, const u64* D, const u8* planes, const u64* PO, const size_t* PS, size_t nT, u64 dstCapacity)
{
    typedef ps_t<E> T;
    constexpr u32 RUNS = (u32)(PLANES_TILE / E / PP_RUN);         // whole runs of a tile
    constexpr bool ROT = 16 % S != 0;                             // the chain of a register depends on the lane
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(D, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 d0 = D[i], first = (d0 >> PL_TILE_LOG) + i;
    if (first > w) return;                                        // (offsets that decrease: the search found no tensor of this item)
    const u64 t = w - first;
    const size_t v = pm_verdict(D, PS, i, E, dstCapacity);
    if (is_err(v) || (t << PL_TILE_LOG) >= (u64)v) return;        // (a good tensor: d0 + n <= D[i + 1] <= dstCapacity; t < 2^24)
    const u64 n = v, m = n / E;
    const u32 lane = threadIdx.x % WAVE;
    const u32 r0 = ROT ? (16 * lane) % S : 0;                     // register q of this lane lies in chain (r0 + q) mod S
    const u32 rEnd = ROT ? (S - (r0 + 16) % S) % S : 0;           // chain a's last element is register 16 - S + (a + rEnd) mod S
    u8* const db = dst + d0;
    const u8* pp[E];
#pragma unroll
    for (int p = 0; p < E; ++p) pp[p] = planes + PO[i * E + p];
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
#pragma unroll
            for (int k = 0; k < E; ++k) __builtin_memcpy(db + e * E + 16 * k, &wv[4 * k], 16);
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
#pragma unroll
                    for (int p = 0; p < E; ++p) db[j * E + p] = (u8)(acc[q % S] >> (8 * p));
                }
            }
            for (u64 k = m * E; k < n; ++k) db[k] = planes[PO[i * E + (k - m * E)] + m];
        }
    }
}

// the dispatch over the stride: f(std::integral_constant<int, S>) for 2 <= S <= FSEHIP_PRED_MAX_STRIDE (bad_stride has let it through)
template <class F> inline void ps_for_stride(unsigned S, F f)
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
inline bool bad_stride(unsigned stride) { return stride == 0 || stride > FSEHIP_PRED_MAX_STRIDE; }
}   // namespace

// stride 1: the kernels of planes_pred.hip.  The offsets kernel runs even for no tensors (it writes the last entry)
hipError_t launch_planes_split_pred_stride(u8* planes, u64* planeOff, size_t* tensorRes, const u8* src, const u64* srcOff, size_t nTensors, unsigned E, u64 capacity,
                                           unsigned stride, hipStream_t s)
{
    if (stride == 1) return launch_planes_split_pred(planes, planeOff, tensorRes, src, srcOff, nTensors, E, capacity, s);
    const hipError_t e0 = launch_planes_offsets(planeOff, tensorRes, srcOff, nTensors, E, capacity, s);
    if (e0 != hipSuccess || nTensors == 0 || capacity == 0) return e0;
    const dim3 g(tile_grid(capacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        ps_for_stride(stride, [&](auto sb) {
            hipLaunchKernelGGL((k_planes_split_pred_stride<decltype(eb)::value, decltype(sb)::value>), g, b, 0, s, planes, src, srcOff, nTensors, capacity);
        });
    });
    return hipGetLastError();
}

hipError_t launch_planes_merge_pred_stride(u8* dst, const u64* dstOff, size_t* results, const u8* planes, const u64* planeOff, const size_t* planeSizes, size_t nTensors,
                                           unsigned E, u64 dstCapacity, unsigned stride, hipStream_t s)
{
    if (stride == 1) return launch_planes_merge_pred(dst, dstOff, results, planes, planeOff, planeSizes, nTensors, E, dstCapacity, s);
    if (nTensors == 0) return hipSuccess;
    const hipError_t e0 = launch_planes_verdicts(results, dstOff, planeSizes, nTensors, E, dstCapacity, s);
    if (e0 != hipSuccess || dstCapacity == 0) return e0;
    const dim3 g(tile_grid(dstCapacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        ps_for_stride(stride, [&](auto sb) {
            hipLaunchKernelGGL((k_planes_merge_pred_stride<decltype(eb)::value, decltype(sb)::value>), g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, nTensors,
                               dstCapacity);
        });
    });
    return hipGetLastError();
}

extern "C" int FSEHIP_planes_split_pred_stride_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const uint64_t* d_srcOffsets,
                                                      size_t nTensors, unsigned elemBytes, uint64_t capacity, unsigned stride, void* stream)
{
    if (bad_stride(stride) || bad_elem(elemBytes) || !d_planes || !d_planeOffsets || !d_tensorResults || !d_src || !d_srcOffsets) return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(capacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_split_pred_stride((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u64*)d_srcOffsets, nTensors, elemBytes,
                                                capacity, stride, (hipStream_t)stream);
}

extern "C" int FSEHIP_planes_merge_pred_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                                      const size_t* d_planeSizes, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, unsigned stride, void* stream)
{
    if (bad_stride(stride) || bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_planes || !d_planeOffsets || !d_planeSizes)
        return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(dstCapacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_merge_pred_stride((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, nTensors,
                                                elemBytes, dstCapacity, stride, (hipStream_t)stream);
}

extern "C" int FSEHIP_tensor_compress_pred_stride_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                         const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                                         size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy,
                                                         unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets, void* d_workspace,
                                                         size_t workspaceBytes, unsigned stride, void* stream)
{
    if (bad_stride(stride) || bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_srcOffsets || !d_planeOffsets || !d_planes)
        return (int)hipErrorInvalidValue;
    return planes_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, nullptr, 0, d_srcOffsets, nTensors, elemBytes, capacity, nullptr, 0, 0,
                           d_planes, d_planeOffsets, nullptr,
                           PlWriter{ maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes }, stream, nullptr, stride);
}

extern "C" int FSEHIP_tensor_compress_seg_pred_stride_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                             const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                                             const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks, unsigned blockSizeId,
                                                             int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes,
                                                             uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace, size_t workspaceBytes, unsigned stride,
                                                             void* stream)
{
    if (bad_stride(stride) || bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_srcOffsets || !d_segFirst || !d_planeOffsets ||
        !d_segOffsets || !d_planes)
        return (int)hipErrorInvalidValue;
    return planes_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, nullptr, 0, d_srcOffsets, nTensors, elemBytes, capacity, d_segFirst,
                           nSegments, segLog, d_planes, d_planeOffsets, d_segOffsets,
                           PlWriter{ maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes }, stream, nullptr, stride);
}

// the argument checks of both steps in front of the first launch
extern "C" int FSEHIP_tensor_decompress_pred_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results, const void* d_frames,
                                                           const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks, void* d_planes,
                                                           uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults, void* d_workspace,
                                                           size_t workspaceBytes, unsigned stride, void* stream)
{
    if (bad_stride(stride) || bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_frames || !d_frameOffsets || !d_planes || !d_planeOffsets || !d_planeResults)
        return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(dstCapacity, nTensors) || bad_reader(d_workspace, workspaceBytes, nTensors * elemBytes, maxTotalBlocks))
        return (int)hipErrorInvalidValue;
    const int r = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_planeOffsets, d_planeResults, d_frames, d_frameOffsets, nTensors * elemBytes,
                                                        maxTotalBlocks, 0, d_workspace, workspaceBytes, stream);
    if (r != 0) return r;
    return (int)launch_planes_merge_pred_stride((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeResults, nTensors,
                                                elemBytes, dstCapacity, stride, (hipStream_t)stream);
}

extern "C" int FSEHIP_tensor_decompress_seg_pred_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results, const void* d_frames,
                                                               const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst,
                                                               size_t nSegments, unsigned segLog, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                                                               uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets, size_t* d_planeSizes,
                                                               void* d_workspace, size_t workspaceBytes, unsigned stride, void* stream)
{
    if (bad_stride(stride) || bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_frames || !d_frameOffsets || !d_segFirst || !d_planes || !d_segOffsets ||
        !d_segResults || !d_planeOffsets || !d_planeSizes)
        return (int)hipErrorInvalidValue;
    if (bad_seg(segLog, 0) || bad_counts(nTensors, elemBytes, nSegments) || bad_grid(dstCapacity, nTensors) || bad_reader(d_workspace, workspaceBytes, nSegments, maxTotalBlocks))
        return (int)hipErrorInvalidValue;
    const int r = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_segOffsets, d_segResults, d_frames, d_frameOffsets, nSegments, maxTotalBlocks, 0,
                                                        d_workspace, workspaceBytes, stream);
    if (r != 0) return r;
    const int f = FSEHIP_planes_fold_segments_dbatch(d_planeOffsets, d_planeSizes, d_segOffsets, d_segResults, d_segFirst, (size_t)nTensors * elemBytes, nSegments, segLog,
                                                     stream);
    if (f != 0) return f;
    return (int)launch_planes_merge_pred_stride((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, nTensors,
                                                elemBytes, dstCapacity, stride, (hipStream_t)stream);
}

// planes_pred.hip -- PREDICTED PLANES (fsehip.h, "predicted planes"): the planes of z[j] = zigzag(t[j] - t[j - 1]), the elements of a tensor
// as unsigned integers, the predecessor taken as 0 at the start of every RUN of 1024 elements.  The byte planes compress a tensor whose bytes
// are skewed at order 0; sorted indices, offsets, position ids and sampled fields are skewed only after the neighbour is subtracted.  Not
// one more op of the delta forms: the inverse is a prefix sum, not an element-wise combine.  No frame byte differs: the frames are
// ordinary .fse frames of the planes of z, and the caller carries the predictor as it carries a delta's op.  Kernel launches only.
//
//   FSEHIP_planes_split_pred_dbatch          : k_planes_offsets (planes.hip) -> k_planes_split_pred
//   FSEHIP_planes_merge_pred_dbatch          : k_planes_verdicts (planes.hip) -> k_planes_merge_pred
//   FSEHIP_tensor_compress_pred_dbatch       : the predicted split -> the packed (mixed) writer            (planes_compress of planes.hip)
//   FSEHIP_tensor_compress_seg_pred_dbatch   : the predicted split -> the segments kernel -> the writer    (the same)
//   FSEHIP_tensor_decompress_pred_dbatch     : the packed reader into the planes buffer -> the predicted merge
//   FSEHIP_tensor_decompress_seg_pred_dbatch : the packed reader -> the fold (planes_seg.hip) -> the predicted merge
// each of them the _pred_stride_ call of planes_stride.hip with stride 1, which launches the kernels of this file.
//
// THE SPLIT is k_planes_split of planes.hip -- its tile mapping over the flat byte axis, its chunks of 16 elements per lane, its E loads,
// byte shuffle and E stores -- with the chunks counted from the TENSOR's start (a chunk begins at an element index that is a multiple of
// 16, so a run begins only where a chunk does) and one more load per chunk: the element in front of it, 0 where the chunk starts a run.
// The predecessors of the other 15 elements are the chunk itself moved up by one element (v_alignbyte_b32 for E < 4, whole dwords above).
// The source is only read: no scan, no workspace, no workgroup depends on another.  Head and tail go an element per thread (pp_elem_split).
//
// THE MERGE cannot take the flat tiles: a run that two workgroups share would need a carry between them.  Its tiles are relative to the
// tensor: work item w belongs to the largest tensor i with first(i) = floor(D[i] / T) + i <= w (pl_find, the search of every mapping here)
// and takes the bytes [t T, (t + 1) T) of that tensor, t = w - first(i).  first(i + 1) - first(i) >= ceil((D[i + 1] - D[i]) / T), and
// ceil(capacity / T) + nTensors - first(nTensors - 1) >= ceil((capacity - D[nTensors - 1]) / T): every tile of every tensor that lies inside
// the capacity has its item in the launch of the plain merge's size; an item whose tile starts behind its tensor's end returns.
// A tile holds T / E / 1024 whole runs, dealt out to the workgroup's four waves; ONE RUN IS ONE ROUND OF ONE WAVE: a lane loads its 16
// elements from the E planes, interleaves and unzigzags them, sums them in registers (pp_prefix: mod 2^W per element, no carry between
// neighbours), the wave's inclusive scan of the lane totals (dev_common.h, the DPP path) gives its carry-in, and the whole tensor-side line
// -- 1024 E contiguous bytes -- is stored.  No LDS, no workspace, nothing crosses a workgroup or even a wave.  Every lane of the wave stays
// in the scan: a lane behind the last whole element contributes 0; the lane that holds the tensor's last, partial chunk goes element by
// element behind the scan and copies the n mod E trailing bytes.
#include "planes_dev.h"

namespace {
template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split_pred(u8* planes, const u8* src, const u64* S, size_t nT, u64 capacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(S, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 s0 = S[i], s1 = S[i + 1], lo = (w - i) << PL_TILE_LOG;
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
        pp_prev<E>(pv, wv, sb + e * E, (e & (PP_RUN - 1)) == 0);
#pragma unroll
        for (int k = 0; k < E; ++k) pl_sub4<E, false>(&wv[4 * k], &pv[4 * k]);
        pl_deinterleave<E>(wv, o);
#pragma unroll
        for (int p = 0; p < E; ++p) __builtin_memcpy(pb + pl_start(n, p, E) + e, o[p], 16);
    }
    const u64 nHead = h.eb - h.e0, nTail = h.e1 - h.et;
    for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) pp_elem_split<E>(pb, sb, n, j < nHead ? h.e0 + j : h.et + (j - nHead));
}

template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_merge_pred(u8* dst, const u64* D, const u8* planes, const u64* PO, const size_t* PS, size_t nT, u64 dstCapacity)
{
    constexpr u32 RUNS = (u32)(PLANES_TILE / E / PP_RUN);         // whole runs of a tile
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
    u8* const db = dst + d0;
    const u8* pp[E];
#pragma unroll
    for (int p = 0; p < E; ++p) pp[p] = planes + PO[i * E + p];
    for (u32 r = threadIdx.x / WAVE; r < RUNS; r += PL_THREADS / WAVE) {
        const u64 e0 = t * (PLANES_TILE / E) + r * PP_RUN, e = e0 + 16 * lane;
        if (e0 * E >= n) break;                                   // (uniform over the wave: the run lies behind the tensor)
        const bool full = e + 16 <= m;
        u32 wv[4 * E];
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
        u64 carry;                                                // what the lanes in front of this one add up to: all 64 lanes scan
        if constexpr (E == 8) carry = group_scan_incl_add64<64>(total, lane) - total;
        else carry = group_scan_incl<64, ScanAdd>((u32)total, lane) - (u32)total;
        if (full) {
            pp_carry<E>(wv, carry);
#pragma unroll
            for (int k = 0; k < E; ++k) __builtin_memcpy(db + e * E + 16 * k, &wv[4 * k], 16);
        } else if (e * E < n) {                                   // the tensor's last chunk: fewer than 16 whole elements, then n mod E bytes
            u64 acc = carry;
            for (u64 j = e; j < m; ++j) {
                u64 z = 0;
#pragma unroll
                for (int p = 0; p < E; ++p) z |= (u64)pp[p][j] << (8 * p);
                acc = pl_unzz<E>(z, acc);
#pragma unroll
                for (int p = 0; p < E; ++p) db[j * E + p] = (u8)(acc >> (8 * p));
            }
            for (u64 k = m * E; k < n; ++k) db[k] = planes[PO[i * E + (k - m * E)] + m];
        }
    }
}
}   // namespace

// the offsets kernel runs even for no tensors (it writes the last entry); the data kernel moves every element size
hipError_t launch_planes_split_pred(u8* planes, u64* planeOff, size_t* tensorRes, const u8* src, const u64* srcOff, size_t nTensors, unsigned E, u64 capacity,
                                    hipStream_t s)
{
    const hipError_t e0 = launch_planes_offsets(planeOff, tensorRes, srcOff, nTensors, E, capacity, s);
    if (e0 != hipSuccess || nTensors == 0 || capacity == 0) return e0;
    const dim3 g(tile_grid(capacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) { hipLaunchKernelGGL((k_planes_split_pred<decltype(eb)::value>), g, b, 0, s, planes, src, srcOff, nTensors, capacity); });
    return hipGetLastError();
}

hipError_t launch_planes_merge_pred(u8* dst, const u64* dstOff, size_t* results, const u8* planes, const u64* planeOff, const size_t* planeSizes, size_t nTensors,
                                    unsigned E, u64 dstCapacity, hipStream_t s)
{
    if (nTensors == 0) return hipSuccess;
    const hipError_t e0 = launch_planes_verdicts(results, dstOff, planeSizes, nTensors, E, dstCapacity, s);
    if (e0 != hipSuccess || dstCapacity == 0) return e0;
    const dim3 g(tile_grid(dstCapacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        hipLaunchKernelGGL((k_planes_merge_pred<decltype(eb)::value>), g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, nTensors, dstCapacity);
    });
    return hipGetLastError();
}

// The six C calls are those of planes_stride.hip with stride 1, which launches the kernels above: one set of argument checks, one chain of
// launches per call
extern "C" int FSEHIP_planes_split_pred_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const uint64_t* d_srcOffsets,
                                               size_t nTensors, unsigned elemBytes, uint64_t capacity, void* stream)
{
    return FSEHIP_planes_split_pred_stride_dbatch(d_planes, d_planeOffsets, d_tensorResults, d_src, d_srcOffsets, nTensors, elemBytes, capacity, 1, stream);
}

extern "C" int FSEHIP_planes_merge_pred_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                               const size_t* d_planeSizes, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream)
{
    return FSEHIP_planes_merge_pred_stride_dbatch(d_dst, d_dstOffsets, d_results, d_planes, d_planeOffsets, d_planeSizes, nTensors, elemBytes, dstCapacity, 1, stream);
}

extern "C" int FSEHIP_tensor_compress_pred_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                  const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                                  size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille,
                                                  unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes, void* stream)
{
    return FSEHIP_tensor_compress_pred_stride_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_srcOffsets, nTensors, elemBytes, capacity,
                                                     maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille, slotAlignLog, d_planes, d_planeOffsets,
                                                     d_workspace, workspaceBytes, 1, stream);
}

extern "C" int FSEHIP_tensor_compress_seg_pred_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                      const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                                      const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks, unsigned blockSizeId,
                                                      int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes,
                                                      uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace, size_t workspaceBytes, void* stream)
{
    return FSEHIP_tensor_compress_seg_pred_stride_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_srcOffsets, nTensors, elemBytes,
                                                         capacity, d_segFirst, nSegments, segLog, maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille,
                                                         slotAlignLog, d_planes, d_planeOffsets, d_segOffsets, d_workspace, workspaceBytes, 1, stream);
}

extern "C" int FSEHIP_tensor_decompress_pred_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results, const void* d_frames,
                                                    const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks, void* d_planes,
                                                    uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults, void* d_workspace, size_t workspaceBytes,
                                                    void* stream)
{
    return FSEHIP_tensor_decompress_pred_stride_dbatch(d_dst, d_dstOffsets, dstCapacity, d_results, d_frames, d_frameOffsets, nTensors, elemBytes, maxTotalBlocks, d_planes,
                                                       planesCapacity, d_planeOffsets, d_planeResults, d_workspace, workspaceBytes, 1, stream);
}

extern "C" int FSEHIP_tensor_decompress_seg_pred_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results, const void* d_frames,
                                                        const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst,
                                                        size_t nSegments, unsigned segLog, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                                                        uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets, size_t* d_planeSizes, void* d_workspace,
                                                        size_t workspaceBytes, void* stream)
{
    return FSEHIP_tensor_decompress_seg_pred_stride_dbatch(d_dst, d_dstOffsets, dstCapacity, d_results, d_frames, d_frameOffsets, nTensors, elemBytes, d_segFirst, nSegments,
                                                           segLog, maxTotalBlocks, d_planes, planesCapacity, d_segOffsets, d_segResults, d_planeOffsets, d_planeSizes,
                                                           d_workspace, workspaceBytes, 1, stream);
}

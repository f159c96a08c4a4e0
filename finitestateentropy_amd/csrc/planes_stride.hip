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
// The bodies of both kernels, ps_split and ps_merge, and their helpers are in planes_dev.h: planes_each_stride.hip takes the same ones.
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
template <int E, int S>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split_pred_stride(u8* planes, const u8* src, const u64* SO, size_t nT, u64 capacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(SO, nT, w, i)) return;                           // (uniform, like every return below)
    const u64 s0 = SO[i], s1 = SO[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(s0 < s1) || s1 > capacity || lo >= s1 || lo + PLANES_TILE <= s0) return;
    ps_split<E, S>(planes + s0, src + s0, s0, s1 - s0, lo, threadIdx.x);
}

template <int E, int S>
__global__ __launch_bounds__(PL_THREADS) void k_planes_merge_pred_stride(u8* dst, const u64* D, const u8* planes, const u64* PO, const size_t* PS, size_t nT, u64 dstCapacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(D, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 d0 = D[i], first = (d0 >> PL_TILE_LOG) + i;
    if (first > w) return;                                        // (offsets that decrease: the search found no tensor of this item)
    const u64 t = w - first;
    const size_t v = pm_verdict(D, PS, i, E, dstCapacity);
    if (is_err(v) || (t << PL_TILE_LOG) >= (u64)v) return;        // (a good tensor: d0 + n <= D[i + 1] <= dstCapacity; t < 2^24)
    ps_merge<E, S>(dst + d0, planes, PO + i * E, v, t);
}
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

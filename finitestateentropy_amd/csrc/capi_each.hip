// capi_each.hip -- the C calls of "a transform per tensor" (fsehip.h): argument checks in front of the first launch, then launches only.
//
//   FSEHIP_planes_split_each_dbatch / _merge_each_dbatch : the launchers of planes_each.hip
//   FSEHIP_tensor_compress(_seg)_each_dbatch   : [CHOOSE: FSEHIP_planes_estimate_dbatch, its choice into d_transforms] -> the split by d_transforms
//                                                -> [the segments kernel] -> the packed (mixed) writer
//   FSEHIP_tensor_decompress(_seg)_each_dbatch : the packed reader -> [the fold] -> the merge by d_transforms
//   FSEHIP_planes_merge_window_each_dbatch     : the launcher of the window form of that merge
//   FSEHIP_tensor_decompress_window_each_dbatch: the selection -> the packed reader over the extents -> the window fold (planes_win.hip, all
//                                                three as they are) -> the window form of the merge
//
//   the seven calls of "a stride per tensor" (at the end): the six above with d_strides behind d_transforms -- the launchers of
//                                                planes_each_stride.hip, and with CHOOSE the estimate over strides (planes_estimate.hip)
//   the two window calls with d_strides (at the very end): FSEHIP_planes_merge_window_each_stride_dbatch and
//                                                FSEHIP_tensor_decompress_window_each_stride_dbatch, the launcher of planes_each_stride_win.hip
//
// The workspace of a CHOOSE call: the estimate's counters, plane costs, estimates and results (each a multiple of 256) in front of the
// writer's workspace; FSEHIP_tensor_each_workspaceHead is their sum.
#include "planes_dev.h"

namespace {
inline size_t r256(size_t x) { return (x + 255) & ~(size_t)255; }
struct EachHead { size_t counters, bits, est, res; size_t total() const { return counters + bits + est + res; } };
// mask and nTensors as FSEHIP_planes_estimate_workspaceBound takes them (an error: counters holds it)
// strideMask 0: the four-candidate estimate; else the estimate over strides (the same numbers for strideMask 1)
inline EachHead each_head(size_t nTensors, unsigned E, unsigned mask, unsigned strideMask = 0)
{
    return { strideMask ? FSEHIP_planes_estimate_stride_workspaceBound(nTensors, E, mask, strideMask) : FSEHIP_planes_estimate_workspaceBound(nTensors, E, mask), r256(nTensors * 4 * E * sizeof(u64)), r256(nTensors * 4 * sizeof(u64)), r256(nTensors * sizeof(size_t)) };
}
inline bool bad_policy(int transformPolicy) { return transformPolicy != FSEHIP_TRANSFORMS_GIVEN && transformPolicy != FSEHIP_TRANSFORMS_CHOOSE; }

// the one compress path of the four composites, each of which has checked its own pointers.  strideMask 0: the _each_ calls, d_strides
// null.  Else the _each_stride_ calls: GIVEN reads d_strides (null: stride 1 everywhere), CHOOSE writes it -- null there only with strideMask 1
int each_compress(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults, const void* d_src, const void* d_base,
                  uint8_t* d_transforms, int transformPolicy, unsigned candidateMask, unsigned marginPermille, uint64_t* d_estBytes, const uint64_t* d_srcOffsets,
                  size_t nTensors, unsigned E, uint64_t capacity, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, void* d_planes, uint64_t* d_planeOffsets,
                  uint64_t* d_segOffsets, const PlWriter& writer, void* stream, uint8_t* d_strides = nullptr, unsigned strideMask = 0)
{
    if (bad_policy(transformPolicy)) return (int)hipErrorInvalidValue;
    if (d_segFirst ? bad_seg(segLog, writer.blockSizeId) || bad_counts(nTensors, E, nSegments) : bad_tensors(nTensors, E)) return (int)hipErrorInvalidValue;
    const size_t nFrames = d_segFirst ? nSegments : nTensors * E;
    const bool choose = transformPolicy == FSEHIP_TRANSFORMS_CHOOSE;
    EachHead h = { 0, 0, 0, 0 };
    if (choose) {
        const unsigned baseBits = (1u << FSEHIP_EST_XOR) | (1u << FSEHIP_EST_SUB);
        if (marginPermille > 1000 || ((candidateMask & baseBits) && !d_base)) return (int)hipErrorInvalidValue;
        if (strideMask > 1 && !d_strides) return (int)hipErrorInvalidValue;
        if (!d_strides) strideMask = 0;                                     // (stride 1 everywhere: the _each_ call)
        h = each_head(nTensors, E, candidateMask, strideMask);
        if (FSEHIP_isError(h.counters)) return (int)hipErrorInvalidValue;   // (a mask of 0 or with an unknown bit; a bad stride set; 2^24 tensors)
    }
    if (((uintptr_t)writer.d_workspace & 255u) || writer.workspaceBytes < h.total() || (h.total() && !writer.d_workspace)) return (int)hipErrorInvalidValue;
    PlWriter w = writer;
    u8* const ws = (u8*)writer.d_workspace;
    if (h.total()) { w.d_workspace = ws + h.total(); w.workspaceBytes -= h.total(); }
    if (bad_grid(capacity, nTensors) || bad_writer(w, nFrames)) return (int)hipErrorInvalidValue;
    if (choose) {
        u64* const bits = (u64*)(ws + h.counters);
        u64* const est = d_estBytes ? (u64*)d_estBytes : (u64*)(ws + h.counters + h.bits);
        size_t* const res = (size_t*)(ws + h.counters + h.bits + h.est);
        const int r = strideMask ? planes_estimate_stride(bits, est, d_transforms, res, nullptr, d_strides, d_src, d_base, d_srcOffsets, nTensors, E, capacity,
                                                          candidateMask, marginPermille, ws, h.counters, strideMask, true, stream)
                                 : FSEHIP_planes_estimate_dbatch(bits, est, d_transforms, res, d_src, d_base, d_srcOffsets, nTensors, E, capacity, candidateMask,
                                                                 marginPermille, ws, h.counters, stream);
        if (r != 0) return r;
    }
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = launch_planes_split_each_stride((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u8*)d_base, d_transforms, d_strides,
                                                   (const u64*)d_srcOffsets, nTensors, E, capacity, s);
    if (e == hipSuccess && d_segFirst)
        e = launch_segments((u64*)d_segOffsets, d_tensorResults, (const u64*)d_planeOffsets, (const u64*)d_srcOffsets, (const u64*)d_segFirst, nTensors, E, nSegments, segLog, s);
    if (e != hipSuccess) return (int)e;
    const uint64_t* const fromOff = d_segFirst ? d_segOffsets : d_planeOffsets;
    if (w.d_codecs)
        return FSEHIP_frame_compress_packed_mixed_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_planes, fromOff, nFrames, w.maxTotalBlocks, w.blockSizeId,
                                                         w.d_codecs, w.policy, w.tolerancePermille, w.slotAlignLog, w.d_workspace, w.workspaceBytes, stream);
    return FSEHIP_frame_compress_packed_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_planes, fromOff, nFrames, w.maxTotalBlocks, w.blockSizeId, w.codec,
                                               w.slotAlignLog, w.d_workspace, w.workspaceBytes, stream);
}
}   // namespace

extern "C" size_t FSEHIP_tensor_each_workspaceHead(size_t nTensors, unsigned elemBytes, int transformPolicy, unsigned candidateMask)
{
    if (bad_elem(elemBytes) || bad_policy(transformPolicy)) return FSEHIP_ERROR(GENERIC);
    if (transformPolicy == FSEHIP_TRANSFORMS_GIVEN) return 0;
    const EachHead h = each_head(nTensors, elemBytes, candidateMask);
    return FSEHIP_isError(h.counters) ? h.counters : h.total();
}

extern "C" int FSEHIP_planes_split_each_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const void* d_base,
                                               const uint8_t* d_transforms, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                               void* stream)
{
    if (bad_elem(elemBytes) || !d_planes || !d_planeOffsets || !d_tensorResults || !d_src || !d_transforms || !d_srcOffsets) return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(capacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_split_each((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u8*)d_base, d_transforms, (const u64*)d_srcOffsets,
                                         nTensors, elemBytes, capacity, (hipStream_t)stream);
}

extern "C" int FSEHIP_planes_merge_each_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                               const size_t* d_planeSizes, const void* d_base, const uint8_t* d_transforms, size_t nTensors, unsigned elemBytes,
                                               uint64_t dstCapacity, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_planes || !d_planeOffsets || !d_planeSizes || !d_transforms) return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(dstCapacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_merge_each((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, (const u8*)d_base,
                                         d_transforms, nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}

extern "C" int FSEHIP_tensor_compress_each_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                  const void* d_src, const void* d_base, uint8_t* d_transforms, int transformPolicy, unsigned candidateMask,
                                                  unsigned marginPermille, uint64_t* d_estBytes, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                  uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy,
                                                  unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets, void* d_workspace,
                                                  size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_transforms || !d_srcOffsets || !d_planeOffsets || !d_planes)
        return (int)hipErrorInvalidValue;
    return each_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, d_transforms, transformPolicy, candidateMask, marginPermille,
                         d_estBytes, d_srcOffsets, nTensors, elemBytes, capacity, nullptr, 0, 0, d_planes, d_planeOffsets, nullptr,
                         PlWriter{ maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes }, stream);
}

extern "C" int FSEHIP_tensor_compress_seg_each_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                      const void* d_src, const void* d_base, uint8_t* d_transforms, int transformPolicy, unsigned candidateMask,
                                                      unsigned marginPermille, uint64_t* d_estBytes, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                      uint64_t capacity, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks,
                                                      unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog,
                                                      void* d_planes, uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace, size_t workspaceBytes,
                                                      void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_transforms || !d_srcOffsets || !d_segFirst || !d_planeOffsets ||
        !d_segOffsets || !d_planes)
        return (int)hipErrorInvalidValue;
    return each_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, d_transforms, transformPolicy, candidateMask, marginPermille,
                         d_estBytes, d_srcOffsets, nTensors, elemBytes, capacity, d_segFirst, nSegments, segLog, d_planes, d_planeOffsets, d_segOffsets,
                         PlWriter{ maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes }, stream);
}

// the argument checks of both steps in front of the first launch
extern "C" int FSEHIP_tensor_decompress_each_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, const uint8_t* d_transforms,
                                                    size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                    size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                                    void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_transforms || !d_results || !d_frames || !d_frameOffsets || !d_planes || !d_planeOffsets || !d_planeResults)
        return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(dstCapacity, nTensors) || bad_reader(d_workspace, workspaceBytes, nTensors * elemBytes, maxTotalBlocks))
        return (int)hipErrorInvalidValue;
    const int r = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_planeOffsets, d_planeResults, d_frames, d_frameOffsets, nTensors * elemBytes,
                                                        maxTotalBlocks, 0, d_workspace, workspaceBytes, stream);
    if (r != 0) return r;
    return (int)launch_planes_merge_each((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeResults,
                                         (const u8*)d_base, d_transforms, nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}

extern "C" int FSEHIP_tensor_decompress_seg_each_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, const uint8_t* d_transforms,
                                                        size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                        const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks, void* d_planes,
                                                        uint64_t planesCapacity, uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets,
                                                        size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_transforms || !d_results || !d_frames || !d_frameOffsets || !d_segFirst || !d_planes || !d_segOffsets ||
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
    return (int)launch_planes_merge_each((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, (const u8*)d_base,
                                         d_transforms, nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}

// ---- windows of tensors with a transform per tensor ----
extern "C" int FSEHIP_planes_merge_window_each_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                                      const size_t* d_planeSizes, const void* d_base, const uint8_t* d_transforms, const uint64_t* d_windows,
                                                      size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_planes || !d_planeOffsets || !d_planeSizes || !d_transforms || !d_windows)
        return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(dstCapacity, 2 * nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_merge_window_each((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes,
                                                (const u8*)d_base, d_transforms, (const u64*)d_windows, nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}

// the argument checks of all four steps in front of the first launch (those of the selection and of the fold are among them)
extern "C" int FSEHIP_tensor_decompress_window_each_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base,
                                                           const uint8_t* d_transforms, size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets,
                                                           const uint64_t* d_srcOffsets, const uint64_t* d_windows, size_t nTensors, unsigned elemBytes,
                                                           const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, const uint64_t* d_selFirst, size_t nSelected,
                                                           size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity, uint64_t* d_selFrameOffsets,
                                                           uint64_t* d_selOffsets, size_t* d_selResults, uint64_t* d_planeOffsets, size_t* d_planeSizes,
                                                           void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_transforms || !d_results || !d_frames || !d_frameOffsets || !d_srcOffsets || !d_windows || !d_segFirst ||
        !d_selFirst || !d_planes || !d_selFrameOffsets || !d_selOffsets || !d_selResults || !d_planeOffsets || !d_planeSizes)
        return (int)hipErrorInvalidValue;
    if (bad_seg(segLog, 0) || bad_counts(nTensors, elemBytes, nSelected) || nSegments >= ((size_t)1 << 31) || nSelected > nSegments || bad_grid(dstCapacity, 2 * nTensors))
        return (int)hipErrorInvalidValue;
    if (bad_reader(d_workspace, workspaceBytes, nSelected, maxTotalBlocks)) return (int)hipErrorInvalidValue;
    int r = FSEHIP_planes_select_window_dbatch(d_selFrameOffsets, d_frameOffsets, d_srcOffsets, d_windows, d_segFirst, d_selFirst, nTensors, elemBytes, nSegments, nSelected,
                                               segLog, stream);
    if (r != 0) return r;
    r = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_selOffsets, d_selResults, d_frames, d_selFrameOffsets, nSelected, maxTotalBlocks, 0,
                                              d_workspace, workspaceBytes, stream);
    if (r != 0) return r;
    r = FSEHIP_planes_fold_window_dbatch(d_planeOffsets, d_planeSizes, d_selOffsets, d_selResults, d_srcOffsets, d_windows, d_segFirst, d_selFirst, nTensors, elemBytes,
                                         nSelected, segLog, stream);
    if (r != 0) return r;
    return (int)launch_planes_merge_window_each((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes,
                                                (const u8*)d_base, d_transforms, (const u64*)d_windows, nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}

// ---- a stride per tensor (fsehip.h, the section of that name): the six calls above with d_strides behind d_transforms ----
extern "C" size_t FSEHIP_tensor_each_stride_workspaceHead(size_t nTensors, unsigned elemBytes, int transformPolicy, unsigned candidateMask, unsigned strideMask)
{
    if (bad_elem(elemBytes) || bad_policy(transformPolicy)) return FSEHIP_ERROR(GENERIC);
    if (transformPolicy == FSEHIP_TRANSFORMS_GIVEN) return 0;
    if (strideMask == 0) return FSEHIP_ERROR(GENERIC);
    const EachHead h = each_head(nTensors, elemBytes, candidateMask, strideMask);
    return FSEHIP_isError(h.counters) ? h.counters : h.total();
}

extern "C" int FSEHIP_planes_split_each_stride_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const void* d_base,
                                                      const uint8_t* d_transforms, const uint8_t* d_strides, const uint64_t* d_srcOffsets, size_t nTensors,
                                                      unsigned elemBytes, uint64_t capacity, void* stream)
{
    if (bad_elem(elemBytes) || !d_planes || !d_planeOffsets || !d_tensorResults || !d_src || !d_transforms || !d_srcOffsets) return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(capacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_split_each_stride((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u8*)d_base, d_transforms, d_strides,
                                                (const u64*)d_srcOffsets, nTensors, elemBytes, capacity, (hipStream_t)stream);
}

extern "C" int FSEHIP_planes_merge_each_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                                      const size_t* d_planeSizes, const void* d_base, const uint8_t* d_transforms, const uint8_t* d_strides,
                                                      size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_planes || !d_planeOffsets || !d_planeSizes || !d_transforms) return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(dstCapacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_merge_each_stride((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes,
                                                (const u8*)d_base, d_transforms, d_strides, nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}

// CHOOSE: a stride set of 0 is refused here (inside each_compress it stands for the _each_ calls); GIVEN ignores the set
extern "C" int FSEHIP_tensor_compress_each_stride_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                         const void* d_src, const void* d_base, uint8_t* d_transforms, uint8_t* d_strides, int transformPolicy,
                                                         unsigned candidateMask, unsigned strideMask, unsigned marginPermille, uint64_t* d_estBytes,
                                                         const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity, size_t maxTotalBlocks,
                                                         unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille,
                                                         unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes,
                                                         void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_transforms || !d_srcOffsets || !d_planeOffsets || !d_planes)
        return (int)hipErrorInvalidValue;
    if (transformPolicy == FSEHIP_TRANSFORMS_CHOOSE && strideMask == 0) return (int)hipErrorInvalidValue;
    return each_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, d_transforms, transformPolicy, candidateMask, marginPermille,
                         d_estBytes, d_srcOffsets, nTensors, elemBytes, capacity, nullptr, 0, 0, d_planes, d_planeOffsets, nullptr,
                         PlWriter{ maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes }, stream, d_strides,
                         strideMask);
}

extern "C" int FSEHIP_tensor_compress_seg_each_stride_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                             const void* d_src, const void* d_base, uint8_t* d_transforms, uint8_t* d_strides, int transformPolicy,
                                                             unsigned candidateMask, unsigned strideMask, unsigned marginPermille, uint64_t* d_estBytes,
                                                             const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                                             const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks, unsigned blockSizeId,
                                                             int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes,
                                                             uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_transforms || !d_srcOffsets || !d_segFirst || !d_planeOffsets ||
        !d_segOffsets || !d_planes)
        return (int)hipErrorInvalidValue;
    if (transformPolicy == FSEHIP_TRANSFORMS_CHOOSE && strideMask == 0) return (int)hipErrorInvalidValue;
    return each_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, d_transforms, transformPolicy, candidateMask, marginPermille,
                         d_estBytes, d_srcOffsets, nTensors, elemBytes, capacity, d_segFirst, nSegments, segLog, d_planes, d_planeOffsets, d_segOffsets,
                         PlWriter{ maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes }, stream, d_strides,
                         strideMask);
}

// the argument checks of both steps in front of the first launch
extern "C" int FSEHIP_tensor_decompress_each_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base,
                                                           const uint8_t* d_transforms, const uint8_t* d_strides, size_t* d_results, const void* d_frames,
                                                           const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks, void* d_planes,
                                                           uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults, void* d_workspace,
                                                           size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_transforms || !d_results || !d_frames || !d_frameOffsets || !d_planes || !d_planeOffsets || !d_planeResults)
        return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(dstCapacity, nTensors) || bad_reader(d_workspace, workspaceBytes, nTensors * elemBytes, maxTotalBlocks))
        return (int)hipErrorInvalidValue;
    const int r = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_planeOffsets, d_planeResults, d_frames, d_frameOffsets, nTensors * elemBytes,
                                                        maxTotalBlocks, 0, d_workspace, workspaceBytes, stream);
    if (r != 0) return r;
    return (int)launch_planes_merge_each_stride((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeResults,
                                                (const u8*)d_base, d_transforms, d_strides, nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}

extern "C" int FSEHIP_tensor_decompress_seg_each_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base,
                                                               const uint8_t* d_transforms, const uint8_t* d_strides, size_t* d_results, const void* d_frames,
                                                               const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst,
                                                               size_t nSegments, unsigned segLog, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                                                               uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets, size_t* d_planeSizes,
                                                               void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_transforms || !d_results || !d_frames || !d_frameOffsets || !d_segFirst || !d_planes || !d_segOffsets ||
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
    return (int)launch_planes_merge_each_stride((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes,
                                                (const u8*)d_base, d_transforms, d_strides, nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}

// ---- windows of tensors with a stride per tensor (fsehip.h, "windows and patches of tensors with a stride per tensor"; the write side is in
// planes_patch.hip): the two window calls above with d_strides behind d_transforms, null: stride 1 everywhere ----
extern "C" int FSEHIP_planes_merge_window_each_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes,
                                                             const uint64_t* d_planeOffsets, const size_t* d_planeSizes, const void* d_base, const uint8_t* d_transforms,
                                                             const uint8_t* d_strides, const uint64_t* d_windows, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity,
                                                             void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_planes || !d_planeOffsets || !d_planeSizes || !d_transforms || !d_windows)
        return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(dstCapacity, 2 * nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_merge_window_each_stride((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes,
                                                       (const u8*)d_base, d_transforms, d_strides, (const u64*)d_windows, nTensors, elemBytes, dstCapacity,
                                                       (hipStream_t)stream);
}

// the argument checks of all four steps in front of the first launch (those of the selection and of the fold are among them)
extern "C" int FSEHIP_tensor_decompress_window_each_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base,
                                                                  const uint8_t* d_transforms, const uint8_t* d_strides, size_t* d_results, const void* d_frames,
                                                                  const uint64_t* d_frameOffsets, const uint64_t* d_srcOffsets, const uint64_t* d_windows, size_t nTensors,
                                                                  unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog,
                                                                  const uint64_t* d_selFirst, size_t nSelected, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                                                                  uint64_t* d_selFrameOffsets, uint64_t* d_selOffsets, size_t* d_selResults, uint64_t* d_planeOffsets,
                                                                  size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_transforms || !d_results || !d_frames || !d_frameOffsets || !d_srcOffsets || !d_windows || !d_segFirst ||
        !d_selFirst || !d_planes || !d_selFrameOffsets || !d_selOffsets || !d_selResults || !d_planeOffsets || !d_planeSizes)
        return (int)hipErrorInvalidValue;
    if (bad_seg(segLog, 0) || bad_counts(nTensors, elemBytes, nSelected) || nSegments >= ((size_t)1 << 31) || nSelected > nSegments || bad_grid(dstCapacity, 2 * nTensors))
        return (int)hipErrorInvalidValue;
    if (bad_reader(d_workspace, workspaceBytes, nSelected, maxTotalBlocks)) return (int)hipErrorInvalidValue;
    int r = FSEHIP_planes_select_window_dbatch(d_selFrameOffsets, d_frameOffsets, d_srcOffsets, d_windows, d_segFirst, d_selFirst, nTensors, elemBytes, nSegments, nSelected,
                                               segLog, stream);
    if (r != 0) return r;
    r = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_selOffsets, d_selResults, d_frames, d_selFrameOffsets, nSelected, maxTotalBlocks, 0,
                                              d_workspace, workspaceBytes, stream);
    if (r != 0) return r;
    r = FSEHIP_planes_fold_window_dbatch(d_planeOffsets, d_planeSizes, d_selOffsets, d_selResults, d_srcOffsets, d_windows, d_segFirst, d_selFirst, nTensors, elemBytes,
                                         nSelected, segLog, stream);
    if (r != 0) return r;
    return (int)launch_planes_merge_window_each_stride((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes,
                                                       (const u8*)d_base, d_transforms, d_strides, (const u64*)d_windows, nTensors, elemBytes, dstCapacity,
                                                       (hipStream_t)stream);
}

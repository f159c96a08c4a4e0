// planes_seg.hip -- SEGMENTED PLANES (fsehip.h, "segmented planes"): a plane of a large tensor cut into segments of 1 << segLog bytes, ONE FRAME
// PER SEGMENT.  A frame ends in one XXH32 over its whole content, a chain that one lane quad walks at about 1.5 GB/s, and the reader walks a
// frame's headers and settles its blocks serially: a plane of hundreds of MiB as one frame takes hundreds of milliseconds whatever the rest of
// the device does.  A segment is a whole number of blocks, blocks are coded independently of their position, so the segment frames hold the
// single frame's blocks byte for byte, eight bytes more per additional frame, and no chain is longer than a segment.  Kernel launches only.
//
//   FSEHIP_planes_segmentFirst           : host arithmetic, the first segment index of every plane from the tensor offsets
//   FSEHIP_planes_segments_dbatch        : k_planes_segments -- per segment entry its offset in the planes buffer; per tensor its verdict
//   FSEHIP_planes_fold_segments_dbatch   : k_planes_fold -- per plane (one wave) the offset and the verdict of its segments' results
//   FSEHIP_tensor_compress_seg_dbatch    : the (XOR) split -> the segments kernel -> the packed (mixed) writer over the segments
//   FSEHIP_tensor_decompress_seg_dbatch  : the packed reader into the planes buffer -> the fold -> the (XOR) merge
// The data kernels of planes.hip run unchanged in front of and behind these.
#include "planes_dev.h"

namespace {
// One thread per segment entry q <= nSeg: the plane j that holds it is the largest j < nP with SF[j] <= q (pl_last_le, the search of
// pl_find), its entry min(P[j] + (q - SF[j]) * seg, P[j + 1]); the entries of a tensor whose counts in SF are not those its size implies are
// all its start P[i * E].  The last entry is P[nP].  Threads i < nT also write tensor i's GENERIC.  SF's values are never used as indices and
// every index is clamped: whatever SF holds, nothing outside the arrays is touched.
__global__ void k_planes_segments(u64* SO, size_t* tres, const u64* P, const u64* S, const u64* SF, size_t nT, u32 E, size_t nSeg, u32 segLog)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nP = nT * E;
    if (q < nT && !ps_tensor_ok(S, SF, q, E, segLog)) tres[q] = FERR(GENERIC);
    if (q > nSeg) return;
    if (q == nSeg || nP == 0) { SO[q] = P[nP]; return; }
    const size_t j = pl_last_le(nP, q, [SF](size_t m) { return SF[m]; }), i = j / E;
    if (!ps_tensor_ok(S, SF, i, E, segLog)) { SO[q] = P[i * E]; return; }
    const u64 f = SF[j], k = q >= f ? q - f : 0, at = P[j] + (k << segLog), end = P[j + 1];
    SO[q] = at < end ? at : end;
}

// One wave per plane, its lanes striding over the plane's segments (ps_fold); the verdict in the order of fsehip.h.  The size rule: every
// segment but the last is full, the last holds 1 .. seg bytes (0 where it is the only one).
__global__ __launch_bounds__(PL_THREADS) void k_planes_fold(u64* PO, size_t* PS, const u64* off, const size_t* res, const u64* SF, size_t nP, size_t nSeg, u32 segLog)
{
    const size_t j = (size_t)blockIdx.x * (PL_THREADS / WAVE) + (threadIdx.x / WAVE);
    if (j >= nP) return;                                          // (uniform over the wave)
    const u32 lane = threadIdx.x % WAVE;
    u64 q1 = SF[j + 1], q0 = SF[j];
    if (q1 > nSeg) q1 = nSeg;
    if (q0 > q1) q0 = q1;
    const u64 cnt = q1 - q0, seg = (u64)1 << segLog;
    const PsFold f = ps_fold(off + q0, res + q0, cnt, lane, [=](u64 k, u64 r) { return k + 1 == cnt ? r <= seg && (r != 0 || cnt == 1) : r == seg; });
    if (lane) return;
    PO[j] = off[q0];
    PS[j] = cnt == 0 ? FERR(GENERIC) : f.firstErr != 0xFFFFFFFFu ? res[q0 + f.firstErr] : f.bad ? FERR(corruption_detected) : (size_t)f.sum;
}

hipError_t launch_fold(u64* planeOff, size_t* planeSizes, const u64* segOff, const size_t* segRes, const u64* segFirst, size_t nPlanes, size_t nSeg, unsigned segLog,
                       hipStream_t s)
{
    if (nPlanes == 0) return hipSuccess;
    const size_t perGroup = PL_THREADS / WAVE;
    hipLaunchKernelGGL(k_planes_fold, dim3((unsigned)((nPlanes + perGroup - 1) / perGroup)), dim3(PL_THREADS), 0, s, planeOff, planeSizes, segOff, segRes, segFirst,
                       nPlanes, nSeg, (u32)segLog);
    return hipGetLastError();
}
}   // namespace

hipError_t launch_segments(u64* segOff, size_t* tensorRes, const u64* planeOff, const u64* srcOff, const u64* segFirst, size_t nTensors, unsigned E, size_t nSeg,
                           unsigned segLog, hipStream_t s)
{
    const size_t n = nSeg + 1 > nTensors ? nSeg + 1 : nTensors;
    hipLaunchKernelGGL(k_planes_segments, dim3(grid_for(n)), dim3(PL_THREADS), 0, s, segOff, tensorRes, planeOff, srcOff, segFirst, nTensors, (u32)E, nSeg, (u32)segLog);
    return hipGetLastError();
}

extern "C" size_t FSEHIP_planes_segmentFirst(uint64_t* h_segFirst, const uint64_t* h_offsets, size_t nTensors, unsigned elemBytes, unsigned segLog)
{
    if (bad_elem(elemBytes) || bad_seg(segLog, 0) || (nTensors && !h_offsets)) return FSEHIP_ERROR(GENERIC);
    const u32 E = elemBytes;
    u64 total = 0;
    if (h_segFirst) h_segFirst[0] = 0;
    for (size_t i = 0; i < nTensors; ++i) {
        const u64 s0 = h_offsets[i], s1 = h_offsets[i + 1], n = s1 > s0 ? s1 - s0 : 0;
        for (u32 p = 0; p < E; ++p) {
            total += ps_count(pl_size(n, p, E), segLog);
            if (total >= ((u64)1 << 31)) return FSEHIP_ERROR(GENERIC);
            if (h_segFirst) h_segFirst[i * E + p + 1] = total;
        }
    }
    return (size_t)total;
}

extern "C" int FSEHIP_planes_segments_dbatch(uint64_t* d_segOffsets, size_t* d_tensorResults, const uint64_t* d_planeOffsets, const uint64_t* d_srcOffsets,
                                             const uint64_t* d_segFirst, size_t nTensors, unsigned elemBytes, size_t nSegments, unsigned segLog, void* stream)
{
    if (bad_elem(elemBytes) || bad_seg(segLog, 0) || !d_segOffsets || !d_tensorResults || !d_planeOffsets || !d_srcOffsets || !d_segFirst) return (int)hipErrorInvalidValue;
    if (bad_counts(nTensors, elemBytes, nSegments)) return (int)hipErrorInvalidValue;
    return (int)launch_segments((u64*)d_segOffsets, d_tensorResults, (const u64*)d_planeOffsets, (const u64*)d_srcOffsets, (const u64*)d_segFirst, nTensors, elemBytes,
                                nSegments, segLog, (hipStream_t)stream);
}

extern "C" int FSEHIP_planes_fold_segments_dbatch(uint64_t* d_planeOffsets, size_t* d_planeSizes, const uint64_t* d_segOffsets, const size_t* d_segResults,
                                                  const uint64_t* d_segFirst, size_t nPlanes, size_t nSegments, unsigned segLog, void* stream)
{
    if (bad_seg(segLog, 0) || !d_planeOffsets || !d_planeSizes || !d_segOffsets || !d_segResults || !d_segFirst) return (int)hipErrorInvalidValue;
    if (nPlanes >= ((size_t)1 << 31) || nSegments >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    return (int)launch_fold((u64*)d_planeOffsets, d_planeSizes, (const u64*)d_segOffsets, d_segResults, (const u64*)d_segFirst, nPlanes, nSegments, segLog,
                            (hipStream_t)stream);
}

extern "C" int FSEHIP_tensor_compress_seg_op_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                    const void* d_src, const void* d_base, unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors,
                                                    unsigned elemBytes, uint64_t capacity, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog,
                                                    size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille,
                                                    unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace,
                                                    size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_srcOffsets || !d_segFirst || !d_planeOffsets || !d_segOffsets ||
        ((elemBytes > 1 || d_base) && !d_planes))
        return (int)hipErrorInvalidValue;
    return planes_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, deltaOp, d_srcOffsets, nTensors, elemBytes, capacity,
                           d_segFirst, nSegments, segLog, d_planes, d_planeOffsets, d_segOffsets,
                           PlWriter{ maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes }, stream);
}
extern "C" int FSEHIP_tensor_compress_seg_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                 const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                 uint64_t capacity, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks,
                                                 unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog,
                                                 void* d_planes, uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace, size_t workspaceBytes, void* stream)
{
    return FSEHIP_tensor_compress_seg_op_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, FSEHIP_DELTA_XOR, d_srcOffsets, nTensors,
                                                elemBytes, capacity, d_segFirst, nSegments, segLog, maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille,
                                                slotAlignLog, d_planes, d_planeOffsets, d_segOffsets, d_workspace, workspaceBytes, stream);
}

extern "C" int FSEHIP_tensor_decompress_seg_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, size_t* d_results,
                                                   const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                   const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks,
                                                   void* d_planes, uint64_t planesCapacity, uint64_t* d_segOffsets, size_t* d_segResults,
                                                   uint64_t* d_planeOffsets, size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream)
{
    return FSEHIP_tensor_decompress_seg_op_dbatch(d_dst, d_dstOffsets, dstCapacity, d_base, FSEHIP_DELTA_XOR, d_results, d_frames, d_frameOffsets, nTensors, elemBytes,
                                                  d_segFirst, nSegments, segLog, maxTotalBlocks, d_planes, planesCapacity, d_segOffsets, d_segResults, d_planeOffsets,
                                                  d_planeSizes, d_workspace, workspaceBytes, stream);
}
// the argument checks of all three steps in front of the first launch
extern "C" int FSEHIP_tensor_decompress_seg_op_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp,
                                                      size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                      const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks,
                                                      void* d_planes, uint64_t planesCapacity, uint64_t* d_segOffsets, size_t* d_segResults,
                                                      uint64_t* d_planeOffsets, size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_op(deltaOp) || bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_frames || !d_frameOffsets || !d_segFirst || !d_planes || !d_segOffsets || !d_segResults ||
        !d_planeOffsets || !d_planeSizes)
        return (int)hipErrorInvalidValue;
    if (bad_seg(segLog, 0) || bad_counts(nTensors, elemBytes, nSegments) || bad_grid(dstCapacity, nTensors) || bad_reader(d_workspace, workspaceBytes, nSegments, maxTotalBlocks))
        return (int)hipErrorInvalidValue;
    const int r = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_segOffsets, d_segResults, d_frames, d_frameOffsets, nSegments, maxTotalBlocks, 0,
                                                        d_workspace, workspaceBytes, stream);
    if (r != 0) return r;
    const hipStream_t s = (hipStream_t)stream;
    const hipError_t e = launch_fold((u64*)d_planeOffsets, d_planeSizes, (const u64*)d_segOffsets, d_segResults, (const u64*)d_segFirst, nTensors * elemBytes, nSegments,
                                     segLog, s);
    if (e != hipSuccess) return (int)e;
    return (int)launch_planes_merge((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, (const u8*)d_base,
                                    deltaOp, nTensors, elemBytes, dstCapacity, s);
}

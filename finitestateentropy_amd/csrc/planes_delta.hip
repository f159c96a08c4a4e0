// planes_delta.hip -- TENSOR DELTAS (fsehip.h, "tensor deltas"): the byte-plane calls of planes.hip on `tensor XOR base`, the XOR fused into the
// two data kernels.  The receiver of a tensor often holds an earlier version of it (weights after a step, the checkpoint before this one);
// XOR against that version zeroes every byte that did not change, the sign / exponent plane becomes almost all zeros, and the order-0 coders
// do the rest.  No bitstream, header or frame byte differs: the frames are ordinary .fse frames of the planes of `tensor XOR base`.
//
//   FSEHIP_planes_split_xor_dbatch       : k_planes_offsets (planes.hip) -> k_planes_split_xor, for every element size (E == 1 too: the XOR has
//                                          to be written somewhere)
//   FSEHIP_planes_merge_xor_dbatch       : k_planes_verdicts (planes.hip) -> k_planes_merge_xor; the base may be the destination itself
//   FSEHIP_tensor_compress_delta_dbatch  : the XOR split -> FSEHIP_frame_compress_packed_dbatch over the planes
//   FSEHIP_tensor_decompress_delta_dbatch: FSEHIP_frame_decompress_packed_dbatch into the planes buffer -> the XOR merge
//
// The data kernels are k_planes_split<E> / k_planes_merge<E> with one more read stream: same work mapping, same share of a tensor per
// workgroup, same chunks of 16 elements per lane (planes_dev.h); per chunk E more loads of 16 bytes from the base, which lies where the
// source (split) or the destination (merge) lies, each XORed into its words as it arrives.  XOR acts bit by bit, so it commutes with the byte
// shuffle: the split XORs in front of it, the merge behind it.  3 n bytes of traffic where the plain kernels have 2 n.
#include "planes_dev.h"

namespace {
DEV void pl_xor16(u32* w, const u8* from)
{
    u32 t[4];
    __builtin_memcpy(t, from, 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] ^= t[k];
}

template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split_xor(u8* planes, const u8* src, const u8* base, const u64* S, size_t nT, u64 capacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(S, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 s0 = S[i], s1 = S[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(s0 < s1) || s1 > capacity || lo >= s1 || lo + PLANES_TILE <= s0) return;
    const u64 n = s1 - s0;
    const u32 tid = threadIdx.x;
    const u8* const sb = src + s0;
    const u8* const bb = base + s0;
    u8* const pb = planes + s0;
    const PlShare h = pl_share<E>(s0, n, lo, (u64)(uintptr_t)pb, 1);
    for (u64 c = tid; c < h.nch; c += PL_THREADS) {
        const u64 e = h.eb + 16 * c;
        u32 wv[4 * E], o[E][4];
#pragma unroll
        for (int k = 0; k < E; ++k) __builtin_memcpy(&wv[4 * k], sb + e * E + 16 * k, 16);
#pragma unroll
        for (int k = 0; k < E; ++k) pl_xor16(&wv[4 * k], bb + e * E + 16 * k);
        pl_deinterleave<E>(wv, o);
#pragma unroll
        for (int p = 0; p < E; ++p) __builtin_memcpy(pb + pl_start(n, p, E) + e, o[p], 16);
    }
    const u64 nHead = (h.eb - h.e0) * E, nTail = (h.e1 - h.et) * E;
    for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) {
        const u64 k = j < nHead ? h.e0 * E + j : h.et * E + (j - nHead);
        if (k < n) pb[pl_start(n, (u32)(k % E), E) + k / E] = sb[k] ^ bb[k];
    }
}

// IN PLACE: `base` may be exactly `dst` (the resident tensors are updated where they lie).  Chunks, head and tail partition the elements of a
// workgroup's share, the shares partition the tensor (planes_dev.h: pl_share, the work mapping), and a tensor's bytes belong to no other
// tensor: every byte of dst is read (as base) and written by exactly ONE thread, and no thread reads a base byte that another one writes.
// Within a thread the base loads of a chunk -- all E of them -- precede its stores in program order, and neither pointer is __restrict__,
// so the compiler keeps that order: a store never lands in front of the load of the same bytes.  Any other overlap of base and dst is the
// caller's error and is not checked.  A refused or failed tensor returns in front of every load and store: in place its base stays as it is.
template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_merge_xor(u8* dst, const u64* D, const u8* planes, const u64* PO, const size_t* PS, const u8* base, size_t nT,
                                                                 u64 dstCapacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(D, nT, w, i)) return;
    const u64 d0 = D[i], d1 = D[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(d0 < d1) || lo >= d1 || lo + PLANES_TILE <= d0) return;
    const size_t v = pm_verdict(D, PS, i, E, dstCapacity);
    if (is_err(v) || lo >= d0 + (u64)v) return;                  // (a good tensor: d0 + n <= d1 <= dstCapacity)
    const u64 n = v;
    const u32 tid = threadIdx.x;
    u8* const db = dst + d0;
    const u8* const bb = base + d0;
    const u8* pp[E];
#pragma unroll
    for (int p = 0; p < E; ++p) pp[p] = planes + PO[i * E + p];
    const u64 addr = (u64)(uintptr_t)db;
    const PlShare h = pl_share<E>(d0, n, lo, addr, (addr % E) ? 0 : E);       // a tensor that starts inside an element's width never reaches a boundary
    for (u64 c = tid; c < h.nch; c += PL_THREADS) {
        const u64 e = h.eb + 16 * c;
        u32 wv[4 * E], o[E][4];
#pragma unroll
        for (int p = 0; p < E; ++p) __builtin_memcpy(o[p], pp[p] + e, 16);
        pl_interleave<E>(wv, o);
#pragma unroll
        for (int k = 0; k < E; ++k) pl_xor16(&wv[4 * k], bb + e * E + 16 * k);              // (in place: these loads, then the stores below)
#pragma unroll
        for (int k = 0; k < E; ++k) __builtin_memcpy(db + e * E + 16 * k, &wv[4 * k], 16);
    }
    const u64 nHead = (h.eb - h.e0) * E, nTail = (h.e1 - h.et) * E;
    for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) {
        const u64 k = j < nHead ? h.e0 * E + j : h.et * E + (j - nHead);
        if (k < n) db[k] = planes[PO[i * E + k % E] + k / E] ^ bb[k];
    }
}
}   // namespace

hipError_t launch_split_xor(u8* planes, u64* planeOff, size_t* tensorRes, const u8* src, const u8* base, const u64* srcOff, size_t nTensors, unsigned E, u64 capacity,
                            hipStream_t s)
{
    launch_planes_offsets(planeOff, tensorRes, srcOff, nTensors, E, capacity, s);
    if (nTensors == 0 || capacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(capacity, nTensors)), b(PL_THREADS);
    if (E == 1) hipLaunchKernelGGL(k_planes_split_xor<1>, g, b, 0, s, planes, src, base, srcOff, nTensors, capacity);
    else if (E == 2) hipLaunchKernelGGL(k_planes_split_xor<2>, g, b, 0, s, planes, src, base, srcOff, nTensors, capacity);
    else if (E == 4) hipLaunchKernelGGL(k_planes_split_xor<4>, g, b, 0, s, planes, src, base, srcOff, nTensors, capacity);
    else hipLaunchKernelGGL(k_planes_split_xor<8>, g, b, 0, s, planes, src, base, srcOff, nTensors, capacity);
    return hipGetLastError();
}

hipError_t launch_merge_xor(u8* dst, const u64* dstOff, size_t* results, const u8* planes, const u64* planeOff, const size_t* planeSizes, const u8* base, size_t nTensors,
                            unsigned E, u64 dstCapacity, hipStream_t s)
{
    if (nTensors == 0) return hipSuccess;
    launch_planes_verdicts(results, dstOff, planeSizes, nTensors, E, dstCapacity, s);
    if (dstCapacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(dstCapacity, nTensors)), b(PL_THREADS);
    if (E == 1) hipLaunchKernelGGL(k_planes_merge_xor<1>, g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, nTensors, dstCapacity);
    else if (E == 2) hipLaunchKernelGGL(k_planes_merge_xor<2>, g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, nTensors, dstCapacity);
    else if (E == 4) hipLaunchKernelGGL(k_planes_merge_xor<4>, g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, nTensors, dstCapacity);
    else hipLaunchKernelGGL(k_planes_merge_xor<8>, g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, nTensors, dstCapacity);
    return hipGetLastError();
}

extern "C" int FSEHIP_planes_split_xor_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const void* d_base,
                                              const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity, void* stream)
{
    if (bad_elem(elemBytes) || !d_planes || !d_planeOffsets || !d_tensorResults || !d_src || !d_base || !d_srcOffsets) return (int)hipErrorInvalidValue;
    if (nTensors >= ((size_t)1 << 31) / elemBytes || bad_grid(capacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_split_xor((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u8*)d_base, (const u64*)d_srcOffsets, nTensors, elemBytes,
                                 capacity, (hipStream_t)stream);
}

extern "C" int FSEHIP_planes_merge_xor_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                              const size_t* d_planeSizes, const void* d_base, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_planes || !d_planeOffsets || !d_planeSizes || !d_base) return (int)hipErrorInvalidValue;
    if (nTensors >= ((size_t)1 << 31) / elemBytes || bad_grid(dstCapacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_merge_xor((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, (const u8*)d_base,
                                 nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}

extern "C" int FSEHIP_tensor_compress_delta_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                   const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                   uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, unsigned slotAlignLog,
                                                   void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes, void* stream)
{
    // the argument checks of both steps in front of the first launch, as FSEHIP_tensor_compress_dbatch has them
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_base || !d_srcOffsets || !d_planeOffsets || !d_planes)
        return (int)hipErrorInvalidValue;
    if (nTensors >= ((size_t)1 << 31) / elemBytes || bad_grid(capacity, nTensors)) return (int)hipErrorInvalidValue;
    if (blockSizeId > 6 || (codec != 0 && codec != 1) || slotAlignLog > 12 || ((uintptr_t)d_workspace & 255u) || maxTotalBlocks >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const size_t nFrames = nTensors * elemBytes;
    if (workspaceBytes < FSEHIP_frame_compress_packed_dbatch_workspaceSize(nFrames, maxTotalBlocks, blockSizeId, codec)) return (int)hipErrorInvalidValue;
    const hipError_t e = launch_split_xor((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u8*)d_base, (const u64*)d_srcOffsets, nTensors,
                                          elemBytes, capacity, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return FSEHIP_frame_compress_packed_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_planes, d_planeOffsets, nFrames, maxTotalBlocks, blockSizeId, codec,
                                               slotAlignLog, d_workspace, workspaceBytes, stream);
}

// the plain (d_base == nullptr) or the XOR split, then the packed writer with a codec per plane; the argument checks of both steps in front
// of the first launch
extern "C" int FSEHIP_tensor_compress_mixed_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                   const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                   uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, uint8_t* d_codecs, int policy,
                                                   unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets,
                                                   void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_srcOffsets || !d_planeOffsets || !d_codecs ||
        ((elemBytes > 1 || d_base) && !d_planes))
        return (int)hipErrorInvalidValue;
    if (nTensors >= ((size_t)1 << 31) / elemBytes || bad_grid(capacity, nTensors)) return (int)hipErrorInvalidValue;
    if (blockSizeId > 6 || (policy != FSEHIP_CODECS_GIVEN && policy != FSEHIP_CODECS_CHOOSE) || (policy == FSEHIP_CODECS_CHOOSE && tolerancePermille > 1000) ||
        slotAlignLog > 12 || ((uintptr_t)d_workspace & 255u) || maxTotalBlocks >= ((size_t)1 << 31))
        return (int)hipErrorInvalidValue;
    const size_t nFrames = nTensors * elemBytes;
    if (workspaceBytes < FSEHIP_frame_mixedWorkspaceBound(nFrames, maxTotalBlocks, blockSizeId, policy)) return (int)hipErrorInvalidValue;
    const hipError_t e = d_base ? launch_split_xor((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u8*)d_base, (const u64*)d_srcOffsets,
                                                   nTensors, elemBytes, capacity, (hipStream_t)stream)
                                : launch_planes_split((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u64*)d_srcOffsets, nTensors, elemBytes,
                                                      capacity, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return FSEHIP_frame_compress_packed_mixed_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, !d_base && elemBytes == 1 ? d_src : d_planes, d_planeOffsets,
                                                     nFrames, maxTotalBlocks, blockSizeId, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes,
                                                     stream);
}

extern "C" int FSEHIP_tensor_decompress_delta_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, size_t* d_results,
                                                     const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks,
                                                     void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                                     void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_base || !d_results || !d_frames || !d_frameOffsets || !d_planes || !d_planeOffsets || !d_planeResults)
        return (int)hipErrorInvalidValue;
    if (nTensors >= ((size_t)1 << 31) / elemBytes || bad_grid(dstCapacity, nTensors)) return (int)hipErrorInvalidValue;
    if (((uintptr_t)d_workspace & 255u) || maxTotalBlocks >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const size_t nFrames = nTensors * elemBytes;
    if (workspaceBytes < FSEHIP_frame_decompress_packed_dbatch_workspaceSize(nFrames, maxTotalBlocks)) return (int)hipErrorInvalidValue;
    const int e = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_planeOffsets, d_planeResults, d_frames, d_frameOffsets, nFrames, maxTotalBlocks, 0,
                                                        d_workspace, workspaceBytes, stream);
    if (e != 0) return e;
    return (int)launch_merge_xor((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeResults, (const u8*)d_base,
                                 nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}

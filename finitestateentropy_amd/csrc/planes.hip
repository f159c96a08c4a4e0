// planes.hip -- tensors of 2-, 4- and 8-byte elements as BYTE PLANES (fsehip.h, "byte planes of tensors"): plane p of a tensor holds byte p of
// every element, the planes of a tensor lie back to back where the tensor lies, and every plane becomes one .fse frame (frame_dev.hip).  An
// order-0 coder then sees the exponent bytes and the mantissa bytes of a bf16 tensor in histograms of their own.  Kernel launches only.
//
//   FSEHIP_planes_split_dbatch     : k_planes_offsets (per tensor: its plane offsets in closed form, its result) -> k_planes_split
//   FSEHIP_planes_merge_dbatch     : k_planes_verdicts (per tensor: its result) -> k_planes_merge
//   FSEHIP_tensor_compress_dbatch  : the split -> FSEHIP_frame_compress_packed_dbatch over the planes (the plane offsets are its source offsets)
//   FSEHIP_tensor_decompress_dbatch: FSEHIP_frame_decompress_packed_dbatch into the planes buffer -> the merge over the offsets and results it leaves
// (The device helpers all of them are made of are in planes_dev.h, shared with the XOR forms of planes_delta.hip.)
//
// The two data kernels are bandwidth kernels (n bytes in, n bytes out) over ragged tensors, with no workspace and no scan: the flat byte axis
// is cut into tiles of PLANES_TILE bytes, ceil(capacity / T) + nTensors workgroups are launched, and workgroup w looks up -- a binary search
// over the offsets -- the largest i with floor(S[i] / T) + i <= w and takes tile t = w - i of tensor i.  That key is strictly increasing in i,
// and the keys of the tiles a tensor touches, floor(S[i] / T) + i .. floor((S[i+1] - 1) / T) + i, end below the next tensor's key plus one:
// every (tile, tensor) intersection has exactly one workgroup, however many small or empty tensors share a tile; a workgroup whose
// intersection is empty returns.  An element belongs to the tile its first byte lies in.
// Inside its intersection a workgroup gives every lane 16 consecutive elements at a time: E loads of 16 bytes, the byte shuffle (v_perm_b32:
// log2(E) rounds of "even bytes / odd bytes" over the lane's 4 E dwords, one permute per dword and round), E stores of 16 bytes, one per
// plane, consecutive lanes at consecutive addresses.  The chunks start where plane 0 (split) or the tensor (merge) reaches a 16-byte boundary;
// the elements in front of the first chunk and behind the last one -- fewer than 32, the partial last element of a tensor whose size is no
// multiple of E among them -- go bytewise.  Sources at any alignment (unaligned 16-byte loads, as k_hist and k_xxh32 take theirs).
#include "planes_dev.h"

namespace {
// ---- split -------------------------------------------------------------------------------------------------------------------------------
// per tensor (and one thread more for the last entry): its E plane offsets and its result.  Offsets are monotone, so the tensors behind the
// capacity are a suffix: all their entries collapse onto the start of the first of them
__global__ void k_planes_offsets(u64* P, size_t* res, const u64* S, size_t nT, u32 E, u64 capacity)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nT) return;
    size_t lo = 0, hi = nT;                                      // the smallest j with S[j + 1] > capacity, nT without one
    while (lo < hi) { const size_t mid = lo + ((hi - lo) >> 1); if (S[mid + 1] > capacity) hi = mid; else lo = mid + 1; }
    const size_t bad = lo;
    if (i == nT) { P[nT * E] = S[bad]; return; }
    if (i >= bad) {
        const u64 at = S[bad];
        for (u32 p = 0; p < E; ++p) P[i * E + p] = at;
        res[i] = FERR(GENERIC);
        return;
    }
    const u64 s0 = S[i], s1 = S[i + 1], n = s1 > s0 ? s1 - s0 : 0;
    for (u32 p = 0; p < E; ++p) P[i * E + p] = s0 + pl_start(n, p, E);
    res[i] = (size_t)n;
}
template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split(u8* planes, const u8* src, const u64* S, size_t nT, u64 capacity)
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
    const PlShare h = pl_share<E>(s0, n, lo, (u64)(uintptr_t)pb, 1);
    for (u64 c = tid; c < h.nch; c += PL_THREADS) {
        const u64 e = h.eb + 16 * c;
        u32 wv[4 * E], o[E][4];
#pragma unroll
        for (int k = 0; k < E; ++k) __builtin_memcpy(&wv[4 * k], sb + e * E + 16 * k, 16);
        pl_deinterleave<E>(wv, o);
#pragma unroll
        for (int p = 0; p < E; ++p) __builtin_memcpy(pb + pl_start(n, p, E) + e, o[p], 16);
    }
    // head and tail, a byte per thread: byte k of the tensor is byte k / E of plane k % E
    const u64 nHead = (h.eb - h.e0) * E, nTail = (h.e1 - h.et) * E;
    for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) {
        const u64 k = j < nHead ? h.e0 * E + j : h.et * E + (j - nHead);
        if (k < n) pb[pl_start(n, (u32)(k % E), E) + k / E] = sb[k];
    }
}

// ---- merge -------------------------------------------------------------------------------------------------------------------------------
__global__ void k_planes_verdicts(size_t* res, const u64* D, const size_t* PS, size_t nT, u32 E, u64 dstCapacity)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nT) res[i] = pm_verdict(D, PS, i, E, dstCapacity);
}
template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_merge(u8* dst, const u64* D, const u8* planes, const u64* PO, const size_t* PS, size_t nT, u64 dstCapacity)
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
        for (int k = 0; k < E; ++k) __builtin_memcpy(db + e * E + 16 * k, &wv[4 * k], 16);
    }
    const u64 nHead = (h.eb - h.e0) * E, nTail = (h.e1 - h.et) * E;
    for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) {
        const u64 k = j < nHead ? h.e0 * E + j : h.et * E + (j - nHead);
        if (k < n) db[k] = planes[PO[i * E + k % E] + k / E];
    }
}

}   // namespace

// the two per-tensor kernels on their own: the XOR forms (planes_delta.hip) launch them in front of data kernels of their own
void launch_planes_offsets(u64* planeOff, size_t* tensorRes, const u64* srcOff, size_t nTensors, unsigned E, u64 capacity, hipStream_t s)
{
    hipLaunchKernelGGL(k_planes_offsets, dim3(grid_for(nTensors + 1)), dim3(PL_THREADS), 0, s, planeOff, tensorRes, srcOff, nTensors, (u32)E, capacity);
}
void launch_planes_verdicts(size_t* results, const u64* dstOff, const size_t* planeSizes, size_t nTensors, unsigned E, u64 dstCapacity, hipStream_t s)
{
    hipLaunchKernelGGL(k_planes_verdicts, dim3(grid_for(nTensors)), dim3(PL_THREADS), 0, s, results, dstOff, planeSizes, nTensors, (u32)E, dstCapacity);
}

hipError_t launch_planes_split(u8* planes, u64* planeOff, size_t* tensorRes, const u8* src, const u64* srcOff, size_t nTensors, unsigned E, u64 capacity, hipStream_t s)
{
    launch_planes_offsets(planeOff, tensorRes, srcOff, nTensors, E, capacity, s);
    if (E == 1 || nTensors == 0 || capacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(capacity, nTensors)), b(PL_THREADS);
    if (E == 2) hipLaunchKernelGGL(k_planes_split<2>, g, b, 0, s, planes, src, srcOff, nTensors, capacity);
    else if (E == 4) hipLaunchKernelGGL(k_planes_split<4>, g, b, 0, s, planes, src, srcOff, nTensors, capacity);
    else hipLaunchKernelGGL(k_planes_split<8>, g, b, 0, s, planes, src, srcOff, nTensors, capacity);
    return hipGetLastError();
}

hipError_t launch_planes_merge(u8* dst, const u64* dstOff, size_t* results, const u8* planes, const u64* planeOff, const size_t* planeSizes, size_t nTensors, unsigned E,
                               u64 dstCapacity, hipStream_t s)
{
    if (nTensors == 0) return hipSuccess;
    launch_planes_verdicts(results, dstOff, planeSizes, nTensors, E, dstCapacity, s);
    if (dstCapacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(dstCapacity, nTensors)), b(PL_THREADS);
    if (E == 1) hipLaunchKernelGGL(k_planes_merge<1>, g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, nTensors, dstCapacity);
    else if (E == 2) hipLaunchKernelGGL(k_planes_merge<2>, g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, nTensors, dstCapacity);
    else if (E == 4) hipLaunchKernelGGL(k_planes_merge<4>, g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, nTensors, dstCapacity);
    else hipLaunchKernelGGL(k_planes_merge<8>, g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, nTensors, dstCapacity);
    return hipGetLastError();
}

extern "C" size_t FSEHIP_planes_blockBound(size_t totalBytes, size_t nTensors, unsigned elemBytes, unsigned blockSizeId)
{
    if (blockSizeId > 6 || bad_elem(elemBytes)) return FSEHIP_ERROR(GENERIC);
    const size_t bs = (size_t)1024 << blockSizeId;
    return totalBytes / bs + (totalBytes % bs ? 1 : 0) + nTensors * elemBytes;
}

extern "C" int FSEHIP_planes_split_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const uint64_t* d_srcOffsets,
                                          size_t nTensors, unsigned elemBytes, uint64_t capacity, void* stream)
{
    if (bad_elem(elemBytes) || !d_planeOffsets || !d_tensorResults || !d_srcOffsets || (elemBytes > 1 && (!d_planes || !d_src))) return (int)hipErrorInvalidValue;
    if (nTensors >= ((size_t)1 << 31) / elemBytes || bad_grid(capacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_split((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u64*)d_srcOffsets, nTensors, elemBytes, capacity,
                                    (hipStream_t)stream);
}

extern "C" int FSEHIP_planes_merge_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                          const size_t* d_planeSizes, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_planes || !d_planeOffsets || !d_planeSizes) return (int)hipErrorInvalidValue;
    if (nTensors >= ((size_t)1 << 31) / elemBytes || bad_grid(dstCapacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_merge((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, nTensors, elemBytes,
                                    dstCapacity, (hipStream_t)stream);
}

extern "C" int FSEHIP_tensor_compress_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                             const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                             size_t maxTotalBlocks, unsigned blockSizeId, int codec, unsigned slotAlignLog,
                                             void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes, void* stream)
{
    // the argument checks of both steps, as they stand today, in front of the first launch (fsehip.h: what the guarantee covers)
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_srcOffsets || !d_planeOffsets || (elemBytes > 1 && !d_planes))
        return (int)hipErrorInvalidValue;
    if (nTensors >= ((size_t)1 << 31) / elemBytes || bad_grid(capacity, nTensors)) return (int)hipErrorInvalidValue;
    if (blockSizeId > 6 || (codec != 0 && codec != 1) || slotAlignLog > 12 || ((uintptr_t)d_workspace & 255u) || maxTotalBlocks >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const size_t nFrames = nTensors * elemBytes;
    if (workspaceBytes < FSEHIP_frame_compress_packed_dbatch_workspaceSize(nFrames, maxTotalBlocks, blockSizeId, codec)) return (int)hipErrorInvalidValue;
    const hipError_t e = launch_planes_split((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u64*)d_srcOffsets, nTensors, elemBytes, capacity,
                                             (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return FSEHIP_frame_compress_packed_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, elemBytes == 1 ? d_src : d_planes, d_planeOffsets, nFrames, maxTotalBlocks,
                                               blockSizeId, codec, slotAlignLog, d_workspace, workspaceBytes, stream);
}

extern "C" int FSEHIP_tensor_decompress_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results,
                                               const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks,
                                               void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                               void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_frames || !d_frameOffsets || !d_planes || !d_planeOffsets || !d_planeResults)
        return (int)hipErrorInvalidValue;
    if (nTensors >= ((size_t)1 << 31) / elemBytes || bad_grid(dstCapacity, nTensors)) return (int)hipErrorInvalidValue;
    if (((uintptr_t)d_workspace & 255u) || maxTotalBlocks >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const size_t nFrames = nTensors * elemBytes;
    if (workspaceBytes < FSEHIP_frame_decompress_packed_dbatch_workspaceSize(nFrames, maxTotalBlocks)) return (int)hipErrorInvalidValue;
    const int e = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_planeOffsets, d_planeResults, d_frames, d_frameOffsets, nFrames, maxTotalBlocks, 0,
                                                        d_workspace, workspaceBytes, stream);
    if (e != 0) return e;
    return (int)launch_planes_merge((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeResults, nTensors, elemBytes,
                                    dstCapacity, (hipStream_t)stream);
}

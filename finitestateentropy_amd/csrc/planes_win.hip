// planes_win.hip -- WINDOWS OF SEGMENTED TENSORS (fsehip.h, "windows of segmented tensors"): an element range [a, b) of every tensor of a
// segmented batch, decoding only the segment frames that hold it.  No frame byte and no reader changes: a frame reader stops at the end mark,
// so the selected frames go to the packed reader as extents that run to the next selected frame, whole unselected frames included; and for a
// window of whole elements every plane contributes the same plane-relative range, so the (XOR) merge of planes.hip runs
// unchanged over plane offsets moved to the window's first byte.  Kernel launches only.
//
//   FSEHIP_planes_windowFirst              : host arithmetic, the first selected frame of every plane and the exact block count of the selection
//   FSEHIP_planes_select_window_dbatch     : k_planes_select -- per selected frame the offset of its extent in the frames buffer
//   FSEHIP_planes_fold_window_dbatch       : k_planes_fold_window -- per plane (one wave) where the window starts and the verdict of its segments
//   FSEHIP_tensor_decompress_window_dbatch : the selection -> the packed reader over the extents -> the fold -> the (XOR) merge
#include "planes_dev.h"

namespace {
// One thread per entry r <= nSel.  The plane j that holds selected frame r is the largest j < nP with WF[j] <= r (the search of
// k_planes_segments), its frame q = SF[j] + k0 + (r - WF[j]); the last entry is the end of the last selected frame, F[q + 1].  The entries
// of a refused tensor are all F[SF[(i + 1) * E]].  Every value read from SF, WF and W is clamped before it indexes: q to nSeg, the segment
// inside the plane to the window's count.
__global__ void k_planes_select(u64* SO, const u64* F, const u64* S, const u64* W, const u64* SF, const u64* WF, size_t nT, u32 E, size_t nSeg, size_t nSel, u32 segLog)
{
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nP = nT * E;
    if (r > nSel) return;
    if (nSel == 0 || nP == 0) { SO[r] = F[0]; return; }
    const size_t at = r < nSel ? r : nSel - 1;
    const size_t j = pl_last_le(nP, at, [WF](size_t m) { return WF[m]; }), i = j / E;
    const PwWin w = pw_window(S, W, SF, WF, i, E, segLog, nSel);
    u64 q;
    if (!w.ok) q = SF[(i + 1) * E];
    else {
        const u64 f = WF[j];
        u64 k = at >= f ? at - f : 0;
        if (k >= w.cnt) k = w.cnt ? w.cnt - 1 : 0;
        q = SF[j] + w.k0 + k + (r == nSel ? 1 : 0);
    }
    SO[r] = F[q < nSeg ? q : nSeg];
}

// One wave per plane, its lanes striding over the plane's selected segments (ps_fold, as k_planes_fold); the verdict in the order of
// fsehip.h.  The size rule: a selected segment regenerates exactly its bytes of the plane.  Whether the tensor is accepted and its window
// empty is the same for all lanes; behind that, q0 + cnt <= nSel.
__global__ __launch_bounds__(PL_THREADS) void k_planes_fold_window(u64* PO, size_t* PS, const u64* off, const size_t* res, const u64* S, const u64* W, const u64* SF,
                                                                   const u64* WF, size_t nT, u32 E, size_t nSel, u32 segLog)
{
    const size_t j = (size_t)blockIdx.x * (PL_THREADS / WAVE) + (threadIdx.x / WAVE);
    if (j >= nT * E) return;                                      // (uniform over the wave)
    const u32 lane = threadIdx.x % WAVE;
    const size_t i = j / E;
    const PwWin w = pw_window(S, W, SF, WF, i, E, segLog, nSel);
    if (!w.ok || w.cnt == 0) {
        if (!lane) { PO[j] = 0; PS[j] = w.ok ? 0 : FERR(GENERIC); }
        return;
    }
    const u64 s0 = S[i], s1 = S[i + 1], sz = pl_size(s1 > s0 ? s1 - s0 : 0, (u32)(j % E), E), seg = (u64)1 << segLog;
    const u64 q0 = WF[j];
    const PsFold f = ps_fold(off + q0, res + q0, w.cnt, lane, [=](u64 t, u64 r) {
        const u64 at = (w.k0 + t) << segLog;                      // (an accepted tensor: at < b <= sz)
        return r == (sz - at < seg ? sz - at : seg);
    });
    if (lane) return;
    const bool good = f.firstErr == 0xFFFFFFFFu && !f.bad;
    PO[j] = good ? off[q0] + (w.a - (w.k0 << segLog)) : 0;
    PS[j] = f.firstErr != 0xFFFFFFFFu ? res[q0 + f.firstErr] : f.bad ? FERR(corruption_detected) : (size_t)(w.b - w.a);
}

hipError_t launch_select(u64* selFrameOff, const u64* frameOff, const u64* srcOff, const u64* windows, const u64* segFirst, const u64* selFirst, size_t nTensors, unsigned E,
                         size_t nSeg, size_t nSel, unsigned segLog, hipStream_t s)
{
    hipLaunchKernelGGL(k_planes_select, dim3(grid_for(nSel + 1)), dim3(PL_THREADS), 0, s, selFrameOff, frameOff, srcOff, windows, segFirst, selFirst, nTensors, (u32)E, nSeg,
                       nSel, (u32)segLog);
    return hipGetLastError();
}
hipError_t launch_fold_window(u64* planeOff, size_t* planeSizes, const u64* selOff, const size_t* selRes, const u64* srcOff, const u64* windows, const u64* segFirst,
                              const u64* selFirst, size_t nTensors, unsigned E, size_t nSel, unsigned segLog, hipStream_t s)
{
    if (nTensors == 0) return hipSuccess;
    const size_t perGroup = PL_THREADS / WAVE, nPlanes = nTensors * E;
    hipLaunchKernelGGL(k_planes_fold_window, dim3((unsigned)((nPlanes + perGroup - 1) / perGroup)), dim3(PL_THREADS), 0, s, planeOff, planeSizes, selOff, selRes, srcOff,
                       windows, segFirst, selFirst, nTensors, (u32)E, nSel, (u32)segLog);
    return hipGetLastError();
}
}   // namespace

extern "C" size_t FSEHIP_planes_windowFirst(uint64_t* h_selFirst, size_t* h_maxBlocks, const uint64_t* h_offsets, const uint64_t* h_windows, size_t nTensors,
                                            unsigned elemBytes, unsigned segLog, unsigned blockSizeId)
{
    if (bad_elem(elemBytes) || blockSizeId > 6 || bad_seg(segLog, blockSizeId) || (nTensors && (!h_offsets || !h_windows))) return FSEHIP_ERROR(GENERIC);
    const u32 E = elemBytes;
    const u64 seg = (u64)1 << segLog, bsLog = 10 + blockSizeId, bs = (u64)1 << bsLog;
    u64 total = 0, blocks = 0;
    if (h_selFirst) h_selFirst[0] = 0;
    for (size_t i = 0; i < nTensors; ++i) {
        const u64 s0 = h_offsets[i], s1 = h_offsets[i + 1], n = s1 > s0 ? s1 - s0 : 0, a = h_windows[2 * i], b = h_windows[2 * i + 1];
        if (a > b || b > n / E) return FSEHIP_ERROR(GENERIC);
        const PwRange r = pw_range(a, b, true, segLog);
        for (u32 p = 0; p < E; ++p) {
            if (r.cnt) {                                         // all selected segments but the last are full; the last one ends where the plane or the segment does
                const u64 last = pl_size(n, p, E) - ((r.k0 + r.cnt - 1) << segLog);
                blocks += (r.cnt - 1) * (seg >> bsLog) + ((last < seg ? last : seg) + bs - 1) / bs;
            }
            total += r.cnt;
            if (total >= ((u64)1 << 31) || blocks >= ((u64)1 << 31)) return FSEHIP_ERROR(GENERIC);
            if (h_selFirst) h_selFirst[i * E + p + 1] = total;
        }
    }
    if (h_maxBlocks) *h_maxBlocks = (size_t)blocks;
    return (size_t)total;
}

extern "C" int FSEHIP_planes_select_window_dbatch(uint64_t* d_selFrameOffsets, const uint64_t* d_frameOffsets, const uint64_t* d_srcOffsets, const uint64_t* d_windows,
                                                  const uint64_t* d_segFirst, const uint64_t* d_selFirst, size_t nTensors, unsigned elemBytes, size_t nSegments,
                                                  size_t nSelected, unsigned segLog, void* stream)
{
    if (bad_elem(elemBytes) || bad_seg(segLog, 0) || !d_selFrameOffsets || !d_frameOffsets || !d_srcOffsets || !d_windows || !d_segFirst || !d_selFirst)
        return (int)hipErrorInvalidValue;
    if (bad_counts(nTensors, elemBytes, nSelected) || nSegments >= ((size_t)1 << 31) || nSelected > nSegments) return (int)hipErrorInvalidValue;
    return (int)launch_select((u64*)d_selFrameOffsets, (const u64*)d_frameOffsets, (const u64*)d_srcOffsets, (const u64*)d_windows, (const u64*)d_segFirst,
                              (const u64*)d_selFirst, nTensors, elemBytes, nSegments, nSelected, segLog, (hipStream_t)stream);
}

extern "C" int FSEHIP_planes_fold_window_dbatch(uint64_t* d_planeOffsets, size_t* d_planeSizes, const uint64_t* d_selOffsets, const size_t* d_selResults,
                                                const uint64_t* d_srcOffsets, const uint64_t* d_windows, const uint64_t* d_segFirst, const uint64_t* d_selFirst,
                                                size_t nTensors, unsigned elemBytes, size_t nSelected, unsigned segLog, void* stream)
{
    if (bad_elem(elemBytes) || bad_seg(segLog, 0) || !d_planeOffsets || !d_planeSizes || !d_selOffsets || !d_selResults || !d_srcOffsets || !d_windows || !d_segFirst ||
        !d_selFirst)
        return (int)hipErrorInvalidValue;
    if (bad_counts(nTensors, elemBytes, nSelected)) return (int)hipErrorInvalidValue;
    return (int)launch_fold_window((u64*)d_planeOffsets, d_planeSizes, (const u64*)d_selOffsets, d_selResults, (const u64*)d_srcOffsets, (const u64*)d_windows,
                                   (const u64*)d_segFirst, (const u64*)d_selFirst, nTensors, elemBytes, nSelected, segLog, (hipStream_t)stream);
}

extern "C" int FSEHIP_tensor_decompress_window_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, size_t* d_results,
                                                      const void* d_frames, const uint64_t* d_frameOffsets, const uint64_t* d_srcOffsets, const uint64_t* d_windows,
                                                      size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog,
                                                      const uint64_t* d_selFirst, size_t nSelected, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                                                      uint64_t* d_selFrameOffsets, uint64_t* d_selOffsets, size_t* d_selResults, uint64_t* d_planeOffsets,
                                                      size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream)
{
    return FSEHIP_tensor_decompress_window_op_dbatch(d_dst, d_dstOffsets, dstCapacity, d_base, FSEHIP_DELTA_XOR, d_results, d_frames, d_frameOffsets, d_srcOffsets, d_windows,
                                                     nTensors, elemBytes, d_segFirst, nSegments, segLog, d_selFirst, nSelected, maxTotalBlocks, d_planes, planesCapacity,
                                                     d_selFrameOffsets, d_selOffsets, d_selResults, d_planeOffsets, d_planeSizes, d_workspace, workspaceBytes, stream);
}
// the argument checks of all four steps in front of the first launch
extern "C" int FSEHIP_tensor_decompress_window_op_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp,
                                                         size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, const uint64_t* d_srcOffsets,
                                                         const uint64_t* d_windows, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments,
                                                         unsigned segLog, const uint64_t* d_selFirst, size_t nSelected, size_t maxTotalBlocks, void* d_planes,
                                                         uint64_t planesCapacity, uint64_t* d_selFrameOffsets, uint64_t* d_selOffsets, size_t* d_selResults,
                                                         uint64_t* d_planeOffsets, size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_op(deltaOp) || bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_frames || !d_frameOffsets || !d_srcOffsets || !d_windows || !d_segFirst || !d_selFirst ||
        !d_planes || !d_selFrameOffsets || !d_selOffsets || !d_selResults || !d_planeOffsets || !d_planeSizes)
        return (int)hipErrorInvalidValue;
    if (bad_seg(segLog, 0) || bad_counts(nTensors, elemBytes, nSelected) || nSegments >= ((size_t)1 << 31) || nSelected > nSegments || bad_grid(dstCapacity, nTensors))
        return (int)hipErrorInvalidValue;
    if (bad_reader(d_workspace, workspaceBytes, nSelected, maxTotalBlocks)) return (int)hipErrorInvalidValue;
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = launch_select((u64*)d_selFrameOffsets, (const u64*)d_frameOffsets, (const u64*)d_srcOffsets, (const u64*)d_windows, (const u64*)d_segFirst,
                                 (const u64*)d_selFirst, nTensors, elemBytes, nSegments, nSelected, segLog, s);
    if (e != hipSuccess) return (int)e;
    const int r = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_selOffsets, d_selResults, d_frames, d_selFrameOffsets, nSelected, maxTotalBlocks,
                                                        0, d_workspace, workspaceBytes, stream);
    if (r != 0) return r;
    e = launch_fold_window((u64*)d_planeOffsets, d_planeSizes, (const u64*)d_selOffsets, d_selResults, (const u64*)d_srcOffsets, (const u64*)d_windows,
                           (const u64*)d_segFirst, (const u64*)d_selFirst, nTensors, elemBytes, nSelected, segLog, s);
    if (e != hipSuccess) return (int)e;
    return (int)launch_planes_merge((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, (const u8*)d_base,
                                    deltaOp, nTensors, elemBytes, dstCapacity, s);
}

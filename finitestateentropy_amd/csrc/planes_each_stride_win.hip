// planes_each_stride_win.hip -- WINDOWS AND PATCHES OF TENSORS WITH A STRIDE PER TENSOR (fsehip.h, the section of that name): the window forms
// of planes_each.hip with, beside the transform byte of tensor i, the stride byte of planes_each_stride.hip, read where that transform is
// FSEHIP_EST_PRED.  Kernel launches only; the C calls are in capi_each.hip (the read side) and planes_patch.hip (the write side).
//
//   launch_planes_merge_window_each_stride : k_planes_verdicts (planes.hip) -> k_each_stride_refuse_window -> k_planes_merge_window_each_stride
//   launch_planes_split_window_each_stride : k_each_stride_stage_offsets -> k_planes_split_window_each_stride
// Without a stride array both are the launchers of planes_each.hip.  The kernels stand in a source of their own, so that the device code of
// planes_each.hip and planes_each_stride.hip stays what it was, byte for byte.
//
// THE WINDOW FORM OF THE MERGE is the WIN form of k_planes_merge_each with the stride's switch of k_planes_merge_each_stride: the key
// floor(D[j] / T) + 2 j, ceil(dstCapacity / T) + 2 nTensors workgroups, pe_win_ok as it is.  A run is PP_RUN elements counted from the
// TENSOR's start at every stride, and element j lies in chain (j mod PP_RUN) mod S: the lead of a window [a, b) is L = a mod PP_RUN whatever
// the stride, the virtual tensor that starts L elements in front of the slot starts on a run, and its runs AND its chains are the tensor's
// own.  ps_merge<E, S, true> sums all S chains through the lead -- a lead below S, or no multiple of S, leaves the chains at different
// lengths, which the per-chain scans do not notice -- and stores from L on.  PLAIN, XOR, SUB and PRED at stride 1 are pe_merge<..., true>.
// The one extra tile: L E <= 1023 * 8 < T, as in planes_each.hip.
//
// THE WINDOW FORM OF THE SPLIT is the frame of k_planes_split_window_each around pe_split and ps_split<E, S>.  The staged sub-tensor starts
// at a multiple of seg = 1 << segLog >= PP_RUN elements, so it starts a run FOR EVERY CHAIN: the first S elements of a run are predicted by
// 0, ps_prev and ps_elem_split read nothing in front of a run start, and the planes of the strided transform of the sub-tensor are segments
// k0 .. k1 of those of the tensor.  No lead, no LDS, no workspace.
//
// REFUSALS: those of the window forms of planes_each.hip with pes_ok in place of pe_ok: a PRED tensor whose stride byte is 0 or above
// FSEHIP_PRED_MAX_STRIDE gets GENERIC for that tensor alone, and the data kernels return for it in front of every load and store.  The
// stride byte of a tensor under another transform is not read.
#include "planes_dev.h"

namespace {
// behind k_planes_verdicts, whose verdict of tensor i stands in res[i]: an error there stays unless the transform or the stride is refused
__global__ void k_each_stride_refuse_window(size_t* res, const u8* T, const u8* ST, const u8* base, const u64* W, const u64* PO, size_t nT, u32 E)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nT) return;
    const size_t v = res[i];
    const u32 tr = T[i];
    u64 L;
    if (!pes_ok(tr, pes_stride(tr, ST, i), base) || (!is_err(v) && !pe_win_ok(W, PO, i, E, tr, (u64)v, L))) res[i] = FERR(GENERIC);
}

// ---- the window merge --------------------------------------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_merge_window_each_stride(u8* dst, const u64* D, const u8* planes, const u64* PO, const size_t* PS, const u8* base,
                                                                                const u8* T, const u8* ST, size_t nT, u64 dstCapacity, const u64* W)
{
    const u64 w = blockIdx.x;
    if (nT == 0 || (D[0] >> PL_TILE_LOG) > w) return;             // (uniform, like every return below)
    const size_t i = pl_last_le(nT, w, [D](size_t j) { return (D[j] >> PL_TILE_LOG) + 2 * j; });   // one more item per tensor
    const u64 d0 = D[i], first = (d0 >> PL_TILE_LOG) + 2 * i;
    if (first > w) return;                                        // (offsets that decrease: the search found no tensor of this item)
    const u64 t = w - first;
    const u32 tr = T[i], st = pes_stride(tr, ST, i);
    if (!pes_ok(tr, st, base)) return;                            // (a refused tensor: in place its old bytes stay)
    const size_t v = pm_verdict(D, PS, i, E, dstCapacity);
    u64 L;
    if (is_err(v) || !pe_win_ok(W, PO, i, E, tr, (u64)v, L)) return;
    const u64 nv = (u64)v + L * E;                                // the virtual tensor (an empty window: 0 bytes)
    if ((t << PL_TILE_LOG) >= nv) return;
    u8* const db = (u8*)((uintptr_t)(dst + d0) - L * E);          // where virtual element 0 would lie; nothing below dst + d0 is written
    const u64* const P = PO + i * E;
    if (tr == FSEHIP_EST_PLAIN) pe_merge<E, FSEHIP_EST_PLAIN, true>(db, nullptr, planes, P, nv, t, L);
    else if (tr == FSEHIP_EST_XOR) pe_merge<E, FSEHIP_EST_XOR, true>(db, base + d0, planes, P, nv, t, L);
    else if (tr == FSEHIP_EST_SUB) pe_merge<E, FSEHIP_EST_SUB, true>(db, base + d0, planes, P, nv, t, L);
    else if (st == 1) pe_merge<E, FSEHIP_EST_PRED, true>(db, nullptr, planes, P, nv, t, L);
    else ps_for_stride(st, [&](auto sc) { ps_merge<E, decltype(sc)::value, true>(db, planes, P, nv, t, L); });
}

// ---- the window split (the patch's stage) ------------------------------------------------------------------------------------------------
// k_each_stage_offsets (planes_each.hip) with one more cause in its rule 1, the stride of a PRED tensor
__global__ void k_each_stride_stage_offsets(u64* P, size_t* res, const u8* TR, const u8* ST, const u8* base, const u64* S, const u64* W, const u64* T, size_t nT, u32 E,
                                            u32 segLog, u64 capacity, u64 stageCapacity)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nT) return;
    const u64 t0 = T[i] < stageCapacity ? T[i] : stageCapacity;
    if (i == nT) { P[nT * E] = t0; return; }
    const PpStage g = pp_stage(S, W, T, i, E, segLog, capacity, stageCapacity);
    const u32 tr = TR[i];
    const bool ok = g.ok && pes_ok(tr, pes_stride(tr, ST, i), base);
    for (u32 p = 0; p < E; ++p) P[i * E + p] = ok ? t0 + pl_start(g.m, p, E) : t0;
    res[i] = ok ? (size_t)g.m : FERR(GENERIC);
}
// workgroup w takes tile w - i of the staged sub-tensor i under transform TR[i] at stride ST[i]: m bytes at src + S[i] + at, planes at stage + T[i]
template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split_window_each_stride(u8* stage, const u8* src, const u8* base, const u8* TR, const u8* ST, const u64* S,
                                                                                const u64* W, const u64* T, size_t nT, u32 segLog, u64 capacity, u64 stageCapacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(T, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 t0 = T[i], t1 = T[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(t0 < t1) || lo >= t1 || lo + PLANES_TILE <= t0) return;
    const u32 tr = TR[i], st = pes_stride(tr, ST, i);
    if (!pes_ok(tr, st, base)) return;                            // (a refused tensor: nothing of it is read or written)
    const PpStage g = pp_stage(S, W, T, i, E, segLog, capacity, stageCapacity);
    if (!g.ok) return;                                            // (accepted: t1 - t0 == m, t1 <= stageCapacity, S[i] + at + m <= S[i + 1] <= capacity)
    const u32 tid = threadIdx.x;
    const u64 at = S[i] + g.at;
    const u8* const sb = src + at;
    u8* const pb = stage + t0;
    if (tr == FSEHIP_EST_PLAIN) pe_split<E, FSEHIP_EST_PLAIN>(pb, sb, nullptr, t0, g.m, lo, tid);
    else if (tr == FSEHIP_EST_XOR) pe_split<E, FSEHIP_EST_XOR>(pb, sb, base + at, t0, g.m, lo, tid);
    else if (tr == FSEHIP_EST_SUB) pe_split<E, FSEHIP_EST_SUB>(pb, sb, base + at, t0, g.m, lo, tid);
    else if (st == 1) pe_split<E, FSEHIP_EST_PRED>(pb, sb, nullptr, t0, g.m, lo, tid);
    else ps_for_stride(st, [&](auto sc) { ps_split<E, decltype(sc)::value>(pb, sb, t0, g.m, lo, tid); });
}
}   // namespace

// strides null: stride 1 everywhere, the launcher of planes_each.hip.  Else the verdicts, the refusals with the window rules and the strides,
// then ceil(dstCapacity / T) + 2 nTensors workgroups (bad_grid with 2 nTensors)
hipError_t launch_planes_merge_window_each_stride(u8* dst, const u64* dstOff, size_t* results, const u8* planes, const u64* planeOff, const size_t* planeSizes, const u8* base,
                                                  const u8* transforms, const u8* strides, const u64* windows, size_t nTensors, unsigned E, u64 dstCapacity, hipStream_t s)
{
    if (!strides) return launch_planes_merge_window_each(dst, dstOff, results, planes, planeOff, planeSizes, base, transforms, windows, nTensors, E, dstCapacity, s);
    if (nTensors == 0) return hipSuccess;
    const hipError_t e0 = launch_planes_verdicts(results, dstOff, planeSizes, nTensors, E, dstCapacity, s);
    if (e0 != hipSuccess) return e0;
    hipLaunchKernelGGL(k_each_stride_refuse_window, dim3(grid_for(nTensors)), dim3(PL_THREADS), 0, s, results, transforms, strides, base, windows, planeOff, nTensors, (u32)E);
    if (dstCapacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(dstCapacity, 2 * nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        hipLaunchKernelGGL((k_planes_merge_window_each_stride<decltype(eb)::value>), g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, transforms, strides, nTensors,
                           dstCapacity, windows);
    });
    return hipGetLastError();
}

// strides null: the launcher of planes_each.hip.  Else the offsets kernel, which runs even for no tensors (it writes the last entry), then
// ceil(stageCapacity / T) + nTensors workgroups
hipError_t launch_planes_split_window_each_stride(u8* stage, u64* planeOff, size_t* stageRes, const u8* src, const u8* base, const u8* transforms, const u8* strides,
                                                  const u64* srcOff, const u64* windows, const u64* stageOff, size_t nTensors, unsigned E, unsigned segLog, u64 capacity,
                                                  u64 stageCapacity, hipStream_t s)
{
    if (!strides)
        return launch_planes_split_window_each(stage, planeOff, stageRes, src, base, transforms, srcOff, windows, stageOff, nTensors, E, segLog, capacity, stageCapacity, s);
    hipLaunchKernelGGL(k_each_stride_stage_offsets, dim3(grid_for(nTensors + 1)), dim3(PL_THREADS), 0, s, planeOff, stageRes, transforms, strides, base, srcOff, windows, stageOff,
                       nTensors, (u32)E, (u32)segLog, capacity, stageCapacity);
    if (nTensors == 0 || stageCapacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(stageCapacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        hipLaunchKernelGGL((k_planes_split_window_each_stride<decltype(eb)::value>), g, b, 0, s, stage, src, base, transforms, strides, srcOff, windows, stageOff, nTensors,
                           (u32)segLog, capacity, stageCapacity);
    });
    return hipGetLastError();
}

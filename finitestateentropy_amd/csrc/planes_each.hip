// planes_each.hip -- A TRANSFORM PER TENSOR (fsehip.h, "a transform per tensor"): the split and the merge of planes.hip and planes_pred.hip with
// the transform read from a device array, one byte per tensor -- FSEHIP_EST_PLAIN, _PRED, _XOR or _SUB, the ids that the estimate
// (planes_estimate.hip) writes to d_choice.  No transform of its own: the planes of tensor i are byte for byte those that the dedicated
// split writes for it under transform T[i], and the merge is that split's inverse.  Kernel launches only; the C calls are in capi_each.hip.
//
//   launch_planes_split_each : k_planes_offsets (planes.hip) -> k_each_refuse -> k_planes_split_each
//   launch_planes_merge_each : k_planes_verdicts (planes.hip) -> k_each_refuse -> k_planes_merge_each
//   launch_planes_merge_window_each : k_planes_verdicts -> k_each_refuse_window -> k_planes_merge_each<E, const u64*> (THE WINDOW FORM below)
//   launch_planes_split_window_each : k_each_stage_offsets -> k_planes_split_window_each (THE WINDOW FORM OF THE SPLIT below)
//
// THE SPLIT has the frame of k_planes_split_pred: the flat ragged mapping (a workgroup per (tile, tensor) intersection, pl_find) and chunks
// of 16 whole elements per lane counted from the TENSOR's start.  That frame serves all four: SUB and PRED need whole elements per dword,
// XOR commutes with the shuffle, and where a chunk starts changes no byte of a plane.  A workgroup has ONE tensor, so the transform is
// uniform over the workgroup -- sixty tiny tensors in a tile are sixty workgroups -- and the branch on it is taken once, in front of the
// loops: each arm is the body of the dedicated kernel, made of the same helpers (planes_dev.h).  The base's chunk is loaded in the XOR and
// SUB arms only, the predecessor element in the PRED arm only.
//
// THE MERGE has the frame of k_planes_merge_pred: tiles relative to the tensor, a workgroup owns whole runs, one run is one round of one
// wave, no LDS, no workspace.  The PRED arm is that kernel's round (all 64 lanes in the scan); the other three are element-wise in the
// same rounds.  IN PLACE (base == dst) as in the delta merge: a byte of dst is read as base and written by one thread, whose base loads
// of a chunk stand in front of its stores.  A PLAIN or PRED tensor reads no base and overwrites its bytes.
//
// THE WINDOW FORM OF THE MERGE (fsehip.h, "windows of tensors with a transform per tensor"; WIN = true of the same templates): the planes hold
// the elements [a, b) of the tensor, W[2 i] and W[2 i + 1], and PO points at the window's first byte of every plane, as the window fold of
// planes_win.hip leaves it.  PLAIN, XOR and SUB are element-wise, so a window is a tensor of its own and they run as above.  PRED sums
// differences inside runs of PP_RUN elements counted from the TENSOR's start: a window that starts inside a run needs the lead, the
// L = a mod PP_RUN differences in front of it (0 for the other three, and for an empty window, of which nothing is read).  Such a tensor is
// merged as a VIRTUAL tensor of n + L E bytes that begins L elements in front of its slot: plane pointers planes + PO - L, tiles and runs
// relative to the virtual tensor -- a run is again one round of one wave, the scan is unchanged -- and every element with virtual index
// below L is loaded and summed but never stored.  The lane whose chunk straddles L stores its elements from L on one by one.  No byte in
// front of the slot is written; the stores at db + (e - L) E are off every alignment, as they are above.
// The work mapping: the non-window key floor(D[i] / T) + i gives tensor i the items floor(D[i] / T) + i .. floor(D[i+1] / T) + i, which are
// floor(D[i+1] / T) - floor(D[i] / T) + 1 >= ceil(n / T) of them and in the worst case no more (D[i] = 0, n = T - 1: one).  The virtual
// tensor has ceil((n + L E) / T) <= ceil(n / T) + 1 tiles, because L E <= 1023 * 8 < T, so it can need one item more (E = 1, D[i] = 0,
// n = T - 1, L = 1023: 33790 bytes, two tiles).  The window key is floor(D[i] / T) + 2 i: still strictly increasing in i, tensor i owns
// the items from its key to below the next one's, floor(D[i+1] / T) - floor(D[i] / T) + 2 of them, and ceil(capacity / T) + 2 nTensors
// workgroups are launched (the last tensor: ceil(capacity / T) - floor(D[i] / T) + 2 items).  A workgroup whose tile lies behind
// n + L E returns.
//
// THE WINDOW FORM OF THE SPLIT (fsehip.h, "patching tensors with a transform per tensor"; k_planes_split_window_each): the frame of
// k_planes_split_window (planes_patch.hip) -- the STAGE offsets T are the axis, tensor i is accepted by pp_stage, its source and its base are
// displaced by S[i] + at -- around pe_split, whose chunks and runs are counted from the staged SUB-TENSOR's start.  at = k0 seg E with
// seg = 1 << segLog >= PP_RUN, so the sub-tensor starts at a multiple of PP_RUN elements of the tensor: its runs and its chunks are the
// tensor's own, the PRED arm's run-start test on the relative index is the tensor's, and no difference reads an element in front of
// src + S[i] + at.  No lead, no LDS, no workspace.  k_each_stage_offsets is k_planes_stage_offsets with the transform's refusal in rule 1.
//
// REFUSALS: a transform byte above FSEHIP_EST_SUB (the estimate's 0xFF among them), or XOR / SUB without a base: k_each_refuse writes GENERIC
// over the tensor's result, and the data kernels return for it in front of every load and store.  The window form adds (pe_win_ok): a window
// with a > b, a window whose E (b - a) is not the n of the merge's verdict, and a PRED tensor whose lead is larger than one of its plane
// offsets -- it would lie in front of the planes buffer.
#include "planes_dev.h"

namespace {
// (pe_ok, pe_win_ok and the arms pe_split and pe_merge are in planes_dev.h: planes_each_stride.hip and planes_each_stride_win.hip take the same ones)
__global__ void k_each_refuse(size_t* res, const u8* T, const u8* base, size_t nT)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nT && !pe_ok(T[i], base)) res[i] = FERR(GENERIC);
}
// behind k_planes_verdicts, whose verdict of tensor i stands in res[i]: an error there stays unless the transform is refused
__global__ void k_each_refuse_window(size_t* res, const u8* T, const u8* base, const u64* W, const u64* PO, size_t nT, u32 E)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nT) return;
    const size_t v = res[i];
    const u32 tr = T[i];
    u64 L;
    if (!pe_ok(tr, base) || (!is_err(v) && !pe_win_ok(W, PO, i, E, tr, (u64)v, L))) res[i] = FERR(GENERIC);
}

// ---- split -------------------------------------------------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split_each(u8* planes, const u8* src, const u8* base, const u8* T, const u64* S, size_t nT, u64 capacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(S, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 s0 = S[i], s1 = S[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(s0 < s1) || s1 > capacity || lo >= s1 || lo + PLANES_TILE <= s0) return;
    const u32 tr = T[i];
    if (!pe_ok(tr, base)) return;                                 // (a refused tensor: nothing of it is read or written)
    const u64 n = s1 - s0;
    const u32 tid = threadIdx.x;
    const u8* const sb = src + s0;
    u8* const pb = planes + s0;
    if (tr == FSEHIP_EST_PLAIN) pe_split<E, FSEHIP_EST_PLAIN>(pb, sb, nullptr, s0, n, lo, tid);
    else if (tr == FSEHIP_EST_PRED) pe_split<E, FSEHIP_EST_PRED>(pb, sb, nullptr, s0, n, lo, tid);
    else if (tr == FSEHIP_EST_XOR) pe_split<E, FSEHIP_EST_XOR>(pb, sb, base + s0, s0, n, lo, tid);
    else pe_split<E, FSEHIP_EST_SUB>(pb, sb, base + s0, s0, n, lo, tid);
}

// ---- the window split (the patch's stage) ----------------------------------------------------------------------------------------------------
// k_planes_stage_offsets (planes_patch.hip) with one more cause in its rule 1: per tensor (and one thread more for the last entry) its E
// staged plane offsets and its result.  The entries of a tensor refused by pp_stage or by its transform are all its stage offset; no entry
// lies behind the stage's capacity
__global__ void k_each_stage_offsets(u64* P, size_t* res, const u8* TR, const u8* base, const u64* S, const u64* W, const u64* T, size_t nT, u32 E, u32 segLog, u64 capacity,
                                     u64 stageCapacity)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nT) return;
    const u64 t0 = T[i] < stageCapacity ? T[i] : stageCapacity;
    if (i == nT) { P[nT * E] = t0; return; }
    const PpStage g = pp_stage(S, W, T, i, E, segLog, capacity, stageCapacity);
    const bool ok = g.ok && pe_ok(TR[i], base);
    for (u32 p = 0; p < E; ++p) P[i * E + p] = ok ? t0 + pl_start(g.m, p, E) : t0;
    res[i] = ok ? (size_t)g.m : FERR(GENERIC);
}
// workgroup w takes tile w - i of the staged sub-tensor i under transform TR[i]: m bytes at src + S[i] + at, planes at stage + T[i]
template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split_window_each(u8* stage, const u8* src, const u8* base, const u8* TR, const u64* S, const u64* W, const u64* T,
                                                                         size_t nT, u32 segLog, u64 capacity, u64 stageCapacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(T, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 t0 = T[i], t1 = T[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(t0 < t1) || lo >= t1 || lo + PLANES_TILE <= t0) return;
    const u32 tr = TR[i];
    if (!pe_ok(tr, base)) return;                                 // (a refused tensor: nothing of it is read or written)
    const PpStage g = pp_stage(S, W, T, i, E, segLog, capacity, stageCapacity);
    if (!g.ok) return;                                            // (accepted: t1 - t0 == m, t1 <= stageCapacity, S[i] + at + m <= S[i + 1] <= capacity)
    const u32 tid = threadIdx.x;
    const u64 at = S[i] + g.at;
    const u8* const sb = src + at;
    u8* const pb = stage + t0;
    if (tr == FSEHIP_EST_PLAIN) pe_split<E, FSEHIP_EST_PLAIN>(pb, sb, nullptr, t0, g.m, lo, tid);
    else if (tr == FSEHIP_EST_PRED) pe_split<E, FSEHIP_EST_PRED>(pb, sb, nullptr, t0, g.m, lo, tid);
    else if (tr == FSEHIP_EST_XOR) pe_split<E, FSEHIP_EST_XOR>(pb, sb, base + at, t0, g.m, lo, tid);
    else pe_split<E, FSEHIP_EST_SUB>(pb, sb, base + at, t0, g.m, lo, tid);
}

// ---- merge -------------------------------------------------------------------------------------------------------------------------------
// Win: empty -- the merge, launched as ever -- or the one more argument of the window form, const u64* W
template <int E, class... Win>
__global__ __launch_bounds__(PL_THREADS) void k_planes_merge_each(u8* dst, const u64* D, const u8* planes, const u64* PO, const size_t* PS, const u8* base, const u8* T,
                                                                  size_t nT, u64 dstCapacity, Win... win)
{
    constexpr bool WIN = sizeof...(Win) != 0;
    const u64 w = blockIdx.x;
    size_t i;
    if constexpr (WIN) {                                          // the key floor(D[j] / T) + 2 j: one more item per tensor
        if (nT == 0 || (D[0] >> PL_TILE_LOG) > w) return;
        i = pl_last_le(nT, w, [D](size_t j) { return (D[j] >> PL_TILE_LOG) + 2 * j; });
    } else if (!pl_find(D, nT, w, i)) return;                     // (uniform, like every return below)
    const u64 d0 = D[i], first = (d0 >> PL_TILE_LOG) + (WIN ? 2 : 1) * i;
    if (first > w) return;                                        // (offsets that decrease: the search found no tensor of this item)
    const u64 t = w - first;
    const u32 tr = T[i];
    if (!pe_ok(tr, base)) return;                                 // (a refused tensor: in place its old bytes stay)
    const size_t v = pm_verdict(D, PS, i, E, dstCapacity);
    if constexpr (WIN) {
        const u64* const W = (win, ...);
        u64 L;
        if (is_err(v) || !pe_win_ok(W, PO, i, E, tr, (u64)v, L)) return;
        const u64 nv = (u64)v + L * E;                            // the virtual tensor (an empty window: 0 bytes)
        if ((t << PL_TILE_LOG) >= nv) return;
        u8* const db = (u8*)((uintptr_t)(dst + d0) - L * E);      // where virtual element 0 would lie; nothing below dst + d0 is written
        const u64* const P = PO + i * E;
        if (tr == FSEHIP_EST_PLAIN) pe_merge<E, FSEHIP_EST_PLAIN, true>(db, nullptr, planes, P, nv, t, L);
        else if (tr == FSEHIP_EST_PRED) pe_merge<E, FSEHIP_EST_PRED, true>(db, nullptr, planes, P, nv, t, L);
        else if (tr == FSEHIP_EST_XOR) pe_merge<E, FSEHIP_EST_XOR, true>(db, base + d0, planes, P, nv, t, L);
        else pe_merge<E, FSEHIP_EST_SUB, true>(db, base + d0, planes, P, nv, t, L);
    } else {
        if (is_err(v) || (t << PL_TILE_LOG) >= (u64)v) return;    // (a good tensor: d0 + n <= D[i + 1] <= dstCapacity; t < 2^24)
        u8* const db = dst + d0;
        const u64* const P = PO + i * E;
        if (tr == FSEHIP_EST_PLAIN) pe_merge<E, FSEHIP_EST_PLAIN>(db, nullptr, planes, P, v, t);
        else if (tr == FSEHIP_EST_PRED) pe_merge<E, FSEHIP_EST_PRED>(db, nullptr, planes, P, v, t);
        else if (tr == FSEHIP_EST_XOR) pe_merge<E, FSEHIP_EST_XOR>(db, base + d0, planes, P, v, t);
        else pe_merge<E, FSEHIP_EST_SUB>(db, base + d0, planes, P, v, t);
    }
}
}   // namespace

// the offsets kernel runs even for no tensors (it writes the last entry); the data kernel moves every element size
hipError_t launch_planes_split_each(u8* planes, u64* planeOff, size_t* tensorRes, const u8* src, const u8* base, const u8* transforms, const u64* srcOff, size_t nTensors,
                                    unsigned E, u64 capacity, hipStream_t s)
{
    const hipError_t e0 = launch_planes_offsets(planeOff, tensorRes, srcOff, nTensors, E, capacity, s);
    if (e0 != hipSuccess || nTensors == 0) return e0;
    hipLaunchKernelGGL(k_each_refuse, dim3(grid_for(nTensors)), dim3(PL_THREADS), 0, s, tensorRes, transforms, base, nTensors);
    if (capacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(capacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        hipLaunchKernelGGL((k_planes_split_each<decltype(eb)::value>), g, b, 0, s, planes, src, base, transforms, srcOff, nTensors, capacity);
    });
    return hipGetLastError();
}

// the window form: the offsets kernel runs even for no tensors (it writes the last entry), then ceil(stageCapacity / T) + nTensors workgroups
hipError_t launch_planes_split_window_each(u8* stage, u64* planeOff, size_t* stageRes, const u8* src, const u8* base, const u8* transforms, const u64* srcOff,
                                           const u64* windows, const u64* stageOff, size_t nTensors, unsigned E, unsigned segLog, u64 capacity, u64 stageCapacity, hipStream_t s)
{
    hipLaunchKernelGGL(k_each_stage_offsets, dim3(grid_for(nTensors + 1)), dim3(PL_THREADS), 0, s, planeOff, stageRes, transforms, base, srcOff, windows, stageOff, nTensors,
                       (u32)E, (u32)segLog, capacity, stageCapacity);
    if (nTensors == 0 || stageCapacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(stageCapacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        hipLaunchKernelGGL((k_planes_split_window_each<decltype(eb)::value>), g, b, 0, s, stage, src, base, transforms, srcOff, windows, stageOff, nTensors, (u32)segLog,
                           capacity, stageCapacity);
    });
    return hipGetLastError();
}

hipError_t launch_planes_merge_each(u8* dst, const u64* dstOff, size_t* results, const u8* planes, const u64* planeOff, const size_t* planeSizes, const u8* base,
                                    const u8* transforms, size_t nTensors, unsigned E, u64 dstCapacity, hipStream_t s)
{
    if (nTensors == 0) return hipSuccess;
    const hipError_t e0 = launch_planes_verdicts(results, dstOff, planeSizes, nTensors, E, dstCapacity, s);
    if (e0 != hipSuccess) return e0;
    hipLaunchKernelGGL(k_each_refuse, dim3(grid_for(nTensors)), dim3(PL_THREADS), 0, s, results, transforms, base, nTensors);
    if (dstCapacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(dstCapacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        hipLaunchKernelGGL((k_planes_merge_each<decltype(eb)::value>), g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, transforms, nTensors, dstCapacity);
    });
    return hipGetLastError();
}

// the window form: the verdicts, the refusals with the window rules, then ceil(dstCapacity / T) + 2 nTensors workgroups (bad_grid with 2 nTensors)
hipError_t launch_planes_merge_window_each(u8* dst, const u64* dstOff, size_t* results, const u8* planes, const u64* planeOff, const size_t* planeSizes, const u8* base,
                                           const u8* transforms, const u64* windows, size_t nTensors, unsigned E, u64 dstCapacity, hipStream_t s)
{
    if (nTensors == 0) return hipSuccess;
    const hipError_t e0 = launch_planes_verdicts(results, dstOff, planeSizes, nTensors, E, dstCapacity, s);
    if (e0 != hipSuccess) return e0;
    hipLaunchKernelGGL(k_each_refuse_window, dim3(grid_for(nTensors)), dim3(PL_THREADS), 0, s, results, transforms, base, windows, planeOff, nTensors, (u32)E);
    if (dstCapacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(dstCapacity, 2 * nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        hipLaunchKernelGGL((k_planes_merge_each<decltype(eb)::value, const u64*>), g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, transforms, nTensors, dstCapacity,
                           windows);
    });
    return hipGetLastError();
}

// planes_each_stride.hip -- A STRIDE PER TENSOR (fsehip.h, "a stride per tensor"): the split and the merge of planes_each.hip with, beside the
// transform byte of tensor i, a stride byte that is read where that transform is FSEHIP_EST_PRED: the predecessor of an element lies
// ST[i] elements back, 1 .. FSEHIP_PRED_MAX_STRIDE, as in planes_stride.hip.  No transform of its own: the planes of a PRED tensor are byte
// for byte those of FSEHIP_planes_split_pred_stride_dbatch at its stride, those of every other tensor are the ones planes_each.hip writes,
// and the merge is the inverse.  Kernel launches only; the C calls are in capi_each.hip.
//
//   launch_planes_split_each_stride : k_planes_offsets (planes.hip) -> k_each_stride_refuse -> k_planes_split_each_stride
//   launch_planes_merge_each_stride : k_planes_verdicts (planes.hip) -> k_each_stride_refuse -> k_planes_merge_each_stride
// Without a stride array both are the launchers of planes_each.hip.
//
// THE KERNELS have the frames of k_planes_split_each and k_planes_merge_each: a workgroup has ONE tensor, so the transform and the stride
// are uniform over it, and the branch on them is taken once, in front of the loops.  Every arm is a body that exists already (planes_dev.h):
// pe_split / pe_merge for PLAIN, XOR, SUB and PRED at stride 1, ps_split / ps_merge -- the bodies of the kernels of planes_stride.hip -- for
// PRED at strides 2 .. 8, reached through a switch so that S is a constant in each of them and every register index is static.  No LDS, no
// scratch, no workspace; nothing crosses a wave.
//
// REFUSALS: those of planes_each.hip (pe_ok), and a PRED tensor whose stride byte is 0 or above FSEHIP_PRED_MAX_STRIDE: k_each_stride_refuse
// writes GENERIC over the tensor's result, and the data kernels return for it in front of every load and store.  The stride byte of a
// tensor under another transform is not read.
#include "planes_dev.h"

namespace {
// (pes_stride and pes_ok are in planes_dev.h: planes_each_stride_win.hip takes the same ones)
__global__ void k_each_stride_refuse(size_t* res, const u8* T, const u8* ST, const u8* base, size_t nT)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nT) return;
    const u32 tr = T[i];
    if (!pes_ok(tr, pes_stride(tr, ST, i), base)) res[i] = FERR(GENERIC);
}

template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split_each_stride(u8* planes, const u8* src, const u8* base, const u8* T, const u8* ST, const u64* S, size_t nT,
                                                                         u64 capacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(S, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 s0 = S[i], s1 = S[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(s0 < s1) || s1 > capacity || lo >= s1 || lo + PLANES_TILE <= s0) return;
    const u32 tr = T[i], st = pes_stride(tr, ST, i);
    if (!pes_ok(tr, st, base)) return;                            // (a refused tensor: nothing of it is read or written)
    const u64 n = s1 - s0;
    const u32 tid = threadIdx.x;
    const u8* const sb = src + s0;
    u8* const pb = planes + s0;
    if (tr == FSEHIP_EST_PLAIN) pe_split<E, FSEHIP_EST_PLAIN>(pb, sb, nullptr, s0, n, lo, tid);
    else if (tr == FSEHIP_EST_XOR) pe_split<E, FSEHIP_EST_XOR>(pb, sb, base + s0, s0, n, lo, tid);
    else if (tr == FSEHIP_EST_SUB) pe_split<E, FSEHIP_EST_SUB>(pb, sb, base + s0, s0, n, lo, tid);
    else if (st == 1) pe_split<E, FSEHIP_EST_PRED>(pb, sb, nullptr, s0, n, lo, tid);
    else ps_for_stride(st, [&](auto sc) { ps_split<E, decltype(sc)::value>(pb, sb, s0, n, lo, tid); });
}

template <int E>
__global__ __launch_bounds__(PL_THREADS) void k_planes_merge_each_stride(u8* dst, const u64* D, const u8* planes, const u64* PO, const size_t* PS, const u8* base,
                                                                         const u8* T, const u8* ST, size_t nT, u64 dstCapacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(D, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 d0 = D[i], first = (d0 >> PL_TILE_LOG) + i;
    if (first > w) return;                                        // (offsets that decrease: the search found no tensor of this item)
    const u64 t = w - first;
    const u32 tr = T[i], st = pes_stride(tr, ST, i);
    if (!pes_ok(tr, st, base)) return;                            // (a refused tensor: in place its old bytes stay)
    const size_t v = pm_verdict(D, PS, i, E, dstCapacity);
    if (is_err(v) || (t << PL_TILE_LOG) >= (u64)v) return;        // (a good tensor: d0 + n <= D[i + 1] <= dstCapacity; t < 2^24)
    u8* const db = dst + d0;
    const u64* const P = PO + i * E;
    if (tr == FSEHIP_EST_PLAIN) pe_merge<E, FSEHIP_EST_PLAIN>(db, nullptr, planes, P, v, t);
    else if (tr == FSEHIP_EST_XOR) pe_merge<E, FSEHIP_EST_XOR>(db, base + d0, planes, P, v, t);
    else if (tr == FSEHIP_EST_SUB) pe_merge<E, FSEHIP_EST_SUB>(db, base + d0, planes, P, v, t);
    else if (st == 1) pe_merge<E, FSEHIP_EST_PRED>(db, nullptr, planes, P, v, t);
    else ps_for_stride(st, [&](auto sc) { ps_merge<E, decltype(sc)::value>(db, planes, P, v, t); });
}
}   // namespace

// strides null: stride 1 everywhere, the launcher of planes_each.hip.  The offsets kernel runs even for no tensors (it writes the last entry)
hipError_t launch_planes_split_each_stride(u8* planes, u64* planeOff, size_t* tensorRes, const u8* src, const u8* base, const u8* transforms, const u8* strides,
                                           const u64* srcOff, size_t nTensors, unsigned E, u64 capacity, hipStream_t s)
{
    if (!strides) return launch_planes_split_each(planes, planeOff, tensorRes, src, base, transforms, srcOff, nTensors, E, capacity, s);
    const hipError_t e0 = launch_planes_offsets(planeOff, tensorRes, srcOff, nTensors, E, capacity, s);
    if (e0 != hipSuccess || nTensors == 0) return e0;
    hipLaunchKernelGGL(k_each_stride_refuse, dim3(grid_for(nTensors)), dim3(PL_THREADS), 0, s, tensorRes, transforms, strides, base, nTensors);
    if (capacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(capacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        hipLaunchKernelGGL((k_planes_split_each_stride<decltype(eb)::value>), g, b, 0, s, planes, src, base, transforms, strides, srcOff, nTensors, capacity);
    });
    return hipGetLastError();
}

hipError_t launch_planes_merge_each_stride(u8* dst, const u64* dstOff, size_t* results, const u8* planes, const u64* planeOff, const size_t* planeSizes, const u8* base,
                                           const u8* transforms, const u8* strides, size_t nTensors, unsigned E, u64 dstCapacity, hipStream_t s)
{
    if (!strides) return launch_planes_merge_each(dst, dstOff, results, planes, planeOff, planeSizes, base, transforms, nTensors, E, dstCapacity, s);
    if (nTensors == 0) return hipSuccess;
    const hipError_t e0 = launch_planes_verdicts(results, dstOff, planeSizes, nTensors, E, dstCapacity, s);
    if (e0 != hipSuccess) return e0;
    hipLaunchKernelGGL(k_each_stride_refuse, dim3(grid_for(nTensors)), dim3(PL_THREADS), 0, s, results, transforms, strides, base, nTensors);
    if (dstCapacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(dstCapacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        hipLaunchKernelGGL((k_planes_merge_each_stride<decltype(eb)::value>), g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, transforms, strides, nTensors,
                           dstCapacity);
    });
    return hipGetLastError();
}

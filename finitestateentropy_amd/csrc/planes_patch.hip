// planes_patch.hip -- PATCHING SEGMENTED TENSORS (fsehip.h, "patching segmented tensors"): the write side of planes_win.hip.  The tensors of a
// segmented batch changed inside an element window each; only the segment frames that hold the windows are coded anew, and a new packed
// object is built from the old frames and the new ones.  No frame byte and no writer changes: the writer codes a block whatever its
// position, a segment is a frame of its own, and the bytes of a tensor that its selected segments k0 .. k1 cover start at a multiple of E, so
// the planes of that sub-tensor ARE those segments -- the split's data path runs over sources displaced per tensor, the segments kernel and
// the packed writers run unchanged over the staged planes, and a ragged gather lays old and new frames behind one another.  Kernel launches only.
//
//   FSEHIP_planes_split_window_dbatch : k_planes_stage_offsets (per tensor: its staged plane offsets, its result) -> k_planes_split_window
//   FSEHIP_planes_splice_dbatch       : k_patch_planes (per plane, one wave: its verdict) -> k_patch_entries (per frame: extent, source,
//                                       result, codec) -> the exclusive scan of frame_dev.hip over the extents -> k_patch_results (per
//                                       tensor) -> k_planes_splice (per (tile, frame) intersection of the new object: the copy)
//   FSEHIP_tensor_patch_window_dbatch : the window split -> the segments kernel over the stage -> the packed (mixed) writer -> the splice
//   FSEHIP_planes_split_window_each_dbatch, FSEHIP_tensor_patch_window_each_dbatch ("patching tensors with a transform per tensor"): the same
//                                       two with the window split of planes_each.hip, which reads a transform per tensor; every later step as it is
//   FSEHIP_planes_split_window_each_stride_dbatch, FSEHIP_tensor_patch_window_each_stride_dbatch ("windows and patches of tensors with a stride
//                                       per tensor"): those two with d_strides, the window split of planes_each_stride_win.hip
#include "planes_dev.h"

namespace {
#define PP_NEW ((u64)1 << 63)          // k_patch_entries' source word: the frame lies in the new frames buffer, at the low bits

// ---- the window split ----------------------------------------------------------------------------------------------------------------------
// per tensor (and one thread more for the last entry): its E staged plane offsets and its result.  The entries of a refused tensor are all
// its stage offset; no entry lies behind the stage's capacity
__global__ void k_planes_stage_offsets(u64* P, size_t* res, const u64* S, const u64* W, const u64* T, size_t nT, u32 E, u32 segLog, u64 capacity, u64 stageCapacity)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nT) return;
    const u64 t0 = T[i] < stageCapacity ? T[i] : stageCapacity;
    if (i == nT) { P[nT * E] = t0; return; }
    const PpStage g = pp_stage(S, W, T, i, E, segLog, capacity, stageCapacity);
    for (u32 p = 0; p < E; ++p) P[i * E + p] = g.ok ? t0 + pl_start(g.m, p, E) : t0;
    res[i] = g.ok ? (size_t)g.m : FERR(GENERIC);
}
// k_planes_split's data path (planes.hip) over the STAGE axis: workgroup w takes tile w - i of the staged sub-tensor i, whose source lies at
// S[i] + at.  E == 1 without a base is the copy
template <int E, int OP>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split_window(u8* stage, const u8* src, const u8* base, const u64* S, const u64* W, const u64* T, size_t nT,
                                                                    u32 segLog, u64 capacity, u64 stageCapacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(T, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 t0 = T[i], t1 = T[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(t0 < t1) || lo >= t1 || lo + PLANES_TILE <= t0) return;
    const PpStage g = pp_stage(S, W, T, i, E, segLog, capacity, stageCapacity);
    if (!g.ok) return;                                            // (accepted: t1 - t0 == m, t1 <= stageCapacity, S[i] + at + m <= S[i + 1] <= capacity)
    const u64 n = g.m;
    const u32 tid = threadIdx.x;
    const u8* const sb = src + S[i] + g.at;
    const u8* const bb = OP != PL_NONE ? base + S[i] + g.at : nullptr;
    u8* const pb = stage + t0;
    const PlShare h = pl_share<E>(t0, n, lo, (u64)(uintptr_t)pb, 1);
    for (u64 c = tid; c < h.nch; c += PL_THREADS) {
        const u64 e = h.eb + 16 * c;
        u32 wv[4 * E], o[E][4];
#pragma unroll
        for (int k = 0; k < E; ++k) __builtin_memcpy(&wv[4 * k], sb + e * E + 16 * k, 16);
        if constexpr (OP != PL_NONE) {
#pragma unroll
            for (int k = 0; k < E; ++k) pl_base16<E, OP, false>(&wv[4 * k], bb + e * E + 16 * k);
        }
        pl_deinterleave<E>(wv, o);
#pragma unroll
        for (int p = 0; p < E; ++p) __builtin_memcpy(pb + pl_start(n, p, E) + e, o[p], 16);
    }
    if constexpr (OP == PL_SUB) {                                  // (an element per thread, as in k_planes_split)
        const u64 nHead = h.eb - h.e0, nTail = h.e1 - h.et;
        for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) pl_sub_elem_split<E>(pb, sb, bb, n, j < nHead ? h.e0 + j : h.et + (j - nHead));
    } else {
        const u64 nHead = (h.eb - h.e0) * E, nTail = (h.e1 - h.et) * E;
        for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) {
            const u64 k = j < nHead ? h.e0 * E + j : h.et * E + (j - nHead);
            if (k < n) {
                u8 v = sb[k];
                if constexpr (OP == PL_XOR) v ^= bb[k];
                pb[pl_start(n, (u32)(k % E), E) + k / E] = v;
            }
        }
    }
}

// ---- the splice ------------------------------------------------------------------------------------------------------------------------------
// the old and the new side of a splice, as the kernels take them
struct PpObj { const u8* frames; const u64* off; const size_t* res; const u8* codecs; u64 capacity; };
// the patch's tensor layout: S, windows, segFirst, selFirst, the split's results (or null)
struct PpMap { const u64* S; const u64* W; const u64* SF; const u64* WF; const size_t* stageRes; size_t nT; u32 E; size_t nSeg, nSel; u32 segLog; };

// One wave per plane: why its tensor is refused (0: it is not), in the order of fsehip.h.  PV[2 j] -- the window and the counts (pw_window;
// the split's error and a range of SF outside nSeg go with them: the same for all planes of a tensor), then the plane's OLD extents;
// PV[2 j + 1] -- the writer's results of its selected frames (ps_fold: the first error in segment order) and their extents in the new
// buffer.  Behind pw_window WF[j] + cnt <= nSel
__global__ __launch_bounds__(PL_THREADS) void k_patch_planes(size_t* PV, PpObj old, PpObj nw, PpMap m)
{
    const size_t j = (size_t)blockIdx.x * (PL_THREADS / WAVE) + (threadIdx.x / WAVE);
    if (j >= m.nT * m.E) return;                                  // (uniform over the wave)
    const u32 lane = threadIdx.x % WAVE;
    const size_t i = j / m.E;
    const PwWin w = pw_window(m.S, m.W, m.SF, m.WF, i, m.E, m.segLog, m.nSel);
    const size_t staged = m.stageRes ? m.stageRes[i] : 0;
    const u64 q0 = m.SF[j], q1 = m.SF[j + 1];
    bool inside = true;
    for (u32 p = 0; p < m.E; ++p) inside = inside && m.SF[i * m.E + p] <= m.SF[i * m.E + p + 1] && m.SF[i * m.E + p + 1] <= m.nSeg;
    if (!w.ok || is_err(staged) || !inside) {
        if (!lane) { PV[2 * j] = is_err(staged) ? staged : FERR(GENERIC); PV[2 * j + 1] = 0; }
        return;
    }
    u32 bad = 0;
    for (u64 q = q0 + lane; q < q1; q += WAVE) if (!pp_extent_ok(old.off, old.res, q, old.capacity)) bad = 1;
    const u64 r0 = m.WF[j];
    u32 badNew = 0;
    const PsFold f = ps_fold(nw.off + r0, nw.res + r0, w.cnt, lane, [&](u64 k, u64) {
        if (!pp_extent_ok(nw.off, nw.res, r0 + k, nw.capacity)) badNew = 1;
        return true;                                              // (slots may be aligned: f.bad, the back-to-back rule, is not used)
    });
    bad = group_reduce<64, ScanMax>(bad, lane);
    badNew = group_reduce<64, ScanMax>(badNew, lane);
    if (lane) return;
    PV[2 * j] = bad ? FERR(corruption_detected) : 0;
    PV[2 * j + 1] = f.firstErr != 0xFFFFFFFFu ? nw.res[r0 + f.firstErr] : badNew ? FERR(corruption_detected) : 0;
}
// tensor i's verdict from those of its planes: the first error in plane order of the rules in front of the writer, then of the writer's; 0
// without one
DEV size_t pp_tensor(const size_t* PV, size_t i, u32 E)
{
    for (u32 k = 0; k < 2; ++k)
        for (u32 p = 0; p < E; ++p) if (PV[2 * (i * E + p) + k]) return PV[2 * (i * E + p) + k];
    return 0;
}
// One thread per frame q < nSeg: its plane j by the search of k_planes_segments, its segment k inside the plane; selected iff its tensor is
// patched and k lies in k0 .. k0 + cnt - 1, then it is new frame r = WF[j] + k - k0 (< nSel behind pw_window).  ext[q] = what the frame takes
// of the new object (scanned in place afterwards: the new frame offsets), from[q] = where its bytes lie, res[q] and codecs[q] = its own.
// A kept frame whose old extent does not hold it (its tensor is refused) takes no room where the extent is not one, and has GENERIC
__global__ void k_patch_entries(u64* ext, u64* from, size_t* res, u8* codecs, const size_t* PV, PpObj old, PpObj nw, PpMap m)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m.nSeg) return;
    const size_t nP = m.nT * m.E;
    if (nP) {
        const size_t j = pl_last_le(nP, q, [&](size_t x) { return m.SF[x]; }), i = j / m.E;
        const PwWin w = pw_window(m.S, m.W, m.SF, m.WF, i, m.E, m.segLog, m.nSel);
        const u64 f = m.SF[j], k = q >= f ? q - f : 0;
        if (w.ok && k >= w.k0 && k - w.k0 < w.cnt && pp_tensor(PV, i, m.E) == 0) {
            const u64 r = m.WF[j] + (k - w.k0);
            ext[q] = nw.off[r + 1] - nw.off[r]; from[q] = PP_NEW | nw.off[r]; res[q] = nw.res[r];
            if (codecs) codecs[q] = nw.codecs[r];
            return;
        }
    }
    const u64 f0 = old.off[q], f1 = old.off[q + 1];
    const bool inside = f0 <= f1 && f1 <= old.capacity;
    const size_t r = old.res[q];
    ext[q] = inside ? f1 - f0 : 0; from[q] = f0;
    res[q] = inside && (is_err(r) || (u64)r <= f1 - f0) ? r : FERR(GENERIC);
    if (codecs) codecs[q] = old.codecs[q];
}
// per tensor, behind the scan: dstSize_tooSmall for all where the new object does not fit, else the split's error, GENERIC for a refused
// window or counts, the first error of its planes, or its size in bytes
__global__ void k_patch_results(size_t* tres, const u64* newOff, u64 outCapacity, const size_t* PV, PpMap m)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m.nT) return;
    const u64 s0 = m.S[i], s1 = m.S[i + 1];
    const size_t v = pp_tensor(PV, i, m.E);
    tres[i] = newOff[m.nSeg] > outCapacity ? FERR(dstSize_tooSmall) : v ? v : (size_t)(s1 > s0 ? s1 - s0 : 0);
}
// The ragged gather: the work mapping of the plane kernels (pl_find) with the NEW frame offsets as its axis -- every (tile, frame)
// intersection has one workgroup.  It copies the frame's real bytes inside its tile, res[q] <= ext[q] of them: bytewise up to the
// destination's 16-byte boundary, 16-byte pieces (unaligned loads, aligned stores), the rest bytewise -- the pattern of fd_copy
// (frame_dev.hip).  Nothing where the object does not fit
__global__ __launch_bounds__(PL_THREADS) void k_planes_splice(u8* out, const u64* newOff, const size_t* res, const u64* from, const u8* oldFrames, const u8* newFrames,
                                                              size_t nSeg, u64 outCapacity)
{
    const u64 w = blockIdx.x, total = newOff[nSeg];
    if (total > outCapacity || w > (total >> PL_TILE_LOG) + nSeg) return;
    size_t q;
    if (!pl_find(newOff, nSeg, w, q)) return;
    const size_t r = res[q];
    const u64 f0 = newOff[q], f1 = f0 + (is_err(r) ? 0 : (u64)r), lo = (w - q) << PL_TILE_LOG;
    const u64 b0 = lo > f0 ? lo : f0, b1 = lo + PLANES_TILE < f1 ? lo + PLANES_TILE : f1;
    if (b0 >= b1) return;
    const u64 at = from[q];
    const u8* const s = ((at & PP_NEW) ? newFrames : oldFrames) + (at & ~PP_NEW) + (b0 - f0);
    u8* const d = out + b0;
    const u64 len = b1 - b0;
    const u32 tid = threadIdx.x;
    u64 head = (0 - (u64)(uintptr_t)d) & 15u;
    if (head > len) head = len;
    if (tid < head) d[tid] = s[tid];
    const u64 body = (len - head) & ~(u64)15;
    for (u64 o = head + 16 * (u64)tid; o < head + body; o += 16 * PL_THREADS) {
        uint4 v;
        __builtin_memcpy(&v, s + o, 16);
        *(uint4*)(d + o) = v;
    }
    const u64 done = head + body;
    if (done + tid < len) d[done + tid] = s[done + tid];
}

// the splice's scratch: the plane verdicts, the frames' sources, the scan's partial sums
struct PpLayout { size_t pv, from, partials, total; };
inline PpLayout pp_layout(size_t nTensors, unsigned E, size_t nSeg)
{
    PpLayout L;
    L.pv = 0;
    L.from = align_up(L.pv + 2 * nTensors * E * sizeof(size_t), 256);
    L.partials = align_up(L.from + nSeg * sizeof(u64), 256);
    L.total = align_up(L.partials + exscan_partials(nSeg) * sizeof(u64), 256);
    return L;
}

hipError_t launch_split_window(u8* stage, u64* planeOff, size_t* stageRes, const u8* src, const u8* base, unsigned deltaOp, const u64* srcOff, const u64* windows, const u64* stageOff,
                               size_t nTensors, unsigned E, unsigned segLog, u64 capacity, u64 stageCapacity, hipStream_t s)
{
    hipLaunchKernelGGL(k_planes_stage_offsets, dim3(grid_for(nTensors + 1)), dim3(PL_THREADS), 0, s, planeOff, stageRes, srcOff, windows, stageOff, nTensors, (u32)E,
                       (u32)segLog, capacity, stageCapacity);
    if (nTensors == 0 || stageCapacity == 0) return hipGetLastError();
    const dim3 g(tile_grid(stageCapacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        constexpr int EB = decltype(eb)::value;
        const int op = pl_op(base, deltaOp);
        if (op == PL_SUB) hipLaunchKernelGGL((k_planes_split_window<EB, PL_SUB>), g, b, 0, s, stage, src, base, srcOff, windows, stageOff, nTensors, (u32)segLog, capacity, stageCapacity);
        else if (op == PL_XOR) hipLaunchKernelGGL((k_planes_split_window<EB, PL_XOR>), g, b, 0, s, stage, src, base, srcOff, windows, stageOff, nTensors, (u32)segLog, capacity, stageCapacity);
        else hipLaunchKernelGGL((k_planes_split_window<EB, PL_NONE>), g, b, 0, s, stage, src, base, srcOff, windows, stageOff, nTensors, (u32)segLog, capacity, stageCapacity);
    });
    return hipGetLastError();
}

hipError_t launch_splice(u8* out, u64 outCapacity, u64* outOff, size_t* outRes, u8* outCodecs, size_t* tensorRes, const PpObj& old, const PpObj& nw, const PpMap& m,
                         u8* scratch, hipStream_t s)
{
    const PpLayout L = pp_layout(m.nT, m.E, m.nSeg);
    size_t* const pv = (size_t*)(scratch + L.pv);
    u64* const from = (u64*)(scratch + L.from);
    const size_t perGroup = PL_THREADS / WAVE, nP = m.nT * m.E;
    if (nP) hipLaunchKernelGGL(k_patch_planes, dim3((unsigned)((nP + perGroup - 1) / perGroup)), dim3(PL_THREADS), 0, s, pv, old, nw, m);
    if (m.nSeg) hipLaunchKernelGGL(k_patch_entries, dim3(grid_for(m.nSeg)), dim3(PL_THREADS), 0, s, outOff, from, outRes, outCodecs, (const size_t*)pv, old, nw, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_exscan(outOff, m.nSeg, (u64*)(scratch + L.partials), s);
    if (e != hipSuccess) return e;
    if (m.nT) hipLaunchKernelGGL(k_patch_results, dim3(grid_for(m.nT)), dim3(PL_THREADS), 0, s, tensorRes, (const u64*)outOff, outCapacity, (const size_t*)pv, m);
    if (m.nSeg && outCapacity)
        hipLaunchKernelGGL(k_planes_splice, dim3(tile_grid(outCapacity, m.nSeg)), dim3(PL_THREADS), 0, s, out, (const u64*)outOff, (const size_t*)outRes, (const u64*)from,
                           old.frames, nw.frames, m.nSeg, outCapacity);
    return hipGetLastError();
}
}   // namespace

extern "C" int FSEHIP_planes_split_window_op_dbatch(void* d_stage, uint64_t* d_stagePlaneOffsets, size_t* d_stageResults, const void* d_src, const void* d_base,
                                                    unsigned deltaOp, const uint64_t* d_srcOffsets, const uint64_t* d_windows, const uint64_t* d_stageOffsets,
                                                    size_t nTensors, unsigned elemBytes, unsigned segLog, uint64_t capacity, uint64_t stageCapacity, void* stream)
{
    if (bad_op(deltaOp) || bad_elem(elemBytes) || bad_seg(segLog, 0) || !d_stagePlaneOffsets || !d_stageResults || !d_srcOffsets || !d_windows || !d_stageOffsets ||
        (stageCapacity && (!d_stage || !d_src)))
        return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(stageCapacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_split_window((u8*)d_stage, (u64*)d_stagePlaneOffsets, d_stageResults, (const u8*)d_src, (const u8*)d_base, deltaOp, (const u64*)d_srcOffsets,
                                    (const u64*)d_windows, (const u64*)d_stageOffsets, nTensors, elemBytes, segLog, capacity, stageCapacity, (hipStream_t)stream);
}
extern "C" int FSEHIP_planes_split_window_dbatch(void* d_stage, uint64_t* d_stagePlaneOffsets, size_t* d_stageResults, const void* d_src, const void* d_base,
                                                 const uint64_t* d_srcOffsets, const uint64_t* d_windows, const uint64_t* d_stageOffsets, size_t nTensors,
                                                 unsigned elemBytes, unsigned segLog, uint64_t capacity, uint64_t stageCapacity, void* stream)
{
    return FSEHIP_planes_split_window_op_dbatch(d_stage, d_stagePlaneOffsets, d_stageResults, d_src, d_base, FSEHIP_DELTA_XOR, d_srcOffsets, d_windows, d_stageOffsets,
                                                nTensors, elemBytes, segLog, capacity, stageCapacity, stream);
}

extern "C" size_t FSEHIP_planes_spliceScratchBound(size_t nTensors, unsigned elemBytes, size_t nSegments)
{
    if (bad_elem(elemBytes) || bad_counts(nTensors, elemBytes, nSegments)) return FSEHIP_ERROR(GENERIC);
    return pp_layout(nTensors, elemBytes, nSegments).total;
}

// what the splice and the composite check of the splice's own arguments
static bool bad_splice(const void* d_out, uint64_t outCapacity, const uint64_t* d_outOffsets, const size_t* d_outResults, const uint8_t* d_outCodecs,
                       const size_t* d_tensorResults, const void* d_frames, const uint64_t* d_frameOffsets, const size_t* d_frameResults, const uint8_t* d_codecs,
                       const uint8_t* d_newCodecs, const uint64_t* d_srcOffsets, const uint64_t* d_windows, size_t nTensors, unsigned E, const uint64_t* d_segFirst,
                       size_t nSegments, unsigned segLog, const uint64_t* d_selFirst, size_t nSelected, const void* d_scratch, size_t scratchBytes)
{
    if (bad_elem(E) || bad_seg(segLog, 0) || !d_outOffsets || !d_outResults || !d_tensorResults || !d_frameOffsets || !d_frameResults || !d_srcOffsets || !d_windows ||
        !d_segFirst || !d_selFirst || !d_scratch || ((uintptr_t)d_scratch & 255u) || (outCapacity && (!d_out || !d_frames)))
        return true;
    if ((d_outCodecs != nullptr) != (d_codecs != nullptr) || (nSelected && (d_newCodecs != nullptr) != (d_codecs != nullptr))) return true;
    if (bad_counts(nTensors, E, nSegments) || nSelected > nSegments || bad_grid(outCapacity, nSegments)) return true;
    return scratchBytes < pp_layout(nTensors, E, nSegments).total;
}

extern "C" int FSEHIP_planes_splice_dbatch(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs, size_t* d_tensorResults,
                                           const void* d_frames, uint64_t framesCapacity, const uint64_t* d_frameOffsets, const size_t* d_frameResults,
                                           const uint8_t* d_codecs, const void* d_newFrames, uint64_t newCapacity, const uint64_t* d_newOffsets,
                                           const size_t* d_newResults, const uint8_t* d_newCodecs, const size_t* d_stageResults, const uint64_t* d_srcOffsets,
                                           const uint64_t* d_windows, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog,
                                           const uint64_t* d_selFirst, size_t nSelected, void* d_scratch, size_t scratchBytes, void* stream)
{
    if (bad_splice(d_out, outCapacity, d_outOffsets, d_outResults, d_outCodecs, d_tensorResults, d_frames, d_frameOffsets, d_frameResults, d_codecs, d_newCodecs,
                   d_srcOffsets, d_windows, nTensors, elemBytes, d_segFirst, nSegments, segLog, d_selFirst, nSelected, d_scratch, scratchBytes))
        return (int)hipErrorInvalidValue;
    if (nSelected && (!d_newFrames || !d_newOffsets || !d_newResults)) return (int)hipErrorInvalidValue;
    const PpObj old = { (const u8*)d_frames, (const u64*)d_frameOffsets, d_frameResults, d_codecs, framesCapacity };
    const PpObj nw = { (const u8*)d_newFrames, (const u64*)d_newOffsets, d_newResults, d_newCodecs, newCapacity };
    const PpMap m = { (const u64*)d_srcOffsets, (const u64*)d_windows, (const u64*)d_segFirst, (const u64*)d_selFirst, d_stageResults, nTensors, elemBytes, nSegments,
                      nSelected, segLog };
    return (int)launch_splice((u8*)d_out, outCapacity, (u64*)d_outOffsets, d_outResults, d_outCodecs, d_tensorResults, old, nw, m, (u8*)d_scratch, (hipStream_t)stream);
}

// the argument checks of all four steps in front of the first launch
extern "C" int FSEHIP_tensor_patch_window_dbatch(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs,
                                                 size_t* d_tensorResults, const void* d_frames, uint64_t framesCapacity, const uint64_t* d_frameOffsets,
                                                 const size_t* d_frameResults, const uint8_t* d_codecs, const void* d_src, const void* d_base,
                                                 const uint64_t* d_srcOffsets, uint64_t capacity, const uint64_t* d_windows, size_t nTensors, unsigned elemBytes,
                                                 const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, const uint64_t* d_selFirst, size_t nSelected,
                                                 const uint64_t* d_stageOffsets, uint64_t stageCapacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec,
                                                 uint8_t* d_newCodecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_stage,
                                                 uint64_t* d_stagePlaneOffsets, uint64_t* d_stageSegOffsets, size_t* d_stageResults, void* d_newFrames,
                                                 uint64_t newCapacity, uint64_t* d_newOffsets, size_t* d_newResults, void* d_scratch, size_t scratchBytes,
                                                 void* d_workspace, size_t workspaceBytes, void* stream)
{
    return FSEHIP_tensor_patch_window_op_dbatch(d_out, outCapacity, d_outOffsets, d_outResults, d_outCodecs, d_tensorResults, d_frames, framesCapacity, d_frameOffsets,
                                                d_frameResults, d_codecs, d_src, d_base, FSEHIP_DELTA_XOR, d_srcOffsets, capacity, d_windows, nTensors, elemBytes, d_segFirst,
                                                nSegments, segLog, d_selFirst, nSelected, d_stageOffsets, stageCapacity, maxTotalBlocks, blockSizeId, codec, d_newCodecs,
                                                policy, tolerancePermille, slotAlignLog, d_stage, d_stagePlaneOffsets, d_stageSegOffsets, d_stageResults, d_newFrames,
                                                newCapacity, d_newOffsets, d_newResults, d_scratch, scratchBytes, d_workspace, workspaceBytes, stream);
}
// the one composite: the window split by one op (d_transforms null) or by a transform per tensor (d_strides: and a stride per PRED tensor;
// null: stride 1 everywhere), then the steps that all share
static int patch_window(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs, size_t* d_tensorResults, const void* d_frames,
                        uint64_t framesCapacity, const uint64_t* d_frameOffsets, const size_t* d_frameResults, const uint8_t* d_codecs, const void* d_src, const void* d_base,
                        unsigned deltaOp, const uint8_t* d_transforms, const uint64_t* d_srcOffsets, uint64_t capacity, const uint64_t* d_windows, size_t nTensors,
                        unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, const uint64_t* d_selFirst, size_t nSelected,
                        const uint64_t* d_stageOffsets, uint64_t stageCapacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_newCodecs, int policy,
                        unsigned tolerancePermille, unsigned slotAlignLog, void* d_stage, uint64_t* d_stagePlaneOffsets, uint64_t* d_stageSegOffsets, size_t* d_stageResults,
                        void* d_newFrames, uint64_t newCapacity, uint64_t* d_newOffsets, size_t* d_newResults, void* d_scratch, size_t scratchBytes, void* d_workspace,
                        size_t workspaceBytes, void* stream, const uint8_t* d_strides = nullptr)
{
    if (bad_op(deltaOp)) return (int)hipErrorInvalidValue;
    if (bad_splice(d_out, outCapacity, d_outOffsets, d_outResults, d_outCodecs, d_tensorResults, d_frames, d_frameOffsets, d_frameResults, d_codecs, d_newCodecs,
                   d_srcOffsets, d_windows, nTensors, elemBytes, d_segFirst, nSegments, segLog, d_selFirst, nSelected, d_scratch, scratchBytes))
        return (int)hipErrorInvalidValue;
    if (!d_stageOffsets || !d_stagePlaneOffsets || !d_stageSegOffsets || !d_stageResults || !d_newOffsets || !d_newResults ||
        (stageCapacity && (!d_stage || !d_src || !d_newFrames)))
        return (int)hipErrorInvalidValue;
    const PlWriter wr = { maxTotalBlocks, blockSizeId, codec, d_newCodecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes };
    if (bad_seg(segLog, blockSizeId) || bad_grid(stageCapacity, nTensors) || bad_writer(wr, nSelected)) return (int)hipErrorInvalidValue;
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = d_transforms ? launch_planes_split_window_each_stride((u8*)d_stage, (u64*)d_stagePlaneOffsets, d_stageResults, (const u8*)d_src, (const u8*)d_base,
                                                                         d_transforms, d_strides, (const u64*)d_srcOffsets, (const u64*)d_windows,
                                                                         (const u64*)d_stageOffsets, nTensors, elemBytes, segLog, capacity, stageCapacity, s)
                                : launch_split_window((u8*)d_stage, (u64*)d_stagePlaneOffsets, d_stageResults, (const u8*)d_src, (const u8*)d_base, deltaOp,
                                                      (const u64*)d_srcOffsets, (const u64*)d_windows, (const u64*)d_stageOffsets, nTensors, elemBytes, segLog, capacity,
                                                      stageCapacity, s);
    if (e != hipSuccess) return (int)e;
    if (nSelected) {                                             // (nothing selected: the splice alone, a copy of the object)
        // a staged sub-tensor has exactly cnt segments per plane: the segments kernel with the stage offsets as the tensors' and selFirst as
        // segFirst.  What it writes into d_tensorResults the splice overwrites
        e = launch_segments((u64*)d_stageSegOffsets, d_tensorResults, (const u64*)d_stagePlaneOffsets, (const u64*)d_stageOffsets, (const u64*)d_selFirst, nTensors,
                            elemBytes, nSelected, segLog, s);
        if (e != hipSuccess) return (int)e;
        const int r = d_newCodecs ? FSEHIP_frame_compress_packed_mixed_dbatch(d_newFrames, newCapacity, d_newOffsets, d_newResults, d_stage, d_stageSegOffsets, nSelected,
                                                                             maxTotalBlocks, blockSizeId, d_newCodecs, policy, tolerancePermille, slotAlignLog, d_workspace,
                                                                             workspaceBytes, stream)
                                  : FSEHIP_frame_compress_packed_dbatch(d_newFrames, newCapacity, d_newOffsets, d_newResults, d_stage, d_stageSegOffsets, nSelected,
                                                                       maxTotalBlocks, blockSizeId, codec, slotAlignLog, d_workspace, workspaceBytes, stream);
        if (r != 0) return r;
    }
    const PpObj old = { (const u8*)d_frames, (const u64*)d_frameOffsets, d_frameResults, d_codecs, framesCapacity };
    const PpObj nw = { (const u8*)d_newFrames, (const u64*)d_newOffsets, d_newResults, d_newCodecs, newCapacity };
    const PpMap m = { (const u64*)d_srcOffsets, (const u64*)d_windows, (const u64*)d_segFirst, (const u64*)d_selFirst, d_stageResults, nTensors, elemBytes, nSegments,
                      nSelected, segLog };
    return (int)launch_splice((u8*)d_out, outCapacity, (u64*)d_outOffsets, d_outResults, d_outCodecs, d_tensorResults, old, nw, m, (u8*)d_scratch, (hipStream_t)stream);
}
extern "C" int FSEHIP_tensor_patch_window_op_dbatch(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs,
                                                    size_t* d_tensorResults, const void* d_frames, uint64_t framesCapacity, const uint64_t* d_frameOffsets,
                                                    const size_t* d_frameResults, const uint8_t* d_codecs, const void* d_src, const void* d_base, unsigned deltaOp,
                                                    const uint64_t* d_srcOffsets, uint64_t capacity, const uint64_t* d_windows, size_t nTensors, unsigned elemBytes,
                                                    const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, const uint64_t* d_selFirst, size_t nSelected,
                                                    const uint64_t* d_stageOffsets, uint64_t stageCapacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec,
                                                    uint8_t* d_newCodecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_stage,
                                                    uint64_t* d_stagePlaneOffsets, uint64_t* d_stageSegOffsets, size_t* d_stageResults, void* d_newFrames,
                                                    uint64_t newCapacity, uint64_t* d_newOffsets, size_t* d_newResults, void* d_scratch, size_t scratchBytes,
                                                    void* d_workspace, size_t workspaceBytes, void* stream)
{
    return patch_window(d_out, outCapacity, d_outOffsets, d_outResults, d_outCodecs, d_tensorResults, d_frames, framesCapacity, d_frameOffsets, d_frameResults, d_codecs,
                        d_src, d_base, deltaOp, nullptr, d_srcOffsets, capacity, d_windows, nTensors, elemBytes, d_segFirst, nSegments, segLog, d_selFirst, nSelected,
                        d_stageOffsets, stageCapacity, maxTotalBlocks, blockSizeId, codec, d_newCodecs, policy, tolerancePermille, slotAlignLog, d_stage, d_stagePlaneOffsets,
                        d_stageSegOffsets, d_stageResults, d_newFrames, newCapacity, d_newOffsets, d_newResults, d_scratch, scratchBytes, d_workspace, workspaceBytes, stream);
}

// ---- patching tensors with a transform per tensor ----
extern "C" int FSEHIP_planes_split_window_each_dbatch(void* d_stage, uint64_t* d_stagePlaneOffsets, size_t* d_stageResults, const void* d_src, const void* d_base,
                                                      const uint8_t* d_transforms, const uint64_t* d_srcOffsets, const uint64_t* d_windows, const uint64_t* d_stageOffsets,
                                                      size_t nTensors, unsigned elemBytes, unsigned segLog, uint64_t capacity, uint64_t stageCapacity, void* stream)
{
    if (!d_transforms || bad_elem(elemBytes) || bad_seg(segLog, 0) || !d_stagePlaneOffsets || !d_stageResults || !d_srcOffsets || !d_windows || !d_stageOffsets ||
        (stageCapacity && (!d_stage || !d_src)))
        return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(stageCapacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_split_window_each((u8*)d_stage, (u64*)d_stagePlaneOffsets, d_stageResults, (const u8*)d_src, (const u8*)d_base, d_transforms,
                                                (const u64*)d_srcOffsets, (const u64*)d_windows, (const u64*)d_stageOffsets, nTensors, elemBytes, segLog, capacity,
                                                stageCapacity, (hipStream_t)stream);
}
extern "C" int FSEHIP_tensor_patch_window_each_dbatch(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs,
                                                      size_t* d_tensorResults, const void* d_frames, uint64_t framesCapacity, const uint64_t* d_frameOffsets,
                                                      const size_t* d_frameResults, const uint8_t* d_codecs, const void* d_src, const void* d_base,
                                                      const uint8_t* d_transforms, const uint64_t* d_srcOffsets, uint64_t capacity, const uint64_t* d_windows, size_t nTensors,
                                                      unsigned elemBytes,
                                                      const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, const uint64_t* d_selFirst, size_t nSelected,
                                                      const uint64_t* d_stageOffsets, uint64_t stageCapacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec,
                                                      uint8_t* d_newCodecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_stage,
                                                      uint64_t* d_stagePlaneOffsets, uint64_t* d_stageSegOffsets, size_t* d_stageResults, void* d_newFrames,
                                                      uint64_t newCapacity, uint64_t* d_newOffsets, size_t* d_newResults, void* d_scratch, size_t scratchBytes,
                                                      void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (!d_transforms) return (int)hipErrorInvalidValue;
    return patch_window(d_out, outCapacity, d_outOffsets, d_outResults, d_outCodecs, d_tensorResults, d_frames, framesCapacity, d_frameOffsets, d_frameResults, d_codecs,
                        d_src, d_base, FSEHIP_DELTA_XOR, d_transforms, d_srcOffsets, capacity, d_windows, nTensors, elemBytes, d_segFirst, nSegments, segLog, d_selFirst,
                        nSelected, d_stageOffsets, stageCapacity, maxTotalBlocks, blockSizeId, codec, d_newCodecs, policy, tolerancePermille, slotAlignLog, d_stage,
                        d_stagePlaneOffsets, d_stageSegOffsets, d_stageResults, d_newFrames, newCapacity, d_newOffsets, d_newResults, d_scratch, scratchBytes, d_workspace, workspaceBytes, stream);
}

// ---- patching tensors with a stride per tensor (fsehip.h, "windows and patches of tensors with a stride per tensor"): the two calls above
// with d_strides behind d_transforms, null: stride 1 everywhere ----
extern "C" int FSEHIP_planes_split_window_each_stride_dbatch(void* d_stage, uint64_t* d_stagePlaneOffsets, size_t* d_stageResults, const void* d_src, const void* d_base,
                                                             const uint8_t* d_transforms, const uint8_t* d_strides, const uint64_t* d_srcOffsets, const uint64_t* d_windows,
                                                             const uint64_t* d_stageOffsets, size_t nTensors, unsigned elemBytes, unsigned segLog, uint64_t capacity,
                                                             uint64_t stageCapacity, void* stream)
{
    if (!d_transforms || bad_elem(elemBytes) || bad_seg(segLog, 0) || !d_stagePlaneOffsets || !d_stageResults || !d_srcOffsets || !d_windows || !d_stageOffsets ||
        (stageCapacity && (!d_stage || !d_src)))
        return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(stageCapacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_split_window_each_stride((u8*)d_stage, (u64*)d_stagePlaneOffsets, d_stageResults, (const u8*)d_src, (const u8*)d_base, d_transforms, d_strides,
                                                       (const u64*)d_srcOffsets, (const u64*)d_windows, (const u64*)d_stageOffsets, nTensors, elemBytes, segLog, capacity,
                                                       stageCapacity, (hipStream_t)stream);
}
extern "C" int FSEHIP_tensor_patch_window_each_stride_dbatch(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs,
                                                             size_t* d_tensorResults, const void* d_frames, uint64_t framesCapacity, const uint64_t* d_frameOffsets,
                                                             const size_t* d_frameResults, const uint8_t* d_codecs, const void* d_src, const void* d_base,
                                                             const uint8_t* d_transforms, const uint8_t* d_strides, const uint64_t* d_srcOffsets, uint64_t capacity,
                                                             const uint64_t* d_windows, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments,
                                                             unsigned segLog, const uint64_t* d_selFirst, size_t nSelected, const uint64_t* d_stageOffsets,
                                                             uint64_t stageCapacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_newCodecs, int policy,
                                                             unsigned tolerancePermille, unsigned slotAlignLog, void* d_stage, uint64_t* d_stagePlaneOffsets,
                                                             uint64_t* d_stageSegOffsets, size_t* d_stageResults, void* d_newFrames, uint64_t newCapacity,
                                                             uint64_t* d_newOffsets, size_t* d_newResults, void* d_scratch, size_t scratchBytes, void* d_workspace,
                                                             size_t workspaceBytes, void* stream)
{
    if (!d_transforms) return (int)hipErrorInvalidValue;
    return patch_window(d_out, outCapacity, d_outOffsets, d_outResults, d_outCodecs, d_tensorResults, d_frames, framesCapacity, d_frameOffsets, d_frameResults, d_codecs,
                        d_src, d_base, FSEHIP_DELTA_XOR, d_transforms, d_srcOffsets, capacity, d_windows, nTensors, elemBytes, d_segFirst, nSegments, segLog, d_selFirst,
                        nSelected, d_stageOffsets, stageCapacity, maxTotalBlocks, blockSizeId, codec, d_newCodecs, policy, tolerancePermille, slotAlignLog, d_stage,
                        d_stagePlaneOffsets, d_stageSegOffsets, d_stageResults, d_newFrames, newCapacity, d_newOffsets, d_newResults, d_scratch, scratchBytes, d_workspace,
                        workspaceBytes, stream, d_strides);
}

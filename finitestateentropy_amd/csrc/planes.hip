// planes.hip -- tensors of 2-, 4- and 8-byte elements as BYTE PLANES (fsehip.h, "byte planes of tensors"): plane p of a tensor holds byte p of
// every element, the planes of a tensor lie back to back where the tensor lies, and every plane becomes one .fse frame (frame_dev.hip).  An
// order-0 coder then sees the exponent bytes and the mantissa bytes of a bf16 tensor in histograms of their own.  Kernel launches only.
//
//   FSEHIP_planes_split_dbatch     : k_planes_offsets (per tensor: its plane offsets in closed form, its result) -> k_planes_split
//   FSEHIP_planes_merge_dbatch     : k_planes_verdicts (per tensor: its result) -> k_planes_merge
//   FSEHIP_tensor_compress_dbatch  : the split -> FSEHIP_frame_compress_packed_dbatch over the planes (the plane offsets are its source offsets)
//   FSEHIP_tensor_decompress_dbatch: FSEHIP_frame_decompress_packed_dbatch into the planes buffer -> the merge over the offsets and results it leaves
// (The device helpers all of them are made of are in planes_dev.h, shared with planes_seg.hip and planes_win.hip.)
// (planes_pred.hip: the same calls on the neighbour differences, with data kernels of its own in front of and behind the steps here.)
//
// TENSOR DELTAS (fsehip.h, "tensor deltas"): the same calls on `tensor XOR base`, the XOR fused into the two data kernels.  The receiver of a
// tensor often holds an earlier version of it (weights after a step, the checkpoint before this one); XOR against that version zeroes every
// byte that did not change, the sign / exponent plane becomes almost all zeros, and the order-0 coders do the rest.  No bitstream, header or
// frame byte differs: the frames are ordinary .fse frames of the planes of `tensor XOR base`.
//
//   FSEHIP_planes_split_xor_dbatch       : the split with a base, for every element size (E == 1 too: the XOR has to be written somewhere)
//   FSEHIP_planes_merge_xor_dbatch       : the merge with a base, which may be the destination itself
//   FSEHIP_tensor_compress_delta_dbatch  : the XOR split -> the packed writer over the planes
//   FSEHIP_tensor_compress_mixed_dbatch  : the plain or the XOR split -> the packed writer with a codec per plane
//   FSEHIP_tensor_decompress_delta_dbatch: the packed reader into the planes buffer -> the XOR merge
//   FSEHIP_*_op_dbatch                   : each of these five with `deltaOp` behind d_base (FSEHIP_DELTA_XOR: the call itself; FSEHIP_DELTA_SUB:
//                                          ARITHMETIC DELTAS below); the names without _op forward to them
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
// The XOR forms (OP = PL_XOR) are the same kernels with one more read stream: per chunk E more loads of 16 bytes from the base, which lies where the
// source (split) or the destination (merge) lies, each XORed into its words as it arrives.  XOR acts bit by bit, so it commutes with the byte
// shuffle: the split XORs in front of it, the merge behind it.  3 n bytes of traffic where the plain kernels have 2 n; the plain kernels
// never read `base`.
//
// ARITHMETIC DELTAS (fsehip.h, "arithmetic tensor deltas"; the *_op_dbatch calls with FSEHIP_DELTA_SUB): the third instantiation of the same
// templates (OP = PL_SUB), the planes of zigzag(tensor - base) on the elements' bit patterns.  A one-ulp change of a float XORs to a carry
// chain (1, 3, 7, ..) but subtracts to 1 or 2, so the high planes stay zero unless the value really moved.  Subtraction does NOT commute with
// the byte shuffle -- borrows run across the bytes of an element -- so it sits on the ELEMENT side of it: the split subtracts in front of
// pl_deinterleave, the merge adds behind pl_interleave, on dwords that hold whole elements (a lane's chunk is 16 whole elements from the
// tensor's start): packed 16-bit forms for E == 2, plain 32-bit for 4, a borrow across the dword pair for 8, SWAR over four bytes for 1
// (planes_dev.h: pl_sub4).  Each base load is combined into its words as it arrives, as the XOR is.  Head and tail go an ELEMENT per thread
// (E bytewise loads, E bytewise stores, any alignment), the partial last element of a tensor byte by byte in the E == 1 form.
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
// OP (planes_dev.h: PL_NONE, PL_XOR, PL_SUB): the planes of src, of src XOR base or of zigzag(src - base), the base laid out as src is
template <int E, int OP>
__global__ __launch_bounds__(PL_THREADS) void k_planes_split(u8* planes, const u8* src, const u8* base, const u64* S, size_t nT, u64 capacity)
{
    const u64 w = blockIdx.x;
    size_t i;
    if (!pl_find(S, nT, w, i)) return;                            // (uniform, like every return below)
    const u64 s0 = S[i], s1 = S[i + 1], lo = (w - i) << PL_TILE_LOG;
    if (!(s0 < s1) || s1 > capacity || lo >= s1 || lo + PLANES_TILE <= s0) return;
    const u64 n = s1 - s0;
    const u32 tid = threadIdx.x;
    const u8* const sb = src + s0;
    const u8* const bb = OP != PL_NONE ? base + s0 : nullptr;
    u8* const pb = planes + s0;
    const PlShare h = pl_share<E>(s0, n, lo, (u64)(uintptr_t)pb, 1);
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
    // head and tail, a byte per thread: byte k of the tensor is byte k / E of plane k % E.  SUB: an element per thread
    if constexpr (OP == PL_SUB) {
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

// ---- merge -------------------------------------------------------------------------------------------------------------------------------
__global__ void k_planes_verdicts(size_t* res, const u64* D, const size_t* PS, size_t nT, u32 E, u64 dstCapacity)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nT) res[i] = pm_verdict(D, PS, i, E, dstCapacity);
}
// OP: every rebuilt tensor as it is, XOR base, or base + unzigzag(it), the base laid out as dst is.
// IN PLACE: `base` may be exactly `dst` (the resident tensors are updated where they lie).  Chunks, head and tail partition the elements of a
// workgroup's share, the shares partition the tensor (planes_dev.h: pl_share, the work mapping), and a tensor's bytes belong to no other
// tensor: every byte of dst is read (as base) and written by exactly ONE thread, and no thread reads a base byte that another one writes.
// Within a thread the base loads of a chunk -- all E of them -- precede its stores in program order, and neither pointer is __restrict__,
// so the compiler keeps that order: a store never lands in front of the load of the same bytes.  SUB is the same argument: a chunk's E base
// loads precede its stores, and in head and tail a thread owns a whole element -- its E base bytes are loaded before its E bytes are stored.  Any other overlap of base and dst is the
// caller's error and is not checked.  A refused or failed tensor returns in front of every load and store: in place its base stays as it is.
template <int E, int OP>
__global__ __launch_bounds__(PL_THREADS) void k_planes_merge(u8* dst, const u64* D, const u8* planes, const u64* PO, const size_t* PS, const u8* base, size_t nT,
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
    const u8* const bb = OP != PL_NONE ? base + d0 : nullptr;
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
        if constexpr (OP != PL_NONE) {
#pragma unroll
            for (int k = 0; k < E; ++k) pl_base16<E, OP, true>(&wv[4 * k], bb + e * E + 16 * k);          // (in place: these loads, then the stores below)
        }
#pragma unroll
        for (int k = 0; k < E; ++k) __builtin_memcpy(db + e * E + 16 * k, &wv[4 * k], 16);
    }
    if constexpr (OP == PL_SUB) {                                  // (an element per thread; in place: its loads, then its stores)
        const u64 nHead = h.eb - h.e0, nTail = h.e1 - h.et;
        for (u64 j = tid; j < nHead + nTail; j += PL_THREADS)
            pl_sub_elem_merge<E>(db, bb, n, j < nHead ? h.e0 + j : h.et + (j - nHead), [&](u32 p) { return planes + PO[i * E + p]; });
    } else {
        const u64 nHead = (h.eb - h.e0) * E, nTail = (h.e1 - h.et) * E;
        for (u64 j = tid; j < nHead + nTail; j += PL_THREADS) {
            const u64 k = j < nHead ? h.e0 * E + j : h.et * E + (j - nHead);
            if (k < n) {
                u8 v8 = planes[PO[i * E + k % E] + k / E];
                if constexpr (OP == PL_XOR) v8 ^= bb[k];             // (in place: this load, then the store)
                db[k] = v8;
            }
        }
    }
}
}   // namespace

// base null: the plain kernels, and no data kernel at all for E == 1 (the planes of such a tensor are the tensor).  The offsets kernel runs
// even for no tensors: it writes the last entry
// the split's first step by itself: the plane layout and the tensor results that a set of tensor offsets implies (planes_sparse.hip reads
// the layout of a destination from it)
hipError_t launch_planes_offsets(u64* planeOff, size_t* tensorRes, const u64* srcOff, size_t nTensors, unsigned E, u64 capacity, hipStream_t s)
{
    hipLaunchKernelGGL(k_planes_offsets, dim3(grid_for(nTensors + 1)), dim3(PL_THREADS), 0, s, planeOff, tensorRes, srcOff, nTensors, (u32)E, capacity);
    return hipGetLastError();
}
hipError_t launch_planes_split(u8* planes, u64* planeOff, size_t* tensorRes, const u8* src, const u8* base, unsigned deltaOp, const u64* srcOff, size_t nTensors,
                               unsigned E, u64 capacity, hipStream_t s)
{
    const hipError_t e0 = launch_planes_offsets(planeOff, tensorRes, srcOff, nTensors, E, capacity, s);
    if (e0 != hipSuccess || (E == 1 && !base) || nTensors == 0 || capacity == 0) return e0;
    const dim3 g(tile_grid(capacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        constexpr int EB = decltype(eb)::value;
        const int op = pl_op(base, deltaOp);
        if (op == PL_SUB) hipLaunchKernelGGL((k_planes_split<EB, PL_SUB>), g, b, 0, s, planes, src, base, srcOff, nTensors, capacity);
        else if (op == PL_XOR) hipLaunchKernelGGL((k_planes_split<EB, PL_XOR>), g, b, 0, s, planes, src, base, srcOff, nTensors, capacity);
        else hipLaunchKernelGGL((k_planes_split<EB, PL_NONE>), g, b, 0, s, planes, src, base, srcOff, nTensors, capacity);
    });
    return hipGetLastError();
}

// the merge's first step by itself (planes_pred.hip puts a data kernel of its own behind it); nTensors > 0
hipError_t launch_planes_verdicts(size_t* results, const u64* dstOff, const size_t* planeSizes, size_t nTensors, unsigned E, u64 dstCapacity, hipStream_t s)
{
    hipLaunchKernelGGL(k_planes_verdicts, dim3(grid_for(nTensors)), dim3(PL_THREADS), 0, s, results, dstOff, planeSizes, nTensors, (u32)E, dstCapacity);
    return hipGetLastError();
}
// base null: the plain merge.  The tail of every decompress composite, over whatever plane offsets and sizes the steps in front of it left
hipError_t launch_planes_merge(u8* dst, const u64* dstOff, size_t* results, const u8* planes, const u64* planeOff, const size_t* planeSizes, const u8* base,
                               unsigned deltaOp, size_t nTensors, unsigned E, u64 dstCapacity, hipStream_t s)
{
    if (nTensors == 0) return hipSuccess;
    const hipError_t e0 = launch_planes_verdicts(results, dstOff, planeSizes, nTensors, E, dstCapacity, s);
    if (dstCapacity == 0 || e0 != hipSuccess) return e0;
    const dim3 g(tile_grid(dstCapacity, nTensors)), b(PL_THREADS);
    pl_for_elem(E, [&](auto eb) {
        constexpr int EB = decltype(eb)::value;
        const int op = pl_op(base, deltaOp);
        if (op == PL_SUB) hipLaunchKernelGGL((k_planes_merge<EB, PL_SUB>), g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, nTensors, dstCapacity);
        else if (op == PL_XOR) hipLaunchKernelGGL((k_planes_merge<EB, PL_XOR>), g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, nTensors, dstCapacity);
        else hipLaunchKernelGGL((k_planes_merge<EB, PL_NONE>), g, b, 0, s, dst, dstOff, planes, planeOff, planeSizes, base, nTensors, dstCapacity);
    });
    return hipGetLastError();
}

// The one compress path of the four composites, each of which has checked its own pointers: the remaining argument checks of all steps in
// front of the first launch (fsehip.h: what the guarantee covers), the split (d_base given: the split of the delta by deltaOp), the segments kernel where
// d_segFirst is given, then the packed writer -- a codec per frame where w.d_codecs is given -- over the planes or their segments, read
// from d_src itself where the split moved nothing.  `sparse` given (planes_sparse.hip): pack stands between the units and the writer, which
// then reads the contents; pack's workspace is the head of the caller's, the writer's the rest.  `pred` != 0 (planes_stride.hip): the predicted
// split of that stride in place of the plain one, which moves every element size
int planes_compress(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults, const void* d_src, const void* d_base,
                    unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors, unsigned E, uint64_t capacity, const uint64_t* d_segFirst, size_t nSegments,
                    unsigned segLog, void* d_planes, uint64_t* d_planeOffsets, uint64_t* d_segOffsets, const PlWriter& writer, void* stream, const PlSparse* sparse, unsigned pred)
{
    if (bad_op(deltaOp) || (pred && d_base)) return (int)hipErrorInvalidValue;
    if (d_segFirst ? bad_seg(segLog, writer.blockSizeId) || bad_counts(nTensors, E, nSegments) : bad_tensors(nTensors, E)) return (int)hipErrorInvalidValue;
    const size_t nFrames = d_segFirst ? nSegments : nTensors * E;
    PlWriter w = writer;
    u8* const packWs = (u8*)writer.d_workspace;
    if (sparse) {
        if (sparse->permille > 1000 || bad_sparse(capacity, nFrames, w.d_workspace, w.workspaceBytes)) return (int)hipErrorInvalidValue;
        const size_t head = sparse_workspace(capacity, nFrames);
        w.d_workspace = packWs + head;
        w.workspaceBytes -= head;
    }
    if (bad_grid(capacity, nTensors) || bad_writer(w, nFrames)) return (int)hipErrorInvalidValue;
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = pred ? launch_planes_split_pred_stride((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u64*)d_srcOffsets, nTensors, E, capacity,
                                                             pred, s)
                        : launch_planes_split((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u8*)d_base, deltaOp, (const u64*)d_srcOffsets,
                                              nTensors, E, capacity, s);
    if (e == hipSuccess && d_segFirst)
        e = launch_segments((u64*)d_segOffsets, d_tensorResults, (const u64*)d_planeOffsets, (const u64*)d_srcOffsets, (const u64*)d_segFirst, nTensors, E, nSegments, segLog, s);
    if (e != hipSuccess) return (int)e;
    const void* from = !d_base && !pred && E == 1 ? d_src : d_planes;
    const uint64_t* fromOff = d_segFirst ? d_segOffsets : d_planeOffsets;
    if (sparse) {
        e = launch_sparse_pack((u8*)sparse->d_contents, (u64*)sparse->d_contentOffsets, (const u8*)from, (const u64*)fromOff, nFrames, capacity, sparse->permille, packWs, s);
        if (e != hipSuccess) return (int)e;
        from = sparse->d_contents; fromOff = sparse->d_contentOffsets;
    }
    if (w.d_codecs)
        return FSEHIP_frame_compress_packed_mixed_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, from, fromOff, nFrames, w.maxTotalBlocks, w.blockSizeId,
                                                         w.d_codecs, w.policy, w.tolerancePermille, w.slotAlignLog, w.d_workspace, w.workspaceBytes, stream);
    return FSEHIP_frame_compress_packed_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, from, fromOff, nFrames, w.maxTotalBlocks, w.blockSizeId, w.codec,
                                               w.slotAlignLog, w.d_workspace, w.workspaceBytes, stream);
}

// FSEHIP_tensor_decompress_dbatch and _delta(_op)_dbatch behind their pointer checks: they differ in the base and its op alone
static int planes_decompress(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp, size_t* d_results, const void* d_frames,
                             const uint64_t* d_frameOffsets, size_t nTensors, unsigned E, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                             uint64_t* d_planeOffsets, size_t* d_planeResults, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_op(deltaOp) || bad_tensors(nTensors, E) || bad_grid(dstCapacity, nTensors) || bad_reader(d_workspace, workspaceBytes, nTensors * E, maxTotalBlocks))
        return (int)hipErrorInvalidValue;
    const int e = FSEHIP_frame_decompress_packed_dbatch(d_planes, (size_t)planesCapacity, d_planeOffsets, d_planeResults, d_frames, d_frameOffsets, nTensors * E, maxTotalBlocks,
                                                        0, d_workspace, workspaceBytes, stream);
    if (e != 0) return e;
    return (int)launch_planes_merge((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeResults, (const u8*)d_base,
                                    deltaOp, nTensors, E, dstCapacity, (hipStream_t)stream);
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
    if (bad_tensors(nTensors, elemBytes) || bad_grid(capacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_split((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, nullptr, 0, (const u64*)d_srcOffsets, nTensors, elemBytes, capacity,
                                    (hipStream_t)stream);
}
extern "C" int FSEHIP_planes_split_op_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const void* d_base,
                                             unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity, void* stream)
{
    if (bad_op(deltaOp) || bad_elem(elemBytes) || !d_planes || !d_planeOffsets || !d_tensorResults || !d_src || !d_base || !d_srcOffsets) return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(capacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_split((u8*)d_planes, (u64*)d_planeOffsets, d_tensorResults, (const u8*)d_src, (const u8*)d_base, deltaOp, (const u64*)d_srcOffsets, nTensors,
                                    elemBytes, capacity, (hipStream_t)stream);
}
extern "C" int FSEHIP_planes_split_xor_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const void* d_base,
                                              const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity, void* stream)
{
    return FSEHIP_planes_split_op_dbatch(d_planes, d_planeOffsets, d_tensorResults, d_src, d_base, FSEHIP_DELTA_XOR, d_srcOffsets, nTensors, elemBytes, capacity, stream);
}

extern "C" int FSEHIP_planes_merge_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                          const size_t* d_planeSizes, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_planes || !d_planeOffsets || !d_planeSizes) return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(dstCapacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_merge((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, nullptr, 0, nTensors,
                                    elemBytes, dstCapacity, (hipStream_t)stream);
}
extern "C" int FSEHIP_planes_merge_op_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                             const size_t* d_planeSizes, const void* d_base, unsigned deltaOp, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity,
                                             void* stream)
{
    if (bad_op(deltaOp) || bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_planes || !d_planeOffsets || !d_planeSizes || !d_base) return (int)hipErrorInvalidValue;
    if (bad_tensors(nTensors, elemBytes) || bad_grid(dstCapacity, nTensors)) return (int)hipErrorInvalidValue;
    return (int)launch_planes_merge((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, (const u8*)d_base,
                                    deltaOp, nTensors, elemBytes, dstCapacity, (hipStream_t)stream);
}
extern "C" int FSEHIP_planes_merge_xor_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                              const size_t* d_planeSizes, const void* d_base, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream)
{
    return FSEHIP_planes_merge_op_dbatch(d_dst, d_dstOffsets, d_results, d_planes, d_planeOffsets, d_planeSizes, d_base, FSEHIP_DELTA_XOR, nTensors, elemBytes, dstCapacity,
                                         stream);
}

extern "C" int FSEHIP_tensor_compress_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                             const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                             size_t maxTotalBlocks, unsigned blockSizeId, int codec, unsigned slotAlignLog,
                                             void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_srcOffsets || !d_planeOffsets || (elemBytes > 1 && !d_planes))
        return (int)hipErrorInvalidValue;
    return planes_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, nullptr, 0, d_srcOffsets, nTensors, elemBytes, capacity, nullptr, 0, 0,
                           d_planes, d_planeOffsets, nullptr, PlWriter{ maxTotalBlocks, blockSizeId, codec, nullptr, 0, 0, slotAlignLog, d_workspace, workspaceBytes }, stream);
}
extern "C" int FSEHIP_tensor_compress_delta_op_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                      const void* d_src, const void* d_base, unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors,
                                                      unsigned elemBytes, uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, unsigned slotAlignLog,
                                                      void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_base || !d_srcOffsets || !d_planeOffsets || !d_planes)
        return (int)hipErrorInvalidValue;
    return planes_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, deltaOp, d_srcOffsets, nTensors, elemBytes, capacity, nullptr,
                           0, 0, d_planes, d_planeOffsets, nullptr,
                           PlWriter{ maxTotalBlocks, blockSizeId, codec, nullptr, 0, 0, slotAlignLog, d_workspace, workspaceBytes }, stream);
}
extern "C" int FSEHIP_tensor_compress_delta_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                   const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                   uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, unsigned slotAlignLog,
                                                   void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes, void* stream)
{
    return FSEHIP_tensor_compress_delta_op_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, FSEHIP_DELTA_XOR, d_srcOffsets,
                                                  nTensors, elemBytes, capacity, maxTotalBlocks, blockSizeId, codec, slotAlignLog, d_planes, d_planeOffsets, d_workspace,
                                                  workspaceBytes, stream);
}
// the plain (d_base == nullptr) or the delta split, then the packed writer with a codec per plane
extern "C" int FSEHIP_tensor_compress_mixed_op_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                      const void* d_src, const void* d_base, unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors,
                                                      unsigned elemBytes, uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, uint8_t* d_codecs, int policy,
                                                      unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets,
                                                      void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_srcOffsets || !d_planeOffsets || !d_codecs ||
        ((elemBytes > 1 || d_base) && !d_planes))
        return (int)hipErrorInvalidValue;
    return planes_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, deltaOp, d_srcOffsets, nTensors, elemBytes, capacity, nullptr,
                           0, 0, d_planes, d_planeOffsets, nullptr,
                           PlWriter{ maxTotalBlocks, blockSizeId, 0, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes }, stream);
}
extern "C" int FSEHIP_tensor_compress_mixed_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                   const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                   uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, uint8_t* d_codecs, int policy,
                                                   unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets,
                                                   void* d_workspace, size_t workspaceBytes, void* stream)
{
    return FSEHIP_tensor_compress_mixed_op_dbatch(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, FSEHIP_DELTA_XOR, d_srcOffsets,
                                                  nTensors, elemBytes, capacity, maxTotalBlocks, blockSizeId, d_codecs, policy, tolerancePermille, slotAlignLog, d_planes,
                                                  d_planeOffsets, d_workspace, workspaceBytes, stream);
}

extern "C" int FSEHIP_tensor_decompress_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results,
                                               const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks,
                                               void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                               void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_frames || !d_frameOffsets || !d_planes || !d_planeOffsets || !d_planeResults)
        return (int)hipErrorInvalidValue;
    return planes_decompress(d_dst, d_dstOffsets, dstCapacity, nullptr, 0, d_results, d_frames, d_frameOffsets, nTensors, elemBytes, maxTotalBlocks, d_planes, planesCapacity,
                             d_planeOffsets, d_planeResults, d_workspace, workspaceBytes, stream);
}
extern "C" int FSEHIP_tensor_decompress_delta_op_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp,
                                                        size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                        size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                                        void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_base || !d_results || !d_frames || !d_frameOffsets || !d_planes || !d_planeOffsets || !d_planeResults)
        return (int)hipErrorInvalidValue;
    return planes_decompress(d_dst, d_dstOffsets, dstCapacity, d_base, deltaOp, d_results, d_frames, d_frameOffsets, nTensors, elemBytes, maxTotalBlocks, d_planes,
                             planesCapacity, d_planeOffsets, d_planeResults, d_workspace, workspaceBytes, stream);
}
extern "C" int FSEHIP_tensor_decompress_delta_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, size_t* d_results,
                                                     const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks,
                                                     void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                                     void* d_workspace, size_t workspaceBytes, void* stream)
{
    return FSEHIP_tensor_decompress_delta_op_dbatch(d_dst, d_dstOffsets, dstCapacity, d_base, FSEHIP_DELTA_XOR, d_results, d_frames, d_frameOffsets, nTensors, elemBytes,
                                                    maxTotalBlocks, d_planes, planesCapacity, d_planeOffsets, d_planeResults, d_workspace, workspaceBytes, stream);
}

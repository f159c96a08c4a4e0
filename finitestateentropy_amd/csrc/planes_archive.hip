// planes_archive.hip -- TENSOR ARCHIVES (fsehip.h, "tensor archives"): `head | frames` in one device buffer, sealed by the sender behind the
// frames that a compress composite wrote at d_archive + headBytes, opened by the receiver into the arrays the reading calls take.
//
//   FSEHIP_archive_headBytes / _inspect / _workspaceBound : host arithmetic
//   FSEHIP_archive_seal_dbatch : k_ar_seal (a thread per 8-byte word of the head: header, sizes, offsets, digests, codecs, meta, padding --
//                                written and checked) -> FSEHIP_tensor_digest_dbatch over [0, headBytes - 8) as one tensor -> k_ar_stamp
//                                (one wave: the verdict, the digest into the last word, the magic zeroed on refusal, the result)
//   FSEHIP_archive_open_dbatch : k_ar_index (a thread per word: checked; the sizes into d_srcOffsets and the per-plane segment counts into
//                                d_segFirst as scan inputs) -> launch_exscan of each -> the digest -> k_ar_verdict (one wave) -> k_ar_emit (a
//                                thread per entry: frame offsets -- zeros on refusal --, digests, codecs)
//
// The head as 8-byte words W[0 .. head / 8): [0, 8) the header, then the regions of ArLay, W[wEnd] the digest.  A wave ORs what its lanes
// found (group_reduce of dev_common.h; 0 fine, 1 only the capacity is short, 2 refused: the maximum is the OR) into a flag of its own, so
// no launch has to clear anything and nothing is atomic; the one-wave kernel behind folds the flags.  The workspace: 256 bytes of control
// words (CT_*), the wave flags, the scan's partials, the digest's workspace.
#include "planes_dev.h"
#include <cstddef>
#include <cstring>

namespace {
#define AR_FLAGS_KNOWN (FSEHIP_ARCHIVE_CODECS | FSEHIP_ARCHIVE_DIGESTS | FSEHIP_ARCHIVE_SPARSE | FSEHIP_ARCHIVE_DELTA)
enum { CT_S0 = 0, CT_S1 = 1, CT_DIGEST = 2, CT_DRES = 3, CT_BAD = 4 };     // control words: the head as one tensor [S0, S1), its digest and result, open's verdict
static_assert(sizeof(FSEHIP_ArchiveInfo) == 72 && offsetof(FSEHIP_ArchiveInfo, nTensors) == 16 && offsetof(FSEHIP_ArchiveInfo, framesBytes) == 56 &&
              offsetof(FSEHIP_ArchiveInfo, headBytes) == 64, "the first 64 bytes of the struct are the header");

// the regions of the head in words: sizes [8, wOffs), frame offsets [wOffs, wDig), digests [wDig, wCod), codecs [wCod, wMeta), meta
// [wMeta, wPad), zeros [wPad, wEnd), the digest at wEnd = head / 8 - 1
struct ArLay { u64 wOffs, wDig, wCod, wMeta, wPad, wEnd; };
HDEV ArLay ar_lay(u64 nT, u64 nF, u32 flags, u64 metaBytes)
{
    ArLay l;
    l.wOffs = 8 + nT;
    l.wDig = l.wOffs + nF + 1;
    l.wCod = l.wDig + ((flags & FSEHIP_ARCHIVE_DIGESTS) ? nT : 0);
    l.wMeta = l.wCod + ((flags & FSEHIP_ARCHIVE_CODECS) ? (nF + 7) / 8 : 0);
    l.wPad = l.wMeta + (metaBytes + 7) / 8;
    l.wEnd = (((l.wPad + 1) * 8 + 255) & ~(u64)255) / 8 - 1;
    return l;
}
struct ArArgs { u64 hdr[8]; u64 nT, nF, totalBytes, framesBytes, metaBytes; ArLay lay; u32 E, segLog, flags; };
DEV u64 ar_hdr(const ArArgs& a, u64 w)
{
    u64 v = 0;
#pragma unroll
    for (u32 k = 0; k < 8; ++k) v = w == k ? a.hdr[k] : v;       // (selects: the argument stays in scalar registers)
    return v;
}
DEV void ar_flag(u32* waveFlags, u64 w, u32 bad, u32 lane)
{
    bad = group_reduce<64, ScanMax>(bad, lane);
    if (lane == 0) waveFlags[w / WAVE] = bad;
}
DEV u32 ar_fold(const u32* waveFlags, u32 nWaves, u32 lane)
{
    u32 bad = 0;
    for (u32 k = lane; k < nWaves; k += WAVE) bad = bad > waveFlags[k] ? bad : waveFlags[k];
    return group_reduce<64, ScanMax>(bad, lane);
}

// SEAL, a thread per word w of the head (the grid covers [0, wEnd), whole waves): its value and what is wrong with it.  `room` =
// archiveCapacity - headBytes.  Word 7 of the header is F[nF], the device's own framesBytes.
__global__ __launch_bounds__(PL_THREADS) void k_ar_seal(u64* W, u32* waveFlags, u64* ctrl, ArArgs a, const u64* S, const u64* F, const size_t* FR, const size_t* TR,
                                                        const u8* codecs, const u64* D, const u8* meta, u64 room)
{
    const u64 w = (u64)blockIdx.x * PL_THREADS + threadIdx.x;
    const u32 lane = threadIdx.x % WAVE;
    const ArLay& l = a.lay;
    u32 bad = 0;
    u64 v = 0;
    if (w < 8) v = w == 7 ? F[a.nF] : ar_hdr(a, w);
    else if (w < l.wOffs) {
        const u64 i = w - 8, s0 = S[i], s1 = S[i + 1];
        if (s1 < s0 || is_err(TR[i])) bad = 2;
        if (i == 0 && S[a.nT] - s0 != a.totalBytes) bad = 2;       // (non-decreasing offsets: their span is the sum of the sizes)
        v = s1 >= s0 ? s1 - s0 : 0;
    } else if (w < l.wDig) {
        const u64 q = w - l.wOffs;
        v = F[q];
        if (q == 0 && v != 0) bad = 2;
        if (q < a.nF) { const u64 f1 = F[q + 1]; const size_t r = FR[q]; if (f1 < v || is_err(r) || (u64)r > f1 - v) bad = 2; }
        else if (v > room) bad = 1;
    } else if (w < l.wCod) v = D[w - l.wDig];
    else if (w < l.wMeta) {
        const u64 k = (w - l.wCod) * 8;
#pragma unroll
        for (u32 j = 0; j < 8; ++j)
            if (k + j < a.nF) { const u32 c = codecs[k + j]; if (c > 1) bad = 2; v |= (u64)c << (8 * j); }
    } else if (w < l.wPad) {
        const u64 k = (w - l.wMeta) * 8;
#pragma unroll
        for (u32 j = 0; j < 8; ++j)
            if (k + j < a.metaBytes) v |= (u64)meta[k + j] << (8 * j);
    }
    if (w < l.wEnd) W[w] = v;
    if (w == 0) { ctrl[CT_S0] = 0; ctrl[CT_S1] = 8 * l.wEnd; }
    ar_flag(waveFlags, w, bad, lane);
}

// one wave: the verdict over the wave flags and the digest's result, the digest into the last word, the result; the magic 0 on refusal
__global__ __launch_bounds__(WAVE) void k_ar_stamp(u64* W, size_t* result, const u32* waveFlags, u32 nWaves, const u64* ctrl, u64 wEnd)
{
    u32 bad = ar_fold(waveFlags, nWaves, threadIdx.x);
    if (threadIdx.x != 0) return;
    if (is_err((size_t)ctrl[CT_DRES])) bad = 2;
    W[wEnd] = ctrl[CT_DIGEST];
    if (bad) reinterpret_cast<u32*>(W)[0] = 0;
    *result = bad == 0 ? (size_t)(8 * (wEnd + 1) + W[7]) : bad == 1 ? FERR(dstSize_tooSmall) : FERR(GENERIC);
}

// OPEN, a thread per word w < wEnd: what is wrong with it.  The size of tensor i goes to SO[i] and (segmented) the segment counts of its E
// planes to SF[i E ..]: the inputs of the two scans.  A size above totalBytes is refused and counts as 0, so neither scan can wrap (the
// limits of inspect keep nTensors * totalBytes below 2^63).
__global__ __launch_bounds__(PL_THREADS) void k_ar_index(const u64* W, u32* waveFlags, u64* ctrl, ArArgs a, u64* SO, u64* SF)
{
    const u64 w = (u64)blockIdx.x * PL_THREADS + threadIdx.x;
    const u32 lane = threadIdx.x % WAVE;
    const ArLay& l = a.lay;
    u32 bad = 0;
    const u64 v = w < l.wEnd ? W[w] : 0;
    if (w < 8) { if (v != ar_hdr(a, w)) bad = 2; }
    else if (w < l.wOffs) {
        const u64 i = w - 8;
        u64 n = v;
        if (n > a.totalBytes) { bad = 2; n = 0; }
        SO[i] = n;
        if (a.segLog)
            for (u32 p = 0; p < a.E; ++p) SF[i * a.E + p] = ps_count(pl_size(n, p, a.E), a.segLog);
    } else if (w < l.wDig) {
        const u64 q = w - l.wOffs;
        if (q == 0 && v != 0) bad = 2;
        if (q < a.nF ? W[w + 1] < v : v != a.framesBytes) bad = 2;
    } else if (w < l.wCod) { }
    else if (w < l.wMeta) {
        const u64 k = (w - l.wCod) * 8;
#pragma unroll
        for (u32 j = 0; j < 8; ++j) { const u32 c = (u32)(v >> (8 * j)) & 0xFFu; if (k + j < a.nF ? c > 1 : c != 0) bad = 2; }
    } else if (w < l.wPad) {
        const u64 k = (w - l.wMeta) * 8;
#pragma unroll
        for (u32 j = 0; j < 8; ++j)
            if (k + j >= a.metaBytes && ((v >> (8 * j)) & 0xFFu)) bad = 2;
    } else if (v != 0) bad = 2;
    if (w == 0) { ctrl[CT_S0] = 0; ctrl[CT_S1] = 8 * l.wEnd; }
    ar_flag(waveFlags, w, bad, lane);
}

// one wave: the verdict -- the wave flags, the digest against the head's last word, the two scans' totals
__global__ __launch_bounds__(WAVE) void k_ar_verdict(const u64* W, size_t* verdict, u64* ctrl, const u32* waveFlags, u32 nWaves, ArArgs a, const u64* SO, const u64* SF)
{
    u32 bad = ar_fold(waveFlags, nWaves, threadIdx.x);
    if (threadIdx.x != 0) return;
    if (is_err((size_t)ctrl[CT_DRES]) || ctrl[CT_DIGEST] != W[a.lay.wEnd]) bad = 2;
    if (SO[a.nT] != a.totalBytes) bad = 2;
    if (a.segLog && SF[a.nT * a.E] != a.nF) bad = 2;
    ctrl[CT_BAD] = bad;
    *verdict = bad ? FERR(corruption_detected) : (size_t)(8 * (a.lay.wEnd + 1) + a.framesBytes);
}

// a thread per entry: the frame offsets (0 on refusal), the digests, the codecs clamped to 1
__global__ void k_ar_emit(const u64* W, const u64* ctrl, ArArgs a, u64* FO, u8* codecs, u64* D)
{
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = ctrl[CT_BAD] == 0;
    if (t <= a.nF) FO[t] = ok ? W[a.lay.wOffs + t] : 0;
    if ((a.flags & FSEHIP_ARCHIVE_DIGESTS) && t < a.nT) D[t] = W[a.lay.wDig + t];
    if ((a.flags & FSEHIP_ARCHIVE_CODECS) && t < a.nF) { const u8 c = reinterpret_cast<const u8*>(W + a.lay.wCod)[t]; codecs[t] = c > 1 ? 1 : c; }
}

inline size_t r256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool bad_ar_counts(u64 nT, u64 nF, u32 flags, u64 metaBytes) { return (flags & ~AR_FLAGS_KNOWN) || nT >= ((u64)1 << 24) || nF >= ((u64)1 << 31) || metaBytes >= ((u64)1 << 31); }
// the header's own rules (fsehip.h): 0, or the error inspect answers with
size_t ar_header_error(const FSEHIP_ArchiveInfo& h)
{
    if (h.magic != FSEHIP_ARCHIVE_MAGIC || h.version != FSEHIP_ARCHIVE_VERSION) return FSEHIP_ERROR(GENERIC);
    const size_t corrupt = FSEHIP_ERROR(corruption_detected);
    if ((h.flags & ~AR_FLAGS_KNOWN) || ((h.flags & FSEHIP_ARCHIVE_DIGESTS) && !(h.flags & FSEHIP_ARCHIVE_DELTA))) return corrupt;
    if (bad_elem(h.elemBytes) || h.blockSizeId > 6 || (h.segLog && bad_seg(h.segLog, h.blockSizeId))) return corrupt;
    if (h.deltaOp > FSEHIP_DELTA_SUB || (h.deltaOp && !(h.flags & FSEHIP_ARCHIVE_DELTA))) return corrupt;
    if (h.sparsePermille > 1000 || (h.sparsePermille && !(h.flags & FSEHIP_ARCHIVE_SPARSE)) || h.reserved) return corrupt;
    if (bad_ar_counts(h.nTensors, h.nFrames, h.flags, h.metaBytes) || bad_grid(h.totalBytes, (size_t)h.nTensors) || h.maxTotalBlocks >= ((u64)1 << 31)) return corrupt;
    if (h.segLog ? h.nFrames < h.nTensors * h.elemBytes : h.nFrames != h.nTensors * h.elemBytes) return corrupt;
    if (h.nTensors == 0 && h.totalBytes != 0) return corrupt;
    return 0;
}
inline u64 ar_head(const FSEHIP_ArchiveInfo& h) { return 8 * (ar_lay(h.nTensors, h.nFrames, h.flags, h.metaBytes).wEnd + 1); }

// the workspace: control words | wave flags | scan partials | the digest's
struct ArWs { size_t flags, partials, digest, digestBytes, total; u32 nWaves; unsigned grid; };
ArWs ar_ws(u64 nT, u64 nF, u64 head)
{
    ArWs x;
    const u64 words = head / 8 - 1;
    x.grid = (unsigned)((words + PL_THREADS - 1) / PL_THREADS);
    x.nWaves = x.grid * (PL_THREADS / WAVE);
    x.flags = 256;
    x.partials = x.flags + r256((size_t)x.nWaves * 4);
    x.digest = x.partials + r256(exscan_partials((size_t)nT * 8) * 8);
    x.digestBytes = FSEHIP_tensor_digest_workspaceBound(head - 8, 1);
    x.total = x.digest + x.digestBytes;
    return x;
}
ArArgs ar_args(const FSEHIP_ArchiveInfo& h)
{
    ArArgs a;
    FSEHIP_ArchiveInfo t = h;
    t.magic = FSEHIP_ARCHIVE_MAGIC; t.version = FSEHIP_ARCHIVE_VERSION;
    memcpy(a.hdr, &t, 64);
    a.nT = h.nTensors; a.nF = h.nFrames; a.totalBytes = h.totalBytes; a.framesBytes = h.framesBytes; a.metaBytes = h.metaBytes;
    a.lay = ar_lay(h.nTensors, h.nFrames, h.flags, h.metaBytes);
    a.E = h.elemBytes; a.segLog = h.segLog; a.flags = h.flags;
    return a;
}
// what both device calls ask of their info and workspace
bool bad_ar_call(const FSEHIP_ArchiveInfo* info, bool sealing, const void* d_workspace, size_t workspaceBytes)
{
    if (!info) return true;
    FSEHIP_ArchiveInfo h = *info;
    if (sealing) { h.magic = FSEHIP_ARCHIVE_MAGIC; h.version = FSEHIP_ARCHIVE_VERSION; }
    if (ar_header_error(h) || h.headBytes != ar_head(h)) return true;
    const ArWs x = ar_ws(h.nTensors, h.nFrames, h.headBytes);
    return FSEHIP_isError(x.digestBytes) || !d_workspace || ((uintptr_t)d_workspace & 255u) || workspaceBytes < x.total;
}
}   // namespace

extern "C" size_t FSEHIP_archive_headBytes(uint64_t nTensors, uint64_t nFrames, unsigned flags, uint64_t metaBytes)
{
    if (bad_ar_counts(nTensors, nFrames, flags, metaBytes)) return FSEHIP_ERROR(GENERIC);
    return (size_t)(8 * (ar_lay(nTensors, nFrames, flags, metaBytes).wEnd + 1));
}

extern "C" size_t FSEHIP_archive_inspect(FSEHIP_ArchiveInfo* out, const void* h_header64, uint64_t archiveBytes)
{
    if (!out || !h_header64) return FSEHIP_ERROR(GENERIC);
    memset(out, 0, sizeof(*out));
    if (archiveBytes < 64) return FSEHIP_ERROR(srcSize_wrong);
    memcpy(out, h_header64, 64);
    const size_t e = ar_header_error(*out);
    if (e) return e;
    const u64 head = ar_head(*out);
    if (head > archiveBytes || out->framesBytes > archiveBytes - head) return FSEHIP_ERROR(srcSize_wrong);
    out->headBytes = head;
    return (size_t)head;
}

extern "C" size_t FSEHIP_archive_workspaceBound(uint64_t nTensors, uint64_t nFrames, uint64_t headBytes)
{
    if (bad_ar_counts(nTensors, nFrames, 0, 0) || headBytes < 256 || (headBytes & 255u) || headBytes >= ((u64)1 << 40)) return FSEHIP_ERROR(GENERIC);
    const ArWs x = ar_ws(nTensors, nFrames, headBytes);
    return FSEHIP_isError(x.digestBytes) ? FSEHIP_ERROR(GENERIC) : x.total;
}

extern "C" int FSEHIP_archive_seal_dbatch(void* d_archive, uint64_t archiveCapacity, size_t* d_result, const FSEHIP_ArchiveInfo* info, const uint64_t* d_srcOffsets,
                                          const uint64_t* d_frameOffsets, const size_t* d_frameResults, const size_t* d_tensorResults, const uint8_t* d_codecs,
                                          const uint64_t* d_digests, const void* d_meta, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (!d_archive || ((uintptr_t)d_archive & 7u) || !d_result || !d_srcOffsets || !d_frameOffsets || !d_frameResults || !d_tensorResults ||
        bad_ar_call(info, true, d_workspace, workspaceBytes))
        return (int)hipErrorInvalidValue;
    if (archiveCapacity < info->headBytes || ((info->flags & FSEHIP_ARCHIVE_CODECS) && !d_codecs) || ((info->flags & FSEHIP_ARCHIVE_DIGESTS) && !d_digests) ||
        (info->metaBytes && !d_meta))
        return (int)hipErrorInvalidValue;
    const ArArgs a = ar_args(*info);
    const ArWs x = ar_ws(a.nT, a.nF, info->headBytes);
    u8* const ws = (u8*)d_workspace;
    u64* const ctrl = (u64*)ws;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ar_seal, dim3(x.grid), dim3(PL_THREADS), 0, s, (u64*)d_archive, (u32*)(ws + x.flags), ctrl, a, (const u64*)d_srcOffsets, (const u64*)d_frameOffsets,
                       d_frameResults, d_tensorResults, d_codecs, (const u64*)d_digests, (const u8*)d_meta, (u64)(archiveCapacity - info->headBytes));
    const int e = FSEHIP_tensor_digest_dbatch(ctrl + CT_DIGEST, (size_t*)(ctrl + CT_DRES), d_archive, ctrl + CT_S0, 1, info->headBytes - 8, ws + x.digest, x.digestBytes, stream);
    if (e) return e;
    hipLaunchKernelGGL(k_ar_stamp, dim3(1), dim3(WAVE), 0, s, (u64*)d_archive, d_result, (const u32*)(ws + x.flags), x.nWaves, (const u64*)ctrl, a.lay.wEnd);
    return (int)hipGetLastError();
}

extern "C" int FSEHIP_archive_open_dbatch(uint64_t* d_srcOffsets, uint64_t* d_frameOffsets, uint8_t* d_codecs, uint64_t* d_digests, uint64_t* d_segFirst, size_t* d_verdict,
                                          const void* d_archive, uint64_t archiveBytes, const FSEHIP_ArchiveInfo* info, void* d_workspace, size_t workspaceBytes,
                                          void* stream)
{
    if (!d_archive || ((uintptr_t)d_archive & 7u) || !d_verdict || !d_srcOffsets || !d_frameOffsets || bad_ar_call(info, false, d_workspace, workspaceBytes))
        return (int)hipErrorInvalidValue;
    if (info->headBytes > archiveBytes || info->framesBytes > archiveBytes - info->headBytes || ((info->flags & FSEHIP_ARCHIVE_CODECS) && !d_codecs) ||
        ((info->flags & FSEHIP_ARCHIVE_DIGESTS) && !d_digests) || (info->segLog && !d_segFirst))
        return (int)hipErrorInvalidValue;
    const ArArgs a = ar_args(*info);
    const ArWs x = ar_ws(a.nT, a.nF, info->headBytes);
    u8* const ws = (u8*)d_workspace;
    u64* const ctrl = (u64*)ws;
    u64* const partials = (u64*)(ws + x.partials);
    const u64* const W = (const u64*)d_archive;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ar_index, dim3(x.grid), dim3(PL_THREADS), 0, s, W, (u32*)(ws + x.flags), ctrl, a, (u64*)d_srcOffsets, (u64*)d_segFirst);
    hipError_t he = launch_exscan((u64*)d_srcOffsets, (size_t)a.nT, partials, s);
    if (he != hipSuccess) return (int)he;
    if (a.segLog) {
        he = launch_exscan((u64*)d_segFirst, (size_t)a.nT * a.E, partials, s);
        if (he != hipSuccess) return (int)he;
    }
    const int e = FSEHIP_tensor_digest_dbatch(ctrl + CT_DIGEST, (size_t*)(ctrl + CT_DRES), d_archive, ctrl + CT_S0, 1, info->headBytes - 8, ws + x.digest, x.digestBytes, stream);
    if (e) return e;
    hipLaunchKernelGGL(k_ar_verdict, dim3(1), dim3(WAVE), 0, s, W, d_verdict, ctrl, (const u32*)(ws + x.flags), x.nWaves, a, (const u64*)d_srcOffsets, (const u64*)d_segFirst);
    const u64 n = (a.nF + 1 > a.nT ? a.nF + 1 : a.nT);
    hipLaunchKernelGGL(k_ar_emit, dim3(grid_for((size_t)n)), dim3(PL_THREADS), 0, s, W, (const u64*)ctrl, a, (u64*)d_frameOffsets, d_codecs, (u64*)d_digests);
    return (int)hipGetLastError();
}

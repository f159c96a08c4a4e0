// capi_batch.hip -- the batched calls of the C ABI (include/fsehip.h) on DEVICE pointers: every *_batch call and its *_batch_workspaceSize,
// for FSE, Huff0 and 16-bit symbols, and the *_view pipelines the device frame calls (frame_dev.hip) drive.  Nothing here allocates,
// copies or synchronises: a call is a sequence of launches on the caller's stream.
#include "internal.h"

// =====================================================================================================
//  a1: HIST_count
// =====================================================================================================
extern "C" int FSEHIP_HIST_count_batch(unsigned* d_counts, unsigned* d_maxSymbolValues, size_t* d_results,
                                       const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                       size_t nBlocks, void* stream)
{
    HistArgs a;
    a.counts = d_counts; a.maxSVs = d_maxSymbolValues; a.uniformMaxSV = 255; a.useUniformIn = 0;
    a.results = d_results; a.src = mkview(d_src, srcStride, d_sizes, uniformSize); a.nBlocks = nBlocks;
    return (int)launch_hist(a, (hipStream_t)stream);
}

// =====================================================================================================
//  a2 / a3: FSE hot loops over a batch
// =====================================================================================================
extern "C" int FSEHIP_FSE_compress_usingCTable_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                                     const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                                     const FSEHIP_FSE_CTable* d_ctables, size_t ctableStrideU32, unsigned maxTableLog,
                                                     size_t nBlocks, void* stream)
{
    if (maxTableLog == 0 || maxTableLog > FSEHIP_FSE_MAX_TABLELOG) maxTableLog = FSEHIP_FSE_MAX_TABLELOG;
    FseEncArgs a;
    a.dst = (u8*)d_dst; a.dstStride = dstStride; a.dstCapacity = dstCapacity; a.results = d_results;
    a.src = mkview(d_src, srcStride, d_sizes, uniformSize);
    a.ctables = d_ctables; a.ctStrideU32 = ctableStrideU32; a.meta = nullptr;
    a.maxTableLog = maxTableLog; a.G = 0; a.slotU32 = 0; a.nBlocks = nBlocks; a.list = nullptr; a.count = nullptr;
    return (int)launch_fse_encode_auto(a, (hipStream_t)stream);
}

extern "C" int FSEHIP_FSE_decompress_usingDTable_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                                       const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                       const FSEHIP_FSE_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                       size_t nBlocks, void* stream)
{
    if (maxTableLog == 0 || maxTableLog > FSEHIP_FSE_MAX_TABLELOG) maxTableLog = FSEHIP_FSE_MAX_TABLELOG;
    FseDecArgs a;
    a.dst = (u8*)d_dst; a.dstStride = dstStride; a.dstCapacity = dstCapacity; a.results = d_results;
    a.csrc = mkview(d_cSrc, cStride, d_cSizes, uniformCSize);
    a.dtables = d_dtables; a.dtStrideU32 = dtableStrideU32; a.atab = nullptr; a.symtab = nullptr; a.meta = nullptr;
    a.maxTableLog = maxTableLog; a.G = 0; a.slotU32 = 0; a.nBlocks = nBlocks; a.tlMin = 0; a.declineNb0 = 0; a.onlyDeclined = 0;
    a.symScratch = nullptr; a.slotBitmap = nullptr; a.nSlots = 0; a.scratchSlotBytes = 0;
    return (int)launch_fse_decode(a, (hipStream_t)stream);
}

// =====================================================================================================
//  Workspaces.  A batch call walks its blocks in passes of `chunk` blocks; a pass uses one region of `chunk` entries per kind of per-block
//  scratch, each region rounded up to 256 bytes, and at most one small region of fixed size behind them.  Every kind of workspace is
//  described once, by a struct whose bytes_per_block is what its *_workspaceSize asks per block and whose constructor is the carve, so
//  the two cannot drift apart.  WS_SLACK pays for the rounding and the fixed region: each struct states its worst case, and every call
//  checks end() against the workspace it was given.
// =====================================================================================================
#define WS_SLACK 2048
#define WS_MAX_CHUNK 131072          // blocks per pass over the workspace (tables of 131072 blocks: 0.8 GiB)
// blocks per pass the size functions provide for
static size_t ws_pass_blocks(size_t nBlocks) { const size_t c = nBlocks < WS_MAX_CHUNK ? nBlocks : WS_MAX_CHUNK; return c ? c : 1; }
static size_t ws_size(size_t nBlocks, size_t perBlock, size_t pad = 0) { return ws_pass_blocks(nBlocks) * perBlock + pad + WS_SLACK; }
// largest chunk <= limit that is a whole number of device-filling rounds of the hot-loop kernel (no ragged last wave of workgroups)
static size_t round_chunk(size_t limit, size_t perRound)
{
    if (perRound == 0 || limit < perRound) return limit;
    return limit / perRound * perRound;
}
// blocks per pass a workspace of workspaceBytes holds (nBlocks > 0), or 0: not even one block -- hipErrorInvalidValue.  pad: bytes the kind
// needs once besides WS_SLACK; perRound: see round_chunk (0: calls without a hot loop)
static size_t ws_chunk(size_t workspaceBytes, size_t nBlocks, size_t perBlock, size_t pad = 0, size_t perRound = 0)
{
    if (workspaceBytes < perBlock + pad + WS_SLACK) return 0;
    const size_t chunk = (workspaceBytes - WS_SLACK - pad) / perBlock;
    return chunk >= nBlocks ? nBlocks : round_chunk(chunk, perRound);
}
// blocks of the pass that starts at block b0
static inline size_t pass_blocks(size_t nBlocks, size_t b0, size_t chunk) { return nBlocks - b0 < chunk ? nBlocks - b0 : chunk; }

struct Carver {
    u8* const base; u8* p;
    explicit Carver(void* ws) : base((u8*)ws), p((u8*)ws) {}
    template <class T> T* take(size_t bytes) { T* const r = (T*)p; p += align_up(bytes, 256); return r; }   // a per-chunk region
    template <class T> T* last(size_t bytes) { T* const r = (T*)p; p += bytes; return r; }                  // the region at the end: not rounded
    size_t used() const { return (size_t)(p - base); }
};
// The counter block at the head of the four compress-side workspaces: what k_hist leaves per block (256 counters, the largest symbol,
// its result) and the prepare kernel's record.  Padding: 4 regions, at most 4 x 255 bytes.
template <class Meta> struct CounterWs {
    static constexpr size_t bytes_per_block = 1024 + 4 + 8 + sizeof(Meta);
    unsigned* counts; unsigned* maxSVs; size_t* hres; Meta* meta;
    CounterWs(Carver& c, size_t chunk)
        : counts(c.take<unsigned>(chunk * 1024)), maxSVs(c.take<unsigned>(chunk * 4)), hres(c.take<size_t>(chunk * 8)), meta(c.take<Meta>(chunk * sizeof(Meta))) {}
    HistArgs hist_args(unsigned msv, const BlockView& src, size_t nb) const
    {
        HistArgs h;
        h.counts = counts; h.maxSVs = maxSVs; h.uniformMaxSV = msv; h.useUniformIn = 1; h.results = hres; h.src = src; h.nBlocks = nb;
        return h;
    }
};
// FSE_buildCTable / HUF_buildCTable over a batch: the counter block alone.  Worst case 4 x 255 = 1020 <= WS_SLACK.
template <class Meta> struct BuildCTableWs {
    static constexpr size_t bytes_per_block = CounterWs<Meta>::bytes_per_block;
    Carver c; CounterWs<Meta> cb;
    BuildCTableWs(void* ws, size_t chunk) : c(ws), cb(c, chunk) {}
    size_t end() const { return c.used(); }
};

// =====================================================================================================
//  one-shot FSE block API over a batch
// =====================================================================================================
struct FseCWs { size_t perBlock; size_t ctU32; size_t ts; unsigned maxTl; };
static FseCWs fse_cws(unsigned tableLog)
{
    FseCWs w;
    unsigned tl = tableLog ? tableLog : FSEHIP_FSE_DEFAULT_TABLELOG;
    if (tl < 9) tl = 9;                  // FSE_optimalTableLog may raise a small request up to highbit(255)+2 (fse_compress.c:316-333)
    if (tl > FSEHIP_FSE_MAX_TABLELOG) tl = FSEHIP_FSE_MAX_TABLELOG;
    w.maxTl = tl;
    w.ctU32 = FSEHIP_FSE_CTABLE_SIZE_U32(tl, 255);
    w.ts = (size_t)1 << tl;
    w.perBlock = 1024 + 4 + 8 + sizeof(FseMeta) + 4 * w.ctU32 + FSE_EBINS * sizeof(u32);
    return w;
}
// FSE compress: the counter block, the tables, the encoder's FSE_EBINS pace lists and their FSE_EBINS lengths.
// Worst case 6 x 255 + 4 * FSE_EBINS = 1546 <= WS_SLACK.
struct FseCompWs {
    Carver c; CounterWs<FseMeta> cb; u32* ctables; u32* encLists; u32* encCounts;
    FseCompWs(void* ws, size_t chunk, const FseCWs& w)
        : c(ws), cb(c, chunk), ctables(c.take<u32>(chunk * 4 * w.ctU32)), encLists(c.take<u32>(chunk * FSE_EBINS * sizeof(u32))),
          encCounts(c.last<u32>(FSE_EBINS * sizeof(u32))) {}
    size_t end() const { return c.used(); }
};

extern "C" size_t FSEHIP_FSE_compress_batch_workspaceSize(size_t nBlocks, unsigned tableLog) { return ws_size(nBlocks, fse_cws(tableLog).perBlock); }

extern "C" int FSEHIP_FSE_compress_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                         const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                         unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks,
                                         void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;          // include/fsehip.h: workspaces are 256-byte aligned; checked before anything else
    if (nBlocks == 0) return 0;
    if (tableLog > FSEHIP_FSE_MAX_TABLELOG)                                       // FSE_compress2 -> tableLog_tooLarge for every block (fse_compress.c:691)
        return batch_arg_error(d_results, nullptr, 0, dstCapacity, nBlocks, FSEHIP_ERROR(tableLog_tooLarge), 0, s);
    if (maxSymbolValue > 255 && tableLog != 0) {
        // FSE_compress2 carves its histogram scratch out of a fixed workspace behind a CTable sized from the REQUESTED maxSymbolValue
        // (lib/fse_compress.c:640-642,680-686): a request above 255 at tableLog 12 leaves the histogram less than HIST_WKSP_SIZE and
        // HIST_count_wksp refuses (lib/hist.c:168) -- after the srcSize <= 1 early-out.  Where the table still fits, the histogram
        // clamps the limit to 255 (lib/hist.c:169-172) and the call behaves as with 255; beyond the workspace the reference is undefined.
        const size_t wksp = 4 * (size_t)FSEHIP_FSE_CTABLE_SIZE_U32(FSEHIP_FSE_MAX_TABLELOG, 255) + ((size_t)1 << FSEHIP_FSE_MAX_TABLELOG);
        const size_t ctBytes = 4 * (1 + ((size_t)1 << (tableLog - 1)) + 2 * ((size_t)maxSymbolValue + 1));
        if (ctBytes <= wksp && wksp - ctBytes < 4096)
            return batch_arg_error(d_results, d_sizes, uniformSize, dstCapacity, nBlocks, FSEHIP_ERROR(workSpace_tooSmall), 2, s);
    }
    return fse_compress_view(d_dst, dstStride, dstCapacity, d_results, mkview(d_src, srcStride, d_sizes, uniformSize), maxSymbolValue, tableLog, nBlocks,
                             d_workspace, workspaceBytes, s);
}
// the pipeline itself, on any view of the source blocks (strided, or packed: BlockView::offsets -- the device frame writer, frame_dev.hip);
// arguments already checked
int fse_compress_view(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results, const BlockView& srcAll, unsigned maxSymbolValue, unsigned tableLog,
                      size_t nBlocks, void* d_workspace, size_t workspaceBytes, hipStream_t s)
{
    const FseCWs w = fse_cws(tableLog);
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, w.perBlock, 0, fse_encode_blocks_per_round(w.maxTl));
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const FseCompWs ws(d_workspace, chunk, w);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    unsigned msv = maxSymbolValue ? maxSymbolValue : 255;        // fse_compress.c:648
    if (msv > 255) msv = 255;
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        const BlockView src = subview(srcAll, b0);
        CK(launch_hist(ws.cb.hist_args(msv, src, nb), s));
        FseCPrepArgs c;
        c.counts = ws.cb.counts; c.maxSVs = ws.cb.maxSVs; c.histResults = ws.cb.hres; c.src = src;
        c.dst = (u8*)d_dst + b0 * dstStride; c.dstStride = dstStride; c.dstCapacity = dstCapacity;
        c.maxSVReq = msv; c.tableLogReq = tableLog;
        c.ctables = ws.ctables; c.ctStrideU32 = w.ctU32; c.maxTl = w.maxTl;
        c.meta = ws.cb.meta; c.results = d_results + b0; c.nBlocks = nb;
        CK(launch_fse_cprep(c, s));
        FseEncArgs e;
        e.dst = (u8*)d_dst + b0 * dstStride; e.dstStride = dstStride; e.dstCapacity = dstCapacity; e.results = d_results + b0;
        e.src = src; e.ctables = ws.ctables; e.ctStrideU32 = w.ctU32; e.meta = ws.cb.meta;
        e.maxTableLog = w.maxTl; e.G = 0; e.slotU32 = 0; e.nBlocks = nb; e.list = ws.encLists; e.count = ws.encCounts;
        CK(launch_fse_encode_auto(e, s));
    }
    return 0;
}

// FSE decode / FSE_buildDTable: per block the record, 256 counters, the decoder-format table (2 + 1 bytes per cell) and one entry in each
// decoder-class list; behind them the FSE_DCLS_COUNT list lengths.  Worst case 5 x 255 + 4 * FSE_DCLS_COUNT = 1467 <= WS_SLACK.
struct FseDecWs {
    static size_t bytes_per_block(unsigned maxLog) { return sizeof(FseMeta) + 512 + 3 * ((size_t)1 << maxLog) + FSE_DCLS_COUNT * sizeof(u32); }
    Carver c; FseMeta* meta; s16* norms; u16* atab; u8* symtab; u32* lists; u32* counts;
    FseDecWs(void* ws, size_t chunk, unsigned maxLog)
        : c(ws), meta(c.take<FseMeta>(chunk * sizeof(FseMeta))), norms(c.take<s16>(chunk * 512)), atab(c.take<u16>((chunk * 2) << maxLog)),
          symtab(c.take<u8>(chunk << maxLog)), lists(c.take<u32>(chunk * FSE_DCLS_COUNT * sizeof(u32))), counts(c.last<u32>(FSE_DCLS_COUNT * sizeof(u32))) {}
    size_t end() const { return c.used(); }
    // the prepare kernels' arguments for one pass (no raw / RLE records: set by the packed decoder alone)
    FseDPrepArgs dprep_args(const BlockView& cs, unsigned maxLog, size_t* results, size_t nb) const
    {
        FseDPrepArgs d;
        d.csrc = cs; d.maxLog = maxLog; d.atab = atab; d.symtab = symtab; d.norms = norms; d.meta = meta; d.lists = lists; d.counts = counts;
        d.results = results; d.nBlocks = nb; d.rawRle = 0; d.origSizes = nullptr; d.uniformOrig = 0;
        return d;
    }
};
static_assert(5 * 255 + FSE_DCLS_COUNT * sizeof(u32) <= WS_SLACK && 6 * 255 + FSE_EBINS * sizeof(u32) <= WS_SLACK, "WS_SLACK covers the padding of the FSE workspaces");
static unsigned clamp_maxlog(unsigned maxLog) { return (maxLog == 0 || maxLog > FSEHIP_FSE_MAX_TABLELOG) ? FSEHIP_FSE_MAX_TABLELOG : maxLog; }

extern "C" size_t FSEHIP_FSE_decompress_batch_workspaceSize(size_t nBlocks, unsigned maxLog) { return ws_size(nBlocks, FseDecWs::bytes_per_block(clamp_maxlog(maxLog))); }

static int fse_decompress_impl(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results, const BlockView& csAll, unsigned maxLog, size_t nBlocks,
                               void* d_workspace, size_t workspaceBytes, hipStream_t s, const size_t* d_origSizes, size_t uniformOrig, int rawRle,
                               const u64* d_dstOffsets = nullptr, const size_t* d_dstCaps = nullptr)
{
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;          // include/fsehip.h: workspaces are 256-byte aligned; checked before anything else
    if (nBlocks == 0) return 0;
    maxLog = clamp_maxlog(maxLog);
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, FseDecWs::bytes_per_block(maxLog), 0, fse_decode_blocks_per_round(maxLog));
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const FseDecWs ws(d_workspace, chunk, maxLog);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        const BlockView cs = subview(csAll, b0);
        if (rawRle) CK(launch_rawrle_expand((u8*)d_dst + b0 * dstStride, dstStride, dstCapacity, d_results + b0, cs, d_origSizes ? d_origSizes + b0 : nullptr, uniformOrig, nb, s));
        FseDPrepArgs d = ws.dprep_args(cs, maxLog, d_results + b0, nb);
        d.rawRle = rawRle; d.origSizes = d_origSizes ? d_origSizes + b0 : nullptr; d.uniformOrig = uniformOrig;
        CK(launch_fse_dprep(d, s));
        FseDecArgs e;
        e.dst = (u8*)d_dst + b0 * dstStride; e.dstStride = dstStride; e.dstCapacity = dstCapacity; e.results = d_results + b0;
        e.csrc = cs; e.dtables = nullptr; e.dtStrideU32 = 0; e.atab = ws.atab; e.symtab = ws.symtab; e.meta = ws.meta;
        e.maxTableLog = maxLog; e.G = 0; e.slotU32 = 0; e.nBlocks = nb; e.tlMin = 0; e.declineNb0 = 0; e.onlyDeclined = 0;
        e.symScratch = nullptr; e.slotBitmap = nullptr; e.nSlots = 0; e.scratchSlotBytes = 0;
        if (d_dstOffsets) { e.dst = (u8*)d_dst; e.dstOffsets = d_dstOffsets + b0; e.dstCaps = d_dstCaps + b0; }
        CK(launch_fse_decode_classes(e, ws.lists, ws.counts, s));
    }
    return 0;
}
extern "C" int FSEHIP_FSE_decompress_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                           const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                           unsigned maxLog, size_t nBlocks,
                                           void* d_workspace, size_t workspaceBytes, void* stream)
{
    return fse_decompress_impl(d_dst, dstStride, dstCapacity, d_results, mkview(d_cSrc, cStride, d_cSizes, uniformCSize), maxLog, nBlocks,
                               d_workspace, workspaceBytes, (hipStream_t)stream, nullptr, 0, 0);
}
int fse_decompress_view(void* d_dst, const u64* d_dstOffsets, const size_t* d_dstCaps, size_t* d_results, const BlockView& csrc, unsigned maxLog, size_t nBlocks,
                        void* d_workspace, size_t workspaceBytes, hipStream_t s)
{
    return fse_decompress_impl(d_dst, 0, 0, d_results, csrc, maxLog, nBlocks, d_workspace, workspaceBytes, s, nullptr, 0, 0, d_dstOffsets, d_dstCaps);
}
// FSE_decompress over a PACKED batch (FSEHIP_compact_batch), with the bench loop's treatment of declined blocks
extern "C" int FSEHIP_FSE_decompress_packed_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                                  const void* d_packed, const uint64_t* d_offsets, const size_t* d_origSizes, size_t uniformOrigSize,
                                                  unsigned maxLog, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    BlockView v = mkview(d_packed, 0, nullptr, 0);
    v.offsets = (const u64*)d_offsets;
    return fse_decompress_impl(d_dst, dstStride, dstCapacity, d_results, v, maxLog, nBlocks, d_workspace, workspaceBytes, (hipStream_t)stream,
                               d_origSizes, uniformOrigSize, 1);
}

// =====================================================================================================
//  Tables for the *_usingCTable / *_usingDTable batch calls, built on the device (SURVEY 8(a') g1-g3, g5-g6 as calls of their own)
// =====================================================================================================
extern "C" size_t FSEHIP_FSE_buildCTable_batch_workspaceSize(size_t nBlocks) { return ws_size(nBlocks, BuildCTableWs<FseMeta>::bytes_per_block); }
extern "C" int FSEHIP_FSE_buildCTable_batch(FSEHIP_FSE_CTable* d_ctables, size_t ctableStrideU32, void* d_headers, size_t headerStride, size_t headerCapacity,
                                            size_t* d_results, const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                            unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (nBlocks == 0) return 0;
    if (tableLog > FSEHIP_FSE_MAX_TABLELOG) return batch_arg_error(d_results, nullptr, 0, headerCapacity, nBlocks, FSEHIP_ERROR(tableLog_tooLarge), 0, s);
    const FseCWs w = fse_cws(tableLog);
    if (ctableStrideU32 < w.ctU32) return (int)hipErrorInvalidValue;              // room for FSE_CTABLE_SIZE_U32(largest table log the request can lead to, 255)
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, BuildCTableWs<FseMeta>::bytes_per_block);
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const BuildCTableWs<FseMeta> ws(d_workspace, chunk);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    unsigned msv = maxSymbolValue ? maxSymbolValue : 255;
    if (msv > 255) msv = 255;
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        const BlockView src = mkview((const u8*)d_src + b0 * srcStride, srcStride, d_sizes ? d_sizes + b0 : nullptr, uniformSize);
        CK(launch_hist(ws.cb.hist_args(msv, src, nb), s));
        FseCPrepArgs c;
        c.counts = ws.cb.counts; c.maxSVs = ws.cb.maxSVs; c.histResults = ws.cb.hres; c.src = src;
        c.dst = (u8*)d_headers + b0 * headerStride; c.dstStride = headerStride; c.dstCapacity = headerCapacity;
        c.maxSVReq = msv; c.tableLogReq = tableLog;
        c.ctables = d_ctables + b0 * ctableStrideU32; c.ctStrideU32 = ctableStrideU32; c.maxTl = w.maxTl;
        c.meta = ws.cb.meta; c.results = d_results + b0; c.nBlocks = nb;
        CK(launch_fse_cprep(c, s));
        CK(launch_hdr_results(ws.cb.meta, sizeof(FseMeta), d_results + b0, nb, s));
    }
    return 0;
}

// ---- the glue steps as calls of their own (fsehip.h "Table glue, step by step")
extern "C" int FSEHIP_FSE_normalizeCount_batch(short* d_norms, size_t normStride, unsigned tableLog, const unsigned* d_counts, size_t countStride,
                                               const size_t* d_totals, const unsigned* d_maxSymbolValues, size_t nBlocks, size_t* d_results, void* stream)
{
    if (nBlocks == 0) return 0;
    if (!d_norms || !d_counts || !d_totals || !d_maxSymbolValues || !d_results || normStride < 256 || countStride < 256) return (int)hipErrorInvalidValue;
    return (int)launch_fse_glue_normalize((s16*)d_norms, normStride, tableLog, d_counts, countStride, d_totals, d_maxSymbolValues, d_results, nBlocks, (hipStream_t)stream);
}
extern "C" int FSEHIP_FSE_writeNCount_batch(void* d_headers, size_t headerStride, size_t headerCapacity, const short* d_norms, size_t normStride,
                                            const unsigned* d_maxSymbolValues, unsigned tableLog, size_t nBlocks, size_t* d_results, void* stream)
{
    if (nBlocks == 0) return 0;
    if (!d_headers || !d_norms || !d_maxSymbolValues || !d_results || normStride < 256 || headerCapacity > headerStride) return (int)hipErrorInvalidValue;
    return (int)launch_fse_glue_write_ncount((u8*)d_headers, headerStride, headerCapacity, (const s16*)d_norms, normStride, d_maxSymbolValues, tableLog, d_results, nBlocks,
                                             (hipStream_t)stream);
}
extern "C" int FSEHIP_FSE_readNCount_batch(short* d_norms, size_t normStride, unsigned* d_maxSymbolValues, unsigned* d_tableLogs,
                                           const void* d_headers, size_t headerStride, const size_t* d_headerSizes, size_t uniformHeaderSize,
                                           size_t nBlocks, size_t* d_results, void* stream)
{
    if (nBlocks == 0) return 0;
    if (!d_norms || !d_maxSymbolValues || !d_tableLogs || !d_headers || !d_results) return (int)hipErrorInvalidValue;
    return (int)launch_fse_glue_read_ncount((s16*)d_norms, normStride, d_maxSymbolValues, d_tableLogs, mkview(d_headers, headerStride, d_headerSizes, uniformHeaderSize),
                                            d_results, nBlocks, (hipStream_t)stream);
}

extern "C" size_t FSEHIP_FSE_buildDTable_batch_workspaceSize(size_t nBlocks, unsigned maxLog) { return FSEHIP_FSE_decompress_batch_workspaceSize(nBlocks, maxLog); }
extern "C" int FSEHIP_FSE_buildDTable_batch(FSEHIP_FSE_DTable* d_dtables, size_t dtableStrideU32, size_t* d_results,
                                            const void* d_headers, size_t headerStride, const size_t* d_headerSizes, size_t uniformHeaderSize,
                                            unsigned maxLog, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (nBlocks == 0) return 0;
    maxLog = clamp_maxlog(maxLog);
    if (dtableStrideU32 < FSEHIP_FSE_DTABLE_SIZE_U32(maxLog)) return (int)hipErrorInvalidValue;
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, FseDecWs::bytes_per_block(maxLog));
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const FseDecWs ws(d_workspace, chunk, maxLog);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        const FseDPrepArgs d = ws.dprep_args(mkview((const u8*)d_headers + b0 * headerStride, headerStride, d_headerSizes ? d_headerSizes + b0 : nullptr, uniformHeaderSize),
                                             maxLog, d_results + b0, nb);
        CK(launch_fse_dprep(d, s));
        CK(launch_fse_export_dtables(d, d_dtables + b0 * dtableStrideU32, dtableStrideU32, s));
        CK(launch_hdr_results(ws.meta, sizeof(FseMeta), d_results + b0, nb, s));
    }
    return 0;
}

// ---- the table builders on counters the caller supplies (fsehip.h "Table glue, step by step")
extern "C" int FSEHIP_FSE_buildCTable_fromNorm_batch(FSEHIP_FSE_CTable* d_ctables, size_t ctableStrideU32, const short* d_norms, size_t normStride,
                                                     const unsigned* d_maxSymbolValues, unsigned tableLog, size_t nBlocks, size_t* d_results, void* stream)
{
    if (nBlocks == 0) return 0;
    if (!d_ctables || !d_norms || !d_maxSymbolValues || !d_results || normStride < 256) return (int)hipErrorInvalidValue;
    if (tableLog >= 1 && tableLog <= FSEHIP_FSE_MAX_TABLELOG && ctableStrideU32 < FSEHIP_FSE_CTABLE_SIZE_U32(tableLog, 255)) return (int)hipErrorInvalidValue;
    return (int)launch_fse_ctable_from_norm((const s16*)d_norms, normStride, d_maxSymbolValues, tableLog, d_ctables, ctableStrideU32, d_results, nBlocks, (hipStream_t)stream);
}
extern "C" size_t FSEHIP_FSE_buildDTable_fromNorm_batch_workspaceSize(size_t nBlocks, unsigned tableLog) { return FSEHIP_FSE_decompress_batch_workspaceSize(nBlocks, tableLog); }
extern "C" int FSEHIP_FSE_buildDTable_fromNorm_batch(FSEHIP_FSE_DTable* d_dtables, size_t dtableStrideU32, const short* d_norms, size_t normStride,
                                                     const unsigned* d_maxSymbolValues, unsigned tableLog, size_t nBlocks, size_t* d_results,
                                                     void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (nBlocks == 0) return 0;
    if (!d_dtables || !d_norms || !d_maxSymbolValues || !d_results || normStride < 256) return (int)hipErrorInvalidValue;
    if (tableLog > FSEHIP_FSE_MAX_TABLELOG) return batch_arg_error(d_results, nullptr, 0, 0, nBlocks, FSEHIP_ERROR(tableLog_tooLarge), 0, s);   // lib/fse_decompress.c:84
    const unsigned maxLog = tableLog ? tableLog : 1;                     // (tableLog 0: refused per block, GENERIC)
    if (dtableStrideU32 < FSEHIP_FSE_DTABLE_SIZE_U32(maxLog)) return (int)hipErrorInvalidValue;
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, FseDecWs::bytes_per_block(maxLog));
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const FseDecWs ws(d_workspace, chunk, maxLog);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        const FseDPrepArgs d = ws.dprep_args(mkview(nullptr, 0, nullptr, 0), maxLog, d_results + b0, nb);
        CK(launch_fse_dprep_from_norm(d, (const s16*)d_norms + b0 * normStride, normStride, d_maxSymbolValues + b0, tableLog, s));
        CK(launch_fse_export_dtables(d, d_dtables + b0 * dtableStrideU32, dtableStrideU32, s));
        CK(launch_hdr_results(ws.meta, sizeof(FseMeta), d_results + b0, nb, s));   // (hdrSize 0: FSE_buildDTable returns 0)
    }
    return 0;
}

extern "C" size_t FSEHIP_HUF_buildCTable_batch_workspaceSize(size_t nBlocks) { return ws_size(nBlocks, BuildCTableWs<HufMeta>::bytes_per_block); }
extern "C" int FSEHIP_HUF_buildCTable_batch(FSEHIP_HUF_CElt* d_ctables, size_t ctableStrideU32, void* d_headers, size_t headerStride, size_t headerCapacity,
                                            size_t* d_results, const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                            unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (nBlocks == 0) return 0;
    if (tableLog > FSEHIP_HUF_TABLELOG_MAX || maxSymbolValue > 255)
        return batch_arg_error(d_results, d_sizes, uniformSize, headerCapacity, nBlocks,
                               tableLog > FSEHIP_HUF_TABLELOG_MAX ? FSEHIP_ERROR(tableLog_tooLarge) : FSEHIP_ERROR(maxSymbolValue_tooLarge), 1, s);
    if (ctableStrideU32 < 256) return (int)hipErrorInvalidValue;
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, BuildCTableWs<HufMeta>::bytes_per_block);
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const BuildCTableWs<HufMeta> ws(d_workspace, chunk);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    const unsigned msv = maxSymbolValue ? maxSymbolValue : 255;
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        const BlockView src = mkview((const u8*)d_src + b0 * srcStride, srcStride, d_sizes ? d_sizes + b0 : nullptr, uniformSize);
        CK(launch_hist(ws.cb.hist_args(msv, src, nb), s));
        HufCPrepArgs c;
        c.counts = ws.cb.counts; c.maxSVs = ws.cb.maxSVs; c.histResults = ws.cb.hres; c.src = src;
        c.dst = (u8*)d_headers + b0 * headerStride; c.dstStride = headerStride; c.dstCapacity = headerCapacity;
        c.maxSVReq = msv; c.huffLogReq = tableLog; c.ctables = d_ctables + b0 * ctableStrideU32; c.ctStrideU32 = ctableStrideU32;
        c.meta = ws.cb.meta; c.results = d_results + b0; c.nBlocks = nb;
        CK(launch_huf_cprep(c, s, nullptr));
        CK(launch_hdr_results(ws.cb.meta, sizeof(HufMeta), d_results + b0, nb, s));
    }
    return 0;
}

// ---- the Huff0 table glue on counters / tables the caller supplies (fsehip.h "Table glue, step by step"): HUF_buildCTable and HUF_writeCTable
extern "C" int FSEHIP_HUF_buildCTable_fromCount_batch(FSEHIP_HUF_CElt* d_ctables, size_t ctableStrideU32, const unsigned* d_counts, size_t countStride,
                                                      const unsigned* d_maxSymbolValues, unsigned maxNbBits, size_t nBlocks, size_t* d_results, void* stream)
{
    if (nBlocks == 0) return 0;
    if (!d_ctables || !d_counts || !d_maxSymbolValues || !d_results || ctableStrideU32 < 256 || (ctableStrideU32 & 3) || countStride != 256) return (int)hipErrorInvalidValue;
    HufCPrepArgs c;
    c.counts = d_counts; c.maxSVs = d_maxSymbolValues; c.histResults = nullptr; c.src = mkview(nullptr, 0, nullptr, 0);
    c.dst = nullptr; c.dstStride = 0; c.dstCapacity = 0; c.maxSVReq = 255; c.huffLogReq = maxNbBits;
    c.ctables = d_ctables; c.ctStrideU32 = ctableStrideU32; c.meta = nullptr; c.results = d_results; c.nBlocks = nBlocks;
    return (int)launch_huf_cprep_glue(c, 1, (hipStream_t)stream);
}
extern "C" int FSEHIP_HUF_writeCTable_batch(void* d_headers, size_t headerStride, size_t headerCapacity, const FSEHIP_HUF_CElt* d_ctables, size_t ctableStrideU32,
                                            const unsigned* d_maxSymbolValues, unsigned huffLog, size_t nBlocks, size_t* d_results, void* stream)
{
    if (nBlocks == 0) return 0;
    if (!d_headers || !d_ctables || !d_maxSymbolValues || !d_results || ctableStrideU32 < 256 || (ctableStrideU32 & 3) || headerCapacity > headerStride) return (int)hipErrorInvalidValue;
    HufCPrepArgs c;
    c.counts = nullptr; c.maxSVs = d_maxSymbolValues; c.histResults = nullptr; c.src = mkview(nullptr, 0, nullptr, 0);
    c.dst = (u8*)d_headers; c.dstStride = headerStride; c.dstCapacity = headerCapacity; c.maxSVReq = 255; c.huffLogReq = huffLog;
    c.ctables = (u32*)d_ctables; c.ctStrideU32 = ctableStrideU32; c.meta = nullptr; c.results = d_results; c.nBlocks = nBlocks;
    return (int)launch_huf_cprep_glue(c, 2, (hipStream_t)stream);
}

// HUF_readDTableX1 / X2 over a batch: the record and one entry in each decoder-class list per block, behind them the HUF_DCLS_COUNT list
// lengths.  Worst case 2 x 255 + 4 * HUF_DCLS_COUNT = 542 <= WS_SLACK.
struct HufReadDTableWs {
    static constexpr size_t bytes_per_block = sizeof(HufMeta) + HUF_DCLS_COUNT * sizeof(u32);
    Carver c; HufMeta* meta; u32* lists; u32* counts;
    HufReadDTableWs(void* ws, size_t chunk)
        : c(ws), meta(c.take<HufMeta>(chunk * sizeof(HufMeta))), lists(c.take<u32>(chunk * HUF_DCLS_COUNT * sizeof(u32))), counts(c.last<u32>(HUF_DCLS_COUNT * sizeof(u32))) {}
    size_t end() const { return c.used(); }
};
// (the two calls below, behind their own checks of maxTableLog and the table stride)
static int huf_read_dtable_batch(hipError_t (*launch)(const HufDPrepArgs&, hipStream_t), FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                 size_t* d_results, const void* d_src, size_t srcStride, const size_t* d_srcSizes, size_t uniformSrcSize,
                                 size_t nBlocks, void* d_workspace, size_t workspaceBytes, hipStream_t s)
{
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, HufReadDTableWs::bytes_per_block);
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const HufReadDTableWs ws(d_workspace, chunk);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        HufDPrepArgs d;
        d.csrc = mkview((const u8*)d_src + b0 * srcStride, srcStride, d_srcSizes ? d_srcSizes + b0 : nullptr, uniformSrcSize);
        d.dstSizes = mkview(nullptr, 0, nullptr, 0); d.dst = nullptr; d.dstStride = 0;
        d.dtables = d_dtables + b0 * dtableStrideU32; d.dtStrideU32 = dtableStrideU32; d.meta = ws.meta; d.lists = ws.lists; d.counts = ws.counts;
        d.results = d_results + b0; d.nBlocks = nb; d.tableOnly = 1; d.dtMaxLog = maxTableLog;
        CK(launch(d, s));
    }
    return 0;
}
extern "C" size_t FSEHIP_HUF_readDTableX1_batch_workspaceSize(size_t nBlocks) { return ws_size(nBlocks, HufReadDTableWs::bytes_per_block); }
extern "C" int FSEHIP_HUF_readDTableX1_batch(FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog, size_t* d_results,
                                             const void* d_src, size_t srcStride, const size_t* d_srcSizes, size_t uniformSrcSize,
                                             size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (nBlocks == 0) return 0;
    if (maxTableLog == 0 || maxTableLog > FSEHIP_HUF_TABLELOG_MAX) maxTableLog = FSEHIP_HUF_TABLELOG_MAX;
    if (dtableStrideU32 < 1 + ((size_t)1 << maxTableLog)) return (int)hipErrorInvalidValue;       // HUF_DTABLE_SIZE(maxTableLog)
    return huf_read_dtable_batch(launch_huf_dprep, d_dtables, dtableStrideU32, maxTableLog, d_results, d_src, srcStride, d_srcSizes, uniformSrcSize,
                                 nBlocks, d_workspace, workspaceBytes, (hipStream_t)stream);
}

// HUF_readDTableX2 over a batch (lib/huf_decompress.c:551-649): double-symbol cells, 1 << maxTableLog of them behind the descriptor.  maxTableLog is
// DTableDesc.maxTableLog as the reference reads it: above 12 every block fails with tableLog_tooLarge (:587), a header deeper than it likewise (:594).
extern "C" size_t FSEHIP_HUF_readDTableX2_batch_workspaceSize(size_t nBlocks) { return FSEHIP_HUF_readDTableX1_batch_workspaceSize(nBlocks); }
extern "C" int FSEHIP_HUF_readDTableX2_batch(FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog, size_t* d_results,
                                             const void* d_src, size_t srcStride, const size_t* d_srcSizes, size_t uniformSrcSize,
                                             size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (nBlocks == 0) return 0;
    if (maxTableLog <= FSEHIP_HUF_TABLELOG_MAX && dtableStrideU32 < 1 + ((size_t)1 << maxTableLog)) return (int)hipErrorInvalidValue;   // HUF_DTABLE_SIZE(maxTableLog)
    return huf_read_dtable_batch(launch_huf_dprep_x2, d_dtables, dtableStrideU32, maxTableLog, d_results, d_src, srcStride, d_srcSizes, uniformSrcSize,
                                 nBlocks, d_workspace, workspaceBytes, (hipStream_t)stream);
}

// =====================================================================================================
//  a4 / a5: Huff0 hot loops over a batch
// =====================================================================================================
extern "C" int FSEHIP_HUF_compress4X_usingCTable_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                                       const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                                       const FSEHIP_HUF_CElt* d_ctables, size_t ctableStrideU32,
                                                       size_t nBlocks, void* stream)
{
    HufEncArgs a;
    a.dst = (u8*)d_dst; a.dstStride = dstStride; a.dstCapacity = dstCapacity; a.results = d_results;
    a.src = mkview(d_src, srcStride, d_sizes, uniformSize);
    a.ctables = d_ctables; a.ctStrideU32 = ctableStrideU32; a.meta = nullptr; a.streams = 4; a.split1X = 0; a.nBlocks = nBlocks;
    return (int)launch_huf_encode(a, (hipStream_t)stream);
}

// HUF_compress1X_usingCTable over a batch (lib/huf.h:290, body lib/huf_compress.c:457-502): one stream per block
extern "C" int FSEHIP_HUF_compress1X_usingCTable_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                                       const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                                       const FSEHIP_HUF_CElt* d_ctables, size_t ctableStrideU32,
                                                       size_t nBlocks, void* stream)
{
    HufEncArgs a;
    a.dst = (u8*)d_dst; a.dstStride = dstStride; a.dstCapacity = dstCapacity; a.results = d_results;
    a.src = mkview(d_src, srcStride, d_sizes, uniformSize);
    a.ctables = d_ctables; a.ctStrideU32 = ctableStrideU32; a.meta = nullptr; a.streams = 1; a.split1X = 1; a.nBlocks = nBlocks;
    return (int)launch_huf_encode(a, (hipStream_t)stream);
}

// HUF_decompress{4X1,4X,1X1,1X}_usingDTable over a batch: four streams per block, or one -- what HUF_compress1X_usingCTable writes (lib/huf.h:318-320;
// lib/huf_decompress.c:239-260,367-375,961-975); acceptX2: dispatch per block on the table's type (lib/huf_decompress.c:980-997) instead of single-symbol tables alone
static int huf_dtable_batch(int streams, int acceptX2, void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                            size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                            const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog, size_t nBlocks, void* stream)
{
    if (maxTableLog == 0 || maxTableLog > FSEHIP_HUF_TABLELOG_MAX) maxTableLog = FSEHIP_HUF_TABLELOG_MAX;
    HufDecArgs a;
    a.dst = (u8*)d_dst; a.dstStride = dstStride; a.dstSizes = mkview(nullptr, 0, d_dstSizes, uniformDstSize);
    a.results = d_results; a.csrc = mkview(d_cSrc, cStride, d_cSizes, uniformCSize);
    a.dtables = d_dtables; a.dtStrideU32 = dtableStrideU32; a.meta = nullptr;
    a.maxTableLog = maxTableLog; a.G = 0; a.slotU32 = 0; a.streams = streams; a.acceptX2 = acceptX2; a.onlyDeclined = 0; a.classLo = 0; a.nBlocks = nBlocks;
    return (int)launch_huf_decode(a, (hipStream_t)stream);
}
extern "C" int FSEHIP_HUF_decompress4X1_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                          size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                          const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                          size_t nBlocks, void* stream)
{
    return huf_dtable_batch(4, 0, d_dst, dstStride, d_dstSizes, uniformDstSize, d_results, d_cSrc, cStride, d_cSizes, uniformCSize, d_dtables, dtableStrideU32, maxTableLog, nBlocks, stream);
}
extern "C" int FSEHIP_HUF_decompress4X_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                         size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                         const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                         size_t nBlocks, void* stream)
{
    return huf_dtable_batch(4, 1, d_dst, dstStride, d_dstSizes, uniformDstSize, d_results, d_cSrc, cStride, d_cSizes, uniformCSize, d_dtables, dtableStrideU32, maxTableLog, nBlocks, stream);
}
extern "C" int FSEHIP_HUF_decompress1X1_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                          size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                          const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                          size_t nBlocks, void* stream)
{
    return huf_dtable_batch(1, 0, d_dst, dstStride, d_dstSizes, uniformDstSize, d_results, d_cSrc, cStride, d_cSizes, uniformCSize, d_dtables, dtableStrideU32, maxTableLog, nBlocks, stream);
}
extern "C" int FSEHIP_HUF_decompress1X_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                         size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                         const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                         size_t nBlocks, void* stream)
{
    return huf_dtable_batch(1, 1, d_dst, dstStride, d_dstSizes, uniformDstSize, d_results, d_cSrc, cStride, d_cSizes, uniformCSize, d_dtables, dtableStrideU32, maxTableLog, nBlocks, stream);
}

// HUF_decompress4X2_usingDTable / HUF_decompress1X2_usingDTable over a batch (lib/huf_decompress.c:867-875, :907-915): the dispatching routes above, after
// which a block whose table is not a double-symbol one has GENERIC for its result (:873, :913) -- what such a block's destination holds is unspecified
__global__ void k_huf_x2_strict(size_t* results, const u32* dtables, size_t dtStrideU32, size_t nBlocks)
{
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nBlocks && ((dtables[b * dtStrideU32] >> 8) & 0xFFu) != 1u) results[b] = FERR(GENERIC);
}
static int huf_x2_strict(size_t* d_results, const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, size_t nBlocks, void* stream)
{
    if (nBlocks == 0) return 0;
    hipLaunchKernelGGL(k_huf_x2_strict, dim3((unsigned)((nBlocks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_results, d_dtables, dtableStrideU32, nBlocks);
    return (int)hipGetLastError();
}
extern "C" int FSEHIP_HUF_decompress4X2_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                          size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                          const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                          size_t nBlocks, void* stream)
{
    const int e = FSEHIP_HUF_decompress4X_usingDTable_batch(d_dst, dstStride, d_dstSizes, uniformDstSize, d_results, d_cSrc, cStride, d_cSizes, uniformCSize,
                                                            d_dtables, dtableStrideU32, maxTableLog, nBlocks, stream);
    return e ? e : huf_x2_strict(d_results, d_dtables, dtableStrideU32, nBlocks, stream);
}
extern "C" int FSEHIP_HUF_decompress1X2_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                          size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                          const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                          size_t nBlocks, void* stream)
{
    const int e = FSEHIP_HUF_decompress1X_usingDTable_batch(d_dst, dstStride, d_dstSizes, uniformDstSize, d_results, d_cSrc, cStride, d_cSizes, uniformCSize,
                                                            d_dtables, dtableStrideU32, maxTableLog, nBlocks, stream);
    return e ? e : huf_x2_strict(d_results, d_dtables, dtableStrideU32, nBlocks, stream);
}

// =====================================================================================================
//  one-shot Huff0 block API over a batch
// =====================================================================================================
// Huff0 compress: the counter block and the tables (256 HUF_CElt per block); behind them the node scratch, 4 KiB per block in slabs of 64 blocks,
// for whose last slab the size function adds HUF_CWS_NODE_PAD.  Worst case 5 x 255 = 1275 <= WS_SLACK, and the slab rounding 63 x 4096 < the pad.
struct HufCompWs {
    static constexpr size_t bytes_per_block = CounterWs<HufMeta>::bytes_per_block + 1024 + 4096;
    static constexpr size_t pad = 64 * 4096;
    Carver c; CounterWs<HufMeta> cb; u32* ctables; void* nodes;
    HufCompWs(void* ws, size_t chunk) : c(ws), cb(c, chunk), ctables(c.take<u32>(chunk * 1024)), nodes(c.last<u8>((chunk + 63) / 64 * 64 * 4096)) {}
    size_t end() const { return c.used(); }
};
extern "C" size_t FSEHIP_HUF_compress_batch_workspaceSize(size_t nBlocks) { return ws_size(nBlocks, HufCompWs::bytes_per_block, HufCompWs::pad); }

int huf_compress_batch_impl(int streams, void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                            const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                            unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;          // include/fsehip.h: workspaces are 256-byte aligned; checked before anything else
    if (nBlocks == 0) return 0;
    if (tableLog > FSEHIP_HUF_TABLELOG_MAX || maxSymbolValue > 255)               // huf_compress.c:656-660, in the reference's order, per block
        return batch_arg_error(d_results, d_sizes, uniformSize, dstCapacity, nBlocks,
                               tableLog > FSEHIP_HUF_TABLELOG_MAX ? FSEHIP_ERROR(tableLog_tooLarge) : FSEHIP_ERROR(maxSymbolValue_tooLarge), 1, s);
    return huf_compress_view(streams, d_dst, dstStride, dstCapacity, d_results, mkview(d_src, srcStride, d_sizes, uniformSize), maxSymbolValue, tableLog, nBlocks,
                             d_workspace, workspaceBytes, s);
}
// (as fse_compress_view)
int huf_compress_view(int streams, void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results, const BlockView& srcAll, unsigned maxSymbolValue,
                      unsigned tableLog, size_t nBlocks, void* d_workspace, size_t workspaceBytes, hipStream_t s)
{
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, HufCompWs::bytes_per_block, HufCompWs::pad);
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const HufCompWs ws(d_workspace, chunk);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    const unsigned msv = maxSymbolValue ? maxSymbolValue : 255;   // huf_compress.c:661
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        const BlockView src = subview(srcAll, b0);
        CK(launch_hist(ws.cb.hist_args(msv, src, nb), s));
        HufCPrepArgs c;
        c.counts = ws.cb.counts; c.maxSVs = ws.cb.maxSVs; c.histResults = ws.cb.hres; c.src = src;
        c.dst = (u8*)d_dst + b0 * dstStride; c.dstStride = dstStride; c.dstCapacity = dstCapacity;
        c.maxSVReq = msv; c.huffLogReq = tableLog; c.ctables = ws.ctables; c.ctStrideU32 = 256;
        c.meta = ws.cb.meta; c.results = d_results + b0; c.nBlocks = nb;
        CK(launch_huf_cprep(c, s, ws.nodes));
        HufEncArgs e;
        e.dst = (u8*)d_dst + b0 * dstStride; e.dstStride = dstStride; e.dstCapacity = dstCapacity; e.results = d_results + b0;
        e.src = src; e.ctables = ws.ctables; e.ctStrideU32 = 256; e.meta = ws.cb.meta; e.streams = streams; e.split1X = 0; e.nBlocks = nb;
        CK(launch_huf_encode(e, s));
    }
    return 0;
}

extern "C" int FSEHIP_HUF_compress_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                         const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                         unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks,
                                         void* d_workspace, size_t workspaceBytes, void* stream)
{
    return huf_compress_batch_impl(4, d_dst, dstStride, dstCapacity, d_results, d_src, srcStride, d_sizes, uniformSize, maxSymbolValue, tableLog, nBlocks,
                             d_workspace, workspaceBytes, stream);
}

// Huff0 decode: the record, the table (2-byte cells: 2^tableLog cells = 2^(tableLog-1) words) and one entry in each decoder-class list per block,
// behind them the HUF_DCLS_COUNT list lengths.  Worst case 3 x 255 + 4 * HUF_DCLS_COUNT = 797 <= WS_SLACK.
struct HufDecWs {
    static constexpr size_t dtU32 = FSEHIP_HUF_DTABLE_SIZE_U32(FSEHIP_HUF_TABLELOG_MAX - 1);
    static constexpr size_t bytes_per_block = sizeof(HufMeta) + 4 * dtU32 + HUF_DCLS_COUNT * sizeof(u32);
    Carver c; HufMeta* meta; u32* dtables; u32* lists; u32* counts;
    HufDecWs(void* ws, size_t chunk)
        : c(ws), meta(c.take<HufMeta>(chunk * sizeof(HufMeta))), dtables(c.take<u32>(chunk * dtU32 * 4)), lists(c.take<u32>(chunk * HUF_DCLS_COUNT * sizeof(u32))),
          counts(c.last<u32>(HUF_DCLS_COUNT * sizeof(u32))) {}
    size_t end() const { return c.used(); }
};
extern "C" size_t FSEHIP_HUF_decompress_batch_workspaceSize(size_t nBlocks) { return ws_size(nBlocks, HufDecWs::bytes_per_block); }

static int huf_decompress_impl(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize, size_t* d_results, const BlockView& csAll,
                               size_t nBlocks, void* d_workspace, size_t workspaceBytes, hipStream_t s, const u64* d_dstOffsets = nullptr)
{
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;          // include/fsehip.h: workspaces are 256-byte aligned; checked before anything else
    if (nBlocks == 0) return 0;
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, HufDecWs::bytes_per_block);
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const HufDecWs ws(d_workspace, chunk);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    const size_t dtU32 = HufDecWs::dtU32;
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        const BlockView cs = subview(csAll, b0);
        const BlockView ds = mkview(nullptr, 0, d_dstSizes ? d_dstSizes + b0 : nullptr, uniformDstSize);
        HufDPrepArgs d;
        d.csrc = cs; d.dstSizes = ds; d.dst = (u8*)d_dst + b0 * dstStride; d.dstStride = dstStride;
        d.dtables = ws.dtables; d.dtStrideU32 = dtU32; d.meta = ws.meta; d.lists = ws.lists; d.counts = ws.counts; d.results = d_results + b0; d.nBlocks = nb;
        d.tableOnly = 0; d.dtMaxLog = FSEHIP_HUF_TABLELOG_MAX - 1;
        if (d_dstOffsets) { d.dst = (u8*)d_dst; d.dstOffsets = d_dstOffsets + b0; }
        CK(launch_huf_dprep(d, s));
        HufDecArgs e;
        e.dst = (u8*)d_dst + b0 * dstStride; e.dstStride = dstStride; e.dstSizes = ds; e.results = d_results + b0;
        e.csrc = cs; e.dtables = ws.dtables; e.dtStrideU32 = dtU32; e.meta = ws.meta;
        e.maxTableLog = FSEHIP_HUF_TABLELOG_MAX; e.G = 0; e.slotU32 = 0; e.streams = 4; e.acceptX2 = 0; e.onlyDeclined = 0; e.classLo = 0; e.nBlocks = nb;
        if (d_dstOffsets) { e.dst = (u8*)d_dst; e.dstOffsets = d_dstOffsets + b0; }
        CK(launch_huf_decode_classes(e, ws.lists, ws.counts, s));
    }
    return 0;
}
extern "C" int FSEHIP_HUF_decompress_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                           size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                           size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    return huf_decompress_impl(d_dst, dstStride, d_dstSizes, uniformDstSize, d_results, mkview(d_cSrc, cStride, d_cSizes, uniformCSize), nBlocks,
                               d_workspace, workspaceBytes, (hipStream_t)stream);
}
int huf_decompress_view(void* d_dst, const u64* d_dstOffsets, const size_t* d_dstSizes, size_t* d_results, const BlockView& csrc, size_t nBlocks,
                        void* d_workspace, size_t workspaceBytes, hipStream_t s)
{
    return huf_decompress_impl(d_dst, 0, d_dstSizes, 0, d_results, csrc, nBlocks, d_workspace, workspaceBytes, s, d_dstOffsets);
}
// HUF_decompress over a PACKED batch (FSEHIP_compact_batch): HUF_decompress itself takes a record as long as the block for the block and
// a record of one byte for that byte repeated (lib/huf_decompress.c:1063-1066), which is how the compaction stores what HUF_compress declined
extern "C" int FSEHIP_HUF_decompress_packed_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize, size_t* d_results,
                                                  const void* d_packed, const uint64_t* d_offsets, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    BlockView v = mkview(d_packed, 0, nullptr, 0);
    v.offsets = (const u64*)d_offsets;
    return huf_decompress_impl(d_dst, dstStride, d_dstSizes, uniformDstSize, d_results, v, nBlocks, d_workspace, workspaceBytes, (hipStream_t)stream);
}

// =====================================================================================================
//  FSE for 16-bit symbols (lib/fseU16.c)
// =====================================================================================================
// 16-bit symbols, compress: the state table and the symbol transforms per block, then the records.  Worst case 2 x 255 = 510 <= WS_SLACK.
struct U16CompWs {
    static constexpr size_t stBytes = (size_t)2 << FSEHIP_FSEU16_MAX_TABLELOG, ttBytes = 8 * (FSEHIP_FSEU16_MAX_SYMBOL_VALUE + 1);
    static constexpr size_t bytes_per_block = stBytes + ttBytes + sizeof(U16Meta);
    Carver c; u16* stateTables; u32* symTT; U16Meta* meta;
    U16CompWs(void* ws, size_t chunk)
        : c(ws), stateTables(c.take<u16>(chunk * stBytes)), symTT(c.take<u32>(chunk * ttBytes)), meta(c.last<U16Meta>(chunk * sizeof(U16Meta))) {}
    size_t end() const { return c.used(); }
};
// 16-bit symbols, decode: a 32 KiB slot per block (internal.h, U16DArgs), then the records.  Worst case 255 <= WS_SLACK.
struct U16DecWs {
    static constexpr size_t bytes_per_block = ((size_t)4 << FSEHIP_FSEU16_MAX_TABLELOG) + sizeof(U16Meta);
    Carver c; u32* cells; U16Meta* meta;
    U16DecWs(void* ws, size_t chunk) : c(ws), cells(c.take<u32>(chunk * ((size_t)4 << FSEHIP_FSEU16_MAX_TABLELOG))), meta(c.last<U16Meta>(chunk * sizeof(U16Meta))) {}
    size_t end() const { return c.used(); }
};
extern "C" size_t FSEHIP_FSE_compressU16_batch_workspaceSize(size_t nBlocks) { return ws_size(nBlocks, U16CompWs::bytes_per_block); }
extern "C" size_t FSEHIP_FSE_decompressU16_batch_workspaceSize(size_t nBlocks) { return ws_size(nBlocks, U16DecWs::bytes_per_block); }

extern "C" int FSEHIP_FSE_countU16_batch(unsigned* d_counts, unsigned* d_maxSymbolValues, size_t* d_results, const unsigned short* d_src, size_t srcStrideBytes,
                                         const size_t* d_srcSizes, size_t uniformSrcSize, unsigned maxSymbolValue, size_t nBlocks, void* stream)
{
    if (nBlocks == 0) return 0;
    U16CArgs a;
    a.src = d_src; a.srcStrideBytes = srcStrideBytes; a.srcSizes = d_srcSizes; a.uniformSrcSize = uniformSrcSize;
    a.dst = nullptr; a.dstStride = 0; a.dstCapacity = 0; a.maxSVReq = maxSymbolValue; a.tableLogReq = 0;
    a.stateTables = nullptr; a.symTT = nullptr; a.meta = nullptr; a.countsOut = d_counts; a.maxSVOut = d_maxSymbolValues;
    a.results = d_results; a.nBlocks = nBlocks;
    return (int)launch_u16_compress(a, (hipStream_t)stream);
}

extern "C" int FSEHIP_FSE_compressU16_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results, const unsigned short* d_src, size_t srcStrideBytes,
                                            const size_t* d_srcSizes, size_t uniformSrcSize, unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks,
                                            void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;          // include/fsehip.h: workspaces are 256-byte aligned; checked before anything else
    if (nBlocks == 0) return 0;
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, U16CompWs::bytes_per_block);
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const U16CompWs ws(d_workspace, chunk);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        U16CArgs a;
        a.src = (const u16*)((const u8*)d_src + b0 * srcStrideBytes); a.srcStrideBytes = srcStrideBytes;
        a.srcSizes = d_srcSizes ? d_srcSizes + b0 : nullptr; a.uniformSrcSize = uniformSrcSize;
        a.dst = (u8*)d_dst + b0 * dstStride; a.dstStride = dstStride; a.dstCapacity = dstCapacity;
        a.maxSVReq = maxSymbolValue; a.tableLogReq = tableLog;
        a.stateTables = ws.stateTables; a.symTT = ws.symTT; a.meta = ws.meta; a.countsOut = nullptr; a.maxSVOut = nullptr;
        a.results = d_results + b0; a.nBlocks = nb;
        CK(launch_u16_compress(a, s));
    }
    return 0;
}

extern "C" int FSEHIP_FSE_decompressU16_batch(unsigned short* d_dst, size_t dstStrideBytes, size_t dstCapacity, size_t* d_results, const void* d_cSrc, size_t cStride,
                                              const size_t* d_cSizes, size_t uniformCSize, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;          // include/fsehip.h: workspaces are 256-byte aligned; checked before anything else
    if (nBlocks == 0) return 0;
    const size_t chunk = ws_chunk(workspaceBytes, nBlocks, U16DecWs::bytes_per_block);
    if (chunk == 0) return (int)hipErrorInvalidValue;
    const U16DecWs ws(d_workspace, chunk);
    if (ws.end() > workspaceBytes) return (int)hipErrorInvalidValue;
    for (size_t b0 = 0; b0 < nBlocks; b0 += chunk) {
        const size_t nb = pass_blocks(nBlocks, b0, chunk);
        U16DArgs a;
        a.dst = (u16*)((u8*)d_dst + b0 * dstStrideBytes); a.dstStrideBytes = dstStrideBytes; a.dstCapacity = dstCapacity;
        a.csrc = (const u8*)d_cSrc + b0 * cStride; a.cStride = cStride; a.cSizes = d_cSizes ? d_cSizes + b0 : nullptr; a.uniformCSize = uniformCSize;
        a.cells = ws.cells; a.meta = ws.meta; a.results = d_results + b0; a.nBlocks = nb;
        CK(launch_u16_decompress(a, s));
    }
    return 0;
}

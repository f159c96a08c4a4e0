// capi_host.hip -- the calls of the C ABI (include/fsehip.h) on HOST pointers, the drop-in surface (libfse_dropin.so binds the reference's
// names to them): every call is a batch of one -- scratch from the calling thread's arena, upload, the batch call of capi_batch.hip,
// the 8-byte result, copy out.  No CPU compute path exists: without a usable device the calls fail.
#include "internal.h"
#include <string.h>
#include <vector>

// =====================================================================================================
//  Layer 1: single-block calls on host pointers = batch of one (H2D, kernels, D2H)
// =====================================================================================================
namespace {
// hipFree takes a pointer of any device, so an arena is given back wherever it was allocated: when the thread moves to another device,
// when it grows, on FSEHIP_releaseScratch and when the thread ends (thread_local destructors run at thread exit and, for the main
// thread, before the destructors of static objects -- the runtime is still there; an error from a runtime already shut down is ignored).
struct Arena { void* base = nullptr; size_t cap = 0, used = 0, live = 0, peak = 0; int dev = -1;
               void drop() { if (base) { (void)hipFree(base); (void)hipGetLastError(); } base = nullptr; cap = 0; used = 0; dev = -1; }
               ~Arena() { if (live == 0) drop(); } };
thread_local Arena t_arena;
}
hipError_t HostCallBuf::alloc(size_t n)
{
    Arena& A = t_arena;
    const size_t need = align_up(n ? n : 1, 256);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (A.live == 0) {                                            // between calls: follow the current device, grow to the last call's peak
        size_t want = A.peak > need ? A.peak : need;
        if (want > FSEHIP_SCRATCH_MAX) want = FSEHIP_SCRATCH_MAX;
        if (A.dev != dev || A.cap < want) {
            A.drop();                                             // (also an arena left on the device the thread used before)
            A.dev = dev;
            if (want < ((size_t)1 << 20)) want = (size_t)1 << 20;
            if (hipMalloc(&A.base, want) == hipSuccess) A.cap = want; else { A.base = nullptr; (void)hipGetLastError(); }
        }
        A.used = 0; A.peak = 0;
    }
    ++A.live;
    A.peak += need;
    if (A.base && A.dev == dev && A.used + need <= A.cap) { p = (u8*)A.base + A.used; A.used += need; carved = need; owned = false; return hipSuccess; }
    owned = true; carved = 0;
    e = hipMalloc(&p, need);
    if (e != hipSuccess) { p = nullptr; --A.live; }
    return e;
}
HostCallBuf::~HostCallBuf()
{
    if (!p) return;
    Arena& A = t_arena;
    if (owned) (void)hipFree(p); else A.used -= carved;           // (stack order: destructors run in reverse order of the allocations)
    --A.live;
}
// gives the calling thread's scratch arena back (between calls); the next call on host pointers allocates a new one
int release_thread_scratch(void)                                  // the calling thread's arena
{
    Arena& A = t_arena;
    if (A.live) return (int)hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (A.base) e = hipFree(A.base);                              // whatever device the thread is on now
    A.base = nullptr; A.cap = 0; A.used = 0; A.peak = 0; A.dev = -1;
    return (int)e;
}
extern "C" int FSEHIP_releaseScratch(void)
{
    const int r = release_thread_scratch();
    const int rp = frame_pool_release_scratch();                  // ... and those of the frame calls' idle helper threads (frame.hip)
    return r ? r : rp;
}
extern "C" int FSEHIP_shutdown(void)
{
    const int r = release_thread_scratch();
    const int rp = frame_pool_shutdown();
    return r ? r : rp;
}

// One call on host pointers.  Scratch comes from the arena in the order it is asked for and goes back in reverse when the call ends.  The
// first failure of the device path latches: every later step is skipped and the call returns GENERIC (ret).  What differs between the
// calls, and is their contract, stays at the call site: which inputs are zero-padded, when the output is fetched and how much of it.
struct HostCall {
    bool ok = true;
    void* alloc(size_t bytes)
    {
        if (!ok) return nullptr;
        if (n == MAXBUF || buf[n].alloc(bytes) != hipSuccess) { ok = false; return nullptr; }
        return buf[n++].p;
    }
    void copy_in(void* d, const void* src, size_t bytes) { if (ok) ok = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) == hipSuccess; }
    void* upload(const void* src, size_t bytes) { void* const d = alloc(bytes); copy_in(d, src, bytes); return d; }
    void* upload_padded(const void* src, size_t bytes, size_t cap)      // `cap` bytes of zeros, src over their head
    {
        void* const d = alloc(cap);
        if (ok) ok = hipMemset(d, 0, cap) == hipSuccess;
        copy_in(d, src, bytes);
        return d;
    }
    template <class T> void* upload_scalar(const T& v) { return upload(&v, sizeof(T)); }
    size_t* alloc_result() { return (size_t*)alloc(8); }
    void fetch(void* dst, const void* d, size_t bytes) { if (ok) ok = hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
    size_t result(const size_t* dres) { size_t r = 0; fetch(&r, dres, 8); return ret(r); }
    size_t ret(size_t r) const { return ok ? r : FSEHIP_ERROR(GENERIC); }
private:
    enum { MAXBUF = 8 };
    HostCallBuf buf[MAXBUF];          // (destroyed in reverse order: the arena is a stack)
    int n = 0;
};
// the device work of a call: skipped once a step has failed (its arguments may be null then), a failure latches like any other
#define RUN(h, call) do { if ((h).ok && (call) != 0) (h).ok = false; } while (0)

static size_t hist_count_host(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize, int trustInput)
{
    HostCall h;
    void* const dsrc = h.upload(src, srcSize); unsigned* const dcnt = (unsigned*)h.alloc(1024); unsigned* const dmsv = (unsigned*)h.upload(maxSymbolValuePtr, 4);
    size_t* const dres = h.alloc_result();
    if (srcSize >= HIST_LARGE_MIN) {                        // a whole buffer: pieces counted as a batch and folded (hist.hip)
        const size_t nPart = (srcSize + HIST_PIECE - 1) / HIST_PIECE;
        unsigned* const dpart = (unsigned*)h.alloc(nPart * 1024); size_t* const dpr = (size_t*)h.alloc(nPart * 8);
        RUN(h, launch_hist_large((const u8*)dsrc, srcSize, *maxSymbolValuePtr, trustInput, dpart, dcnt, dmsv, dres, dpr, nullptr));
        RUN(h, hipDeviceSynchronize());
    } else {
        HistArgs a;
        a.counts = dcnt; a.maxSVs = dmsv; a.uniformMaxSV = 255; a.useUniformIn = 0; a.trustInput = trustInput;
        a.results = dres; a.src = mkview(dsrc, srcSize, nullptr, srcSize); a.nBlocks = 1;
        RUN(h, launch_hist(a, nullptr));
    }
    const size_t r = h.result(dres);
    if (FSEHIP_isError(r)) return r;
    const unsigned in = *maxSymbolValuePtr;
    h.fetch(count, dcnt, (in < 255 ? in + 1 : 256) * 4);
    h.fetch(maxSymbolValuePtr, dmsv, 4);
    return h.ret(r);
}
// HIST_count_wksp's view of its workspace (lib/hist.c:163-173): validated exactly as the reference validates it and then left alone -- the
// counting happens in the kernel's LDS
static size_t hist_wksp_error(const void* workSpace, size_t workSpaceSize)
{
    if ((size_t)workSpace & 3) return FSEHIP_ERROR(GENERIC);
    return workSpaceSize < FSEHIP_HIST_WKSP_SIZE ? FSEHIP_ERROR(workSpace_tooSmall) : 0;
}
// lib/hist.h:46-74.  HIST_countFast (lib/hist.c:141-159) is the unchecked variant: a limit below 255 bounds the entries written to count[] but a
// larger symbol in src is not an error -- the result and *maxSymbolValuePtr are taken over all 256 symbols (HIST_count_parallel_wksp with
// trustInput, :120-131).  Below 1500 bytes the reference runs HIST_count_simple (:29-54), which never looks at the workspace and writes beyond
// count[] for such input; the defined behaviour is kept at every size.  HIST_count_simple returns the largest count as `unsigned`: a device
// failure reads as 0 (the function has no error channel).
extern "C" size_t FSEHIP_HIST_count(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize) { return hist_count_host(count, maxSymbolValuePtr, src, srcSize, 0); }
extern "C" size_t FSEHIP_HIST_countFast(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize) { return hist_count_host(count, maxSymbolValuePtr, src, srcSize, 1); }
extern "C" size_t FSEHIP_HIST_count_wksp(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize, void* workSpace, size_t workSpaceSize)
{
    const size_t e = hist_wksp_error(workSpace, workSpaceSize);
    return e ? e : hist_count_host(count, maxSymbolValuePtr, src, srcSize, 0);
}
extern "C" size_t FSEHIP_HIST_countFast_wksp(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize, void* workSpace, size_t workSpaceSize)
{
    const size_t e = srcSize >= 1500 ? hist_wksp_error(workSpace, workSpaceSize) : 0;
    return e ? e : hist_count_host(count, maxSymbolValuePtr, src, srcSize, 1);
}
extern "C" unsigned FSEHIP_HIST_count_simple(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize)
{
    const size_t r = hist_count_host(count, maxSymbolValuePtr, src, srcSize, 1);
    return FSEHIP_isError(r) ? 0u : (unsigned)r;
}

extern "C" size_t FSEHIP_FSE_compress_usingCTable(void* dst, size_t dstCapacity, const void* src, size_t srcSize, const FSEHIP_FSE_CTable* ct)
{
    const u16* hd = (const u16*)ct;
    const unsigned tl = hd[0], msv = hd[1];
    if (tl > FSEHIP_FSE_MAX_TABLELOG) return FSEHIP_ERROR(tableLog_tooLarge);
    const size_t words = 1 + (tl ? ((size_t)1 << (tl - 1)) : 1) + 2 * ((size_t)(msv > 255 ? 255 : msv) + 1);   // byte symbols: larger entries are unreachable
    HostCall h;
    void* const dsrc = h.upload(src, srcSize); void* const ddst = h.alloc(dstCapacity); void* const dct = h.upload(ct, words * 4); size_t* const dres = h.alloc_result();
    RUN(h, FSEHIP_FSE_compress_usingCTable_batch(ddst, dstCapacity, dstCapacity, dres, dsrc, srcSize, nullptr, srcSize, (const unsigned*)dct, 0, FSEHIP_FSE_MAX_TABLELOG, 1, nullptr));
    const size_t r = h.result(dres);
    if (!FSEHIP_isError(r) && r > 0) h.fetch(dst, ddst, r);
    return h.ret(r);
}

extern "C" size_t FSEHIP_FSE_decompress_usingDTable(void* dst, size_t dstCapacity, const void* cSrc, size_t cSrcSize, const FSEHIP_FSE_DTable* dt)
{
    const unsigned tl = ((const u16*)dt)[0];
    if (tl > FSEHIP_FSE_MAX_TABLELOG) return FSEHIP_ERROR(tableLog_tooLarge);
    const size_t words = 1 + ((size_t)1 << tl);
    HostCall h;
    void* const dsrc = h.upload(cSrc, cSrcSize); void* const ddst = h.alloc(dstCapacity); void* const ddt = h.upload(dt, words * 4); size_t* const dres = h.alloc_result();
    RUN(h, FSEHIP_FSE_decompress_usingDTable_batch(ddst, dstCapacity, dstCapacity, dres, dsrc, cSrcSize, nullptr, cSrcSize,
                                                   (const unsigned*)ddt, 0, tl ? tl : 1, 1, nullptr));   // (the table's own log: one launch, its class)
    const size_t r = h.result(dres);
    if (!FSEHIP_isError(r) && r > 0) h.fetch(dst, ddst, r <= dstCapacity ? r : dstCapacity);
    return h.ret(r);
}

extern "C" size_t FSEHIP_FSE_compress2(void* dst, size_t dstCapacity, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog)
{
    if (tableLog > FSEHIP_FSE_MAX_TABLELOG) return FSEHIP_ERROR(tableLog_tooLarge);   // fse_compress.c:691
    const size_t wsBytes = FSEHIP_FSE_compress_batch_workspaceSize(1, tableLog);
    HostCall h;
    void* const dsrc = h.upload(src, srcSize); void* const ddst = h.alloc(dstCapacity); void* const dws = h.alloc(wsBytes); size_t* const dres = h.alloc_result();
    RUN(h, FSEHIP_FSE_compress_batch(ddst, dstCapacity, dstCapacity, dres, dsrc, srcSize, nullptr, srcSize, maxSymbolValue, tableLog, 1, dws, wsBytes, nullptr));
    const size_t r = h.result(dres);
    if (!FSEHIP_isError(r) && r > 1) h.fetch(dst, ddst, r);      // (0: not compressible, 1: one symbol -- dst is not written, fse_compress.c:652-664)
    return h.ret(r);
}

extern "C" size_t FSEHIP_FSE_compress(void* dst, size_t dstCapacity, const void* src, size_t srcSize)   // fse_compress.c:695-698
{
    return FSEHIP_FSE_compress2(dst, dstCapacity, src, srcSize, 255, FSEHIP_FSE_DEFAULT_TABLELOG);
}

// lib/fse.h:315 (lib/fse_compress.c:632-677).  The workspace is checked as the reference checks it -- its size in BYTES against
// FSE_WKSP_SIZE_U32(tableLog, maxSymbolValue), the comparison of :646 as written, on the arguments as passed (before 0 -> 255 / default) --
// and then left alone: tables and counters live in device memory.  A table log above FSE_MAX_TABLELOG is not refused here (FSE_compress2
// refuses it, :691): FSE_optimalTableLog clamps it to 12 (:340), so it codes like 12.
extern "C" size_t FSEHIP_FSE_compress_wksp(void* dst, size_t dstSize, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog,
                                           void* workSpace, size_t wkspSize)
{
    (void)workSpace;
    // 1 << (tableLog - 1) with tableLog 0 is undefined in the reference's macro (x86: 1 << 31); such a call cannot pass the check
    if (tableLog == 0 || tableLog > 31) return FSEHIP_ERROR(tableLog_tooLarge);
    const unsigned long long need = 1ull + (1ull << (tableLog - 1)) + 2ull * ((unsigned long long)maxSymbolValue + 1) + (tableLog > 12 ? (1ull << (tableLog - 2)) : 1024ull);
    if (wkspSize < need) return FSEHIP_ERROR(tableLog_tooLarge);
    return FSEHIP_FSE_compress2(dst, dstSize, src, srcSize, maxSymbolValue, tableLog > FSEHIP_FSE_MAX_TABLELOG ? FSEHIP_FSE_MAX_TABLELOG : tableLog);
}

// lib/fse.h:335 (lib/fse_decompress.c:255-274): FSE_decompress with the caller's table-log limit.  The reference builds its DTable in
// `workSpace` (FSE_DTABLE_SIZE_U32(maxLog) words); when one is given it receives the same table here (built on the device in the reference's
// layout), so a caller that looks at it afterwards finds what it expects.  Limits above FSE_MAX_TABLELOG count as 12, the library's
// build-time limit (a stream with a larger table log: tableLog_tooLarge).
extern "C" size_t FSEHIP_FSE_decompress_wksp(void* dst, size_t dstCapacity, const void* cSrc, size_t cSrcSize, FSEHIP_FSE_DTable* workSpace, unsigned maxLog)
{
    const unsigned ml = maxLog > FSEHIP_FSE_MAX_TABLELOG ? FSEHIP_FSE_MAX_TABLELOG : maxLog;
    HostCall h;
    void* const dsrc = h.upload(cSrc, cSrcSize);
    if (ml == 0) {      // no table log fits: FSE_readNCount's own errors first, then tableLog_tooLarge (every valid header has tableLog >= 5)
        const size_t wsB = FSEHIP_FSE_buildDTable_batch_workspaceSize(1, FSEHIP_FSE_MAX_TABLELOG);
        void* const ddt = h.alloc(4 * (size_t)FSEHIP_FSE_DTABLE_SIZE_U32(FSEHIP_FSE_MAX_TABLELOG)); void* const dws = h.alloc(wsB); size_t* const dres = h.alloc_result();
        RUN(h, FSEHIP_FSE_buildDTable_batch((unsigned*)ddt, FSEHIP_FSE_DTABLE_SIZE_U32(FSEHIP_FSE_MAX_TABLELOG), dres, dsrc, cSrcSize, nullptr, cSrcSize,
                                            FSEHIP_FSE_MAX_TABLELOG, 1, dws, wsB, nullptr));
        const size_t r = h.result(dres);
        return FSEHIP_isError(r) ? r : FSEHIP_ERROR(tableLog_tooLarge);
    }
    const size_t wsBytes = FSEHIP_FSE_decompress_batch_workspaceSize(1, ml);
    void* const ddst = h.alloc(dstCapacity); void* const dws = h.alloc(wsBytes); size_t* const dres = h.alloc_result();
    RUN(h, FSEHIP_FSE_decompress_batch(ddst, dstCapacity, dstCapacity, dres, dsrc, cSrcSize, nullptr, cSrcSize, ml, 1, dws, wsBytes, nullptr));
    const size_t r = h.result(dres);
    if (!FSEHIP_isError(r) && r > 0) h.fetch(dst, ddst, r <= dstCapacity ? r : dstCapacity);
    if (workSpace) {    // the table the reference leaves in the workspace (whenever the header parsed and its table log fits)
        const size_t wsB = FSEHIP_FSE_buildDTable_batch_workspaceSize(1, ml);
        const size_t dtU32 = FSEHIP_FSE_DTABLE_SIZE_U32(ml);
        void* const ddt = h.alloc(4 * dtU32); void* const dws2 = h.alloc(wsB); size_t* const dres2 = h.alloc_result();
        RUN(h, FSEHIP_FSE_buildDTable_batch((unsigned*)ddt, dtU32, dres2, dsrc, cSrcSize, nullptr, cSrcSize, ml, 1, dws2, wsB, nullptr));
        if (!FSEHIP_isError(h.result(dres2))) {
            u32 h0 = 0;
            h.fetch(&h0, ddt, 4);
            const unsigned tl = h0 & 0xFFFFu;
            if (tl <= ml) h.fetch(workSpace, ddt, 4 * ((size_t)1 + ((size_t)1 << tl)));
        }
    }
    return h.ret(r);
}
extern "C" size_t FSEHIP_FSE_decompress(void* dst, size_t dstCapacity, const void* cSrc, size_t cSrcSize)   // fse_decompress.c:279-283
{
    return FSEHIP_FSE_decompress_wksp(dst, dstCapacity, cSrc, cSrcSize, nullptr, FSEHIP_FSE_MAX_TABLELOG);
}

// ---- the table glue on host pointers, reference signatures (lib/fse.h:111-163, :222-241): what a caller of the "advanced" flow -- count, normalise,
//      write the header, build the table, code with it -- finds under the reference's names in libfse_dropin.so.  FSE_optimalTableLog and
//      FSE_NCountWriteBound are arithmetic on the arguments (lib/fse_compress.c:186-190, :325-347); the others are batches of one.
extern "C" unsigned FSEHIP_FSE_optimalTableLog(unsigned maxTableLog, size_t srcSize, unsigned maxSymbolValue)
{
    // lib/bitstream.h:139.  srcSize > 1 and maxSymbolValue >= 1 are the reference's preconditions (highbit of 0 is undefined there); here the
    // highest bit of 0 counts as bit 0, so the call returns for every argument
    auto hb = [](u32 v) { return v ? 31u - (u32)__builtin_clz(v) : 0u; };
    const u32 maxBitsSrc = hb((u32)(srcSize - 1)) - 2;
    const u32 minBitsSrc = hb((u32)srcSize) + 1, minBitsSymbols = hb(maxSymbolValue) + 2;
    const u32 minBits = minBitsSrc < minBitsSymbols ? minBitsSrc : minBitsSymbols;
    u32 tl = maxTableLog ? maxTableLog : FSEHIP_FSE_DEFAULT_TABLELOG;
    if (maxBitsSrc < tl) tl = maxBitsSrc;
    if (minBits > tl) tl = minBits;
    if (tl < FSEHIP_FSE_MIN_TABLELOG) tl = FSEHIP_FSE_MIN_TABLELOG;
    if (tl > FSEHIP_FSE_MAX_TABLELOG) tl = FSEHIP_FSE_MAX_TABLELOG;
    return tl;
}
extern "C" size_t FSEHIP_FSE_NCountWriteBound(unsigned maxSymbolValue, unsigned tableLog)
{
    return maxSymbolValue ? (size_t)((((maxSymbolValue + 1) * tableLog) >> 3) + 3) : (size_t)FSEHIP_FSE_NCOUNTBOUND;
}
extern "C" size_t FSEHIP_FSE_normalizeCount(short* normalizedCounter, unsigned tableLog, const unsigned* count, size_t total, unsigned maxSymbolValue)
{
    if (maxSymbolValue > 255) return FSEHIP_ERROR(maxSymbolValue_tooLarge);      // (byte alphabets; the reference would index beyond its FSE_MAX_SYMBOL_VALUE-sized users' arrays)
    HostCall h;
    void* const dn = h.alloc(512); void* const dc = h.alloc(1024);
    h.copy_in(dc, count, 4 * ((size_t)maxSymbolValue + 1));                       // (not padded: entries above maxSymbolValue are not read)
    void* const dt = h.upload_scalar(total); void* const dm = h.upload_scalar(maxSymbolValue); size_t* const dr = h.alloc_result();
    RUN(h, FSEHIP_FSE_normalizeCount_batch((short*)dn, 256, tableLog, (const unsigned*)dc, 256, (const size_t*)dt, (const unsigned*)dm, 1, dr, nullptr));
    const size_t r = h.result(dr);
    if (!FSEHIP_isError(r)) h.fetch(normalizedCounter, dn, 2 * ((size_t)maxSymbolValue + 1));
    return h.ret(r);
}
extern "C" size_t FSEHIP_FSE_writeNCount(void* buffer, size_t bufferSize, const short* normalizedCounter, unsigned maxSymbolValue, unsigned tableLog)
{
    if (tableLog > FSEHIP_FSE_MAX_TABLELOG) return FSEHIP_ERROR(tableLog_tooLarge);   // lib/fse_compress.c:281-282
    if (tableLog < FSEHIP_FSE_MIN_TABLELOG || maxSymbolValue > 255) return FSEHIP_ERROR(GENERIC);
    const size_t cap = bufferSize < 512 ? bufferSize : 512;                      // (no header is longer than FSE_NCOUNTBOUND = 512 bytes)
    HostCall h;
    void* const dh = h.alloc(512); void* const dn = h.upload_padded(normalizedCounter, 2 * ((size_t)maxSymbolValue + 1), 512);
    void* const dm = h.upload_scalar(maxSymbolValue); size_t* const dr = h.alloc_result();
    RUN(h, FSEHIP_FSE_writeNCount_batch(dh, 512, cap, (const short*)dn, 256, (const unsigned*)dm, tableLog, 1, dr, nullptr));
    const size_t r = h.result(dr);
    if (!FSEHIP_isError(r) && r > 0) h.fetch(buffer, dh, r);
    return h.ret(r);
}
extern "C" size_t FSEHIP_FSE_readNCount(short* normalizedCounter, unsigned* maxSVPtr, unsigned* tableLogPtr, const void* rBuffer, size_t rBuffSize)
{
    const unsigned limit = *maxSVPtr;
    if (limit > 255) return FSEHIP_ERROR(maxSymbolValue_tooLarge);
    const size_t n = rBuffSize < 1024 ? rBuffSize : 1024;                          // (a header describes at most 256 symbols: it ends long before)
    HostCall h;
    void* const dh = n ? h.upload(rBuffer, n) : h.alloc(1); void* const dn = h.alloc(512); void* const dm = h.upload_scalar(limit); void* const dl = h.alloc(4);
    size_t* const dr = h.alloc_result();
    RUN(h, FSEHIP_FSE_readNCount_batch((short*)dn, 256, (unsigned*)dm, (unsigned*)dl, dh, n, nullptr, n, 1, dr, nullptr));
    const size_t r = h.result(dr);
    if (FSEHIP_isError(r)) return r;
    h.fetch(normalizedCounter, dn, 2 * ((size_t)limit + 1));   // (the reference clears [0, limit] first: lib/entropy_common.c:68)
    h.fetch(maxSVPtr, dm, 4);
    h.fetch(tableLogPtr, dl, 4);
    return h.ret(r);
}
extern "C" size_t FSEHIP_FSE_buildCTable(FSEHIP_FSE_CTable* ct, const short* normalizedCounter, unsigned maxSymbolValue, unsigned tableLog)
{
    if (maxSymbolValue > 255) return FSEHIP_ERROR(maxSymbolValue_tooLarge);
    if (tableLog > FSEHIP_FSE_MAX_TABLELOG) return FSEHIP_ERROR(tableLog_tooLarge);   // lib/fse_compress.c:86 with the 4096-byte workspace of :172-176
    if (tableLog == 0 || tableLog == 1 || tableLog == 3) return FSEHIP_ERROR(GENERIC);   // (no table, or an even FSE_TABLESTEP: fsehip.h)
    const size_t words = FSEHIP_FSE_CTABLE_SIZE_U32(tableLog, 255);
    HostCall h;
    void* const dn = h.upload_padded(normalizedCounter, 2 * ((size_t)maxSymbolValue + 1), 512); void* const dm = h.upload_scalar(maxSymbolValue);
    void* const dct = h.alloc(4 * words); size_t* const dr = h.alloc_result();
    RUN(h, FSEHIP_FSE_buildCTable_fromNorm_batch((unsigned*)dct, words, (const short*)dn, 256, (const unsigned*)dm, tableLog, 1, dr, nullptr));
    const size_t r = h.result(dr);
    if (!FSEHIP_isError(r)) h.fetch(ct, dct, 4 * (size_t)FSEHIP_FSE_CTABLE_SIZE_U32(tableLog, maxSymbolValue));
    return h.ret(r);
}
// lib/fse.h:341 (lib/fse_compress.c:70-87): the workspace is checked as the reference checks it and then left alone
extern "C" size_t FSEHIP_FSE_buildCTable_wksp(FSEHIP_FSE_CTable* ct, const short* normalizedCounter, unsigned maxSymbolValue, unsigned tableLog, void* workSpace, size_t wkspSize)
{
    (void)workSpace;
    if (tableLog > 31 || ((size_t)1 << tableLog) > wkspSize) return FSEHIP_ERROR(tableLog_tooLarge);
    return FSEHIP_FSE_buildCTable(ct, normalizedCounter, maxSymbolValue, tableLog);
}
extern "C" size_t FSEHIP_FSE_buildDTable(FSEHIP_FSE_DTable* dt, const short* normalizedCounter, unsigned maxSymbolValue, unsigned tableLog)
{
    if (maxSymbolValue > 255) return FSEHIP_ERROR(maxSymbolValue_tooLarge);       // lib/fse_decompress.c:83-84
    if (tableLog > FSEHIP_FSE_MAX_TABLELOG) return FSEHIP_ERROR(tableLog_tooLarge);
    if (tableLog == 0 || tableLog == 1 || tableLog == 3) return FSEHIP_ERROR(GENERIC);   // (no table, or an even FSE_TABLESTEP: fsehip.h)
    const size_t words = FSEHIP_FSE_DTABLE_SIZE_U32(tableLog);
    const size_t wsB = FSEHIP_FSE_buildDTable_fromNorm_batch_workspaceSize(1, tableLog);
    HostCall h;
    void* const dn = h.upload_padded(normalizedCounter, 2 * ((size_t)maxSymbolValue + 1), 512); void* const dm = h.upload_scalar(maxSymbolValue);
    void* const ddt = h.alloc(4 * words); void* const dws = h.alloc(wsB); size_t* const dr = h.alloc_result();
    RUN(h, FSEHIP_FSE_buildDTable_fromNorm_batch((unsigned*)ddt, words, (const short*)dn, 256, (const unsigned*)dm, tableLog, 1, dr, dws, wsB, nullptr));
    const size_t r = h.result(dr);
    if (!FSEHIP_isError(r)) h.fetch(dt, ddt, 4 * words);
    return h.ret(r);
}

// ---- Layer 1, Huff0 ---------------------------------------------------------------------------------
static size_t huf_using_ctable_host(int streams, void* dst, size_t dstSize, const void* src, size_t srcSize, const FSEHIP_HUF_CElt* CTable)
{
    // the opaque HUF_CElt table holds maxSymbolValue+1 entries; only entries of symbols present in src are read
    unsigned maxByte = 0;
    for (size_t i = 0; i < srcSize; i++) { const unsigned v = ((const u8*)src)[i]; if (v > maxByte) maxByte = v; }
    u32 table[256];
    memset(table, 0, sizeof(table));
    memcpy(table, CTable, ((size_t)maxByte + 1) * 4);
    HostCall h;
    void* const dsrc = h.upload(src, srcSize); void* const ddst = h.alloc(dstSize); void* const dct = h.upload(table, 1024); size_t* const dres = h.alloc_result();
    HufEncArgs a;
    a.dst = (u8*)ddst; a.dstStride = dstSize; a.dstCapacity = dstSize; a.results = dres;
    a.src = mkview(dsrc, srcSize, nullptr, srcSize);
    a.ctables = (const u32*)dct; a.ctStrideU32 = 0; a.meta = nullptr; a.streams = streams; a.split1X = 0; a.nBlocks = 1;
    RUN(h, launch_huf_encode(a, nullptr));
    const size_t r = h.result(dres);
    if (!FSEHIP_isError(r) && r > 0) h.fetch(dst, ddst, r);
    return h.ret(r);
}
extern "C" size_t FSEHIP_HUF_compress1X_usingCTable(void* dst, size_t dstSize, const void* src, size_t srcSize, const FSEHIP_HUF_CElt* CTable) { return huf_using_ctable_host(1, dst, dstSize, src, srcSize, CTable); }
extern "C" size_t FSEHIP_HUF_compress4X_usingCTable(void* dst, size_t dstSize, const void* src, size_t srcSize, const FSEHIP_HUF_CElt* CTable) { return huf_using_ctable_host(4, dst, dstSize, src, srcSize, CTable); }

// The *_usingDTable batch call that decodes what a name of the 4X1 / 1X1 / 4X / 1X families decodes: `streams` streams per block, single-symbol tables alone or
// (acceptX2) the dispatch on the table's type of lib/huf_decompress.c:980-997 -- single-symbol (X1) cells -> k_huf_decode, double-symbol (X2) cells -> k_huf_decode_x2
typedef int (*HufDTableBatchFn)(void*, size_t, const size_t*, size_t, size_t*, const void*, size_t, const size_t*, size_t, const FSEHIP_HUF_DTable*, size_t, unsigned, size_t, void*);
static HufDTableBatchFn huf_dtable_batch_fn(int streams, bool acceptX2)
{
    return streams == 1 ? (acceptX2 ? FSEHIP_HUF_decompress1X_usingDTable_batch : FSEHIP_HUF_decompress1X1_usingDTable_batch)
                        : (acceptX2 ? FSEHIP_HUF_decompress4X_usingDTable_batch : FSEHIP_HUF_decompress4X1_usingDTable_batch);
}
// one block at d_src decoded into ddst with the table at ddt (all in device memory), then the common end of every Huff0 decoder call on host pointers
static size_t huf_decode_host(HostCall& h, int streams, bool acceptX2, void* dst, size_t dstSize, void* ddst, size_t* dres, const void* d_src, size_t cSrcSize, const void* ddt)
{
    RUN(h, huf_dtable_batch_fn(streams, acceptX2)(ddst, dstSize, nullptr, dstSize, dres, d_src, cSrcSize, nullptr, cSrcSize, (const u32*)ddt, 0, FSEHIP_HUF_TABLELOG_MAX, 1, nullptr));
    const size_t r = h.result(dres);
    if (!FSEHIP_isError(r) && r > 0) h.fetch(dst, ddst, r <= dstSize ? r : dstSize);
    return h.ret(r);
}
static size_t huf_using_dtable_host(int streams, bool acceptX2, void* dst, size_t maxDstSize, const void* cSrc, size_t cSrcSize, const FSEHIP_HUF_DTable* DTable)
{
    const u32 desc = DTable[0];
    const unsigned type = (desc >> 8) & 0xFF;
    if (type != 0 && !(acceptX2 && type == 1)) return FSEHIP_ERROR(GENERIC);   // huf_decompress.c:411-412
    const unsigned tl = (desc >> 16) & 0xFF;
    if (tl > FSEHIP_HUF_TABLELOG_MAX) return FSEHIP_ERROR(tableLog_tooLarge);
    // single-symbol cells are 2 bytes, double-symbol cells 4 (lib/huf_decompress.c:116, :480)
    const size_t words = 1 + (type ? ((size_t)1 << tl) : (tl ? ((size_t)1 << (tl - 1)) : 1));
    HostCall h;
    void* const dsrc = h.upload(cSrc, cSrcSize); void* const ddst = h.alloc(maxDstSize); void* const ddt = h.upload(DTable, words * 4); size_t* const dres = h.alloc_result();
    return huf_decode_host(h, streams, acceptX2, dst, maxDstSize, ddst, dres, dsrc, cSrcSize, ddt);
}
// the strict double-symbol names (lib/huf_decompress.c:873, :913): any other table is GENERIC
static bool huf_is_x2(const FSEHIP_HUF_DTable* DTable) { return ((DTable[0] >> 8) & 0xFFu) == 1u; }
#define HUF_USING_DTABLE_ARGS void* dst, size_t maxDstSize, const void* cSrc, size_t cSrcSize, const FSEHIP_HUF_DTable* DTable
extern "C" size_t FSEHIP_HUF_decompress4X1_usingDTable(HUF_USING_DTABLE_ARGS) { return huf_using_dtable_host(4, false, dst, maxDstSize, cSrc, cSrcSize, DTable); }
extern "C" size_t FSEHIP_HUF_decompress4X_usingDTable(HUF_USING_DTABLE_ARGS) { return huf_using_dtable_host(4, true, dst, maxDstSize, cSrc, cSrcSize, DTable); }
extern "C" size_t FSEHIP_HUF_decompress1X1_usingDTable(HUF_USING_DTABLE_ARGS) { return huf_using_dtable_host(1, false, dst, maxDstSize, cSrc, cSrcSize, DTable); }
extern "C" size_t FSEHIP_HUF_decompress1X_usingDTable(HUF_USING_DTABLE_ARGS) { return huf_using_dtable_host(1, true, dst, maxDstSize, cSrc, cSrcSize, DTable); }
extern "C" size_t FSEHIP_HUF_decompress4X2_usingDTable(HUF_USING_DTABLE_ARGS) { return huf_is_x2(DTable) ? huf_using_dtable_host(4, true, dst, maxDstSize, cSrc, cSrcSize, DTable) : FSEHIP_ERROR(GENERIC); }
extern "C" size_t FSEHIP_HUF_decompress1X2_usingDTable(HUF_USING_DTABLE_ARGS) { return huf_is_x2(DTable) ? huf_using_dtable_host(1, true, dst, maxDstSize, cSrc, cSrcSize, DTable) : FSEHIP_ERROR(GENERIC); }

static size_t huf_compress_host(int streams, void* dst, size_t dstCapacity, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog)
{
    // argument checks in the reference's order (huf_compress.c:654-660)
    if (!srcSize) return 0;
    if (!dstCapacity) return 0;
    if (srcSize > FSEHIP_HUF_BLOCKSIZE_MAX) return FSEHIP_ERROR(srcSize_wrong);
    if (tableLog > FSEHIP_HUF_TABLELOG_MAX) return FSEHIP_ERROR(tableLog_tooLarge);
    if (maxSymbolValue > 255) return FSEHIP_ERROR(maxSymbolValue_tooLarge);
    const size_t wsBytes = FSEHIP_HUF_compress_batch_workspaceSize(1);
    HostCall h;
    void* const dsrc = h.upload(src, srcSize); void* const ddst = h.alloc(dstCapacity); void* const dws = h.alloc(wsBytes); size_t* const dres = h.alloc_result();
    RUN(h, huf_compress_batch_impl(streams, ddst, dstCapacity, dstCapacity, dres, dsrc, srcSize, nullptr, srcSize, maxSymbolValue, tableLog, 1, dws, wsBytes, nullptr));
    const size_t r = h.result(dres);
    if (!FSEHIP_isError(r) && r > 0) h.fetch(dst, ddst, r);   // r == 1: the RLE byte sits in dst[0] (:673)
    return h.ret(r);
}
// lib/huf.h:95, :289 (lib/huf_compress.c:727-768 -> HUF_compress_internal :637-724): the workspace is validated as :654-655 validate it
// (alignment first, then size) and then left alone; the 1X form writes one stream without a jump table (HUF_singleStream, :615-617)
static size_t huf_compress_wksp_host(int streams, void* dst, size_t dstCapacity, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog,
                                     void* workSpace, size_t wkspSize)
{
    if (((size_t)workSpace & 3) != 0) return FSEHIP_ERROR(GENERIC);
    if (wkspSize < FSEHIP_HUF_WORKSPACE_SIZE) return FSEHIP_ERROR(workSpace_tooSmall);
    return huf_compress_host(streams, dst, dstCapacity, src, srcSize, maxSymbolValue, tableLog);
}
#define HUF_COMPRESS_ARGS void* dst, size_t dstCapacity, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog
extern "C" size_t FSEHIP_HUF_compress2(HUF_COMPRESS_ARGS) { return huf_compress_host(4, dst, dstCapacity, src, srcSize, maxSymbolValue, tableLog); }
extern "C" size_t FSEHIP_HUF_compress1X(HUF_COMPRESS_ARGS) { return huf_compress_host(1, dst, dstCapacity, src, srcSize, maxSymbolValue, tableLog); }   // lib/huf.h:288 (huf_compress.c:750-756)
extern "C" size_t FSEHIP_HUF_compress4X_wksp(HUF_COMPRESS_ARGS, void* workSpace, size_t wkspSize) { return huf_compress_wksp_host(4, dst, dstCapacity, src, srcSize, maxSymbolValue, tableLog, workSpace, wkspSize); }
extern "C" size_t FSEHIP_HUF_compress1X_wksp(HUF_COMPRESS_ARGS, void* workSpace, size_t wkspSize) { return huf_compress_wksp_host(1, dst, dstCapacity, src, srcSize, maxSymbolValue, tableLog, workSpace, wkspSize); }

// HUF_readDTableX1_wksp (lib/huf_decompress.c:118-185) / HUF_readDTableX2_wksp (:551-649) on a block that is in device memory already: dctx (host) -- whose
// descriptor carries the table-log limit (HUF_CREATE_STATIC_DTABLEX1 / X2) -- receives descriptor and cells as the reference leaves them, *ddt (device) the
// same table for a decoder call behind it.  Returns the header size or an error code.  The reference's workspace is checked as it checks it and left alone.
static const size_t HUF_X1_WKSP_BYTES = 4 * (16 + 64);      // :137
// :570-581: rankVal, rankStats, rankStart0, sortedSymbol, weightList
static const size_t HUF_X2_WKSP_BYTES = 4 * ((FSEHIP_HUF_TABLELOG_MAX + 1) * FSEHIP_HUF_TABLELOG_MAX + (FSEHIP_HUF_TABLELOG_MAX + 1) + (FSEHIP_HUF_TABLELOG_MAX + 2) + 2 * 256 / 4 + 256 / 4);
static size_t huf_read_dtable_host(HostCall& h, bool x2, FSEHIP_HUF_DTable* dctx, const void* d_src, size_t cSrcSize, size_t wkspSize, void** ddtOut)
{
    const u32 desc = dctx[0];
    unsigned mtl = desc & 0xFFu;                                   // DTableDesc.maxTableLog
    if (x2) {
        // double-symbol: the workspace first (:581), then the descriptor's limit (:587); the table has 1 << maxTableLog cells of 4 bytes whatever the header's depth
        if (wkspSize < HUF_X2_WKSP_BYTES) return FSEHIP_ERROR(tableLog_tooLarge);
        if (mtl > FSEHIP_HUF_TABLELOG_MAX) return FSEHIP_ERROR(tableLog_tooLarge);
    } else {
        // single-symbol: tables up to maxTableLog + 1 fit (:149); HUF_readStats refuses table logs above 12 anyway.  The batch call reads 0 as "default":
        // a limit of 0 is enforced below
        if (mtl > FSEHIP_HUF_TABLELOG_MAX - 1) mtl = FSEHIP_HUF_TABLELOG_MAX - 1;
        if (mtl == 0) mtl = 1;
    }
    const size_t dtU32 = 1 + ((size_t)1 << mtl);
    const size_t wsB = FSEHIP_HUF_readDTableX1_batch_workspaceSize(1);               // (the X2 call asks for the same)
    u32* const ddt = (u32*)h.alloc(4 * dtU32); void* const dws = h.alloc(wsB); size_t* const dres = h.alloc_result();
    *ddtOut = ddt;
    RUN(h, (x2 ? FSEHIP_HUF_readDTableX2_batch : FSEHIP_HUF_readDTableX1_batch)(ddt, dtU32, mtl, dres, d_src, cSrcSize, nullptr, cSrcSize, 1, dws, wsB, nullptr));
    const size_t hSize = h.result(dres);
    if (FSEHIP_isError(hSize)) return hSize;
    u32 dNew;
    if (x2) {
        h.fetch(dctx + 1, ddt + 1, (size_t)4 << mtl);
        dNew = (desc & 0xFF0000FFu) | 0x100u | ((u32)mtl << 16);    // {maxTableLog and reserved byte as found, tableType 1, tableLog = maxTableLog} (:645-647)
    } else {
        u32 d0 = 0;
        h.fetch(&d0, ddt, 4);
        if (!h.ok) return h.ret(0);
        const unsigned tl = (d0 >> 16) & 0xFFu;
        if (tl > (desc & 0xFFu) + 1) return FSEHIP_ERROR(tableLog_tooLarge);
        h.fetch(dctx + 1, ddt + 1, tl ? ((size_t)2 << tl) : 2);     // 2-byte cells
        dNew = (desc & 0xFF0000FFu) | (tl << 16);                   // {tableType 0, tableLog}; maxTableLog and the reserved byte stay the caller's (:150-152)
    }
    if (!h.ok) return h.ret(0);
    dctx[0] = dNew;
    h.copy_in(ddt, &dNew, 4);
    return h.ret(hSize);
}
// HUF_decompress{4X1,1X1,4X2,1X2}_DCtx_wksp (lib/huf_decompress.c:377-389, :416-436, :877-890, :917-930): the table from the block's header into dctx, then the
// four streams (or the one stream) behind it.  The double-symbol forms decode through the table-dispatching route -- the lock-step double-symbol decoder, which
// returns what the reference's X2 decoder returns on damaged streams too.  The single-symbol forms check their workspace (:137) before anything else, the
// double-symbol forms inside the table read.
static size_t huf_dctx_host(int streams, bool x2, FSEHIP_HUF_DTable* dctx, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize, size_t wkspSize)
{
    if (!x2 && wkspSize < HUF_X1_WKSP_BYTES) return FSEHIP_ERROR(tableLog_tooLarge);
    HostCall h;
    void* const dsrc = h.upload(cSrc, cSrcSize);                    // (scratch in the order dsrc, ddst, dres, then ddt inside the table read)
    void* const ddst = h.alloc(dstSize); size_t* const dres = h.alloc_result();
    void* ddt = nullptr;
    const size_t hSize = huf_read_dtable_host(h, x2, dctx, dsrc, cSrcSize, wkspSize, &ddt);
    if (FSEHIP_isError(hSize)) return hSize;
    if (hSize >= cSrcSize) return FSEHIP_ERROR(srcSize_wrong);     // :386, :886, :926
    return huf_decode_host(h, streams, x2, dst, dstSize, ddst, dres, (const u8*)dsrc + hSize, cSrcSize - hSize, ddt);
}
// The forms without a workspace are the reference's wrappers around the forms with one (lib/huf.h:141-167,209-211,271-280,299-323; lib/huf_decompress.c:186-192,
// :391-404, :439-452, :893-905, :940-952), the forms without a DCtx have a DTable of their own where the reference has one on its stack: HUF_CREATE_STATIC_DTABLEX1
// with HUF_TABLELOG_MAX - 1 (descriptor 0x0B00000B), HUF_CREATE_STATIC_DTABLEX2 with HUF_TABLELOG_MAX.
static size_t huf_decompress_host(int streams, bool x2, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize)
{
    const unsigned maxLog = x2 ? FSEHIP_HUF_TABLELOG_MAX : FSEHIP_HUF_TABLELOG_MAX - 1;
    std::vector<u32> dt(FSEHIP_HUF_DTABLE_SIZE_U32(maxLog), 0);
    dt[0] = (u32)maxLog * 0x01000001u;
    return huf_dctx_host(streams, x2, dt.data(), dst, dstSize, cSrc, cSrcSize, FSEHIP_HUF_DECOMPRESS_WORKSPACE_SIZE);
}
#define HUF_DCTX_ARGS FSEHIP_HUF_DTable* dctx, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize
#define HUF_DEC_ARGS void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize
extern "C" size_t FSEHIP_HUF_decompress4X1_DCtx_wksp(HUF_DCTX_ARGS, void*, size_t wkspSize) { return huf_dctx_host(4, false, dctx, dst, dstSize, cSrc, cSrcSize, wkspSize); }
extern "C" size_t FSEHIP_HUF_decompress1X1_DCtx_wksp(HUF_DCTX_ARGS, void*, size_t wkspSize) { return huf_dctx_host(1, false, dctx, dst, dstSize, cSrc, cSrcSize, wkspSize); }
extern "C" size_t FSEHIP_HUF_decompress4X2_DCtx_wksp(HUF_DCTX_ARGS, void*, size_t wkspSize) { return huf_dctx_host(4, true, dctx, dst, dstSize, cSrc, cSrcSize, wkspSize); }
extern "C" size_t FSEHIP_HUF_decompress1X2_DCtx_wksp(HUF_DCTX_ARGS, void*, size_t wkspSize) { return huf_dctx_host(1, true, dctx, dst, dstSize, cSrc, cSrcSize, wkspSize); }
extern "C" size_t FSEHIP_HUF_decompress4X1_DCtx(HUF_DCTX_ARGS) { return huf_dctx_host(4, false, dctx, dst, dstSize, cSrc, cSrcSize, FSEHIP_HUF_DECOMPRESS_WORKSPACE_SIZE); }
extern "C" size_t FSEHIP_HUF_decompress1X1_DCtx(HUF_DCTX_ARGS) { return huf_dctx_host(1, false, dctx, dst, dstSize, cSrc, cSrcSize, FSEHIP_HUF_DECOMPRESS_WORKSPACE_SIZE); }
extern "C" size_t FSEHIP_HUF_decompress4X2_DCtx(HUF_DCTX_ARGS) { return huf_dctx_host(4, true, dctx, dst, dstSize, cSrc, cSrcSize, FSEHIP_HUF_DECOMPRESS_WORKSPACE_SIZE); }
extern "C" size_t FSEHIP_HUF_decompress1X2_DCtx(HUF_DCTX_ARGS) { return huf_dctx_host(1, true, dctx, dst, dstSize, cSrc, cSrcSize, FSEHIP_HUF_DECOMPRESS_WORKSPACE_SIZE); }
extern "C" size_t FSEHIP_HUF_decompress4X1(HUF_DEC_ARGS) { return huf_decompress_host(4, false, dst, dstSize, cSrc, cSrcSize); }
extern "C" size_t FSEHIP_HUF_decompress1X1(HUF_DEC_ARGS) { return huf_decompress_host(1, false, dst, dstSize, cSrc, cSrcSize); }
extern "C" size_t FSEHIP_HUF_decompress4X2(HUF_DEC_ARGS) { return huf_decompress_host(4, true, dst, dstSize, cSrc, cSrcSize); }
extern "C" size_t FSEHIP_HUF_decompress1X2(HUF_DEC_ARGS) { return huf_decompress_host(1, true, dst, dstSize, cSrc, cSrcSize); }

static size_t huf_read_dtable_wksp_host(bool x2, FSEHIP_HUF_DTable* DTable, const void* src, size_t srcSize, size_t wkspSize)
{
    if (!x2 && wkspSize < HUF_X1_WKSP_BYTES) return FSEHIP_ERROR(tableLog_tooLarge);
    HostCall h;
    void* const dsrc = h.upload(src, srcSize);
    void* ddt = nullptr;
    return huf_read_dtable_host(h, x2, DTable, dsrc, srcSize, wkspSize, &ddt);
}
extern "C" size_t FSEHIP_HUF_readDTableX1_wksp(FSEHIP_HUF_DTable* DTable, const void* src, size_t srcSize, void*, size_t wkspSize) { return huf_read_dtable_wksp_host(false, DTable, src, srcSize, wkspSize); }
extern "C" size_t FSEHIP_HUF_readDTableX2_wksp(FSEHIP_HUF_DTable* DTable, const void* src, size_t srcSize, void*, size_t wkspSize) { return huf_read_dtable_wksp_host(true, DTable, src, srcSize, wkspSize); }
extern "C" size_t FSEHIP_HUF_readDTableX1(FSEHIP_HUF_DTable* DTable, const void* src, size_t srcSize) { return huf_read_dtable_wksp_host(false, DTable, src, srcSize, FSEHIP_HUF_DECOMPRESS_WORKSPACE_SIZE); }
extern "C" size_t FSEHIP_HUF_readDTableX2(FSEHIP_HUF_DTable* DTable, const void* src, size_t srcSize) { return huf_read_dtable_wksp_host(true, DTable, src, srcSize, FSEHIP_HUF_DECOMPRESS_WORKSPACE_SIZE); }    // :651-656

// lib/huf.h:204-218 (lib/huf_compress.c:334-421): HUF_buildCTable[_wksp] on the caller's counters, HUF_writeCTable (lib/huf.h:205, lib/huf_compress.c:113-148) on the
// caller's table -- batches of one on the phases of k_huf_cprep (huf_prep.hip).  The workspace is checked as the reference checks it (:345-348) and left alone.
extern "C" size_t FSEHIP_HUF_buildCTable(FSEHIP_HUF_CElt* tree, const unsigned* count, unsigned maxSymbolValue, unsigned maxNbBits)
{
    if (maxSymbolValue > 255) return FSEHIP_ERROR(maxSymbolValue_tooLarge);       // :350
    HostCall h;
    void* const dc = h.upload_padded(count, 4 * ((size_t)maxSymbolValue + 1), 1024); void* const dm = h.upload_scalar(maxSymbolValue); void* const dct = h.alloc(1024);
    size_t* const dr = h.alloc_result();
    RUN(h, FSEHIP_HUF_buildCTable_fromCount_batch((u32*)dct, 256, (const unsigned*)dc, 256, (const unsigned*)dm, maxNbBits, 1, dr, nullptr));
    const size_t r = h.result(dr);
    if (!FSEHIP_isError(r)) h.fetch(tree, dct, 4 * ((size_t)maxSymbolValue + 1));
    return h.ret(r);
}
extern "C" size_t FSEHIP_HUF_buildCTable_wksp(FSEHIP_HUF_CElt* tree, const unsigned* count, unsigned maxSymbolValue, unsigned maxNbBits, void* workSpace, size_t wkspSize)
{
    if ((size_t)workSpace & 3) return FSEHIP_ERROR(GENERIC);
    if (wkspSize < 4352) return FSEHIP_ERROR(workSpace_tooSmall);                 // sizeof(HUF_buildCTable_wksp_tables): 512 nodes of 8 bytes + 32 rank positions of 8
    return FSEHIP_HUF_buildCTable(tree, count, maxSymbolValue, maxNbBits);
}
extern "C" size_t FSEHIP_HUF_writeCTable(void* dst, size_t maxDstSize, const FSEHIP_HUF_CElt* CTable, unsigned maxSymbolValue, unsigned huffLog)
{
    if (maxSymbolValue > 255) return FSEHIP_ERROR(maxSymbolValue_tooLarge);       // :123
    const size_t cap = maxDstSize < 512 ? maxDstSize : 512;                       // (no header is longer than 1 + 255 bytes)
    HostCall h;
    void* const dh = h.alloc(512); void* const dct = h.upload_padded(CTable, 4 * ((size_t)maxSymbolValue + 1), 1024); void* const dm = h.upload_scalar(maxSymbolValue);
    size_t* const dr = h.alloc_result();
    RUN(h, FSEHIP_HUF_writeCTable_batch(dh, 512, cap, (const u32*)dct, 256, (const unsigned*)dm, huffLog, 1, dr, nullptr));
    const size_t r = h.result(dr);
    if (!FSEHIP_isError(r) && r > 0) h.fetch(dst, dh, r);
    return h.ret(r);
}
extern "C" size_t FSEHIP_HUF_compress(void* dst, size_t dstCapacity, const void* src, size_t srcSize)   // huf_compress.c:795-798
{
    return FSEHIP_HUF_compress2(dst, dstCapacity, src, srcSize, 255, FSEHIP_HUF_TABLELOG_DEFAULT);
}
extern "C" size_t FSEHIP_HUF_decompress(void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize)   // huf_decompress.c:1056-1081 (4X1 branch)
{
    if (dstSize == 0) return FSEHIP_ERROR(dstSize_tooSmall);
    const size_t wsBytes = FSEHIP_HUF_decompress_batch_workspaceSize(1);
    HostCall h;
    void* const dsrc = h.upload(cSrc, cSrcSize); void* const ddst = h.alloc(dstSize); void* const dws = h.alloc(wsBytes); size_t* const dres = h.alloc_result();
    RUN(h, FSEHIP_HUF_decompress_batch(ddst, dstSize, nullptr, dstSize, dres, dsrc, cSrcSize, nullptr, cSrcSize, 1, dws, wsBytes, nullptr));
    const size_t r = h.result(dres);
    if (!FSEHIP_isError(r) && r > 0) h.fetch(dst, ddst, r <= dstSize ? r : dstSize);
    return h.ret(r);
}

// ---- Layer 1, FSE for 16-bit symbols (lib/fseU16.c) ---------------------------------------------------
extern "C" size_t FSEHIP_FSE_countU16(unsigned* count, unsigned* maxSymbolValuePtr, const unsigned short* src, size_t srcSize)
{
    const unsigned in = *maxSymbolValuePtr;
    if (in > FSEHIP_FSEU16_MAX_SYMBOL_VALUE) return FSEHIP_ERROR(maxSymbolValue_tooLarge);
    HostCall h;
    void* const dsrc = h.upload(src, srcSize * 2); void* const dcnt = h.alloc(4 * (FSEHIP_FSEU16_MAX_SYMBOL_VALUE + 1)); void* const dmsv = h.alloc(4);
    size_t* const dres = h.alloc_result();
    RUN(h, FSEHIP_FSE_countU16_batch((unsigned*)dcnt, (unsigned*)dmsv, dres, (const unsigned short*)dsrc, srcSize * 2, nullptr, srcSize, in, 1, nullptr));
    const size_t r = h.result(dres);
    if (FSEHIP_isError(r)) return r;
    h.fetch(count, dcnt, 4 * ((size_t)in + 1));
    h.fetch(maxSymbolValuePtr, dmsv, 4);
    return h.ret(r);
}

extern "C" size_t FSEHIP_FSE_compressU16(void* dst, size_t dstCapacity, const unsigned short* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog)
{
    const size_t wsBytes = FSEHIP_FSE_compressU16_batch_workspaceSize(1);
    HostCall h;
    void* const dsrc = h.upload(src, srcSize * 2); void* const ddst = h.alloc(dstCapacity); void* const dws = h.alloc(wsBytes); size_t* const dres = h.alloc_result();
    RUN(h, FSEHIP_FSE_compressU16_batch(ddst, dstCapacity, dstCapacity, dres, (const unsigned short*)dsrc, srcSize * 2, nullptr, srcSize, maxSymbolValue, tableLog, 1, dws, wsBytes, nullptr));
    const size_t r = h.result(dres);
    if (!FSEHIP_isError(r) && r > 1) h.fetch(dst, ddst, r <= dstCapacity ? r : dstCapacity);
    return h.ret(r);
}

extern "C" size_t FSEHIP_FSE_decompressU16(unsigned short* dst, size_t dstCapacity, const void* cSrc, size_t cSrcSize)
{
    const size_t wsBytes = FSEHIP_FSE_decompressU16_batch_workspaceSize(1);
    HostCall h;
    void* const dsrc = h.upload(cSrc, cSrcSize); void* const ddst = h.alloc(dstCapacity * 2); void* const dws = h.alloc(wsBytes); size_t* const dres = h.alloc_result();
    // the device buffer starts as a copy of the caller's: what the decoder does not write stays what it was, as with the reference
    if (dstCapacity) h.copy_in(ddst, dst, dstCapacity * 2);
    RUN(h, FSEHIP_FSE_decompressU16_batch((unsigned short*)ddst, dstCapacity * 2, dstCapacity, dres, dsrc, cSrcSize, nullptr, cSrcSize, 1, dws, wsBytes, nullptr));
    const size_t r = h.result(dres);
    if (dstCapacity) h.fetch(dst, ddst, dstCapacity * 2);   // always, not on success alone: the reference writes what it decoded before it notices corruption
    return h.ret(r);
}

/* fsehip.h -- C ABI of libfsehip.so: the MI355X (gfx950) block-entropy-coding hot path.
 *
 * Drop-in boundary for the reference library's block API (Cyan4973/FiniteStateEntropy):
 *   lib/hist.h:30-31      HIST_count
 *   lib/fse.h:67-105      FSE_compress / FSE_decompress / FSE_compress2 (one-shot block API)
 *   lib/fse.h:142-247     FSE_compress_usingCTable (:174), FSE_decompress_usingDTable (:247)
 *   lib/huf.h:54-98       HUF_compress / HUF_decompress / HUF_compress2
 *   lib/huf.h:190,290     HUF_compress4X_usingCTable, HUF_compress1X_usingCTable
 *   lib/huf.h:275-277     HUF_decompress4X_usingDTable, HUF_decompress4X1_usingDTable
 *   lib/huf.h:157-167,271-280,304-323   the double-symbol family: HUF_readDTableX2[_wksp], HUF_decompress4X2 / 1X2[_DCtx[_wksp]],
 *                         HUF_decompress4X2_usingDTable, HUF_decompress1X2_usingDTable -- the table is built on the device
 *
 * Every function keeps the reference's signature, argument meaning, in-memory table layouts
 * (FSE_CTable / FSE_DTable = unsigned[], HUF_CElt = {U16 val; BYTE nbBits;} stride 4,
 * HUF_DTable = U32[] with a 4-byte DTableDesc), bitstream/header format and the size_t error
 * convention (lib/error_private.h:77-79: (size_t)-code, code in FSEHIP_ErrorCode).  Encoders
 * return 0 ("not compressible / does not fit") and, for the one-shot forms, 1 ("single repeated
 * byte") exactly where the reference does (lib/fse.h:62-65, lib/huf.h:50-52).
 *
 * All computation happens in hand-written HIP kernels; there is NO CPU fallback: if no gfx950
 * device is usable the single-block calls return FSEHIP_ERROR(GENERIC) and the batch calls return
 * the failing hipError_t.
 *
 * Two layers:
 *   1. single-block calls on HOST pointers (same signatures as the reference, prefix FSEHIP_;
 *      define FSEHIP_DROPIN_NAMES before including this header to also get the original names
 *      as macros so reference callers such as programs/fuzzer.c or programs/fullbench.c link
 *      against this library unchanged);
 *   2. batched calls on DEVICE pointers (many independent blocks per launch -- the data-parallel
 *      axis of programs/bench.c:353-364,389-424), which is what reaches throughput.
 */
#ifndef FSEHIP_H
#define FSEHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSEHIP_API __attribute__((visibility("default")))

/* ---- error convention (lib/error_public.h:45-56, lib/error_private.h:77-79) ------------------ */
typedef enum {
    FSEHIP_error_no_error = 0,
    FSEHIP_error_GENERIC = 1,
    FSEHIP_error_dstSize_tooSmall = 2,
    FSEHIP_error_srcSize_wrong = 3,
    FSEHIP_error_corruption_detected = 4,
    FSEHIP_error_tableLog_tooLarge = 5,
    FSEHIP_error_maxSymbolValue_tooLarge = 6,
    FSEHIP_error_maxSymbolValue_tooSmall = 7,
    FSEHIP_error_workSpace_tooSmall = 8,
    FSEHIP_error_maxCode = 9
} FSEHIP_ErrorCode;
#define FSEHIP_ERROR(name) ((size_t)0 - (size_t)FSEHIP_error_##name)
FSEHIP_API unsigned FSEHIP_isError(size_t code);            /* FSE_isError / HUF_isError / HIST_isError */
FSEHIP_API const char* FSEHIP_getErrorName(size_t code);    /* FSE_getErrorName */

/* ---- sizes (lib/fse.h:290-296, lib/huf.h:131-145) --------------------------------------------- */
#define FSEHIP_FSE_MAX_TABLELOG 12
#define FSEHIP_FSE_DEFAULT_TABLELOG 11
#define FSEHIP_FSE_MIN_TABLELOG 5
#define FSEHIP_FSE_NCOUNTBOUND 512
#define FSEHIP_FSE_BLOCKBOUND(size) ((size) + ((size) >> 7) + 4 + sizeof(size_t))
#define FSEHIP_FSE_COMPRESSBOUND(size) (FSEHIP_FSE_NCOUNTBOUND + FSEHIP_FSE_BLOCKBOUND(size))
#define FSEHIP_FSE_CTABLE_SIZE_U32(maxTableLog, maxSymbolValue) (1 + (1 << ((maxTableLog)-1)) + (((maxSymbolValue) + 1) * 2))
#define FSEHIP_FSE_DTABLE_SIZE_U32(maxTableLog) (1 + (1 << (maxTableLog)))
#define FSEHIP_FSE_WKSP_SIZE_U32(maxTableLog, maxSymbolValue) (FSEHIP_FSE_CTABLE_SIZE_U32(maxTableLog, maxSymbolValue) + (((maxTableLog) > 12) ? (1 << ((maxTableLog)-2)) : 1024))   /* lib/fse.h:314 */
#define FSEHIP_HIST_WKSP_SIZE_U32 1024                                             /* lib/hist.h:38-39 */
#define FSEHIP_HIST_WKSP_SIZE (FSEHIP_HIST_WKSP_SIZE_U32 * sizeof(unsigned))
#define FSEHIP_HUF_WORKSPACE_SIZE ((6 << 10) + 256)                                /* lib/huf.h:93-94 */
#define FSEHIP_HUF_WORKSPACE_SIZE_U32 (FSEHIP_HUF_WORKSPACE_SIZE / sizeof(uint32_t))
#define FSEHIP_HUF_DECOMPRESS_WORKSPACE_SIZE (2 << 10)                             /* lib/huf.h:263 */
#define FSEHIP_HUF_TABLELOG_MAX 12
#define FSEHIP_HUF_TABLELOG_DEFAULT 11
#define FSEHIP_HUF_BLOCKSIZE_MAX (128 * 1024)
#define FSEHIP_HUF_COMPRESSBOUND(size) (129 + ((size) + ((size) >> 8) + 8))
#define FSEHIP_HUF_CTABLE_SIZE_U32(maxSymbolValue) ((maxSymbolValue) + 1)
#define FSEHIP_HUF_DTABLE_SIZE_U32(maxTableLog) (1 + (1 << (maxTableLog)))

typedef unsigned FSEHIP_FSE_CTable;   /* lib/fse.h:160 */
typedef unsigned FSEHIP_FSE_DTable;   /* lib/fse.h:233 */
typedef uint32_t FSEHIP_HUF_CElt;     /* lib/huf.h:187 + lib/huf_compress.c:106-109 : {U16 val; BYTE nbBits; pad} */
typedef uint32_t FSEHIP_HUF_DTable;   /* lib/huf.h:144 */

/* =================================================================================================
 *  Layer 1 -- single-block, HOST pointers, reference signatures
 * ================================================================================================= */
/* lib/hist.h:30  (semantics lib/hist.c:163-180) */
FSEHIP_API size_t FSEHIP_HIST_count(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize);

/* lib/hist.h:46, :54.  The _wksp forms below are what the reference's own callers go through (SURVEY 8(b) "what calls it": fse_compress.c:652,
 * huf_compress.c:672, huf_decompress.c:428).  Their workspaces are validated exactly as the reference validates them -- same checks, same order, same
 * error codes -- and then left alone: every table and counter lives in device memory.  HIST_countFast is the unchecked variant: a limit below
 * 255 bounds the entries written, larger symbols are counted into the result and *maxSymbolValuePtr but are no error (lib/hist.c:120-131). */
FSEHIP_API size_t FSEHIP_HIST_count_wksp(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize, void* workSpace, size_t workSpaceSize);
FSEHIP_API size_t FSEHIP_HIST_countFast(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize);
/* lib/hist.h:62 (below 1500 bytes the workspace is not looked at, lib/hist.c:141-150) and :74 (returns the largest count as `unsigned`) */
FSEHIP_API size_t FSEHIP_HIST_countFast_wksp(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize, void* workSpace, size_t workSpaceSize);
FSEHIP_API unsigned FSEHIP_HIST_count_simple(unsigned* count, unsigned* maxSymbolValuePtr, const void* src, size_t srcSize);

/* lib/fse.h:174 */
FSEHIP_API size_t FSEHIP_FSE_compress_usingCTable(void* dst, size_t dstCapacity, const void* src, size_t srcSize, const FSEHIP_FSE_CTable* ct);
/* lib/fse.h:247 */
FSEHIP_API size_t FSEHIP_FSE_decompress_usingDTable(void* dst, size_t dstCapacity, const void* cSrc, size_t cSrcSize, const FSEHIP_FSE_DTable* dt);
/* lib/fse.h:76, :104, :90 */
FSEHIP_API size_t FSEHIP_FSE_compress(void* dst, size_t dstCapacity, const void* src, size_t srcSize);
FSEHIP_API size_t FSEHIP_FSE_compress2(void* dst, size_t dstCapacity, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog);
FSEHIP_API size_t FSEHIP_FSE_decompress(void* dst, size_t dstCapacity, const void* cSrc, size_t cSrcSize);
/* lib/fse.h:315 (wkspSize in bytes against FSE_WKSP_SIZE_U32, as lib/fse_compress.c:646 compares them; a table log above 12 codes like 12,
 * :340) and lib/fse.h:335 (maxLog honoured, limits above FSE_MAX_TABLELOG count as 12; `workSpace`, when given, receives the DTable the
 * reference would have built there) */
FSEHIP_API size_t FSEHIP_FSE_compress_wksp(void* dst, size_t dstSize, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog, void* workSpace, size_t wkspSize);
FSEHIP_API size_t FSEHIP_FSE_decompress_wksp(void* dst, size_t dstCapacity, const void* cSrc, size_t cSrcSize, FSEHIP_FSE_DTable* workSpace, unsigned maxLog);
/* The steps between the histogram and the hot loops under their own names -- the reference's "advanced" flow (lib/fse.h:107-163, :218-241: count,
 * FSE_optimalTableLog, FSE_normalizeCount, FSE_writeNCount, FSE_buildCTable, FSE_compress_usingCTable / FSE_readNCount, FSE_buildDTable,
 * FSE_decompress_usingDTable), each a batch of one on the device routines the one-shot calls run (csrc/wave_glue.h, ncount_reader.h,
 * fse_wave_build.h); FSE_optimalTableLog and FSE_NCountWriteBound are arithmetic on their arguments (lib/fse_compress.c:186-190, :325-347).
 * lib/fse.h:119, :137, :144, :150, :162 (+ :341 the _wksp form: workspace checked as lib/fse_compress.c:86 checks it, then left alone), :222, :240.
 * Where the reference is undefined the call refuses: normalised counters that do not add up to 1 << tableLog cells or go below -1 (the CTable
 * builder asserts, lib/fse_compress.c:127; the DTable builder returns GENERIC, lib/fse_decompress.c:107) -> GENERIC from both builders;
 * tableLog 0, 1 or 3 -> GENERIC (FSE_TABLESTEP(2) and (8) are even, lib/fse.h:683: the reference's spread never leaves cell 0 and the rest of its table is
 * whatever the memory held; 2, 4 and everything from FSE_MIN_TABLELOG up are exact); maxSymbolValue > 255 -> maxSymbolValue_tooLarge (byte alphabets; FSE_buildDTable says so itself, :83).  A failed
 * FSE_writeNCount / FSE_readNCount leaves its output untouched (the reference may have written part of it). */
/* Precondition, as in the reference: srcSize > 1 and maxSymbolValue >= 1.  Outside it the call still returns (the highest bit of 0 counts as bit 0). */
FSEHIP_API unsigned FSEHIP_FSE_optimalTableLog(unsigned maxTableLog, size_t srcSize, unsigned maxSymbolValue);
FSEHIP_API size_t FSEHIP_FSE_normalizeCount(short* normalizedCounter, unsigned tableLog, const unsigned* count, size_t srcSize, unsigned maxSymbolValue);
FSEHIP_API size_t FSEHIP_FSE_NCountWriteBound(unsigned maxSymbolValue, unsigned tableLog);
FSEHIP_API size_t FSEHIP_FSE_writeNCount(void* buffer, size_t bufferSize, const short* normalizedCounter, unsigned maxSymbolValue, unsigned tableLog);
FSEHIP_API size_t FSEHIP_FSE_readNCount(short* normalizedCounter, unsigned* maxSymbolValuePtr, unsigned* tableLogPtr, const void* rBuffer, size_t rBuffSize);
FSEHIP_API size_t FSEHIP_FSE_buildCTable(FSEHIP_FSE_CTable* ct, const short* normalizedCounter, unsigned maxSymbolValue, unsigned tableLog);
FSEHIP_API size_t FSEHIP_FSE_buildCTable_wksp(FSEHIP_FSE_CTable* ct, const short* normalizedCounter, unsigned maxSymbolValue, unsigned tableLog, void* workSpace, size_t wkspSize);
FSEHIP_API size_t FSEHIP_FSE_buildDTable(FSEHIP_FSE_DTable* dt, const short* normalizedCounter, unsigned maxSymbolValue, unsigned tableLog);

/* lib/huf.h:290, :190 */
FSEHIP_API size_t FSEHIP_HUF_compress1X_usingCTable(void* dst, size_t dstSize, const void* src, size_t srcSize, const FSEHIP_HUF_CElt* CTable);
FSEHIP_API size_t FSEHIP_HUF_compress4X_usingCTable(void* dst, size_t dstSize, const void* src, size_t srcSize, const FSEHIP_HUF_CElt* CTable);
/* lib/huf.h:275-277.  HUF_decompress4X_usingDTable dispatches on the table type like lib/huf_decompress.c:980-997: tableType 0 = X1
 * (single-symbol) cells, tableType 1 = X2 (double-symbol) cells from the reference's HUF_readDTableX2 -- both accepted.
 * HUF_decompress4X1_usingDTable rejects an X2 table with GENERIC exactly as the reference does (lib/huf_decompress.c:411-412). */
FSEHIP_API size_t FSEHIP_HUF_decompress4X_usingDTable(void* dst, size_t maxDstSize, const void* cSrc, size_t cSrcSize, const FSEHIP_HUF_DTable* DTable);
FSEHIP_API size_t FSEHIP_HUF_decompress4X1_usingDTable(void* dst, size_t maxDstSize, const void* cSrc, size_t cSrcSize, const FSEHIP_HUF_DTable* DTable);
/* lib/huf.h:318-320: single-stream blocks, what HUF_compress1X_usingCTable writes (lib/huf_decompress.c:239-260, 961-975).  The 1X1 form
 * rejects a double-symbol table with GENERIC (:367-369), the 1X form takes both table types like its 4X sibling. */
FSEHIP_API size_t FSEHIP_HUF_decompress1X_usingDTable(void* dst, size_t maxDstSize, const void* cSrc, size_t cSrcSize, const FSEHIP_HUF_DTable* DTable);
FSEHIP_API size_t FSEHIP_HUF_decompress1X1_usingDTable(void* dst, size_t maxDstSize, const void* cSrc, size_t cSrcSize, const FSEHIP_HUF_DTable* DTable);
/* lib/huf.h:66, :95, :82 */
FSEHIP_API size_t FSEHIP_HUF_compress(void* dst, size_t dstCapacity, const void* src, size_t srcSize);
FSEHIP_API size_t FSEHIP_HUF_compress2(void* dst, size_t dstCapacity, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog);
FSEHIP_API size_t FSEHIP_HUF_decompress(void* dst, size_t originalSize, const void* cSrc, size_t cSrcSize);
/* lib/huf.h:95, :289 (workSpace: 4-byte aligned, at least HUF_WORKSPACE_SIZE bytes -- GENERIC / workSpace_tooSmall otherwise, lib/huf_compress.c:654-655;
 * the 1X form writes a single stream without jump table) and lib/huf.h:164 (dctx: a DTable whose descriptor holds the table-log limit, as
 * HUF_CREATE_STATIC_DTABLEX1 leaves it; it receives the table read from the block's header, lib/huf_decompress.c:417-431) */
FSEHIP_API size_t FSEHIP_HUF_compress4X_wksp(void* dst, size_t dstCapacity, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog, void* workSpace, size_t wkspSize);
FSEHIP_API size_t FSEHIP_HUF_compress1X(void* dst, size_t dstSize, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog);   /* lib/huf.h:288: HUF_compress1X_wksp with a workspace of its own */
FSEHIP_API size_t FSEHIP_HUF_compress1X_wksp(void* dst, size_t dstSize, const void* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog, void* workSpace, size_t wkspSize);
FSEHIP_API size_t FSEHIP_HUF_decompress4X1_DCtx_wksp(FSEHIP_HUF_DTable* dctx, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize, void* workSpace, size_t wkspSize);
/* the rest of the single-symbol family (lib/huf.h:141-143 HUF_decompress4X1, :161-163 its DCtx form, :209-211 HUF_readDTableX1[_wksp], :299-304 the 1X1
 * forms; lib/huf_decompress.c:118-192, :377-404, :439-452): the header's table into the caller's DTable / DCtx, then the four streams (4X1) or the single
 * stream (1X1) behind it.  Workspaces are checked as the reference checks them ((16 + 64) words, tableLog_tooLarge) and then left alone. */
/* the double-symbol family, lib/huf.h:157 HUF_decompress4X2, :166-167 its DCtx forms, :271-272 HUF_readDTableX2[_wksp], :280 HUF_decompress4X2_usingDTable,
 * :304 HUF_decompress1X2, :314-315 its DCtx forms, :323 HUF_decompress1X2_usingDTable (lib/huf_decompress.c:551-656, :867-952).  The table -- descriptor
 * {maxTableLog as found, tableType 1, tableLog = maxTableLog} and 1 << maxTableLog cells {U16 sequence; BYTE nbBits; BYTE length} -- is built on the device
 * from the weights header and is word for word the reference's.  workSpace: smaller than the 1500 bytes lib/huf_decompress.c:570-581 lay out ->
 * tableLog_tooLarge, before the descriptor's maxTableLog > 12 -> tableLog_tooLarge (:587), before the header is read; otherwise left alone.  The
 * _usingDTable forms refuse a table of tableType 0 with GENERIC (:873, :913).  Streams are decoded by the double-symbol decoder, so damaged ones
 * get the verdict of the reference's X2 functions (which is not always that of its X1 functions). */
FSEHIP_API size_t FSEHIP_HUF_readDTableX2(FSEHIP_HUF_DTable* DTable, const void* src, size_t srcSize);
FSEHIP_API size_t FSEHIP_HUF_readDTableX2_wksp(FSEHIP_HUF_DTable* DTable, const void* src, size_t srcSize, void* workSpace, size_t wkspSize);
FSEHIP_API size_t FSEHIP_HUF_decompress4X2(void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize);
FSEHIP_API size_t FSEHIP_HUF_decompress4X2_DCtx(FSEHIP_HUF_DTable* dctx, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize);
FSEHIP_API size_t FSEHIP_HUF_decompress4X2_DCtx_wksp(FSEHIP_HUF_DTable* dctx, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize, void* workSpace, size_t wkspSize);
FSEHIP_API size_t FSEHIP_HUF_decompress1X2(void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize);
FSEHIP_API size_t FSEHIP_HUF_decompress1X2_DCtx(FSEHIP_HUF_DTable* dctx, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize);
FSEHIP_API size_t FSEHIP_HUF_decompress1X2_DCtx_wksp(FSEHIP_HUF_DTable* dctx, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize, void* workSpace, size_t wkspSize);
FSEHIP_API size_t FSEHIP_HUF_decompress4X2_usingDTable(void* dst, size_t maxDstSize, const void* cSrc, size_t cSrcSize, const FSEHIP_HUF_DTable* DTable);
FSEHIP_API size_t FSEHIP_HUF_decompress1X2_usingDTable(void* dst, size_t maxDstSize, const void* cSrc, size_t cSrcSize, const FSEHIP_HUF_DTable* DTable);
/* lib/huf.h:204-218 (lib/huf_compress.c:113-148, :334-421): the compress-side table calls on the caller's own statistics -- HUF_buildCTable[_wksp] from
 * count[0 .. maxSymbolValue] (returns the table log; tree[0 .. maxSymbolValue] receives the codes), HUF_writeCTable from such a table (returns the header
 * size).  Refused where the reference is undefined: no symbol in use, a count of 2^23 or more (blocks are at most HUF_BLOCKSIZE_MAX = 128 KB), more
 * symbols in use than codes of maxNbBits bits, a code length above huffLog or a huffLog above 12 in HUF_writeCTable -> GENERIC. */
FSEHIP_API size_t FSEHIP_HUF_buildCTable(FSEHIP_HUF_CElt* tree, const unsigned* count, unsigned maxSymbolValue, unsigned maxNbBits);
FSEHIP_API size_t FSEHIP_HUF_buildCTable_wksp(FSEHIP_HUF_CElt* tree, const unsigned* count, unsigned maxSymbolValue, unsigned maxNbBits, void* workSpace, size_t wkspSize);
FSEHIP_API size_t FSEHIP_HUF_writeCTable(void* dst, size_t maxDstSize, const FSEHIP_HUF_CElt* CTable, unsigned maxSymbolValue, unsigned huffLog);
FSEHIP_API size_t FSEHIP_HUF_readDTableX1(FSEHIP_HUF_DTable* DTable, const void* src, size_t srcSize);
FSEHIP_API size_t FSEHIP_HUF_readDTableX1_wksp(FSEHIP_HUF_DTable* DTable, const void* src, size_t srcSize, void* workSpace, size_t wkspSize);
FSEHIP_API size_t FSEHIP_HUF_decompress4X1(void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize);
FSEHIP_API size_t FSEHIP_HUF_decompress4X1_DCtx(FSEHIP_HUF_DTable* dctx, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize);
FSEHIP_API size_t FSEHIP_HUF_decompress1X1(void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize);
FSEHIP_API size_t FSEHIP_HUF_decompress1X1_DCtx(FSEHIP_HUF_DTable* dctx, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize);
FSEHIP_API size_t FSEHIP_HUF_decompress1X1_DCtx_wksp(FSEHIP_HUF_DTable* dctx, void* dst, size_t dstSize, const void* cSrc, size_t cSrcSize, void* workSpace, size_t wkspSize);

/* =================================================================================================
 *  Layer 2 -- batched, DEVICE pointers.  Block b lives at base + b*stride.  `d_sizes` may be
 *  NULL, in which case every block has `uniformSize` bytes.  `d_results[b]` receives exactly what
 *  the corresponding single-block reference call would return for block b.  `stream` is a
 *  hipStream_t (NULL = default stream).  Return value: 0 (hipSuccess) or a hipError_t.
 *  Launches are asynchronous on `stream`; the library never allocates on these paths (one exception, made once per device: FSEHIP_prepareDevice below).
 *  Streams and graphs: a call is kernel launches on `stream` and nothing else -- no host synchronisation, no
 *  read-back (what one stage decides for the next travels in device-side lists inside the workspace), no
 *  memset or copy nodes -- so after one ordinary call (which sets the kernels' function attributes) the calls
 *  can be captured into a HIP graph (hipStreamBeginCapture on `stream`) and replayed on new contents of the
 *  same buffers (tests/test_gpu_graph.py).
 * ================================================================================================= */
/* HIST_count over a batch.  d_counts: nBlocks x 256 unsigned (entries 0..min(maxSV_in,255) written).
 * d_maxSymbolValues: nBlocks in/out values (NULL = 255 in, not reported). */
FSEHIP_API int FSEHIP_HIST_count_batch(unsigned* d_counts, unsigned* d_maxSymbolValues, size_t* d_results,
                                       const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                       size_t nBlocks, void* stream);

/* FSE_compress_usingCTable over a batch.  Table of block b: d_ctables + b*ctableStrideU32 (reference
 * layout; pass ctableStrideU32 = 0 to share one table).  maxTableLog bounds the tableLog found in the
 * tables (<= 12; smaller values raise occupancy); a table exceeding it yields ERROR(tableLog_tooLarge). */
FSEHIP_API int FSEHIP_FSE_compress_usingCTable_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                                     const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                                     const FSEHIP_FSE_CTable* d_ctables, size_t ctableStrideU32, unsigned maxTableLog,
                                                     size_t nBlocks, void* stream);
/* FSE_decompress_usingDTable over a batch (d_cSizes: exact compressed size per block). */
FSEHIP_API int FSEHIP_FSE_decompress_usingDTable_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                                       const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                       const FSEHIP_FSE_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                       size_t nBlocks, void* stream);

/* One-shot block API over a batch: FSE_compress2 (histogram, normalisation, NCount header, CTable,
 * payload) and FSE_decompress_wksp(maxLog) entirely on the device.  d_workspace/workspaceBytes: scratch,
 * at least FSEHIP_*_workspaceSize(1,...) bytes; larger workspaces process more blocks per pass (the
 * *_workspaceSize(nBlocks, ...) value never needs to be exceeded).  Every d_workspace of this header must be
 * 256-byte aligned (hipMalloc'ed memory is); a misaligned one is refused with hipErrorInvalidValue. */
FSEHIP_API size_t FSEHIP_FSE_compress_batch_workspaceSize(size_t nBlocks, unsigned tableLog);
FSEHIP_API int FSEHIP_FSE_compress_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                         const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                         unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks,
                                         void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API size_t FSEHIP_FSE_decompress_batch_workspaceSize(size_t nBlocks, unsigned maxLog);
FSEHIP_API int FSEHIP_FSE_decompress_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                           const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                           unsigned maxLog, size_t nBlocks,
                                           void* d_workspace, size_t workspaceBytes, void* stream);

/* Huff0: HUF_compress4X_usingCTable / HUF_decompress4X1_usingDTable over a batch, and the one-shot
 * HUF_compress2 / HUF_decompress (4X1 decoder) over a batch.  For the one-shot decoder d_dstSizes (or
 * uniformDstSize) is the exact regenerated size of each block, as HUF_decompress requires.
 * Memory contract of the batched calls (tests/test_gpu_edges.py, guard mode of tests/conftest.py): nothing is read behind
 * src + srcSize / cSrc + cSrcSize, nothing is written behind dst + dstCapacity (decoders: dst + dstSize); FSE tables are read
 * at their exact sizes (FSE_CTABLE_SIZE_U32(tableLog, maxSymbolValue) / FSE_DTABLE_SIZE_U32(tableLog) of the table's own header),
 * Huff0 DTables at 1 + (1 << tableLog) cells of their type.  A HUF_CElt table carries no header, so every table of a batch must
 * be readable at HUF_CTABLE_SIZE_U32(255) = 256 entries (what the reference's own callers declare, lib/huf_compress.c:628-632);
 * entries of symbols that do not occur are not interpreted.  The single-block calls on host pointers read only the entries of
 * symbols present in src, like the reference. */
FSEHIP_API int FSEHIP_HUF_compress4X_usingCTable_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                                       const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                                       const FSEHIP_HUF_CElt* d_ctables, size_t ctableStrideU32,
                                                       size_t nBlocks, void* stream);
/* HUF_compress1X_usingCTable over a batch (lib/huf.h:290; lib/huf_compress.c:457-502): one stream per block, no jump table */
FSEHIP_API int FSEHIP_HUF_compress1X_usingCTable_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                                       const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                                       const FSEHIP_HUF_CElt* d_ctables, size_t ctableStrideU32,
                                                       size_t nBlocks, void* stream);
FSEHIP_API int FSEHIP_HUF_decompress4X1_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                          size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                          const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                          size_t nBlocks, void* stream);
/* HUF_decompress4X_usingDTable over a batch (lib/huf.h:275, lib/huf_decompress.c:980-997): per block, tables of tableType 0
 * (single-symbol cells, from HUF_readDTableX1) take the fast decoder, tables of tableType 1 (double-symbol cells, from the
 * reference's HUF_readDTableX2: 4 bytes per cell, 1 + (1 << tableLog) words) an acceptance path with the reference's lock-step
 * semantics.  The 4X1 call above rejects tableType 1 with GENERIC exactly like HUF_decompress4X1_usingDTable. */
FSEHIP_API int FSEHIP_HUF_decompress4X_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                         size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                         const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                         size_t nBlocks, void* stream);
/* HUF_decompress1X1_usingDTable / HUF_decompress1X_usingDTable over a batch: one stream per block (the inverse of FSEHIP_HUF_compress1X_usingCTable_batch).
 * The stream is split across the 64 lanes of a wave like the streams of the 4X layout, in pieces when it exceeds the LDS budget. */
FSEHIP_API int FSEHIP_HUF_decompress1X1_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                          size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                          const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                          size_t nBlocks, void* stream);
FSEHIP_API int FSEHIP_HUF_decompress1X_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                         size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                         const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                         size_t nBlocks, void* stream);
/* HUF_decompress4X2_usingDTable / HUF_decompress1X2_usingDTable over a batch (lib/huf.h:280, :323; lib/huf_decompress.c:867-875, :907-915): the two
 * dispatching calls above, except that a block whose table has tableType 0 gets GENERIC (:873, :913; what its destination then holds is unspecified). */
FSEHIP_API int FSEHIP_HUF_decompress4X2_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                          size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                          const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                          size_t nBlocks, void* stream);
FSEHIP_API int FSEHIP_HUF_decompress1X2_usingDTable_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                                          size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                                          const FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog,
                                                          size_t nBlocks, void* stream);
FSEHIP_API size_t FSEHIP_HUF_compress_batch_workspaceSize(size_t nBlocks);
FSEHIP_API int FSEHIP_HUF_compress_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                         const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                         unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks,
                                         void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API size_t FSEHIP_HUF_decompress_batch_workspaceSize(size_t nBlocks);
FSEHIP_API int FSEHIP_HUF_decompress_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize,
                                           size_t* d_results, const void* d_cSrc, size_t cStride, const size_t* d_cSizes, size_t uniformCSize,
                                           size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream);

/* ---- Tables for the *_usingCTable / *_usingDTable batch calls, built on the device from the blocks themselves: the steps the
 * reference runs between HIST_count and the hot loops (SURVEY 8(a') g1-g3, g5-g6), as calls of their own so that a caller of the
 * using-table forms never has to build tables on the host and upload them.
 *   FSE_buildCTable_batch  = HIST_count + the early-outs of FSE_compress_wksp + FSE_optimalTableLog + FSE_normalizeCount +
 *                            FSE_writeNCount + FSE_buildCTable_wksp per block (lib/fse_compress.c:646-665).  d_ctables + b*ctableStrideU32
 *                            receives the CTable in the reference's layout (ctableStrideU32 >= FSE_CTABLE_SIZE_U32(max(tableLog, 9), 255):
 *                            FSE_optimalTableLog may raise a small request), d_headers + b*headerStride the NCount header (at most
 *                            headerCapacity bytes), d_results[b] the header size (> 1: table and header valid) or what FSE_compress2 returns
 *                            when it stops before coding: 0 (not compressible), 1 (one repeated byte) or an error code.
 *   FSE_buildDTable_batch  = FSE_readNCount + the maxLog check + FSE_buildDTable per block (lib/fse_decompress.c:264-271): d_headers
 *                            points at the NCount headers (or at whole compressed blocks); d_dtables + b*dtableStrideU32 receives the DTable
 *                            in the reference's layout (dtableStrideU32 >= FSE_DTABLE_SIZE_U32(maxLog)); d_results[b] = bytes the header
 *                            takes (where the payload starts) or an error code.
 *   HUF_buildCTable_batch  = HIST_count + early-outs + HUF_buildCTable_wksp + HUF_writeCTable per block (lib/huf_compress.c:654-703): 256
 *                            HUF_CElt per table (ctableStrideU32 >= 256), the weights header in d_headers, d_results[b] = header size or
 *                            0 / 1 (the repeated byte goes to d_headers[b][0]) / error as HUF_compress2.
 *   HUF_readDTableX1_batch = HUF_readDTableX1 per block (lib/huf_decompress.c:118-185): single-symbol DTable with DTableDesc.maxTableLog =
 *                            maxTableLog (dtableStrideU32 >= HUF_DTABLE_SIZE(maxTableLog) = 1 + (1 << maxTableLog)); d_results[b] = header size or error. */
FSEHIP_API size_t FSEHIP_FSE_buildCTable_batch_workspaceSize(size_t nBlocks);
FSEHIP_API int FSEHIP_FSE_buildCTable_batch(FSEHIP_FSE_CTable* d_ctables, size_t ctableStrideU32, void* d_headers, size_t headerStride, size_t headerCapacity,
                                            size_t* d_results, const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                            unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API size_t FSEHIP_FSE_buildDTable_batch_workspaceSize(size_t nBlocks, unsigned maxLog);
FSEHIP_API int FSEHIP_FSE_buildDTable_batch(FSEHIP_FSE_DTable* d_dtables, size_t dtableStrideU32, size_t* d_results,
                                            const void* d_headers, size_t headerStride, const size_t* d_headerSizes, size_t uniformHeaderSize,
                                            unsigned maxLog, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API size_t FSEHIP_HUF_buildCTable_batch_workspaceSize(size_t nBlocks);
FSEHIP_API int FSEHIP_HUF_buildCTable_batch(FSEHIP_HUF_CElt* d_ctables, size_t ctableStrideU32, void* d_headers, size_t headerStride, size_t headerCapacity,
                                            size_t* d_results, const void* d_src, size_t srcStride, const size_t* d_sizes, size_t uniformSize,
                                            unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream);
/*   HUF_buildCTable_fromCount / HUF_writeCTable : the two halves of HUF_buildCTable_batch on the CALLER's statistics -- d_counts + b*256 holds
 *                            count[0 .. d_maxSymbolValues[b]] (countStride must be 256), d_ctables + b*ctableStrideU32 the 256 HUF_CElt of table b
 *                            (ctableStrideU32 >= 256, a multiple of 4: anything else is hipErrorInvalidValue from both calls, nothing launched);
 *                            d_results[b] = the table log / the header size, or an error.  Entries of count[] and of the HUF_CElt row above
 *                            d_maxSymbolValues[b] are ignored and may hold anything (the built table is zero there). */
FSEHIP_API int FSEHIP_HUF_buildCTable_fromCount_batch(FSEHIP_HUF_CElt* d_ctables, size_t ctableStrideU32, const unsigned* d_counts, size_t countStride,
                                                      const unsigned* d_maxSymbolValues, unsigned maxNbBits, size_t nBlocks, size_t* d_results, void* stream);
FSEHIP_API int FSEHIP_HUF_writeCTable_batch(void* d_headers, size_t headerStride, size_t headerCapacity, const FSEHIP_HUF_CElt* d_ctables, size_t ctableStrideU32,
                                            const unsigned* d_maxSymbolValues, unsigned huffLog, size_t nBlocks, size_t* d_results, void* stream);
FSEHIP_API size_t FSEHIP_HUF_readDTableX1_batch_workspaceSize(size_t nBlocks);
FSEHIP_API int FSEHIP_HUF_readDTableX1_batch(FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog, size_t* d_results,
                                             const void* d_src, size_t srcStride, const size_t* d_srcSizes, size_t uniformSrcSize,
                                             size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream);
/*   HUF_readDTableX2_batch = HUF_readDTableX2 per block (lib/huf_decompress.c:551-649): the double-symbol DTable -- descriptor {maxTableLog, tableType 1,
 *                            tableLog = maxTableLog, reserved as HUF_CREATE_STATIC_DTABLEX2 leaves it} and 1 << maxTableLog cells {U16 sequence; BYTE nbBits;
 *                            BYTE length}, word for word the reference's -- for the dispatching / 4X2 / 1X2 _usingDTable batch calls.  d_dtables 4-byte
 *                            aligned, dtableStrideU32 >= 1 + (1 << maxTableLog); d_results[b] = header size or the reference's error, and a failing block
 *                            writes nothing to its table.  maxTableLog is DTableDesc.maxTableLog as the reference reads it, NOT a request with a default:
 *                            above 12 every block fails with tableLog_tooLarge (:587), a header with a larger tableLog likewise (:594). */
FSEHIP_API size_t FSEHIP_HUF_readDTableX2_batch_workspaceSize(size_t nBlocks);
FSEHIP_API int FSEHIP_HUF_readDTableX2_batch(FSEHIP_HUF_DTable* d_dtables, size_t dtableStrideU32, unsigned maxTableLog, size_t* d_results,
                                             const void* d_src, size_t srcStride, const size_t* d_srcSizes, size_t uniformSrcSize,
                                             size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream);

/* ---- Table glue, step by step: the reference's public FSE_normalizeCount (lib/fse.h:137-144, lib/fse_compress.c:431-494), FSE_writeNCount
 * (lib/fse.h:150-156, lib/fse_compress.c:275-298) and FSE_readNCount (lib/fse.h:222-229, lib/entropy_common.c:41-144) as batch calls on counters /
 * headers the CALLER supplies -- the same device routines FSE_buildCTable_batch / FSE_buildDTable_batch run between the histogram and the tables,
 * reachable one step at a time (a caller with its own statistics; the reference's unit vectors, programs/fuzzer.c:325-417).
 *   normalizeCount : d_counts + b*countStride holds count[0 .. maxSymbolValues[b]] (countStride, normStride >= 256 elements), d_totals[b] their sum;
 *                    d_norms + b*normStride receives normalizedCounter[0 .. maxSymbolValues[b]]; d_results[b] = tableLog used (0 = default 11) or error.
 *   writeNCount    : d_headers + b*headerStride receives at most headerCapacity bytes; d_results[b] = header size, or dstSize_tooSmall / GENERIC as
 *                    the reference (no byte is written for a failed block).
 *   readNCount     : d_maxSymbolValues[b] in = the alphabet limit (< normStride), out = last symbol described; d_tableLogs[b] out;
 *                    d_results[b] = bytes read or error (maxSymbolValue_tooSmall, tableLog_tooLarge, corruption_detected). */
FSEHIP_API int FSEHIP_FSE_normalizeCount_batch(short* d_norms, size_t normStride, unsigned tableLog, const unsigned* d_counts, size_t countStride,
                                               const size_t* d_totals, const unsigned* d_maxSymbolValues, size_t nBlocks, size_t* d_results, void* stream);
FSEHIP_API int FSEHIP_FSE_writeNCount_batch(void* d_headers, size_t headerStride, size_t headerCapacity, const short* d_norms, size_t normStride,
                                            const unsigned* d_maxSymbolValues, unsigned tableLog, size_t nBlocks, size_t* d_results, void* stream);
FSEHIP_API int FSEHIP_FSE_readNCount_batch(short* d_norms, size_t normStride, unsigned* d_maxSymbolValues, unsigned* d_tableLogs,
                                           const void* d_headers, size_t headerStride, const size_t* d_headerSizes, size_t uniformHeaderSize,
                                           size_t nBlocks, size_t* d_results, void* stream);
/*   buildCTable_fromNorm / buildDTable_fromNorm : FSE_buildCTable (lib/fse.h:162, lib/fse_compress.c:66-177) and FSE_buildDTable (lib/fse.h:240,
 *                    lib/fse_decompress.c:71-126) on normalised counters the CALLER supplies -- d_norms + b*normStride holds
 *                    normalizedCounter[0 .. d_maxSymbolValues[b]] (normStride >= 256), one tableLog (2, 4 .. 12) per call; tables in the reference's
 *                    layouts (ctableStrideU32 >= FSE_CTABLE_SIZE_U32(tableLog, 255), dtableStrideU32 >= FSE_DTABLE_SIZE_U32(tableLog));
 *                    d_results[b] = 0 or an error (see the single calls above for what is refused).  The DTable form needs the workspace of
 *                    FSEHIP_FSE_buildDTable_fromNorm_batch_workspaceSize(nBlocks, tableLog). */
FSEHIP_API int FSEHIP_FSE_buildCTable_fromNorm_batch(FSEHIP_FSE_CTable* d_ctables, size_t ctableStrideU32, const short* d_norms, size_t normStride,
                                                     const unsigned* d_maxSymbolValues, unsigned tableLog, size_t nBlocks, size_t* d_results, void* stream);
FSEHIP_API size_t FSEHIP_FSE_buildDTable_fromNorm_batch_workspaceSize(size_t nBlocks, unsigned tableLog);
FSEHIP_API int FSEHIP_FSE_buildDTable_fromNorm_batch(FSEHIP_FSE_DTable* d_dtables, size_t dtableStrideU32, const short* d_norms, size_t normStride,
                                                     const unsigned* d_maxSymbolValues, unsigned tableLog, size_t nBlocks, size_t* d_results,
                                                     void* d_workspace, size_t workspaceBytes, void* stream);

/* ---- Packed (variable-length) batches.  The batched compressors write fixed-stride slots like the reference bench's buffers
 * (programs/bench.c:514-516); what the reference's container stores (programs/fileio.c:343-400) and what is worth moving between GPUs
 * or to the host is every block at its real size.  FSEHIP_compact_batch turns slots + results into records back to back:
 *   record b = the compressed bytes (d_results[b] > 1) | the block itself, srcSize bytes (d_results[b] == 0: programs/bench.c:393-396) |
 *              its first byte (d_results[b] == 1: :397-400) | nothing (d_results[b] an error code),
 * d_offsets[b] = where record b starts, d_offsets[nBlocks] = the packed size (nBlocks + 1 entries).  A device exclusive scan and one
 * coalesced copy; if the packed size exceeds packedCapacity the records that do not fit are not written and d_offsets[nBlocks] tells.
 * d_results must be what the call that filled d_slots returned: a value above slotStride (it cannot have come from that call) yields no record.
 * FSEHIP_compact_batch_bound(nBlocks, blockSize) = nBlocks * blockSize always suffices for blocks of at most blockSize bytes.
 * The decoders of a packed batch read the records where they lie and tell the three kinds apart by size, as HUF_decompress itself does
 * (lib/huf_decompress.c:1063-1066): a record as long as the block is the block, a record of one byte that byte repeated, anything else
 * goes through FSE_decompress / HUF_decompress.  d_origSizes / d_dstSizes: the regenerated size of every block. */
FSEHIP_API size_t FSEHIP_compact_batch_workspaceSize(size_t nBlocks);
FSEHIP_API size_t FSEHIP_compact_batch_bound(size_t nBlocks, size_t blockSize);
FSEHIP_API int FSEHIP_compact_batch(void* d_packed, size_t packedCapacity, uint64_t* d_offsets, const void* d_slots, size_t slotStride, const size_t* d_results,
                                    const void* d_src, size_t srcStride, const size_t* d_srcSizes, size_t uniformSrcSize, size_t nBlocks,
                                    void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_FSE_decompress_packed_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results,
                                                  const void* d_packed, const uint64_t* d_offsets, const size_t* d_origSizes, size_t uniformOrigSize,
                                                  unsigned maxLog, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_HUF_decompress_packed_batch(void* d_dst, size_t dstStride, const size_t* d_dstSizes, size_t uniformDstSize, size_t* d_results,
                                                  const void* d_packed, const uint64_t* d_offsets, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream);

/* Workload generator of the reference's benchmark (programs/probaGenerator.c:70-74,95-126), on the
 * device: block b = generate(blockSize bytes, table, seed = firstSeed + b).  h_table4096 is the
 * HOST 4096-entry symbol table built by FSEHIP_probagen_table(); it is consumed before the call returns (the
 * call is asynchronous on `stream` like the others). */
FSEHIP_API void FSEHIP_probagen_table(uint8_t table4096[4096], double p);
FSEHIP_API int FSEHIP_probagen_batch(void* d_dst, size_t dstStride, size_t blockSize, size_t nBlocks,
                                     const uint8_t h_table4096[4096], uint32_t firstSeed, void* stream);
/* same with seed = firstSeed + b * seedStep: lets a caller interleave several distributions in one corpus (BASELINE config 5:
 * block g of the corpus = distribution g mod 3, seed g + 1 -> three calls with dstStride = 3 blocks and seedStep = 3) */
FSEHIP_API int FSEHIP_probagen_batch_ex(void* d_dst, size_t dstStride, size_t blockSize, size_t nBlocks,
                                        const uint8_t h_table4096[4096], uint32_t firstSeed, uint32_t seedStep, void* stream);

/* ---- .fse frames on HOST buffers: the container written / read by the reference's command-line tool
 * (programs/fileio.c:266-285 format, FIO_compressFilename :286-432, FIO_decompressFilename :462-626) around blocks of
 * 1 KB << blockSizeId (id 0..6, the tool's default is 5 = 32 KB).  codec 0 = FSE_compress blocks (magic 0x183E2309),
 * 1 = HUF_compress blocks (magic 0x183E3309); blocks the codec declines are stored raw, single-byte blocks as RLE, and
 * the frame ends with 22 bits of XXH32 over the content, exactly as the tool writes them.  All blocks of a frame are
 * coded by one batched device call.  Returns the frame size / the regenerated size, or an error code (bad magic or
 * block-size id: GENERIC; truncated frame: srcSize_wrong; checksum mismatch: corruption_detected; a block decoder's
 * own code otherwise).  The zlibh mode of the tool is not supported. */
FSEHIP_API size_t FSEHIP_frame_compressBound(size_t srcSize, unsigned blockSizeId);
FSEHIP_API size_t FSEHIP_frame_compress(void* dst, size_t dstCapacity, const void* src, size_t srcSize, unsigned blockSizeId, int codec);
FSEHIP_API size_t FSEHIP_frame_decompress(void* dst, size_t dstCapacity, const void* src, size_t srcSize);
/* Many frames per call (no counterpart in the tool, which walks its files one by one: programs/fileio.c:286-432 per file).  Frame i
 * is coded from srcs[i] / srcSizes[i] into dsts[i] / dstCapacities[i] exactly as the single-frame call would code it -- same bytes,
 * same result, in results[i] -- by a pool of nThreads host threads (0: half the host's hardware threads, at most 4; never more than
 * nFrames), each with a device stream and a scratch arena of its own: one frame is bound by one host thread's XXH32 and its copies,
 * many frames are not.  The helper threads are persistent: created at the first such call, they keep their streams and arenas between calls
 * (no hipMalloc / hipFree per call) and sit idle on a condition variable otherwise; FSEHIP_releaseScratch() makes the idle ones give their arenas
 * back.  One batch call uses them at a time -- a second caller arriving meanwhile runs on threads of its own.  All pointers are HOST pointers.  Returns 0, or an error code when the call itself cannot run (null arrays,
 * no device); a frame's own failure is in its results entry only. */
FSEHIP_API size_t FSEHIP_frame_compress_batch(void* const* dsts, const size_t* dstCapacities, const void* const* srcs, const size_t* srcSizes,
                                              size_t* results, size_t nFrames, unsigned blockSizeId, int codec, unsigned nThreads);
FSEHIP_API size_t FSEHIP_frame_decompress_batch(void* const* dsts, const size_t* dstCapacities, const void* const* srcs, const size_t* srcSizes,
                                                size_t* results, size_t nFrames, unsigned nThreads);

/* ---- .fse frames on DEVICE buffers (frame_dev.hip): the same container (programs/fileio.c:266-285), written and read without the bytes
 * leaving the device.  Like every batched call: kernel launches on `stream` and nothing else (no synchronisation, no read-back, no
 * allocation, no memset / copy nodes), so the calls can be captured into a HIP graph; all pointers are DEVICE pointers, workspaces
 * 256-byte aligned; the return value is a hipError_t (0 = launched; hipErrorInvalidValue: blockSizeId > 6, codec not 0 / 1, workspace
 * misaligned or too small), a frame's own outcome is its d_results entry.
 *
 *   FSEHIP_XXH32_batch   d_hashes[i] = XXH32(d_data[d_offsets[i] .. d_offsets[i+1]), seed) -- the checksum the tool streams over the
 *                        content (fileio.c:303,339,408), here as a call of its own (per-block or per-tensor checksums on the device).
 *                        nItems + 1 offsets; items start at any alignment; one lane quad per item (the hash is four serial chains: the
 *                        parallel axis is the items).  Reads exactly the items' bytes.
 *
 *   FSEHIP_frame_blockCount   host arithmetic: blocks of a content of srcSize bytes, ceil(srcSize / (1 KB << blockSizeId)); id > 6: GENERIC.
 *
 *   FSEHIP_frame_compress_dbatch   (FIO_compressFilename, fileio.c:286-432, over many contents)
 *     content i = d_src[d_srcOffsets[i] .. d_srcOffsets[i+1])  (contents back to back), frame i is written at d_dst + d_dstOffsets[i],
 *     its capacity is d_dstOffsets[i+1] - d_dstOffsets[i] (nFrames + 1 entries each).  d_results[i] = what FSEHIP_frame_compress returns
 *     for that content and capacity, byte for byte the same frame: dstSize_tooSmall below FSEHIP_frame_compressBound, a block coder's
 *     error otherwise.  maxTotalBlocks is the caller's promise >= sum of FSEHIP_frame_blockCount(size_i): it sizes the launches, so that no
 *     size is read back.  A frame whose blocks do not all lie inside the promise gets GENERIC; the others are unaffected.  All blocks of all
 *     frames go through ONE call of the one-shot coder.
 *     Memory: reads the contents; writes exactly the bytes of every frame that succeeds -- nothing into the slot of a frame that fails,
 *     nothing behind a frame's last byte.
 *
 *   FSEHIP_frame_packedBound   host arithmetic (works without a device): totalSrcBytes + 8 * nFrames + 5 * totalBlocks + nFrames *
 *     ((1 << slotAlignLog) - 1), a dstCapacity of the packed writer at which no frame fails for lack of room (every frame at its
 *     FSEHIP_frame_compressBound plus its padding).  slotAlignLog > 12: GENERIC.
 *
 *   FSEHIP_frame_compress_packed_dbatch   the writer above with the frames BACK TO BACK at their real sizes: d_dstOffsets is an OUTPUT
 *     (nFrames + 1 entries).  size_i = what FSEHIP_frame_compress returns for content i at a capacity of FSEHIP_frame_compressBound, byte for
 *     byte the same frame; where that is an error (a block coder's, passed on as it is; GENERIC for a frame whose blocks do not all lie
 *     inside maxTotalBlocks) d_results[i] is that error and the frame takes 0 bytes.  With U[i] = sum over j < i of roundup(size_j,
 *     1 << slotAlignLog):  d_dstOffsets[i] = min(U[i], dstCapacity) -- the clamping rule of FSEHIP_frame_plan_dbatch; a frame that does not
 *     fit still counts with its size, so d_dstOffsets[nFrames] = min(packed total, dstCapacity).  Frame i is written at d_dst +
 *     d_dstOffsets[i] and d_results[i] = size_i if its slot d_dstOffsets[i+1] - d_dstOffsets[i] holds size_i bytes; otherwise d_results[i] =
 *     dstSize_tooSmall and no byte of it is written.  d_dst == NULL with dstCapacity = UINT64_MAX is the sizing query: offsets and results
 *     are produced and nothing else is written -- the contents are still CODED (a frame's size is not known otherwise), so the query costs
 *     what the call costs less the copy of the records.  nFrames == 0 writes d_dstOffsets[0] = 0; maxTotalBlocks == 0 is legal (empty
 *     contents still give their 8-byte frames); slotAlignLog > 12: hipErrorInvalidValue, like the other bad arguments, and nothing written.
 *     Memory: reads the contents; writes exactly the bytes of the frames that succeed -- not the padding between frames, nothing into the
 *     slot of a frame that fails, nothing at or behind d_dst + dstCapacity.
 *     The offsets are directly usable as d_frameOffsets of FSEHIP_frame_decompress_packed_dbatch (and of the other readers), for every
 *     slotAlignLog: a reader's header walk stops at the frame's end mark, so the unwritten padding behind a frame is never interpreted.
 *     Writer and reader thus chain on one stream, or in one graph, without a byte or a size leaving the device.
 *
 *   FSEHIP_frame_compress_packed_mixed_dbatch   the packed writer with a codec PER FRAME (the magic is per frame, and the readers take FSE and
 *     Huff0 frames mixed in one call).  d_codecs has nFrames bytes, 0 = FSE, 1 = Huff0.  Everything not named here is the packed writer's
 *     contract: launches on `stream` only, capturable, no size leaves the device; dstCapacity, maxTotalBlocks, slotAlignLog, the sizing query
 *     with d_dst == NULL, dstSize_tooSmall for a frame the capacity cuts short, nothing written outside the frames' bytes, argument errors
 *     (also: a policy that is neither of the two, a null d_codecs) decided before any device call.
 *     policy FSEHIP_CODECS_GIVEN: d_codecs is an INPUT.  Frame i is byte for byte FSEHIP_frame_compress(content i, blockSizeId, d_codecs[i]);
 *     each block is coded by its frame's coder only.  A d_codecs[i] above 1 gives frame i the result GENERIC: it takes no room, nothing of it
 *     is written, its neighbours are unaffected.  tolerancePermille is ignored.  With all codecs 0 (or all 1) d_dst, d_dstOffsets and d_results
 *     are the packed writer's with codec 0 (or 1), bit for bit.
 *     policy FSEHIP_CODECS_CHOOSE: d_codecs is an OUTPUT, written in full (nFrames bytes, no other) in the sizing query too.  Every block goes
 *     through BOTH one-shot coders -- a trial, not an estimate: with F and H what FSEHIP_frame_compress returns for content i at
 *     FSEHIP_frame_compressBound with codec 0 and 1, the frame is Huff0 iff H * 1000 <= F * (1000 + tolerancePermille) in 64-bit integers
 *     ("Huff0 unless it costs more than the tolerance over FSE").  If exactly one of F and H is an error the other codec is taken; if both
 *     are (a frame beyond the block promise), the codec is 0 and the result F's.  The choice does not depend on dstCapacity.  The frame
 *     written is byte for byte the GIVEN frame of the chosen codec.  tolerancePermille > 1000: hipErrorInvalidValue.  A steady workload calls
 *     CHOOSE once and GIVEN afterwards with the codecs it got back.
 *   FSEHIP_frame_mixedWorkspaceBound   host arithmetic (works without a device): the workspace of the call above.  With P(c) =
 *     FSEHIP_frame_compress_packed_dbatch_workspaceSize(nFrames, maxTotalBlocks, blockSizeId, c), R(x) = x rounded up to 256 and B =
 *     maxTotalBlocks -- GIVEN: max(P(0), P(1)) + 3 * R(8 * B) (the coders share one coder workspace serially; two per-block size arrays, one
 *     more per-block result array).  CHOOSE: max(P(0), P(1)) + R(8 * B) + R(8 * (B + 1)) + R(B * slot), slot = FSE_compressBound(block size)
 *     rounded up to 16 (the second coder's results, record positions and slots) -- less than P(0) + P(1).  A bad blockSizeId or policy: GENERIC.
 *
 *   FSEHIP_frame_decompress_dbatch   (FIO_decompressFilename, fileio.c:462-626, over many frames)
 *     frame i = d_frames[d_frameOffsets[i] .. d_frameOffsets[i+1]), regenerated at d_dst + d_dstOffsets[i], capacity d_dstOffsets[i+1] -
 *     d_dstOffsets[i].  Frames describe themselves: codecs and block-size ids may differ inside one call.  d_results[i] = what
 *     FSEHIP_frame_decompress(dst, capacity_i, frame_i, size_i) returns, with the same regenerated bytes, for intact and damaged frames
 *     alike -- blocks in order (per block dstSize_tooSmall before its decoding error), then the structural error of the header walk, then
 *     the checksum.  maxTotalBlocks >= the number of blocks in all frames (a frame of F bytes has at most (F - 8) / 2); a frame beyond the
 *     promise gets GENERIC and writes nothing.
 *     Memory: a frame's result depends on nothing outside its [offset, next offset) -- the header walk reads nothing else; the block
 *     decoders fetch aligned 64-byte pieces and may touch, without using them, bytes of the neighbouring frames inside d_frames.  Nothing is
 *     written outside a frame's destination slot; inside the slot, bytes behind the regenerated size are undefined.
 *
 * Frames of UNKNOWN size (a file, another rank, the reference's tool): a frame does not store its content size (fileio.c:266-285), so the
 * caller of the reader above has neither d_dstOffsets nor a promise better than (F - 8) / 2 blocks.  What a frame does say without a
 * block being decoded is what its block headers ANNOUNCE:
 *
 *   FSEHIP_FrameInfo   contentBound = the sum of the announced regenerated sizes of the blocks the header walk passes (it stops at the end
 *                      mark or at the first structural problem), nBlocks = their number.  The bound is a CAPACITY, not a size:
 *                      FSEHIP_frame_decompress with capacity contentBound returns what it returns with any larger capacity, but a
 *                      compressed FSE block may regenerate less than it announces (then the content is shorter than the bound), and a block
 *                      decoder may still report dstSize_tooSmall of its own.  For every frame the tool or this library writes the bound
 *                      equals the content size.  status = 0 or the FSEHIP_ErrorCode of what the reader decides without decoding a block:
 *                      GENERIC (bad magic or block-size id; contentBound = nBlocks = 0), srcSize_wrong (shorter than 8 bytes, or
 *                      truncated), corruption_detected (a block announces more than the block size) -- contentBound and nBlocks then
 *                      cover the blocks in front of that point.  checksum22 = the end mark's 22 bits (0 without one), codec and
 *                      blockSizeId as the first five bytes give them (0 where status is GENERIC or the frame is shorter than 8 bytes).
 *
 *   FSEHIP_frame_inspect   HOST pointer, host arithmetic only (works without a device): fills *info (may be NULL) and returns contentBound,
 *                      or (size_t)-status.
 *
 *   FSEHIP_frame_plan_dbatch   the same walk for every frame of a device batch, one lane per frame, and two scans.  With
 *                      U[i] = sum over j < i of roundup(contentBound_j, 1 << slotAlignLog):  d_dstOffsets[i] = min(U[i], dstCapacity) and
 *                      d_blockFirst[i] = the blocks of the frames before i (nFrames + 1 entries each; d_blockFirst[nFrames] is the exact
 *                      maxTotalBlocks of the reader), d_infos[i] = frame i's record.  d_blockFirst and d_infos may be NULL.  dstCapacity =
 *                      UINT64_MAX is the sizing query: d_dstOffsets[nFrames] is then the capacity all frames need.  slotAlignLog > 12:
 *                      hipErrorInvalidValue.  nFrames == 0 writes entry 0 (= 0) of both arrays.  Reads nothing outside a frame's
 *                      [offset, next offset).
 *
 *   FSEHIP_frame_decompress_packed_dbatch   the plan followed by FSEHIP_frame_decompress_dbatch's decoding in one call (no frame is walked a
 *                      third time): d_dstOffsets is an OUTPUT (nFrames + 1 entries, as the plan writes them for dstCapacity and
 *                      slotAlignLog), d_results[i] = what FSEHIP_frame_decompress(d_dst + off[i], off[i+1] - off[i], frame_i, size_i)
 *                      returns, with the same bytes.  A frame that straddles dstCapacity therefore gets a short (or empty) slot and the host
 *                      call's verdict for that slot; nothing is written at or behind d_dst + dstCapacity.  maxTotalBlocks is the same
 *                      promise as above -- exact from a sizing query's d_blockFirst[nFrames], or any upper bound; a frame beyond it gets
 *                      GENERIC and writes nothing.  Memory contract of the reader above.
 */
typedef struct {
    uint64_t contentBound;
    uint64_t nBlocks;
    uint32_t status;
    uint32_t checksum22;
    uint8_t  codec;
    uint8_t  blockSizeId;
    uint8_t  reserved[6];   /* zero */
} FSEHIP_FrameInfo;
FSEHIP_API int FSEHIP_XXH32_batch(uint32_t* d_hashes, const void* d_data, const uint64_t* d_offsets, size_t nItems, uint32_t seed, void* stream);
FSEHIP_API size_t FSEHIP_frame_blockCount(size_t srcSize, unsigned blockSizeId);
FSEHIP_API size_t FSEHIP_frame_compress_dbatch_workspaceSize(size_t nFrames, size_t maxTotalBlocks, unsigned blockSizeId, int codec);
FSEHIP_API int FSEHIP_frame_compress_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_src, const uint64_t* d_srcOffsets,
                                            size_t nFrames, size_t maxTotalBlocks, unsigned blockSizeId, int codec,
                                            void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API size_t FSEHIP_frame_packedBound(size_t totalSrcBytes, size_t nFrames, size_t totalBlocks, unsigned slotAlignLog);
FSEHIP_API size_t FSEHIP_frame_compress_packed_dbatch_workspaceSize(size_t nFrames, size_t maxTotalBlocks, unsigned blockSizeId, int codec);
FSEHIP_API int FSEHIP_frame_compress_packed_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_dstOffsets, size_t* d_results,
                                                   const void* d_src, const uint64_t* d_srcOffsets, size_t nFrames, size_t maxTotalBlocks,
                                                   unsigned blockSizeId, int codec, unsigned slotAlignLog,
                                                   void* d_workspace, size_t workspaceBytes, void* stream);
#define FSEHIP_CODECS_GIVEN  0   /* d_codecs is an INPUT: nFrames bytes, 0 = FSE, 1 = Huff0 */
#define FSEHIP_CODECS_CHOOSE 1   /* d_codecs is an OUTPUT: the codec chosen per frame */
FSEHIP_API size_t FSEHIP_frame_mixedWorkspaceBound(size_t nFrames, size_t maxTotalBlocks, unsigned blockSizeId, int policy);
FSEHIP_API int FSEHIP_frame_compress_packed_mixed_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_dstOffsets, size_t* d_results,
                                                         const void* d_src, const uint64_t* d_srcOffsets, size_t nFrames, size_t maxTotalBlocks,
                                                         unsigned blockSizeId, uint8_t* d_codecs, int policy, unsigned tolerancePermille,
                                                         unsigned slotAlignLog, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API size_t FSEHIP_frame_decompress_dbatch_workspaceSize(size_t nFrames, size_t maxTotalBlocks);
FSEHIP_API int FSEHIP_frame_decompress_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets,
                                              size_t nFrames, size_t maxTotalBlocks, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API size_t FSEHIP_frame_inspect(FSEHIP_FrameInfo* info, const void* src, size_t srcSize);
FSEHIP_API size_t FSEHIP_frame_plan_dbatch_workspaceSize(size_t nFrames);
FSEHIP_API int FSEHIP_frame_plan_dbatch(uint64_t* d_dstOffsets, uint64_t* d_blockFirst, FSEHIP_FrameInfo* d_infos, const void* d_frames, const uint64_t* d_frameOffsets,
                                        size_t nFrames, uint64_t dstCapacity, unsigned slotAlignLog, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API size_t FSEHIP_frame_decompress_packed_dbatch_workspaceSize(size_t nFrames, size_t maxTotalBlocks);
FSEHIP_API int FSEHIP_frame_decompress_packed_dbatch(void* d_dst, size_t dstCapacity, uint64_t* d_dstOffsets, size_t* d_results, const void* d_frames,
                                                     const uint64_t* d_frameOffsets, size_t nFrames, size_t maxTotalBlocks, unsigned slotAlignLog,
                                                     void* d_workspace, size_t workspaceBytes, void* stream);

/* ---- Byte planes of tensors (planes.hip): tensors of 2-, 4- and 8-byte elements through the frame calls above, ONE FRAME PER BYTE PLANE.
 * An order-0 coder over the raw bytes of such a tensor sees the bytes of an element (sign and exponent, mantissa) mixed in one histogram;
 * plane by plane each byte position gets a table of its own, and a plane that does not compress falls through the frame's raw-block path.
 * No bitstream, header or frame byte differs: every frame these calls write is a frame of the container above, read by the reference's tool.
 * Like the device frame calls: kernel launches on `stream` and nothing else, all pointers DEVICE pointers, no size leaves the device, the
 * return value is a hipError_t.  hipErrorInvalidValue -- elemBytes not 1 / 2 / 4 / 8, a null array, 2^31 planes or more, a capacity whose
 * launch (capacity / 32 KB + nTensors workgroups) reaches 2^24 workgroups -- is decided before any device call (it answers on a host without
 * a device) and nothing is written.
 *
 *   The layout.  Tensor i is the byte range [S[i], S[i+1]) of a flat buffer, the tensors back to back (nTensors + 1 offsets, any sizes, any
 *     alignments).  With E = elemBytes, PLANE p (p < E) of a tensor of n bytes holds its bytes at the tensor-relative positions k with
 *     k mod E == p, in order -- on a little-endian host byte p of every element: size_p = ceil((n - p) / E) for n > p, else 0.  n need not be
 *     a multiple of E: the bytes of the last, partial element go to the first n mod E planes; there is no error case for a size.  The planes
 *     of tensor i lie back to back, in plane order, where the tensor lies: P[i * E + p] = S[i] + size_0 + .. + size_(p-1), and
 *     P[nTensors * E] = S[nTensors].  The planes buffer has the size of the source, and P (nTensors * E + 1 entries) is directly the
 *     d_srcOffsets of FSEHIP_frame_compress_packed_dbatch with nFrames = nTensors * E.
 *
 *   FSEHIP_planes_split_dbatch   d_src -> d_planes, P into d_planeOffsets, per tensor its size into d_tensorResults.  `capacity` is the byte size
 *     of d_src and of d_planes: it sizes the launch, no offset is read back.  A tensor with S[i+1] > capacity is REFUSED: its result is GENERIC,
 *     nothing of it is read or written, and every entry of d_planeOffsets from its first plane on equals its start S[i] -- offsets are
 *     monotone, so every later tensor is refused too, and all those planes are empty contents to the frame writer.
 *     Memory: reads the accepted tensors' bytes; writes exactly their plane bytes, nothing else of d_planes.  d_planes must not overlap d_src.
 *     elemBytes == 1: offsets and results only, no kernel over the data -- plane 0 of a tensor is the tensor; d_planes may be NULL.
 *
 *   FSEHIP_planes_merge_dbatch   the inverse.  Tensor i is rebuilt at d_dst + d_dstOffsets[i], its slot d_dstOffsets[i+1] - d_dstOffsets[i]
 *     (nTensors + 1 entries, an INPUT); its plane p is d_planeSizes[i * E + p] bytes at d_planes + d_planeOffsets[i * E + p] -- exactly what
 *     FSEHIP_frame_decompress_packed_dbatch leaves in its d_dstOffsets and d_results (error codes pass through).  d_results[i], in this order:
 *     GENERIC if the slot ends behind dstCapacity; the first error among its E plane sizes, in plane order; corruption_detected if the sizes
 *     are not the size_p of n = their sum; dstSize_tooSmall if n exceeds the slot; otherwise n.
 *     Memory: a tensor whose result is n gets exactly n bytes written, every other tensor none; reads the planes of the good tensors.
 *
 *   Both data kernels read n bytes and write n bytes, and need no workspace and no scan: the flat byte axis is cut into tiles of T = 32 KB,
 *     ceil(capacity / T) + nTensors workgroups are launched, and workgroup w takes tile t = w - i of the tensor i that is the largest with
 *     floor(S[i] / T) + i <= w (a binary search over the offsets) -- every (tile, tensor) intersection exactly once, however many small or
 *     empty tensors a tile holds.  An element belongs to the tile its first byte lies in.
 *
 *   FSEHIP_planes_blockBound   host arithmetic (works without a device): ceil(totalBytes / blockSize) + nTensors * elemBytes, a sufficient
 *     maxTotalBlocks for the planes of nTensors tensors of totalBytes bytes in all (every plane may end in a partial block).  blockSizeId > 6
 *     or a bad elemBytes: GENERIC.
 *
 *   FSEHIP_tensor_compress_dbatch   FSEHIP_planes_split_dbatch, then FSEHIP_frame_compress_packed_dbatch over the planes: frame i * E + p is
 *     byte for byte FSEHIP_frame_compress of plane p of tensor i.  d_frameOffsets (nTensors * E + 1 entries) and d_frameResults (nTensors * E)
 *     are the packed writer's d_dstOffsets and d_results, with its rules for dstCapacity, maxTotalBlocks and slotAlignLog; d_tensorResults are
 *     the split's.  A refused tensor yields E empty frames of eight bytes and GENERIC in its tensor result.  d_planes (capacity bytes) and
 *     d_planeOffsets (nTensors * E + 1 entries) are scratch, left as the split leaves them.  With elemBytes == 1 the writer reads d_src itself
 *     and d_planes may be NULL.  d_workspace is the PACKED WRITER'S OWN: size it with
 *     FSEHIP_frame_compress_packed_dbatch_workspaceSize(nTensors * elemBytes, maxTotalBlocks, blockSizeId, codec).
 *     A call refused for one of the argument errors listed here or at the packed writer (blockSizeId, codec, slotAlignLog, a misaligned or
 *     too small workspace, 2^31 blocks) has written nothing; that covers those checks only -- for any other error the writer returns, the
 *     split has already run (d_planes, d_planeOffsets and d_tensorResults are written).
 *
 *   FSEHIP_tensor_decompress_dbatch   FSEHIP_frame_decompress_packed_dbatch with slotAlignLog 0 into d_planes (planesCapacity bytes;
 *     d_planeOffsets, nTensors * E + 1 entries, and d_planeResults, nTensors * E, are its outputs), then FSEHIP_planes_merge_dbatch into the
 *     slots d_dstOffsets (an INPUT).  A tensor one of whose frames fails has that frame's error as its result and its slot is not written.
 *     d_workspace is the packed reader's: FSEHIP_frame_decompress_packed_dbatch_workspaceSize(nTensors * elemBytes, maxTotalBlocks).
 */
FSEHIP_API size_t FSEHIP_planes_blockBound(size_t totalBytes, size_t nTensors, unsigned elemBytes, unsigned blockSizeId);
FSEHIP_API int FSEHIP_planes_split_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const uint64_t* d_srcOffsets,
                                          size_t nTensors, unsigned elemBytes, uint64_t capacity, void* stream);
FSEHIP_API int FSEHIP_planes_merge_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                          const size_t* d_planeSizes, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                             const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                             size_t maxTotalBlocks, unsigned blockSizeId, int codec, unsigned slotAlignLog,
                                             void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results,
                                               const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks,
                                               void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                               void* d_workspace, size_t workspaceBytes, void* stream);

/* Tensor deltas (planes.hip): the four calls above on `tensor XOR base`, the XOR fused into the two data kernels.  For a tensor the
 * receiver already holds an earlier version of -- weights after a training step, checkpoint N + 1 next to checkpoint N, optimizer state --
 * XOR against that version zeroes every byte that did not change; the sign / exponent plane becomes almost all zeros and the order-0 coders
 * do the rest.  The frames are ordinary .fse frames (of the planes of `tensor XOR base`): nothing in them says that they hold a delta or
 * against what, and pairing them with the right base is the caller's business.
 * Semantics: those of the plain call on src XOR base, and the inverse.  Offsets, results, refusals, what is written and what is not, the
 * work mapping, and every argument rejection (decided before any device call) are the plain call's, word for word.  In addition a null
 * d_base is hipErrorInvalidValue, for every elemBytes; and so is a null d_planes with elemBytes == 1 in the split and the compress call: the
 * XOR has to be written somewhere, so the `<1>` data kernel runs and the packed writer then reads d_planes, not d_src.
 *
 *   FSEHIP_planes_split_xor_dbatch   d_base has THE LAYOUT OF d_src: the same offsets d_srcOffsets, the same capacity.  Plane p of tensor i holds
 *     the bytes k mod E == p of src_i XOR base_i.  A refused tensor is not read, and neither is its base.  d_planes overlaps neither d_src
 *     nor d_base (d_src and d_base are only read and may be anything, each other included).
 *   FSEHIP_planes_merge_xor_dbatch   d_base has THE LAYOUT OF d_dst: d_dstOffsets, dstCapacity.  A tensor whose result is n gets the n bytes
 *     merge(planes) XOR base_i; a tensor whose result is an error is neither written nor is its base read.
 *     IN PLACE: d_base == d_dst is allowed -- the resident tensors become the new ones where they lie.  Every byte of a tensor is read (as
 *     base) and written by exactly one thread, the load in front of the store, so there is nothing to order between threads.  A tensor
 *     whose result is an error leaves its slot untouched: in place, it keeps its old bytes.  ANY OTHER overlap of d_base and d_dst (a
 *     shifted one, a partial one) is the caller's error; it is not checked and the result is undefined.  d_planes overlaps neither.
 *   FSEHIP_tensor_compress_delta_dbatch    the XOR split, then FSEHIP_frame_compress_packed_dbatch over d_planes: frame i * E + p is byte for
 *     byte FSEHIP_frame_compress of plane p of tensor_i XOR base_i.  An unchanged tensor costs a few bytes per plane (RLE blocks).
 *   FSEHIP_tensor_decompress_delta_dbatch  FSEHIP_frame_decompress_packed_dbatch into d_planes, then the XOR merge against d_base; with
 *     d_base == d_dst a tensor one of whose frames is damaged keeps the base's bytes.
 *   Workspaces are the packed writer's / reader's, sized as for the plain calls: there is no *_workspaceSize of these.
 *   FSEHIP_tensor_compress_mixed_dbatch    d_base == NULL: FSEHIP_planes_split_dbatch, otherwise FSEHIP_planes_split_xor_dbatch; then
 *     FSEHIP_frame_compress_packed_mixed_dbatch over the nTensors * E planes.  d_codecs has nTensors * E entries, entry i * E + p belongs to
 *     plane p of tensor i; policy and tolerancePermille are the mixed writer's.  All other rules are those of FSEHIP_tensor_compress_dbatch /
 *     _delta_dbatch: refused tensors, elemBytes == 1 with a null d_planes in the plain form only, what has been written when a later check
 *     refuses.  The workspace is the mixed writer's: FSEHIP_frame_mixedWorkspaceBound(nTensors * E, maxTotalBlocks, blockSizeId, policy).
 *     Nothing changes on the reading side: FSEHIP_tensor_decompress_dbatch / _delta_dbatch read such frames as they read any.
 * Out of scope: a base with offsets of its own (it lies where the tensors lie); any record in the frames that they hold a delta.  The
 * subtract-and-zigzag delta is "arithmetic tensor deltas" below: every call here that takes d_base has an *_op_dbatch sibling. */
FSEHIP_API int FSEHIP_planes_split_xor_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const void* d_base,
                                              const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity, void* stream);
FSEHIP_API int FSEHIP_planes_merge_xor_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                              const size_t* d_planeSizes, const void* d_base, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_delta_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                   const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                   uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, unsigned slotAlignLog,
                                                   void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_mixed_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                   const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                   uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, uint8_t* d_codecs, int policy,
                                                   unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets,
                                                   void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_delta_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, size_t* d_results,
                                                     const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks,
                                                     void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                                     void* d_workspace, size_t workspaceBytes, void* stream);

/* Segmented planes (planes_seg.hip): the tensor calls above with ONE FRAME PER SEGMENT OF A PLANE.  A frame ends in one XXH32 over its whole
 * content -- a serial chain, about 1.5 GB/s per frame -- and the reader walks a frame's headers and settles its blocks frame by frame: a plane
 * of hundreds of MiB as one frame takes hundreds of milliseconds however idle the device is.  The frame writer codes every block independently
 * of its position, so a plane cut at multiples of the block size gives the same blocks, byte for byte, in several ordinary frames: eight
 * bytes (5 of header, 3 of end mark) per additional frame, and no chain longer than a segment.  Nothing in a frame says that it is a segment;
 * which frames make up a plane is `segFirst`, which the caller keeps beside the tensor offsets.
 * Like the calls above: launches on `stream` only, capturable, no size leaves the device, argument errors (also: a segLog outside its range,
 * 2^31 segments or more) are hipErrorInvalidValue, decided before any device call.  No *_workspaceSize of their own: the workspaces are the
 * packed writer's, the mixed writer's and the packed reader's with nFrames = nSegments.
 *
 *   The layout.  seg = 1 << segLog with 10 + blockSizeId <= segLog <= 30 (calls that take no blockSizeId: 10 <= segLog <= 30), so that a
 *     segment is a whole number of blocks.  Plane j = i * E + p of size_j bytes has cnt_j = max(1, ceil(size_j / seg)) segments, segment k
 *     its bytes [k * seg, min((k + 1) * seg, size_j)); an empty plane has one empty segment, every plane keeps at least one frame.
 *     segFirst[j] = the sum of cnt over the planes before j: nTensors * E + 1 entries, segFirst[0] = 0, segFirst[nTensors * E] = nSegments.
 *     cnt is a function of the tensor offsets S alone -- a tensor refused for capacity still counts the segments its size in S implies, all
 *     of them empty -- so the count never depends on what the device decides.  Frame q of a call is segment q - segFirst[j] of the plane j
 *     that holds it: tensor order, plane order, segment order.  Full segments are whole blocks and only the last segment of a plane may end
 *     in a partial one, so FSEHIP_planes_blockBound as it stands is still a sufficient maxTotalBlocks.
 *
 *   FSEHIP_planes_segmentFirst   host arithmetic (works without a device): fills h_segFirst (nTensors * E + 1 entries; NULL: count only) from the
 *     tensor offsets (nTensors + 1) and returns nSegments; GENERIC for a bad elemBytes or segLog or when the count reaches 2^31.  Tensor shapes
 *     are static: the caller uploads segFirst once, next to the offsets.
 *
 *   FSEHIP_planes_segments_dbatch   d_planeOffsets as the split leaves them + d_srcOffsets + d_segFirst -> d_segOffsets (nSegments + 1 entries,
 *     directly the d_srcOffsets of the packed writers with nFrames = nSegments): entry q = min(P[j] + k * seg, P[j + 1]) for segment k of plane
 *     j, the last entry P[nTensors * E].  One thread per entry, a binary search over segFirst for its plane.  Validation is local: tensor i is
 *     accepted iff segFirst[j + 1] - segFirst[j] == cnt_j for each of its E planes; otherwise d_tensorResults[i] becomes GENERIC and all its
 *     entries equal its start P[i * E] -- its segments are empty contents, frames of eight bytes, EXCEPT the last one, which the shared offset
 *     array ends at the next tensor's start: that frame holds the refused tensor's bytes of d_planes as one content (or GENERIC beyond the
 *     block promise) and is, like the others, to be discarded.  A tensor the split refused keeps its collapsed entries (P does it), and the
 *     results of accepted tensors are not touched.  A segFirst that is not non-decreasing from 0 to nSegments is the caller's error as a
 *     non-monotone offset array is: the outputs are then unspecified, but segFirst's values are never used as indices -- nothing outside the
 *     given arrays is touched.
 *
 *   FSEHIP_planes_fold_segments_dbatch   the packed reader's per-segment d_dstOffsets (nSegments + 1) and d_results (nSegments) + d_segFirst ->
 *     per plane d_planeOffsets[j] = its first segment's offset and d_planeSizes[j] (nPlanes entries each), exactly what
 *     FSEHIP_planes_merge_dbatch takes.  d_planeSizes[j], in this order: GENERIC for a plane without a segment; the first error among its
 *     segments' results, in segment order; corruption_detected unless every segment but the last holds exactly seg bytes and the last 1 .. seg
 *     (0 only as the plane's only segment); corruption_detected unless off[q + 1] == off[q] + res[q] inside the plane -- the decoded segments
 *     lie back to back, which the reader's slot alignment 0 gives whenever announced and decoded sizes agree; otherwise the sum.  One wave per
 *     plane, its lanes striding over the segments; segment ranges are clamped to nSegments.
 *
 *   FSEHIP_tensor_compress_seg_dbatch   the split (d_base == NULL) or the XOR split, the segments kernel, then the packed writer with `codec`
 *     (d_codecs == NULL) or the mixed writer with d_codecs (nSegments entries, one per segment, given or chosen), policy and
 *     tolerancePermille.  Frame q is byte for byte FSEHIP_frame_compress of its segment.  d_frameOffsets (nSegments + 1) and d_frameResults
 *     (nSegments) are the writer's; d_planes, d_planeOffsets (nTensors * E + 1) and d_segOffsets (nSegments + 1) are scratch the caller
 *     supplies.  With elemBytes == 1 a null d_planes is allowed without a base only.  The workspace is the writer's for nSegments frames.
 *     The argument checks of all steps run before the first launch; for any later error the earlier steps have run.
 *
 *   FSEHIP_tensor_decompress_seg_dbatch   FSEHIP_frame_decompress_packed_dbatch with slotAlignLog 0 into d_planes (d_segOffsets, nSegments + 1,
 *     and d_segResults, nSegments, are its outputs), the fold (d_planeOffsets and d_planeSizes, nTensors * E each, its outputs), then the merge
 *     (d_base == NULL) or the XOR merge, in place with d_base == d_dst included.  d_segFirst is an INPUT: what the sender used, or
 *     FSEHIP_planes_segmentFirst of the tensor sizes.  A tensor any of whose segments fails gets that error and its slot is not written (in
 *     place: it keeps its old bytes); frames read with another segLog than they were written with give corruption_detected. */
FSEHIP_API size_t FSEHIP_planes_segmentFirst(uint64_t* h_segFirst, const uint64_t* h_offsets, size_t nTensors, unsigned elemBytes, unsigned segLog);
FSEHIP_API int FSEHIP_planes_segments_dbatch(uint64_t* d_segOffsets, size_t* d_tensorResults, const uint64_t* d_planeOffsets, const uint64_t* d_srcOffsets,
                                             const uint64_t* d_segFirst, size_t nTensors, unsigned elemBytes, size_t nSegments, unsigned segLog, void* stream);
FSEHIP_API int FSEHIP_planes_fold_segments_dbatch(uint64_t* d_planeOffsets, size_t* d_planeSizes, const uint64_t* d_segOffsets, const size_t* d_segResults,
                                                  const uint64_t* d_segFirst, size_t nPlanes, size_t nSegments, unsigned segLog, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_seg_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                 const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                 uint64_t capacity, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks,
                                                 unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog,
                                                 void* d_planes, uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_seg_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, size_t* d_results,
                                                   const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                   const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks,
                                                   void* d_planes, uint64_t planesCapacity, uint64_t* d_segOffsets, size_t* d_segResults,
                                                   uint64_t* d_planeOffsets, size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream);

/* Windows of segmented tensors (planes_win.hip): an ELEMENT RANGE of every tensor of a segmented batch, decoding only the segments that hold it.
 * The segmented layout above leaves a large tensor as a row of independently decodable frames of seg = 1 << segLog plane bytes, and segFirst
 * says which frame holds which part; a tensor-parallel rank that wants its row shard, a loader that wants a slice, an embedding update that
 * patches a row range need 1 / share of them.  No frame byte changes and neither does a reader: every frame reader stops its header walk at
 * the end mark and looks at no byte behind it (what the padding between packed frames already relies on), so the selected frames are handed
 * to FSEHIP_frame_decompress_packed_dbatch as a batch of EXTENTS -- extent r runs from the start of selected frame r to the start of the next
 * selected frame, whole unselected frames included, and reads as the frame at its start.  The merge does not change either: for a window of
 * whole elements [a, b) every plane contributes the same plane-relative byte range [a, b); with the selected segments k0 .. k1 of a plane
 * decoded back to back at X, plane byte e lies at X + (e - k0 * seg), so the window is the merge of a tensor of b - a elements whose plane p
 * starts at X_p + (a - k0 * seg).
 * Like the calls above: launches on `stream` only, capturable, no size leaves the device, argument errors (also: 2^31 selected frames or
 * more, more selected frames than segments) are hipErrorInvalidValue, decided before any device call.  No *_workspaceSize of their own: the
 * workspace is the packed reader's, FSEHIP_frame_decompress_packed_dbatch_workspaceSize(nSelected, maxTotalBlocks).
 *
 *   Definitions.  S = d_srcOffsets (nTensors + 1 entries) is the SENDER'S tensor layout: tensor i has n_i = S[i+1] - S[i] bytes, its plane p
 *     sz = size_p(n_i) bytes, and segFirst is what the frames were written with.  `windows` holds 2 * nTensors uint64_t: (a_i, b_i) in
 *     ELEMENTS of tensor i, valid iff a_i <= b_i <= floor(n_i / E) -- the partial last element of a tensor whose size is no multiple of E is
 *     not addressable; reading everything remains FSEHIP_tensor_decompress_seg_dbatch's job.  The selected segments of EVERY plane of
 *     tensor i: none if a == b, otherwise k0 = a >> segLog .. k1 = (b - 1) >> segLog, cnt = k1 - k0 + 1 (a valid window ends inside every
 *     plane, so all E planes have these segments).  selFirst (nTensors * E + 1 entries) is the running sum of cnt in tensor, plane order,
 *     selFirst[nTensors * E] = nSelected: like segFirst a function of shapes and windows alone, computed on the host and uploaded, so that
 *     no launch size depends on the device.
 *     Tensor i is ACCEPTED iff its window is valid, each of its E planes has the count cnt in selFirst, its entries of selFirst end at or
 *     below nSelected (selFirst[i * E] <= selFirst[(i + 1) * E] <= nSelected), and each of its planes has in segFirst the count its size
 *     implies (the rule of FSEHIP_planes_segments_dbatch).  Both kernels decide this locally, from the same arrays.  Values of segFirst,
 *     selFirst and windows are never used as indices unclamped: whatever they hold, nothing outside the given arrays is touched.
 *
 *   FSEHIP_planes_windowFirst   host arithmetic (works without a device): fills h_selFirst (nTensors * E + 1 entries; NULL: count only) and
 *     *h_maxBlocks (may be NULL) and returns nSelected.  *h_maxBlocks is the EXACT block count of the selected segments, the sum of
 *     ceil(min(seg, sz - k * seg) / blockSize): the reader's block promise, which also sizes its workspace.  GENERIC for a bad elemBytes,
 *     blockSizeId > 6, a segLog outside 10 + blockSizeId .. 30, a window that is not valid, or when either count reaches 2^31.
 *
 *   FSEHIP_planes_select_window_dbatch   the full d_frameOffsets F (nSegments + 1) + S + windows + segFirst + selFirst -> d_selFrameOffsets
 *     (nSelected + 1 entries, directly the d_frameOffsets of the packed reader with nFrames = nSelected).  One thread per entry r, a binary
 *     search over selFirst for its plane j; entry r = F[q] with q = segFirst[j] + k0 + (r - selFirst[j]).  The last entry is F[q + 1] of the
 *     last selected frame, and F[0] when nothing is selected.  All entries of a refused tensor, the last entry included where it is the
 *     last tensor with entries, are F[min(segFirst[(i + 1) * E], nSegments)]: its extents are empty (srcSize_wrong to the reader) except
 *     possibly the last, which runs to the next tensor's first selected frame and is, like the others, to be discarded.  With monotone
 *     inputs the array is non-decreasing and extent r holds selected frame r at its start.
 *
 *   FSEHIP_planes_fold_window_dbatch   the packed reader's per-extent d_dstOffsets (d_selOffsets, nSelected + 1) and d_results (d_selResults,
 *     nSelected) + S + windows + segFirst + selFirst -> per plane d_planeOffsets[j] and d_planeSizes[j] (nTensors * E entries each) as the
 *     merge takes them.  d_planeSizes[j], in this order: GENERIC if the tensor is refused; 0 for an empty window; the first error among its
 *     selected segments' results, in segment order; corruption_detected unless segment k0 + t regenerated EXACTLY min(seg, sz - (k0 + t) * seg)
 *     bytes (the plane's size is known here: stricter than the fold of the full read); corruption_detected unless off[r + 1] == off[r] + res[r]
 *     between the plane's selected segments; otherwise b - a, and d_planeOffsets[j] = off[selFirst[j]] + (a - k0 * seg).  In every other
 *     case d_planeOffsets[j] = 0.  One wave per plane, its lanes striding over the plane's selected segments.
 *
 *   FSEHIP_tensor_decompress_window_dbatch   the selection (d_selFrameOffsets its output), FSEHIP_frame_decompress_packed_dbatch over the
 *     nSelected extents with slot alignment 0 into d_planes (d_selOffsets, nSelected + 1, and d_selResults, nSelected, are its outputs), the
 *     fold (d_planeOffsets and d_planeSizes, nTensors * E each), then the merge (d_base == NULL) or the XOR merge into the caller's slots
 *     d_dstOffsets (nTensors + 1 entries, an INPUT).  The slot of tensor i receives the E * (b - a) bytes tensor_i[a * E .. b * E);
 *     d_results are the merge's, its five rules unchanged (n = E * (b - a)).  d_base has THE LAYOUT OF d_dst: it holds the same window of
 *     the base.  IN PLACE (d_base == d_dst) is allowed: with d_dstOffsets[i] = T[i] + a_i * E over a resident buffer whose tensor i starts
 *     at T[i], rows [a, b) of every resident tensor are patched where they lie; nothing outside the window is written, and a tensor with
 *     an error keeps its old bytes.  planesCapacity >= nSelected << segLog is always sufficient.  maxTotalBlocks: what
 *     FSEHIP_planes_windowFirst gives, or any upper bound.  The argument checks of all steps run before the first launch. */
FSEHIP_API size_t FSEHIP_planes_windowFirst(uint64_t* h_selFirst, size_t* h_maxBlocks, const uint64_t* h_offsets, const uint64_t* h_windows, size_t nTensors,
                                            unsigned elemBytes, unsigned segLog, unsigned blockSizeId);
FSEHIP_API int FSEHIP_planes_select_window_dbatch(uint64_t* d_selFrameOffsets, const uint64_t* d_frameOffsets, const uint64_t* d_srcOffsets, const uint64_t* d_windows,
                                                  const uint64_t* d_segFirst, const uint64_t* d_selFirst, size_t nTensors, unsigned elemBytes, size_t nSegments,
                                                  size_t nSelected, unsigned segLog, void* stream);
FSEHIP_API int FSEHIP_planes_fold_window_dbatch(uint64_t* d_planeOffsets, size_t* d_planeSizes, const uint64_t* d_selOffsets, const size_t* d_selResults,
                                                const uint64_t* d_srcOffsets, const uint64_t* d_windows, const uint64_t* d_segFirst, const uint64_t* d_selFirst,
                                                size_t nTensors, unsigned elemBytes, size_t nSelected, unsigned segLog, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_window_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, size_t* d_results,
                                                      const void* d_frames, const uint64_t* d_frameOffsets, const uint64_t* d_srcOffsets, const uint64_t* d_windows,
                                                      size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog,
                                                      const uint64_t* d_selFirst, size_t nSelected, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                                                      uint64_t* d_selFrameOffsets, uint64_t* d_selOffsets, size_t* d_selResults, uint64_t* d_planeOffsets,
                                                      size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream);

/* Patching segmented tensors (planes_patch.hip): the WRITE side of the windows above.  The tensors of a segmented batch changed inside an
 * element window each; the frames of the selected segments -- those FSEHIP_planes_windowFirst picks for the windows, k0 .. k1 of every plane,
 * selFirst and nSelected as above -- are coded anew from the whole current tensors and a NEW packed object is built from the old frames and
 * the new ones.  No frame byte, no reader and no writer changes: the frame writer codes a block whatever its position and a segment is a
 * frame of its own.  Like the calls above: launches on `stream` only, capturable, no size leaves the device, argument errors are
 * hipErrorInvalidValue, decided before any device call.  No *_workspaceSize of their own: the workspace is the packed (mixed) writer's for
 * nSelected frames; the splice's scratch is FSEHIP_planes_spliceScratchBound bytes, 256-byte aligned.
 *
 *   Granularity.  The patch works on WHOLE SEGMENTS: of a selected segment ALL bytes come from d_src (XOR d_base, laid out as d_src, for an
 *     object of deltas), those outside [a, b) included.  The caller's contract is that the tensors equal the object's content outside the
 *     windows; it is not checked.  Otherwise: inside selected segments the new bytes win, everywhere else the old ones stay.
 *   The identity.  For tensors `old` and `new` that differ inside the windows only, the patch of FSEHIP_tensor_compress_seg_dbatch(old) with
 *     `new` IS FSEHIP_tensor_compress_seg_dbatch(new): offsets, results, codecs and every frame byte, for one codec, given and chosen codecs.
 *
 *   Layout of the output (out of place: d_out must not overlap d_frames, the new frames or the stage).  F = d_frameOffsets, R = d_frameResults
 *     of the object, F', R' = d_outOffsets (nSegments + 1), d_outResults (nSegments).  F'[0] = 0, F'[q + 1] = F'[q] + extent_q; extent_q is
 *     the old extent F[q + 1] - F[q] of a kept frame and the new frame's slot (the writer's, at the slotAlignLog given: pass what the object
 *     was written with) of a selected one.  Of every frame only its real bytes R'[q] are copied: padding inside an extent and every byte
 *     behind F'[nSegments] are left as they are.  R'[q] and d_outCodecs[q] are the kept frame's old ones or the writer's.
 *   Capacity.  If F'[nSegments] > outCapacity nothing is written to d_out and every tensor's result is dstSize_tooSmall; F' is still whole.
 *
 *   A tensor is patched WHOLE OR NOT AT ALL.  Tensor i keeps ALL its old frames, d_tensorResults[i] gets the error, and no other tensor is
 *     affected, by these rules in their order:
 *       1. GENERIC (the split's own result where it refused): its window is not valid (a > b or b > floor(n / E)), its slot of d_srcOffsets
 *          ends behind `capacity`, or its pair of stage offsets does not hold its sub-tensor below stageCapacity;
 *       2. GENERIC: its counts in segFirst or selFirst are not those its size and its window imply (the acceptance rule of the windows
 *          above), or a plane's range of segFirst does not lie inside nSegments;
 *       3. corruption_detected: one of its old frames q -- selected or not -- is not 0 <= F[q] <= F[q + 1] <= framesCapacity with
 *          R[q] <= F[q + 1] - F[q].  Such a frame of the refused tensor cannot be kept: it gets GENERIC in R', and no room where the extent
 *          itself is not one; its other frames are kept;
 *       4. the writer's error for one of its new frames, the first in plane and segment order (corruption_detected for a new frame that does
 *          not lie inside newCapacity as rule 3 asks of the old ones).
 *     Otherwise d_tensorResults[i] = n_i, its size in bytes.  A window (a, a) selects nothing: the tensor keeps its frames and gets n_i.
 *     Values of segFirst, selFirst, windows and both frame offset arrays are clamped or checked before they index anything.
 *
 *   FSEHIP_planes_split_window_dbatch   stages, per tensor, the planes of its sub-tensor: the bytes [k0 * seg * E, min((k0 + cnt) * seg * E, n))
 *     of it, which start at a multiple of E, so that by size_p and the plane starts of "byte planes" plane p of the sub-tensor is exactly
 *     segments k0 .. k1 of plane p of the tensor, a partial last element included.  T = d_stageOffsets (nTensors + 1) is the running sum of the
 *     sub-tensor sizes, like selFirst a function of shapes and windows alone; sub-tensor i is staged at d_stage + T[i] .. T[i + 1], and
 *     d_stagePlaneOffsets (nTensors * E + 1) and d_stageResults (the staged bytes, or GENERIC by rule 1) are what the split of "byte planes"
 *     writes, over T.  The entries of a refused tensor are all min(T[i], stageCapacity).  d_base != NULL: the planes of src XOR base.  The
 *     data path is the split's, the source displaced per tensor; elemBytes == 1 without a base stages by copy.
 *   Segment offsets.  A staged sub-tensor has exactly cnt segments per plane, so FSEHIP_planes_segments_dbatch runs unchanged with
 *     d_stagePlaneOffsets, T as d_srcOffsets and selFirst as d_segFirst: its d_segOffsets (nSelected + 1) are the writers' d_srcOffsets.  (It
 *     reports GENERIC for a tensor with an empty window, whose planes it expects one empty segment of: give it a results array of its own.)
 *   FSEHIP_planes_splice_dbatch   old object (d_frames, framesCapacity, F, R, d_codecs or NULL) + new frames (d_newFrames, newCapacity,
 *     d_newOffsets nSelected + 1, d_newResults, d_newCodecs -- given iff d_codecs is) -> the output above.  d_stageResults (nTensors, may be
 *     NULL) are the split's: an error there refuses the tensor.  One wave per plane settles rules 1 to 4, one thread per frame its extent,
 *     source, result and codec, an exclusive scan the offsets, and a gather with one workgroup per (32 KiB tile of d_out, frame) intersection
 *     copies: bytewise up to a 16-byte boundary of d_out, 16-byte pieces, a bytewise rest.  nSelected == 0 copies the object.
 *   FSEHIP_tensor_patch_window_dbatch   the window split, the segments kernel, FSEHIP_frame_compress_packed_dbatch with `codec`
 *     (d_newCodecs == NULL) or FSEHIP_frame_compress_packed_mixed_dbatch with d_newCodecs (nSelected entries, given or chosen) into
 *     d_newFrames, then the splice.  d_src, d_base, d_srcOffsets and `capacity` are as for FSEHIP_tensor_compress_seg_dbatch; d_stage
 *     (stageCapacity >= T[nTensors] bytes), d_stagePlaneOffsets, d_stageSegOffsets (nSelected + 1), d_stageResults, d_newFrames
 *     (FSEHIP_frame_packedBound of the staged bytes is sufficient), d_newOffsets and d_newResults are scratch the caller supplies.
 *     maxTotalBlocks: what FSEHIP_planes_windowFirst gives, or an upper bound; the new frames of a promise that is short fail (rule 4).  The
 *     argument checks of all steps run before the first launch. */
FSEHIP_API int FSEHIP_planes_split_window_dbatch(void* d_stage, uint64_t* d_stagePlaneOffsets, size_t* d_stageResults, const void* d_src, const void* d_base,
                                                 const uint64_t* d_srcOffsets, const uint64_t* d_windows, const uint64_t* d_stageOffsets, size_t nTensors,
                                                 unsigned elemBytes, unsigned segLog, uint64_t capacity, uint64_t stageCapacity, void* stream);
FSEHIP_API size_t FSEHIP_planes_spliceScratchBound(size_t nTensors, unsigned elemBytes, size_t nSegments);
FSEHIP_API int FSEHIP_planes_splice_dbatch(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs, size_t* d_tensorResults,
                                           const void* d_frames, uint64_t framesCapacity, const uint64_t* d_frameOffsets, const size_t* d_frameResults,
                                           const uint8_t* d_codecs, const void* d_newFrames, uint64_t newCapacity, const uint64_t* d_newOffsets,
                                           const size_t* d_newResults, const uint8_t* d_newCodecs, const size_t* d_stageResults, const uint64_t* d_srcOffsets,
                                           const uint64_t* d_windows, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog,
                                           const uint64_t* d_selFirst, size_t nSelected, void* d_scratch, size_t scratchBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_patch_window_dbatch(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs,
                                                 size_t* d_tensorResults, const void* d_frames, uint64_t framesCapacity, const uint64_t* d_frameOffsets,
                                                 const size_t* d_frameResults, const uint8_t* d_codecs, const void* d_src, const void* d_base,
                                                 const uint64_t* d_srcOffsets, uint64_t capacity, const uint64_t* d_windows, size_t nTensors, unsigned elemBytes,
                                                 const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, const uint64_t* d_selFirst, size_t nSelected,
                                                 const uint64_t* d_stageOffsets, uint64_t stageCapacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec,
                                                 uint8_t* d_newCodecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_stage,
                                                 uint64_t* d_stagePlaneOffsets, uint64_t* d_stageSegOffsets, size_t* d_stageResults, void* d_newFrames,
                                                 uint64_t newCapacity, uint64_t* d_newOffsets, size_t* d_newResults, void* d_scratch, size_t scratchBytes,
                                                 void* d_workspace, size_t workspaceBytes, void* stream);

/* Arithmetic tensor deltas (planes.hip, planes_patch.hip): SUBTRACT AND ZIGZAG beside XOR, in every call that takes d_base.  A one-ulp change
 * of a float does not flip one bit but a carry chain -- the element XORs to 1, 3, 7, 15, .. and one change in 128 reaches the sign / exponent
 * byte -- and an order-0 coder pays for every one of those patterns.  Subtracting the elements' bit patterns as integers and folding the sign
 * into the low bit turns a one-ulp change into 1 or 2 and leaves the high planes zero unless the value really moved: 11 to 19 % fewer frame
 * bytes than XOR on bf16 and fp32 weight updates.  No bitstream, header or frame byte changes: the frames are ordinary .fse frames of the
 * planes of the transformed tensor, and nothing in them records the op -- pairing frames, base AND op is the caller's business.
 *
 *   The operation (deltaOp == FSEHIP_DELTA_SUB).  For elemBytes E read element t of the tensor and b of the base as little-endian unsigned
 *     integers of E bytes, W = 8 E:
 *       forward   d = (t - b) mod 2^W,   z = ((d << 1) mod 2^W) XOR (d's top bit set ? 2^W - 1 : 0)
 *       inverse   d = (z >> 1) XOR ((z & 1) ? 2^W - 1 : 0),   t = (b + d) mod 2^W
 *     a bijection for every bit pattern, NaNs and the most negative d included; no float arithmetic anywhere.  An unchanged element gives
 *     z = 0, so an unchanged tensor still becomes RLE blocks.  The trailing n mod E bytes of a tensor whose size is no multiple of E are
 *     coded with the E == 1 form, each byte by itself.  Unlike XOR this is NOT symmetric: swapping tensor and base gives other planes.
 *     Elements are counted from the tensor's start (d_srcOffsets[i], d_dstOffsets[i]), whatever its address.
 *   deltaOp == FSEHIP_DELTA_XOR is the call without _op, byte for byte: the old names forward to these with it.
 *
 *   Every sibling takes `unsigned deltaOp` directly behind d_base and is otherwise the call it is named after, word for word on the
 *   transformed tensor: offsets, results, refusals, what is written and what is not, workspace rules, launches only, graph capture, the
 *   merge IN PLACE with d_base == d_dst (every destination byte is read and written by exactly one thread, its loads in front of its stores).
 *   deltaOp > 1 is hipErrorInvalidValue before any device call -- also where d_base is nullable (mixed, seg, window, patch) and null, which
 *   otherwise makes the op irrelevant.  SUB needs d_planes for elemBytes == 1 exactly as XOR does. */
#define FSEHIP_DELTA_XOR 0u
#define FSEHIP_DELTA_SUB 1u
FSEHIP_API int FSEHIP_planes_split_op_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const void* d_base,
                                             unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity, void* stream);
FSEHIP_API int FSEHIP_planes_merge_op_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                             const size_t* d_planeSizes, const void* d_base, unsigned deltaOp, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity,
                                             void* stream);
FSEHIP_API int FSEHIP_planes_split_window_op_dbatch(void* d_stage, uint64_t* d_stagePlaneOffsets, size_t* d_stageResults, const void* d_src, const void* d_base,
                                                    unsigned deltaOp, const uint64_t* d_srcOffsets, const uint64_t* d_windows, const uint64_t* d_stageOffsets,
                                                    size_t nTensors, unsigned elemBytes, unsigned segLog, uint64_t capacity, uint64_t stageCapacity, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_delta_op_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                      const void* d_src, const void* d_base, unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors,
                                                      unsigned elemBytes, uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, unsigned slotAlignLog,
                                                      void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_delta_op_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp,
                                                        size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                        size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                                        void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_mixed_op_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                      const void* d_src, const void* d_base, unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors,
                                                      unsigned elemBytes, uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, uint8_t* d_codecs, int policy,
                                                      unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets,
                                                      void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_seg_op_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                    const void* d_src, const void* d_base, unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors,
                                                    unsigned elemBytes, uint64_t capacity, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog,
                                                    size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille,
                                                    unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace,
                                                    size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_seg_op_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp,
                                                      size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                      const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks,
                                                      void* d_planes, uint64_t planesCapacity, uint64_t* d_segOffsets, size_t* d_segResults,
                                                      uint64_t* d_planeOffsets, size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_window_op_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp,
                                                         size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, const uint64_t* d_srcOffsets,
                                                         const uint64_t* d_windows, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments,
                                                         unsigned segLog, const uint64_t* d_selFirst, size_t nSelected, size_t maxTotalBlocks, void* d_planes,
                                                         uint64_t planesCapacity, uint64_t* d_selFrameOffsets, uint64_t* d_selOffsets, size_t* d_selResults,
                                                         uint64_t* d_planeOffsets, size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_patch_window_op_dbatch(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs,
                                                    size_t* d_tensorResults, const void* d_frames, uint64_t framesCapacity, const uint64_t* d_frameOffsets,
                                                    const size_t* d_frameResults, const uint8_t* d_codecs, const void* d_src, const void* d_base, unsigned deltaOp,
                                                    const uint64_t* d_srcOffsets, uint64_t capacity, const uint64_t* d_windows, size_t nTensors, unsigned elemBytes,
                                                    const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, const uint64_t* d_selFirst, size_t nSelected,
                                                    const uint64_t* d_stageOffsets, uint64_t stageCapacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec,
                                                    uint8_t* d_newCodecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_stage,
                                                    uint64_t* d_stagePlaneOffsets, uint64_t* d_stageSegOffsets, size_t* d_stageResults, void* d_newFrames,
                                                    uint64_t newCapacity, uint64_t* d_newOffsets, size_t* d_newResults, void* d_scratch, size_t scratchBytes,
                                                    void* d_workspace, size_t workspaceBytes, void* stream);

/* Sparse planes (planes_sparse.hip): ZERO MASK AND PACKED NON-ZEROS ahead of the frame writers.  The sign / exponent plane of a tensor delta
 * is almost all zeros, and an order-0 coder still sends every one of its n symbols through its chains (FSE, which decodes such a plane at
 * its slowest) or spends at least a bit on each (Huff0: 33 KB for a 256 KB plane that FSE codes in 1.8 KB).  A plane of n bytes of which nnz
 * are non-zero is handed to the writer as a bit mask of ceil(n / 8) bytes followed by the nnz non-zero bytes: the same order-0 information in
 * up to 8x fewer symbols, masks and values in blocks with tables of their own.  No frame byte format changes: a content is coded into an
 * ordinary .fse frame by the packed writers and read by the packed reader; nothing in a frame says which form it holds.  The transform is one
 * more layer between split and writer and between reader and merge, as the delta ops are.
 * Like the calls above: launches on `stream` only, capturable, no size leaves the device, argument errors (also: sparsePermille > 1000, 2^31
 * units or more, a null, misaligned -- 256 bytes -- or too small workspace) are hipErrorInvalidValue, decided before any device call, with
 * nothing written.
 *
 *   The transform.  A UNIT is a run of n bytes: a whole plane in the unsegmented calls, a segment of a plane in the segmented ones.  nnz = the
 *     number of its non-zero bytes, m = ceil(n / 8).
 *     Writer rule: the unit is SPARSE iff nnz * 1000 <= n * sparsePermille and m + nnz < n, in 64-bit integers (sparsePermille 0 .. 1000).
 *     Sparse content: m mask bytes, then the nnz non-zero bytes in order; bit i & 7 (LSB first) of mask byte i >> 3 is set iff byte i is
 *       non-zero, padding bits are zero; c = m + nnz < n.  Dense content: the unit itself, c = n -- the frame is byte for byte that of the
 *       calls without _sparse.  With sparsePermille 0 only units without a non-zero byte (and n >= 2) are sparse.
 *     Reader rule: the reader neither knows sparsePermille nor needs a flag -- the content size c says which form it is.  For a unit of n
 *       bytes, in this order: an error of the frame reader passes through; c == n: dense, copied; c > n: corruption_detected; otherwise
 *       sparse, and corruption_detected unless c >= m, popcount(mask) == c - m, every padding bit is zero and every value byte is non-zero
 *       (these four keep the transform a bijection).  Otherwise the result is n.  The verdict stands before any unit byte is written: a
 *       unit that fails is not written at all.
 *     THE READER NEEDS EXACT SIZES: it has to know n per unit.  In the sparse reading calls a tensor's size IS its slot,
 *       d_dstOffsets[i + 1] - d_dstOffsets[i]: the plane layout P and the segment layout follow from those sizes alone (the offsets step of
 *       the split and FSEHIP_planes_segments_dbatch over d_dstOffsets).  This is STRICTER than FSEHIP_planes_merge_dbatch, whose slots may
 *       be larger than the tensors: pass the tensors' own offsets.
 *
 *   FSEHIP_sparse_workspaceBound   host arithmetic (works without a device): the workspace of the two calls below for units inside a buffer
 *     of `capacity` bytes -- a count per work item (ceil(capacity / 32 KB) + nUnits of them), the scans' partial sums, a flag per unit; a
 *     multiple of 256.  GENERIC for 2^31 units or a capacity whose launch reaches 2^24 workgroups.
 *
 *   FSEHIP_sparse_pack_dbatch   d_units + d_unitOffsets (nUnits + 1 entries: unit u is [U[u], U[u + 1]), back to back, any alignment) ->
 *     d_contents (the contents back to back; at most `capacity` bytes in all, since c <= n) and d_contentOffsets (nUnits + 1 entries, directly
 *     the d_srcOffsets of the packed writers).  `capacity` is the byte size of d_units and of d_contents and sizes the launch.  A unit with
 *     U[u + 1] > capacity or U[u] > U[u + 1] -- collapsed offsets of a tensor refused upstream, n = 0 -- is an empty content.  d_contents must
 *     not overlap d_units.  Three passes over the work items of the ragged mapping of "byte planes" (32 KB tiles of the flat axis plus one
 *     workgroup per unit boundary, bytes dealt out by mask byte): non-zeros per item; two scans and the writer rule per unit; then every item
 *     again -- a lane takes 16 bytes a round, its position among the values is a wave prefix plus the totals of the waves in front, masks and
 *     values are staged in LDS on the 16-byte grid of their destination and stored in 16-byte pieces (fewer than 16 bytes at either end
 *     bytewise); a dense unit is copied in the same pass.  No workgroup waits on another: the scans are launches of their own.
 *
 *   FSEHIP_sparse_expand_dbatch   d_contents + d_contentOffsets + d_contentResults (the packed reader's d_dstOffsets and d_results;
 *     contentsCapacity = the size of d_contents) + the dense layout d_unitOffsets (capacity = the size of d_units) -> d_units (the dense
 *     bytes at their offsets) and d_unitResults[u] by the reader rule; a content that does not lie inside d_contents with its result is
 *     corruption_detected.  (d_unitOffsets, d_unitResults) are then exactly what the fold and the merge take.  Passes: set bits per mask
 *     tile, with zero value bytes and padding bits into a flag per unit; a scan; the verdict per unit; then the expansion of the good units --
 *     a lane takes 8 mask bytes and writes 64 unit bytes in 16-byte stores, the round's values staged in LDS.  Nothing outside the dense
 *     range of a good unit is written.
 *
 *   The composites take one more scratch buffer, d_contents (`capacity` bytes; reading: contentsCapacity, the tensors' total is sufficient)
 *     with d_contentOffsets (one entry per frame and one more; reading also d_contentResults, one per frame).  Their workspace is
 *     FSEHIP_sparse_workspaceBound(capacity, nFrames) -- reading: of min(dstCapacity, planesCapacity) -- followed by the writer's or the
 *     reader's for nFrames frames, nFrames = nTensors * E or nSegments.  FSEHIP_planes_blockBound stays a sufficient maxTotalBlocks (c <= n).
 *   FSEHIP_tensor_compress_sparse_dbatch       the split (d_base == NULL), else the split of the delta by deltaOp -> pack over the plane
 *     offsets -> FSEHIP_frame_compress_packed_dbatch with `codec` (d_codecs == NULL) or the mixed writer with d_codecs (nTensors * E entries),
 *     policy and tolerancePermille, as FSEHIP_tensor_compress_seg_dbatch takes them.  Frame j is byte for byte FSEHIP_frame_compress of the
 *     content of plane j.  With a sparsePermille under which no unit qualifies every output is that of the call without _sparse, bit for bit.
 *   FSEHIP_tensor_decompress_sparse_dbatch     the plane layout of d_dstOffsets -> the packed reader (slot alignment 0) into d_contents ->
 *     expand into d_planes (d_planeOffsets, nTensors * E + 1, the layout; d_planeResults, nTensors * E, the units' results) -> the merge,
 *     plain or by deltaOp against d_base, IN PLACE (d_base == d_dst) allowed: the expansion writes scratch only, so a tensor one of whose
 *     frames or contents is damaged keeps its old bytes.
 *   FSEHIP_tensor_compress_seg_sparse_dbatch   split -> segments -> pack over the SEGMENT offsets -> writer: a unit is a segment.
 *   FSEHIP_tensor_decompress_seg_sparse_dbatch layout and segment layout of d_dstOffsets (d_segOffsets, nSegments + 1) -> reader -> expand
 *     (d_segResults, nSegments) -> fold (d_planeOffsets, d_planeSizes) -> merge.
 *   Out of scope, and refused by the callers of these (no call combines them): windows and patches of sparse segmented objects; a threshold
 *     per unit; run-length forms. */
FSEHIP_API size_t FSEHIP_sparse_workspaceBound(uint64_t capacity, size_t nUnits);
FSEHIP_API int FSEHIP_sparse_pack_dbatch(void* d_contents, uint64_t* d_contentOffsets, const void* d_units, const uint64_t* d_unitOffsets, size_t nUnits, uint64_t capacity,
                                         unsigned sparsePermille, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_sparse_expand_dbatch(void* d_units, size_t* d_unitResults, const uint64_t* d_unitOffsets, size_t nUnits, uint64_t capacity, const void* d_contents,
                                           uint64_t contentsCapacity, const uint64_t* d_contentOffsets, const size_t* d_contentResults, void* d_workspace,
                                           size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_sparse_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                    const void* d_src, const void* d_base, unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors,
                                                    unsigned elemBytes, uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs,
                                                    int policy, unsigned tolerancePermille, unsigned slotAlignLog, unsigned sparsePermille, void* d_planes,
                                                    uint64_t* d_planeOffsets, void* d_contents, uint64_t* d_contentOffsets, void* d_workspace, size_t workspaceBytes,
                                                    void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_sparse_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp,
                                                      size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                      size_t maxTotalBlocks, void* d_contents, uint64_t contentsCapacity, uint64_t* d_contentOffsets,
                                                      size_t* d_contentResults, void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                                      void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_seg_sparse_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                        const void* d_src, const void* d_base, unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors,
                                                        unsigned elemBytes, uint64_t capacity, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog,
                                                        size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille,
                                                        unsigned slotAlignLog, unsigned sparsePermille, void* d_planes, uint64_t* d_planeOffsets, uint64_t* d_segOffsets,
                                                        void* d_contents, uint64_t* d_contentOffsets, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_seg_sparse_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp,
                                                          size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                          const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks, void* d_contents,
                                                          uint64_t contentsCapacity, uint64_t* d_contentOffsets, size_t* d_contentResults, void* d_planes,
                                                          uint64_t planesCapacity, uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets,
                                                          size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream);

/* Tensor digests and checked deltas (planes_digest.hip): A DIGEST OF THE BASE AND A GATE AGAINST A WRONG ONE.  Every reading call above
 * protects the resident tensor from a damaged frame or content; none can tell that the receiver's base is not the one the sender's delta was
 * made against (a missed step, a rank restored from an older checkpoint, two updates out of order): every frame is intact then, and the
 * in-place merge writes garbage over good weights and reports success.  The sender digests its base and sends the digests along; the receiver
 * digests what it holds, and the gate turns a mismatch into frames that every reader refuses.
 * Like the calls above: launches on `stream` only, capturable, no size leaves the device, argument errors (a null array, 2^31 tensors or
 * more, a capacity whose launch reaches 2^24 workgroups, a null, misaligned -- 256 bytes -- or too small workspace, elemBytes not 1 / 2 / 4
 * / 8, 2^31 frames, a frame count that does not fit) are hipErrorInvalidValue, decided before any device call, with nothing written.
 * THE DIGEST IS NOT CRYPTOGRAPHIC: it is built to catch accidents, not adversaries -- two bases that differ by chance collide with
 * probability about 2^-64; someone who wants a collision can make one.
 *
 *   The digest (normative).  All hashing is XXH32 (the public algorithm, FSEHIP_XXH32_batch) with the seeds S0 = 0 and S1 = 0x9E3779B1;
 *     T = 32768.  A tensor of n bytes has nt = ceil(n / T) tiles; tile k is its bytes [k T, min((k + 1) T, n)), L of them, counted from the
 *     tensor's first byte -- the digest depends on nothing but the tensor's bytes: not on its address, its alignment, its neighbours in the
 *     batch or its slot in d_srcOffsets.
 *     Lane streams: the tile is cut into 16-byte pieces q = 0 .. ceil(L / 16) - 1, of which only the last may be shorter.  Lane l (0 .. 63)
 *       owns the pieces with q mod 64 == l; its stream is those pieces concatenated in rising q (512 bytes in a full tile, possibly empty in a
 *       partial one), and h[l] = XXH32(stream_l, S0).  All 64 lanes produce a hash: an empty stream gives the XXH32 of no bytes.
 *     Tile digest: H = the 64 values h[l] as 256 bytes, little endian, in lane order; lo = XXH32(H, S0), hi = XXH32(H, S1).
 *     Tensor digest: A = the tile digests in tile order, each as lo then hi in little-endian 32-bit words, followed by the 8 bytes of n,
 *       little endian (n = 0: just those 8 zero bytes).  digest = XXH32(A, S0) | (uint64_t)XXH32(A, S1) << 32.
 *
 *   FSEHIP_tensor_digest_workspaceBound   host arithmetic (works without a device): eight bytes per work item and per tensor, for the tile
 *     digests and the sizes behind them; a multiple of 256.  GENERIC for 2^31 tensors or a capacity whose launch reaches 2^24 workgroups.
 *   FSEHIP_tensor_digest_dbatch   tensor i = [S[i], S[i + 1]) of d_src (S = d_srcOffsets, nTensors + 1 entries, any sizes and alignments;
 *     `capacity` = the size of d_src, it sizes the launch) -> d_digests[i] and d_results[i] = n_i.  Where S[i] > S[i + 1] or S[i + 1] >
 *     capacity, d_results[i] = GENERIC and d_digests[i] = 0, and nothing of that tensor is read.  nTensors == 0 is legal.  Offsets are
 *     expected non-decreasing, as everywhere: around a slot that decreases a tensor may be given tiles of another (never a byte outside
 *     [0, capacity)) and a digest that is not its own, which the gate then refuses.
 *     The work: ceil(capacity / T) + nTensors work items in the ragged mapping of "byte planes" (item w takes tile w - first(i) of the tensor
 *     the search gives it, idle where the tensor has no such tile), a WAVE per item: a round is one coalesced 1 KB read, a lane one 16-byte
 *     load (unaligned where the tensor is), the loads of eight rounds in flight ahead of the lane's four accumulators; the 64 -> 1 fold by
 *     cross-lane reads, a lane quad per seed.  No scan, no workgroup waits on another.  The top level is one more launch, a lane quad per
 *     tensor and seed over the tensor's 8 nt + 8 bytes with the chain of the frame calls' XXH32 kernel: a serial chain per tensor, 256 KB
 *     of it for one tensor of 1 GiB (about 1.5 GB/s: the known cost of a single giant tensor).
 *
 *   FSEHIP_tensor_gate_dbatch   F = d_frameOffsets (nFrames + 1 entries) -> G = d_gatedOffsets (nFrames + 1) and d_gateResults (nTensors).
 *     Tensor i owns a range of frames: with d_frameFirst == NULL the frames i E .. (i + 1) E - 1, E = elemBytes (nFrames != nTensors * E is
 *     an argument error); otherwise d_frameFirst is the segFirst of a segmented object (nTensors * E + 1 entries) and tensor i owns the
 *     frames segFirst[i E] .. segFirst[(i + 1) E] - 1 =: end_i - 1, every value clamped to nFrames.
 *     Tensor i PASSES iff d_digestResults[i] is no error and d_digests[i] == d_expected[i].
 *       pass: G[q] = F[q] for its frames; d_gateResults[i] = d_digestResults[i].
 *       fail: G[q] = F[end_i] for ALL its frames -- the start of the next tensor's first frame; d_gateResults[i] = the digest's own error,
 *             or corruption_detected for a mismatch.
 *     G[nFrames] = F[nFrames] either way, and a frame that no tensor owns keeps its offset.
 *     With a non-decreasing F, G is non-decreasing; every frame of a failed tensor is an EMPTY EXTENT, which every reader answers with
 *     srcSize_wrong, so the merge refuses the tensor and it keeps every old byte, in place too; the frame in front of a failed tensor runs
 *     on over frames that are not its own, and a reader stops at its frame's end mark (the windows rely on the same).  G therefore goes
 *     wherever d_frameOffsets goes above, with no reader changed: the delta calls and their _op siblings, the segmented calls, the window
 *     calls (G is the full array they select from), the four sparse calls.  d_gateResults tells a wrong base (corruption_detected) from
 *     damage (the readers' own results).  One thread per entry.
 *   Out of scope: cryptographic strength; a record of the digest inside the frames (the caller carries the digests beside them); gating of
 *     FSEHIP_tensor_patch_window_dbatch. */
FSEHIP_API size_t FSEHIP_tensor_digest_workspaceBound(uint64_t capacity, size_t nTensors);
FSEHIP_API int FSEHIP_tensor_digest_dbatch(uint64_t* d_digests, size_t* d_results, const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, uint64_t capacity,
                                           void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_gate_dbatch(uint64_t* d_gatedOffsets, size_t* d_gateResults, const uint64_t* d_frameOffsets, size_t nFrames, const uint64_t* d_frameFirst,
                                         unsigned elemBytes, const uint64_t* d_digests, const size_t* d_digestResults, const uint64_t* d_expected, size_t nTensors,
                                         void* stream);

/* Tensor archives (planes_archive.hip): ONE SEALED DEVICE BUFFER PER BATCH, OPENED ON THE DEVICE.  Every tensor call above leaves a piece of
 * state outside the frames -- the sizes, the frame offsets, the op of a delta, segLog, the sparse threshold, the codecs, the digests of the
 * base -- and a receiver that gets one of them wrong decodes garbage.  An archive is `head | frames`: one contiguous buffer that a sender
 * hands to a send call or writes to a file as it lies, and that a receiver opens with launches only into exactly the arrays the reading calls
 * above take.  No frame byte and no call above changes: the archive is a head in front of the frames the compress composites (or the patch
 * composite) already write.  headBytes is host arithmetic over counts alone, so the sender gives the composite `d_archive + headBytes` as its
 * destination and the frames are written in place: there is no copy pass.
 *
 *   The format (normative, little endian; a model in tests/archive_corpus.py).  headBytes is a multiple of 256.
 *     Header, 64 bytes:
 *        0  u32  magic: the bytes 'F' 'S' 'T' 'A' (FSEHIP_ARCHIVE_MAGIC as a little-endian number)
 *        4  u16  version = 1
 *        6  u16  flags: FSEHIP_ARCHIVE_CODECS | _DIGESTS | _SPARSE | _DELTA, every other bit zero; DIGESTS only with DELTA
 *        8  u8   elemBytes (1, 2, 4, 8)          9  u8  blockSizeId (0 .. 6)
 *       10  u8   segLog: 0 = unsegmented, else 10 + blockSizeId .. 30 (the rule of "segmented planes")
 *       11  u8   deltaOp: FSEHIP_DELTA_XOR / _SUB; 0 unless DELTA
 *       12  u16  sparsePermille (<= 1000); 0 unless SPARSE           14  u16  zero
 *       16  u64  nTensors        24  u64  nFrames (unsegmented: exactly nTensors * elemBytes; segmented: at least that; below 2^31)
 *       32  u64  totalBytes = the sum of the tensor sizes.  nTensors and totalBytes stay inside the launch limit of the composites:
 *                totalBytes < 2^46 and floor(totalBytes / 32768) + 1 + nTensors < 2^24
 *       40  u64  maxTotalBlocks (< 2^31): a block promise under which the packed reader accepts these frames -- what the sender gave its writer
 *       48  u64  metaBytes (< 2^31)      56  u64  framesBytes = frameOffsets[nFrames]
 *     Index, from byte 64, every array 8-byte aligned:
 *       1. the tensor sizes, nTensors x u64
 *       2. the frame offsets relative to the first frame byte, (nFrames + 1) x u64: the first is 0, they do not decrease, the last is framesBytes
 *       3. with DIGESTS: the digests of the base tensors, nTensors x u64
 *       4. with CODECS: nFrames codec bytes (0 = FSE, 1 = Huff0), zero-padded to a multiple of 8
 *       5. metaBytes opaque bytes of the caller's, zero-padded to a multiple of 8
 *       6. zeros up to headBytes - 8
 *       7. the last 8 bytes of the head: the digest of the bytes [0, headBytes - 8), as FSEHIP_tensor_digest_dbatch defines it for one tensor
 *     headBytes = 64 + the index + 8, rounded up to 256.  The frames keep their own XXH32.  NOT CRYPTOGRAPHIC, like the digest itself.
 *     segFirst is not stored: it is FSEHIP_planes_segmentFirst of the sizes, elemBytes and segLog; open recomputes it on the device and checks
 *     its total against nFrames.
 *
 *   FSEHIP_archive_headBytes   host arithmetic: headBytes for these counts, or GENERIC (an unknown flag bit, nTensors >= 2^24, nFrames or
 *     metaBytes >= 2^31).
 *   FSEHIP_archive_inspect   parses and validates the 64 header bytes at h_header64 (host memory: the one small transfer a receiver makes,
 *     as FSEHIP_frame_inspect needs for a frame) of an archive of archiveBytes bytes; fills *out with every field and headBytes; returns
 *     headBytes or: GENERIC (a null argument, a wrong magic, another version), corruption_detected (a field outside its range above, an
 *     unknown flag bit, a broken coupling, nTensors == 0 with totalBytes != 0), srcSize_wrong (archiveBytes < 64, headBytes > archiveBytes,
 *     framesBytes > archiveBytes - headBytes).  On an error *out holds the fields as far as they were read, headBytes 0.
 *   FSEHIP_archive_workspaceBound   host arithmetic, a multiple of 256, for seal and open alike; GENERIC for counts headBytes refuses or a
 *     headBytes that is no multiple of 256.
 *
 *   Both device calls: launches on `stream` only, capturable; every argument error (a null array that the flags need, d_archive not 8-byte
 *   aligned, a workspace that is null, not 256-byte aligned or below the bound, an info that inspect would refuse or whose headBytes is not
 *   FSEHIP_archive_headBytes of its counts, a capacity below headBytes) is hipErrorInvalidValue, decided before the first launch with nothing
 *   written.
 *   FSEHIP_archive_seal_dbatch   writes the head in front of the frames that lie at d_archive + info->headBytes.  The inputs are the writer's
 *     outputs as they are: d_srcOffsets (nTensors + 1), d_frameOffsets (nFrames + 1, relative to the first frame byte), d_frameResults
 *     (nFrames), d_tensorResults (nTensors); d_codecs (nFrames bytes) with CODECS, d_digests (nTensors) with DIGESTS, d_meta (metaBytes, host
 *     order of bytes) where metaBytes > 0.  info->framesBytes and info->magic / version are ignored: framesBytes is read from the device.
 *     A thread per 8-byte word of the head writes it (coalesced stores) and checks what it wrote; the verdict is the OR over all of them, and
 *     the head is accepted only if: every frame result and tensor result is a success and no frame result exceeds its extent; the frame
 *     offsets start at 0, do not decrease and end within archiveCapacity - headBytes; the source offsets do not decrease and span totalBytes;
 *     every codec byte is <= 1.  Then the digest of the head and the stamp: *d_result = headBytes + framesBytes, the archive's size -- or,
 *     on refusal, dstSize_tooSmall (only the capacity was short) or GENERIC, and THE MAGIC IS WRITTEN AS 0: an unsealed buffer can never be
 *     opened.
 *   FSEHIP_archive_open_dbatch   d_archive of archiveBytes and the info that inspect filled from its first 64 bytes -> d_srcOffsets
 *     (nTensors + 1: the exclusive scan of the sizes from 0), d_frameOffsets (nFrames + 1), with CODECS d_codecs (nFrames bytes), with
 *     DIGESTS d_digests (nTensors), for a segmented archive d_segFirst (nTensors * elemBytes + 1: the per-plane segment counts, scanned on
 *     the device) and *d_verdict = headBytes + framesBytes or corruption_detected.  The readers are then called with d_frames = d_archive +
 *     headBytes.  The host's copy of the header is not trusted: the device header must equal info word for word.  Refused are: a header that
 *     differs from info, a digest mismatch, a size above totalBytes or sizes that do not sum to it, a segment total that is not nFrames,
 *     frame offsets that break a rule of the format, a codec byte above 1, a non-zero padding byte.  ON REFUSAL EVERY d_frameOffsets ENTRY
 *     IS 0: empty extents, which every reader refuses (the gate of "tensor digests and checked deltas" relies on the same), so a damaged
 *     archive opened over resident weights and read in place leaves them untouched.  No value read from the archive is used as an index;
 *     codec bytes are stored clamped to 1.
 *   Out of scope: encryption or cryptographic integrity; archives that span element sizes (a caller concatenates one archive per element
 *     size, each at a multiple of 256, as the Python layer does); streaming a partially received archive; big-endian hosts; a compress call
 *     that allocates its frames inside an archive by itself. */
#define FSEHIP_ARCHIVE_MAGIC 0x41545346u
#define FSEHIP_ARCHIVE_VERSION 1u
#define FSEHIP_ARCHIVE_CODECS 1u
#define FSEHIP_ARCHIVE_DIGESTS 2u
#define FSEHIP_ARCHIVE_SPARSE 4u
#define FSEHIP_ARCHIVE_DELTA 8u
typedef struct {                 /* the first 64 bytes are the header as it lies in the archive */
    uint32_t magic; uint16_t version; uint16_t flags;
    uint8_t elemBytes, blockSizeId, segLog, deltaOp; uint16_t sparsePermille; uint16_t reserved;
    uint64_t nTensors, nFrames, totalBytes, maxTotalBlocks, metaBytes, framesBytes;
    uint64_t headBytes;
} FSEHIP_ArchiveInfo;
FSEHIP_API size_t FSEHIP_archive_headBytes(uint64_t nTensors, uint64_t nFrames, unsigned flags, uint64_t metaBytes);
FSEHIP_API size_t FSEHIP_archive_inspect(FSEHIP_ArchiveInfo* out, const void* h_header64, uint64_t archiveBytes);
FSEHIP_API size_t FSEHIP_archive_workspaceBound(uint64_t nTensors, uint64_t nFrames, uint64_t headBytes);
FSEHIP_API int FSEHIP_archive_seal_dbatch(void* d_archive, uint64_t archiveCapacity, size_t* d_result, const FSEHIP_ArchiveInfo* info, const uint64_t* d_srcOffsets,
                                          const uint64_t* d_frameOffsets, const size_t* d_frameResults, const size_t* d_tensorResults, const uint8_t* d_codecs,
                                          const uint64_t* d_digests, const void* d_meta, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_archive_open_dbatch(uint64_t* d_srcOffsets, uint64_t* d_frameOffsets, uint8_t* d_codecs, uint64_t* d_digests, uint64_t* d_segFirst, size_t* d_verdict,
                                          const void* d_archive, uint64_t archiveBytes, const FSEHIP_ArchiveInfo* info, void* d_workspace, size_t workspaceBytes,
                                          void* stream);

/* Predicted planes (planes_pred.hip): NEIGHBOUR DELTA IN THE SPLIT, RUN SCANS IN THE MERGE.  The planes above compress a tensor whose bytes
 * are skewed at order 0.  A tensor whose neighbouring elements are close -- sorted indices, offsets, position ids, sampled fields, audio --
 * is skewed only after the previous element is subtracted from each one, as integers.  These calls are the plain calls on that difference:
 * the same plane layout, the same offsets, results and refusals, ordinary .fse frames; nothing in a frame records the predictor, the caller
 * carries it as it carries a delta's op.  Opt-in: no call chooses prediction by itself.
 *
 *   The transform (normative; a numpy model in tests/planes_pred_corpus.py).  For a tensor of n bytes and elemBytes E: W = 8 E, m =
 *   floor(n / E) whole elements t[0 .. m), little-endian unsigned integers counted from the tensor's start whatever its address.  A RUN is
 *   R = 1 << FSEHIP_PRED_RUN_LOG = 1024 elements.
 *     forward:  p[j] = 0 where j mod R == 0, else t[j - 1];  z[j] = zigzag((t[j] - p[j]) mod 2^W), the zigzag of "arithmetic tensor deltas"
 *     inverse:  d[j] = unzigzag(z[j]);  t[j] = the sum of d[k] over k = R floor(j / R) .. j, mod 2^W
 *   The trailing n mod E bytes pass unchanged.  A bijection for every bit pattern, no float arithmetic; independent of where the tensor
 *   lies in the batch.  The planes are the plain planes of z.  A run divides every plane segment (segLog >= 10), so segment frames of
 *   predicted planes are those of "segmented planes" with no rule of their own.
 *
 *   FSEHIP_planes_split_pred_dbatch   FSEHIP_planes_split_dbatch on z: the same arguments, offsets and results.  d_planes and d_src are
 *     required for elemBytes == 1 too (the differences have to be written somewhere), as with XOR.  The source is only read.
 *   FSEHIP_planes_merge_pred_dbatch   FSEHIP_planes_merge_dbatch with the inverse: the same arguments, verdicts and rules for what is
 *     written (a refused tensor: nothing).  d_dst must not overlap d_planes.  Work item w belongs to the largest tensor i with
 *     floor(D[i] / T) + i <= w and rebuilds the bytes [t T, (t + 1) T) OF THAT TENSOR, t = w - floor(D[i] / T) - i: tiles are relative to
 *     the tensor, so that a workgroup owns whole runs (T / E / R of them).  One run is one round of one wave: a lane sums its 16 elements
 *     in registers, a wave scan of the lane totals gives its carry-in.  No LDS, no workspace, no workgroup waits on another.
 *   FSEHIP_tensor_compress_pred_dbatch   the predicted split, then the packed writer with `codec`, or -- d_codecs given -- the mixed writer
 *     with policy and tolerancePermille: FSEHIP_tensor_compress_mixed_dbatch without d_base, codec and d_codecs taken as
 *     FSEHIP_tensor_compress_seg_dbatch takes them.  d_planes is required.
 *   FSEHIP_tensor_decompress_pred_dbatch   FSEHIP_tensor_decompress_dbatch with the predicted merge.
 *   FSEHIP_tensor_compress_seg_pred_dbatch / FSEHIP_tensor_decompress_seg_pred_dbatch   the segmented pair: the _seg_op_ calls without d_base
 *     and deltaOp.
 *   All six: launches only (capturable); every argument error is hipErrorInvalidValue before any device call, with nothing written;
 *   workspaces are the writers' and readers' own.
 *   Out of scope: (strides 2 .. 8, interleaved channels: "strided predicted planes" below); higher-order or float-aware predictors; prediction combined with a base or
 *   with sparse planes; (windows and patches of predicted tensors: "windows of" and "patching tensors with a transform per tensor" below); a record of the predictor in frames or in the archive head. */
#define FSEHIP_PRED_RUN_LOG 10
FSEHIP_API int FSEHIP_planes_split_pred_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const uint64_t* d_srcOffsets,
                                               size_t nTensors, unsigned elemBytes, uint64_t capacity, void* stream);
FSEHIP_API int FSEHIP_planes_merge_pred_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                               const size_t* d_planeSizes, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_pred_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                  const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                                  size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille,
                                                  unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes,
                                                  void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_pred_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results, const void* d_frames,
                                                    const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks, void* d_planes,
                                                    uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults, void* d_workspace, size_t workspaceBytes,
                                                    void* stream);
FSEHIP_API int FSEHIP_tensor_compress_seg_pred_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                      const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                                      const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks, unsigned blockSizeId,
                                                      int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes,
                                                      uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_seg_pred_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results, const void* d_frames,
                                                        const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst,
                                                        size_t nSegments, unsigned segLog, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                                                        uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets, size_t* d_planeSizes, void* d_workspace,
                                                        size_t workspaceBytes, void* stream);

/* Strided predicted planes (planes_stride.hip): NEIGHBOUR DELTA ACROSS INTERLEAVED CHANNELS.  In stereo int16 audio, RGB / RGBA uint8
 * pixels, [N, 3] coordinates, (x, y, w, h) boxes or complex64 seen as pairs of float32 the element in front of an element belongs to another
 * channel: its difference is as wide as the values, and the predicted planes above compress worse than the plain ones.  These calls take the
 * predecessor S elements back, the same channel.  Nothing in a frame changes: ordinary .fse frames of the planes of z, and the caller carries
 * the stride as it carries the predictor.
 *
 *   The transform (normative; a numpy model in tests/planes_stride_corpus.py).  For a tensor of n bytes and elemBytes E in {1, 2, 4, 8}:
 *   W = 8 E, m = floor(n / E) elements t[0 .. m), little-endian unsigned integers, R = 1 << FSEHIP_PRED_RUN_LOG = 1024 elements, and a
 *   stride S, 1 <= S <= FSEHIP_PRED_MAX_STRIDE = 8.
 *     forward:  p[j] = 0 where (j mod R) < S, else t[j - S];  z[j] = zigzag((t[j] - p[j]) mod 2^W), the zigzag of "arithmetic tensor deltas"
 *     inverse:  d[j] = unzigzag(z[j]);  t[j] = the sum of d[k] over k = j, j - S, j - 2 S, .. while k >= R floor(j / R), mod 2^W
 *   The trailing n mod E bytes pass unchanged.  A tensor of fewer than S elements is zigzag(t).  S = 1 is exactly "predicted planes".  Runs
 *   stay 1024 elements counted from the tensor's start whatever S is, and every plane segment still starts on a run (segLog >= 10), so
 *   segmented frames need no rule of their own; S of every 1024 elements are coded without a predecessor, the price of that independence.
 *   The chain an element belongs to is (j mod R) mod S -- not j mod S: 1024 mod S != 0 for S = 3, 5, 6, 7 -- it starts again at every run,
 *   and each of the first S elements of a run is its own chain head.
 *
 *   The six calls are the _pred_ calls they are named after with `stride` directly in front of `stream`: offsets, results, refusals and
 *   the rules for what is written are those.  stride == 0 or stride > FSEHIP_PRED_MAX_STRIDE: hipErrorInvalidValue before any launch, nothing
 *   written.  stride == 1 launches the kernels of the _pred_ calls (which are these calls with stride 1).  The split reads the S elements in
 *   front of a chunk of 16 where it read one; the merge sums S chains per run in one round of one wave: an in-lane recurrence, S wave
 *   scans of the lanes' per-chain totals, no LDS, no workspace, nothing crosses a workgroup.  Launches only (capturable); workspaces are the
 *   writers' and readers' own.
 *   Out of scope: strides above 8 (a row-above or 2-D predictor needs strides far beyond a run); (a stride per tensor and strides in the
 *   estimate: "strides in the estimate" and "a stride per tensor" below); windows and patches of strided objects; prediction combined with a
 *   base or with sparse planes; a record of the stride in frames or in the archive head. */
#define FSEHIP_PRED_MAX_STRIDE 8
FSEHIP_API int FSEHIP_planes_split_pred_stride_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const uint64_t* d_srcOffsets,
                                                      size_t nTensors, unsigned elemBytes, uint64_t capacity, unsigned stride, void* stream);
FSEHIP_API int FSEHIP_planes_merge_pred_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                                      const size_t* d_planeSizes, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, unsigned stride, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_pred_stride_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                         const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                                         size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy,
                                                         unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets, void* d_workspace,
                                                         size_t workspaceBytes, unsigned stride, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_pred_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results, const void* d_frames,
                                                           const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks, void* d_planes,
                                                           uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults, void* d_workspace,
                                                           size_t workspaceBytes, unsigned stride, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_seg_pred_stride_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                             const void* d_src, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                                             const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks, unsigned blockSizeId,
                                                             int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes,
                                                             uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace, size_t workspaceBytes, unsigned stride,
                                                             void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_seg_pred_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, size_t* d_results, const void* d_frames,
                                                               const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst,
                                                               size_t nSegments, unsigned segLog, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                                                               uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets, size_t* d_planeSizes,
                                                               void* d_workspace, size_t workspaceBytes, unsigned stride, void* stream);

/* Plane estimates (planes_estimate.hip): THE TRANSFORM CHOSEN PER TENSOR FROM DEVICE HISTOGRAMS.  The tensor line has four ways to turn a
 * tensor into byte planes -- plain, predicted, XOR against a base, SUB against a base -- each opt-in and per call, and a wrong guess costs
 * a lot either way: a bf16 gaussian grows by 5 % under prediction, sorted int64 shrinks by a third, position ids by a factor of hundreds.
 * What decides is the byte histogram of every candidate's planes, and that is one read of the tensor (and of its base): no plane buffer,
 * no coder.  This call returns, per tensor and candidate, the order-0 cost of every plane, an estimated size, and a choice.  It changes
 * no other call and no frame byte; the caller hands the chosen transform to the compress calls above.
 *
 *   The cost (normative, in integers; a numpy model in tests/planes_estimate_corpus.py -- device and model agree to the last bit).
 *     T[f] = floor(256 log2(1 + f / 256) + 0.5) for f = 0 .. 255, a constant table; T[0] = 0.
 *     L(x) for an integer x >= 1:  e = floor(log2 x);  f = the eight bits below the leading one, ((x << (63 - e)) >> 55) & 0xFF on 64
 *       bits;  L(x) = 256 e + T[f].  L does not decrease, L(2^k) = 256 k, and |L(x) / 256 - log2 x| < 1.95 / 256 (the truncation to eight
 *       bits, log2(1 + 1 / 256), plus half a unit of rounding; 1.87 / 256 is the largest seen over 1 .. 69999).
 *     A plane with counts c[0 .. 255], N = their sum:  bits256 = the sum over s with c[s] > 0 of c[s] (L(N) - L(c[s])), in uint64.
 *     estBytes(plane) = min(N, (bits256 + 2047) >> 11) -- the min stands for a raw block;  estBytes(tensor, candidate) = the sum over its
 *       E planes.  No term for headers or tables: every candidate writes the same number of frames and blocks.
 *   The planes are exactly the ones the corresponding split writes, the trailing n mod E bytes included: candidate
 *     FSEHIP_EST_PLAIN  FSEHIP_planes_split_dbatch          FSEHIP_EST_PRED  FSEHIP_planes_split_pred_dbatch
 *     FSEHIP_EST_XOR    FSEHIP_planes_split_xor_dbatch      FSEHIP_EST_SUB   FSEHIP_planes_split_op_dbatch with FSEHIP_DELTA_SUB
 *   Candidate c is requested with bit 1u << c of candidateMask.
 *   The choice of a tensor: best = the lowest requested id; every further requested c, in rising order, replaces it iff
 *     estBytes[c] * 1000 < estBytes[best] * (1000 - marginPermille).  marginPermille (0 .. 1000) is hysteresis towards the simpler form, a
 *     policy argument as the mixed writer's tolerancePermille is, not a measurement.
 *
 *   FSEHIP_planes_estimate_workspaceBound   host arithmetic, a multiple of 256: per tensor and REQUESTED candidate E histograms of 256
 *     32-bit counters.  GENERIC for an elemBytes other than 1, 2, 4, 8, a candidateMask of 0 or with an unknown bit, or 2^24 tensors.
 *   FSEHIP_planes_estimate_dbatch   tensor i = [S[i], S[i + 1]) of d_src (S = d_srcOffsets, nTensors + 1 entries, any sizes and alignments;
 *     `capacity` = the size of d_src, it sizes the launch); d_base, read only where XOR or SUB is requested, is laid out as d_src is.  ->
 *       d_planeBits[(i * 4 + c) * E + p]   bits256 of plane p of tensor i under candidate c
 *       d_estBytes[i * 4 + c]              estBytes(tensor i, c)
 *       d_choice[i]                        the chosen candidate id
 *       d_results[i]                       n_i
 *     Slots of candidates that were not requested are all-ones.  A tensor of 0 bytes: estimates 0, the lowest requested id, result 0.
 *     Where S[i] > S[i + 1] or S[i + 1] > capacity: d_results[i] = GENERIC, d_choice[i] = 0xFF, all its d_estBytes and d_planeBits entries
 *     all-ones, and nothing of that tensor is read.  COUNTS ARE EXACT AND 32 BITS WIDE: a tensor of 2^32 bytes or more is refused in the
 *     same way with srcSize_wrong (cut it, as the segmented calls do).  Offsets are expected non-decreasing, as everywhere: around a slot
 *     that decreases a tensor may miss tiles of its own (never a byte outside [0, capacity) is read) and its estimate is then too low.
 *     The source and the base are only read.  nTensors == 0 is legal.
 *     The work: a launch that zeroes the counters (the call does so itself, every time: a replayed graph returns the same numbers); the
 *     counting kernel in the ragged mapping of "byte planes" -- ceil(capacity / T) + nTensors workgroups, chunks of 16 elements per lane
 *     counted from the tensor's start, head and tail an element per thread -- where a lane loads its chunk (and the base's) once, derives
 *     every requested candidate in registers and counts where the split would store, into LDS histograms per (candidate, plane) -- 8 / E
 *     columns per bin, 32 KB -- that are flushed to the tensor's counters by integer atomics; a lane, or a whole wave, whose 16 bytes of a
 *     plane are one value adds them in one addition (the zero planes of a delta); then a wave per tensor for L(), the sums and the choice.
 *     Launches only (capturable).  Every argument error is hipErrorInvalidValue before any device call, with nothing written: a null
 *     output, d_src or d_srcOffsets; candidateMask == 0 or an unknown bit; XOR or SUB requested with d_base == NULL; elemBytes not 1, 2, 4
 *     or 8; marginPermille > 1000; a launch beyond the limits of "byte planes"; a workspace that is misaligned (256) or below the bound.
 *   Out of scope: sparse planes as a candidate (the sparse pack selects itself per plane); a record of the choice inside frames; costs
 *   beyond order 0. */
#define FSEHIP_EST_PLAIN 0
#define FSEHIP_EST_PRED 1
#define FSEHIP_EST_XOR 2
#define FSEHIP_EST_SUB 3
FSEHIP_API size_t FSEHIP_planes_estimate_workspaceBound(size_t nTensors, unsigned elemBytes, unsigned candidateMask);
FSEHIP_API int FSEHIP_planes_estimate_dbatch(uint64_t* d_planeBits, uint64_t* d_estBytes, uint8_t* d_choice, size_t* d_results, const void* d_src, const void* d_base,
                                             const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity, unsigned candidateMask,
                                             unsigned marginPermille, void* d_workspace, size_t workspaceBytes, void* stream);

/* A transform per tensor (planes_each.hip, capi_each.hip): ONE SPLIT, ONE MERGE AND ONE COMPOSITE FOR A BATCH WHOSE TENSORS TAKE DIFFERENT
 * TRANSFORMS.  Every call above takes one transform per call, so a caller of the estimate had to read the choices back, cut the batch by
 * choice and call once per part.  These calls read the transform of tensor i from a device array, d_transforms[i] = FSEHIP_EST_PLAIN,
 * _PRED, _XOR or _SUB -- the ids the estimate writes to d_choice -- given by the caller or chosen by the call itself and returned: choose
 * once, then give, as the mixed writer treats d_codecs.  No transform is defined here and no frame byte differs.
 *
 *   The contract (normative; a numpy model in tests/planes_each_corpus.py): the planes of tensor i are byte for byte the planes that
 *     FSEHIP_planes_split_dbatch (PLAIN), FSEHIP_planes_split_pred_dbatch (PRED), FSEHIP_planes_split_xor_dbatch (XOR) or
 *     FSEHIP_planes_split_op_dbatch with FSEHIP_DELTA_SUB (SUB) writes for that tensor, the trailing n mod E bytes included, at the same
 *     plane offsets and with the same result; the merge is the exact inverse.
 *   Refused tensors: a transform byte that is none of the four (the estimate's 0xFF for a tensor it refused among them), or XOR / SUB where
 *     d_base is NULL: the tensor's result is GENERIC and nothing of it is read or written -- merged in place, its old bytes stay.  Its plane
 *     offsets are those of its size; a composite writes frames of whatever d_planes held there, and the tensor's result says to drop them.
 *
 *   FSEHIP_planes_split_each_dbatch   FSEHIP_planes_split_pred_dbatch with d_base (may be NULL; laid out as d_src is, read for XOR and SUB
 *     tensors only) and d_transforms (nTensors bytes): the same arguments, offsets, results and refusals as the call it is named after.
 *     d_planes and d_src are required for elemBytes == 1 too (a PLAIN tensor of one-byte elements is copied).  The flat ragged mapping of
 *     "byte planes", chunks of 16 whole elements counted from the tensor's start; a workgroup has one tensor, so the branch on the
 *     transform is uniform over it.
 *   FSEHIP_planes_merge_each_dbatch   FSEHIP_planes_merge_pred_dbatch with d_base and d_transforms: the same arguments, verdicts and rules
 *     for what is written.  Tiles relative to the tensor, as there; a PRED tensor takes the run scan, the others are element-wise in the
 *     same rounds.  d_base may be exactly d_dst (in place, as in FSEHIP_planes_merge_xor_dbatch); a PLAIN or PRED tensor overwrites its
 *     bytes.  d_dst must not overlap d_planes.
 *   FSEHIP_tensor_compress_each_dbatch / FSEHIP_tensor_compress_seg_each_dbatch   FSEHIP_tensor_compress_pred_dbatch /
 *     FSEHIP_tensor_compress_seg_pred_dbatch with d_base (may be NULL), d_transforms and transformPolicy; codec, d_codecs, policy and
 *     tolerancePermille exactly as there.
 *       FSEHIP_TRANSFORMS_GIVEN    d_transforms is an INPUT; candidateMask, marginPermille and d_estBytes are ignored.
 *       FSEHIP_TRANSFORMS_CHOOSE   d_transforms is an OUTPUT: the call runs FSEHIP_planes_estimate_dbatch with candidateMask and marginPermille
 *         (its rules) on the stream, writes d_choice to d_transforms, splits by it and runs the writer -- no host read in between.  d_estBytes
 *         (may be NULL): nTensors * 4 entries, the estimate's d_estBytes.  The same inputs, mask and margin give the same bytes.
 *     The workspace: FSEHIP_tensor_each_workspaceHead(nTensors, elemBytes, transformPolicy, candidateMask) bytes (host arithmetic, a multiple
 *     of 256; 0 for GIVEN; GENERIC where the estimate's bound is) in front of the writer's own workspace, whose bound is that of the _pred_
 *     composite.
 *   FSEHIP_tensor_decompress_each_dbatch / FSEHIP_tensor_decompress_seg_each_dbatch   the _pred_ pair with d_base (may be NULL) and
 *     d_transforms, always an input.
 *   All six: launches only (capturable); nTensors == 0 is legal; every argument error is hipErrorInvalidValue before any device call, with
 *     nothing written: a null mandatory pointer; elemBytes not 1, 2, 4 or 8; an unknown transformPolicy; with CHOOSE a candidateMask of 0
 *     or with an unknown bit, XOR or SUB in it with d_base == NULL, marginPermille > 1000, 2^24 tensors; a workspace that is misaligned
 *     (256) or short; a launch beyond the limits of "byte planes"; whatever the writer or the reader refuses.
 *   Out of scope: sparse planes around these calls; digests and gating (windows and patches: the next two sections); a record of the transforms in frames or in
 *   the archive head (the caller carries d_transforms as it carries a delta's op); new candidates or costs in the estimate. */
#define FSEHIP_TRANSFORMS_GIVEN  0   /* d_transforms is an INPUT: nTensors bytes, FSEHIP_EST_PLAIN .. FSEHIP_EST_SUB */
#define FSEHIP_TRANSFORMS_CHOOSE 1   /* d_transforms is an OUTPUT: the estimate's choice per tensor */
FSEHIP_API size_t FSEHIP_tensor_each_workspaceHead(size_t nTensors, unsigned elemBytes, int transformPolicy, unsigned candidateMask);
FSEHIP_API int FSEHIP_planes_split_each_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const void* d_base,
                                               const uint8_t* d_transforms, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                               void* stream);
FSEHIP_API int FSEHIP_planes_merge_each_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                               const size_t* d_planeSizes, const void* d_base, const uint8_t* d_transforms, size_t nTensors, unsigned elemBytes,
                                               uint64_t dstCapacity, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_each_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                  const void* d_src, const void* d_base, uint8_t* d_transforms, int transformPolicy, unsigned candidateMask,
                                                  unsigned marginPermille, uint64_t* d_estBytes, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                  uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy,
                                                  unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets, void* d_workspace,
                                                  size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_seg_each_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                      const void* d_src, const void* d_base, uint8_t* d_transforms, int transformPolicy, unsigned candidateMask,
                                                      unsigned marginPermille, uint64_t* d_estBytes, const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes,
                                                      uint64_t capacity, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks,
                                                      unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog,
                                                      void* d_planes, uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace, size_t workspaceBytes,
                                                      void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_each_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, const uint8_t* d_transforms,
                                                    size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                    size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                                    void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_seg_each_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, const uint8_t* d_transforms,
                                                        size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                        const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks, void* d_planes,
                                                        uint64_t planesCapacity, uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets,
                                                        size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream);

/* Windows of tensors with a transform per tensor (planes_each.hip, capi_each.hip): THE READ SIDE OF "windows of segmented tensors" FOR OBJECTS
 * WRITTEN BY FSEHIP_tensor_compress_seg_each_dbatch -- and, with all bytes FSEHIP_EST_PRED, by FSEHIP_tensor_compress_seg_pred_dbatch: the
 * elements [a, b) of every tensor, decoding only the segment frames that hold them.  No frame byte, reader, selection or fold changes:
 * FSEHIP_planes_windowFirst, FSEHIP_planes_select_window_dbatch and FSEHIP_planes_fold_window_dbatch are used as they are.
 *
 *   Why one more merge.  For a window of whole elements every plane contributes the same plane-relative range.  PLAIN, XOR and SUB are
 *     element-wise, so their window is merged like a tensor of its own.  PRED sums zigzag differences inside runs of 1 << FSEHIP_PRED_RUN_LOG
 *     = 1024 elements counted from the TENSOR's start, each run's first element predicted by 0: a window with a % 1024 != 0 starts inside a
 *     run, and its first element can only be rebuilt from the lead, the a % 1024 differences in front of it.
 *   The lead is always decoded already, and costs no frame.  A segment is 1 << segLog bytes of a plane with segLog >= 10 + blockSizeId >=
 *     FSEHIP_PRED_RUN_LOG, so every segment starts on a run boundary; the first selected segment starts at (a >> segLog) << segLog, which
 *     is at or below a - a % 1024; and the fold writes d_planeOffsets[j] = off[selFirst[j]] + (a - ((a >> segLog) << segLog)), so the
 *     a % 1024 bytes in front of d_planeOffsets[j] lie inside the decoded extent of plane j.  nSelected and the block count are those of
 *     FSEHIP_planes_windowFirst: the lead selects nothing.
 *
 *   FSEHIP_planes_merge_window_each_dbatch   FSEHIP_planes_merge_each_dbatch with d_windows (2 * nTensors entries: a_i, b_i in elements, as
 *     every window call takes them).  d_planeOffsets[i * E + p] points at the WINDOW's first byte of plane p, d_planeSizes are b - a (what the
 *     window fold writes), the slot d_dstOffsets[i] .. [i + 1] receives the E * (b - a) bytes tensor_i[a * E .. b * E).  THE CALLER'S
 *     CONTRACT for a PRED tensor with a < b: the a % 1024 bytes in front of every one of its plane offsets are the decoded plane bytes in
 *     front of the window; they are read, summed and not stored.  The results are the merge's five rules with n = E * (b - a), then GENERIC,
 *     with nothing of the tensor read or written (in place its old bytes stay), for: a transform byte that is none of the four; XOR or SUB
 *     with d_base == NULL; a > b; E * (b - a) != n, the window and the plane sizes disagree; a PRED tensor with a < b and a % 1024 larger
 *     than one of its plane offsets (the lead would lie in front of d_planes).  An error of the five rules -- a plane whose fold failed
 *     among them -- stays the result.  No byte outside [d_dstOffsets[i], d_dstOffsets[i] + n) is written for tensor i.  d_base has the layout
 *     of d_dst (the same windows of the base) and may be exactly d_dst.  Checked before the first launch: a null pointer other than d_base,
 *     elemBytes not 1, 2, 4 or 8, 2^31 planes, a launch beyond the limits of "byte planes" counted with 2 * nTensors (the work mapping
 *     gives every tensor one more item than the merge: a lead can add a tile).  It only launches.
 *   FSEHIP_tensor_decompress_window_each_dbatch   the argument list of FSEHIP_tensor_decompress_window_op_dbatch with d_transforms (nTensors
 *     bytes, an input) in place of deltaOp: the selection, FSEHIP_frame_decompress_packed_dbatch over the nSelected extents into d_planes, the
 *     window fold, then the merge above.  d_base may be NULL -- the tensors whose byte says XOR or SUB are then refused alone -- and may be
 *     d_dst (in place over resident window slices).  The workspace is the packed reader's for nSelected frames and nothing else.  Checked
 *     before the first launch, for all four steps: a null pointer other than d_base and d_workspace's own rule, elemBytes, segLog outside
 *     10 .. 30, 2^31 planes, segments or selected frames, nSelected > nSegments, the launch limit above, a workspace that is misaligned (256)
 *     or short, maxTotalBlocks >= 2^31.  It only launches.  A refused tensor's slot is not written; other tensors are not affected.
 *   Both: every argument error is hipErrorInvalidValue with nothing written; nTensors == 0 is legal; capturable into a graph.
 *   Out of scope: windows of sparse objects; windows finer than an element; other run lengths.  (Patches of such objects: the next section.) */
FSEHIP_API int FSEHIP_planes_merge_window_each_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                                      const size_t* d_planeSizes, const void* d_base, const uint8_t* d_transforms, const uint64_t* d_windows,
                                                      size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_window_each_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base,
                                                           const uint8_t* d_transforms, size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets,
                                                           const uint64_t* d_srcOffsets, const uint64_t* d_windows, size_t nTensors, unsigned elemBytes,
                                                           const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, const uint64_t* d_selFirst, size_t nSelected,
                                                           size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity, uint64_t* d_selFrameOffsets,
                                                           uint64_t* d_selOffsets, size_t* d_selResults, uint64_t* d_planeOffsets, size_t* d_planeSizes,
                                                           void* d_workspace, size_t workspaceBytes, void* stream);

/* Patching tensors with a transform per tensor (planes_each.hip, planes_patch.hip): THE WRITE SIDE OF "windows of tensors with a transform per
 * tensor" -- "patching segmented tensors" FOR OBJECTS WRITTEN BY FSEHIP_tensor_compress_seg_each_dbatch and, with all bytes FSEHIP_EST_PRED, by
 * FSEHIP_tensor_compress_seg_pred_dbatch.  The tensors changed inside an element window each; only the segment frames that hold the windows are
 * coded anew, under the transform the tensor was written with.  No frame byte, writer, segments kernel or splice changes: one more split.
 *
 *   Why the patch needs no lead.  PLAIN, XOR and SUB are element-wise.  PRED takes differences inside runs of 1 << FSEHIP_PRED_RUN_LOG = 1024
 *     elements counted from the TENSOR's start, each run's first element predicted by 0.  A segment is 1 << segLog bytes of a plane with
 *     segLog >= 10 + blockSizeId >= FSEHIP_PRED_RUN_LOG, so every segment starts on a run boundary; the patch stages WHOLE segments k0 .. k1 of
 *     every plane, the sub-tensor that starts at byte k0 * seg * E ("patching segmented tensors"), a multiple of 1024 elements.  Runs -- and
 *     chunks of 16 elements -- counted from the sub-tensor's start are therefore the tensor's own: no difference inside a selected segment
 *     reads an element in front of it, none outside reads an element inside.  The planes of transform(sub-tensor) ARE segments k0 .. k1 of the
 *     planes of transform(tensor), byte for byte, for all four transforms -- unlike the window READ, which may start inside a run.
 *   The identity of "patching segmented tensors" carries over: for tensors `old` and `new` that differ inside the windows only, the patch of
 *     FSEHIP_tensor_compress_seg_each_dbatch(old, T) with `new` IS FSEHIP_tensor_compress_seg_each_dbatch(new, T given): offsets, results,
 *     codecs and every frame byte.  The transforms are GIVEN only: choosing again would change a tensor's transform and with it every one of
 *     its frames, which is a full compress.
 *
 *   FSEHIP_planes_split_window_each_dbatch   the argument list of FSEHIP_planes_split_window_op_dbatch with d_transforms (nTensors bytes, an
 *     input, always given) in place of deltaOp.  The staged bytes, d_stagePlaneOffsets and d_stageResults of tensor i are byte for byte those
 *     of FSEHIP_planes_split_window_op_dbatch for FSEHIP_EST_PLAIN (d_base NULL), _XOR and _SUB; for _PRED they are segments k0 .. k1 of what
 *     FSEHIP_planes_split_pred_dbatch writes for the whole tensor.  d_base (laid out as d_src) is read for XOR and SUB tensors only and may be
 *     NULL.  Rule 1 of "patching segmented tensors" gains one cause: a transform byte above FSEHIP_EST_SUB (the estimate's 0xFF among them), or
 *     XOR / SUB with d_base == NULL -- GENERIC in d_stageResults[i], every d_stagePlaneOffsets entry of the tensor min(T[i], stageCapacity),
 *     nothing of it read or written.  Checked before the first launch: NULL d_transforms, the pointers, elemBytes, segLog outside 10 .. 30,
 *     2^31 planes and the launch limit of FSEHIP_planes_split_window_op_dbatch.  elemBytes == 1 is staged through the same kernel.
 *   FSEHIP_tensor_patch_window_each_dbatch   the argument list of FSEHIP_tensor_patch_window_op_dbatch with d_transforms in place of deltaOp:
 *     the split above, FSEHIP_planes_segments_dbatch over the stage, FSEHIP_frame_compress_packed_dbatch or _packed_mixed_dbatch, then
 *     FSEHIP_planes_splice_dbatch, all on `stream`: launches only, capturable.  Every argument check of every step runs before the first
 *     launch; argument errors are hipErrorInvalidValue with nothing written, a NULL d_transforms among them.  No *_workspaceSize of its own:
 *     the workspace is the writer's for nSelected frames, the scratch FSEHIP_planes_spliceScratchBound.  The four rules "a tensor is patched
 *     WHOLE OR NOT AT ALL" hold as written; a refused transform is a rule-1 GENERIC for that tensor alone, which keeps all its old frames.
 *   Out of scope: patches of sparse objects; choosing transforms inside a patch; patching in place; tensors that grow or shrink; windows finer
 *     than a segment; another segLog for the same object. */
FSEHIP_API int FSEHIP_planes_split_window_each_dbatch(void* d_stage, uint64_t* d_stagePlaneOffsets, size_t* d_stageResults, const void* d_src, const void* d_base,
                                                      const uint8_t* d_transforms, const uint64_t* d_srcOffsets, const uint64_t* d_windows, const uint64_t* d_stageOffsets,
                                                      size_t nTensors, unsigned elemBytes, unsigned segLog, uint64_t capacity, uint64_t stageCapacity, void* stream);
FSEHIP_API int FSEHIP_tensor_patch_window_each_dbatch(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs,
                                                      size_t* d_tensorResults, const void* d_frames, uint64_t framesCapacity, const uint64_t* d_frameOffsets,
                                                      const size_t* d_frameResults, const uint8_t* d_codecs, const void* d_src, const void* d_base,
                                                      const uint8_t* d_transforms, const uint64_t* d_srcOffsets, uint64_t capacity, const uint64_t* d_windows, size_t nTensors,
                                                      unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, const uint64_t* d_selFirst,
                                                      size_t nSelected, const uint64_t* d_stageOffsets, uint64_t stageCapacity, size_t maxTotalBlocks, unsigned blockSizeId,
                                                      int codec, uint8_t* d_newCodecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_stage,
                                                      uint64_t* d_stagePlaneOffsets, uint64_t* d_stageSegOffsets, size_t* d_stageResults, void* d_newFrames,
                                                      uint64_t newCapacity, uint64_t* d_newOffsets, size_t* d_newResults, void* d_scratch, size_t scratchBytes,
                                                      void* d_workspace, size_t workspaceBytes, void* stream);

/* Strides in the estimate (planes_estimate.hip): THE PRED STRIDE CHOSEN PER TENSOR FROM DEVICE HISTOGRAMS.  "Plane estimates" knows PRED at
 * stride 1 only, so it chooses plain planes for every interleaved tensor -- stereo int16, RGB, xyz, boxes -- and leaves the factor of two of
 * "strided predicted planes" on the table.  This call is FSEHIP_planes_estimate_dbatch with a SET of strides for the PRED candidate: per
 * tensor an estimate for every requested stride, the stride chosen among them, and the four-candidate outputs with PRED at that stride.
 *
 *   Meaning (normative, in integers; a numpy model in tests/planes_each_stride_corpus.py).  T, L, bits256 and estBytes are those of "plane
 *     estimates", unchanged.  The planes of stride candidate S are exactly what FSEHIP_planes_split_pred_stride_dbatch writes at that stride:
 *     the trailing n mod E bytes, a tensor of fewer than S elements and the chain heads (j mod 1024) < S included.
 *   strideMask: bit S - 1 requests stride S, 1 <= S <= FSEHIP_PRED_MAX_STRIDE.
 *   The stride of a tensor: best = the lowest requested stride; every further requested S, in rising order, replaces it iff
 *     est[S] * 1000 < est[best] * (1000 - marginPermille) -- the margin, rule and direction of the transform choice.  The multiples of the
 *     channel count cost a little more than the channel count itself (every run has more chain heads), so rising order lands on it.
 *
 *   FSEHIP_planes_estimate_stride_workspaceBound   host arithmetic, a multiple of 256: per tensor E histograms of 256 32-bit counters for
 *     every requested candidate beside PRED and, where PRED is requested, for every requested stride.  GENERIC where
 *     FSEHIP_planes_estimate_workspaceBound is, and for a strideMask the call refuses.  With strideMask == 1 it is that bound.
 *   FSEHIP_planes_estimate_stride_dbatch   the arguments of FSEHIP_planes_estimate_dbatch, strideMask in front of stream, two outputs behind
 *     d_results:
 *       d_strideEstBytes[i * 8 + (S - 1)]  estBytes of tensor i under PRED at stride S; all-ones for a stride that was not requested, and
 *                                          everywhere where PRED is no candidate.  May be NULL.
 *       d_strides[i]                       the chosen stride (1 where PRED is no candidate).  It is the best stride found also where
 *                                          d_choice[i] is another transform.
 *     d_planeBits, d_estBytes, d_choice and d_results are laid out as there; the PRED slots hold the numbers of the CHOSEN stride and
 *     d_choice is made by the rule of "plane estimates" over those.  A refused tensor (offsets, 2^32 bytes) is refused as there, its
 *     d_strideEstBytes entries all-ones and d_strides[i] = 0xFF.
 *     IDENTITY: with strideMask == 1 every output the two calls share is that of FSEHIP_planes_estimate_dbatch, and the entries of stride 1
 *     are its PRED numbers bit for bit under every strideMask.
 *     The work: the zeroing launch; k_est_count of "plane estimates" for the candidates beside PRED; the stride counting kernel in the same
 *     frame -- a lane loads its chunk ONCE and the 8 elements in front of it (zeros where a run starts), derives every requested stride's
 *     differences in registers and counts into LDS histograms per (requested stride, plane), 8 / E columns per bin, 8 KB per stride: 32 KB
 *     for four strides, 64 KB for all eight; a stride that is not requested costs neither a load nor a branch taken -- then a wave per
 *     tensor for the costs and both choices.  Launches only (capturable); the counters are zeroed by the call every time.
 *     Argument errors (hipErrorInvalidValue before any device call, nothing written): those of FSEHIP_planes_estimate_dbatch; a null
 *     d_strides; strideMask == 0 or with a bit above bit 7; a strideMask other than 1 where FSEHIP_EST_PRED is not in candidateMask.
 *   Out of scope: strides above 8 and 2-D predictors; costs beyond order 0. */
FSEHIP_API size_t FSEHIP_planes_estimate_stride_workspaceBound(size_t nTensors, unsigned elemBytes, unsigned candidateMask, unsigned strideMask);
FSEHIP_API int FSEHIP_planes_estimate_stride_dbatch(uint64_t* d_planeBits, uint64_t* d_estBytes, uint8_t* d_choice, size_t* d_results, uint64_t* d_strideEstBytes,
                                                    uint8_t* d_strides, const void* d_src, const void* d_base, const uint64_t* d_srcOffsets, size_t nTensors,
                                                    unsigned elemBytes, uint64_t capacity, unsigned candidateMask, unsigned marginPermille, void* d_workspace,
                                                    size_t workspaceBytes, unsigned strideMask, void* stream);

/* A stride per tensor (planes_each_stride.hip, capi_each.hip): THE SIX CALLS OF "a transform per tensor" WITH A STRIDE BYTE BESIDE THE
 * TRANSFORM BYTE.  A state dict that holds audio (stride 2), [N, 3] coordinates (3), boxes (4) and bf16 weights (plain) goes through one
 * call.  Each call has the argument list of the _each_ call it is named after with d_strides directly behind d_transforms -- const where
 * d_transforms is const, an output beside it in the compress composites, which also take strideMask behind candidateMask.  No transform is
 * defined here and no frame byte differs; the caller carries d_strides as it carries d_transforms.
 *
 *   The contract (normative; a numpy model in tests/planes_each_stride_corpus.py): the planes and frames of tensor i are byte for byte those
 *     of the dedicated call for d_transforms[i]; for FSEHIP_EST_PRED those of the _pred_stride_ call at stride d_strides[i].  The merge is
 *     the exact inverse, in place over the base as in "a transform per tensor".
 *   d_strides[i] is read only where d_transforms[i] == FSEHIP_EST_PRED.  A value of 0 or above FSEHIP_PRED_MAX_STRIDE there refuses that
 *     tensor alone, as a bad transform byte does: result GENERIC, nothing of it read or written, merged in place its bytes stay.  Under
 *     every other transform the byte is ignored, whatever it holds.
 *   d_strides == NULL: stride 1 everywhere; the call then is the _each_ call (in a CHOOSE composite only with strideMask == 1).
 *   FSEHIP_TRANSFORMS_GIVEN    d_transforms and d_strides are INPUTS; candidateMask, strideMask, marginPermille and d_estBytes are ignored.
 *   FSEHIP_TRANSFORMS_CHOOSE   both are OUTPUTS of FSEHIP_planes_estimate_stride_dbatch with candidateMask, strideMask and marginPermille, run
 *     on the stream with no host read in between; d_strides[i] is 1 for an accepted tensor whose choice is not PRED.  d_estBytes as in
 *     the _each_ composites (PRED at the chosen stride).
 *   FSEHIP_tensor_each_stride_workspaceHead   the bytes in front of the writer's workspace: 0 for GIVEN; for CHOOSE
 *     FSEHIP_planes_estimate_stride_workspaceBound and the estimate's outputs, a multiple of 256, GENERIC where that bound is or for
 *     strideMask == 0.
 *   The kernels have the frames of the _each_ kernels, a workgroup has one tensor, the branch on the transform and inside PRED on the stride
 *     is uniform over the workgroup; the bodies are those of the dedicated kernels.  No LDS, no workspace of their own.
 *   All six: launches only (capturable); nTensors == 0 is legal; the argument errors of the _each_ calls, and with CHOOSE those of
 *     FSEHIP_planes_estimate_stride_dbatch: hipErrorInvalidValue before any device call, nothing written.
 *   Windows and patches of objects with a stride above 1: "windows and patches of tensors with a stride per tensor", below (the window forms
 *     of "a transform per tensor" take stride 1).  Out of scope: strides above 8; prediction combined with a base or with sparse planes; a record of the strides in frames or in the archive head. */
FSEHIP_API size_t FSEHIP_tensor_each_stride_workspaceHead(size_t nTensors, unsigned elemBytes, int transformPolicy, unsigned candidateMask, unsigned strideMask);
FSEHIP_API int FSEHIP_planes_split_each_stride_dbatch(void* d_planes, uint64_t* d_planeOffsets, size_t* d_tensorResults, const void* d_src, const void* d_base,
                                                      const uint8_t* d_transforms, const uint8_t* d_strides, const uint64_t* d_srcOffsets, size_t nTensors,
                                                      unsigned elemBytes, uint64_t capacity, void* stream);
FSEHIP_API int FSEHIP_planes_merge_each_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes, const uint64_t* d_planeOffsets,
                                                      const size_t* d_planeSizes, const void* d_base, const uint8_t* d_transforms, const uint8_t* d_strides,
                                                      size_t nTensors, unsigned elemBytes, uint64_t dstCapacity, void* stream);
FSEHIP_API int FSEHIP_tensor_compress_each_stride_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                         const void* d_src, const void* d_base, uint8_t* d_transforms, uint8_t* d_strides, int transformPolicy,
                                                         unsigned candidateMask, unsigned strideMask, unsigned marginPermille, uint64_t* d_estBytes,
                                                         const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity, size_t maxTotalBlocks,
                                                         unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille,
                                                         unsigned slotAlignLog, void* d_planes, uint64_t* d_planeOffsets, void* d_workspace, size_t workspaceBytes,
                                                         void* stream);
FSEHIP_API int FSEHIP_tensor_compress_seg_each_stride_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                             const void* d_src, const void* d_base, uint8_t* d_transforms, uint8_t* d_strides, int transformPolicy,
                                                             unsigned candidateMask, unsigned strideMask, unsigned marginPermille, uint64_t* d_estBytes,
                                                             const uint64_t* d_srcOffsets, size_t nTensors, unsigned elemBytes, uint64_t capacity,
                                                             const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks, unsigned blockSizeId,
                                                             int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille, unsigned slotAlignLog, void* d_planes,
                                                             uint64_t* d_planeOffsets, uint64_t* d_segOffsets, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_each_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base,
                                                           const uint8_t* d_transforms, const uint8_t* d_strides, size_t* d_results, const void* d_frames,
                                                           const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, size_t maxTotalBlocks, void* d_planes,
                                                           uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults, void* d_workspace,
                                                           size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_seg_each_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base,
                                                               const uint8_t* d_transforms, const uint8_t* d_strides, size_t* d_results, const void* d_frames,
                                                               const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst,
                                                               size_t nSegments, unsigned segLog, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                                                               uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets, size_t* d_planeSizes,
                                                               void* d_workspace, size_t workspaceBytes, void* stream);

/* Windows and patches of tensors with a stride per tensor (planes_each_stride_win.hip, capi_each.hip, planes_patch.hip): THE FOUR WINDOW CALLS
 * OF "windows of tensors with a transform per tensor" AND "patching tensors with a transform per tensor" WITH THE STRIDE BYTE OF "a stride per
 * tensor".  An object written by FSEHIP_tensor_compress_seg_each_stride_dbatch, or by FSEHIP_tensor_compress_seg_pred_stride_dbatch with all
 * transform bytes FSEHIP_EST_PRED and all stride bytes its stride, is read and rewritten by element windows.  Each call has the argument
 * list of its _window_each_ sibling with const uint8_t* d_strides directly behind d_transforms.  No frame byte, selection, reader, fold,
 * segments kernel, writer or splice changes.
 *
 *   The arithmetic.  A run is 1 << FSEHIP_PRED_RUN_LOG = 1024 elements counted from the TENSOR's start at every stride; element j lies in
 *     chain (j % 1024) % S and is predicted by element j - S, the first S elements of a run by 0.  A segment starts on a multiple of 1024
 *     elements (1 << segLog >= 1024 plane bytes).
 *   Window.  [a, b) with a % 1024 != 0 needs the lead L = a % 1024, exactly as at stride 1 and whatever S is: the virtual tensor that starts
 *     L elements in front of the slot starts on a run, so its runs and its chains are the tensor's own.  All S chains are summed through
 *     the lead -- also where L < S or L % S != 0, when the chains have different lengths inside it -- and nothing of the lead is stored.
 *     THE CALLER'S CONTRACT is that of "windows of tensors with a transform per tensor": the a % 1024 bytes in front of every plane offset of
 *     a PRED tensor with a < b are the decoded plane bytes in front of the window, which the window fold guarantees.
 *   Patch.  A staged sub-tensor starts on a run, hence on a run FOR EVERY CHAIN: the planes of the strided transform of the sub-tensor are
 *     segments k0 .. k1 of the planes of the strided transform of the tensor, byte for byte.  No lead.  The identity carries over: the patch
 *     of FSEHIP_tensor_compress_seg_each_stride_dbatch(old, T, ST) with `new` IS that call on new with T and ST given.  The patch never
 *     chooses: transforms and strides are GIVEN.
 *
 *   d_strides[i] is read only where d_transforms[i] == FSEHIP_EST_PRED.  A value of 0 or above FSEHIP_PRED_MAX_STRIDE there refuses that
 *     tensor alone -- GENERIC, one more cause beside a bad transform byte in the refusals of the sibling (the merge's GENERIC; rule 1 of
 *     the stage) -- with nothing of it read or written: in place its old bytes stay, in the patch it keeps all its old frames.  Under every
 *     other transform the byte is ignored, whatever it holds.
 *   d_strides == NULL: stride 1 everywhere; the call then IS its _window_each_ sibling, byte for byte.
 *   FSEHIP_planes_merge_window_each_stride_dbatch, FSEHIP_tensor_decompress_window_each_stride_dbatch, FSEHIP_planes_split_window_each_stride_dbatch,
 *     FSEHIP_tensor_patch_window_each_stride_dbatch: results, rules, workspaces, scratch and argument errors are those of the sibling; every
 *     argument check of every step stands in front of the first launch; launches only, capturable; nTensors == 0 is legal.  The merge has
 *     the sibling's work mapping, 2 * nTensors workgroups beyond the tiles of dstCapacity; no LDS, no workspace of the kernels' own.
 *   Out of scope: windows and patches of sparse objects; digest checks on windows; choosing a stride inside a patch. */
FSEHIP_API int FSEHIP_planes_merge_window_each_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, size_t* d_results, const void* d_planes,
                                                             const uint64_t* d_planeOffsets, const size_t* d_planeSizes, const void* d_base, const uint8_t* d_transforms,
                                                             const uint8_t* d_strides, const uint64_t* d_windows, size_t nTensors, unsigned elemBytes, uint64_t dstCapacity,
                                                             void* stream);
FSEHIP_API int FSEHIP_tensor_decompress_window_each_stride_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base,
                                                                  const uint8_t* d_transforms, const uint8_t* d_strides, size_t* d_results, const void* d_frames,
                                                                  const uint64_t* d_frameOffsets, const uint64_t* d_srcOffsets, const uint64_t* d_windows, size_t nTensors,
                                                                  unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog,
                                                                  const uint64_t* d_selFirst, size_t nSelected, size_t maxTotalBlocks, void* d_planes, uint64_t planesCapacity,
                                                                  uint64_t* d_selFrameOffsets, uint64_t* d_selOffsets, size_t* d_selResults, uint64_t* d_planeOffsets,
                                                                  size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_planes_split_window_each_stride_dbatch(void* d_stage, uint64_t* d_stagePlaneOffsets, size_t* d_stageResults, const void* d_src, const void* d_base,
                                                             const uint8_t* d_transforms, const uint8_t* d_strides, const uint64_t* d_srcOffsets, const uint64_t* d_windows,
                                                             const uint64_t* d_stageOffsets, size_t nTensors, unsigned elemBytes, unsigned segLog, uint64_t capacity,
                                                             uint64_t stageCapacity, void* stream);
FSEHIP_API int FSEHIP_tensor_patch_window_each_stride_dbatch(void* d_out, uint64_t outCapacity, uint64_t* d_outOffsets, size_t* d_outResults, uint8_t* d_outCodecs,
                                                             size_t* d_tensorResults, const void* d_frames, uint64_t framesCapacity, const uint64_t* d_frameOffsets,
                                                             const size_t* d_frameResults, const uint8_t* d_codecs, const void* d_src, const void* d_base,
                                                             const uint8_t* d_transforms, const uint8_t* d_strides, const uint64_t* d_srcOffsets, uint64_t capacity,
                                                             const uint64_t* d_windows, size_t nTensors, unsigned elemBytes, const uint64_t* d_segFirst, size_t nSegments,
                                                             unsigned segLog, const uint64_t* d_selFirst, size_t nSelected, const uint64_t* d_stageOffsets,
                                                             uint64_t stageCapacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_newCodecs, int policy,
                                                             unsigned tolerancePermille, unsigned slotAlignLog, void* d_stage, uint64_t* d_stagePlaneOffsets,
                                                             uint64_t* d_stageSegOffsets, size_t* d_stageResults, void* d_newFrames, uint64_t newCapacity,
                                                             uint64_t* d_newOffsets, size_t* d_newResults, void* d_scratch, size_t scratchBytes, void* d_workspace,
                                                             size_t workspaceBytes, void* stream);

/* ---- FSE for 16-bit symbols (lib/fseU16.h:62-80, lib/fseU16.c) -- SURVEY 8(f) rank 4.  Alphabets of up to
 * FSEHIP_FSEU16_MAX_SYMBOL_VALUE + 1 symbols, table logs up to 13 (default 12), ONE tANS state per stream: a different format from
 * the byte coder's.  Sizes of the uncompressed side are in SYMBOLS (as in the reference), strides in bytes.
 *   FSE_countU16      lib/fseU16.c:121-146   count[0..*maxSymbolValuePtr], returns the largest count; a symbol above the limit:
 *                                            maxSymbolValue_tooSmall (limits above FSEHIP_FSEU16_MAX_SYMBOL_VALUE: maxSymbolValue_tooLarge)
 *   FSE_compressU16   lib/fseU16.c:203-256   returns the compressed size, 0 (not compressible), 1 (one symbol only), or an error
 *   FSE_decompressU16 lib/fseU16.c:306-329   returns the number of symbols regenerated or an error
 * Undefined behaviour of the reference is refused instead of reproduced: 8 bytes or less of room behind the header store no payload
 * (the reference writes in front of its buffer, fseU16.c:164 ignoring bitstream.h:191) and a stream without payload is
 * srcSize_wrong (the reference reads through a null pointer). */
#define FSEHIP_FSEU16_MAX_SYMBOL_VALUE 286
#define FSEHIP_FSEU16_MAX_TABLELOG 13
#define FSEHIP_FSEU16_DEFAULT_TABLELOG 12
FSEHIP_API size_t FSEHIP_FSE_countU16(unsigned* count, unsigned* maxSymbolValuePtr, const unsigned short* src, size_t srcSize);
FSEHIP_API size_t FSEHIP_FSE_compressU16(void* dst, size_t dstCapacity, const unsigned short* src, size_t srcSize, unsigned maxSymbolValue, unsigned tableLog);
FSEHIP_API size_t FSEHIP_FSE_decompressU16(unsigned short* dst, size_t dstCapacity, const void* cSrc, size_t cSrcSize);
/* batched, device-resident: block b reads d_src + b * srcStrideBytes (d_srcSizes[b] or uniformSrcSize symbols) and writes
 * d_dst + b * dstStride; d_counts holds (FSEHIP_FSEU16_MAX_SYMBOL_VALUE + 1) entries per block */
FSEHIP_API size_t FSEHIP_FSE_compressU16_batch_workspaceSize(size_t nBlocks);
FSEHIP_API size_t FSEHIP_FSE_decompressU16_batch_workspaceSize(size_t nBlocks);
FSEHIP_API int FSEHIP_FSE_countU16_batch(unsigned* d_counts, unsigned* d_maxSymbolValues, size_t* d_results, const unsigned short* d_src, size_t srcStrideBytes,
                                         const size_t* d_srcSizes, size_t uniformSrcSize, unsigned maxSymbolValue, size_t nBlocks, void* stream);
FSEHIP_API int FSEHIP_FSE_compressU16_batch(void* d_dst, size_t dstStride, size_t dstCapacity, size_t* d_results, const unsigned short* d_src, size_t srcStrideBytes,
                                            const size_t* d_srcSizes, size_t uniformSrcSize, unsigned maxSymbolValue, unsigned tableLog, size_t nBlocks,
                                            void* d_workspace, size_t workspaceBytes, void* stream);
FSEHIP_API int FSEHIP_FSE_decompressU16_batch(unsigned short* d_dst, size_t dstStrideBytes, size_t dstCapacity, size_t* d_results, const void* d_cSrc, size_t cStride,
                                              const size_t* d_cSizes, size_t uniformCSize, size_t nBlocks, void* d_workspace, size_t workspaceBytes, void* stream);

/* ---- UNSTABLE: measurement aids, not part of the codec API.  Process-wide switches meant for ONE thread that owns the device while they are on
 * (bench.py's roofline figures); their numbering and meaning change with the kernels.  Declared only for a translation unit that defines
 * FSEHIP_INTERNAL before including this header; a product caller has no business with them.
 * Kernel timing probe for benchmarks: between probe_begin and probe_collect every kernel launch of the library is
 * bracketed by HIP events on its own stream.  probe_collect synchronises and returns, per kernel id
 * (0 hist, 1 fse_cprep, 2 fse_encode [lane per block], 3 fse_dprep, 4 fse_decode, 5 huf_cprep, 6 huf_encode, 7 huf_dprep,
 * 8 huf_decode, 9 fse_encode_wave [wave per block]), the summed duration in milliseconds and the number of launches.  Arrays hold 16 entries. */
#ifdef FSEHIP_INTERNAL
FSEHIP_API int FSEHIP_probe_begin(void);
FSEHIP_API int FSEHIP_probe_collect(double* totalMs16, unsigned* launches16);
/* Cycle accounting inside the FSE decoder (the bound that actually holds for it is chain latency x LDS-resident blocks, not HBM):
 * between (1, NULL) and (0, out16) the one-shot FSE decompressor runs an instrumented instantiation of its hot-loop kernel.
 * out16: [0] cycles of decoder-wave rounds that ran a phase of 16 iterations (4 symbols each), [1] cycles of rounds that waited,
 * [2] / [3] their numbers, [4] workgroups, [5] / [6] busy / idle cycles of one service wave per workgroup, [7] cycles inside the phases proper (without the
 * bookkeeping between them),
 * [8] engine clock in kHz, [9] blocks per workgroup | workgroups per CU << 32 | decoder waves per workgroup << 40 | iterations per phase << 48, [10] rounds of finishing phases (two iterations) and
 * [15] their cycles, [11] / [12] lifetime of the decoder waves in cycles / in ticks of the constant 100 MHz clock, [13] cycles before
 * the first phase (set-up), [14] cycles after the last (literal tail).  Synchronises the device; for benchmarks only. */
FSEHIP_API int FSEHIP_debug_decodeTiming(int enable, unsigned long long* out16);
#endif /* FSEHIP_INTERNAL */

/* Sharding a batch over the GPUs of a node (one process per GPU; the reference's chunk loop, programs/bench.c:353-364,389-424, has no
 * carried dependence, so contiguous ranges of blocks need no collective on the data path): rank `rank` of `world` codes blocks
 * [*first, *first + *count), ranges differ by at most one block.  The RCCL calls a C host puts around it when the corpus lives on
 * one rank -- one ncclGroup per direction -- are in INTEGRATION.md section 2c. */
FSEHIP_API void FSEHIP_shardRange(size_t nBlocks, int rank, int world, size_t* first, size_t* count);

/* The calls on HOST pointers (layer 1, the frames) take their device scratch from an arena the calling thread keeps between calls
 * (grow-only, at most 1 GiB; larger buffers are allocated and freed per call): no hipMalloc / hipFree on the repeated-call path.
 * FSEHIP_releaseScratch() gives the calling thread's arena back (and those of the batched frame calls' idle helper threads); a thread that
 * exits without calling it leaves its arena to the process teardown.  Returns 0 when everything was given back, the hipError_t of the first
 * hipFree that failed, hipErrorInvalidValue (1) when the calling thread is inside a call, or FSEHIP_SCRATCH_BUSY when a batched frame call
 * is running on the helper pool right now: those helpers keep their arenas (up to 64 x 1 GiB) -- call again when it has returned.
 *
 * Threads.  The batched frame calls keep a pool of helper threads inside the library (created at the first such call; each holds a HIP stream
 * and a scratch arena and sleeps on a condition variable between calls).  Consequences for the host process:
 *   - do not dlclose() the library while the pool exists: FSEHIP_shutdown() ends and joins the helpers (and frees their arenas and the calling
 *     thread's) first; it returns 0, or FSEHIP_SCRATCH_BUSY if a batch call is still running on them.  The pool restarts on demand.
 *   - do not fork() and go on using the library in the child: neither the helper threads nor the HIP runtime's own state exist there. */
#define FSEHIP_SCRATCH_BUSY (-2)
FSEHIP_API int FSEHIP_releaseScratch(void);
FSEHIP_API int FSEHIP_shutdown(void);

/* The one allocation the batched calls make themselves: FSEHIP_FSE_decompress_usingDTable_batch (whose reference signature, lib/fse.h:247, has
 * no workspace) keeps the symbol bytes of its tables in a per-device scratch of 2 x CUs slots of 72 KB that the library allocates at the first such
 * call on a device -- a hipMalloc and a synchronous hipMemset, once, kept until the process ends.  FSEHIP_prepareDevice() does that now, on the
 * current device (idempotent; returns 0 or a hipError_t): call it before a timed region or before capturing such a call into a graph -- a first
 * call that finds itself inside a stream capture without the scratch returns hipErrorStreamCaptureUnsupported instead of breaking the capture. */
FSEHIP_API int FSEHIP_prepareDevice(void);

/* build / device info: returns 0 and fills the fields when a gfx950 device is current */
typedef struct { int deviceOrdinal; int computeUnits; int ldsBytesPerCU; int wavefrontSize; char archName[64]; } FSEHIP_DeviceInfo;
FSEHIP_API int FSEHIP_deviceInfo(FSEHIP_DeviceInfo* info);
FSEHIP_API const char* FSEHIP_versionString(void);

#ifdef FSEHIP_DROPIN_NAMES
#define HIST_count FSEHIP_HIST_count
#define FSE_compress FSEHIP_FSE_compress
#define FSE_compress2 FSEHIP_FSE_compress2
#define FSE_decompress FSEHIP_FSE_decompress
#define FSE_compress_usingCTable FSEHIP_FSE_compress_usingCTable
#define FSE_decompress_usingDTable FSEHIP_FSE_decompress_usingDTable
#define HUF_compress FSEHIP_HUF_compress
#define HUF_compress2 FSEHIP_HUF_compress2
#define HUF_decompress FSEHIP_HUF_decompress
#define HUF_compress1X_usingCTable FSEHIP_HUF_compress1X_usingCTable
#define HUF_compress4X_usingCTable FSEHIP_HUF_compress4X_usingCTable
#define HUF_decompress4X_usingDTable FSEHIP_HUF_decompress4X_usingDTable
#define HUF_decompress4X1_usingDTable FSEHIP_HUF_decompress4X1_usingDTable
#define HUF_decompress1X_usingDTable FSEHIP_HUF_decompress1X_usingDTable
#define HUF_decompress1X1_usingDTable FSEHIP_HUF_decompress1X1_usingDTable
#define HIST_count_wksp FSEHIP_HIST_count_wksp
#define HIST_countFast FSEHIP_HIST_countFast
#define HIST_countFast_wksp FSEHIP_HIST_countFast_wksp
#define HIST_count_simple FSEHIP_HIST_count_simple
#define FSE_compress_wksp FSEHIP_FSE_compress_wksp
#define FSE_decompress_wksp FSEHIP_FSE_decompress_wksp
#define HUF_compress4X_wksp FSEHIP_HUF_compress4X_wksp
#define HUF_compress1X_wksp FSEHIP_HUF_compress1X_wksp
#define HUF_compress1X FSEHIP_HUF_compress1X
#define HUF_decompress4X1_DCtx_wksp FSEHIP_HUF_decompress4X1_DCtx_wksp
#endif
#ifdef FSEHIP_DROPIN_GLUE_NAMES      /* separate switch: the table glue and the header-reading single- and double-symbol decoders (a program that wants the reference's own builders beside the device's hot loops leaves it off) */
#define FSE_optimalTableLog FSEHIP_FSE_optimalTableLog
#define FSE_normalizeCount FSEHIP_FSE_normalizeCount
#define FSE_NCountWriteBound FSEHIP_FSE_NCountWriteBound
#define FSE_writeNCount FSEHIP_FSE_writeNCount
#define FSE_readNCount FSEHIP_FSE_readNCount
#define FSE_buildCTable FSEHIP_FSE_buildCTable
#define FSE_buildCTable_wksp FSEHIP_FSE_buildCTable_wksp
#define FSE_buildDTable FSEHIP_FSE_buildDTable
#define HUF_buildCTable FSEHIP_HUF_buildCTable
#define HUF_buildCTable_wksp FSEHIP_HUF_buildCTable_wksp
#define HUF_writeCTable FSEHIP_HUF_writeCTable
#define HUF_readDTableX1 FSEHIP_HUF_readDTableX1
#define HUF_readDTableX1_wksp FSEHIP_HUF_readDTableX1_wksp
#define HUF_decompress4X1 FSEHIP_HUF_decompress4X1
#define HUF_decompress4X1_DCtx FSEHIP_HUF_decompress4X1_DCtx
#define HUF_decompress1X1 FSEHIP_HUF_decompress1X1
#define HUF_decompress1X1_DCtx FSEHIP_HUF_decompress1X1_DCtx
#define HUF_decompress1X1_DCtx_wksp FSEHIP_HUF_decompress1X1_DCtx_wksp
#define HUF_readDTableX2 FSEHIP_HUF_readDTableX2
#define HUF_readDTableX2_wksp FSEHIP_HUF_readDTableX2_wksp
#define HUF_decompress4X2 FSEHIP_HUF_decompress4X2
#define HUF_decompress4X2_DCtx FSEHIP_HUF_decompress4X2_DCtx
#define HUF_decompress4X2_DCtx_wksp FSEHIP_HUF_decompress4X2_DCtx_wksp
#define HUF_decompress1X2 FSEHIP_HUF_decompress1X2
#define HUF_decompress1X2_DCtx FSEHIP_HUF_decompress1X2_DCtx
#define HUF_decompress1X2_DCtx_wksp FSEHIP_HUF_decompress1X2_DCtx_wksp
#define HUF_decompress4X2_usingDTable FSEHIP_HUF_decompress4X2_usingDTable
#define HUF_decompress1X2_usingDTable FSEHIP_HUF_decompress1X2_usingDTable
#endif
#ifdef FSEHIP_DROPIN_U16_NAMES       /* separate switch: programs/fuzzer.c declares FSE_countU16 with another (stale) prototype */
#define FSE_countU16 FSEHIP_FSE_countU16
#define FSE_compressU16 FSEHIP_FSE_compressU16
#define FSE_decompressU16 FSEHIP_FSE_decompressU16
#endif

#ifdef __cplusplus
}
#endif
#endif /* FSEHIP_H */

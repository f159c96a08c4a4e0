/* tests/host/san_window_each_stride.c -- TEST INFRASTRUCTURE: the host side of "windows and patches of tensors with a stride per tensor"
 * (csrc/capi_each.hip, csrc/planes_patch.hip; fsehip.h) under the sanitizers, as a program of its own: every argument refusal of
 * FSEHIP_planes_merge_window_each_stride_dbatch, FSEHIP_tensor_decompress_window_each_stride_dbatch,
 * FSEHIP_planes_split_window_each_stride_dbatch and FSEHIP_tensor_patch_window_each_stride_dbatch, each with d_strides given and NULL.  Every
 * refusal is decided before any device call -- so the program needs no GPU, and its pointers are host memory of the exact sizes, which a
 * refused call must leave as it is.
 *
 * Build and run (from the repository root; the host side of every source under AddressSanitizer and UndefinedBehaviorSanitizer, the
 * device code unchanged -- the composites reach into the checks of the selection, the reader, the fold, the writers and the splice, so the
 * whole library is linked):
 *   make -C finitestateentropy_amd/csrc SAN=1
 *   hipcc -O1 -g -fsanitize=address,undefined -shared-libsan tests/host/san_window_each_stride.c -o san_window_each_stride \
 *         -Lfinitestateentropy_amd/csrc/variants/san -lfsehip -Wl,-rpath,$PWD/finitestateentropy_amd/csrc/variants/san
 *   LD_LIBRARY_PATH=$(dirname $(/opt/rocm/lib/llvm/bin/clang --print-file-name=libclang_rt.asan-x86_64.so)) ./san_window_each_stride
 * (the program itself is linked against the sanitizers' shared runtime: nothing is preloaded.)  Exit code 0 and
 * "san_window_each_stride OK" on success. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/fsehip.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)
#define INVALID 1                                     /* hipErrorInvalidValue */
#define GUARD 0xF9

static void* guarded(size_t n) { void* p = malloc(n ? n : 1); if (p) memset(p, GUARD, n); return p; }
static int intact(const void* p, size_t n) { for (size_t k = 0; k < n; ++k) if (((const uint8_t*)p)[k] != GUARD) return 0; return 1; }

/* everything the four calls take, so that one field at a time can be made wrong */
typedef struct {
    /* the read side */
    void *dst, *planes, *base, *frames, *ws;
    uint64_t *off, *soff, *win, *foff, *sf, *wf, *sfo, *so, *poff;
    size_t *res, *sres, *psz;
    uint8_t *tr, *st;
    uint64_t cap;
    size_t n, nSeg, nSel, blocks, wsBytes;
    unsigned E, segLog;
    /* the write side */
    void *out, *src, *stage, *fresh, *scratch, *wws;
    uint64_t *ooff, *toff, *spo, *sso, *noff;
    size_t *ores, *tres, *fres, *stres, *nres;
    uint8_t *ocod, *cod, *ncod;
    uint64_t outCap, stageCap;
    size_t scratchBytes, wwsBytes;
    unsigned bsid, tol, align;
    int codec, policy;
} Args;

static int merge(const Args* a)
{
    return FSEHIP_planes_merge_window_each_stride_dbatch(a->dst, a->off, a->res, a->planes, a->poff, a->psz, a->base, a->tr, a->st, a->win, a->n, a->E, a->cap, NULL);
}
static int window(const Args* a)
{
    return FSEHIP_tensor_decompress_window_each_stride_dbatch(a->dst, a->off, a->cap, a->base, a->tr, a->st, a->res, a->frames, a->foff, a->soff, a->win, a->n, a->E, a->sf,
                                                              a->nSeg, a->segLog, a->wf, a->nSel, a->blocks, a->planes, 64, a->sfo, a->so, a->sres, a->poff, a->psz, a->ws,
                                                              a->wsBytes, NULL);
}
static int split(const Args* a)
{
    return FSEHIP_planes_split_window_each_stride_dbatch(a->stage, a->spo, a->stres, a->src, a->base, a->tr, a->st, a->soff, a->win, a->toff, a->n, a->E, a->segLog, 64,
                                                         a->stageCap, NULL);
}
static int patch(const Args* a)
{
    return FSEHIP_tensor_patch_window_each_stride_dbatch(a->out, a->outCap, a->ooff, a->ores, a->ocod, a->tres, a->frames, 256, a->foff, a->fres, a->cod, a->src, a->base,
                                                         a->tr, a->st, a->soff, 64, a->win, a->n, a->E, a->sf, a->nSeg, a->segLog, a->wf, a->nSel, a->toff, a->stageCap,
                                                         a->blocks, a->bsid, a->codec, a->ncod, a->policy, a->tol, a->align, a->stage, a->spo, a->sso, a->stres, a->fresh, 256,
                                                         a->noff, a->nres, a->scratch, a->scratchBytes, a->wws, a->wwsBytes, NULL);
}

int main(void)
{
    /* host arrays of the exact sizes, so that a write or a read the contract does not allow is the sanitizer's to find */
    const size_t n = 2, E = 2, nSeg = 4, nSel = 2, blocks = 4, total = 64;
    uint8_t *planes = guarded(total), *base = guarded(total), *dst = guarded(total), *frames = guarded(256), *tr = guarded(n), *st = guarded(n);
    uint64_t *off = guarded((n + 1) * 8), *soff = guarded((n + 1) * 8), *win = guarded(2 * n * 8), *foff = guarded((nSeg + 1) * 8), *sf = guarded((n * E + 1) * 8);
    uint64_t *wf = guarded((n * E + 1) * 8), *sfo = guarded((nSel + 1) * 8), *so = guarded((nSel + 1) * 8), *poff = guarded(n * E * 8);
    size_t *res = guarded(n * sizeof(size_t)), *sres = guarded(nSel * sizeof(size_t)), *psz = guarded(n * E * sizeof(size_t));
    uint8_t *out = guarded(256), *src = guarded(total), *stage = guarded(total), *fresh = guarded(256), *ocod = guarded(nSeg), *cod = guarded(nSeg), *ncod = guarded(nSel);
    uint64_t *ooff = guarded((nSeg + 1) * 8), *toff = guarded((n + 1) * 8), *spo = guarded((n * E + 1) * 8), *sso = guarded((nSel + 1) * 8), *noff = guarded((nSel + 1) * 8);
    size_t *ores = guarded(nSeg * sizeof(size_t)), *tres = guarded(n * sizeof(size_t)), *fres = guarded(nSeg * sizeof(size_t)), *stres = guarded(n * sizeof(size_t));
    size_t* nres = guarded(nSel * sizeof(size_t));
    const size_t rneed = FSEHIP_frame_decompress_packed_dbatch_workspaceSize(nSel, blocks);
    const size_t wneed = FSEHIP_frame_compress_packed_dbatch_workspaceSize(nSel, blocks, 0, 0);
    const size_t wneedMixed = FSEHIP_frame_mixedWorkspaceBound(nSel, blocks, 0, FSEHIP_CODECS_CHOOSE);
    const size_t sneed = FSEHIP_planes_spliceScratchBound(n, (unsigned)E, nSeg);
    CHECK(!FSEHIP_isError(rneed) && rneed > 1 && !FSEHIP_isError(wneed) && wneed > 1 && !FSEHIP_isError(wneedMixed) && wneedMixed >= wneed && !FSEHIP_isError(sneed) &&
          sneed > 1, "the workspace sizes");
    uint8_t *rroom = guarded(rneed + 256), *wroom = guarded(wneedMixed + 256), *sroom = guarded(sneed + 256);
    CHECK(planes && base && dst && frames && tr && st && off && soff && win && foff && sf && wf && sfo && so && poff && res && sres && psz && out && src && stage && fresh &&
          ocod && cod && ncod && ooff && toff && spo && sso && noff && ores && tres && fres && stres && nres && rroom && wroom && sroom, "malloc");
    uint8_t* rws = (uint8_t*)(((uintptr_t)rroom + 255) & ~(uintptr_t)255);
    uint8_t* wws = (uint8_t*)(((uintptr_t)wroom + 255) & ~(uintptr_t)255);
    uint8_t* sc = (uint8_t*)(((uintptr_t)sroom + 255) & ~(uintptr_t)255);

    Args good;
    memset(&good, 0, sizeof good);
    good.dst = dst; good.planes = planes; good.base = base; good.frames = frames; good.ws = rws; good.off = off; good.soff = soff; good.win = win; good.foff = foff;
    good.sf = sf; good.wf = wf; good.sfo = sfo; good.so = so; good.poff = poff; good.res = res; good.sres = sres; good.psz = psz; good.tr = tr; good.st = st;
    good.cap = total; good.n = n; good.nSeg = nSeg; good.nSel = nSel; good.blocks = blocks; good.wsBytes = rneed; good.E = (unsigned)E; good.segLog = 10;
    good.out = out; good.src = src; good.stage = stage; good.fresh = fresh; good.scratch = sc; good.wws = wws; good.ooff = ooff; good.toff = toff; good.spo = spo;
    good.sso = sso; good.noff = noff; good.ores = ores; good.tres = tres; good.fres = fres; good.stres = stres; good.nres = nres; good.outCap = 256; good.stageCap = total;
    good.scratchBytes = sneed; good.wwsBytes = wneed; good.policy = FSEHIP_CODECS_GIVEN;
    Args a;
    /* every refusal twice: with d_strides given and with d_strides NULL, which by itself is no refusal */
#define BAD(call, what, ...) do { for (int nul = 0; nul < 2; ++nul) { a = good; if (nul) a.st = NULL; __VA_ARGS__; \
                                  CHECK(call(&a) == INVALID, #call ": %s (strides %s)", what, nul ? "NULL" : "given"); } } while (0)

    /* ---- FSEHIP_planes_merge_window_each_stride_dbatch */
    BAD(merge, "null destination", a.dst = NULL);
    BAD(merge, "null offsets", a.off = NULL);
    BAD(merge, "null results", a.res = NULL);
    BAD(merge, "null planes", a.planes = NULL);
    BAD(merge, "null plane offsets", a.poff = NULL);
    BAD(merge, "null plane sizes", a.psz = NULL);
    BAD(merge, "null transforms", a.tr = NULL);
    BAD(merge, "null transforms and null base", a.tr = NULL; a.base = NULL);
    BAD(merge, "null windows", a.win = NULL);
    for (unsigned e = 0; e < 20; ++e)
        if (e != 1 && e != 2 && e != 4 && e != 8) BAD(merge, "elemBytes", a.E = e);
    BAD(merge, "2^31 planes", a.n = (size_t)1 << 30);
    BAD(merge, "a capacity beyond the launch", a.cap = (uint64_t)1 << 46);
    BAD(merge, "2^24 tiles", a.cap = (uint64_t)32768 << 24);
    BAD(merge, "2^23 tensors: the doubled tensor count", a.n = (size_t)1 << 23; a.E = 1);
    BAD(merge, "2^24 - 2 items and three tiles", a.n = ((size_t)1 << 23) - 1; a.E = 1; a.cap = 2 * 32768);

    /* ---- FSEHIP_tensor_decompress_window_each_stride_dbatch */
    BAD(window, "null destination", a.dst = NULL);
    BAD(window, "null offsets", a.off = NULL);
    BAD(window, "null transforms", a.tr = NULL);
    BAD(window, "null results", a.res = NULL);
    BAD(window, "null frames", a.frames = NULL);
    BAD(window, "null frame offsets", a.foff = NULL);
    BAD(window, "null source offsets", a.soff = NULL);
    BAD(window, "null windows", a.win = NULL);
    BAD(window, "null segFirst", a.sf = NULL);
    BAD(window, "null selFirst", a.wf = NULL);
    BAD(window, "null planes", a.planes = NULL);
    BAD(window, "null selected frame offsets", a.sfo = NULL);
    BAD(window, "null selected offsets", a.so = NULL);
    BAD(window, "null selected results", a.sres = NULL);
    BAD(window, "null plane offsets", a.poff = NULL);
    BAD(window, "null plane sizes", a.psz = NULL);
    BAD(window, "elemBytes 3", a.E = 3);
    BAD(window, "segLog 9", a.segLog = 9);
    BAD(window, "segLog 31", a.segLog = 31);
    BAD(window, "nSelected > nSegments", a.nSel = nSeg + 1; a.wsBytes = rneed + (1 << 20));
    BAD(window, "2^31 segments", a.nSeg = (size_t)1 << 31);
    BAD(window, "2^31 planes", a.n = (size_t)1 << 30);
    BAD(window, "2^31 blocks", a.blocks = (size_t)1 << 31);
    BAD(window, "a short reader workspace", a.wsBytes = rneed - 1);
    BAD(window, "no workspace bytes", a.wsBytes = 0);
    BAD(window, "no workspace", a.ws = NULL; a.wsBytes = 0);
    BAD(window, "a misaligned workspace", a.ws = rws + 8);
    BAD(window, "the launch limit", a.cap = (uint64_t)1 << 46);
    BAD(window, "the launch limit with the doubled tensor count", a.n = (size_t)1 << 23; a.E = 1);
    BAD(window, "a null base is no refusal by itself", a.base = NULL; a.wsBytes = rneed - 1);

    /* ---- FSEHIP_planes_split_window_each_stride_dbatch */
    BAD(split, "null stage", a.stage = NULL);
    BAD(split, "null plane offsets", a.spo = NULL);
    BAD(split, "null results", a.stres = NULL);
    BAD(split, "null source", a.src = NULL);
    BAD(split, "null transforms", a.tr = NULL);
    BAD(split, "null transforms and null base", a.tr = NULL; a.base = NULL);
    BAD(split, "null source offsets", a.soff = NULL);
    BAD(split, "null windows", a.win = NULL);
    BAD(split, "null stage offsets", a.toff = NULL);
    for (unsigned e = 0; e < 20; ++e)
        if (e != 1 && e != 2 && e != 4 && e != 8) BAD(split, "elemBytes", a.E = e);
    BAD(split, "segLog 9", a.segLog = 9);
    BAD(split, "segLog 31", a.segLog = 31);
    BAD(split, "2^31 planes", a.n = (size_t)1 << 30);
    BAD(split, "a stage beyond the launch", a.stageCap = (uint64_t)1 << 46);
    BAD(split, "2^24 tiles", a.stageCap = (uint64_t)32768 << 24);
    BAD(split, "2^24 tensors", a.n = (size_t)1 << 24; a.E = 1);

    /* ---- FSEHIP_tensor_patch_window_each_stride_dbatch */
    BAD(patch, "null transforms", a.tr = NULL);
    BAD(patch, "null transforms and null base", a.tr = NULL; a.base = NULL);
    BAD(patch, "null output", a.out = NULL);
    BAD(patch, "null output offsets", a.ooff = NULL);
    BAD(patch, "null output results", a.ores = NULL);
    BAD(patch, "null tensor results", a.tres = NULL);
    BAD(patch, "null frames", a.frames = NULL);
    BAD(patch, "null frame offsets", a.foff = NULL);
    BAD(patch, "null frame results", a.fres = NULL);
    BAD(patch, "null source", a.src = NULL);
    BAD(patch, "null source offsets", a.soff = NULL);
    BAD(patch, "null windows", a.win = NULL);
    BAD(patch, "null segFirst", a.sf = NULL);
    BAD(patch, "null selFirst", a.wf = NULL);
    BAD(patch, "null stage offsets", a.toff = NULL);
    BAD(patch, "null stage", a.stage = NULL);
    BAD(patch, "null stage plane offsets", a.spo = NULL);
    BAD(patch, "null stage segment offsets", a.sso = NULL);
    BAD(patch, "null stage results", a.stres = NULL);
    BAD(patch, "null new frames", a.fresh = NULL);
    BAD(patch, "null new offsets", a.noff = NULL);
    BAD(patch, "null new results", a.nres = NULL);
    BAD(patch, "null scratch", a.scratch = NULL);
    BAD(patch, "misaligned scratch", a.scratch = sc + 8);
    BAD(patch, "short scratch", a.scratchBytes = sneed - 1);
    BAD(patch, "no workspace", a.wws = NULL; a.wwsBytes = 0);
    BAD(patch, "misaligned workspace", a.wws = wws + 8);
    BAD(patch, "a short writer workspace", a.wwsBytes = wneed - 1);
    BAD(patch, "elemBytes 3", a.E = 3);
    BAD(patch, "elemBytes 0", a.E = 0);
    BAD(patch, "segLog 9", a.segLog = 9);
    BAD(patch, "segLog 31", a.segLog = 31);
    BAD(patch, "segLog below 10 + blockSizeId", a.bsid = 1);
    BAD(patch, "blockSizeId 7", a.bsid = 7; a.segLog = 20);
    BAD(patch, "nSelected > nSegments", a.nSel = nSeg + 1; a.wwsBytes = wneedMixed);
    BAD(patch, "2^31 segments", a.nSeg = (size_t)1 << 31; a.scratchBytes = (size_t)1 << 62);
    BAD(patch, "2^31 planes", a.n = (size_t)1 << 30; a.scratchBytes = (size_t)1 << 62);
    BAD(patch, "2^31 blocks", a.blocks = (size_t)1 << 31);
    BAD(patch, "an output beyond the launch", a.outCap = (uint64_t)1 << 46);
    BAD(patch, "a stage beyond the launch", a.stageCap = (uint64_t)1 << 46);
    BAD(patch, "2^24 tiles of the stage", a.stageCap = (uint64_t)32768 << 24);
    BAD(patch, "codec 2", a.codec = 2);
    BAD(patch, "slotAlignLog 13", a.align = 13);
    BAD(patch, "output codecs without the object's", a.ocod = ocod);
    BAD(patch, "the object's codecs without output codecs", a.cod = cod);
    BAD(patch, "new codecs without the object's", a.ncod = ncod);
    BAD(patch, "codecs without new codecs", a.ocod = ocod; a.cod = cod; a.wwsBytes = wneedMixed);
    BAD(patch, "a policy that is none", a.ocod = ocod; a.cod = cod; a.ncod = ncod; a.policy = 2; a.wwsBytes = wneedMixed);
    BAD(patch, "a tolerance above 1000", a.ocod = ocod; a.cod = cod; a.ncod = ncod; a.policy = FSEHIP_CODECS_CHOOSE; a.tol = 1001; a.wwsBytes = wneedMixed);
    BAD(patch, "a short mixed workspace", a.ocod = ocod; a.cod = cod; a.ncod = ncod; a.policy = FSEHIP_CODECS_CHOOSE; a.wwsBytes = wneedMixed - 1);

    CHECK(intact(planes, total) && intact(base, total) && intact(dst, total) && intact(frames, 256) && intact(tr, n) && intact(st, n), "a byte buffer of the read side was written");
    CHECK(intact(out, 256) && intact(src, total) && intact(stage, total) && intact(fresh, 256), "a byte buffer of the write side was written");
    CHECK(intact(ocod, nSeg) && intact(cod, nSeg) && intact(ncod, nSel), "codecs written");
    CHECK(intact(off, (n + 1) * 8) && intact(soff, (n + 1) * 8) && intact(win, 2 * n * 8) && intact(foff, (nSeg + 1) * 8) && intact(sf, (n * E + 1) * 8), "offsets written");
    CHECK(intact(wf, (n * E + 1) * 8) && intact(sfo, (nSel + 1) * 8) && intact(so, (nSel + 1) * 8) && intact(poff, n * E * 8), "scratch offsets of the read side written");
    CHECK(intact(ooff, (nSeg + 1) * 8) && intact(toff, (n + 1) * 8) && intact(spo, (n * E + 1) * 8) && intact(sso, (nSel + 1) * 8) && intact(noff, (nSel + 1) * 8),
          "offsets of the write side written");
    CHECK(intact(res, n * sizeof(size_t)) && intact(sres, nSel * sizeof(size_t)) && intact(psz, n * E * sizeof(size_t)), "results of the read side written");
    CHECK(intact(ores, nSeg * sizeof(size_t)) && intact(tres, n * sizeof(size_t)) && intact(fres, nSeg * sizeof(size_t)) && intact(stres, n * sizeof(size_t)) &&
          intact(nres, nSel * sizeof(size_t)), "results of the write side written");
    CHECK(intact(rroom, rneed + 256) && intact(wroom, wneedMixed + 256) && intact(sroom, sneed + 256), "workspace or scratch written");
    free(planes); free(base); free(dst); free(frames); free(tr); free(st); free(off); free(soff); free(win); free(foff); free(sf); free(wf); free(sfo); free(so); free(poff);
    free(res); free(sres); free(psz); free(out); free(src); free(stage); free(fresh); free(ocod); free(cod); free(ncod); free(ooff); free(toff); free(spo); free(sso);
    free(noff); free(ores); free(tres); free(fres); free(stres); free(nres); free(rroom); free(wroom); free(sroom);
    printf("san_window_each_stride OK\n");
    return 0;
}

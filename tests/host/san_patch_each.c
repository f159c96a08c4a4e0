/* tests/host/san_patch_each.c -- TEST INFRASTRUCTURE: the host side of "patching tensors with a transform per tensor"
 * (csrc/planes_patch.hip; fsehip.h) under the sanitizers, as a program of its own: every argument refusal of
 * FSEHIP_planes_split_window_each_dbatch and FSEHIP_tensor_patch_window_each_dbatch, which is decided before any device call -- so the
 * program needs no GPU, and its pointers are host memory of the exact sizes, which a refused call must leave as it is.
 *
 * Build and run (from the repository root; the host side of every source under AddressSanitizer and UndefinedBehaviorSanitizer, the
 * device code unchanged -- the composite reaches into the checks of the writers and the splice, so the whole library is linked):
 *   make -C finitestateentropy_amd/csrc SAN=1
 *   hipcc -O1 -g -fsanitize=address,undefined -shared-libsan tests/host/san_patch_each.c -o san_patch_each \
 *         -Lfinitestateentropy_amd/csrc/variants/san -lfsehip -Wl,-rpath,$PWD/finitestateentropy_amd/csrc/variants/san
 *   LD_LIBRARY_PATH=$(dirname $(/opt/rocm/lib/llvm/bin/clang --print-file-name=libclang_rt.asan-x86_64.so)) ./san_patch_each
 * (the program itself is linked against the sanitizers' shared runtime: nothing is preloaded.)  Exit code 0 and "san_patch_each OK" on
 * success. */
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

/* everything the composite takes, so that one field at a time can be made wrong */
typedef struct {
    void *out, *frames, *src, *base, *stage, *fresh, *scratch, *ws;
    uint64_t *ooff, *foff, *soff, *win, *sf, *wf, *toff, *spo, *sso, *noff;
    size_t *ores, *tres, *fres, *sres, *nres;
    uint8_t *ocod, *cod, *ncod, *tr;
    uint64_t outCap, stageCap;
    size_t n, nSeg, nSel, blocks, scratchBytes, wsBytes;
    unsigned E, segLog, bsid, tol, align;
    int codec, policy;
} Args;

static int patch(const Args* a)
{
    return FSEHIP_tensor_patch_window_each_dbatch(a->out, a->outCap, a->ooff, a->ores, a->ocod, a->tres, a->frames, 256, a->foff, a->fres, a->cod, a->src, a->base, a->tr,
                                                  a->soff, 64, a->win, a->n, a->E, a->sf, a->nSeg, a->segLog, a->wf, a->nSel, a->toff, a->stageCap, a->blocks, a->bsid,
                                                  a->codec, a->ncod, a->policy, a->tol, a->align, a->stage, a->spo, a->sso, a->sres, a->fresh, 256, a->noff, a->nres,
                                                  a->scratch, a->scratchBytes, a->ws, a->wsBytes, NULL);
}

int main(void)
{
    /* host arrays of the exact sizes, so that a write or a read the contract does not allow is the sanitizer's to find */
    const size_t n = 2, E = 2, nSeg = 4, nSel = 2, blocks = 4, total = 64;
    uint8_t *out = guarded(256), *frames = guarded(256), *src = guarded(total), *base = guarded(total), *stage = guarded(total), *fresh = guarded(256), *tr = guarded(n);
    uint8_t *ocod = guarded(nSeg), *cod = guarded(nSeg), *ncod = guarded(nSel);
    uint64_t *ooff = guarded((nSeg + 1) * 8), *foff = guarded((nSeg + 1) * 8), *soff = guarded((n + 1) * 8), *win = guarded(2 * n * 8), *sf = guarded((n * E + 1) * 8);
    uint64_t *wf = guarded((n * E + 1) * 8), *toff = guarded((n + 1) * 8), *spo = guarded((n * E + 1) * 8), *sso = guarded((nSel + 1) * 8), *noff = guarded((nSel + 1) * 8);
    size_t *ores = guarded(nSeg * sizeof(size_t)), *tres = guarded(n * sizeof(size_t)), *fres = guarded(nSeg * sizeof(size_t)), *sres = guarded(n * sizeof(size_t));
    size_t* nres = guarded(nSel * sizeof(size_t));
    const size_t need = FSEHIP_frame_compress_packed_dbatch_workspaceSize(nSel, blocks, 0, 0);
    const size_t needMixed = FSEHIP_frame_mixedWorkspaceBound(nSel, blocks, 0, FSEHIP_CODECS_CHOOSE);
    const size_t sneed = FSEHIP_planes_spliceScratchBound(n, (unsigned)E, nSeg);
    CHECK(!FSEHIP_isError(need) && need > 1 && !FSEHIP_isError(needMixed) && needMixed >= need && !FSEHIP_isError(sneed) && sneed > 1, "the workspace sizes");
    uint8_t *room = guarded(needMixed + 256), *sroom = guarded(sneed + 256);
    CHECK(out && frames && src && base && stage && fresh && tr && ocod && cod && ncod && ooff && foff && soff && win && sf && wf && toff && spo && sso && noff && ores &&
          tres && fres && sres && nres && room && sroom, "malloc");
    uint8_t* ws = (uint8_t*)(((uintptr_t)room + 255) & ~(uintptr_t)255);
    uint8_t* sc = (uint8_t*)(((uintptr_t)sroom + 255) & ~(uintptr_t)255);

#define SPLIT(pst, ppo, pr, ps, pb, pt, pso, pw, pto, nn, ee, sl, scap) FSEHIP_planes_split_window_each_dbatch(pst, ppo, pr, ps, pb, pt, pso, pw, pto, nn, ee, sl, total, scap, NULL)
    CHECK(SPLIT(NULL, spo, sres, src, base, tr, soff, win, toff, n, 2, 10, total) == INVALID, "split: null stage");
    CHECK(SPLIT(stage, NULL, sres, src, base, tr, soff, win, toff, n, 2, 10, total) == INVALID, "split: null plane offsets");
    CHECK(SPLIT(stage, spo, NULL, src, base, tr, soff, win, toff, n, 2, 10, total) == INVALID, "split: null results");
    CHECK(SPLIT(stage, spo, sres, NULL, base, tr, soff, win, toff, n, 2, 10, total) == INVALID, "split: null source");
    CHECK(SPLIT(stage, spo, sres, src, base, NULL, soff, win, toff, n, 2, 10, total) == INVALID, "split: null transforms");
    CHECK(SPLIT(stage, spo, sres, src, NULL, NULL, soff, win, toff, n, 2, 10, total) == INVALID, "split: null base and null transforms");
    CHECK(SPLIT(stage, spo, sres, src, base, tr, NULL, win, toff, n, 2, 10, total) == INVALID, "split: null source offsets");
    CHECK(SPLIT(stage, spo, sres, src, base, tr, soff, NULL, toff, n, 2, 10, total) == INVALID, "split: null windows");
    CHECK(SPLIT(stage, spo, sres, src, base, tr, soff, win, NULL, n, 2, 10, total) == INVALID, "split: null stage offsets");
    for (unsigned e = 0; e < 20; ++e)
        if (e != 1 && e != 2 && e != 4 && e != 8) CHECK(SPLIT(stage, spo, sres, src, base, tr, soff, win, toff, n, e, 10, total) == INVALID, "split: elemBytes %u", e);
    CHECK(SPLIT(stage, spo, sres, src, base, tr, soff, win, toff, n, 2, 9, total) == INVALID, "split: segLog 9");
    CHECK(SPLIT(stage, spo, sres, src, base, tr, soff, win, toff, n, 2, 31, total) == INVALID, "split: segLog 31");
    CHECK(SPLIT(stage, spo, sres, src, base, tr, soff, win, toff, (size_t)1 << 30, 2, 10, total) == INVALID, "split: 2^31 planes");
    CHECK(SPLIT(stage, spo, sres, src, base, tr, soff, win, toff, n, 2, 10, (uint64_t)1 << 46) == INVALID, "split: a stage beyond the launch");
    CHECK(SPLIT(stage, spo, sres, src, base, tr, soff, win, toff, n, 2, 10, (uint64_t)32768 << 24) == INVALID, "split: 2^24 tiles");
    CHECK(SPLIT(stage, spo, sres, src, base, tr, soff, win, toff, (size_t)1 << 24, 1, 10, total) == INVALID, "split: 2^24 tensors");

    const Args good = { out, frames, src, base, stage, fresh, sc, ws, ooff, foff, soff, win, sf, wf, toff, spo, sso, noff, ores, tres, fres, sres, nres, NULL, NULL, NULL, tr,
                        256, total, n, nSeg, nSel, blocks, sneed, need, (unsigned)E, 10, 0, 0, 0, 0, FSEHIP_CODECS_GIVEN };
    Args a;
#define BAD(what, ...) do { a = good; __VA_ARGS__; CHECK(patch(&a) == INVALID, "patch: %s", what); } while (0)
    BAD("null transforms", a.tr = NULL);
    BAD("null transforms and null base", a.tr = NULL; a.base = NULL);
    BAD("null output", a.out = NULL);
    BAD("null output offsets", a.ooff = NULL);
    BAD("null output results", a.ores = NULL);
    BAD("null tensor results", a.tres = NULL);
    BAD("null frames", a.frames = NULL);
    BAD("null frame offsets", a.foff = NULL);
    BAD("null frame results", a.fres = NULL);
    BAD("null source", a.src = NULL);
    BAD("null source offsets", a.soff = NULL);
    BAD("null windows", a.win = NULL);
    BAD("null segFirst", a.sf = NULL);
    BAD("null selFirst", a.wf = NULL);
    BAD("null stage offsets", a.toff = NULL);
    BAD("null stage", a.stage = NULL);
    BAD("null stage plane offsets", a.spo = NULL);
    BAD("null stage segment offsets", a.sso = NULL);
    BAD("null stage results", a.sres = NULL);
    BAD("null new frames", a.fresh = NULL);
    BAD("null new offsets", a.noff = NULL);
    BAD("null new results", a.nres = NULL);
    BAD("null scratch", a.scratch = NULL);
    BAD("misaligned scratch", a.scratch = sc + 8);
    BAD("short scratch", a.scratchBytes = sneed - 1);
    BAD("no workspace", a.ws = NULL; a.wsBytes = 0);
    BAD("misaligned workspace", a.ws = ws + 8);
    BAD("a short writer workspace", a.wsBytes = need - 1);
    BAD("elemBytes 3", a.E = 3);
    BAD("elemBytes 0", a.E = 0);
    BAD("segLog 9", a.segLog = 9);
    BAD("segLog 31", a.segLog = 31);
    BAD("segLog below 10 + blockSizeId", a.bsid = 1);
    BAD("blockSizeId 7", a.bsid = 7; a.segLog = 20);
    BAD("nSelected > nSegments", a.nSel = nSeg + 1; a.wsBytes = needMixed);
    BAD("2^31 segments", a.nSeg = (size_t)1 << 31; a.scratchBytes = (size_t)1 << 62);
    BAD("2^31 planes", a.n = (size_t)1 << 30; a.scratchBytes = (size_t)1 << 62);
    BAD("2^31 blocks", a.blocks = (size_t)1 << 31);
    BAD("an output beyond the launch", a.outCap = (uint64_t)1 << 46);
    BAD("a stage beyond the launch", a.stageCap = (uint64_t)1 << 46);
    BAD("2^24 tiles of the stage", a.stageCap = (uint64_t)32768 << 24);
    BAD("codec 2", a.codec = 2);
    BAD("slotAlignLog 13", a.align = 13);
    BAD("output codecs without the object's", a.ocod = ocod);
    BAD("the object's codecs without output codecs", a.cod = cod);
    BAD("new codecs without the object's", a.ncod = ncod);
    BAD("codecs without new codecs", a.ocod = ocod; a.cod = cod; a.wsBytes = needMixed);
    BAD("a policy that is none", a.ocod = ocod; a.cod = cod; a.ncod = ncod; a.policy = 2; a.wsBytes = needMixed);
    BAD("a tolerance above 1000", a.ocod = ocod; a.cod = cod; a.ncod = ncod; a.policy = FSEHIP_CODECS_CHOOSE; a.tol = 1001; a.wsBytes = needMixed);
    BAD("a short mixed workspace", a.ocod = ocod; a.cod = cod; a.ncod = ncod; a.policy = FSEHIP_CODECS_CHOOSE; a.wsBytes = needMixed - 1);

    CHECK(intact(out, 256) && intact(frames, 256) && intact(src, total) && intact(base, total) && intact(stage, total) && intact(fresh, 256) && intact(tr, n), "a byte buffer was written");
    CHECK(intact(ocod, nSeg) && intact(cod, nSeg) && intact(ncod, nSel), "codecs written");
    CHECK(intact(ooff, (nSeg + 1) * 8) && intact(foff, (nSeg + 1) * 8) && intact(soff, (n + 1) * 8) && intact(win, 2 * n * 8) && intact(sf, (n * E + 1) * 8), "offsets written");
    CHECK(intact(wf, (n * E + 1) * 8) && intact(toff, (n + 1) * 8) && intact(spo, (n * E + 1) * 8) && intact(sso, (nSel + 1) * 8) && intact(noff, (nSel + 1) * 8), "scratch offsets written");
    CHECK(intact(ores, nSeg * sizeof(size_t)) && intact(tres, n * sizeof(size_t)) && intact(fres, nSeg * sizeof(size_t)) && intact(sres, n * sizeof(size_t)) &&
          intact(nres, nSel * sizeof(size_t)), "results written");
    CHECK(intact(room, needMixed + 256) && intact(sroom, sneed + 256), "workspace or scratch written");
    free(out); free(frames); free(src); free(base); free(stage); free(fresh); free(tr); free(ocod); free(cod); free(ncod); free(ooff); free(foff); free(soff); free(win);
    free(sf); free(wf); free(toff); free(spo); free(sso); free(noff); free(ores); free(tres); free(fres); free(sres); free(nres); free(room); free(sroom);
    printf("san_patch_each OK\n");
    return 0;
}

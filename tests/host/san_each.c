/* tests/host/san_each.c -- TEST INFRASTRUCTURE: the host side of "a transform per tensor" (csrc/capi_each.hip; fsehip.h) under the
 * sanitizers, as a program of its own: FSEHIP_tensor_each_workspaceHead, which is host arithmetic, and every argument refusal of the six
 * FSEHIP_*_each_dbatch calls, which is decided before any device call -- so the program needs no GPU, and its pointers are host memory of
 * the exact sizes, which a refused call must leave as it is.
 *
 * Build and run (from the repository root; the host side of every source under AddressSanitizer and UndefinedBehaviorSanitizer, the
 * device code unchanged -- the calls reach into the writer's, the reader's and the estimate's checks, so the whole library is linked):
 *   make -C finitestateentropy_amd/csrc SAN=1
 *   hipcc -O1 -g -fsanitize=address,undefined -shared-libsan tests/host/san_each.c -o san_each \
 *         -Lfinitestateentropy_amd/csrc/variants/san -lfsehip -Wl,-rpath,$PWD/finitestateentropy_amd/csrc/variants/san
 *   LD_LIBRARY_PATH=$(dirname $(/opt/rocm/lib/llvm/bin/clang --print-file-name=libclang_rt.asan-x86_64.so)) ./san_each
 * (the program itself is linked against the sanitizers' shared runtime: nothing is preloaded.)  Exit code 0 and "san_each OK" on success. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/fsehip.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)
#define INVALID 1                                     /* hipErrorInvalidValue */
#define GUARD 0xF9
#define GIVEN FSEHIP_TRANSFORMS_GIVEN
#define CHOOSE FSEHIP_TRANSFORMS_CHOOSE

static size_t r256(size_t x) { return (x + 255) & ~(size_t)255; }
static void* guarded(size_t n) { void* p = malloc(n ? n : 1); if (p) memset(p, GUARD, n); return p; }
static int intact(const void* p, size_t n) { for (size_t k = 0; k < n; ++k) if (((const uint8_t*)p)[k] != GUARD) return 0; return 1; }

int main(void)
{
    static const unsigned elems[4] = { 1, 2, 4, 8 };
    for (int k = 0; k < 4; ++k) {
        const unsigned E = elems[k];
        for (size_t n = 0; n < 70; ++n) {
            CHECK(FSEHIP_tensor_each_workspaceHead(n, E, GIVEN, 0) == 0 && FSEHIP_tensor_each_workspaceHead(n, E, GIVEN, 99) == 0, "given: no head");
            for (unsigned mask = 1; mask < 16; ++mask) {
                const size_t want = FSEHIP_planes_estimate_workspaceBound(n, E, mask) + r256(n * 4 * E * 8) + r256(n * 4 * 8) + r256(n * 8);
                const size_t got = FSEHIP_tensor_each_workspaceHead(n, E, CHOOSE, mask);
                CHECK(got == want && got % 256 == 0, "head(%zu, %u, %u) = %zu, not %zu", n, E, mask, got, want);
            }
        }
        CHECK(FSEHIP_tensor_each_workspaceHead(1, E, CHOOSE, 0) == FSEHIP_ERROR(GENERIC) && FSEHIP_tensor_each_workspaceHead(1, E, CHOOSE, 16) == FSEHIP_ERROR(GENERIC), "masks");
        CHECK(FSEHIP_tensor_each_workspaceHead((size_t)1 << 24, E, CHOOSE, 1) == FSEHIP_ERROR(GENERIC) && FSEHIP_tensor_each_workspaceHead(~(size_t)0, E, CHOOSE, 15) == FSEHIP_ERROR(GENERIC),
              "2^24 tensors and more");
        CHECK(FSEHIP_tensor_each_workspaceHead(1, E, 2, 1) == FSEHIP_ERROR(GENERIC) && FSEHIP_tensor_each_workspaceHead(1, E, -1, 1) == FSEHIP_ERROR(GENERIC), "policies");
    }
    for (unsigned e = 0; e < 20; ++e)
        if (e != 1 && e != 2 && e != 4 && e != 8)
            CHECK(FSEHIP_tensor_each_workspaceHead(1, e, GIVEN, 1) == FSEHIP_ERROR(GENERIC) && FSEHIP_tensor_each_workspaceHead(1, e, CHOOSE, 1) == FSEHIP_ERROR(GENERIC), "elemBytes %u", e);

    /* the refusals: host arrays of the exact sizes, so that a write or a read the contract does not allow is the sanitizer's to find */
    const size_t n = 2, E = 2, nSeg = 4, blocks = 8, total = 64;
    uint8_t *src = guarded(total), *base = guarded(total), *planes = guarded(total), *dst = guarded(256), *tr = guarded(n), *codecs = guarded(nSeg);
    uint64_t *off = guarded((n + 1) * 8), *poff = guarded((n * E + 1) * 8), *foff = guarded((nSeg + 1) * 8), *soff = guarded((nSeg + 1) * 8), *sf = guarded((n * E + 1) * 8);
    uint64_t* est = guarded(n * 4 * 8);
    size_t *fres = guarded(nSeg * sizeof(size_t)), *tres = guarded(n * sizeof(size_t)), *psz = guarded(n * E * sizeof(size_t));
    const size_t head = FSEHIP_tensor_each_workspaceHead(n, E, CHOOSE, 15);
    size_t need = FSEHIP_frame_compress_packed_dbatch_workspaceSize(nSeg, blocks, 0, 0);
    if (FSEHIP_frame_mixedWorkspaceBound(nSeg, blocks, 0, FSEHIP_CODECS_CHOOSE) > need) need = FSEHIP_frame_mixedWorkspaceBound(nSeg, blocks, 0, FSEHIP_CODECS_CHOOSE);
    if (FSEHIP_frame_decompress_packed_dbatch_workspaceSize(nSeg, blocks) > need) need = FSEHIP_frame_decompress_packed_dbatch_workspaceSize(nSeg, blocks);
    need += head;
    uint8_t* room = guarded(need + 256);
    CHECK(src && base && planes && dst && tr && codecs && off && poff && foff && soff && sf && est && fres && tres && psz && room, "malloc");
    uint8_t* ws = (uint8_t*)(((uintptr_t)room + 255) & ~(uintptr_t)255);

#define SPLIT(pl, po, pr, ps, pb, pt, pso, nn, ee, cap) FSEHIP_planes_split_each_dbatch(pl, po, pr, ps, pb, pt, pso, nn, ee, cap, NULL)
    CHECK(SPLIT(NULL, poff, tres, src, base, tr, off, n, 2, total) == INVALID, "split: null planes");
    CHECK(SPLIT(planes, NULL, tres, src, base, tr, off, n, 2, total) == INVALID, "split: null plane offsets");
    CHECK(SPLIT(planes, poff, NULL, src, base, tr, off, n, 2, total) == INVALID, "split: null results");
    CHECK(SPLIT(planes, poff, tres, NULL, base, tr, off, n, 2, total) == INVALID, "split: null source");
    CHECK(SPLIT(planes, poff, tres, src, base, NULL, off, n, 2, total) == INVALID, "split: null transforms");
    CHECK(SPLIT(planes, poff, tres, src, base, tr, NULL, n, 2, total) == INVALID, "split: null offsets");
    CHECK(SPLIT(planes, poff, tres, src, base, tr, off, n, 3, total) == INVALID, "split: elemBytes 3");
    CHECK(SPLIT(planes, poff, tres, src, base, tr, off, n, 2, (uint64_t)1 << 46) == INVALID, "split: a capacity beyond the launch");
    CHECK(SPLIT(planes, poff, tres, src, base, tr, off, (size_t)1 << 30, 2, total) == INVALID, "split: 2^31 planes");

#define MERGE(pd, pdo, pr, pl, po, pz, pb, pt, nn, ee, cap) FSEHIP_planes_merge_each_dbatch(pd, pdo, pr, pl, po, pz, pb, pt, nn, ee, cap, NULL)
    CHECK(MERGE(NULL, off, tres, planes, poff, psz, base, tr, n, 2, total) == INVALID, "merge: null destination");
    CHECK(MERGE(dst, NULL, tres, planes, poff, psz, base, tr, n, 2, total) == INVALID, "merge: null offsets");
    CHECK(MERGE(dst, off, NULL, planes, poff, psz, base, tr, n, 2, total) == INVALID, "merge: null results");
    CHECK(MERGE(dst, off, tres, NULL, poff, psz, base, tr, n, 2, total) == INVALID, "merge: null planes");
    CHECK(MERGE(dst, off, tres, planes, NULL, psz, base, tr, n, 2, total) == INVALID, "merge: null plane offsets");
    CHECK(MERGE(dst, off, tres, planes, poff, NULL, base, tr, n, 2, total) == INVALID, "merge: null plane sizes");
    CHECK(MERGE(dst, off, tres, planes, poff, psz, base, NULL, n, 2, total) == INVALID, "merge: null transforms");
    CHECK(MERGE(dst, off, tres, planes, poff, psz, base, tr, n, 5, total) == INVALID, "merge: elemBytes 5");
    CHECK(MERGE(dst, off, tres, planes, poff, psz, base, tr, n, 2, (uint64_t)1 << 46) == INVALID, "merge: a capacity beyond the launch");

    /* the composites: one argument off at a time; seg = 0 / 1 */
    for (int seg = 0; seg < 2; ++seg) {
#define COMP(pfo, pfr, ptr, ps, pb, pt, pol, mask, margin, pso, nn, ee, cap, sl, bsid, cdc, pc, cpol, tol, al, pl, po, w, wb) \
        (seg ? FSEHIP_tensor_compress_seg_each_dbatch(dst, 256, pfo, pfr, ptr, ps, pb, pt, pol, mask, margin, est, pso, nn, ee, cap, sf, nSeg, sl, blocks, bsid, cdc, pc, cpol, tol, al, \
                                                      pl, po, soff, w, wb, NULL) \
             : FSEHIP_tensor_compress_each_dbatch(dst, 256, pfo, pfr, ptr, ps, pb, pt, pol, mask, margin, est, pso, nn, ee, cap, blocks, bsid, cdc, pc, cpol, tol, al, pl, po, w, wb, \
                                                  NULL))
        CHECK(COMP(NULL, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "null frame offsets");
        CHECK(COMP(foff, NULL, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "null frame results");
        CHECK(COMP(foff, fres, NULL, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "null tensor results");
        CHECK(COMP(foff, fres, tres, NULL, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "null source");
        CHECK(COMP(foff, fres, tres, src, base, NULL, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "null transforms");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, NULL, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "null offsets");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, NULL, poff, ws, need) == INVALID, "null planes");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, NULL, ws, need) == INVALID, "null plane offsets");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 6, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "elemBytes 6");
        CHECK(COMP(foff, fres, tres, src, base, tr, 2, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "an unknown policy");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 0, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "mask 0");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 16, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "an unknown bit");
        CHECK(COMP(foff, fres, tres, src, NULL, tr, CHOOSE, 4, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "XOR without a base");
        CHECK(COMP(foff, fres, tres, src, NULL, tr, CHOOSE, 9, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "SUB without a base");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 1001, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "margin 1001");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws + 8, need) == INVALID, "a misaligned workspace");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, NULL, need) == INVALID, "no workspace");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, head) == INVALID, "the head alone");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, head - 1) == INVALID, "a short head");
        CHECK(COMP(foff, fres, tres, src, base, tr, GIVEN, 0, 0, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, 0) == INVALID, "given: no writer workspace");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, (size_t)1 << 24, 2, total, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "2^24 tensors");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, (uint64_t)1 << 46, 10, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "the launch limit");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 7, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "block-size id 7");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 2, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "codec 2");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, codecs, 2, 0, 0, planes, poff, ws, need) == INVALID, "an unknown codec policy");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, codecs, 1, 1001, 0, planes, poff, ws, need) == INVALID, "tolerance 1001");
        CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 0, 0, NULL, 0, 0, 13, planes, poff, ws, need) == INVALID, "slot alignment 13");
        if (seg) {
            CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 9, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "segLog 9");
            CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 31, 0, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "segLog 31");
            CHECK(COMP(foff, fres, tres, src, base, tr, CHOOSE, 15, 50, off, n, 2, total, 10, 1, 0, NULL, 0, 0, 0, planes, poff, ws, need) == INVALID, "a segment below a block");
        }
#define DEC(pd, pdo, pt, pr, pf, pfo, ee, cap, sl, bl, pl, w, wb) \
        (seg ? FSEHIP_tensor_decompress_seg_each_dbatch(pd, pdo, cap, base, pt, pr, pf, pfo, n, ee, sf, nSeg, sl, bl, pl, total, soff, fres, poff, psz, w, wb, NULL) \
             : FSEHIP_tensor_decompress_each_dbatch(pd, pdo, cap, base, pt, pr, pf, pfo, n, ee, bl, pl, total, poff, psz, w, wb, NULL))
        CHECK(DEC(NULL, off, tr, tres, dst, foff, 2, total, 10, blocks, planes, ws, need) == INVALID, "read: null destination");
        CHECK(DEC(planes, NULL, tr, tres, dst, foff, 2, total, 10, blocks, src, ws, need) == INVALID, "read: null offsets");
        CHECK(DEC(planes, off, NULL, tres, dst, foff, 2, total, 10, blocks, src, ws, need) == INVALID, "read: null transforms");
        CHECK(DEC(planes, off, tr, NULL, dst, foff, 2, total, 10, blocks, src, ws, need) == INVALID, "read: null results");
        CHECK(DEC(planes, off, tr, tres, NULL, foff, 2, total, 10, blocks, src, ws, need) == INVALID, "read: null frames");
        CHECK(DEC(planes, off, tr, tres, dst, NULL, 2, total, 10, blocks, src, ws, need) == INVALID, "read: null frame offsets");
        CHECK(DEC(planes, off, tr, tres, dst, foff, 2, total, 10, blocks, NULL, ws, need) == INVALID, "read: null planes");
        CHECK(DEC(planes, off, tr, tres, dst, foff, 7, total, 10, blocks, src, ws, need) == INVALID, "read: elemBytes 7");
        CHECK(DEC(planes, off, tr, tres, dst, foff, 2, (uint64_t)1 << 46, 10, blocks, src, ws, need) == INVALID, "read: the launch limit");
        CHECK(DEC(planes, off, tr, tres, dst, foff, 2, total, 10, (size_t)1 << 31, src, ws, need) == INVALID, "read: 2^31 blocks");
        CHECK(DEC(planes, off, tr, tres, dst, foff, 2, total, 10, blocks, src, ws + 8, need) == INVALID, "read: a misaligned workspace");
        CHECK(DEC(planes, off, tr, tres, dst, foff, 2, total, 10, blocks, src, ws, 0) == INVALID, "read: no workspace");
        if (seg) CHECK(DEC(planes, off, tr, tres, dst, foff, 2, total, 9, blocks, src, ws, need) == INVALID, "read: segLog 9");
    }
    CHECK(intact(src, total) && intact(base, total) && intact(planes, total) && intact(dst, 256) && intact(tr, n) && intact(codecs, nSeg), "a byte buffer was written");
    CHECK(intact(off, (n + 1) * 8) && intact(poff, (n * E + 1) * 8) && intact(foff, (nSeg + 1) * 8) && intact(soff, (nSeg + 1) * 8) && intact(sf, (n * E + 1) * 8), "offsets written");
    CHECK(intact(est, n * 4 * 8) && intact(fres, nSeg * sizeof(size_t)) && intact(tres, n * sizeof(size_t)) && intact(psz, n * E * sizeof(size_t)), "results written");
    CHECK(intact(room, need + 256), "workspace written");
    free(src); free(base); free(planes); free(dst); free(tr); free(codecs); free(off); free(poff); free(foff); free(soff); free(sf); free(est); free(fres); free(tres);
    free(psz); free(room);
    puts("san_each OK");
    return 0;
}

/* tests/host/san_window_each.c -- TEST INFRASTRUCTURE: the host side of "windows of tensors with a transform per tensor"
 * (csrc/capi_each.hip; fsehip.h) under the sanitizers, as a program of its own: every argument refusal of
 * FSEHIP_planes_merge_window_each_dbatch and FSEHIP_tensor_decompress_window_each_dbatch, which is decided before any device call -- so the
 * program needs no GPU, and its pointers are host memory of the exact sizes, which a refused call must leave as it is.
 *
 * Build and run (from the repository root; the host side of every source under AddressSanitizer and UndefinedBehaviorSanitizer, the
 * device code unchanged -- the composite reaches into the checks of the selection, the reader and the fold, so the whole library is linked):
 *   make -C finitestateentropy_amd/csrc SAN=1
 *   hipcc -O1 -g -fsanitize=address,undefined -shared-libsan tests/host/san_window_each.c -o san_window_each \
 *         -Lfinitestateentropy_amd/csrc/variants/san -lfsehip -Wl,-rpath,$PWD/finitestateentropy_amd/csrc/variants/san
 *   LD_LIBRARY_PATH=$(dirname $(/opt/rocm/lib/llvm/bin/clang --print-file-name=libclang_rt.asan-x86_64.so)) ./san_window_each
 * (the program itself is linked against the sanitizers' shared runtime: nothing is preloaded.)  Exit code 0 and "san_window_each OK" on
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

int main(void)
{
    /* host arrays of the exact sizes, so that a write or a read the contract does not allow is the sanitizer's to find */
    const size_t n = 2, E = 2, nSeg = 4, nSel = 2, blocks = 4, total = 64;
    uint8_t *planes = guarded(total), *base = guarded(total), *dst = guarded(total), *frames = guarded(256), *tr = guarded(n);
    uint64_t *off = guarded((n + 1) * 8), *soff = guarded((n + 1) * 8), *win = guarded(2 * n * 8), *foff = guarded((nSeg + 1) * 8), *sf = guarded((n * E + 1) * 8);
    uint64_t *wf = guarded((n * E + 1) * 8), *sfo = guarded((nSel + 1) * 8), *so = guarded((nSel + 1) * 8), *poff = guarded(n * E * 8);
    size_t *res = guarded(n * sizeof(size_t)), *sres = guarded(nSel * sizeof(size_t)), *psz = guarded(n * E * sizeof(size_t));
    const size_t need = FSEHIP_frame_decompress_packed_dbatch_workspaceSize(nSel, blocks);
    CHECK(!FSEHIP_isError(need) && need > 1, "the reader's workspace size");
    uint8_t* room = guarded(need + 256);
    CHECK(planes && base && dst && frames && tr && off && soff && win && foff && sf && wf && sfo && so && poff && res && sres && psz && room, "malloc");
    uint8_t* ws = (uint8_t*)(((uintptr_t)room + 255) & ~(uintptr_t)255);

#define MERGE(pd, pdo, pr, pl, po, pz, pb, pt, pw, nn, ee, cap) FSEHIP_planes_merge_window_each_dbatch(pd, pdo, pr, pl, po, pz, pb, pt, pw, nn, ee, cap, NULL)
    CHECK(MERGE(NULL, off, res, planes, poff, psz, base, tr, win, n, 2, total) == INVALID, "merge: null destination");
    CHECK(MERGE(dst, NULL, res, planes, poff, psz, base, tr, win, n, 2, total) == INVALID, "merge: null offsets");
    CHECK(MERGE(dst, off, NULL, planes, poff, psz, base, tr, win, n, 2, total) == INVALID, "merge: null results");
    CHECK(MERGE(dst, off, res, NULL, poff, psz, base, tr, win, n, 2, total) == INVALID, "merge: null planes");
    CHECK(MERGE(dst, off, res, planes, NULL, psz, base, tr, win, n, 2, total) == INVALID, "merge: null plane offsets");
    CHECK(MERGE(dst, off, res, planes, poff, NULL, base, tr, win, n, 2, total) == INVALID, "merge: null plane sizes");
    CHECK(MERGE(dst, off, res, planes, poff, psz, base, NULL, win, n, 2, total) == INVALID, "merge: null transforms");
    CHECK(MERGE(dst, off, res, planes, poff, psz, base, tr, NULL, n, 2, total) == INVALID, "merge: null windows");
    CHECK(MERGE(dst, off, res, planes, poff, psz, NULL, NULL, win, n, 2, total) == INVALID, "merge: null base and null transforms");
    for (unsigned e = 0; e < 20; ++e)
        if (e != 1 && e != 2 && e != 4 && e != 8) CHECK(MERGE(dst, off, res, planes, poff, psz, base, tr, win, n, e, total) == INVALID, "merge: elemBytes %u", e);
    CHECK(MERGE(dst, off, res, planes, poff, psz, base, tr, win, (size_t)1 << 30, 2, total) == INVALID, "merge: 2^31 planes");
    CHECK(MERGE(dst, off, res, planes, poff, psz, base, tr, win, n, 2, (uint64_t)1 << 46) == INVALID, "merge: a capacity beyond the launch");
    CHECK(MERGE(dst, off, res, planes, poff, psz, base, tr, win, n, 2, (uint64_t)32768 << 24) == INVALID, "merge: 2^24 tiles");
    /* the doubled tensor count: 2^23 tensors are within the merge's launch and beyond the window form's */
    CHECK(MERGE(dst, off, res, planes, poff, psz, base, tr, win, (size_t)1 << 23, 1, total) == INVALID, "merge: 2^23 tensors");
    CHECK(MERGE(dst, off, res, planes, poff, psz, base, tr, win, ((size_t)1 << 23) - 1, 1, 2 * 32768) == INVALID, "merge: 2^24 - 2 items and three tiles");

#define WIN(pd, pdo, cap, pt, pr, pf, pfo, pso, pw, nn, ee, psf, ns, sl, pwf, nsel, bl, pl, psfo, pse, psr, po, pz, w, wb) \
    FSEHIP_tensor_decompress_window_each_dbatch(pd, pdo, cap, base, pt, pr, pf, pfo, pso, pw, nn, ee, psf, ns, sl, pwf, nsel, bl, pl, total, psfo, pse, psr, po, pz, w, wb, NULL)
    CHECK(WIN(NULL, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "null destination");
    CHECK(WIN(dst, NULL, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "null offsets");
    CHECK(WIN(dst, off, total, NULL, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "null transforms");
    CHECK(WIN(dst, off, total, tr, NULL, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "null results");
    CHECK(WIN(dst, off, total, tr, res, NULL, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "null frames");
    CHECK(WIN(dst, off, total, tr, res, frames, NULL, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "null frame offsets");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, NULL, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "null source offsets");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, NULL, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "null windows");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, NULL, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "null segFirst");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, NULL, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "null selFirst");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, NULL, sfo, so, sres, poff, psz, ws, need) == INVALID, "null planes");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, NULL, so, sres, poff, psz, ws, need) == INVALID, "null selected frame offsets");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, NULL, sres, poff, psz, ws, need) == INVALID, "null selected offsets");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, NULL, poff, psz, ws, need) == INVALID, "null selected results");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, NULL, psz, ws, need) == INVALID, "null plane offsets");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, NULL, ws, need) == INVALID, "null plane sizes");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 3, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "elemBytes 3");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 9, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "segLog 9");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 31, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "segLog 31");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSeg + 1, blocks, planes, sfo, so, sres, poff, psz, ws, need + (1 << 20)) == INVALID,
          "nSelected > nSegments");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, (size_t)1 << 31, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "2^31 segments");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, (size_t)1 << 30, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "2^31 planes");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, (size_t)1 << 31, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "2^31 blocks");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need - 1) == INVALID, "a short reader workspace");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, 0) == INVALID, "no workspace bytes");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, NULL, 0) == INVALID, "no workspace");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws + 8, need) == INVALID, "a misaligned workspace");
    CHECK(WIN(dst, off, (uint64_t)1 << 46, tr, res, frames, foff, soff, win, n, 2, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID, "the launch limit");
    CHECK(WIN(dst, off, total, tr, res, frames, foff, soff, win, (size_t)1 << 23, 1, sf, nSeg, 10, wf, nSel, blocks, planes, sfo, so, sres, poff, psz, ws, need) == INVALID,
          "the launch limit with the doubled tensor count");

    CHECK(intact(planes, total) && intact(base, total) && intact(dst, total) && intact(frames, 256) && intact(tr, n), "a byte buffer was written");
    CHECK(intact(off, (n + 1) * 8) && intact(soff, (n + 1) * 8) && intact(win, 2 * n * 8) && intact(foff, (nSeg + 1) * 8) && intact(sf, (n * E + 1) * 8), "offsets written");
    CHECK(intact(wf, (n * E + 1) * 8) && intact(sfo, (nSel + 1) * 8) && intact(so, (nSel + 1) * 8) && intact(poff, n * E * 8), "scratch offsets written");
    CHECK(intact(res, n * sizeof(size_t)) && intact(sres, nSel * sizeof(size_t)) && intact(psz, n * E * sizeof(size_t)), "results written");
    CHECK(intact(room, need + 256), "workspace written");
    free(planes); free(base); free(dst); free(frames); free(tr); free(off); free(soff); free(win); free(foff); free(sf); free(wf); free(sfo); free(so); free(poff);
    free(res); free(sres); free(psz); free(room);
    printf("san_window_each OK\n");
    return 0;
}

/* tests/host/san_estimate.c -- TEST INFRASTRUCTURE: the host side of the plane estimates (csrc/planes_estimate.hip; fsehip.h, "plane
 * estimates") under the sanitizers, as a program of its own: FSEHIP_planes_estimate_workspaceBound, which is host arithmetic, and every
 * argument refusal of FSEHIP_planes_estimate_dbatch, which is decided before any device call -- so the program needs no GPU, and its
 * pointers are host memory that a refused call must leave as it is.
 *
 * Build and run (from the repository root; the host side of the one source under AddressSanitizer and UndefinedBehaviorSanitizer, the
 * device code unchanged):
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-gpu-sanitize -x hip \
 *         finitestateentropy_amd/csrc/planes_estimate.hip tests/host/san_estimate.c -o san_estimate && ./san_estimate
 * Exit code 0 and "san_estimate OK" on success. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/fsehip.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)
#define INVALID 1                                     /* hipErrorInvalidValue */

int main(void)
{
    static const unsigned elems[4] = { 1, 2, 4, 8 };
    for (int k = 0; k < 4; ++k) {
        for (unsigned mask = 1; mask < 16; ++mask) {
            size_t prev = 0;
            unsigned req = 0;
            for (unsigned c = 0; c < 4; ++c) req += (mask >> c) & 1u;
            for (size_t n = 0; n < 70; ++n) {
                const size_t b = FSEHIP_planes_estimate_workspaceBound(n, elems[k], mask);
                CHECK(b % 256 == 0 && b >= prev && b >= n * req * elems[k] * 1024, "bound(%zu, %u, %u) = %zu", n, elems[k], mask, b);
                prev = b;
            }
            CHECK(FSEHIP_planes_estimate_workspaceBound(((size_t)1 << 24) - 1, elems[k], mask) < ((size_t)1 << 40), "the largest count");
            CHECK(FSEHIP_planes_estimate_workspaceBound((size_t)1 << 24, elems[k], mask) == FSEHIP_ERROR(GENERIC), "2^24 tensors");
            CHECK(FSEHIP_planes_estimate_workspaceBound(~(size_t)0, elems[k], mask) == FSEHIP_ERROR(GENERIC), "SIZE_MAX tensors");
        }
        CHECK(FSEHIP_planes_estimate_workspaceBound(1, elems[k], 0) == FSEHIP_ERROR(GENERIC) && FSEHIP_planes_estimate_workspaceBound(1, elems[k], 16) == FSEHIP_ERROR(GENERIC),
              "masks");
    }
    for (unsigned e = 0; e < 20; ++e)
        if (e != 1 && e != 2 && e != 4 && e != 8) CHECK(FSEHIP_planes_estimate_workspaceBound(1, e, 1) == FSEHIP_ERROR(GENERIC), "elemBytes %u", e);

    /* the refusals: exact-size host arrays, so that a write or a read the contract does not allow is the sanitizer's to find */
    const size_t n = 2, E = 2;
    uint64_t* bits = (uint64_t*)malloc(n * 4 * E * 8);
    uint64_t* est = (uint64_t*)malloc(n * 4 * 8);
    uint8_t* choice = (uint8_t*)malloc(n);
    size_t* res = (size_t*)malloc(n * sizeof(size_t));
    uint64_t* off = (uint64_t*)malloc((n + 1) * 8);
    uint8_t* src = (uint8_t*)malloc(64);
    const size_t need = FSEHIP_planes_estimate_workspaceBound(n, (unsigned)E, 15);
    uint8_t* room = (uint8_t*)malloc(need + 256);
    CHECK(bits && est && choice && res && off && src && room, "malloc");
    uint8_t* ws = (uint8_t*)(((uintptr_t)room + 255) & ~(uintptr_t)255);
    memset(bits, 0xF9, n * 4 * E * 8); memset(est, 0xF9, n * 4 * 8); memset(choice, 0xF9, n); memset(res, 0xF9, n * sizeof(size_t));
    memset(src, 7, 64); memset(room, 0xA5, need + 256);
    off[0] = 0; off[1] = 30; off[2] = 64;
#define EST(pb, pe, pc, pr, ps, pbase, po, nn, ee, cap, mask, margin, w, wb) \
    FSEHIP_planes_estimate_dbatch(pb, pe, pc, pr, ps, pbase, po, nn, ee, cap, mask, margin, w, wb, NULL)
    CHECK(EST(NULL, est, choice, res, src, src, off, n, 2, 64, 15, 50, ws, need) == INVALID, "null plane bits");
    CHECK(EST(bits, NULL, choice, res, src, src, off, n, 2, 64, 15, 50, ws, need) == INVALID, "null estimates");
    CHECK(EST(bits, est, NULL, res, src, src, off, n, 2, 64, 15, 50, ws, need) == INVALID, "null choice");
    CHECK(EST(bits, est, choice, NULL, src, src, off, n, 2, 64, 15, 50, ws, need) == INVALID, "null results");
    CHECK(EST(bits, est, choice, res, NULL, src, off, n, 2, 64, 15, 50, ws, need) == INVALID, "null source");
    CHECK(EST(bits, est, choice, res, src, src, NULL, n, 2, 64, 15, 50, ws, need) == INVALID, "null offsets");
    CHECK(EST(bits, est, choice, res, src, src, off, n, 2, 64, 0, 50, ws, need) == INVALID, "mask 0");
    CHECK(EST(bits, est, choice, res, src, src, off, n, 2, 64, 16, 50, ws, need) == INVALID, "an unknown bit");
    CHECK(EST(bits, est, choice, res, src, NULL, off, n, 2, 64, 4, 50, ws, need) == INVALID, "XOR without a base");
    CHECK(EST(bits, est, choice, res, src, NULL, off, n, 2, 64, 9, 50, ws, need) == INVALID, "SUB without a base");
    CHECK(EST(bits, est, choice, res, src, src, off, n, 3, 64, 15, 50, ws, need) == INVALID, "elemBytes 3");
    CHECK(EST(bits, est, choice, res, src, src, off, n, 2, 64, 15, 1001, ws, need) == INVALID, "margin 1001");
    CHECK(EST(bits, est, choice, res, src, src, off, n, 2, 64, 15, 50, ws, need - 1) == INVALID, "a short workspace");
    CHECK(EST(bits, est, choice, res, src, src, off, n, 2, 64, 15, 50, NULL, need) == INVALID, "no workspace");
    CHECK(EST(bits, est, choice, res, src, src, off, n, 2, 64, 15, 50, ws + 8, need) == INVALID, "a misaligned workspace");
    CHECK(EST(bits, est, choice, res, src, src, off, (size_t)1 << 24, 2, 64, 15, 50, ws, need) == INVALID, "2^24 tensors");
    CHECK(EST(bits, est, choice, res, src, src, off, n, 2, (uint64_t)1 << 46, 15, 50, ws, need) == INVALID, "a capacity beyond the launch");
    CHECK(EST(bits, est, choice, res, src, NULL, off, 0, 2, 64, 3, 50, NULL, 0) == 0, "no tensors: legal, nothing launched");
    for (size_t k = 0; k < n * 4 * E * 8; ++k) CHECK(((uint8_t*)bits)[k] == 0xF9, "plane bits written");
    for (size_t k = 0; k < n * 4 * 8; ++k) CHECK(((uint8_t*)est)[k] == 0xF9, "estimates written");
    for (size_t k = 0; k < n; ++k) CHECK(choice[k] == 0xF9, "choice written");
    for (size_t k = 0; k < n * sizeof(size_t); ++k) CHECK(((uint8_t*)res)[k] == 0xF9, "results written");
    for (size_t k = 0; k < need + 256; ++k) CHECK(room[k] == 0xA5, "workspace written");
    free(bits); free(est); free(choice); free(res); free(off); free(src); free(room);
    puts("san_estimate OK");
    return 0;
}

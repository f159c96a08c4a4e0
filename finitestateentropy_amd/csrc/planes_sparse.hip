// planes_sparse.hip -- SPARSE PLANES (fsehip.h, "sparse planes"): a plane (or a segment of one) of n bytes of which nnz are non-zero goes to
// the frame writers as a bit mask of m = ceil(n / 8) bytes followed by its nnz non-zero bytes, where that is shorter and the plane is sparse
// enough; otherwise as it is.  The sign / exponent plane of a tensor delta is almost all zeros, and an order-0 coder still pushes every one
// of its n symbols through its chains (FSE) or spends a bit on each (Huff0): the content carries the same order-0 information in up to 8x
// fewer symbols, and mask bytes and value bytes fall into blocks with tables of their own.  No frame byte format changes: a content is coded
// into an ordinary .fse frame by the packed writers and read by the packed reader; the transform is one more layer between split and
// writer and between reader and merge, as the delta ops are.  The reader needs no flag: a content shorter than its unit is sparse.
//
//   FSEHIP_sparse_pack_dbatch    : k_sp_count (non-zeros per work item) -> scan -> k_sp_decide (per unit: sparse or dense, its content size)
//                                  -> scan (the content offsets) -> k_sp_pack (masks and compacted values, or the copy of a dense unit)
//   FSEHIP_sparse_expand_dbatch  : k_se_clear -> k_se_count (mask popcount per work item; zero value bytes and padding bits into a flag per
//                                  unit) -> scan -> k_se_verdict (per unit: the reader rule) -> k_se_expand (good units only)
//   FSEHIP_tensor_compress_sparse_dbatch / _seg_sparse_dbatch     : the (delta) split [-> the segments kernel] -> pack -> the packed (mixed) writer
//                                  (planes_compress of planes.hip, with pack in front of its writer)
//   FSEHIP_tensor_decompress_sparse_dbatch / _seg_sparse_dbatch   : the layout of the destination (the split's offsets kernel [and the segments
//                                  kernel]) -> the packed reader into the contents buffer -> expand into the planes buffer [-> the fold] -> merge
//
// Work mapping (the ragged one of planes.hip): a UNIT is the byte range [U[u], U[u + 1]) of a flat buffer; the flat axis is cut into tiles of
// PLANES_TILE bytes, G = ceil(capacity / T) + nUnits work items are launched, and item w takes tile w - u of the unit u that pl_find gives
// it.  Inside a unit the bytes are dealt out by MASK BYTE: byte i belongs to the item in whose tile byte 8 * (i >> 3) lies, so that an item
// owns whole mask bytes -- its share [a, b) of the unit starts at a multiple of 8 and has at most T + 7 bytes.  The items of unit u are
// first(u) .. first(u + 1) - 1 with first(u) = floor(U[u] / T) + u and first(nUnits) = G, so the exclusive scan A of the per-item counts gives
// a unit's count as A[first(u + 1)] - A[first(u)] and an item's first value index inside its unit as A[w] - A[first(u)].  No workgroup waits
// for another: the scans are launches of their own (launch_exscan, the scan of frame_dev.hip).
// A unit with U[u + 1] > capacity or U[u] > U[u + 1] counts as empty (n = 0); every value read from the arrays is checked before it places a
// store, so whatever the arrays hold nothing outside the buffers is written.
#include "planes_dev.h"

namespace {
#define SP_ROUND 4096u                                            // bytes of a unit per round of k_sp_pack / k_sp_count: 16 per thread
#define SE_ROUND 2048u                                            // mask bytes per round of k_se_expand: 8 per thread, 64 unit bytes
static_assert(SP_ROUND == 16 * PL_THREADS && SE_ROUND == 8 * PL_THREADS, "round sizes");

DEV u64 sp_unit_size(const u64* U, size_t u, u64 capacity) { const u64 u0 = U[u], u1 = U[u + 1]; return u0 <= u1 && u1 <= capacity ? u1 - u0 : 0; }
// the first work item of unit u; G for u == nU and for an offset behind the capacity
DEV u64 sp_first(const u64* U, size_t nU, u64 G, size_t u)
{
    if (u >= nU) return G;
    const u64 f = (U[u] >> PL_TILE_LOG) + u;
    return f < G ? f : G;
}
// item w: its unit u (at u0, n bytes) and its share [a, b) of it; false where it has none
struct SpItem { size_t u; u64 u0, n, a, b; };
DEV bool sp_item(const u64* U, size_t nU, u64 capacity, u64 w, SpItem& t)
{
    if (!pl_find(U, nU, w, t.u)) return false;
    const u64 u0 = U[t.u], u1 = U[t.u + 1], lo = (w - t.u) << PL_TILE_LOG;
    if (!(u0 < u1) || u1 > capacity || lo >= u1 || lo + PLANES_TILE <= u0) return false;
    t.u0 = u0; t.n = u1 - u0;
    const u64 ra = lo > u0 ? lo - u0 : 0, rb = (lo + PLANES_TILE < u1 ? lo + PLANES_TILE : u1) - u0;
    t.a = (ra + 7) & ~(u64)7;
    t.b = (rb + 7) & ~(u64)7;
    if (t.b > t.n) t.b = t.n;
    return t.a < t.b;
}
// the top bit of every byte of x that is not zero
DEV u32 sp_nz4(u32 x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }
// ... and those four bits side by side (bits 7, 15, 23, 31 -> 0 .. 3: the products' bit positions are all distinct, no carry)
DEV u32 sp_nib(u32 t) { return (((t >> 7) * 0x00204081u) >> 21) & 0xFu; }
// k <= 16 bytes at p into four dwords, the rest zero: one unaligned 16-byte load for a whole piece
DEV void sp_load16(u32* w, const u8* p, u32 k)
{
    if (k == 16) { __builtin_memcpy(w, p, 16); return; }
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (u32 j = 0; j < 16; ++j)                                  // (unrolled: the dwords stay registers)
        if (j < k) w[j >> 2] |= (u32)p[j] << (8 * (j & 3));
}
// exclusive prefix of v over the PL_THREADS threads of the workgroup (all of them call it), the workgroup's total in `total`: the lane's
// position inside its wave on the DPP path (dev_common.h), the waves' totals through sh[4]
DEV u32 sp_wg_excl(u32 v, u32* sh, u32 tid, u32& total)
{
    const u32 lane = tid & 63u, wv = tid >> 6;
    const u32 incl = group_scan_incl<64, ScanAdd>(v, lane);
    if (lane == 63) sh[wv] = incl;
    __syncthreads();
    u32 base = 0, tot = 0;
#pragma unroll
    for (u32 k = 0; k < PL_THREADS / WAVE; ++k) { const u32 s = sh[k]; base += k < wv ? s : 0; tot += s; }
    __syncthreads();
    total = tot;
    return base + incl - v;
}
DEV u64 sp_wg_sum(u32 v, u32* sh, u32 tid) { u32 total; sp_wg_excl(v, sh, tid, total); return total; }
// `count` bytes staged in LDS at lds[mis ..), mis = the destination's address mod 16, to dst: LDS and destination then share their 16-byte
// grid, so everything between the first and the last boundary goes as aligned 16-byte LDS reads and 16-byte global stores; fewer than 16
// bytes in front and behind go bytewise
DEV void sp_flush(u8* dst, const u8* lds, u32 mis, u32 count, u32 tid)
{
    u8* const base = dst - mis;
    const u32 end = mis + count;
    u32 c0 = (mis + 15u) & ~15u;
    if (c0 > end) c0 = end;
    const u32 c1 = c0 + ((end - c0) & ~15u);
    for (u32 i = mis + tid; i < c0; i += PL_THREADS) base[i] = lds[i];
    for (u32 i = c0 + 16 * tid; i < c1; i += 16 * PL_THREADS) *reinterpret_cast<uint4*>(base + i) = *reinterpret_cast<const uint4*>(lds + i);
    for (u32 i = c1 + tid; i < end; i += PL_THREADS) base[i] = lds[i];
}
// len bytes from s to d, any alignments: bytewise up to a 16-byte boundary of d, unaligned 16-byte loads and aligned stores, a bytewise rest
DEV void sp_copy(u8* d, const u8* s, u64 len, u32 tid)
{
    u64 head = (0 - (u64)(uintptr_t)d) & 15u;
    if (head > len) head = len;
    const u64 nch = (len - head) >> 4, tail = head + 16 * nch;
    for (u64 i = tid; i < head; i += PL_THREADS) d[i] = s[i];
    for (u64 c = tid; c < nch; c += PL_THREADS) { u32 w[4]; __builtin_memcpy(w, s + head + 16 * c, 16); __builtin_memcpy(d + head + 16 * c, w, 16); }
    for (u64 i = tail + tid; i < len; i += PL_THREADS) d[i] = s[i];
}

// ---- pack --------------------------------------------------------------------------------------------------------------------------------
// per work item the non-zero bytes of its share (0 where it has none: every entry is written)
__global__ __launch_bounds__(PL_THREADS) void k_sp_count(u64* cnt, const u8* units, const u64* U, size_t nU, u64 capacity)
{
    __shared__ u32 sh[PL_THREADS / WAVE];
    const u32 tid = threadIdx.x;
    SpItem t;
    u32 c = 0;
    if (sp_item(U, nU, capacity, blockIdx.x, t)) {                // (uniform)
        const u8* const sb = units + t.u0 + t.a;
        const u64 L = t.b - t.a;
        for (u64 pos = 16 * (u64)tid; pos < L; pos += SP_ROUND) {
            u32 w[4];
            sp_load16(w, sb + pos, L - pos < 16 ? (u32)(L - pos) : 16u);
#pragma unroll
            for (int k = 0; k < 4; ++k) c += (u32)__popc(sp_nz4(w[k]));
        }
    }
    const u64 total = sp_wg_sum(c, sh, tid);
    if (tid == 0) cnt[blockIdx.x] = total;
}
// per unit the writer rule over the scanned counts A: its content size into CO (scanned in place afterwards)
__global__ void k_sp_decide(u64* CO, const u64* A, const u64* U, size_t nU, u64 G, u64 capacity, u32 permille)
{
    const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nU) return;
    const u64 n = sp_unit_size(U, u, capacity), f0 = sp_first(U, nU, G, u), f1 = sp_first(U, nU, G, u + 1);
    u64 nnz = f1 >= f0 ? A[f1] - A[f0] : 0;
    if (nnz > n) nnz = n;                                         // (offsets that do not increase: keep c <= n whatever was counted)
    const u64 m = (n + 7) >> 3;
    CO[u] = nnz * 1000 <= n * permille && m + nnz < n ? m + nnz : n;
}
// per work item: the mask bytes and the compacted values of its share of a sparse unit, staged in LDS and flushed in 16-byte pieces, or its
// share of a dense unit copied.  A lane takes 16 bytes a round; its position among the round's values is its wave-prefix (DPP scan) plus
// the totals of the waves in front of it.
__global__ __launch_bounds__(PL_THREADS) void k_sp_pack(u8* contents, const u64* CO, const u64* A, const u8* units, const u64* U, size_t nU, u64 G, u64 capacity)
{
    __shared__ __attribute__((aligned(16))) u8 vals[PLANES_TILE + 32];
    __shared__ __attribute__((aligned(16))) u8 msk[PLANES_TILE / 8 + 32];
    __shared__ u32 sh[PL_THREADS / WAVE];
    const u32 tid = threadIdx.x;
    const u64 w = blockIdx.x;
    SpItem t;
    if (!sp_item(U, nU, capacity, w, t)) return;                  // (uniform, like every return below)
    const u64 co = CO[t.u], co1 = CO[t.u + 1];
    if (co > co1 || co1 > capacity) return;
    const u64 c = co1 - co, m = (t.n + 7) >> 3, L = t.b - t.a;
    const u8* const sb = units + t.u0 + t.a;
    if (c == t.n) { sp_copy(contents + co + t.a, sb, L, tid); return; }
    const u64 f0 = sp_first(U, nU, G, t.u);
    if (c > t.n || c < m || w < f0) return;
    const u64 voff = A[w] - A[f0], nv = c - m;
    if (voff > nv) return;
    u8* const vdst = contents + co + m + voff;
    u8* const mdst = contents + co + (t.a >> 3);
    const u32 vmis = (u32)((uintptr_t)vdst & 15u), mmis = (u32)((uintptr_t)mdst & 15u);
    u32 run = 0;
    for (u32 r0 = 0; r0 < L; r0 += SP_ROUND) {
        const u32 pos = r0 + 16 * tid;
        const u32 k = pos < L ? (L - pos < 16 ? (u32)(L - pos) : 16u) : 0u;
        u32 wv[4] = { 0, 0, 0, 0 };
        if (k) sp_load16(wv, sb + pos, k);
        const u32 z0 = sp_nz4(wv[0]), z1 = sp_nz4(wv[1]), z2 = sp_nz4(wv[2]), z3 = sp_nz4(wv[3]);
        const u32 bits = sp_nib(z0) | (sp_nib(z1) << 4) | (sp_nib(z2) << 8) | (sp_nib(z3) << 12);
        u32 total;
        u32 at = vmis + run + sp_wg_excl((u32)__popc(bits), sh, tid, total);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (bits & (1u << j)) vals[at++] = (u8)(wv[j >> 2] >> (8 * (j & 3)));
        if (k) msk[mmis + (pos >> 3)] = (u8)bits;
        if (k > 8) msk[mmis + (pos >> 3) + 1] = (u8)(bits >> 8);
        run += total;
    }
    __syncthreads();
    if ((u64)run > nv - voff) return;                            // (counted otherwise in the first pass: the units changed in between)
    sp_flush(vdst, vals, vmis, run, tid);
    sp_flush(mdst, msk, mmis, (u32)((L + 7) >> 3), tid);
}

// ---- expand ------------------------------------------------------------------------------------------------------------------------------
// what the reader rule says of unit u before any mask bit is looked at (fsehip.h: the checks in their order)
enum { SE_FAIL = 0, SE_DENSE = 1, SE_SPARSE = 2 };
struct SeUnit { int cls; size_t res; u64 n, c, m, co; };
DEV SeUnit se_unit(const u64* U, size_t u, u64 capacity, const u64* CO, const size_t* CR, u64 contentsCapacity)
{
    SeUnit s;
    s.n = sp_unit_size(U, u, capacity); s.m = (s.n + 7) >> 3; s.co = CO[u]; s.c = 0; s.cls = SE_FAIL;
    const size_t r = CR[u];
    const u64 co1 = CO[u + 1];
    if (is_err(r)) { s.res = r; return s; }
    s.res = FERR(corruption_detected);
    if (s.co > co1 || co1 > contentsCapacity || (u64)r > co1 - s.co) return s;       // (a content that does not lie inside its buffer)
    s.c = r;
    if (s.c == s.n) { s.cls = SE_DENSE; s.res = (size_t)s.n; return s; }
    if (s.c > s.n || s.c < s.m) return s;
    s.cls = SE_SPARSE;
    return s;
}
__global__ void k_se_clear(u32* flags, size_t nU)
{
    const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < nU) flags[u] = 0;
}
// per work item of a sparse candidate: the set bits of its mask bytes; into the unit's flag a set padding bit (the item that holds the
// unit's end) and a zero among its share of the value bytes -- the unit's c - m value bytes are dealt out evenly over the tiles it touches
__global__ __launch_bounds__(PL_THREADS) void k_se_count(u64* cnt, u32* flags, const u8* contents, u64 contentsCapacity, const u64* CO, const size_t* CR, const u64* U,
                                                         size_t nU, u64 capacity)
{
    __shared__ u32 sh[PL_THREADS / WAVE];
    const u32 tid = threadIdx.x;
    const u64 w = blockIdx.x;
    SpItem t;
    u32 pc = 0, bad = 0;
    if (pl_find(U, nU, w, t.u)) {
        const SeUnit s = se_unit(U, t.u, capacity, CO, CR, contentsCapacity);
        const u64 u0 = U[t.u], lo = (w - t.u) << PL_TILE_LOG;
        if (s.cls == SE_SPARSE && lo < u0 + s.n && lo + PLANES_TILE > u0) {             // (uniform; s.n > 0 here)
            const u8* const cb = contents + s.co;
            if (sp_item(U, nU, capacity, w, t)) {
                const u64 mi0 = t.a >> 3, nM = ((t.b + 7) >> 3) - mi0;
                for (u64 pos = 16 * (u64)tid; pos < nM; pos += SP_ROUND) {
                    u32 wv[4];
                    sp_load16(wv, cb + mi0 + pos, nM - pos < 16 ? (u32)(nM - pos) : 16u);
#pragma unroll
                    for (int k = 0; k < 4; ++k) pc += (u32)__popc(wv[k]);
                }
                if (tid == 0 && t.b == s.n && (s.n & 7) && (cb[s.m - 1] >> (s.n & 7))) bad = 1;
            }
            const u64 K = ((u0 + s.n - 1) >> PL_TILE_LOG) - (u0 >> PL_TILE_LOG) + 1, j = (lo >> PL_TILE_LOG) - (u0 >> PL_TILE_LOG);
            const u64 nv = s.c - s.m, share = (nv + K - 1) / K;
            const u64 v0 = j * share < nv ? j * share : nv, v1 = v0 + share < nv ? v0 + share : nv;
            const u8* const vb = cb + s.m;
            for (u64 pos = v0 + 16 * (u64)tid; pos < v1; pos += SP_ROUND) {
                const u32 k = v1 - pos < 16 ? (u32)(v1 - pos) : 16u;
                u32 wv[4];
                sp_load16(wv, vb + pos, k);
                const u32 nz = (u32)__popc(sp_nz4(wv[0])) + (u32)__popc(sp_nz4(wv[1])) + (u32)__popc(sp_nz4(wv[2])) + (u32)__popc(sp_nz4(wv[3]));
                if (nz != k) bad = 1;
            }
            if (bad) atomicOr(&flags[t.u], 1u);
        }
    }
    const u64 total = sp_wg_sum(pc, sh, tid);
    if (tid == 0) cnt[w] = total;
}
// per unit the reader rule: the verdict stands before any unit byte is written
__global__ void k_se_verdict(size_t* UR, const u64* A, const u32* flags, const u64* CO, const size_t* CR, u64 contentsCapacity, const u64* U, size_t nU, u64 G,
                             u64 capacity)
{
    const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nU) return;
    const SeUnit s = se_unit(U, u, capacity, CO, CR, contentsCapacity);
    size_t r = s.res;
    if (s.cls == SE_SPARSE) {
        const u64 f0 = sp_first(U, nU, G, u), f1 = sp_first(U, nU, G, u + 1);
        r = f1 >= f0 && A[f1] - A[f0] == s.c - s.m && flags[u] == 0 ? (size_t)s.n : FERR(corruption_detected);
    }
    UR[u] = r;
}
// per work item of a good unit: a dense content copied, or -- a lane takes 8 mask bytes a round -- 64 unit bytes rebuilt from the mask and
// the round's values, which the workgroup stages in LDS first, and stored in 16-byte pieces
__global__ __launch_bounds__(PL_THREADS) void k_se_expand(u8* units, const size_t* UR, const u64* A, const u8* contents, u64 contentsCapacity, const u64* CO,
                                                          const size_t* CR, const u64* U, size_t nU, u64 G, u64 capacity)
{
    __shared__ __attribute__((aligned(16))) u8 vbuf[8 * SE_ROUND];
    __shared__ u32 sh[PL_THREADS / WAVE];
    const u32 tid = threadIdx.x;
    const u64 w = blockIdx.x;
    SpItem t;
    if (!sp_item(U, nU, capacity, w, t)) return;                  // (uniform, like every return below)
    if (is_err(UR[t.u])) return;
    const SeUnit s = se_unit(U, t.u, capacity, CO, CR, contentsCapacity);
    const u8* const cb = contents + s.co;
    u8* const db = units + t.u0;
    if (s.cls == SE_DENSE) { sp_copy(db + t.a, cb + t.a, t.b - t.a, tid); return; }
    const u64 f0 = sp_first(U, nU, G, t.u);
    if (s.cls != SE_SPARSE || w < f0) return;
    const u64 voff = A[w] - A[f0], nv = s.c - s.m;
    const u64 mi0 = t.a >> 3, nM = ((t.b + 7) >> 3) - mi0;
    const u8* const vb = cb + s.m + voff;
    u64 run = 0;
    for (u32 r0 = 0; r0 < nM; r0 += SE_ROUND) {
        const u32 mi = r0 + 8 * tid;
        const u32 k = mi < nM ? (nM - mi < 8 ? (u32)(nM - mi) : 8u) : 0u;
        u64 mk = 0;
        if (k == 8) __builtin_memcpy(&mk, cb + mi0 + mi, 8);
        else for (u32 j = 0; j < k; ++j) mk |= (u64)cb[mi0 + mi + j] << (8 * j);
        u32 total;
        u32 at = sp_wg_excl((u32)__popcll(mk), sh, tid, total);
        if (voff + run + total > nv) return;                      // (the verdict has counted the same bits: the contents changed in between)
        for (u32 i = 16 * tid; i < total; i += 16 * PL_THREADS) {
            u32 wv[4];
            sp_load16(wv, vb + run + i, total - i < 16 ? total - i : 16u);
            *reinterpret_cast<uint4*>(vbuf + i) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
        }
        __syncthreads();
        if (k) {
            const u64 opos = t.a + 8 * (u64)mi;
            const u32 avail = t.b - opos < 64 ? (u32)(t.b - opos) : 64u;
            u32 o[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                u32 word = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((mk >> (4 * q + j)) & 1) word |= (u32)vbuf[at++] << (8 * j);
                o[q] = word;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                u8* const d = db + opos + 16 * q;
                if (avail >= 16u * (q + 1)) __builtin_memcpy(d, &o[4 * q], 16);
                else {
#pragma unroll
                    for (u32 j = 0; j < 16; ++j)
                        if (16u * q + j < avail) d[j] = (u8)(o[4 * q + (j >> 2)] >> (8 * (j & 3)));
                }
            }
        }
        __syncthreads();
        run += total;
    }
}

// ---- workspace and launches --------------------------------------------------------------------------------------------------------------
inline size_t r256(size_t x) { return (x + 255) & ~(size_t)255; }
// the per-item counts (G + 1 entries, scanned in place), the scan's partial sums (the item scan and, in pack, the unit scan), a flag per unit
struct SpLayout { size_t cnt, partials, flags, total; };
inline SpLayout sp_layout(u64 capacity, size_t nUnits)
{
    const size_t G = tile_grid(capacity, nUnits);
    SpLayout L;
    L.cnt = 0;
    L.partials = L.cnt + r256((G + 1) * 8);
    L.flags = L.partials + r256(exscan_partials(G > nUnits ? G : nUnits) * 8);
    L.total = L.flags + r256(nUnits * 4);
    return L;
}
}   // namespace

// (declared in internal.h: planes_compress of planes.hip puts pack in front of its writer)
size_t sparse_workspace(u64 capacity, size_t nUnits) { return sp_layout(capacity, nUnits).total; }
bool bad_sparse(u64 capacity, size_t nUnits, const void* d_workspace, size_t workspaceBytes)
{
    return nUnits >= ((size_t)1 << 31) || bad_grid(capacity, nUnits) || !d_workspace || ((uintptr_t)d_workspace & 255u) || workspaceBytes < sp_layout(capacity, nUnits).total;
}

hipError_t launch_sparse_pack(u8* contents, u64* contentOff, const u8* units, const u64* unitOff, size_t nUnits, u64 capacity, unsigned permille, u8* ws, hipStream_t s)
{
    const SpLayout L = sp_layout(capacity, nUnits);
    u64* const cnt = (u64*)(ws + L.cnt), * const partials = (u64*)(ws + L.partials);
    const unsigned G = tile_grid(capacity, nUnits);
    if (nUnits == 0 || G == 0) return launch_exscan(contentOff, 0, partials, s);
    hipLaunchKernelGGL(k_sp_count, dim3(G), dim3(PL_THREADS), 0, s, cnt, units, unitOff, nUnits, capacity);
    hipError_t e = launch_exscan(cnt, G, partials, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sp_decide, dim3(grid_for(nUnits)), dim3(PL_THREADS), 0, s, contentOff, (const u64*)cnt, unitOff, nUnits, (u64)G, capacity, (u32)permille);
    e = launch_exscan(contentOff, nUnits, partials, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sp_pack, dim3(G), dim3(PL_THREADS), 0, s, contents, (const u64*)contentOff, (const u64*)cnt, units, unitOff, nUnits, (u64)G, capacity);
    return hipGetLastError();
}

namespace {
hipError_t launch_sparse_expand(u8* units, size_t* unitRes, const u64* unitOff, size_t nUnits, u64 capacity, const u8* contents, u64 contentsCapacity,
                                const u64* contentOff, const size_t* contentRes, u8* ws, hipStream_t s)
{
    if (nUnits == 0) return hipSuccess;
    const SpLayout L = sp_layout(capacity, nUnits);
    u64* const cnt = (u64*)(ws + L.cnt), * const partials = (u64*)(ws + L.partials);
    u32* const flags = (u32*)(ws + L.flags);
    const unsigned G = tile_grid(capacity, nUnits);
    hipLaunchKernelGGL(k_se_clear, dim3(grid_for(nUnits)), dim3(PL_THREADS), 0, s, flags, nUnits);
    hipLaunchKernelGGL(k_se_count, dim3(G), dim3(PL_THREADS), 0, s, cnt, flags, contents, contentsCapacity, contentOff, contentRes, unitOff, nUnits, capacity);
    const hipError_t e = launch_exscan(cnt, G, partials, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_se_verdict, dim3(grid_for(nUnits)), dim3(PL_THREADS), 0, s, unitRes, (const u64*)cnt, (const u32*)flags, contentOff, contentRes, contentsCapacity,
                       unitOff, nUnits, (u64)G, capacity);
    hipLaunchKernelGGL(k_se_expand, dim3(G), dim3(PL_THREADS), 0, s, units, (const size_t*)unitRes, (const u64*)cnt, contents, contentsCapacity, contentOff, contentRes,
                       unitOff, nUnits, (u64)G, capacity);
    return hipGetLastError();
}

// The decompress path of both sparse composites behind their pointer checks: the dense layout from the destination's slots (a tensor's size IS its slot), the packed reader into the
// contents buffer, expand into the planes buffer, the fold where d_segFirst is given, the merge
int sparse_decompress(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp, size_t* d_results, const void* d_frames,
                      const uint64_t* d_frameOffsets, size_t nTensors, unsigned E, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks,
                      void* d_contents, uint64_t contentsCapacity, uint64_t* d_contentOffsets, size_t* d_contentResults, void* d_planes, uint64_t planesCapacity,
                      uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets, size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_op(deltaOp)) return (int)hipErrorInvalidValue;
    if (d_segFirst ? bad_seg(segLog, 0) || bad_counts(nTensors, E, nSegments) : bad_tensors(nTensors, E)) return (int)hipErrorInvalidValue;
    const size_t nFrames = d_segFirst ? nSegments : nTensors * E;
    const u64 cap = dstCapacity < planesCapacity ? dstCapacity : planesCapacity;
    if (bad_grid(dstCapacity, nTensors) || bad_sparse(cap, nFrames, d_workspace, workspaceBytes)) return (int)hipErrorInvalidValue;
    const size_t head = sp_layout(cap, nFrames).total;
    u8* const ws = (u8*)d_workspace;
    if (bad_reader(ws + head, workspaceBytes - head, nFrames, maxTotalBlocks)) return (int)hipErrorInvalidValue;
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = launch_planes_offsets((u64*)d_planeOffsets, d_results, (const u64*)d_dstOffsets, nTensors, E, cap, s);
    if (e == hipSuccess && d_segFirst)
        e = launch_segments((u64*)d_segOffsets, d_results, (const u64*)d_planeOffsets, (const u64*)d_dstOffsets, (const u64*)d_segFirst, nTensors, E, nSegments, segLog, s);
    if (e != hipSuccess) return (int)e;
    const int r = FSEHIP_frame_decompress_packed_dbatch(d_contents, (size_t)contentsCapacity, d_contentOffsets, d_contentResults, d_frames, d_frameOffsets, nFrames,
                                                        maxTotalBlocks, 0, ws + head, workspaceBytes - head, stream);
    if (r != 0) return r;
    e = launch_sparse_expand((u8*)d_planes, d_segFirst ? d_segResults : d_planeSizes, (const u64*)(d_segFirst ? d_segOffsets : d_planeOffsets), nFrames, cap,
                             (const u8*)d_contents, contentsCapacity, (const u64*)d_contentOffsets, d_contentResults, ws, s);
    if (e != hipSuccess) return (int)e;
    if (d_segFirst) {
        const int f = FSEHIP_planes_fold_segments_dbatch(d_planeOffsets, d_planeSizes, d_segOffsets, d_segResults, d_segFirst, nTensors * E, nSegments, segLog, stream);
        if (f != 0) return f;
    }
    return (int)launch_planes_merge((u8*)d_dst, (const u64*)d_dstOffsets, d_results, (const u8*)d_planes, (const u64*)d_planeOffsets, d_planeSizes, (const u8*)d_base,
                                    deltaOp, nTensors, E, dstCapacity, s);
}
}   // namespace

extern "C" size_t FSEHIP_sparse_workspaceBound(uint64_t capacity, size_t nUnits)
{
    if (nUnits >= ((size_t)1 << 31) || bad_grid(capacity, nUnits)) return FSEHIP_ERROR(GENERIC);
    return sp_layout(capacity, nUnits).total;
}

extern "C" int FSEHIP_sparse_pack_dbatch(void* d_contents, uint64_t* d_contentOffsets, const void* d_units, const uint64_t* d_unitOffsets, size_t nUnits, uint64_t capacity,
                                         unsigned sparsePermille, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (sparsePermille > 1000 || !d_contents || !d_contentOffsets || !d_units || !d_unitOffsets || bad_sparse(capacity, nUnits, d_workspace, workspaceBytes))
        return (int)hipErrorInvalidValue;
    return (int)launch_sparse_pack((u8*)d_contents, (u64*)d_contentOffsets, (const u8*)d_units, (const u64*)d_unitOffsets, nUnits, capacity, sparsePermille, (u8*)d_workspace,
                                   (hipStream_t)stream);
}

extern "C" int FSEHIP_sparse_expand_dbatch(void* d_units, size_t* d_unitResults, const uint64_t* d_unitOffsets, size_t nUnits, uint64_t capacity, const void* d_contents,
                                           uint64_t contentsCapacity, const uint64_t* d_contentOffsets, const size_t* d_contentResults, void* d_workspace,
                                           size_t workspaceBytes, void* stream)
{
    if (!d_units || !d_unitResults || !d_unitOffsets || !d_contents || !d_contentOffsets || !d_contentResults || bad_sparse(capacity, nUnits, d_workspace, workspaceBytes))
        return (int)hipErrorInvalidValue;
    return (int)launch_sparse_expand((u8*)d_units, d_unitResults, (const u64*)d_unitOffsets, nUnits, capacity, (const u8*)d_contents, contentsCapacity,
                                     (const u64*)d_contentOffsets, d_contentResults, (u8*)d_workspace, (hipStream_t)stream);
}

extern "C" int FSEHIP_tensor_compress_sparse_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                    const void* d_src, const void* d_base, unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors,
                                                    unsigned elemBytes, uint64_t capacity, size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs,
                                                    int policy, unsigned tolerancePermille, unsigned slotAlignLog, unsigned sparsePermille, void* d_planes,
                                                    uint64_t* d_planeOffsets, void* d_contents, uint64_t* d_contentOffsets, void* d_workspace, size_t workspaceBytes,
                                                    void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_srcOffsets || !d_planeOffsets || !d_contents || !d_contentOffsets ||
        ((elemBytes > 1 || d_base) && !d_planes))
        return (int)hipErrorInvalidValue;
    const PlSparse sparse = { sparsePermille, d_contents, d_contentOffsets };
    return planes_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, deltaOp, d_srcOffsets, nTensors, elemBytes, capacity, nullptr, 0,
                           0, d_planes, d_planeOffsets, nullptr,
                           PlWriter{ maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes }, stream, &sparse);
}

extern "C" int FSEHIP_tensor_compress_seg_sparse_dbatch(void* d_dst, uint64_t dstCapacity, uint64_t* d_frameOffsets, size_t* d_frameResults, size_t* d_tensorResults,
                                                        const void* d_src, const void* d_base, unsigned deltaOp, const uint64_t* d_srcOffsets, size_t nTensors,
                                                        unsigned elemBytes, uint64_t capacity, const uint64_t* d_segFirst, size_t nSegments, unsigned segLog,
                                                        size_t maxTotalBlocks, unsigned blockSizeId, int codec, uint8_t* d_codecs, int policy, unsigned tolerancePermille,
                                                        unsigned slotAlignLog, unsigned sparsePermille, void* d_planes, uint64_t* d_planeOffsets, uint64_t* d_segOffsets,
                                                        void* d_contents, uint64_t* d_contentOffsets, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_frameOffsets || !d_frameResults || !d_tensorResults || !d_src || !d_srcOffsets || !d_segFirst || !d_planeOffsets || !d_segOffsets ||
        !d_contents || !d_contentOffsets || ((elemBytes > 1 || d_base) && !d_planes))
        return (int)hipErrorInvalidValue;
    const PlSparse sparse = { sparsePermille, d_contents, d_contentOffsets };
    return planes_compress(d_dst, dstCapacity, d_frameOffsets, d_frameResults, d_tensorResults, d_src, d_base, deltaOp, d_srcOffsets, nTensors, elemBytes, capacity, d_segFirst,
                           nSegments, segLog, d_planes, d_planeOffsets, d_segOffsets,
                           PlWriter{ maxTotalBlocks, blockSizeId, codec, d_codecs, policy, tolerancePermille, slotAlignLog, d_workspace, workspaceBytes }, stream, &sparse);
}

extern "C" int FSEHIP_tensor_decompress_sparse_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp,
                                                      size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                      size_t maxTotalBlocks, void* d_contents, uint64_t contentsCapacity, uint64_t* d_contentOffsets,
                                                      size_t* d_contentResults, void* d_planes, uint64_t planesCapacity, uint64_t* d_planeOffsets, size_t* d_planeResults,
                                                      void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_frames || !d_frameOffsets || !d_contents || !d_contentOffsets || !d_contentResults || !d_planes ||
        !d_planeOffsets || !d_planeResults)
        return (int)hipErrorInvalidValue;
    return sparse_decompress(d_dst, d_dstOffsets, dstCapacity, d_base, deltaOp, d_results, d_frames, d_frameOffsets, nTensors, elemBytes, nullptr, 0, 0, maxTotalBlocks,
                             d_contents, contentsCapacity, d_contentOffsets, d_contentResults, d_planes, planesCapacity, nullptr, nullptr, d_planeOffsets, d_planeResults,
                             d_workspace, workspaceBytes, stream);
}

extern "C" int FSEHIP_tensor_decompress_seg_sparse_dbatch(void* d_dst, const uint64_t* d_dstOffsets, uint64_t dstCapacity, const void* d_base, unsigned deltaOp,
                                                          size_t* d_results, const void* d_frames, const uint64_t* d_frameOffsets, size_t nTensors, unsigned elemBytes,
                                                          const uint64_t* d_segFirst, size_t nSegments, unsigned segLog, size_t maxTotalBlocks, void* d_contents,
                                                          uint64_t contentsCapacity, uint64_t* d_contentOffsets, size_t* d_contentResults, void* d_planes,
                                                          uint64_t planesCapacity, uint64_t* d_segOffsets, size_t* d_segResults, uint64_t* d_planeOffsets,
                                                          size_t* d_planeSizes, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (bad_elem(elemBytes) || !d_dst || !d_dstOffsets || !d_results || !d_frames || !d_frameOffsets || !d_segFirst || !d_contents || !d_contentOffsets ||
        !d_contentResults || !d_planes || !d_segOffsets || !d_segResults || !d_planeOffsets || !d_planeSizes)
        return (int)hipErrorInvalidValue;
    return sparse_decompress(d_dst, d_dstOffsets, dstCapacity, d_base, deltaOp, d_results, d_frames, d_frameOffsets, nTensors, elemBytes, d_segFirst, nSegments, segLog,
                             maxTotalBlocks, d_contents, contentsCapacity, d_contentOffsets, d_contentResults, d_planes, planesCapacity, d_segOffsets, d_segResults,
                             d_planeOffsets, d_planeSizes, d_workspace, workspaceBytes, stream);
}

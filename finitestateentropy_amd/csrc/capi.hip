// capi.hip -- the common ground of the C ABI of libfsehip.so (include/fsehip.h): error names, device properties, the kernel timing probe,
// the workload generator, per-block argument errors and the packed form of a batch.  The batched calls on device pointers are in
// capi_batch.hip, the single-block calls on host pointers in capi_host.hip.  No CPU compute path exists: every result is produced by a
// kernel; without a usable device the calls fail.
#include "internal.h"
#include <string.h>
#include <stdlib.h>
#include <new>

extern "C" unsigned FSEHIP_isError(size_t code) { return code > FSEHIP_ERROR(maxCode); }

extern "C" const char* FSEHIP_getErrorName(size_t code)   // lib/error_private.h:88-104
{
    if (!FSEHIP_isError(code)) return "No error detected";
    switch ((int)(0 - code)) {
        case FSEHIP_error_GENERIC: return "Error (generic)";
        case FSEHIP_error_dstSize_tooSmall: return "Destination buffer is too small";
        case FSEHIP_error_srcSize_wrong: return "Src size is incorrect";
        case FSEHIP_error_corruption_detected: return "Corrupted block detected";
        case FSEHIP_error_tableLog_tooLarge: return "tableLog requires too much memory : unsupported";
        case FSEHIP_error_maxSymbolValue_tooLarge: return "Unsupported max Symbol Value : too large";
        case FSEHIP_error_maxSymbolValue_tooSmall: return "Specified maxSymbolValue is too small";
        case FSEHIP_error_workSpace_tooSmall: return "workspace buffer is too small";
        default: return "Unspecified error code";
    }
}

extern "C" const char* FSEHIP_versionString(void) { return "fsehip 0.3 (gfx950)"; }

extern "C" void FSEHIP_shardRange(size_t nBlocks, int rank, int world, size_t* first, size_t* count)   // = shard.shard_range
{
    if (world < 1) world = 1;
    if (rank < 0) rank = 0;
    const size_t base = nBlocks / (size_t)world, rem = nBlocks % (size_t)world, r = (size_t)rank;
    const size_t lo = r * base + (r < rem ? r : rem);
    if (first) *first = lo;
    if (count) *count = r < (size_t)world ? base + (r < rem ? 1 : 0) : 0;
}

// Per-device caches (a process may drive several devices: the attribute and the CU count belong to the current one),
// guarded for concurrent host threads.
#include <mutex>
#include <vector>
#include <utility>
namespace {
std::mutex g_devMutex;
const int MAX_DEVS = 64;
DevProps g_props[MAX_DEVS];
std::vector<std::pair<int, const void*>> g_ldsAttrDone;      // (device, kernel) pairs already configured
}
const DevProps& dev_props()
{
    static const DevProps none = { 0, 0, false };
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVS) return none;
    std::lock_guard<std::mutex> lock(g_devMutex);
    DevProps& p = g_props[dev];
    if (!p.ok) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
            p.cus = prop.multiProcessorCount;
            p.ldsPerCU = (int)prop.maxSharedMemoryPerMultiProcessor;
            p.ok = true;
        }
    }
    return p;
}
hipError_t ensure_dyn_lds(const void* kernel, int bytes)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_devMutex);
    for (auto& d : g_ldsAttrDone) if (d.first == dev && d.second == kernel) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) g_ldsAttrDone.emplace_back(dev, kernel);
    return e;
}

extern "C" int FSEHIP_deviceInfo(FSEHIP_DeviceInfo* info)
{
    int dev = 0;
    hipDeviceProp_t prop;
    CK(hipGetDevice(&dev));
    CK(hipGetDeviceProperties(&prop, dev));
    info->deviceOrdinal = dev;
    info->computeUnits = prop.multiProcessorCount;
    info->ldsBytesPerCU = (int)prop.maxSharedMemoryPerMultiProcessor;
    info->wavefrontSize = prop.warpSize;
    strncpy(info->archName, prop.gcnArchName, sizeof(info->archName) - 1);
    info->archName[sizeof(info->archName) - 1] = 0;
    return 0;
}

// ---- kernel timing probe ------------------------------------------------------------------------------
namespace {
std::mutex g_probeMutex;
struct Probe {
    bool on = false;
    std::vector<hipEvent_t> pool;            // reusable events
    size_t used = 0;
    struct Rec { int id; hipEvent_t a, b; };
    std::vector<Rec> recs;
    hipEvent_t pending[PK_COUNT] = {};
    hipEvent_t get()
    {
        if (used == pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; pool.push_back(e); }
        return pool[used++];
    }
} g_probe;
}
void probe_before(int id, hipStream_t s)
{
    if (!g_probe.on) return;
    std::lock_guard<std::mutex> lock(g_probeMutex);
    hipEvent_t e = g_probe.get();
    g_probe.pending[id] = e;
    if (e) (void)hipEventRecord(e, s);
}
void probe_after(int id, hipStream_t s)
{
    if (!g_probe.on) return;
    std::lock_guard<std::mutex> lock(g_probeMutex);
    hipEvent_t e = g_probe.get();
    if (e && g_probe.pending[id]) { (void)hipEventRecord(e, s); g_probe.recs.push_back({ id, g_probe.pending[id], e }); }
}
extern "C" int FSEHIP_probe_begin(void)
{
    std::lock_guard<std::mutex> lock(g_probeMutex);
    g_probe.on = true; g_probe.used = 0; g_probe.recs.clear();
    return 0;
}
extern "C" int FSEHIP_probe_collect(double* totalMs, unsigned* launches)
{
    for (int i = 0; i < 16; ++i) { totalMs[i] = 0; launches[i] = 0; }
    std::lock_guard<std::mutex> lock(g_probeMutex);
    g_probe.on = false;
    for (auto& r : g_probe.recs) {
        CK(hipEventSynchronize(r.b));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, r.a, r.b));
        totalMs[r.id] += ms; launches[r.id] += 1;
    }
    g_probe.recs.clear(); g_probe.used = 0;
    return 0;
}

// =====================================================================================================
//  workload generator
// =====================================================================================================
extern "C" void FSEHIP_probagen_table(uint8_t table[4096], double p)   // programs/probaGenerator.c:95-118
{
    int remaining = 4096;
    unsigned pos = 0, s = 0;
    if (p == 0.0) p = 0.005;
    while (remaining) {
        unsigned n = (unsigned)(remaining * p);
        if (!n) n = 1;
        memset(table + pos, (int)(uint8_t)s, n);
        pos += n; s++; remaining -= (int)n;
    }
}

extern "C" int FSEHIP_probagen_batch(void* d_dst, size_t dstStride, size_t blockSize, size_t nBlocks,
                                     const uint8_t h_table[4096], uint32_t firstSeed, void* stream)
{
    return FSEHIP_probagen_batch_ex(d_dst, dstStride, blockSize, nBlocks, h_table, firstSeed, 1, stream);
}
extern "C" int FSEHIP_probagen_batch_ex(void* d_dst, size_t dstStride, size_t blockSize, size_t nBlocks,
                                        const uint8_t h_table[4096], uint32_t firstSeed, uint32_t seedStep, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    // The 4 KiB table goes through a small per-thread, per-device ring of slots (device memory + pinned staging, allocated once): no
    // hipMalloc / hipFree and no host synchronisation per call.  h_table is consumed before the call returns (host copy into
    // the pinned slot); a slot is reused 16 calls later, after the event recorded behind the kernel that read it.
    enum { SLOTS = 16 };
    struct Ring { u8* dev = nullptr; u8* pin = nullptr; int device = -1; unsigned next = 0; hipEvent_t ev[SLOTS] = {}; bool used[SLOTS] = {}; int nEv = 0;
                  void drop() { for (int i = 0; i < nEv; ++i) (void)hipEventDestroy(ev[i]); nEv = 0;
                                if (pin) (void)hipHostFree(pin); if (dev) (void)hipFree(dev); pin = nullptr; dev = nullptr; device = -1; (void)hipGetLastError(); } };
    struct Rings { std::vector<Ring> v; ~Rings() { for (auto& r : v) r.drop(); } };
    static thread_local Rings rings;                              // one ring per device the thread has generated on
    int dev = 0;
    CK(hipGetDevice(&dev));
    Ring* rp = nullptr;
    for (auto& r : rings.v) if (r.device == dev) rp = &r;
    if (!rp) {
        Ring r;
        hipError_t e = hipMalloc((void**)&r.dev, SLOTS * 4096);
        if (e == hipSuccess) e = hipHostMalloc((void**)&r.pin, SLOTS * 4096, hipHostMallocDefault);
        for (int i = 0; i < SLOTS && e == hipSuccess; ++i) { e = hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming); if (e == hipSuccess) r.nEv = i + 1; }
        if (e != hipSuccess) { r.drop(); return (int)e; }         // nothing half-built is kept
        r.device = dev;
        rings.v.push_back(r);
        rp = &rings.v.back();
    }
    Ring& ring = *rp;
    const unsigned k = ring.next++ % SLOTS;
    if (ring.used[k]) CK(hipEventSynchronize(ring.ev[k]));
    memcpy(ring.pin + 4096u * k, h_table, 4096);
    u8* const d_table = ring.dev + 4096u * k;
    hipError_t e = hipMemcpyAsync(d_table, ring.pin + 4096u * k, 4096, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_probagen((u8*)d_dst, dstStride, blockSize, nBlocks, d_table, firstSeed, seedStep, s);
    if (e == hipSuccess) { e = hipEventRecord(ring.ev[k], s); ring.used[k] = e == hipSuccess; }
    return (int)e;
}

// Argument errors of the one-shot calls are per-block results, like everything else the reference call would return for
// block b (include/fsehip.h): the batch call itself still succeeds.
//   mode 0 (FSE_compress2, lib/fse_compress.c:691): every block gets `code`;
//   mode 1 (HUF_compress_internal, lib/huf_compress.c:654-660): srcSize 0 or dstCapacity 0 -> 0, srcSize > HUF_BLOCKSIZE_MAX ->
//          srcSize_wrong come first, then `code`;
//   mode 2 (FSE_compress_wksp, lib/fse_compress.c:646-650): srcSize <= 1 -> 0 comes first, then `code`.
__global__ void k_batch_arg_error(size_t* results, const size_t* sizes, size_t uniform, size_t dstCapacity, size_t nBlocks, size_t code, int mode)
{
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nBlocks) return;
    size_t r = code;
    if (mode == 1) {
        const size_t n = sizes ? sizes[b] : uniform;
        if (n == 0 || dstCapacity == 0) r = 0;
        else if (n > FSEHIP_HUF_BLOCKSIZE_MAX) r = FERR(srcSize_wrong);
    }
    if (mode == 2) { const size_t n = sizes ? sizes[b] : uniform; if (n <= 1) r = 0; }
    results[b] = r;
}
int batch_arg_error(size_t* d_results, const size_t* d_sizes, size_t uniform, size_t dstCapacity, size_t nBlocks, size_t code, int mode, hipStream_t s)
{
    hipLaunchKernelGGL(k_batch_arg_error, dim3((unsigned)((nBlocks + 255) / 256)), dim3(256), 0, s, d_results, d_sizes, uniform, dstCapacity, nBlocks, code, mode);
    return (int)hipGetLastError();
}

// results[b] = the header size for every block a prepare kernel left pending: the table-building batch calls (capi_batch.hip)
__global__ void k_hdr_results(const u8* meta, size_t metaStride, size_t* results, size_t nBlocks)
{
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nBlocks) return;
    const u32* const m = (const u32*)(meta + b * metaStride);            // {state, hdrSize, ...} in FseMeta and HufMeta alike
    if (m[0] != 0) results[b] = m[1];
}
hipError_t launch_hdr_results(const void* meta, size_t metaStride, size_t* results, size_t nBlocks, hipStream_t s)
{
    hipLaunchKernelGGL(k_hdr_results, dim3((unsigned)((nBlocks + 255) / 256)), dim3(256), 0, s, (const u8*)meta, metaStride, results, nBlocks);
    return hipGetLastError();
}

// =====================================================================================================
//  Packed (variable-length) form of a batch of compressed blocks -- compact.hip
// =====================================================================================================
extern "C" size_t FSEHIP_compact_batch_workspaceSize(size_t nBlocks) { return ((nBlocks + 1023) / 1024 + 2) * sizeof(u64) + 256; }
extern "C" size_t FSEHIP_compact_batch_bound(size_t nBlocks, size_t blockSize) { return nBlocks * blockSize; }
extern "C" int FSEHIP_compact_batch(void* d_packed, size_t packedCapacity, uint64_t* d_offsets, const void* d_slots, size_t slotStride, const size_t* d_results,
                                    const void* d_src, size_t srcStride, const size_t* d_srcSizes, size_t uniformSrcSize, size_t nBlocks,
                                    void* d_workspace, size_t workspaceBytes, void* stream)
{
    if ((uintptr_t)d_workspace & 255u) return (int)hipErrorInvalidValue;
    if (workspaceBytes < FSEHIP_compact_batch_workspaceSize(nBlocks)) return (int)hipErrorInvalidValue;
    return (int)launch_compact((u8*)d_packed, packedCapacity, (u64*)d_offsets, (const u8*)d_slots, slotStride, d_results,
                               mkview(d_src, srcStride, d_srcSizes, uniformSrcSize), nBlocks, (u64*)d_workspace, (hipStream_t)stream);
}

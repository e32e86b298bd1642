// vt_api.hip -- the C ABI of include/voltools_hip.h (hipMalloc / hipMemcpyAsync / kernel launches).
#include "vt_internal.h"
#include "vt_device.h"
#include "vt_host.h"

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#include <unistd.h>

using namespace vt;

// ---- VT_DEBUG_GUARD=1: every device allocation of this library gets 1 MiB of NaN (0xFF bytes) in front of it and behind
// it.  A kernel that reads out of bounds then produces NaN (parity tests fail instead of passing on whatever the neighbouring
// allocation held, or faulting when the neighbour has been freed); one that writes out of bounds is caught when the buffer
// is released (message + abort).  A poor man's address sanitizer for the GPU side (the real one is not available here). ----
namespace vt_guard {
constexpr size_t kGuard = (size_t)1 << 20;
struct Entry { void* base; size_t bytes; };
static std::mutex mu;
static std::unordered_map<void*, Entry> live;
static bool enabled()
{
    static const bool on = std::getenv("VT_DEBUG_GUARD") != nullptr;
    return on;
}
static hipError_t alloc(void** p, size_t bytes)
{
    if (!enabled()) return hipMalloc(p, bytes);
    char* base = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&base), bytes + 2 * kGuard);
    if (e != hipSuccess) return e;
    (void)hipMemset(base, 0xFF, kGuard);
    (void)hipMemset(base + kGuard + bytes, 0xFF, kGuard);
    (void)hipDeviceSynchronize();
    *p = base + kGuard;
    std::lock_guard<std::mutex> lk(mu);
    live[*p] = Entry{base, bytes};
    return hipSuccess;
}
static hipError_t release(void* p)
{
    if (!enabled() || !p) return hipFree(p);
    Entry en{nullptr, 0};
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it == live.end()) return hipFree(p);
        en = it->second;
        live.erase(it);
    }
    (void)hipDeviceSynchronize();
    std::vector<unsigned char> h(2 * kGuard);
    (void)hipMemcpy(h.data(), en.base, kGuard, hipMemcpyDeviceToHost);
    (void)hipMemcpy(h.data() + kGuard, static_cast<char*>(en.base) + kGuard + en.bytes, kGuard, hipMemcpyDeviceToHost);
    for (size_t i = 0; i < 2 * kGuard; ++i)
        if (h[i] != 0xFF) {
            std::fprintf(stderr, "[vt guard] out-of-bounds WRITE %s a device buffer of %zu bytes (guard offset %zu)\n",
                         i < kGuard ? "in front of" : "behind", en.bytes, i < kGuard ? kGuard - i : i - kGuard);
            std::fflush(stderr);
            std::abort();
        }
    return hipFree(en.base);
}
}  // namespace vt_guard
#define hipMalloc(p, n) vt_guard::alloc(reinterpret_cast<void**>(p), (n))
#define hipFree(p) vt_guard::release(p)

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define VT_HIP(call)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (void)hipGetLastError();   /* the runtime's last-error is sticky: a failure reported here must not resurface at the next launch check */ \
            return fail((int)e_, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
        }                                                                                          \
    } while (0)

int use_device(int dev)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(VT_ENODEV, "no HIP device available (%s)", hipGetErrorString(e));
    if (dev < 0 || dev >= n) return fail(VT_ENODEV, "device index %d out of range (0..%d)", dev, n - 1);
    VT_HIP(hipSetDevice(dev));
    return 0;
}

std::once_flag g_init_flag[64];
hipError_t g_init_err[64];
// per-device constants, fetched once (hipGetDeviceProperties and a hipMalloc per handle were a visible part of the
// ~0.4 ms a one-shot transform of a tiny volume costs)
int g_cu_count[64], g_lds_limit[64];
float* g_zeros[64];                // 256 bytes of zeros per device: the border fetch target of the tiled kernels (never freed)


// ---------------------------------------------------------------------------------------------------
// Per-device recycling of what a handle's life costs besides the copies: a HIP stream, two events and small device buffers.
// A one-shot transform() of a tiny volume spent 0.38 of its 0.43 ms creating and destroying these
// (round-1 measurement).  Streams and events go back to a free list when a handle is destroyed (it synchronises
// first); device buffers up to 64 MiB are kept by exact size, at most 16 of them and 256 MiB in total per device.
// ---------------------------------------------------------------------------------------------------
struct DeviceCache {
    std::mutex mu;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;
    std::vector<std::pair<size_t, void*>> bufs;
    size_t buf_bytes = 0;
    std::vector<std::pair<size_t, void*>> big;     // large buffers, most recently released last
    size_t big_bytes = 0;
    // one-shot pipeline: two NON-blocking copy streams (uploads / downloads), one pipelined call at a time per device
    std::mutex pipe_mu;
    hipStream_t copy_up = nullptr, copy_dn = nullptr, pipe_k = nullptr;
};
DeviceCache g_cache[64];
constexpr size_t kCacheBufMax = (size_t)64 << 20, kCacheTotalMax = (size_t)256 << 20;
// Large buffers (resident sources, result staging) are recycled too, a few of them: a transfer to or from a device
// allocation only reaches full PCIe duplex from its third pass on ([measured, round 1] 512 MiB up + down
// through a buffer from hipMalloc 19.4, 18.0, then 11.7 ms; a buffer allocated per call never gets there), so a one-shot
// transform() that allocated its buffers per call could not overlap its upload with its download.  With 288 GB of HBM the
// cache may hold 16 GiB; vt_device_trim releases it.
constexpr size_t kBigBufMax = (size_t)8 << 30, kBigTotalMax = (size_t)16 << 30;
constexpr size_t kBigCount = 6;

hipError_t cached_stream(int dev, hipStream_t* s)
{
    if (dev < 64) {
        std::lock_guard<std::mutex> lk(g_cache[dev].mu);
        if (!g_cache[dev].streams.empty()) { *s = g_cache[dev].streams.back(); g_cache[dev].streams.pop_back(); return hipSuccess; }
    }
    // a blocking stream: ordered against the legacy null stream (torch's default), like the reference, which does
    // everything on cupy's null stream (transforms.py:168, volume.py:66)
    return hipStreamCreateWithFlags(s, hipStreamDefault);
}
void recycle_stream(int dev, hipStream_t s)
{
    if (dev < 64) {
        std::lock_guard<std::mutex> lk(g_cache[dev].mu);
        if (g_cache[dev].streams.size() < 8) { g_cache[dev].streams.push_back(s); return; }
    }
    (void)hipStreamDestroy(s);
}
hipError_t cached_event(int dev, hipEvent_t* e)
{
    if (dev < 64) {
        std::lock_guard<std::mutex> lk(g_cache[dev].mu);
        if (!g_cache[dev].events.empty()) { *e = g_cache[dev].events.back(); g_cache[dev].events.pop_back(); return hipSuccess; }
    }
    return hipEventCreate(e);
}
void recycle_event(int dev, hipEvent_t e)
{
    if (dev < 64) {
        std::lock_guard<std::mutex> lk(g_cache[dev].mu);
        if (g_cache[dev].events.size() < 16) { g_cache[dev].events.push_back(e); return; }
    }
    (void)hipEventDestroy(e);
}
hipError_t cached_malloc(int dev, void** p, size_t bytes)
{
    if (dev < 64 && bytes <= kCacheBufMax) {
        std::lock_guard<std::mutex> lk(g_cache[dev].mu);
        auto& b = g_cache[dev].bufs;
        for (size_t i = 0; i < b.size(); ++i)
            if (b[i].first == bytes) {
                *p = b[i].second;
                g_cache[dev].buf_bytes -= bytes;
                b.erase(b.begin() + (long)i);
                return hipSuccess;
            }
    }
    if (dev < 64 && bytes > kCacheBufMax && bytes <= kBigBufMax) {
        std::lock_guard<std::mutex> lk(g_cache[dev].mu);
        auto& b = g_cache[dev].big;
        for (size_t i = b.size(); i-- > 0;)
            if (b[i].first == bytes) {
                *p = b[i].second;
                g_cache[dev].big_bytes -= bytes;
                b.erase(b.begin() + (long)i);
                return hipSuccess;
            }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess && dev < 64) {
        // out of memory with buffers parked in the cache: release them and try once more
        (void)hipGetLastError();
        std::vector<std::pair<size_t, void*>> drop;
        {
            std::lock_guard<std::mutex> lk(g_cache[dev].mu);
            drop.swap(g_cache[dev].big);
            g_cache[dev].big_bytes = 0;
        }
        if (!drop.empty()) {
            for (auto& d : drop) (void)hipFree(d.second);
            e = hipMalloc(p, bytes);
        }
    }
    return e;
}
void cached_free(int dev, void* p, size_t bytes)
{
    if (!p) return;
    if (dev < 64 && bytes > kCacheBufMax && bytes <= kBigBufMax) {
        std::vector<void*> drop;
        {
            std::lock_guard<std::mutex> lk(g_cache[dev].mu);
            auto& b = g_cache[dev].big;
            b.emplace_back(bytes, p);
            g_cache[dev].big_bytes += bytes;
            while (!b.empty() && (b.size() > kBigCount || g_cache[dev].big_bytes > kBigTotalMax)) {   // oldest first
                drop.push_back(b.front().second);
                g_cache[dev].big_bytes -= b.front().first;
                b.erase(b.begin());
            }
        }
        for (void* d : drop) (void)hipFree(d);
        return;
    }
    if (dev < 64 && bytes <= kCacheBufMax) {
        // most recently released last; when the cache is full the oldest entries make room (a cache that only ever kept its
        // first 16 buffers sent every later size to hipMalloc / hipFree: 0.24 -> 0.7 ms per one-shot call at 100^3 after a
        // run over other sizes)
        std::vector<void*> drop;
        {
            std::lock_guard<std::mutex> lk(g_cache[dev].mu);
            auto& b = g_cache[dev].bufs;
            b.emplace_back(bytes, p);
            g_cache[dev].buf_bytes += bytes;
            while (!b.empty() && (b.size() > 16 || g_cache[dev].buf_bytes > kCacheTotalMax)) {
                drop.push_back(b.front().second);
                g_cache[dev].buf_bytes -= b.front().first;
                b.erase(b.begin());
            }
        }
        for (void* d : drop) (void)hipFree(d);
        return;
    }
    (void)hipFree(p);
}

int init_device(int dev)
{
    int rc = use_device(dev);
    if (rc) return rc;
    if (dev < 64) {
        std::call_once(g_init_flag[dev], [dev]() {
            g_init_err[dev] = init_affine_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_quad_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_block_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_rows_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_span_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_extract_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_projbatch_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_extractsum_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_extractdot_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_extractdotmulti_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_extractsummulti_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_place_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_backproject_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_backproject_boxes_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_warp_kernels();
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = init_warp_stack_sum_kernels();
            hipDeviceProp_t prop;
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = hipGetDeviceProperties(&prop, dev);
            if (g_init_err[dev] == hipSuccess) {
                g_cu_count[dev] = prop.multiProcessorCount;
                g_lds_limit[dev] = (int)std::min<size_t>(160 * 1024, prop.sharedMemPerBlock > 0 ? prop.sharedMemPerBlock : 65536);
                g_init_err[dev] = hipMalloc(reinterpret_cast<void**>(&g_zeros[dev]), 256);
            }
            if (g_init_err[dev] == hipSuccess) g_init_err[dev] = hipMemset(g_zeros[dev], 0, 256);
        });
        if (g_init_err[dev] != hipSuccess)
            return fail((int)g_init_err[dev], "kernel attribute setup failed: %s", hipGetErrorString(g_init_err[dev]));
    }
    return 0;
}

}  // namespace

namespace {

// Host <-> device copies of caller-owned (pageable) numpy buffers.  Pageable copies run at ~10 GB/s through the
// runtime's staging path; pinning the caller's buffer in place for the duration of the copy lets the DMA engines run at
// PCIe rate.  Falls back to the plain copy when registration is refused (VT_NO_PIN=1 disables it).
//
// What must never happen (round 5, the cause of the `Memory access fault by GPU` on a host address that rounds 1, 2 and 4 each met and
// explained differently; found with VT_DEBUG_PIN=1, profiles/r05_pin_trace.txt): a registration of ours that OVERLAPS a pin of the
// runtime's own.  The runtime serves a pageable transfer of more than 1 MiB by pinning the caller's pages in place, and keeps the last few
// such pins (a cache keyed by address and size, released first-in first-out or when the queue dies), long after the transfer and after the
// caller's array has been freed.  When the heap hands the same addresses to the next, larger array and that array's interior is
// registered here, two pinned objects cover the same pages: the registration succeeds, the copy resolves its host address to the OLD,
// smaller object and runs off its end -- or the old pin is dropped from the cache under the copy -- and the GPU faults inside a range that
// was registered "ok" a moment ago.  (The trace: four 1.3 MB results at 0x..3d8eef90 .. 0x..3dcbd840, then a 32 MB input at 0x..3d8eef90,
// interior [0x..3da00000, 0x..3f600000) registered ok, fault at 0x..3f3c7000.  What the trace does not show is the step in between: the
// small arrays were FREED, the heap gave their pages back, and the next array got new pages at the old addresses -- a replay of the same
// transfers inside one arena whose pages never go away does not fault, tools/diag/pin_probe_check.py: the stale object is a pin whose pages
// are gone.)  Two rules follow:
//   1. no transfer issued here is ever pinned by the runtime: every pageable piece goes in slices of kSlice = 512 KiB, half the runtime's
//      threshold, i.e. through its staging buffers (1-8 MiB arrays lose the pinned rate they used to get: 0.3 ms on 4 MiB);
//   2. nothing is registered over a range in which the runtime already knows a pinned object (somebody else's pageable transfer, a caller's
//      own registration): the range is probed every kSlice bytes -- a runtime pin is longer than 1 MiB, so none can hide between two probes.
struct PinnedScope {
    void* ptr = nullptr;
    bool pinned = false;
    static bool trace() { return std::getenv("VT_DEBUG_PIN") != nullptr; }      // (read per scope: a test switches it on for one call)
    // VT_DEBUG_PIN=1: to stderr; VT_DEBUG_PIN=<path with a slash>: appended to that file line by line (a trace that survives the abort of a
    // GPU fault under a test runner that captures stderr)
    static void say(const char* fmt, ...) __attribute__((format(printf, 1, 2)))
    {
        const char* e = std::getenv("VT_DEBUG_PIN");
        if (!e) return;
        FILE* f = std::strchr(e, '/') ? std::fopen(e, "a") : stderr;
        if (!f) return;
        va_list ap;
        va_start(ap, fmt);
        std::vfprintf(f, fmt, ap);
        va_end(ap);
        if (f != stderr) std::fclose(f); else std::fflush(f);
    }
    // The process heap [start of the [heap] mapping, current break): arrays that live there are never registered (rule 3 below).
    static bool in_brk_heap(const void* p, size_t bytes)
    {
        static std::atomic<uintptr_t> heap_lo{0};
        uintptr_t lo_ = heap_lo.load(std::memory_order_relaxed);
        if (!lo_) {
            if (FILE* f = std::fopen("/proc/self/maps", "r")) {
                char line[512];
                while (std::fgets(line, sizeof line, f))
                    if (std::strstr(line, "[heap]")) { lo_ = (uintptr_t)std::strtoull(line, nullptr, 16); break; }
                std::fclose(f);
            }
            if (lo_) heap_lo.store(lo_, std::memory_order_relaxed);
        }
        if (!lo_) return false;
        const uintptr_t a = reinterpret_cast<uintptr_t>(p), brk_now = reinterpret_cast<uintptr_t>(sbrk(0));
        return a + bytes > lo_ && a < brk_now;
    }
    // Memory the runtime already knows as pinned host memory (the Python layer's pooled result buffers, a caller's own
    // hipHostMalloc / hipHostRegister, the runtime's own pins): registering the same range a second time SUCCEEDS, and the matching
    // unregister at the end of the scope then strips the owner's registration ([measured, round 2] the pool's later
    // hipHostUnregister failed with "pointer does not correspond to a registered memory region", and the sticky error
    // failed the next kernel-launch check).
    static bool already_registered(const void* p)
    {
        hipPointerAttribute_t attr;
        const hipError_t e = hipPointerGetAttributes(&attr, p);
        if (e != hipSuccess) { (void)hipGetLastError(); return false; }
        return attr.type == hipMemoryTypeHost;
    }
    static bool any_registered(uintptr_t a, uintptr_t b)
    {
        for (uintptr_t x = a; x < b; x += kSlice)
            if (already_registered(reinterpret_cast<const void*>(x))) return true;
        return b > a && already_registered(reinterpret_cast<const void*>(b - 1));
    }
    // Only WHOLE 2 MiB units that lie INSIDE the caller's array are registered, and the copies below are cut at the ends of that
    // interior: a range rounded outward would pin memory that is not the caller's (its heap neighbours'), and the host's transparent huge
    // pages make 2 MiB the unit in which a pin can come and go without touching anything else.  The ragged head and tail of the array
    // (< 2 MiB each) travel as pageable slices.
    char* lo = nullptr;               // the registered interior [lo, hi) of the caller's range
    char* hi = nullptr;
    mutable hipStream_t last_stream = nullptr;
    mutable bool used_stream = false;
    static constexpr uintptr_t kUnit = 2u << 20;
    static constexpr size_t kSlice = 512u << 10;
    static constexpr size_t kHeapMax = 32u << 20;          // glibc's DEFAULT_MMAP_THRESHOLD_MAX on 64-bit
    PinnedScope(const void* p, size_t bytes)
    {
        static const bool off = std::getenv("VT_NO_PIN") != nullptr;
        if (trace() && p) say("[vt pin] scope %p + %zu%s\n", p, bytes, in_brk_heap(p, bytes) ? " (process heap)" : "");
        // Rule 3: nothing in the process heap is registered, and nothing the heap COULD hold: glibc serves requests up to 32 MiB from the
        // heap once its dynamic mmap threshold has risen (it rises to the size of every freed mapping up to that maximum), larger ones always
        // from mappings of their own.  Every fault seen -- rounds 1, 2, 4 and three this round -- was at a heap address, inside an interior
        // registered "ok" a moment before, after the heap had taken pages back and handed the addresses out again (profiles/r05_pin_trace.txt).
        if (off || !p || bytes <= kHeapMax || in_brk_heap(p, bytes)) return;
        const uintptr_t a0 = (reinterpret_cast<uintptr_t>(p) + kUnit - 1) & ~(kUnit - 1);
        const uintptr_t a1 = (reinterpret_cast<uintptr_t>(p) + bytes) & ~(kUnit - 1);
        if (a1 <= a0 || a1 - a0 < (4u << 20)) return;
        // (the head and tail are probed too: a runtime pin that starts in the head reaches into the interior)
        if (any_registered(reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + bytes)) {
            if (trace()) say("[vt pin] %p + %zu overlaps memory the runtime has pinned already: not registered\n", p, bytes);
            return;
        }
        ptr = reinterpret_cast<void*>(a0);
        pinned = hipHostRegister(ptr, a1 - a0, hipHostRegisterDefault) == hipSuccess;
        if (trace()) say("[vt pin] registered [%p, %p): %s\n", ptr, (void*)a1, pinned ? "ok" : "refused");
        if (!pinned) { (void)hipGetLastError(); return; }
        lo = reinterpret_cast<char*>(a0);
        hi = reinterpret_cast<char*>(a1);
    }
    // one pageable piece, in slices the runtime stages (rule 1)
    static hipError_t sliced(char* dst, const char* src, size_t bytes, hipMemcpyKind kind, hipStream_t st)
    {
        // VT_PIN_UNSLICED=1 (diagnosis only: tools/diag/pin_probe_check.py): one transfer, which the runtime pins in place when it is large
        if (std::getenv("VT_PIN_UNSLICED")) return hipMemcpyAsync(dst, src, bytes, kind, st);
        for (size_t off = 0; off < bytes; off += kSlice) {
            const hipError_t e = hipMemcpyAsync(dst + off, src + off, std::min(kSlice, bytes - off), kind, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // A copy between device memory and a part of the caller's range, cut so that every piece lies either wholly inside the registered
    // interior or wholly outside it: the runtime decides "pinned or pageable" from a transfer's first host byte, and a pinned transfer
    // that runs past the end of the registration would let the DMA engine read unmapped pages.  `host` may be the source or the target.
    hipError_t copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) const
    {
        if (bytes == 0) return hipSuccess;
        last_stream = st; used_stream = true;
        const bool h2d = kind == hipMemcpyHostToDevice;
        const char* const h0 = h2d ? static_cast<const char*>(src) : static_cast<const char*>(dst);
        const char* const h1 = h0 + bytes;
        if (!pinned) {
            // memory that is registered as a whole (the Python layer's pooled result buffers, a caller's own pinned array): one transfer
            if (already_registered(h0) && already_registered(h1 - 1)) return hipMemcpyAsync(dst, src, bytes, kind, st);
            return sliced(static_cast<char*>(dst), static_cast<const char*>(src), bytes, kind, st);
        }
        const char* cuts[4] = {h0, std::min(std::max(h0, (const char*)lo), h1), std::min(std::max(h0, (const char*)hi), h1), h1};
        for (int i = 0; i < 3; ++i) {
            const size_t off = (size_t)(cuts[i] - h0), len = (size_t)(cuts[i + 1] - cuts[i]);
            if (!len) continue;
            const hipError_t e = (i == 1) ? hipMemcpyAsync(static_cast<char*>(dst) + off, static_cast<const char*>(src) + off, len, kind, st)
                                          : sliced(static_cast<char*>(dst) + off, static_cast<const char*>(src) + off, len, kind, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // ... and the pitched form: `rows` dense host rows of `row_bytes` to / from device rows `dpitch` apart.  Whole rows inside the interior
    // go as one 2-D copy, rows outside it in blocks of at most kSlice bytes, a row that straddles one of its ends is cut there.
    hipError_t copy2d(void* dev, size_t dpitch, const void* host, size_t row_bytes, size_t rows, bool h2d, hipStream_t st) const
    {
        const hipMemcpyKind kind = h2d ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
        auto block = [&](size_t r0, size_t r1) -> hipError_t {
            if (r1 <= r0) return hipSuccess;
            char* d = static_cast<char*>(dev) + r0 * dpitch;
            const char* h = static_cast<const char*>(host) + r0 * row_bytes;
            return h2d ? hipMemcpy2DAsync(d, dpitch, h, row_bytes, row_bytes, r1 - r0, kind, st)
                       : hipMemcpy2DAsync(const_cast<char*>(h), row_bytes, d, dpitch, row_bytes, r1 - r0, kind, st);
        };
        auto one_row = [&](size_t r) -> hipError_t {          // through copy(): cut at the interior's ends, sliced where pageable
            char* d = static_cast<char*>(dev) + r * dpitch;
            const char* h = static_cast<const char*>(host) + r * row_bytes;
            return h2d ? copy(d, h, row_bytes, kind, st) : copy(const_cast<char*>(h), d, row_bytes, kind, st);
        };
        auto pageable = [&](size_t r0, size_t r1) -> hipError_t {       // rows outside the interior: blocks the runtime stages (rule 1)
            if (r1 <= r0) return hipSuccess;
            if (row_bytes > kSlice) {
                for (size_t r = r0; r < r1; ++r) { const hipError_t e = one_row(r); if (e != hipSuccess) return e; }
                return hipSuccess;
            }
            const size_t step = std::max<size_t>(1, kSlice / row_bytes);
            for (size_t r = r0; r < r1; r += step) { const hipError_t e = block(r, std::min(r + step, r1)); if (e != hipSuccess) return e; }
            return hipSuccess;
        };
        if (rows == 0 || row_bytes == 0) return hipSuccess;
        last_stream = st; used_stream = true;
        const char* const h0 = static_cast<const char*>(host);
        if (!pinned) {
            if (already_registered(h0) && already_registered(h0 + rows * row_bytes - 1)) return block(0, rows);
            return pageable(0, rows);
        }
        auto row_of = [&](const char* a) -> size_t {          // row that holds byte a
            if (a <= h0) return 0;
            return std::min(rows, (size_t)(a - h0) / row_bytes);
        };
        // rows [0, ra): wholly below lo; row ra may straddle lo; rows (ra', rb): wholly inside; row rb may straddle hi; rows beyond: outside
        const size_t ra = row_of(lo), rb = row_of(hi);
        const bool cut_a = ra < rows && h0 + ra * row_bytes < lo;                              // row ra starts below lo
        const size_t in0 = cut_a ? ra + 1 : ra;
        const bool cut_b = rb < rows && rb >= in0 && h0 + rb * row_bytes < hi;                 // row rb starts inside and ends beyond hi
        hipError_t e = pageable(0, ra);
        if (e == hipSuccess && cut_a) e = one_row(ra);
        if (e == hipSuccess) e = block(in0, std::max(in0, rb));
        if (e == hipSuccess && cut_b) e = one_row(rb);
        if (e == hipSuccess) e = pageable(std::max(in0, cut_b ? rb + 1 : rb), rows);
        return e;
    }
    ~PinnedScope()
    {
        if (!pinned) return;
        // (no transfer may still be reading or writing the range when its mapping goes: the regular paths have waited already, an error
        //  return in between has not)
        if (used_stream) (void)hipStreamSynchronize(last_stream);
        const hipError_t e = hipHostUnregister(ptr);
        if (trace()) say("[vt pin] released [%p, %p): %s\n", ptr, (void*)hi, e == hipSuccess ? "ok" : hipGetErrorString(e));
        if (e != hipSuccess) (void)hipGetLastError();
    }
};

// Run the three passes X, Y, Z (reference order, transforms.py:305-307) on d_a, using d_b as the
// ping-pong partner.  Returns which buffer holds the coefficients.  in_plane_only (VT_STACK handles): the planes are independent
// images, the axis-0 pass does not run.
int run_prefilter(float* d_a, float* d_b, int D, int H, int W, int P, bool lo_interior_axis0, hipStream_t st, float** result,
                  bool in_plane_only = false)
{
    float* cur = d_a;
    float* oth = d_b;
    const int order[3] = {2, 1, 0};
    int first_pass = 0;
    if (prefilter_xy_ok(D, H, W, P, cur, oth)) {
        // X and Y in one launch (vt_kernels_prefilter.hip: prefilter_xy): the plane is read once and written once for both
        VT_HIP(launch_prefilter_xy(cur, oth, D, H, W, P, st));
        float* t = cur; cur = oth; oth = t;
        first_pass = 2;
    }
    for (int i = first_pass; i < (in_plane_only ? 2 : 3); ++i) {
        const int axis = order[i];
        const bool interior = (axis == 0) && lo_interior_axis0;
        if (prefilter_axis_in_place_ok(axis, D, H, W)) {
            VT_HIP(launch_prefilter_axis(axis, cur, cur, D, H, W, P, interior, st));
        } else {
            VT_HIP(launch_prefilter_axis(axis, cur, oth, D, H, W, P, interior, st));
            float* t = cur; cur = oth; oth = t;
        }
    }
    *result = cur;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// one transform call: fold offsets -> pick the resident copy and the plan -> launch -> (host output) copy back
// ---------------------------------------------------------------------------------------------------

// Which resident copy a launch samples, and what is special about its output.
struct Orientation {
    const float* src_plain = nullptr;  // plain-layout copy the launch (or its pair / quad relayout) is based on
    int quad_idx = 0;                  // 0..3: plain, axes 0 <-> 1, in-plane transposed, axes 0 <-> 2 -- its plane-quad forms are the
                                       // copies kCopyQ0 + quad_idx and (z-convolved) kCopyQe0 + quad_idx, its plane-pair form kCopyP0 + quad_idx
    int plain_id = -1;                 // LazyCopyId of the exchanged plain-layout copy this orientation is based on (-1: the handle's own plain copy);
                                       // built by ensure_secondary_copy only when the launch -- or the relayout of a missing quad form -- reads it
    int srcD = 0, srcH = 0;            // depth / height of that copy
    int rowW = 0, rowP = 0;            // row width / pitch of that copy
    bool xswap = false;                // the kernels write an axis-0 <-> 2 exchanged result into the copy kCopyTmpX
};

bool is_marching(int kind) { return kind == 4 || kind == 5 || kind == 8; }

// src_resident = M . (d + out_plane0, h, w, 1) - (plane0, 0, 0): output-plane and resident-window offsets go into column 3
void fold_matrix(const vt_volume* v, const double m4x4[16], double m[12])
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 4; ++c) m[4 * r + c] = m4x4[4 * r + c];
        m[4 * r + 3] = std::fma(m4x4[4 * r], (double)v->out_plane0, m4x4[4 * r + 3]);
    }
    m[3] -= (double)v->plane0;
    for (int r = 0; r < 3; ++r) m[4 * r + 3] += (double)v->edge_pad;       // VT_EDGE_SCIPY: resident coordinate = volume coordinate + pad
}

// a handle-shaped view of the same volume with axes permuted (planning only: no buffers)
vt_volume planning_view(const vt_volume* v, int D, int H, int W, int P, int oD, int oH, int oW, bool keep_window)
{
    vt_volume sw;
    sw.dev = v->dev; sw.interp = v->interp;
    sw.D = D; sw.H = H; sw.W = W; sw.P = P;
    sw.oD = oD; sw.oH = oH; sw.oW = oW;
    sw.plane0 = keep_window ? v->plane0 : 0; sw.gD = keep_window ? v->gD : D; sw.out_plane0 = keep_window ? v->out_plane0 : 0;
    sw.lds_limit = v->lds_limit; sw.cu_count = v->cu_count; sw.tune = v->tune;
    sw.edge_pad = v->edge_pad;
    return sw;
}


// ---------------------------------------------------------------------------------------------------
// lazily built resident copies: one place that allocates, times, budgets and evicts them
// ---------------------------------------------------------------------------------------------------
// A handle that has used every orientation holds up to 13 buffers besides its plain copy.  They live in one table
// (vt_resident.h), which decides what a build may evict; the functions below carry its decisions out on the device.  A copy that cannot
// be built -- over the budget, or hipMalloc fails with nothing left to evict -- sends the caller to a family that reads the plain layout.

float* copy_ptr(const vt_volume* v, int id) { return static_cast<float*>(v->lazy.copy[id].ptr); }

// what the budget counts besides the lazy copies: the plain copy and the projection helper's
uint64_t fixed_bytes(const vt_volume* v) { return v->src_bytes + (v->proj ? v->proj->src_bytes : 0); }
uint64_t resident_now(const vt_volume* v) { return fixed_bytes(v) + v->lazy.held(); }

// free what a decision of the table let go of, once no launch may still read it (an evicted buffer may be built over at once)
void release(vt_volume* v, LazyCopies::Released& rel)
{
    if (rel.empty()) return;
    (void)hipStreamSynchronize(v->stream);
    for (void* b : rel.bufs) (void)hipFree(b);
    (void)hipGetLastError();
    v->copies_evicted += (int)rel.evicted.size();
    if (std::getenv("VT_DEBUG_ALLOC"))
        for (int id : rel.evicted)
            std::fprintf(stderr, "[vt] evicted lazy copy %d (last used at launch %llu of %llu)\n", id,
                         (unsigned long long)v->lazy.copy[id].used, (unsigned long long)v->lazy.use_clock);
    rel = LazyCopies::Released();
}

// a copy whose build failed (a zero-filled copy must never survive: later calls would sample it silently), or that is too small
void discard_copy(vt_volume* v, int id)
{
    (void)hipGetLastError();
    (void)hipStreamSynchronize(v->stream);                       // nothing may still be writing the buffer that is freed
    (void)hipFree(v->lazy.forget(id));
    (void)hipGetLastError();
}

// Allocate lazy copy `id` (`bytes` large): hipSuccess, or hipErrorOutOfMemory when the budget or the device cannot hold it beside the
// copies this call has touched.  `transient`: the copy the build reads, not counted against the budget (LazyCopies::make_room) -- the
// budget bounds what a handle KEEPS; for the few milliseconds of a relayout the handle may hold that source beside it.
hipError_t alloc_lazy(vt_volume* v, int id, size_t bytes, int transient = -1)
{
    LazyCopies::Released rel;
    const bool fits = v->lazy.make_room(id, bytes, fixed_bytes(v), transient, rel);
    release(v, rel);
    if (!fits) return hipErrorOutOfMemory;
    if (v->lazy.take_spare(id, bytes)) return hipSuccess;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    while (e != hipSuccess) {
        (void)hipGetLastError();
        if (!v->lazy.free_some(rel)) return hipErrorOutOfMemory;
        release(v, rel);
        e = hipMalloc(&p, bytes);
    }
    v->lazy.record(id, p, bytes);
    return hipSuccess;
}

// GPU time of a copy's build, for vt_volume_info.copies_ms (events of their own: the handle's timer may be running)
void lazy_build_begin(vt_volume* v)
{
    if (!v->evc0) { (void)hipEventCreate(&v->evc0); (void)hipEventCreate(&v->evc1); }
    if (v->evc0) (void)hipEventRecord(v->evc0, v->stream);
}
void lazy_build_end(vt_volume* v)
{
    v->copies_built += 1;
    if (!v->evc0 || !v->evc1) return;
    float ms = 0.f;
    if (hipEventRecord(v->evc1, v->stream) == hipSuccess && hipEventSynchronize(v->evc1) == hipSuccess &&
        hipEventElapsedTime(&ms, v->evc0, v->evc1) == hipSuccess) v->copies_ms += ms;
    (void)hipGetLastError();
}

// The exchanged plain-layout copy of an orientation (kCopyT / kCopyR / kCopyX): 0 = it exists, 1 = it cannot be built.
int ensure_lazy_plain(vt_volume* v, int id)
{
    if (v->lazy.copy[id].ptr) { v->lazy.touch(id); return 0; }
    size_t bytes = 0;
    if (id == kCopyT) bytes = (size_t)v->D * v->H * v->P * sizeof(float);
    else if (id == kCopyR) { v->Pr = resident_pitch(v->H); bytes = (size_t)v->D * v->W * v->Pr * sizeof(float); }
    else if (id == kCopyX) { v->Px = resident_pitch(v->D); bytes = (size_t)v->W * v->H * v->Px * sizeof(float); }
    else return 1;
    if (alloc_lazy(v, id, bytes) != hipSuccess) return 1;
    float* const dst = copy_ptr(v, id);
    lazy_build_begin(v);
    hipError_t e = hipSuccess;
    if (id == kCopyT) {
        e = launch_relayout_swap01(v->d_src, dst, v->D, v->H, v->P, v->stream);
    } else {
        e = hipMemsetAsync(dst, 0, bytes, v->stream);                                     // pad columns must be zero
        if (e == hipSuccess && id == kCopyR)        // dst[z][x][y]: element (i = y, j = z, k = x) -> (k = x, j = z, i = y)
            e = launch_transpose02(v->d_src, dst, v->H, v->D, v->W, v->P, (int64_t)v->H * v->P, v->Pr, (int64_t)v->W * v->Pr, v->stream);
        else if (e == hipSuccess)
            e = launch_transpose02(v->d_src, dst, v->D, v->H, v->W, (int64_t)v->H * v->P, v->P, (int64_t)v->H * v->Px, v->Px, v->stream);
    }
    if (e != hipSuccess) { discard_copy(v, id); return 1; }
    lazy_build_end(v);
    return 0;
}

// Rotations about axis 1 ([a 0 b; 0 1 0; c 0 d]): the same problem with axes 0 and 1 exchanged is axis-0-separable.
// A second resident copy with those axes exchanged (built once, lazily) lets the marching kernels serve it; only
// the output addressing changes (plane stride oW, row stride oH*oW).  Whole-volume handles only (no slab offsets).
int try_axis1_exchange(vt_volume* v, const double m[12], int flags, size_t n_out, AffineParams* p, TilePlan* plan, Orientation* ori)
{
    const bool ysep = !(flags & (VT_NO_ZSEP | VT_NO_MARCH | VT_FORCE_DIRECT)) && m[5] == 1.0 && m[4] == 0.0 && m[6] == 0.0 &&
                      m[1] == 0.0 && m[9] == 0.0 && std::fabs(m[7]) < 1.0e9 &&
                      !(m[0] == 1.0 && m[2] == 0.0 && m[8] == 0.0) &&
                      v->plane0 == 0 && v->out_plane0 == 0 && v->gD == v->D && v->D <= 65535 && v->H <= 65535 &&
                      (n_out >= (size_t)64 * 64 * 64 || (flags & VT_FORCE_TILED));
    if (!ysep) return 0;
    vt_volume sw = planning_view(v, v->H, v->D, v->W, v->P, v->oH, v->oD, v->oW, false);
    const int pi[3] = {1, 0, 2};
    double ms[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) ms[4 * r + c] = m[4 * pi[r] + pi[c]];
        ms[4 * r + 3] = m[4 * pi[r] + 3];
    }
    AffineParams ps;
    std::memset(&ps, 0, sizeof(ps));
    TilePlan plans;
    plan_launch(&sw, ms, flags, &ps, &plans);
    if (!is_marching(plans.kind)) return 0;
    *p = ps; *plan = plans;
    p->ostride = v->oW; p->orow = (int64_t)v->oH * v->oW;
    p->ord[0] = 1; p->ord[1] = 0; p->ord[2] = 2;          // original (d, h, w) = this launch's columns (1, 0, 2)
    ori->src_plain = copy_ptr(v, kCopyT); ori->plain_id = kCopyT; ori->quad_idx = 1;
    ori->srcD = v->H; ori->srcH = v->D;
    return 0;
}

// Rotations about axis 2 ([a b 0; c d 0; 0 0 1]): axis-0-separable after exchanging axes 0 and 2.  The marching kernels
// run on the exchanged copy and produce an exchanged result, which one transpose pass (8 B/voxel) turns back.
// Cubic only: trilinear rotations about axis 2 are the bounding-box kernel's best case (x stays contiguous: 0.34 ms at
// 512^3, faster than marching 0.25 + transposing 0.2); VT_FORCE_XSWAP (diagnostic) takes the exchange path regardless.
int try_axis2_exchange(vt_volume* v, const double m[12], int flags, size_t n_out, AffineParams* p, TilePlan* plan, Orientation* ori)
{
    const bool xsep = !(flags & (VT_NO_ZSEP | VT_NO_MARCH | VT_FORCE_DIRECT | VT_KEEP_OUTSIDE)) &&
                      (is_cubic(v->interp) || (flags & VT_FORCE_XSWAP)) &&
                      m[10] == 1.0 && m[8] == 0.0 && m[9] == 0.0 && m[2] == 0.0 && m[6] == 0.0 && std::fabs(m[11]) < 1.0e9 &&
                      !(m[0] == 1.0 && m[1] == 0.0 && m[4] == 0.0) && !(m[5] == 1.0 && m[1] == 0.0 && m[4] == 0.0) &&
                      v->plane0 == 0 && v->out_plane0 == 0 && v->gD == v->D && v->H <= 65535 && v->oH <= 65535 &&
                      (n_out >= (size_t)64 * 64 * 64 || (flags & VT_FORCE_TILED));
    if (!xsep) return 0;
    vt_volume sw = planning_view(v, v->W, v->H, v->D, resident_pitch(v->D), v->oW, v->oH, v->oD, false);
    const int pi[3] = {2, 1, 0};
    double ms[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) ms[4 * r + c] = m[4 * pi[r] + pi[c]];
        ms[4 * r + 3] = m[4 * pi[r] + 3];
    }
    AffineParams ps;
    std::memset(&ps, 0, sizeof(ps));
    TilePlan plans;
    plan_launch(&sw, ms, flags, &ps, &plans);
    if (!is_marching(plans.kind)) return 0;
    v->Px = sw.P;
    *p = ps; *plan = plans;
    p->ord[0] = 2; p->ord[1] = 1; p->ord[2] = 0;          // original (d, h, w) = this launch's columns (2, 1, 0)
    ori->src_plain = copy_ptr(v, kCopyX); ori->plain_id = kCopyX; ori->quad_idx = 3;
    ori->srcD = v->W; ori->srcH = v->H; ori->rowW = v->D; ori->rowP = v->Px;
    ori->xswap = true;
    return 0;
}

// In-plane maps closer to a quarter turn than to the identity (|m12| > |m11|: rotations about axis 0 by 45..135 and
// 225..315 degrees): sampled from an in-plane TRANSPOSED resident copy the same map has its rows 1 and 2 exchanged and
// falls into the 0..45 degree class, whose footprints are wide in x (long staged rows, lanes walk along LDS rows
// instead of down a column).  Only the source side changes; the output is written as usual.
int try_inplane_transposed(vt_volume* v, const double m[12], int flags, size_t n_out, AffineParams* p, TilePlan* plan, Orientation* ori)
{
    const bool zsep_m = m[0] == 1.0 && m[1] == 0.0 && m[2] == 0.0 && m[4] == 0.0 && m[8] == 0.0 && std::fabs(m[3]) < 1.0e9;
    const bool rsep = zsep_m && !(flags & (VT_NO_ZSEP | VT_NO_MARCH | VT_FORCE_DIRECT | VT_NO_RSWAP)) &&
                      std::fabs(m[6]) > std::fabs(m[5]) && std::fabs(m[9]) > std::fabs(m[10]) && v->D <= 65535 &&
                      (n_out >= (size_t)64 * 64 * 64 || (flags & VT_FORCE_TILED));
    if (!rsep) return 0;
    vt_volume sw = planning_view(v, v->D, v->W, v->H, resident_pitch(v->H), v->oD, v->oH, v->oW, true);
    double ms[12];
    for (int c = 0; c < 4; ++c) { ms[c] = m[c]; ms[4 + c] = m[8 + c]; ms[8 + c] = m[4 + c]; }
    AffineParams ps;
    std::memset(&ps, 0, sizeof(ps));
    TilePlan plans;
    plan_launch(&sw, ms, flags, &ps, &plans);
    if (!is_marching(plans.kind)) return 0;
    v->Pr = sw.P;
    *p = ps; *plan = plans;
    ori->src_plain = copy_ptr(v, kCopyR); ori->plain_id = kCopyR; ori->quad_idx = 2;
    ori->srcD = v->D; ori->srcH = v->W; ori->rowW = v->H; ori->rowP = v->Pr;
    // Tile order on the transposed copy: h fastest for the round-1 marching kernels (consecutive tiles read neighbouring source
    // rows); the plane-quad kernel with its 2-D grid keeps w fastest -- [measured, angles 50..130] 1024^3 trilinear 1.58-1.70 ->
    // 1.51-1.63 ms, 1024^3 cubic at 80 / 90 degrees 1.76 / 1.79 -> 1.65 / 1.61, 512^3 equal or better (consecutive tiles complete whole
    // output rows instead of writing down a column of tiles).  VT_RSWAP_WFAST=1 / 0 forces either.
    const bool wfast = v->tune.rswap_wfast >= 0 ? v->tune.rswap_wfast != 0 : plans.kind == 8;
    if (!wfast) p->flags |= (1 << 24);
    return 0;
}

// General matrices (none of the forms above): the general-matrix kernels stage source ROWS -- runs along the resident copy's fastest axis --
// and their lanes walk along the output's w axis.  Where w follows source axis 0 or 1 more closely than axis 2, the rows a tile touches
// are many and short on the plain copy (partly used cache lines, short staged vectors, lanes of a wave scattered over LDS rows); sampled
// from the copy whose FASTEST axis is the one w follows ([x][y][z] of the axis-2 exchange, [z][x][y] of the in-plane transposition: the
// copies the marching kernels use) the same launch has long rows.  Only the source side changes -- the matrix rows are permuted with the
// copy's axes, the output is written as usual, the skirt test's chains are per row and unchanged.  [measured, 512^3, the reference's 100
// random rotations, tools/general_reorient_probe.py] trilinear 0.449 -> 0.426 ms, cubic 1.004 -> 0.956 (best of the three copies per
// matrix: 0.422 / 0.949).  A copy is built at the handle's FOURTH call that asks for it: a handle used once or twice (vt_affine_oneshot)
// never pays a transpose pass for a few per cent of one launch.
int try_general_reorient(vt_volume* v, const double m[12], int flags, size_t n_out, AffineParams* p, TilePlan* plan, Orientation* ori)
{
    if ((flags & (VT_FORCE_DIRECT | VT_NO_REORIENT)) || v->tune.reorient == 0) return 0;
    if (n_out < (size_t)192 * 192 * 192 && !(flags & VT_FORCE_TILED)) return 0;      // launch-bound sizes: nothing to win
    // the source axis the output's w direction follows (the plain copy keeps ties and near-ties: no copy, no churn)
    const double c[3] = {std::fabs(m[2]), std::fabs(m[6]), std::fabs(m[10])};
    int a = 2;
    if (c[1] > 1.15 * c[2] && c[1] >= c[0]) a = 1;
    if (c[0] > 1.15 * c[2] && c[0] > c[1]) a = 0;
    if (a == 2) return 0;
    if (a == 0 && !(v->plane0 == 0 && v->out_plane0 == 0 && v->gD == v->D)) return 0;  // slab windows live on axis 0: it stays the slowest
    const int id = (a == 1) ? kCopyR : kCopyX;
    int* const asked = &v->reorient_asked[a];
    if (!v->lazy.copy[id].ptr && ++*asked < ((flags & VT_FORCE_TILED) ? 1 : v->tune.reorient)) return 0;
    const vt_volume sw = (a == 1) ? planning_view(v, v->D, v->W, v->H, resident_pitch(v->H), v->oD, v->oH, v->oW, true)
                                  : planning_view(v, v->W, v->H, v->D, resident_pitch(v->D), v->oD, v->oH, v->oW, false);
    const int pi[3] = {a == 1 ? 0 : 2, a == 1 ? 2 : 1, a == 1 ? 1 : 0};                // source axis of the copy's axis r
    double ms[12];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) ms[4 * r + k] = m[4 * pi[r] + k];
    AffineParams ps;
    std::memset(&ps, 0, sizeof(ps));
    TilePlan plans;
    plan_launch(&sw, ms, flags, &ps, &plans);
    if (!(plans.kind == 2 || plans.kind == 6 || plans.kind == 9)) return 0;           // the general-matrix kernels only
    if (a == 1) v->Pr = sw.P; else v->Px = sw.P;
    if (ensure_lazy_plain(v, id)) {
        *asked = -64;                         // no room for another copy: the plain layout serves this matrix and the next 64 requests
        return 0;
    }
    *p = ps; *plan = plans;
    ori->src_plain = copy_ptr(v, id); ori->plain_id = id;
    ori->srcD = sw.D; ori->srcH = sw.H; ori->rowW = sw.W; ori->rowP = sw.P;
    return 0;
}

// Maps that leave axis 2 alone with an integer offset (rotations about axis 2 through the default centre): the row kernel on the plain
// copy (trilinear) or on its x-convolved form (cubic; built lazily, one relayout pass).  vt_kernels_rows.hip.
int try_rows(vt_volume* v, const double m[12], int flags, AffineParams* p, TilePlan* plan, Orientation* ori)
{
    AffineParams ps;
    std::memset(&ps, 0, sizeof(ps));
    TilePlan plans = TilePlan();
    plans.kind = 0;
    if (!plan_rows(v, m, flags, &ps, &plans) || plans.kind != 10) return 0;
    const bool use_xe = is_cubic(v->interp) && !(ps.flags & (1 << 16));      // (a fractional axis-2 offset forms its own x-sums on the plain copy)
    LazyCopy& xe = v->lazy.copy[kCopyXe];
    if (use_xe && !xe.ptr) {
        // no room for the copy, or a refused relayout: the exchange path or the general kernels serve this matrix and the next 64
        if (xe.retry_in > 0) { --xe.retry_in; return 0; }
        if (alloc_lazy(v, kCopyXe, (size_t)v->D * v->H * v->P * sizeof(float)) != hipSuccess) { xe.retry_in = 64; return 0; }
        lazy_build_begin(v);
        const bool simple = v->interp == VT_BSPLINE_SIMPLE || v->interp == VT_FILT_BSPLINE_SIMPLE;
        if (launch_relayout_xfir(v->d_src, copy_ptr(v, kCopyXe), v->D, v->H, v->W, v->P, simple, v->stream) != hipSuccess) {
            discard_copy(v, kCopyXe);
            xe.retry_in = 64;
            return 0;
        }
        lazy_build_end(v);
    }
    *p = ps; *plan = plans;
    if (use_xe) v->lazy.touch(kCopyXe);
    ori->src_plain = use_xe ? copy_ptr(v, kCopyXe) : v->d_src;
    return 0;
}

void note_launch(vt_volume* v, int kind, const TilePlan& plan, const AffineParams& p, size_t n_out)
{
    v->last_kernel = kind;
    const bool tiled = kind >= 2;
    v->last_tile[0] = tiled ? plan.td : 0; v->last_tile[1] = tiled ? plan.th : 0; v->last_tile[2] = tiled ? plan.tw : 0;
    v->last_lds[0] = tiled ? p.Lz : 0; v->last_lds[1] = tiled ? p.Ly : 0; v->last_lds[2] = tiled ? p.Lx : 0;
    v->last_lds_bytes = tiled ? plan.lds_bytes : 0;
    v->last_grid = tiled ? plan.grid : (int)((n_out + 255) / 256);
}

// the exchanged-result buffer of an axis-0 <-> 2 launch holds its output
bool xswap_buffer_ok(const vt_volume* v, size_t n_out)
{
    return v->lazy.copy[kCopyTmpX].ptr && v->lazy.copy[kCopyTmpX].bytes >= n_out * sizeof(float);
}

// Build the secondary resident copy a plan needs (once per handle and orientation).  Returns 0 when the copy exists, 1 when it
// could not be built -- no device memory for it, or a relayout launch that was refused: the copy is freed (a zero-filled copy must
// never survive: later calls would sample it silently) and the caller re-plans without this kernel family --, < 0 never.
int ensure_secondary_copy(vt_volume* v, const TilePlan& plan, const AffineParams& p, Orientation& ori)
{
    size_t bytes = 0;
    int id = -1;
    const bool zfir = plan.kind == 8 && (p.flags & (1 << 19)) != 0;       // the z-convolved copy (vt_plan.hip: plan_quad)
    if (plan.kind == 8) {
        id = (zfir ? kCopyQe0 : kCopyQ0) + ori.quad_idx;
        bytes = (size_t)((ori.srcD + 3) / 4) * ori.srcH * p.sPq * sizeof(float);
#ifdef VT_LEGACY
    } else if (plan.kind == 5) {
        id = kCopyP0 + ori.quad_idx;
        bytes = (size_t)((ori.srcD + 1) / 2) * ori.srcH * p.sP2 * sizeof(float);
#endif
    }
    const bool built = id >= 0 && v->lazy.copy[id].ptr;
    if (built) v->lazy.touch(id);              // (pinned before the result buffer below is allocated)
    // the exchanged result buffer of the axis-0 <-> 2 orientation (allocated first: every copy built below is then sized against it)
    const size_t n_out = (size_t)v->oD * v->oH * v->oW;
    if (ori.xswap) {
        if (!xswap_buffer_ok(v, n_out)) {
            if (v->lazy.copy[kCopyTmpX].ptr) discard_copy(v, kCopyTmpX);
            if (alloc_lazy(v, kCopyTmpX, n_out * sizeof(float)) != hipSuccess) return 1;
        }
        v->lazy.touch(kCopyTmpX);
    }
    // (every return of success below: what the launch reads is still there -- a mistake in the pins fails a call, it does not fault the GPU)
    auto ready = [&] { return ori.xswap && !xswap_buffer_ok(v, n_out) ? 1 : 0; };
    if (built) return ready();                 // the launch reads this form only: its plain-layout source may be gone
    // The exchanged plain-layout copy of the orientation: read by the launch itself (kinds that sample the plain layout) or by the relayout
    // that builds the missing plane-quad form.  Built here and not when the orientation is chosen: under a budget it is the first copy
    // evicted once its quad form exists, and a sweep must not rebuild it on every call.
    // (Round 5: the plane-quad forms of the in-plane transposed orientation come straight from the handle's own plain copy --
    // relayout_zquad_swap12 -- when that exchanged copy does not exist yet: nothing else reads it on this path.)
    const bool fused_swap12 = plan.kind == 8 && ori.plain_id == kCopyR && !v->lazy.copy[kCopyR].ptr && !v->tune.no_fused_relayout;
    const int transient = fused_swap12 ? -1 : ori.plain_id;
    if (transient >= 0) {
        if (ensure_lazy_plain(v, transient)) return 1;
        ori.src_plain = copy_ptr(v, transient);
    }
    if (id < 0) return ready();
#ifdef VT_LEGACY
    if (v->tune.test_fail_copy) return 1;      // VT_TEST_FAIL_COPY (test build): the allocation-failure path, for tests/test_gpu_parity.py
#endif
    // A copy that did not fit is not attempted again at once: a device that is short of memory would pay a volume-sized hipMalloc
    // (and its failure) on every call.  The next attempt comes kCopyRetryCalls calls later.
    constexpr int kCopyRetryCalls = 64;
    int& retry = v->lazy.copy[id].retry_in;
    if (retry > 0) { --retry; return 1; }
    if (alloc_lazy(v, id, bytes, transient) != hipSuccess) {
        retry = kCopyRetryCalls;               // no room for another copy of the volume: a family that reads the plain layout serves the call
        return 1;
    }
    float* const dst = copy_ptr(v, id);
    lazy_build_begin(v);
    hipError_t e = hipSuccess;
    if (plan.kind != 8) e = hipMemsetAsync(dst, 0, bytes, v->stream);         // positions beyond the row's width stay zero (the plane-quad relayouts write them themselves)
    if (e == hipSuccess) {
        if (fused_swap12)
            e = launch_relayout_zquad_swap12(v->d_src, dst, v->D, v->H, v->W, v->P, p.sPq, zfir, (p.flags & (1 << 18)) != 0, v->stream);
        else if (zfir)
            e = launch_relayout_zquad_fir(ori.src_plain, dst, ori.srcD, ori.srcH, ori.rowW, ori.rowP, p.sPq, (p.flags & (1 << 18)) != 0, v->stream);
        else if (plan.kind == 8)
            e = launch_relayout_zquad(ori.src_plain, dst, ori.srcD, ori.srcH, ori.rowW, ori.rowP, p.sPq, v->stream);
#ifdef VT_LEGACY
        else
            e = launch_relayout_zpair(ori.src_plain, dst, ori.srcD, ori.srcH, ori.rowW, ori.rowP, p.sP2, v->stream);
#endif
    }
    if (e != hipSuccess) {
        discard_copy(v, id);
        retry = kCopyRetryCalls;
        return 1;
    }
    lazy_build_end(v);
    {   // (lazy_build_end has waited for the relayout: its source may go)
        LazyCopies::Released rel;
        v->lazy.trim(fixed_bytes(v), transient, rel);
        release(v, rel);
    }
    if (std::getenv("VT_DEBUG_ALLOC")) std::fprintf(stderr, "[vt] secondary copy kind %d orientation %d at %p, %zu bytes (plain source %p)\n", plan.kind, ori.quad_idx, (void*)dst, bytes, (const void*)ori.src_plain);
    return ready();
}

// launch the plan's kernel into d_out (the secondary copy it reads exists: ensure_secondary_copy)
int launch_planned(vt_volume* v, const TilePlan& plan, const AffineParams& p, const Orientation& ori, float* d_out, size_t n_out)
{
    if (ori.xswap && !xswap_buffer_ok(v, n_out)) return fail(VT_EINVAL, "internal: exchanged-result copy missing");
    if (plan.kind == 8) {
        float* const srcq = copy_ptr(v, ((p.flags & (1 << 19)) ? kCopyQe0 : kCopyQ0) + ori.quad_idx);
        if (!srcq) return fail(VT_EINVAL, "internal: plane-quad copy missing");
        // Every other launch of a handle walks the chunk layers from the last to the first: the source planes the previous launch
        // read last are still in the memory-side cache (256 MB, it sees reads and writes alike) when this one starts with them.
        // A schedule only: each workgroup computes what it computed before.  (VT_QUAD_PINGPONG=0: always first to last; 2: always
        // last to first -- the control, which measures like 0.)
        AffineParams q = p;
        if (v->tune.quad_pingpong == 2 || (v->tune.quad_pingpong == 1 && ((v->launch_no++) & 1))) q.flags |= (1 << 20);
        // KIND 4 (plan_quad set bit 17): one plan slot per in-plane tile, a new epoch per launch.  A granule left by an earlier launch
        // carries an older epoch and is ignored, so nothing is cleared between launches; the buffer is per handle like its stream.
        if (q.flags & (1 << 17)) {
            const size_t need = (size_t)q.nTh * q.nTw * quad_tile_plan_granules(plan.cfg) * 16;
            if (v->tplan_bytes < need) {
                if (v->d_tplan) { VT_HIP(hipFree(v->d_tplan)); v->d_tplan = nullptr; v->tplan_bytes = 0; }
                VT_HIP(hipMalloc(&v->d_tplan, need));
                v->tplan_bytes = need;
                v->tplan_epoch = 0;
            }
            if (v->tplan_epoch == 0 || v->tplan_epoch == 0xffffffffu) {      // new buffer, or the epochs wrapped: start from zeros again
                VT_HIP(hipMemsetAsync(v->d_tplan, 0, v->tplan_bytes, v->stream));
                v->tplan_epoch = 0;
            }
            q.tplan = v->d_tplan;
            q.tplan_epoch = ++v->tplan_epoch;
        }
        // (Round 5 measured per-launch TILE TABLES here -- the in-plane set-up of every tile worked out once, by a one-layer pass of the same
        //  kernel in front of the real launch, and read back by every chunk layer: bit-identical, the real launch faster and flatter over the
        //  angles, but the pass itself sits in front of every launch with 12-14 us, twice what it saves: 512^3 filt_bspline sweep 0.1983 ms
        //  against 0.1915, 1024^3 1.586 against 1.565, and the second code path cost the default one 1 %.  profiles/r05_tile_tables.txt;
        //  not in the tree.)
        VT_HIP(launch_affine_quad(plan.cfg, v->interp, srcq, d_out, q, plan.grid, plan.lds_bytes, v->stream));
#ifdef VT_LEGACY
    } else if (plan.kind == 5) {
        float* const srcp = copy_ptr(v, kCopyP0 + ori.quad_idx);
        if (!srcp) return fail(VT_EINVAL, "internal: plane-pair copy missing");
        VT_HIP(launch_affine_zpair(plan.cfg, v->interp, srcp, d_out, p, plan.grid, plan.lds_bytes, v->stream));
#endif
    } else if (plan.kind == 9 || plan.kind == 6) {
        if (!v->d_queue) {                                           // tile counters of the persistent kernels: zero between launches
            VT_HIP(hipMalloc(reinterpret_cast<void**>(&v->d_queue), 9 * 128));
            VT_HIP(hipMemsetAsync(v->d_queue, 0, 9 * 128, v->stream));
        }
        if (plan.kind == 9) {
#ifdef VT_EXPERIMENTS      // occupancy experiment: fewer resident workgroups per CU through a larger LDS request / a smaller persistent grid
            static const int exp_lds = std::getenv("VT_EXP_BLOCK_LDS") ? std::atoi(std::getenv("VT_EXP_BLOCK_LDS")) : 0;
            static const int exp_grid = std::getenv("VT_EXP_BLOCK_GRID") ? std::atoi(std::getenv("VT_EXP_BLOCK_GRID")) : 0;
            VT_HIP(launch_affine_block(plan.cfg, plan.th, v->interp, ori.src_plain, d_out, v->d_zeros, v->d_queue, p, plan.geo, exp_grid > 0 ? exp_grid : plan.grid,
                                       std::max(plan.lds_bytes, exp_lds), v->stream));
#else
            VT_HIP(launch_affine_block(plan.cfg, plan.th, v->interp, ori.src_plain, d_out, v->d_zeros, v->d_queue, p, plan.geo, plan.grid, plan.lds_bytes, v->stream));
#endif
        }
        else if (!is_cubic(v->interp) && v->tune.span != 0)
            VT_HIP(launch_affine_span(plan.cfg, ori.src_plain, d_out, v->d_zeros, v->d_queue, p, plan.geo, plan.grid, plan.lds_bytes, v->stream));
        else
            VT_HIP(launch_affine_packed(plan.cfg, v->interp, ori.src_plain, d_out, v->d_zeros, v->d_queue, p, plan.geo, plan.grid, plan.lds_bytes, v->stream));
#ifdef VT_LEGACY
    } else if (plan.kind == 4) {
        VT_HIP(launch_affine_march(plan.cfg, v->interp, ori.src_plain, d_out, p, plan.grid, plan.lds_bytes, v->stream));
#endif
    } else if (plan.kind == 10) {
        VT_HIP(launch_affine_rows(v->interp, plan.td, ori.src_plain, d_out, v->d_zeros, p, plan.lds_bytes, v->stream));
    } else if (plan.kind >= 2) {
        VT_HIP(launch_affine_tiled(plan.cfg, v->interp, plan.kind == 3, ori.src_plain, d_out, v->d_zeros, p, plan.grid, plan.lds_bytes, v->stream));
    } else {
        VT_HIP(launch_affine_direct(v->interp, v->d_src, d_out, p, v->stream));
    }
    note_launch(v, plan.kind >= 2 ? plan.kind : 1, plan, p, n_out);
    return 0;
}

// device staging buffer for a host `out` (recycled through the per-device cache)
int host_output_buffer(vt_volume* v, size_t n_elems, float** d_out)
{
    if (v->scratch_elems < n_elems) {
        if (v->d_scratch_out) { cached_free(v->dev, v->d_scratch_out, v->scratch_elems * sizeof(float)); v->d_scratch_out = nullptr; v->scratch_elems = 0; }
        VT_HIP(cached_malloc(v->dev, reinterpret_cast<void**>(&v->d_scratch_out), n_elems * sizeof(float)));
        v->scratch_elems = n_elems;
    }
    *d_out = v->d_scratch_out;
    return 0;
}

// A VT_STACK handle with a filt_* interpolation holds coefficients that were prefiltered inside each plane only: every entry point that
// samples in three dimensions refuses it (vt_volume_backproject is the one that reads them).
int refuse_in_plane(const vt_volume* v)
{
    if (v->stack && is_filtered(v->interp))
        return fail(VT_EUNSUPPORTED, "the handle's coefficients are in-plane (VT_STACK with a filt_* interpolation): only vt_volume_backproject samples them");
    return 0;
}

int do_affine(vt_volume* v, const double m4x4[16], float* out, int flags)
{
    if (!v || !m4x4 || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    if (v->deferred) return fail(VT_EINVAL, "handle was created with VT_SRC_DEFERRED and has not been finalized (vt_volume_finalize)");
    int rc = use_device(v->dev);
    if (rc) return rc;
    (void)hipGetLastError();                      // a stale sticky error of an unrelated call must not fail this launch's check
    double m[12];
    fold_matrix(v, m4x4, m);
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(m[i])) return fail(VT_EINVAL, "matrix entry %d is not finite", i);

    AffineParams p;
    TilePlan plan;
    Orientation ori;
    const size_t n_out = (size_t)v->oD * v->oH * v->oW;
    struct CallPins {                             // the copies this call touches are pinned until it returns (vt_resident.h)
        LazyCopies& lazy;
        explicit CallPins(LazyCopies& l) : lazy(l) { lazy.begin_call(); }
        ~CallPins() { lazy.end_call(); }
    } pins(v->lazy);
    // Plan, then make sure the resident copy the plan reads exists.  A copy that cannot be built (device memory: a handle that has
    // used every orientation holds up to 8 copies of its volume) takes its kernel family out of the running and the call is
    // planned again: quad -> pair (cubic) / plain marching -> ... every family from kind 4 down reads the plain layout.
    int deny = 0;
    for (int attempt = 0;; ++attempt) {
        std::memset(&p, 0, sizeof(p));
        plan = TilePlan();
        plan.kind = 0;
        ori = Orientation();
        ori.src_plain = v->d_src;
        ori.srcD = v->D; ori.srcH = v->H; ori.rowW = v->W; ori.rowP = v->P;
        const int pf = flags | deny;
        // single-axis rotations about axes 1 / 2 and in-plane maps near a quarter turn march on an exchanged resident copy
        if ((rc = try_rows(v, m, pf, &p, &plan, &ori))) return rc;
        if (plan.kind == 0 && (rc = try_axis1_exchange(v, m, pf, n_out, &p, &plan, &ori))) return rc;
        if (plan.kind == 0 && (rc = try_axis2_exchange(v, m, pf, n_out, &p, &plan, &ori))) return rc;
        if (plan.kind == 0 && (rc = try_inplane_transposed(v, m, pf, n_out, &p, &plan, &ori))) return rc;
        if (plan.kind == 0 && (rc = try_general_reorient(v, m, pf, n_out, &p, &plan, &ori))) return rc;
        if (plan.kind == 0) plan_launch(v, m, pf, &p, &plan);
        const int miss = ensure_secondary_copy(v, plan, p, ori);
        if (miss == 0) break;
        if (attempt >= 3) return fail(VT_EINVAL, "no kernel family can serve this call (secondary resident copies cannot be built)");
        // (the z-convolved copy of KIND 4 missing: the four-plane kernel on the plain plane-quad copy is next in line; a general-matrix
        //  launch whose axis-permuted plain copy could not be built samples the plain copy)
        if (plan.kind == 8) deny |= ((p.flags & (1 << 19)) && !(deny & VT_NO_ZFIR)) ? VT_NO_ZFIR : VT_NO_QUAD;
        else if (plan.kind == 2 || plan.kind == 6 || plan.kind == 9) deny |= VT_NO_REORIENT;
        else deny |= VT_NO_ZPAIR;
    }

    float* d_out = out;
    const bool host_out = !(flags & VT_OUT_DEVICE);
    PinnedScope pin(host_out ? out : nullptr, host_out ? n_out * sizeof(float) : 0);       // the caller's array: in (keep_outside) and out
    if (host_out) {
        if ((rc = host_output_buffer(v, n_out, &d_out))) return rc;
        if (flags & VT_KEEP_OUTSIDE)   // caller's stale values must survive: bring them in first
            VT_HIP(pin.copy(d_out, out, n_out * sizeof(float), hipMemcpyHostToDevice, v->stream));
    }
    float* const d_final = d_out;
    if (ori.xswap) d_out = copy_ptr(v, kCopyTmpX);       // the kernels write the exchanged result [w][h][d]
    if ((rc = launch_planned(v, plan, p, ori, d_out, n_out))) return rc;
    if (ori.xswap)                                // [w][h][d] -> [d][h][w]
        VT_HIP(launch_transpose02(d_out, d_final, v->oW, v->oH, v->oD, (int64_t)v->oH * v->oD, v->oD,
                                  (int64_t)v->oH * v->oW, v->oW, v->stream));
    if (host_out) {
        VT_HIP(pin.copy(out, d_final, n_out * sizeof(float), hipMemcpyDeviceToHost, v->stream));
        VT_HIP(hipStreamSynchronize(v->stream));
    }
    return 0;
}

constexpr int kSrcNone = 1 << 30;   // internal create flag: no source data (zero-filled resident buffer)

// Last step of building a handle: the one-time prefilter of filt_* interpolations over the resident samples
// (transforms.py:195-197, volume.py:48-50), then the handle is usable.
int finalize_resident(vt_volume* v, bool lo_interior)
{
    const int dev = v->dev;
    if (is_filtered(v->interp)) {
        const size_t bytes = v->src_bytes;
        float* d_tmp = nullptr;
        VT_HIP(cached_malloc(dev, reinterpret_cast<void**>(&d_tmp), bytes));
        {
            hipError_t em = hipMemset2DAsync(d_tmp + v->W, (size_t)v->P * sizeof(float), 0, (size_t)(v->P - v->W) * sizeof(float),
                                             (size_t)v->D * v->H, v->stream);
            if (em != hipSuccess) { cached_free(dev, d_tmp, bytes); return fail((int)em, "memset: %s", hipGetErrorString(em)); }
        }
        float* res = nullptr;
        hipEventRecord(v->ev0, v->stream);
        int rc = run_prefilter(v->d_src, d_tmp, v->D, v->H, v->W, v->P, lo_interior, v->stream, &res, v->stack);
        hipEventRecord(v->ev1, v->stream);
        hipError_t es = hipStreamSynchronize(v->stream);
        if (rc || es != hipSuccess) {
            cached_free(dev, d_tmp, bytes);
            if (!rc) rc = fail((int)es, "prefilter: %s", hipGetErrorString(es));
            return rc;
        }
        hipEventElapsedTime(&v->prefilter_ms, v->ev0, v->ev1);
        if (res == d_tmp) { cached_free(dev, v->d_src, bytes); v->d_src = d_tmp; }
        else cached_free(dev, d_tmp, bytes);
    } else {
        VT_HIP(hipStreamSynchronize(v->stream));
    }
    v->deferred = false;
    v->proj_sum_valid = false;
    return 0;
}

int create_common(int dev, int D, int H, int W, int interp, const float* data, int cflags,
                  int64_t plane0, int64_t gD, int64_t out_plane0, int oD, vt_volume_t** out)
{
    if (!out) return fail(VT_EINVAL, "NULL handle pointer");
    *out = nullptr;
    if (!data && !(cflags & (kSrcNone | VT_SRC_DEFERRED))) return fail(VT_EINVAL, "NULL data pointer");
    if (D <= 0 || H <= 0 || W <= 0 || oD <= 0) return fail(VT_EINVAL, "non-positive dims (%d,%d,%d) out depth %d", D, H, W, oD);
    if (interp < VT_LINEAR || interp > VT_FILT_BSPLINE_SIMPLE) return fail(VT_EINVAL, "unknown interpolation code %d", interp);
    if ((int64_t)D * H > 0x7fffffffLL || (int64_t)H * W > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "plane count/size exceeds 2^31");
    if (gD <= 0 || plane0 + D < 0 || plane0 > gD) return fail(VT_EINVAL, "slab window [%lld,%lld) outside global depth %lld",
                                                               (long long)plane0, (long long)(plane0 + D), (long long)gD);
    if (cflags & VT_STACK) {
        if (cflags & VT_EDGE_SCIPY) return fail(VT_EUNSUPPORTED, "VT_STACK cannot be combined with VT_EDGE_SCIPY");
        if (plane0 != 0 || gD != D || out_plane0 != 0 || oD != D) return fail(VT_EUNSUPPORTED, "VT_STACK is available for whole-volume handles only (no slab window)");
        if (cflags & VT_SRC_DEFERRED) return fail(VT_EUNSUPPORTED, "VT_STACK cannot be combined with deferred construction (VT_SRC_DEFERRED)");
    }
    int rc = init_device(dev);
    if (rc) return rc;

    const int uD = D, uH = H, uW = W;              // the caller's dims; D, H, W below are the resident copy's
    int pad = 0;
    if (cflags & VT_EDGE_SCIPY) {
        if (plane0 != 0 || gD != D || out_plane0 != 0 || oD != D || (cflags & (kSrcNone | VT_SRC_DEFERRED)))
            return fail(VT_EUNSUPPORTED, "VT_EDGE_SCIPY is available for whole-volume handles only");
        // one mirrored voxel serves every in-range tap; the prefiltered interpolations carry 16, so that the ordinary prefilter's
        // own boundary treatment sits 16 samples away from the data (|z|^16 = 7e-10) and what reaches the data is the
        // mirror-boundary solution scipy computes
        pad = is_filtered(interp) ? 16 : 1;
        D += 2 * pad; H += 2 * pad; W += 2 * pad;
        gD = D;
        if ((int64_t)D * H > 0x7fffffffLL || (int64_t)H * W > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "plane count/size exceeds 2^31");
    }
    vt_volume* v = new (std::nothrow) vt_volume();
    if (!v) return fail(VT_ENOMEM, "out of host memory");
    v->dev = dev; v->interp = interp; v->D = D; v->H = H; v->W = W;
    v->oD = oD; v->oH = uH; v->oW = uW;
    v->plane0 = plane0; v->gD = gD; v->out_plane0 = out_plane0;
    v->edge_pad = pad;
    v->stack = (cflags & VT_STACK) != 0;
    v->tune.read();
    if (v->tune.max_resident_gb > 0.0) v->lazy.max_resident = (uint64_t)(v->tune.max_resident_gb * 1073741824.0);

    auto cleanup = [&](int code) {
        vt_volume_destroy(v);
        return code;
    };
    if (dev < 64) {
        v->cu_count = g_cu_count[dev];
        v->lds_limit = g_lds_limit[dev];
        v->d_zeros = g_zeros[dev];
    } else {
        return cleanup(fail(VT_ENODEV, "device index %d beyond the supported 64", dev));
    }

#define VT_HIPC(call)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return cleanup(fail((int)e_, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__)); \
    } while (0)

    VT_HIPC(cached_stream(dev, &v->stream));      // blocking stream (see cached_stream)
    VT_HIPC(cached_event(dev, &v->ev0));
    VT_HIPC(cached_event(dev, &v->ev1));
    // resident layout: rows padded to a multiple of 4 floats so every row starts 16-byte aligned (the tiled
    // kernel stages with 16-byte direct-to-LDS loads); pad columns are zero = the border value
    v->P = resident_pitch(W);
    const size_t bytes = (size_t)D * H * v->P * sizeof(float);
    VT_HIPC(cached_malloc(dev, reinterpret_cast<void**>(&v->d_src), bytes));
    v->src_bytes = bytes;
    const hipMemcpyKind kind = (cflags & VT_SRC_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (cflags & (kSrcNone | VT_SRC_DEFERRED)) {
        // internal helper volumes (written by a kernel later) and deferred handles (filled by vt_volume_upload_planes, made
        // usable by vt_volume_finalize): zero-filled -- planes that are never uploaded read as the border colour
        VT_HIPC(hipMemsetAsync(v->d_src, 0, bytes, v->stream));
        VT_HIPC(hipStreamSynchronize(v->stream));
        v->deferred = (cflags & VT_SRC_DEFERRED) != 0;
        v->lo_interior = (cflags & VT_SLAB_LO_INTERIOR) != 0;
        *out = v;
        return 0;
    }
    if (pad > 0) {
        // dense copy of the caller's samples on the device, then one pass writes the mirrored, padded resident copy
        const size_t ubytes = (size_t)uD * uH * uW * sizeof(float);
        float* d_dense = nullptr;
        VT_HIPC(cached_malloc(dev, reinterpret_cast<void**>(&d_dense), ubytes));
        hipError_t ec;
        {
            PinnedScope pin((cflags & VT_SRC_DEVICE) ? nullptr : data, (cflags & VT_SRC_DEVICE) ? 0 : ubytes);
            ec = (cflags & VT_SRC_DEVICE) ? hipMemcpyAsync(d_dense, data, ubytes, kind, v->stream) : pin.copy(d_dense, data, ubytes, kind, v->stream);
            if (ec == hipSuccess) ec = launch_mirror_pad(d_dense, v->d_src, uD, uH, uW, pad, v->P, v->stream);
            if (ec == hipSuccess) ec = hipStreamSynchronize(v->stream);
        }
        cached_free(dev, d_dense, ubytes);
        if (ec != hipSuccess) return cleanup(fail((int)ec, "mirror padding: %s", hipGetErrorString(ec)));
        rc = finalize_resident(v, false);
        if (rc) return cleanup(rc);
        *out = v;
        return 0;
    }
    // only the pad columns need zeroing (a full memset would cost another 4 B/voxel of HBM writes)
    VT_HIPC(hipMemset2DAsync(v->d_src + W, (size_t)v->P * sizeof(float), 0, (size_t)(v->P - W) * sizeof(float), (size_t)D * H, v->stream));
    {
        PinnedScope pin((cflags & VT_SRC_DEVICE) ? nullptr : data, (cflags & VT_SRC_DEVICE) ? 0 : (size_t)D * H * W * sizeof(float));
        if (cflags & VT_SRC_DEVICE)
            VT_HIPC(hipMemcpy2DAsync(v->d_src, (size_t)v->P * sizeof(float), data, (size_t)W * sizeof(float),
                                     (size_t)W * sizeof(float), (size_t)D * H, kind, v->stream));
        else
            VT_HIPC(pin.copy2d(v->d_src, (size_t)v->P * sizeof(float), data, (size_t)W * sizeof(float), (size_t)D * H, true, v->stream));
        VT_HIPC(hipStreamSynchronize(v->stream));
    }

    rc = finalize_resident(v, (cflags & VT_SLAB_LO_INTERIOR) != 0);
    if (rc) return cleanup(rc);
#undef VT_HIPC
    *out = v;
    return 0;
}

// Pipelined one-shot.  The source is uploaded in chunks of planes into ONE resident buffer on a non-blocking
// copy stream; the transform is launched per output slab on the handle's stream as soon as the last chunk that slab taps
// has arrived (stream waits on the upload events); every finished slab is downloaded on a second non-blocking copy stream
// while later chunks are still going up.  The sequence is the one of tools/probes/pipeline_probe.hip (512^3: 12.3 ms
// against 19.8 ms sequential).  Axis-0-separable matrices stream (each output plane taps a window of source
// planes), only the plain resident layout (the secondary copies are built from a complete source).  filt_* interpolations:
// the X and Y passes of the prefilter are plane-local and run per uploaded chunk; the axis-0 pass already works in chunks
// of 64 / 128 planes with 16 planes of warm-up, so each of its chunks is launched as soon as those planes are there.  (A
// resident volume filters axes 0 and 1 with the block-form kernel since round 2: the pipeline's coefficients agree with a
// resident volume's to ~1e-9 relative, not bit for bit; tests/test_gpu_parity.py compares the two paths on filt_*.)  Returns 1
// when the call does not qualify.
// VT_PIPE_TRACE: host-side timeline and per-chunk event times of one pipelined one-shot call
void pipeline_trace(double t_begin, double t_created, double t_pinned, double t_uploads, double t_slabs, double t_done, int nch,
                    const std::vector<hipEvent_t>& ev_up, const std::vector<hipEvent_t>& ev_k, const std::vector<hipEvent_t>& ev_dn)
{
    std::fprintf(stderr, "[pipe] host: create %.2f  alloc+pin %.2f  enqueue uploads %.2f  enqueue slabs %.2f  drain %.2f  total %.2f ms\n",
                 t_created - t_begin, t_pinned - t_created, t_uploads - t_pinned, t_slabs - t_uploads, t_done - t_slabs, t_done - t_begin);
    for (int k = 0; k < nch; ++k) {
        float a = 0, b = 0, c = 0;
        hipEventElapsedTime(&a, ev_up[0], ev_up[(size_t)k]);
        hipEventElapsedTime(&b, ev_up[0], ev_k[(size_t)k]);
        hipEventElapsedTime(&c, ev_up[0], ev_dn[(size_t)k]);
        std::fprintf(stderr, "[pipe] chunk %2d: upload done %+7.2f  kernel done %+7.2f  download done %+7.2f ms\n", k, a, b, c);
    }
}

// may this call take the pipelined path?  (see oneshot_pipelined)
bool pipeline_eligible(const float* h_volume, int D, int H, int W, int interp, const float* m4x4, const float* h_out, int flags)
{
    const size_t n = (size_t)D * H * W;
    if ((flags & (VT_KEEP_OUTSIDE | VT_FORCE_DIRECT | VT_NO_ZSEP | VT_NO_MARCH)) || n * sizeof(float) < ((size_t)32 << 20) || D < 32)
        return false;
    {   // result written over the input (output=volume): slabs would be downloaded over planes still waiting to be uploaded
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(h_volume), b0 = reinterpret_cast<uintptr_t>(h_out);
        if (a0 < b0 + n * sizeof(float) && b0 < a0 + n * sizeof(float)) return false;
    }
    // prefilter passes as run_prefilter orders them for such a volume: X in place, Y into the partner buffer, Z back
    if (is_filtered(interp) && (W > 2048 || prefilter_axis_in_place_ok(1, D, H, W) || prefilter_axis_in_place_ok(0, D, H, W))) return false;
    double m[12];
    for (int i = 0; i < 12; ++i) m[i] = (double)m4x4[i];
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(m[i])) return false;
    // (axis-0-separable matrices stream: an output slab needs a window of source planes.  Any other matrix needs the whole source
    // before its first output voxel; the pipeline still hides the plane-local prefilter passes behind the uploads and the transform
    // behind the downloads -- the floor is the two PCIe transfers back to back.  [measured, tools/oneshot_time.py] 512^3 general
    // rotation: filt_bspline 21.06 -> 20.11 ms, linear 19.76 -> 20.00 (nothing to hide but the chunking's own cost); 250^3 no gain.)
    const bool separable = m[0] == 1.0 && m[1] == 0.0 && m[2] == 0.0 && m[4] == 0.0 && m[8] == 0.0;
    if (!separable && !(is_filtered(interp) && n * sizeof(float) >= ((size_t)256 << 20))) return false;
    return std::fabs(m[3]) < 1.0e9;
}

// Three streams created back to back: the runtime deals hardware queues to streams round-robin (4 queues), and a
// download that shares its hardware queue with the kernels is executed in that queue, in order, by a shader copy at half
// the PCIe rate ([measured] kernel j only started when download j-1 had finished, 27 GB/s) -- so the pipeline's kernels
// run on a stream of their own, created with the two copy streams, not on whichever stream the handle got.
bool pipeline_streams(int dev)
{
    hipStream_t& s_up = g_cache[dev].copy_up;
    hipStream_t& s_dn = g_cache[dev].copy_dn;
    hipStream_t& s_k = g_cache[dev].pipe_k;
    if (s_up && s_dn && s_k) return true;
    if (hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&s_dn, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&s_k, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        s_up = s_dn = s_k = nullptr;         // (a leaked stream on this error path is harmless)
        return false;
    }
    return true;
}

int oneshot_pipelined(int dev, const float* h_volume, int D, int H, int W, int interp, const float* m4x4, float* h_out, int flags)
{
    const size_t n = (size_t)D * H * W;
    if (dev >= 64 || !pipeline_eligible(h_volume, D, H, W, interp, m4x4, h_out, flags)) return 1;
    const bool filt = is_filtered(interp);
    double m[16];
    for (int i = 0; i < 16; ++i) m[i] = (double)m4x4[i];
    std::unique_lock<std::mutex> pipe_lock(g_cache[dev].pipe_mu, std::try_to_lock);
    if (!pipe_lock.owns_lock()) return 1;          // another thread is in the pipeline on this device: plain sequence
    if (!pipeline_streams(dev)) return 1;
    hipStream_t s_up = g_cache[dev].copy_up, s_dn = g_cache[dev].copy_dn, s_k = g_cache[dev].pipe_k;

    static const bool trace = std::getenv("VT_PIPE_TRACE") != nullptr;
    auto now_ms = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now_ms();
    vt_volume_t* v = nullptr;
    int rc = create_common(dev, D, H, W, interp, nullptr, kSrcNone, 0, D, 0, D, &v);
    if (rc) return rc;
    const double t_created = now_ms();
    hipStream_t own_stream = v->stream;           // the slab launches go to the pipeline's kernel stream
    v->stream = s_k;
    float* d_out = nullptr;
    float* d_tmp = nullptr;                        // prefilter ping-pong partner (filt_* only)
    const size_t src_bytes = (size_t)D * H * v->P * sizeof(float);
    int nch = D >= 256 ? 16 : 8;
    if (const char* e = std::getenv("VT_PIPE_NCH")) nch = std::max(1, std::min(D / 2, std::atoi(e)));
    const int Dc = (D + nch - 1) / nch;
    std::vector<hipEvent_t> ev_up((size_t)nch, nullptr), ev_k((size_t)nch, nullptr), ev_dn((size_t)nch, nullptr);
    auto finish = [&](int code) {
        (void)hipStreamSynchronize(s_up);
        (void)hipStreamSynchronize(s_k);
        (void)hipStreamSynchronize(s_dn);
        v->stream = own_stream;
        for (hipEvent_t e : ev_up) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_k) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_dn) if (e) (void)hipEventDestroy(e);
        cached_free(dev, d_out, n * sizeof(float));
        cached_free(dev, d_tmp, src_bytes);
        vt_volume_destroy(v);
        return code;
    };
#define VT_HIPP(call)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) return finish(fail((int)e_, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__)); \
    } while (0)
    VT_HIPP(cached_malloc(dev, reinterpret_cast<void**>(&d_out), n * sizeof(float)));
    if (filt) VT_HIPP(cached_malloc(dev, reinterpret_cast<void**>(&d_tmp), src_bytes));
    // dependency-only events (no timestamps) unless the timeline is being traced
    const unsigned evflags = trace ? hipEventDefault : hipEventDisableTiming;
    for (int k = 0; k < nch; ++k) {
        VT_HIPP(hipEventCreateWithFlags(&ev_up[(size_t)k], evflags)); VT_HIPP(hipEventCreateWithFlags(&ev_k[(size_t)k], evflags));
        if (trace) VT_HIPP(hipEventCreateWithFlags(&ev_dn[(size_t)k], evflags));
    }
    PinnedScope pin_in(h_volume, n * sizeof(float)), pin_out(h_out, n * sizeof(float));
    const double t_pinned = now_ms();

    // uploads: all queued at once, in plane order (events complete in order)
    for (int k = 0; k < nch; ++k) {
        const int z0 = k * Dc, z1 = std::min(D, z0 + Dc);
        if (z0 < z1)
            VT_HIPP(pin_in.copy2d(v->d_src + (size_t)z0 * H * v->P, (size_t)v->P * sizeof(float), h_volume + (size_t)z0 * H * W,
                                  (size_t)W * sizeof(float), (size_t)(z1 - z0) * H, true, s_up));
        VT_HIPP(hipEventRecord(ev_up[(size_t)k], s_up));
    }
    const double t_uploads = now_ms();
    const int halo = is_cubic(interp) ? 2 : 1;
    const bool separable = m[0] == 1.0 && m[1] == 0.0 && m[2] == 0.0 && m[4] == 0.0 && m[8] == 0.0;
    const int lflags = (flags | VT_OUT_DEVICE | VT_NO_ZPAIR | VT_NO_QUAD | VT_NO_RSWAP) & ~VT_KEEP_OUTSIDE;
    // Kernel stream, per uploaded chunk: (filt_*) X and Y passes of the prefilter on the chunk's planes (plane-local), then
    // every axis-0 chunk of the prefilter whose input planes (its own + warm-up) are there, then every output slab whose
    // source planes are final.  The axis-0 pass uses the chunked kernel (prefilter_chunk_size / prefilter_warmup describe ITS grid).
    const int zC = filt ? prefilter_chunk_size(D) : 1;
    const int nzc = filt ? (D + zC - 1) / zC : 0;
    int z_chunks_done = 0, next_slab = 0;
    const int nslabs = (D + Dc - 1) / Dc;
    for (int k = 0; k < nch; ++k) {
        const int z0 = k * Dc, z1 = std::min(D, z0 + Dc);
        if (z0 >= z1) break;
        VT_HIPP(hipStreamWaitEvent(s_k, ev_up[(size_t)k], 0));
        int final_planes = z1;                     // source planes [0, final_planes) hold what the transform samples
        if (filt) {
            const size_t off = (size_t)z0 * H * v->P;
            if (prefilter_xy_ok(z1 - z0, H, W, v->P, v->d_src + off, d_tmp + off)) {
                VT_HIPP(launch_prefilter_xy(v->d_src + off, d_tmp + off, z1 - z0, H, W, v->P, s_k));
            } else {
                VT_HIPP(launch_prefilter_axis(2, v->d_src + off, v->d_src + off, z1 - z0, H, W, v->P, false, s_k));
                VT_HIPP(launch_prefilter_axis(1, v->d_src + off, d_tmp + off, z1 - z0, H, W, v->P, false, s_k));
            }
            int c1 = z_chunks_done;
            while (c1 < nzc && std::min(D, (c1 + 1) * zC + prefilter_warmup()) <= z1) ++c1;
            if (c1 > z_chunks_done) {
                VT_HIPP(launch_prefilter_axis0_chunks(d_tmp, v->d_src, D, H, W, v->P, z_chunks_done, c1, s_k));
                z_chunks_done = c1;
            }
            final_planes = std::min(D, z_chunks_done * zC);
        }
        while (next_slab < nslabs) {
            const int d0 = next_slab * Dc, d1 = std::min(D, d0 + Dc);
            // output plane d of an axis-0-separable map taps source planes floor(d + tz) - halo + 1 ... floor(d + tz) + halo; any
            // other matrix (and the secondary copies its kernels may build) needs every plane
            const double hi = separable ? std::floor((double)(d1 - 1) + m[3]) + halo : (double)(D - 1);
            if (std::min(hi, (double)(D - 1)) >= (double)final_planes) break;          // wait for more planes
            v->out_plane0 = d0;
            v->oD = d1 - d0;
            rc = do_affine(v, m, d_out + (size_t)d0 * H * W, lflags);
            v->out_plane0 = 0;
            v->oD = D;
            if (rc) return finish(rc);
            VT_HIPP(hipEventRecord(ev_k[(size_t)next_slab], s_k));
            ++next_slab;
        }
    }
    if (next_slab < nslabs) return finish(fail(VT_EINVAL, "one-shot pipeline left %d slabs unlaunched", nslabs - next_slab));
    // downloads: each one is queued when its slab is done (host wait -- the calling thread has nothing else to do)
    for (int j = 0; j < nslabs; ++j) {
        const int d0 = j * Dc, d1 = std::min(D, d0 + Dc);
        VT_HIPP(hipEventSynchronize(ev_k[(size_t)j]));
        VT_HIPP(pin_out.copy(h_out + (size_t)d0 * H * W, d_out + (size_t)d0 * H * W, (size_t)(d1 - d0) * H * W * sizeof(float),
                             hipMemcpyDeviceToHost, s_dn));
        if (trace) VT_HIPP(hipEventRecord(ev_dn[(size_t)j], s_dn));
    }
    const double t_slabs = now_ms();
    VT_HIPP(hipStreamSynchronize(s_dn));
    if (trace)
        pipeline_trace(t_begin, t_created, t_pinned, t_uploads, t_slabs, now_ms(), nch, ev_up, ev_k, ev_dn);
#undef VT_HIPP
    return finish(0);
}

// ---------------------------------------------------------------------------------------------------
// the host path of a batched call: checks -> tables in v->h_batch_m -> launch parameters -> scratch on the
// device -> launches -> the record of the launch -> the caller's result.  Each entry point below writes only what is its own.
// ---------------------------------------------------------------------------------------------------

// ---- checks: the codes and texts of the C ABI; their order within an entry point is part of its behaviour ----
int check_batch_size(int n) { return n <= 0 ? fail(VT_EINVAL, "batch size %d", n) : 0; }

// `noun`: "box" or "output"
int check_shape(const char* noun, int d, int h, int w)
{
    if (d <= 0 || h <= 0 || w <= 0) return fail(VT_EINVAL, "non-positive %s dims (%d,%d,%d)", noun, d, h, w);
    if ((int64_t)d * h > 0x7fffffffLL || (int64_t)h * w > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "%s too large", noun);
    return 0;
}

// `what`: the operation, as the refusal names it
int check_whole_volume(const vt_volume* v, const char* what)
{
    if (v->deferred) return fail(VT_EINVAL, "handle has not been finalized (vt_volume_finalize)");
    if (v->plane0 != 0 || v->gD != v->D || v->out_plane0 != 0)
        return fail(VT_EINVAL, "%s is available for whole-volume handles only (this one holds a slab window)", what);
    return 0;
}

// the handle's device, and no stale sticky error of an unrelated call to fail this call's launch check
int select_device(const vt_volume* v)
{
    const int rc = use_device(v->dev);
    if (rc) return rc;
    (void)hipGetLastError();
    return 0;
}

// MT: float or double (an entry point that takes both precisions reads the caller's matrices where they are)
template <typename MT>
int check_finite_matrices(const MT* m4x4s, size_t n)
{
    for (size_t i = 0; i < n * 16; ++i)
        if (!std::isfinite(m4x4s[i])) return fail(VT_EINVAL, "matrix %zu entry %zu is not finite", i / 16, i % 16);
    return 0;
}

int check_finite_weights(const double* weights, size_t n)      // weights == nullptr: ones
{
    if (weights)
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(weights[i])) return fail(VT_EINVAL, "weight %zu is not finite", i);
    return 0;
}

// back-projection reads in-plane coefficients, never a padded copy, and one image per entry
int check_backproject_handle(const vt_volume* v)
{
    if (int rc = check_whole_volume(v, "back-projection")) return rc;
    if (is_filtered(v->interp) && !v->stack)
        return fail(VT_EUNSUPPORTED, "the handle's coefficients are prefiltered along axis 0 as well: back-projection with a filt_* interpolation "
                                     "needs in-plane coefficients (create the handle with VT_STACK)");
    if (v->edge_pad) return fail(VT_EUNSUPPORTED, "back-projection is not available on VT_EDGE_SCIPY handles");
    return 0;
}

int check_planes(const vt_volume* v, int n, const int32_t* planes, const char* per)
{
    if (planes) {
        for (int i = 0; i < n; ++i)
            if (planes[i] < 0 || planes[i] >= v->D) return fail(VT_EINVAL, "plane index %d of entry %d outside [0, %d)", planes[i], i, v->D);
    } else if (n != v->D) {
        return fail(VT_EINVAL, "%d matrices%s for a stack of %d images and no plane indices", n, per, v->D);
    }
    return 0;
}

// ---- tables: v->h_batch_m is the staging vector of every batched call, ExtractEntry first, the call's other tables behind them ----
static_assert(sizeof(ExtractEntry) % sizeof(double) == 0, "the staging vector of doubles holds whole table entries");
constexpr size_t kEntryDoubles = sizeof(ExtractEntry) / sizeof(double);

ExtractEntry* host_entries(vt_volume* v) { return reinterpret_cast<ExtractEntry*>(v->h_batch_m.data()); }
const ExtractEntry* device_entries(const vt_volume* v) { return reinterpret_cast<const ExtractEntry*>(v->d_batch_m); }

// The staging vector, `doubles` long, once no copy of an earlier call can still be reading it.  What a call does not write keeps what
// an earlier call left.
int begin_tables(vt_volume* v, size_t doubles)
{
    VT_HIP(hipStreamSynchronize(v->stream));          // the previous batch may still be reading the staging vector
    v->h_batch_m.resize(doubles);
    return 0;
}

struct TableDims {
    int L[3];              // the largest staged box over the entries (the two-patch form of back-projection: 2, rows, row stride)
    int lds_bytes;         // dynamic LDS of the launch
};

// The table of the three-dimensional family (kinds 11-17): n entries in front of `extra` doubles.  min_lds: what the kernel needs
// whatever the entries stage.
int build_box_table(vt_volume* v, const double* m4x4s, int n, size_t extra, int cfg, bool force_direct, int min_lds, TableDims* dims)
{
    if (int rc = begin_tables(v, (size_t)n * kEntryDoubles + extra)) return rc;
    ExtractEntry* const e = host_entries(v);
    const bool cubic = is_cubic(v->interp);
    const double pad = (double)v->edge_pad;
    int64_t lds_bytes = min_lds;
    int L[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
        double m[12];                                   // fold_matrix on a whole-volume handle: the matrix, plus the pad
        std::memcpy(m, m4x4s + 16 * (size_t)i, sizeof(m));
        m[3] += pad; m[7] += pad; m[11] += pad;
        extract_fill_entry(m, cfg, cubic, v->lds_limit, force_direct, &e[i]);
        if (e[i].tiled) {
            L[0] = std::max(L[0], e[i].Lz); L[1] = std::max(L[1], e[i].Ly); L[2] = std::max(L[2], e[i].Lx);
            lds_bytes = std::max<int64_t>(lds_bytes, (int64_t)e[i].Lz * e[i].Ly * e[i].Lx * 4);
        }
    }
    *dims = TableDims{{L[0], L[1], L[2]}, (int)lds_bytes};
    return 0;
}

// The tables of the back-projection family (kinds 18, 19): nb x n entries, then as many weights (nullptr: ones).  Entry k belongs to
// image planes[k % n] (nullptr: k % n), which is row 0 of its matrix; rows 1 and 2 are the caller's.  An entry stages into LDS when two
// patches of ITS size fit lds_limit (the kernel keeps the next entry's patch in flight while it samples), whatever the rest of the batch
// holds; the largest staged patch only sizes the allocation and places the second buffer.  *buf_floats: that patch, in floats.
// MT: float or double matrices, widened entry by entry (no nb x n x 16 float64 copy of a float32 batch).
template <typename MT>
int build_backproject_tables(vt_volume* v, const MT* m4x4s, int nb, int n, const int32_t* planes, const double* weights, int cfg,
                             bool force_direct, TableDims* dims, int* buf_floats)
{
    const size_t total = (size_t)nb * (size_t)n;      // < 2^31 pairs of 200 bytes: no overflow
    if (int rc = begin_tables(v, total * (kEntryDoubles + 1))) return rc;
    ExtractEntry* const e = host_entries(v);
    double* const w = v->h_batch_m.data() + kEntryDoubles * total;
    const bool cubic = is_cubic(v->interp);
    int64_t largest = 4;
    dims->L[0] = 2; dims->L[1] = dims->L[2] = 0;
    int i = 0;                                        // k % n, without a division per entry
    for (size_t k = 0; k < total; ++k, i = (i + 1 == n) ? 0 : i + 1) {
        const MT* a = m4x4s + 16 * k;
        const double m[12] = {0, 0, 0, (double)(planes ? planes[i] : i), (double)a[4], (double)a[5], (double)a[6], (double)a[7],
                              (double)a[8], (double)a[9], (double)a[10], (double)a[11]};
        // tile reach, Q32.32 increments and patch dims by extract_box_dims' rule (no cap: the cap below is on two 2-D patches)
        extract_fill_entry(m, cfg, cubic, 0x7fffffff, false, &e[k]);
        const int64_t patch = (int64_t)e[k].Ly * e[k].Lx;
        if (e[k].tiled && !force_direct && 2 * patch * 4 <= (int64_t)v->lds_limit) {
            if (patch > largest || dims->L[1] == 0) { dims->L[1] = e[k].Ly; dims->L[2] = e[k].Lx; }
            largest = std::max(largest, patch);
        } else {
            e[k].tiled = 0;
        }
        w[k] = weights ? weights[k] : 1.0;
    }
    *buf_floats = (int)largest;
    dims->lds_bytes = (int)(2 * largest * 4);
    return 0;
}

// ---- launch parameters ----
struct BoxTiles {
    int cfg;               // extract_tile's index
    int T[3], nT[3];       // the tile, and tiles per axis of the shape
    int64_t count;         // nT[0] x nT[1] x nT[2]
};

BoxTiles box_tiles(int cfg, int d, int h, int w)
{
    BoxTiles t;
    t.cfg = cfg;
    extract_tile(cfg, &t.T[0], &t.T[1], &t.T[2]);
    const int shape[3] = {d, h, w};
    for (int k = 0; k < 3; ++k) t.nT[k] = (shape[k] + t.T[k] - 1) / t.T[k];
    t.count = (int64_t)t.nT[0] * t.nT[1] * t.nT[2];
    return t;
}

// AffineParams of a launch that writes shape (d, h, w) from the tables in v->h_batch_m: source dims, output dims, valid interval, and
// `nT` tiles per axis
AffineParams box_params(const vt_volume* v, int d, int h, int w, const int nT[3])
{
    AffineParams p;
    std::memset(&p, 0, sizeof(p));
    TilePlan plan;
    const vt_volume view = planning_view(v, v->D, v->H, v->W, v->P, d, h, w, true);
    plan_launch(&view, v->h_batch_m.data(), VT_FORCE_DIRECT, &p, &plan);
    p.nTd = nT[0]; p.nTh = nT[1]; p.nTw = nT[2];
    return p;
}

// ---- scratch on the device: grown when too small, never shrunk ----
// v->h_batch_m, whole, into v->d_batch_m on the handle's stream
int upload_tables(vt_volume* v)
{
    const std::vector<double>& tab = v->h_batch_m;
    if (v->batch_m_cap < tab.size()) {
        if (v->d_batch_m) { VT_HIP(hipFree(v->d_batch_m)); v->d_batch_m = nullptr; v->batch_m_cap = 0; }
        VT_HIP(hipMalloc(reinterpret_cast<void**>(&v->d_batch_m), tab.size() * sizeof(double)));
        v->batch_m_cap = tab.size();
    }
    // (pageable host memory never travels in pieces the runtime would pin in place: PinnedScope, rule 1)
    VT_HIP(PinnedScope::sliced(reinterpret_cast<char*>(v->d_batch_m), reinterpret_cast<const char*>(tab.data()), tab.size() * sizeof(double),
                               hipMemcpyHostToDevice, v->stream));
    return 0;
}

// v->d_proj_part: the float64 partial sums a launch leaves for its reduction
int ensure_partials(vt_volume* v, size_t bytes)
{
    if (v->proj_part_bytes < bytes) {
        if (v->d_proj_part) { cached_free(v->dev, v->d_proj_part, v->proj_part_bytes); v->d_proj_part = nullptr; v->proj_part_bytes = 0; }
        VT_HIP(cached_malloc(v->dev, reinterpret_cast<void**>(&v->d_proj_part), bytes));
        v->proj_part_bytes = bytes;
    }
    return 0;
}

// ---- the caller's result array: the launches write ptr(), which is `out` itself (VT_OUT_DEVICE) or the handle's staging buffer ----
struct ResultScope {
    vt_volume* v;
    void* out;
    size_t bytes;
    bool host_out;
    PinnedScope pin;       // the caller's array: in (copy_in) and out
    void* d_out;
    ResultScope(vt_volume* v_, void* out_, size_t bytes_, bool host_out_)
        : v(v_), out(out_), bytes(bytes_), host_out(host_out_), pin(host_out_ ? out_ : nullptr, host_out_ ? bytes_ : 0), d_out(out_) {}
    // copy_in: the caller's contents count (VT_ACCUMULATE, VT_KEEP_OUTSIDE) and go to the device first
    int open(bool copy_in = false)
    {
        if (!host_out) return 0;
        float* d_stage = nullptr;
        if (int rc = host_output_buffer(v, (bytes + sizeof(float) - 1) / sizeof(float), &d_stage)) return rc;
        d_out = d_stage;
        if (copy_in) VT_HIP(pin.copy(d_out, out, bytes, hipMemcpyHostToDevice, v->stream));
        return 0;
    }
    template <typename T> T* ptr() const { return static_cast<T*>(d_out); }
    // a host result is complete when this returns; a device result is ordered on the handle's stream
    int finish()
    {
        if (!host_out) return 0;
        VT_HIP(pin.copy(out, d_out, bytes, hipMemcpyDeviceToHost, v->stream));
        VT_HIP(hipStreamSynchronize(v->stream));
        return 0;
    }
};

// ---- the record of the launch (vt_volume_info); T, L == nullptr: zeros ----
void record_launch(vt_volume* v, int kind, const int T[3], const int L[3], int lds_bytes, int64_t grid)
{
    v->last_kernel = kind;
    for (int k = 0; k < 3; ++k) { v->last_tile[k] = T ? T[k] : 0; v->last_lds[k] = L ? L[k] : 0; }
    v->last_lds_bytes = lds_bytes;
    v->last_grid = (int)grid;
}

// the batched direct kernel over `n` matrices of 12 doubles in v->d_batch_m, 65535 at a time, each writing n_out voxels
int launch_direct_batches(vt_volume* v, int n, float* d_out, size_t n_out, const AffineParams& p)
{
    for (int first = 0; first < n; first += 65535) {
        const int cnt = std::min(65535, n - first);
        VT_HIP(launch_affine_direct_batch(v->interp, v->d_src, d_out + (size_t)first * n_out, v->d_batch_m + 12 * (size_t)first,
                                          cnt, p, v->stream));
    }
    record_launch(v, 1, nullptr, nullptr, 0, (int64_t)((n_out + 255) / 256));
    return 0;
}

// n transforms of one resident volume in one call.  Small volumes (the launch-latency regime: template
// rotations, sub-tomogram alignment) take ONE launch of the batched direct kernel, 65535 matrices at a time; larger
// ones are queued back to back on the handle's stream without returning to the caller in between.
int do_affine_batch(vt_volume* v, int n, const double* m4x4s, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    if (v->deferred) return fail(VT_EINVAL, "handle has not been finalized (vt_volume_finalize)");
    int rc = check_batch_size(n);
    if (rc || (rc = use_device(v->dev))) return rc;
    const size_t n_out = (size_t)v->oD * v->oH * v->oW;
    const bool small = n_out <= (size_t)96 * 96 * 96 && !(flags & VT_FORCE_TILED);
    if (!small) {
        for (int i = 0; i < n; ++i) {
            rc = do_affine(v, m4x4s + 16 * (size_t)i, out + (size_t)i * n_out, flags);
            if (rc) return rc;
        }
        return 0;
    }
    if ((rc = check_finite_matrices(m4x4s, (size_t)n))) return rc;
    // 12 doubles per matrix, the output-plane / slab offsets folded exactly as do_affine does
    if ((rc = begin_tables(v, (size_t)n * 12))) return rc;
    for (int i = 0; i < n; ++i) fold_matrix(v, m4x4s + 16 * (size_t)i, v->h_batch_m.data() + 12 * (size_t)i);
    AffineParams p;
    std::memset(&p, 0, sizeof(p));
    TilePlan plan;
    plan_launch(v, v->h_batch_m.data(), (flags & VT_KEEP_OUTSIDE) | VT_FORCE_DIRECT, &p, &plan);   // dims, valid interval, flags
    if ((rc = upload_tables(v))) return rc;
    ResultScope res(v, out, n_out * (size_t)n * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open((flags & VT_KEEP_OUTSIDE) != 0))) return rc;
    if ((rc = launch_direct_batches(v, n, res.ptr<float>(), n_out, p))) return rc;
    return res.finish();
}

// Which box shapes the batched extraction kernel (kind 11) serves by default; the others take the batched direct kernel.
// The rule follows from profiles/pr_extract.txt: out of a 1024 x 1024 x 512 source kernel 11 took 0.24 / 1.45 /
// 4.55 / 10.85 us per trilinear box of 32^3 / 64^3 / 96^3 / 128^3 where the former path took 0.66 / 4.62 / 16.74 / 15.45, and
// 0.42 / 2.70 / 9.06 / 22.11 against 2.86 / 22.15 / 81.19 / 29.13 for filt_bspline -- no measured shape is better off on the old path.
// VT_FORCE_TILED / VT_FORCE_DIRECT override the rule.
bool extract_routes_tiled(int interp, int bd, int bh, int bw)
{
    (void)interp; (void)bd; (void)bh; (void)bw;
    return true;
}

// n boxes of one shape cut out of the resident volume, one pull matrix each (sub-tomogram extraction): scipy's output_shape
// (transforms.py:136-150) per matrix, in one launch.  Does not read or change the handle's own output shape.
int do_extract(vt_volume* v, int n, const double* m4x4s, int bd, int bh, int bw, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    int rc = check_batch_size(n);
    if (rc || (rc = check_shape("box", bd, bh, bw)) || (rc = check_whole_volume(v, "box extraction")) || (rc = select_device(v)) ||
        (rc = check_finite_matrices(m4x4s, (size_t)n)))
        return rc;

    const int box[3] = {bd, bh, bw};
    const size_t n_box = (size_t)bd * bh * bw;
    const bool tiled = (flags & VT_FORCE_TILED) || (!(flags & VT_FORCE_DIRECT) && extract_routes_tiled(v->interp, bd, bh, bw));
    const BoxTiles t = box_tiles(extract_pick_tile(is_cubic(v->interp), box, nullptr), bd, bh, bw);

    // the launch's table: ExtractEntry per matrix (kind 11) or 12 doubles per matrix (batched direct kernel)
    TableDims dims;
    if (tiled) {
        if ((rc = build_box_table(v, m4x4s, n, 0, t.cfg, false, 16, &dims))) return rc;
    } else {
        if ((rc = begin_tables(v, (size_t)n * 12))) return rc;
        for (int i = 0; i < n; ++i) fold_matrix(v, m4x4s + 16 * (size_t)i, v->h_batch_m.data() + 12 * (size_t)i);
    }
    const AffineParams p = box_params(v, bd, bh, bw, t.nT);
    if (tiled && t.count > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "box too large");

    if ((rc = upload_tables(v))) return rc;
    ResultScope res(v, out, n_box * (size_t)n * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open())) return rc;
    if (tiled) {
        int64_t last_grid = 0;
        const int per_launch = (int)std::min<int64_t>(n, 0x7fffffffLL / t.count);
        for (int first = 0; first < n; first += per_launch) {
            const int cnt = std::min(per_launch, n - first);
            last_grid = t.count * cnt;
            VT_HIP(launch_extract(t.cfg, v->interp, v->d_src, res.ptr<float>() + (size_t)first * n_box, v->d_zeros, device_entries(v) + first, p,
                                  last_grid, dims.lds_bytes, v->stream));
        }
        record_launch(v, 11, t.T, dims.L, dims.lds_bytes, last_grid);
    } else if ((rc = launch_direct_batches(v, n, res.ptr<float>(), n_box, p))) {
        return rc;
    }
    return res.finish();
}

// Axis-0 projection: out[h, w] = sum_d affine(m)[d, h, w]  (see vt_kernels_project.hip)
int do_project(vt_volume* v, const double m4x4[16], float* out, int flags)
{
    if (!v || !m4x4 || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    if (v->deferred) return fail(VT_EINVAL, "handle has not been finalized (vt_volume_finalize)");
    int rc = use_device(v->dev);
    if (rc) return rc;
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(m4x4[i])) return fail(VT_EINVAL, "matrix entry %d is not finite", i);
    // fold the output-plane / slab offsets exactly as do_affine does
    double m[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 4; ++c) m[4 * r + c] = m4x4[4 * r + c];
        m[4 * r + 3] = std::fma(m4x4[4 * r], (double)v->out_plane0, m4x4[4 * r + 3]);
    }
    m[3] -= (double)v->plane0;
    const bool host_out = !(flags & VT_OUT_DEVICE);
    const size_t n2 = (size_t)v->oH * v->oW;
    // (VT_EDGE_SCIPY handles: the fused plane sum assumes the texture contract's skirt; they transform, then sum)
    const bool zsep = v->edge_pad == 0 && !(flags & VT_NO_ZSEP) && m[0] == 1.0 && m[1] == 0.0 && m[2] == 0.0 && m[4] == 0.0 && m[8] == 0.0 &&
                      std::fabs(m[3]) < 1.0e9;
    if (zsep) {
        if (!v->proj) {
            const int kind = !is_cubic(v->interp) ? VT_LINEAR
                             : ((v->interp == VT_BSPLINE_SIMPLE || v->interp == VT_FILT_BSPLINE_SIMPLE) ? VT_BSPLINE_SIMPLE : VT_BSPLINE);
            vt_volume* h = nullptr;
            rc = create_common(v->dev, 3, v->H, v->W, kind, nullptr, kSrcNone, 0, 3, 1, 1, &h);
            if (rc) return rc;
            recycle_stream(h->dev, h->stream);   // the helper runs on this handle's stream (ordered after the sum)
            h->stream = v->stream;
            h->owns_stream = false;
            v->proj = h;
        }
        vt_volume* h = v->proj;
        h->oD = 1; h->oH = v->oH; h->oW = v->oW;
        ProjectParams q;
        std::memset(&q, 0, sizeof(q));
        q.D = v->D; q.H = v->H;
        q.vec = 4; q.nxv = (v->P - 4) / 4;
        q.src_pitch = v->P; q.dst_pitch = h->P; q.dst_plane = (int64_t)h->H * h->P; q.copies = 3;
        q.uniform = 0;
        const double fl = std::floor(m[3]);
        q.zoff = (int)fl;
        const float fz = (float)(m[3] - fl);
        if (!is_cubic(v->interp)) {
            q.halo = 0; q.ntap = 2; q.wz[0] = 1.0f - fz; q.wz[1] = fz;
        } else {
            q.halo = 1; q.ntap = 4;
            if (v->interp == VT_BSPLINE_SIMPLE || v->interp == VT_FILT_BSPLINE_SIMPLE) cubic_weights<true>(fz, q.wz);
            else cubic_weights<false>(fz, q.wz);
        }
        // valid output planes: 0 <= d < oD and the skirt rule vlo <= d + m[3] < vhi on the resident coordinates
        const double vlo = -0.5 - (double)v->plane0, vhi = (double)v->gD - 0.5 - (double)v->plane0;
        const double dlo = std::max(0.0, std::ceil(vlo - m[3])), dhi = std::min((double)v->oD - 1.0, std::ceil(vhi - m[3]) - 1.0);
        q.dlo = (int)std::max(-1.0e9, std::min(1.0e9, dlo));
        q.dhi = (int)std::max(-1.0e9, std::min(1.0e9, dhi));
        // The weighted plane sum depends on the axis-0 part of the map alone (offset m[3], output depth, slab offsets folded into
        // m[3]): a tilt series about the projection axis (examples/projections.py:20-26) asks for the same sum at every angle.
        // The helper keeps it; only the 2-D interpolation below runs again (512^3: 0.112 ms -> 0.01 ms per projection).
        if (v->tune.no_proj_cache || !(v->proj_sum_valid && v->proj_sum_m3 == m[3] && v->proj_sum_oD == v->oD && v->proj_sum_oplane0 == v->out_plane0)) {
            v->proj_sum_valid = false;
            VT_HIP(launch_plane_sum(v->d_src, h->d_src, q, v->stream));
            v->proj_sum_valid = true; v->proj_sum_m3 = m[3]; v->proj_sum_oD = v->oD; v->proj_sum_oplane0 = v->out_plane0;
        }
        double m2[16] = {1, 0, 0, 0, 0, m[5], m[6], m[7], 0, m[9], m[10], m[11], 0, 0, 0, 1};
        // the helper's planes change with every call: no cached pair copy, and a 2-D image does not need LDS staging
        rc = do_affine(h, m2, out, (flags & VT_OUT_DEVICE) | VT_FORCE_DIRECT);
        record_launch(v, 7, nullptr, nullptr, 0, 0);
        return rc;
    }

    // general matrices: transform into scratch, then sum the planes
    const size_t n_out = (size_t)v->oD * n2;
    if (v->proj_tmp_elems < n_out) {
        if (v->d_proj_tmp) { VT_HIP(hipFree(v->d_proj_tmp)); v->d_proj_tmp = nullptr; v->proj_tmp_elems = 0; }
        VT_HIP(hipMalloc(reinterpret_cast<void**>(&v->d_proj_tmp), n_out * sizeof(float)));
        v->proj_tmp_elems = n_out;
    }
    rc = do_affine(v, m4x4, v->d_proj_tmp, (flags & ~VT_KEEP_OUTSIDE) | VT_OUT_DEVICE);
    if (rc) return rc;
    float* d_out = out;
    if (host_out) {
        if (v->scratch_elems < n2) {
            if (v->d_scratch_out) { cached_free(v->dev, v->d_scratch_out, v->scratch_elems * sizeof(float)); v->d_scratch_out = nullptr; v->scratch_elems = 0; }
            VT_HIP(cached_malloc(v->dev, reinterpret_cast<void**>(&v->d_scratch_out), n2 * sizeof(float)));
            v->scratch_elems = n2;
        }
        d_out = v->d_scratch_out;
    }
    ProjectParams q;
    std::memset(&q, 0, sizeof(q));
    q.D = v->oD; q.H = v->oH;
    q.vec = (v->oW % 4 == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0) ? 4 : 1;
    q.nxv = v->oW / q.vec;
    q.src_pitch = v->oW; q.dst_pitch = v->oW; q.dst_plane = 0; q.copies = 1; q.uniform = 1;
    VT_HIP(launch_plane_sum(v->d_proj_tmp, d_out, q, v->stream));
    if (host_out) {
        PinnedScope pin(out, n2 * sizeof(float));
        VT_HIP(pin.copy(out, d_out, n2 * sizeof(float), hipMemcpyDeviceToHost, v->stream));
        VT_HIP(hipStreamSynchronize(v->stream));
    }
    return 0;
}

// Which (output shape, interpolation) classes vt_volume_project_batch sends to the fused kernel (kind 12) by default; the others loop over
// do_project inside the call.  A class takes kernel 12 only where profiles/pr_project_batch.txt shows it to be no
// slower than that loop by more than the round-to-round spread (<= 0.005 ms on every row); ms per projection, loop -> kernel 12:
//   trilinear     64^3 0.012 -> 0.003, 128^3 0.017 -> 0.009, 256^3 0.040 -> 0.032: kernel 12 up to 256 in every dimension;
//                 512^3: 0.264 -> 0.285 (61 tilts about axis 1), 0.275 -> 0.259 (about axis 2), 0.267 -> 0.341 (n = 1), 0.499 -> 0.634 (24 random
//                 rotations): it loses three rows of four, and the rule cannot see the matrices, so the class loops;
//   filt_bspline  64^3 0.014 -> 0.006: kernel 12 up to 64 in every dimension; 128^3 0.019 -> 0.024, 256^3 0.047 -> 0.149, 512^3 0.273 -> 1.147 /
//                 0.358 -> 0.941 / 0.276 -> 1.160 / 0.986 -> 2.129: loop.  `bspline` runs the same instantiations on both arms and follows it.
// Shapes between two measured sizes belong to the larger one's class; bspline_simple / filt_bspline_simple (kernel 12's KIND 2) were not
// measured and loop.  VT_FORCE_TILED / VT_FORCE_DIRECT override the rule.
bool project_batch_routes_fused(int interp, int depth, int height, int width)
{
    const int longest = std::max(depth, std::max(height, width));
    if (interp == VT_LINEAR) return longest <= 256;
    if (interp == VT_BSPLINE || interp == VT_FILT_BSPLINE) return longest <= 64;
    return false;
}

// n projections of the resident volume along output axis 0, one pull matrix each (a tilt series), with an output shape of the call's own:
// image i = sum over d < depth of what vt_volume_affine would write for matrix i at output shape (depth, height, width).
int do_project_batch(vt_volume* v, int n, const double* m4x4s, int depth, int height, int width, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    int rc = check_batch_size(n);
    if (rc || (rc = check_shape("output", depth, height, width)) || (rc = check_whole_volume(v, "batched projection")) ||
        (rc = select_device(v)) || (rc = check_finite_matrices(m4x4s, (size_t)n)))
        return rc;

    const size_t n2 = (size_t)height * width;
    const bool fused = (flags & VT_FORCE_TILED) || (!(flags & VT_FORCE_DIRECT) && project_batch_routes_fused(v->interp, depth, height, width));
    ResultScope res(v, out, n2 * (size_t)n * sizeof(float), !(flags & VT_OUT_DEVICE));

    if (!fused) {
        // the single-matrix path, once per matrix, on the requested output shape (the handle's own shape is put back before the call returns;
        // calls on a handle are serialised).  Each image goes to its place in the device buffer; a host `out` is copied once at the end.
        if ((rc = res.open())) return rc;
        struct ShapeScope {
            vt_volume* v; int d, h, w;
            ShapeScope(vt_volume* v_, int od, int oh, int ow) : v(v_), d(v_->oD), h(v_->oH), w(v_->oW) { v->oD = od; v->oH = oh; v->oW = ow; }
            ~ShapeScope() { v->oD = d; v->oH = h; v->oW = w; }
        } shape(v, depth, height, width);
        const int lf = (flags & ~(VT_FORCE_DIRECT | VT_FORCE_TILED | VT_KEEP_OUTSIDE)) | VT_OUT_DEVICE;
        for (int i = 0; i < n; ++i)
            if ((rc = do_project(v, m4x4s + 16 * (size_t)i, res.ptr<float>() + (size_t)i * n2, lf))) return rc;
        return res.finish();
    }
    int cfg = 0, nseg = 1, tps = 1;
    project_batch_shape_plan(is_cubic(v->interp), depth, height, width, &cfg, &nseg, &tps);
    const BoxTiles t = box_tiles(cfg, depth, height, width);

    TableDims dims;
    if ((rc = build_box_table(v, m4x4s, n, 0, cfg, false, 2048, &dims))) return rc;      // 256 doubles: the lane groups of the small tiles meet in LDS
    AffineParams p = box_params(v, depth, height, width, t.nT);
    p.nTd = nseg; p.dch = tps;                        // depth: segments of tps tiles
    const int64_t units = (int64_t)nseg * p.nTh * p.nTw;
    if (units > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "output too large");

    // matrices per launch: the grid limit, and partial sums of no more than max(one output volume in float32, one matrix's partials)
    int64_t per_launch = std::min<int64_t>(n, 0x7fffffffLL / units);
    if (nseg > 1) {
        const size_t image_bytes = (size_t)nseg * n2 * sizeof(double);
        const size_t cap = std::max((size_t)depth * n2 * sizeof(float), image_bytes);
        per_launch = std::min<int64_t>(per_launch, (int64_t)(cap / image_bytes));
        if ((rc = ensure_partials(v, image_bytes * (size_t)per_launch))) return rc;
    }
    if ((rc = upload_tables(v)) || (rc = res.open())) return rc;

    int64_t last_grid = 0;
    for (int first = 0; first < n; first += (int)per_launch) {
        const int cnt = (int)std::min<int64_t>(per_launch, n - first);
        float* const d_img = res.ptr<float>() + (size_t)first * n2;
        last_grid = units * cnt;
        VT_HIP(launch_project_tiled(cfg, v->interp, v->d_src, d_img, v->d_proj_part, v->d_zeros, device_entries(v) + first, p, last_grid,
                                    dims.lds_bytes, v->stream));
        if (nseg > 1) VT_HIP(launch_project_reduce(v->d_proj_part, d_img, nseg, (int64_t)n2, cnt, v->stream));
    }
    record_launch(v, 12, t.T, dims.L, dims.lds_bytes, last_grid);
    return res.finish();
}

// One box: the weighted sum of the n boxes do_extract would write (sub-tomogram averaging; symmetrisation with the volume as the box), in
// one launch of kernel 13 (vt_kernels_extractsum.hip) and, when the matrices are split into segments, a small reduction.  The boxes are
// never written.  Does not read or change the handle's own output shape.
int do_extract_sum(vt_volume* v, int n, const double* m4x4s, const double* weights, int bd, int bh, int bw, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    int rc = check_batch_size(n);
    if (rc || (rc = check_shape("box", bd, bh, bw)) || (rc = check_whole_volume(v, "box summation")) || (rc = select_device(v)) ||
        (rc = check_finite_matrices(m4x4s, (size_t)n)) || (rc = check_finite_weights(weights, (size_t)n)))
        return rc;

    const int box[3] = {bd, bh, bw};
    const size_t n_box = (size_t)bd * bh * bw;
    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);
    int cfg = 0, nseg = 1, per_seg = n;
    extract_sum_shape_plan(is_cubic(v->interp), box, n, &cfg, &nseg, &per_seg);
    const BoxTiles t = box_tiles(cfg, bd, bh, bw);

    // the launch's tables: one ExtractEntry per matrix, then the n weights
    TableDims dims;
    if ((rc = build_box_table(v, m4x4s, n, (size_t)n, cfg, force_direct, 16, &dims))) return rc;
    double* const w = v->h_batch_m.data() + kEntryDoubles * (size_t)n;
    for (int i = 0; i < n; ++i) w[i] = weights ? weights[i] : 1.0;
    const AffineParams p = box_params(v, bd, bh, bw, t.nT);
    const int64_t grid = t.count * nseg;
    if (grid > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "box too large");

    if (nseg > 1 && (rc = ensure_partials(v, (size_t)nseg * n_box * sizeof(double)))) return rc;      // tiles x nseg < 2048: under 64 MiB
    if ((rc = upload_tables(v))) return rc;
    ResultScope res(v, out, n_box * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open())) return rc;

    VT_HIP(launch_extract_sum(cfg, v->interp, v->d_src, res.ptr<float>(), v->d_proj_part, v->d_zeros, device_entries(v),
                              v->d_batch_m + kEntryDoubles * (size_t)n, n, per_seg, nseg, p, dims.lds_bytes, v->stream));
    if (nseg > 1) VT_HIP(launch_project_reduce(v->d_proj_part, res.ptr<float>(), nseg, (int64_t)n_box, 1, v->stream));
    record_launch(v, 13, t.T, dims.L, dims.lds_bytes, grid);
    return res.finish();
}

// The part of the two scoring entry points' checks that is the same: kernels 14 and 15 index a template and the mask with 32 bits.
int check_dot_box(const vt_volume* v, int bd, int bh, int bw)
{
    if (int rc = check_shape("box", bd, bh, bw)) return rc;
    if ((int64_t)(bd + 16) * bh * bw > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "box too large");
    return check_whole_volume(v, "box scoring");
}

// n x 3 float64: (sum mask * B_i, sum mask * B_i^2, sum tmpl * B_i) over the voxels of each box B_i do_extract would write (scoring n candidate
// poses against one template), in launches of kernel 14 (vt_kernels_extractdot.hip), each followed by its small reduction over the tiles of
// a box.  The boxes are never written.  Does not read or change the handle's own output shape.
int do_extract_dot(vt_volume* v, int n, const double* m4x4s, const float* tmpl, const float* mask, int bd, int bh, int bw, double* out, int flags)
{
    if (!v || !m4x4s || !tmpl || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    int rc = check_batch_size(n);
    if (rc || (rc = check_dot_box(v, bd, bh, bw)) || (rc = select_device(v)) || (rc = check_finite_matrices(m4x4s, (size_t)n))) return rc;
    const size_t n_box = (size_t)bd * bh * bw;
    for (size_t i = 0; i < n_box; ++i) {
        if (!std::isfinite(tmpl[i])) return fail(VT_EINVAL, "template voxel %zu is not finite", i);
        if (mask && !std::isfinite(mask[i])) return fail(VT_EINVAL, "mask voxel %zu is not finite", i);
    }

    const int box[3] = {bd, bh, bw};
    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);
    const BoxTiles t = box_tiles(extract_pick_tile(is_cubic(v->interp), box, nullptr), bd, bh, bw);

    // the call's tables in one staging vector: one ExtractEntry per matrix, then the template and the mask (float32, padded to 16 bytes each)
    const size_t box_dbl = (n_box + 3) / 4 * 2;       // doubles that hold one box of float32
    const size_t tmpl_at = kEntryDoubles * (size_t)n, mask_at = tmpl_at + box_dbl;
    TableDims dims;
    if ((rc = build_box_table(v, m4x4s, n, box_dbl * (mask ? 2 : 1), t.cfg, force_direct, extract_dot_min_lds(), &dims))) return rc;
    std::memcpy(v->h_batch_m.data() + tmpl_at, tmpl, n_box * sizeof(float));
    if (mask) std::memcpy(v->h_batch_m.data() + mask_at, mask, n_box * sizeof(float));
    const AffineParams p = box_params(v, bd, bh, bw, t.nT);
    if (t.count > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "box too large");

    // matrices per launch: their partials stay within the cap (one matrix's partials at least), the grid within 2^31
    const int64_t part_one = t.count * 3 * (int64_t)sizeof(double);
    const int per_launch = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)n, v->tune.dot_part_cap / part_one, 0x7fffffffLL / t.count}));
    if ((rc = ensure_partials(v, (size_t)per_launch * (size_t)part_one)) || (rc = upload_tables(v))) return rc;
    const float* d_tmpl = reinterpret_cast<const float*>(v->d_batch_m + tmpl_at);
    const float* d_mask = mask ? reinterpret_cast<const float*>(v->d_batch_m + mask_at) : nullptr;
    ResultScope res(v, out, (size_t)n * 3 * sizeof(double), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open())) return rc;

    int last_cnt = 0;
    for (int first = 0; first < n; first += per_launch) {
        last_cnt = std::min(per_launch, n - first);
        VT_HIP(launch_extract_dot(t.cfg, v->interp, v->d_src, res.ptr<double>() + (size_t)first * 3, v->d_proj_part, v->d_zeros,
                                  device_entries(v) + first, d_tmpl, d_mask, last_cnt, p, dims.lds_bytes, v->stream));
    }
    record_launch(v, 14, t.T, dims.L, dims.lds_bytes, t.count * last_cnt);
    return res.finish();
}

// n x (2 + k) float64: do_extract_dot's two mask sums followed by one template sum per template of the stack (scoring n candidate poses
// against k references under one mask), in launches of kernel 15 (vt_kernels_extractdotmulti.hip), each followed by its small reduction
// over the tiles of a box.  Every column holds the bits do_extract_dot gives for that template alone; each box is staged and sampled
// once.  The boxes are never written.  Does not read or change the handle's own output shape.
int do_extract_dot_multi(vt_volume* v, int n, const double* m4x4s, int k, const float* tmpls, const float* mask, int bd, int bh, int bw,
                         double* out, int flags)
{
    if (!v || !m4x4s || !tmpls || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    int rc = check_batch_size(n);
    if (rc) return rc;
    if (k <= 0) return fail(VT_EINVAL, "template count %d", k);
    if ((rc = check_dot_box(v, bd, bh, bw))) return rc;

    const int box[3] = {bd, bh, bw};
    const BoxTiles t = box_tiles(extract_pick_tile(is_cubic(v->interp), box, nullptr), bd, bh, bw);
    const int64_t ncol = 2 + (int64_t)k;
    if (t.count > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "box too large");
    if (t.count * ncol > 0x7fffffffLL)
        return fail(VT_EUNSUPPORTED, "box tiles x (2 + k) = %lld exceeds 2^31 - 1", (long long)(t.count * ncol));

    if ((rc = select_device(v)) || (rc = check_finite_matrices(m4x4s, (size_t)n))) return rc;
    const size_t n_box = (size_t)bd * bh * bw;
    for (size_t j = 0; j < (size_t)k; ++j) {
        const float* tj = tmpls + j * n_box;
        for (size_t i = 0; i < n_box; ++i)
            if (!std::isfinite(tj[i])) return fail(VT_EINVAL, "template %zu voxel %zu is not finite", j, i);
    }
    if (mask)
        for (size_t i = 0; i < n_box; ++i)
            if (!std::isfinite(mask[i])) return fail(VT_EINVAL, "mask voxel %zu is not finite", i);

    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);

    // the call's tables in one staging vector: one ExtractEntry per matrix, then the k templates back to back and the mask (float32,
    // the stack and the mask padded to 16 bytes each)
    const size_t stack_dbl = ((size_t)k * n_box + 3) / 4 * 2;      // doubles that hold the stack of float32 templates
    const size_t box_dbl = (n_box + 3) / 4 * 2;                    // ... and one box
    const size_t tmpls_at = kEntryDoubles * (size_t)n, mask_at = tmpls_at + stack_dbl;
    TableDims dims;
    if ((rc = build_box_table(v, m4x4s, n, stack_dbl + (mask ? box_dbl : 0), t.cfg, force_direct, extract_dot_min_lds(), &dims))) return rc;
    std::memcpy(v->h_batch_m.data() + tmpls_at, tmpls, (size_t)k * n_box * sizeof(float));
    if (mask) std::memcpy(v->h_batch_m.data() + mask_at, mask, n_box * sizeof(float));
    const AffineParams p = box_params(v, bd, bh, bw, t.nT);

    // matrices per launch: their partials stay within the cap (one matrix's partials at least), the grid within 2^31
    const int64_t part_one = t.count * ncol * (int64_t)sizeof(double);
    const int per_launch = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)n, v->tune.dot_part_cap / part_one, 0x7fffffffLL / t.count}));
    if ((rc = ensure_partials(v, (size_t)per_launch * (size_t)part_one)) || (rc = upload_tables(v))) return rc;
    const float* d_tmpls = reinterpret_cast<const float*>(v->d_batch_m + tmpls_at);
    const float* d_mask = mask ? reinterpret_cast<const float*>(v->d_batch_m + mask_at) : nullptr;
    ResultScope res(v, out, (size_t)n * (size_t)ncol * sizeof(double), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open())) return rc;

    int last_cnt = 0;
    for (int first = 0; first < n; first += per_launch) {
        last_cnt = std::min(per_launch, n - first);
        VT_HIP(launch_extract_dot_multi(t.cfg, v->interp, v->d_src, res.ptr<double>() + (size_t)first * (size_t)ncol, v->d_proj_part, v->d_zeros,
                                        device_entries(v) + first, d_tmpls, d_mask, k, last_cnt, p, dims.lds_bytes, v->stream));
    }
    record_launch(v, 15, t.T, dims.L, dims.lds_bytes, t.count * last_cnt);
    return res.finish();
}

// g boxes: column j of the n x g weights applied to the n boxes do_extract would write, box j holding the bits do_extract_sum gives for
// that column alone (class averages, half-set maps, bootstrap replicas), in launches of kernel 16 (vt_kernels_extractsummulti.hip), each
// followed by its reduction when the matrices are split into segments.  Each (matrix, box tile) is staged and sampled once per chunk of
// columns.  The boxes are never written.  Does not read or change the handle's own output shape.
int do_extract_sum_multi(vt_volume* v, int n, const double* m4x4s, int g, const double* weights, int bd, int bh, int bw, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    int rc = check_batch_size(n);
    if (rc) return rc;
    if (g <= 0) return fail(VT_EINVAL, "column count %d", g);
    if (!weights) return fail(VT_EINVAL, "NULL weights");
    if ((rc = check_shape("box", bd, bh, bw)) || (rc = check_whole_volume(v, "box summation")) || (rc = select_device(v)) ||
        (rc = check_finite_matrices(m4x4s, (size_t)n)))
        return rc;
    for (size_t i = 0; i < (size_t)n * (size_t)g; ++i)
        if (!std::isfinite(weights[i])) return fail(VT_EINVAL, "weight (%zu, %zu) is not finite", i / (size_t)g, i % (size_t)g);

    const int box[3] = {bd, bh, bw};
    const size_t n_box = (size_t)bd * bh * bw;
    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);
    int cfg = 0, nseg = 1, per_seg = n;
    extract_sum_shape_plan(is_cubic(v->interp), box, n, &cfg, &nseg, &per_seg);      // do_extract_sum's, whatever g is: every column sees its segments
    const BoxTiles t = box_tiles(cfg, bd, bh, bw);
    const int GC = extract_sum_multi_chunk(cfg);
    if (t.count * nseg > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "box too large");

    // columns per launch: whole chunks, at least one; their partials stay within the cap, the grid within 2^31
    const int64_t chunks_all = ((int64_t)g + GC - 1) / GC;
    int64_t chunks_per = std::min<int64_t>(chunks_all, 0x7fffffffLL / (t.count * nseg));
    if (nseg > 1) {
        const int64_t part_chunk = (int64_t)GC * nseg * (int64_t)n_box * (int64_t)sizeof(double);
        chunks_per = std::min<int64_t>(chunks_per, v->tune.dot_part_cap / part_chunk);
    }
    chunks_per = std::max<int64_t>(1, chunks_per);
    const int cols_per = (int)std::min<int64_t>(g, chunks_per * GC);

    // the call's tables in one staging vector: one ExtractEntry per matrix, then the n x g weights, then eight doubles of zeros behind the
    // last row (a chunk is at most eight columns wide)
    const size_t n_wts = (size_t)n * (size_t)g;
    TableDims dims;
    if ((rc = build_box_table(v, m4x4s, n, n_wts + 8, cfg, force_direct, 16, &dims))) return rc;
    double* const w = v->h_batch_m.data() + kEntryDoubles * (size_t)n;
    std::memcpy(w, weights, n_wts * sizeof(double));
    std::fill(w + n_wts, w + n_wts + 8, 0.0);
    const AffineParams p = box_params(v, bd, bh, bw, t.nT);
    if (t.count * nseg * (((int64_t)cols_per + GC - 1) / GC) > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "box too large");

    if (nseg > 1 && (rc = ensure_partials(v, (size_t)cols_per * (size_t)nseg * n_box * sizeof(double)))) return rc;
    if ((rc = upload_tables(v))) return rc;
    ResultScope res(v, out, (size_t)g * n_box * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open())) return rc;

    int64_t last_grid = 0;
    for (int first = 0; first < g; first += cols_per) {
        const int cnt = std::min(cols_per, g - first);
        float* const d_boxes = res.ptr<float>() + (size_t)first * n_box;
        VT_HIP(launch_extract_sum_multi(cfg, v->interp, v->d_src, d_boxes, v->d_proj_part, v->d_zeros, device_entries(v),
                                        v->d_batch_m + kEntryDoubles * (size_t)n + first, n, per_seg, nseg, g, cnt, p, dims.lds_bytes, v->stream));
        if (nseg > 1) VT_HIP(launch_project_reduce(v->d_proj_part, d_boxes, nseg, (int64_t)n_box, cnt, v->stream));
        last_grid = t.count * nseg * ((cnt + GC - 1) / GC);
    }
    record_launch(v, 16, t.T, dims.L, dims.lds_bytes, last_grid);
    return res.finish();
}

// Output tiles whose base can pass place_tiled's tile test (any_valid) for entry e, as an axis-aligned range of tile indices per axis
// (t_lo[k] > t_hi[k]: none).  The test accepts a tile base y = A x0 + t iff vlo - kTileMargin - pos <= y < vhi + kTileMargin - neg on
// every row; the inverse image of that box under A is a parallelepiped whose bounding box (the 8 corners, taken term by term) is widened
// by 1 + 1e-6 max|bound| voxels -- far more than float64 rounding moves a bound once A is accepted below -- and cut to whole tiles.
// Every tile, whatever the matrix: a 3 x 3 part with a zero row, a non-finite determinant or |det A| < 1e-6 |row 0| |row 1| |row 2| (the
// rows span less than a millionth of the volume their lengths allow: the inverse would amplify rounding by more than the slack covers),
// or non-finite bounds.  Nothing is divided before A has passed that test.  Direct (untiled) entries use the same range: their per-voxel
// inside test implies the tile test up to rounding that the margins cover.
void place_tile_range(const ExtractEntry& e, const AffineParams& p, const int T[3], const int nT[3], int t_lo[3], int t_hi[3])
{
    for (int k = 0; k < 3; ++k) { t_lo[k] = 0; t_hi[k] = nT[k] - 1; }
    const double* m = e.m;
    const double a[3][3] = {{m[0], m[1], m[2]}, {m[4], m[5], m[6]}, {m[8], m[9], m[10]}};
    double norm[3];
    for (int r = 0; r < 3; ++r) norm[r] = std::sqrt(a[r][0] * a[r][0] + a[r][1] * a[r][1] + a[r][2] * a[r][2]);
    const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2], c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    const double det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02;
    const double span = norm[0] * norm[1] * norm[2];
    if (!std::isfinite(det) || !std::isfinite(span) || !(span > 0.0) || !(std::fabs(det) >= 1.0e-6 * span)) return;
    const double inv[3][3] = {
        {c00 / det, (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det, (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det},
        {c01 / det, (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det, (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det},
        {c02 / det, (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det, (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det}};
    double y_lo[3], y_hi[3];
    for (int r = 0; r < 3; ++r) {
        y_lo[r] = p.vlo[r] - kTileMargin - e.pos[r] - m[4 * r + 3];
        y_hi[r] = p.vhi[r] + kTileMargin - e.neg[r] - m[4 * r + 3];
    }
    int lo_i[3], hi_i[3];
    for (int k = 0; k < 3; ++k) {
        double lo = 0.0, hi = 0.0;
        for (int r = 0; r < 3; ++r) {
            const double u = inv[k][r] * y_lo[r], w = inv[k][r] * y_hi[r];
            lo += std::min(u, w); hi += std::max(u, w);
        }
        if (!std::isfinite(lo) || !std::isfinite(hi)) return;
        const double pad = 1.0 + 1.0e-6 * std::max(std::fabs(lo), std::fabs(hi));
        const double first = std::ceil((lo - pad) / T[k]), last = std::floor((hi + pad) / T[k]);
        lo_i[k] = (int)std::max(0.0, std::min(first, (double)nT[k]));
        hi_i[k] = (int)std::min((double)(nT[k] - 1), std::max(last, -1.0));
    }
    for (int k = 0; k < 3; ++k) { t_lo[k] = lo_i[k]; t_hi[k] = hi_i[k]; }
}

// One map of shape (od, oh, ow): n weighted copies of the resident map, each through its own pull matrix, summed in float64 in ascending
// order and rounded once -- do_extract_sum's expression with the output as "the box", but only where a copy can land: the entries are
// binned into per-tile lists here, and kernel 17 (vt_kernels_place.hip) runs one workgroup per tile with a non-empty list.  VT_ACCUMULATE
// starts the sums from `out` as found and leaves the other tiles alone; otherwise `out` is zeroed first.  Does not read or change the
// handle's own output shape.
int do_place(vt_volume* v, int n, const double* m4x4s, const double* weights, int od, int oh, int ow, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    int rc = check_batch_size(n);
    if (rc || (rc = check_shape("output", od, oh, ow)) || (rc = check_whole_volume(v, "placing copies")) || (rc = select_device(v)) ||
        (rc = check_finite_matrices(m4x4s, (size_t)n)) || (rc = check_finite_weights(weights, (size_t)n)))
        return rc;

    const int shape[3] = {od, oh, ow};
    const size_t n_out = (size_t)od * oh * ow;
    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);
    const bool accumulate = (flags & VT_ACCUMULATE) != 0;
    const bool dense = (flags & VT_PLACE_DENSE) != 0;
    // a function of (output shape, interpolation): do_extract_sum's tile
    const BoxTiles t = box_tiles(extract_pick_tile(is_cubic(v->interp), shape, nullptr), od, oh, ow);
    const int* const nT = t.nT;
    if (t.count > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "output too large (%lld tiles)", (long long)t.count);

    // the launch's tables: one ExtractEntry per matrix, then the n weights, then (below) the lists
    const size_t ints_at = (size_t)n * (kEntryDoubles + 1);
    TableDims dims;
    if ((rc = build_box_table(v, m4x4s, n, (size_t)n, t.cfg, force_direct, 16, &dims))) return rc;
    std::vector<double>& tab = v->h_batch_m;
    for (int i = 0; i < n; ++i) tab[kEntryDoubles * (size_t)n + (size_t)i] = weights ? weights[i] : 1.0;
    const AffineParams p = box_params(v, od, oh, ow, nT);

    // ---- binning: count, then fill, both in ascending entry order, so every list is ascending by construction; O(sum of candidate tiles) ----
    std::vector<int> range((size_t)n * 6);
    std::vector<int> cursor((size_t)t.count, 0);      // per tile: entries listed, then the write position of its list
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        int* lo = &range[6 * (size_t)i];
        int* hi = lo + 3;
        if (dense) for (int k = 0; k < 3; ++k) { lo[k] = 0; hi[k] = nT[k] - 1; }
        else place_tile_range(host_entries(v)[i], p, t.T, nT, lo, hi);
        if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) { lo[0] = 0; hi[0] = -1; continue; }
        total += (int64_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
        if (total > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "tile lists too long (more than 2^31 - 1 (tile, matrix) pairs)");
        for (int a = lo[0]; a <= hi[0]; ++a)
            for (int b = lo[1]; b <= hi[1]; ++b) {
                int* row = &cursor[((size_t)a * nT[1] + b) * nT[2]];
                for (int c = lo[2]; c <= hi[2]; ++c) ++row[c];
            }
    }
    int64_t n_tiles = 0;
    for (int64_t k = 0; k < t.count; ++k) n_tiles += cursor[(size_t)k] > 0;
    const size_t ints = n_tiles > 0 ? (size_t)(2 * n_tiles + 1 + total) : 0;      // tile ids, offsets, list entries
    tab.resize(ints_at + (ints + 1) / 2);
    int* const ids = reinterpret_cast<int*>(tab.data() + ints_at);
    int* const offs = ids + n_tiles;
    int* const idx = offs + n_tiles + 1;
    if (n_tiles > 0) {
        int64_t k = 0, at = 0;
        for (int64_t tile = 0; tile < t.count; ++tile) {
            const int cnt = cursor[(size_t)tile];
            if (cnt == 0) continue;
            ids[k] = (int)tile; offs[k] = (int)at; ++k;
            cursor[(size_t)tile] = (int)at;
            at += cnt;
        }
        offs[n_tiles] = (int)at;
        for (int i = 0; i < n; ++i) {
            const int* lo = &range[6 * (size_t)i];
            const int* hi = lo + 3;
            for (int a = lo[0]; a <= hi[0]; ++a)
                for (int b = lo[1]; b <= hi[1]; ++b) {
                    int* row = &cursor[((size_t)a * nT[1] + b) * nT[2]];
                    for (int c = lo[2]; c <= hi[2]; ++c) idx[row[c]++] = i;
                }
        }
    }

    record_launch(v, 17, t.T, dims.L, dims.lds_bytes, n_tiles);
    if (n_tiles == 0 && accumulate) return 0;          // nothing can land anywhere: `out` stays as found, nothing is launched

    ResultScope res(v, out, n_out * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open(accumulate))) return rc;
    if (!accumulate) VT_HIP(hipMemsetAsync(res.ptr<float>(), 0, n_out * sizeof(float), v->stream));
    if (n_tiles > 0) {                                // (a grid of 0 is an error)
        if ((rc = upload_tables(v))) return rc;
        const int* d_ids = reinterpret_cast<const int*>(v->d_batch_m + ints_at);
        VT_HIP(launch_place(t.cfg, v->interp, v->d_src, res.ptr<float>(), v->d_zeros, device_entries(v), v->d_batch_m + kEntryDoubles * (size_t)n,
                            d_ids, d_ids + n_tiles, d_ids + 2 * n_tiles + 1, (int)n_tiles, accumulate, p, dims.lds_bytes, v->stream));
    }
    return res.finish();
}

// One volume of shape (od, oh, ow) from the handle's planes taken as a stack of T images: n weighted 2-D samples per voxel, image
// planes[i] at rows 1 and 2 of matrix i, summed in float64 in ascending order and rounded once -- do_place without the lists: kernel 18
// (vt_kernels_backproject.hip) runs one workgroup per output tile over all n entries, so nothing is zeroed first.  The tile is do_place's,
// the tables are build_backproject_tables' for one box.  Does not read or change the handle's own output shape.
int do_backproject(vt_volume* v, int n, const double* m4x4s, const int32_t* planes, const double* weights, int od, int oh, int ow, float* out,
                   int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    int rc = check_batch_size(n);
    if (rc || (rc = check_shape("output", od, oh, ow)) || (rc = check_backproject_handle(v)) || (rc = select_device(v)) ||
        (rc = check_finite_matrices(m4x4s, (size_t)n)) || (rc = check_finite_weights(weights, (size_t)n)) ||
        (rc = check_planes(v, n, planes, "")))
        return rc;

    const int shape[3] = {od, oh, ow};
    const size_t n_out = (size_t)od * oh * ow;
    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);
    const bool accumulate = (flags & VT_ACCUMULATE) != 0;
    // a function of (output shape, interpolation): do_place's tile
    const BoxTiles t = box_tiles(extract_pick_tile(is_cubic(v->interp), shape, nullptr), od, oh, ow);
    if (t.count > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "output too large (%lld tiles)", (long long)t.count);

    TableDims dims;
    int buf_floats = 0;
    if ((rc = build_backproject_tables(v, m4x4s, 1, n, planes, weights, t.cfg, force_direct, &dims, &buf_floats))) return rc;
    const AffineParams p = box_params(v, od, oh, ow, t.nT);
    record_launch(v, 18, t.T, dims.L, dims.lds_bytes, t.count);

    ResultScope res(v, out, n_out * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open(accumulate)) || (rc = upload_tables(v))) return rc;
    VT_HIP(launch_backproject(t.cfg, v->interp, v->d_src, res.ptr<float>(), v->d_zeros, device_entries(v), v->d_batch_m + kEntryDoubles * (size_t)n,
                              n, buf_floats, accumulate, p, dims.lds_bytes, v->stream));
    return res.finish();
}

// nb boxes of one shape (bd, bh, bw) from the handle's stack, n entries per box: box b is what do_backproject writes for matrices
// m4x4s + 16 n b, the shared planes and weights + n b at that output shape, bit for bit -- the same tile, the same tables
// (build_backproject_tables) and kernel 18's text with a box index (kernel 19, vt_kernels_backprojectboxes.hip): one launch of nb x tiles
// workgroups instead of nb launches, syncs and uploads.  MT: float or double matrices.
template <typename MT>
int do_backproject_boxes(vt_volume* v, int nb, int n, const MT* m4x4s, const int32_t* planes, const double* weights, int bd, int bh,
                         int bw, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (nb <= 0) return fail(VT_EINVAL, "number of boxes %d", nb);
    int rc = check_batch_size(n);
    if (rc || (rc = check_shape("box", bd, bh, bw)) || (rc = check_backproject_handle(v))) return rc;
    // the bounds, before anything of the caller's arrays is read
    const int64_t total = (int64_t)nb * n;                // entries of the call
    if (total > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "%d boxes x %d entries: more than 2^31 - 1 (box, entry) pairs", nb, n);
    const int shape[3] = {bd, bh, bw};
    const size_t box_vox = (size_t)bd * bh * bw;          // < 2^62 by the checks above
    if (box_vox > (SIZE_MAX / sizeof(float)) / (size_t)nb) return fail(VT_EUNSUPPORTED, "output too large (%d boxes)", nb);
    // a function of (box shape, interpolation): do_backproject's tile
    const BoxTiles t = box_tiles(extract_pick_tile(is_cubic(v->interp), shape, nullptr), bd, bh, bw);
    if (t.count > 0x7fffffffLL || t.count * nb > 0x7fffffffLL)
        return fail(VT_EUNSUPPORTED, "grid too large (%d boxes x %lld tiles)", nb, (long long)t.count);
    if ((rc = select_device(v)) || (rc = check_finite_matrices(m4x4s, (size_t)total)) || (rc = check_finite_weights(weights, (size_t)total)) ||
        (rc = check_planes(v, n, planes, " per box")))
        return rc;

    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);
    const bool accumulate = (flags & VT_ACCUMULATE) != 0;

    TableDims dims;
    int buf_floats = 0;
    if ((rc = build_backproject_tables(v, m4x4s, nb, n, planes, weights, t.cfg, force_direct, &dims, &buf_floats))) return rc;
    const AffineParams p = box_params(v, bd, bh, bw, t.nT);
    record_launch(v, 19, t.T, dims.L, dims.lds_bytes, t.count * nb);

    ResultScope res(v, out, box_vox * (size_t)nb * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open(accumulate)) || (rc = upload_tables(v))) return rc;
    VT_HIP(launch_backproject_boxes(t.cfg, v->interp, v->d_src, res.ptr<float>(), v->d_zeros, device_entries(v),
                                    v->d_batch_m + kEntryDoubles * (size_t)total, nb, n, buf_floats, accumulate, p, dims.lds_bytes, v->stream));
    return res.finish();
}

// n images of shape (oh, ow) from the handle's stack, image i from image planes[i] under rows 1 and 2 of matrix i: what do_backproject
// writes for that single entry at an output of depth 1 (to rounding on the staged cubic routes, bit for bit with VT_FORCE_DIRECT), in one
// launch of kernel 21 (vt_kernels_stackaffine.hip), n x tiles workgroups.  The tile is a function of (image shape, interpolation);
// whether an entry stages follows from that entry, the image shape and kStackAffinePatchCap.  The tables are n entries, then n weights
// (nullptr: ones).  MT: float or double matrices.  Does not read or change the handle's own output shape.
template <typename MT>
int do_affine_stack(vt_volume* v, int n, const MT* m4x4s, const int32_t* planes, const double* weights, int oh, int ow, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    int rc = check_batch_size(n);
    if (rc || (rc = check_shape("output", 1, oh, ow)) || (rc = check_backproject_handle(v))) return rc;
    // the bounds, before anything of the caller's arrays is read
    const bool cubic = is_cubic(v->interp);
    const int cfg = stack_affine_pick_tile(cubic, oh, ow);
    int T[3] = {1, 0, 0};
    stack_affine_tile(cfg, &T[1], &T[2]);
    const int nT[3] = {1, (oh + T[1] - 1) / T[1], (ow + T[2] - 1) / T[2]};
    const int64_t tiles = (int64_t)nT[1] * nT[2];
    if (tiles * n > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "grid too large (%d images x %lld tiles)", n, (long long)tiles);
    const size_t image = (size_t)oh * ow;                  // < 2^31 by check_shape
    if (image > (SIZE_MAX / sizeof(float)) / (size_t)n) return fail(VT_EUNSUPPORTED, "output too large (%d images)", n);
    if ((rc = select_device(v)) || (rc = check_finite_matrices(m4x4s, (size_t)n)) || (rc = check_finite_weights(weights, (size_t)n)) ||
        (rc = check_planes(v, n, planes, "")))
        return rc;

    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);
    if ((rc = begin_tables(v, (size_t)n * (kEntryDoubles + 1)))) return rc;
    ExtractEntry* const e = host_entries(v);
    double* const w = v->h_batch_m.data() + kEntryDoubles * (size_t)n;
    int L[3] = {0, 0, 0};
    int64_t largest = 0;
    for (int i = 0; i < n; ++i) {
        const MT* a = m4x4s + 16 * (size_t)i;
        const double rows[8] = {(double)a[4], (double)a[5], (double)a[6], (double)a[7], (double)a[8], (double)a[9], (double)a[10], (double)a[11]};
        stack_affine_fill_entry(rows, planes ? planes[i] : i, cfg, cubic, oh, ow, force_direct, &e[i]);
        const int64_t patch = (int64_t)e[i].Ly * e[i].Lx;
        if (e[i].tiled && patch > largest) { largest = patch; L[0] = 1; L[1] = e[i].Ly; L[2] = e[i].Lx; }
        w[i] = weights ? weights[i] : 1.0;
    }
    const int lds_bytes = (int)(largest * 4);
    const AffineParams p = box_params(v, 1, oh, ow, nT);
    record_launch(v, 21, T, L, lds_bytes, tiles * n);

    ResultScope res(v, out, image * (size_t)n * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open()) || (rc = upload_tables(v))) return rc;
    VT_HIP(launch_stack_affine(cfg, v->interp, v->d_src, res.ptr<float>(), v->d_zeros, device_entries(v), v->d_batch_m + kEntryDoubles * (size_t)n,
                               n, p, lds_bytes, v->stream));
    return res.finish();
}

// The resident volume resampled through a displacement grid: out[v] = sample(src, M.v + u(v)), u the float64 trilinear interpolation of
// the (gd, gh, gw, 3) float32 grid whose nodes span the (od, oh, ow) output corner to corner (vt_kernels_warp.hip has the expression).
// m4x4 == nullptr: the identity.  One launch of kernel 20, one workgroup per output tile; the tile is do_place's, a function of (output
// shape, interpolation).  The table (WarpTable) and the grid behind it travel in the staging vector.  Does not read or change the handle's
// own output shape.
int do_warp(vt_volume* v, const double* m4x4, const float* grid, int gd, int gh, int gw, int od, int oh, int ow, float* out, int flags)
{
    if (!v || !grid || !out) return fail(VT_EINVAL, "NULL argument");
    if (refuse_in_plane(v)) return VT_EUNSUPPORTED;
    int rc = check_shape("output", od, oh, ow);
    if (rc || (rc = check_whole_volume(v, "warping"))) return rc;
    const int shape[3] = {od, oh, ow}, g[3] = {gd, gh, gw};
    for (int k = 0; k < 3; ++k)
        if (g[k] != 1 && (g[k] < 2 || g[k] > shape[k]))
            return fail(VT_EINVAL, "grid dims (%d,%d,%d): per axis 1 node, or 2 up to the output's %d x %d x %d", gd, gh, gw, od, oh, ow);
    // the bounds, before anything of the caller's arrays is read
    const int64_t node_floats = (int64_t)gd * gh * gw * 3;      // g_k <= o_k, o_d o_h < 2^31: no overflow
    if (node_floats > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "grid too large (%d x %d x %d nodes)", gd, gh, gw);
    const BoxTiles t = box_tiles(extract_pick_tile(is_cubic(v->interp), shape, nullptr), od, oh, ow);
    if (t.count > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "output too large (%lld tiles)", (long long)t.count);
    const size_t n_out = (size_t)od * oh * ow;                   // < 2^62 by check_shape
    static const double identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!m4x4) m4x4 = identity;
    if ((rc = select_device(v)) || (rc = check_finite_matrices(m4x4, 1))) return rc;
    for (int64_t i = 0; i < node_floats; ++i)
        if (!std::isfinite(grid[i])) return fail(VT_EINVAL, "grid node %lld component %d is not finite", (long long)(i / 3), (int)(i % 3));

    // the launch's table: WarpTable, then the grid
    constexpr size_t kTableDoubles = sizeof(WarpTable) / sizeof(double);
    if ((rc = begin_tables(v, kTableDoubles + ((size_t)node_floats + 1) / 2))) return rc;
    WarpTable* const wt = reinterpret_cast<WarpTable*>(v->h_batch_m.data());
    std::memcpy(v->h_batch_m.data() + kTableDoubles, grid, (size_t)node_floats * sizeof(float));
    double m[12];                                                // fold_matrix on a whole-volume handle: the matrix, plus the pad
    std::memcpy(m, m4x4, sizeof(m));
    const double pad = (double)v->edge_pad;
    m[3] += pad; m[7] += pad; m[11] += pad;
    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);
    int L[3], lds_bytes = 0;
    warp_plan(m, grid, g, shape, t.cfg, is_cubic(v->interp), force_direct, wt, L, &lds_bytes);
    if (lds_bytes > v->lds_limit) return fail(VT_EUNSUPPORTED, "the launch needs %d bytes of LDS, the device grants %d", lds_bytes, v->lds_limit);
    const AffineParams p = box_params(v, od, oh, ow, t.nT);
    record_launch(v, 20, t.T, L, lds_bytes, t.count);

    ResultScope res(v, out, n_out * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open()) || (rc = upload_tables(v))) return rc;
    VT_HIP(launch_warp(t.cfg, v->interp, v->d_src, res.ptr<float>(), v->d_zeros, reinterpret_cast<const WarpTable*>(v->d_batch_m),
                       reinterpret_cast<const float*>(v->d_batch_m + kTableDoubles), p, t.count, lds_bytes, v->stream));
    return res.finish();
}

// The grids of a warp_stack call (kinds 22, 26): checked, ranged (ranges: four floats per grid, warp_stack_grid_range's) and copied to dst
// in ONE pass, in pieces that stay in the cache between the three.
int warp_stack_take_grids(const float* grids, int n_grids, int gh, int gw, float* dst, float* ranges)
{
    constexpr size_t kPieceNodes = 32768;                   // 256 KiB
    const size_t nodes = (size_t)gh * gw;
    for (int k = 0; k < n_grids; ++k) {
        float* const r = &ranges[4 * (size_t)k];
        r[0] = r[2] = INFINITY; r[1] = r[3] = -INFINITY;
        for (size_t at = 0; at < nodes; at += kPieceNodes) {
            const size_t cnt = std::min(kPieceNodes, nodes - at), first = 2 * ((size_t)k * nodes + at);
            if (!warp_stack_grid_range(grids + first, cnt, r)) {
                size_t i = first;
                while (std::isfinite(grids[i])) ++i;
                return fail(VT_EINVAL, "grid node %zu component %d is not finite", i / 2, (int)(i % 2));
            }
            std::memcpy(dst + first, grids + first, 2 * cnt * sizeof(float));
        }
    }
    return 0;
}

// n images of shape (oh, ow) from the handle's stack, image i from image planes[i] at rows 1 and 2 of matrix i (nullptr: the identity)
// plus the float64 bilinear interpolation of grid i (n_grids == 1: of the one grid) of gh x gw x 2 float32, whose nodes span the output
// image corner to corner (vt_kernels_warpstack.hip has the expression): one launch of kernel 22, n x tiles workgroups, do_affine_stack's
// tile.  The tables travel in one upload: n entries, the weights (padded to an even count), the grid header, the grids.  MT: float or
// double matrices.  Does not read or change the handle's own output shape.
template <typename MT>
int do_warp_stack(vt_volume* v, int n, const MT* m4x4s, const float* grids, int n_grids, int gh, int gw, const int32_t* planes,
                  const double* weights, int oh, int ow, float* out, int flags)
{
    if (!v || !grids || !out) return fail(VT_EINVAL, "NULL argument");
    int rc = check_batch_size(n);
    if (rc || (rc = check_shape("output", 1, oh, ow)) || (rc = check_backproject_handle(v))) return rc;
    if (n_grids != 1 && n_grids != n) return fail(VT_EINVAL, "%d grids for %d entries: one shared grid, or one per entry", n_grids, n);
    const int g[2] = {gh, gw}, o[2] = {oh, ow};
    for (int k = 0; k < 2; ++k)
        if (g[k] != 1 && (g[k] < 2 || g[k] > o[k]))
            return fail(VT_EINVAL, "grid dims (%d,%d): per axis 1 node, or 2 up to the output's %d x %d", gh, gw, oh, ow);
    // the bounds, before anything of the caller's arrays is read
    const int64_t per_grid = (int64_t)gh * gw * 2;             // g_k <= o_k, o_h o_w < 2^31: no overflow
    if (per_grid > 0x7fffffffLL || per_grid * n_grids > 0x7fffffffLL)
        return fail(VT_EUNSUPPORTED, "grids too large (%d grids of %d x %d nodes)", n_grids, gh, gw);
    const int64_t grid_floats = per_grid * n_grids;
    const bool cubic = is_cubic(v->interp);
    const int cfg = stack_affine_pick_tile(cubic, oh, ow);
    int T[3] = {1, 0, 0};
    stack_affine_tile(cfg, &T[1], &T[2]);
    const int nT[3] = {1, (oh + T[1] - 1) / T[1], (ow + T[2] - 1) / T[2]};
    const int64_t tiles = (int64_t)nT[1] * nT[2];
    if (tiles * n > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "grid too large (%d images x %lld tiles)", n, (long long)tiles);
    const size_t image = (size_t)oh * ow;                      // < 2^31 by check_shape
    if (image > (SIZE_MAX / sizeof(float)) / (size_t)n) return fail(VT_EUNSUPPORTED, "output too large (%d images)", n);
    if ((rc = select_device(v)) || (m4x4s && (rc = check_finite_matrices(m4x4s, (size_t)n))) || (rc = check_finite_weights(weights, (size_t)n)) ||
        (rc = check_planes(v, n, planes, "")))
        return rc;

    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);
    constexpr size_t kHeaderDoubles = sizeof(WarpStackHeader) / sizeof(double);
    const size_t n_wts = ((size_t)n + 1) & ~(size_t)1;         // the header behind them stays 16-byte aligned
    const size_t hdr_at = (size_t)n * kEntryDoubles + n_wts, grids_at = hdr_at + kHeaderDoubles;
    if ((rc = begin_tables(v, grids_at + ((size_t)grid_floats + 1) / 2))) return rc;
    ExtractEntry* const e = host_entries(v);
    double* const w = v->h_batch_m.data() + kEntryDoubles * (size_t)n;
    WarpStackHeader* const hd = reinterpret_cast<WarpStackHeader*>(v->h_batch_m.data() + hdr_at);
    // the grids: checked, ranged and copied in ONE pass, in pieces that stay in the cache between the three -- with a dense field per
    // image this pass and the upload are the call
    std::vector<float> ranges((size_t)n_grids * 4);
    if ((rc = warp_stack_take_grids(grids, n_grids, gh, gw, reinterpret_cast<float*>(v->h_batch_m.data() + grids_at), ranges.data()))) return rc;
    for (int i = 0; i < n; ++i) {
        double rows[8] = {0, 1, 0, 0, 0, 0, 1, 0};
        if (m4x4s) {
            const MT* a = m4x4s + 16 * (size_t)i;
            for (int k = 0; k < 8; ++k) rows[k] = (double)a[4 + k];
        }
        warp_stack_fill_entry(rows, planes ? planes[i] : i, cfg, cubic, oh, ow, force_direct, &e[i]);
        w[i] = weights ? weights[i] : 1.0;
    }
    if (n_wts > (size_t)n) w[n] = 0.0;
    int L2[2], patch_bytes = 0;
    warp_stack_plan(e, n, ranges.data(), n_grids, g, cfg, cubic, oh, ow, hd, L2, &patch_bytes);
    const int L[3] = {patch_bytes ? 1 : 0, L2[0], L2[1]};
    const int lds_bytes = (kWarpScratchFloats + hd->node_floats) * 4 + patch_bytes;
    const AffineParams p = box_params(v, 1, oh, ow, nT);
    record_launch(v, 22, T, L, lds_bytes, tiles * n);

    ResultScope res(v, out, image * (size_t)n * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open()) || (rc = upload_tables(v))) return rc;
    VT_HIP(launch_warp_stack(cfg, v->interp, v->d_src, res.ptr<float>(), v->d_zeros, device_entries(v), v->d_batch_m + kEntryDoubles * (size_t)n,
                             reinterpret_cast<const WarpStackHeader*>(v->d_batch_m + hdr_at),
                             reinterpret_cast<const float*>(v->d_batch_m + grids_at), n, p, lds_bytes, v->stream));
    return res.finish();
}

// g images of shape (oh, ow): column c of the n x g weights (nullptr: one column of ones) over the n images do_warp_stack would write
// unweighted, summed in float64 in ascending order and rounded once, the images never written (vt_kernels_warpstacksum.hip has the
// expression): one launch of kernel 26, column chunks x tiles workgroups.  Checks in do_warp_stack's order; entries, grid pass, node block
// and patch allocation are its own (warp_stack_fill_entry, warp_stack_take_grids, warp_stack_plan).  The tables travel in one upload:
// n entries, the n x g weights (padded to an even count), the grid header, the grids.  MT: float or double matrices.  Does not read or
// change the handle's own output shape.
template <typename MT>
int do_warp_stack_sum(vt_volume* v, int n, const MT* m4x4s, const float* grids, int n_grids, int gh, int gw, const int32_t* planes, int g,
                      const double* weights, int oh, int ow, float* out, int flags)
{
    if (!v || !grids || !out) return fail(VT_EINVAL, "NULL argument");
    int rc = check_batch_size(n);
    if (rc || (rc = check_shape("output", 1, oh, ow)) || (rc = check_backproject_handle(v))) return rc;
    if (g <= 0) return fail(VT_EINVAL, "column count %d", g);
    if (!weights && g != 1) return fail(VT_EINVAL, "NULL weights with %d columns: without weights there is one column", g);
    if (n_grids != 1 && n_grids != n) return fail(VT_EINVAL, "%d grids for %d entries: one shared grid, or one per entry", n_grids, n);
    const int gd[2] = {gh, gw}, o[2] = {oh, ow};
    for (int k = 0; k < 2; ++k)
        if (gd[k] != 1 && (gd[k] < 2 || gd[k] > o[k]))
            return fail(VT_EINVAL, "grid dims (%d,%d): per axis 1 node, or 2 up to the output's %d x %d", gh, gw, oh, ow);
    // the bounds, before anything of the caller's arrays is read
    const int64_t per_grid = (int64_t)gh * gw * 2;
    if (per_grid > 0x7fffffffLL || per_grid * n_grids > 0x7fffffffLL)
        return fail(VT_EUNSUPPORTED, "grids too large (%d grids of %d x %d nodes)", n_grids, gh, gw);
    const int64_t grid_floats = per_grid * n_grids;
    const bool cubic = is_cubic(v->interp);
    const int cfg = stack_affine_pick_tile(cubic, oh, ow);
    int T[3] = {1, 0, 0};
    stack_affine_tile(cfg, &T[1], &T[2]);
    const int nT[3] = {1, (oh + T[1] - 1) / T[1], (ow + T[2] - 1) / T[2]};
    const int64_t tiles = (int64_t)nT[1] * nT[2];
    const int64_t chunks = ((int64_t)g + kWarpStackSumChunk - 1) / kWarpStackSumChunk;
    if (tiles * chunks > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "grid too large (%d columns x %lld tiles)", g, (long long)tiles);
    const size_t image = (size_t)oh * ow;                      // < 2^31 by check_shape
    if (image > (SIZE_MAX / sizeof(float)) / (size_t)g) return fail(VT_EUNSUPPORTED, "output too large (%d images)", g);
    if ((size_t)g > (SIZE_MAX / sizeof(double) / 4) / (size_t)n) return fail(VT_EUNSUPPORTED, "weights too large (%d x %d)", n, g);
    if ((rc = select_device(v)) || (m4x4s && (rc = check_finite_matrices(m4x4s, (size_t)n))) ||
        (rc = check_finite_weights(weights, (size_t)n * (size_t)g)) || (rc = check_planes(v, n, planes, "")))
        return rc;

    const bool force_direct = (flags & VT_FORCE_DIRECT) && !(flags & VT_FORCE_TILED);
    const bool accumulate = (flags & VT_ACCUMULATE) != 0;
    constexpr size_t kHeaderDoubles = sizeof(WarpStackHeader) / sizeof(double);
    const size_t n_w = (size_t)n * (size_t)g, n_wts = (n_w + 1) & ~(size_t)1;      // the header behind them stays 16-byte aligned
    const size_t hdr_at = (size_t)n * kEntryDoubles + n_wts, grids_at = hdr_at + kHeaderDoubles;
    if ((rc = begin_tables(v, grids_at + ((size_t)grid_floats + 1) / 2))) return rc;
    ExtractEntry* const e = host_entries(v);
    double* const w = v->h_batch_m.data() + kEntryDoubles * (size_t)n;
    WarpStackHeader* const hd = reinterpret_cast<WarpStackHeader*>(v->h_batch_m.data() + hdr_at);
    std::vector<float> ranges((size_t)n_grids * 4);
    if ((rc = warp_stack_take_grids(grids, n_grids, gh, gw, reinterpret_cast<float*>(v->h_batch_m.data() + grids_at), ranges.data()))) return rc;
    for (int i = 0; i < n; ++i) {
        double rows[8] = {0, 1, 0, 0, 0, 0, 1, 0};
        if (m4x4s) {
            const MT* a = m4x4s + 16 * (size_t)i;
            for (int k = 0; k < 8; ++k) rows[k] = (double)a[4 + k];
        }
        warp_stack_fill_entry(rows, planes ? planes[i] : i, cfg, cubic, oh, ow, force_direct, &e[i]);
    }
    if (weights) std::memcpy(w, weights, n_w * sizeof(double));
    else std::fill(w, w + n_w, 1.0);
    if (n_wts > n_w) w[n_w] = 0.0;
    int L2[2], patch_bytes = 0;
    warp_stack_plan(e, n, ranges.data(), n_grids, gd, cfg, cubic, oh, ow, hd, L2, &patch_bytes);
    const int L[3] = {patch_bytes ? 2 : 0, L2[0], L2[1]};
    const int lds_bytes = warp_stack_sum_lds_bytes(*hd, patch_bytes);
    const AffineParams p = box_params(v, 1, oh, ow, nT);
    record_launch(v, 26, T, L, lds_bytes, tiles * chunks);

    ResultScope res(v, out, image * (size_t)g * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open(accumulate)) || (rc = upload_tables(v))) return rc;
    VT_HIP(launch_warp_stack_sum(cfg, v->interp, v->d_src, res.ptr<float>(), v->d_zeros, device_entries(v),
                                 v->d_batch_m + kEntryDoubles * (size_t)n, reinterpret_cast<const WarpStackHeader*>(v->d_batch_m + hdr_at),
                                 reinterpret_cast<const float*>(v->d_batch_m + grids_at), n, g, patch_bytes, accumulate, p, lds_bytes,
                                 v->stream));
    return res.finish();
}

// n images of the stack's own shape, image i = image planes[i] convolved along `axis` (1 or 2) with tap row i (row 0 when n_taps == 1),
// times weight i: numpy.convolve(line, taps, 'same') with zero (pad 0) or edge (pad 1) samples outside, summed in float64 over the
// non-zero taps in ascending order, rounded once (vt_kernels_filterstack.hip has the expression).  One launch of kernel 23, n x strips x
// segments workgroups.  The tables are n FilterEntry, every tap row compacted to the FilterTap pairs of its non-zero taps, and the rows
// themselves, each followed by kFilterChunk zeros.  The handle must hold samples: filt_* handles hold coefficients.  Does not read or
// change the handle's own output shape.
int do_filter_stack(vt_volume* v, int n, const int32_t* planes, const double* taps, int n_taps, int k, int axis, int pad,
                    const double* weights, float* out, int flags)
{
    if (!v || !taps || !out) return fail(VT_EINVAL, "NULL argument");
    int rc = check_batch_size(n);
    if (rc || (rc = check_whole_volume(v, "filter_stack"))) return rc;
    if (v->edge_pad) return fail(VT_EUNSUPPORTED, "filter_stack is not available on VT_EDGE_SCIPY handles");
    if (is_filtered(v->interp))
        return fail(VT_EUNSUPPORTED, "the handle holds prefilter coefficients, not samples: filter on a linear handle and build the filt_* "
                                     "handle from the result");
    if (axis != 1 && axis != 2) return fail(VT_EINVAL, "axis %d (1 or 2)", axis);
    if (pad != 0 && pad != 1) return fail(VT_EINVAL, "pad %d (0 zero, 1 edge)", pad);
    if (n_taps != 1 && n_taps != n) return fail(VT_EINVAL, "%d tap rows for %d images (1 or n)", n_taps, n);
    const int L = axis == 2 ? v->W : v->H, lines = axis == 2 ? v->H : v->W;
    if (k < 1 || !(k & 1) || (int64_t)k > 2 * (int64_t)L - 1)
        return fail(VT_EINVAL, "%d taps: an odd count inside [1, %lld] for an extent of %d", k, 2 * (long long)L - 1, L);
    // the bounds, before anything of the caller's arrays is read
    const int64_t wgs = filter_stack_strips(lines) * filter_stack_segments(L);
    if (wgs * n > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "grid too large (%d images x %lld workgroups)", n, (long long)wgs);
    const size_t image = (size_t)v->H * v->W;
    if (image > (SIZE_MAX / sizeof(float)) / (size_t)n) return fail(VT_EUNSUPPORTED, "output too large (%d images)", n);
    if (L > kFilterStackMaxExtent) return fail(VT_EUNSUPPORTED, "an extent of %d along axis %d", L, axis);
    if ((int64_t)n_taps * k > kFilterStackMaxTaps)
        return fail(VT_EUNSUPPORTED, "%d rows of %d taps: more than %lld taps in one call", n_taps, k, (long long)kFilterStackMaxTaps);
    if ((rc = select_device(v))) return rc;
    const size_t all = (size_t)n_taps * (size_t)k;
    size_t nnz_all = 0;
    for (size_t i = 0; i < all; ++i) {
        if (!std::isfinite(taps[i])) return fail(VT_EINVAL, "tap %zu of row %zu is not finite", i % (size_t)k, i / (size_t)k);
        nnz_all += taps[i] != 0.0;
    }
    if ((rc = check_finite_weights(weights, (size_t)n)) || (rc = check_planes(v, n, planes, ""))) return rc;

    constexpr size_t kFE = sizeof(FilterEntry) / sizeof(double);
    const size_t taps_at = kFE * (size_t)n, rows_at = taps_at + 2 * nnz_all, row_len = (size_t)k + kFilterChunk;
    if ((rc = begin_tables(v, rows_at + (size_t)n_taps * row_len))) return rc;
    FilterEntry* const e = reinterpret_cast<FilterEntry*>(v->h_batch_m.data());
    FilterTap* const tp = reinterpret_cast<FilterTap*>(v->h_batch_m.data() + taps_at);
    double* const rows = v->h_batch_m.data() + rows_at;
    size_t at = 0;
    for (int row = 0; row < n_taps; ++row) {
        const size_t first = at;
        const double* t = taps + (size_t)row * (size_t)k;
        double* const dense = rows + (size_t)row * row_len;
        std::memcpy(dense, t, (size_t)k * sizeof(double));
        std::fill(dense + k, dense + row_len, 0.0);
        for (int j = 0; j < k; ++j)
            if (t[j] != 0.0) { tp[at].t = t[j]; tp[at].j = j; tp[at].pad_ = 0; ++at; }
        for (int i = row; i < (n_taps == 1 ? n : row + 1); ++i) {
            e[i].weight = weights ? weights[i] : 1.0;
            e[i].first = (int64_t)first;
            e[i].dense = (int64_t)((size_t)row * row_len);
            e[i].plane = planes ? planes[i] : i;
            e[i].nnz = (int32_t)(at - first);
        }
    }
    const int T[3] = {1, axis == 2 ? kFilterStrip : kFilterSeg, axis == 2 ? kFilterSeg : kFilterStrip};
    const int Lds[3] = {1, kFilterSeg + kFilterChunk - 1, kFilterStrip + 1};
    record_launch(v, 23, T, Lds, kFilterLdsBytes, wgs * n);

    ResultScope res(v, out, image * (size_t)n * sizeof(float), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open()) || (rc = upload_tables(v))) return rc;
    VT_HIP(launch_filter_stack(v->d_src, res.ptr<float>(), reinterpret_cast<const FilterEntry*>(v->d_batch_m),
                               reinterpret_cast<const FilterTap*>(v->d_batch_m + taps_at), v->d_batch_m + rows_at, n, v->H, v->W, v->P, axis, pad,
                               k, v->stream));
    return res.finish();
}

// n x gh x gw x (2 rh + 1) x (2 rw + 1) float64: for entry i, patch (a, b) of the grid and shift (u, v), the sum over the patch of
// reference i times image planes[i] displaced by (u - rh, v - rw), zeros outside the image (vt_kernels_correlatestack.hip has the
// expression and the order of additions).  The reference of entry i is host image i of `refs` (image 0 when n_refs == 1) or, with refs
// == NULL, the resident image ref_planes[i].  Launches of kernel 24 over runs of (entry, patch) units whose partials stay within the
// cap, each followed by its reduction when a patch has several pieces.  Does not read or change the handle's own output shape.
int do_correlate_stack(vt_volume* v, int n, const int32_t* planes, const float* refs, int n_refs, const int32_t* ref_planes, int gh, int gw,
                       int rh, int rw, double* out, int flags)
{
    if (!v || !out) return fail(VT_EINVAL, "NULL argument");
    int rc = check_batch_size(n);
    if (rc || (rc = check_whole_volume(v, "correlate_stack"))) return rc;
    if (v->edge_pad) return fail(VT_EUNSUPPORTED, "correlate_stack is not available on VT_EDGE_SCIPY handles");
    if (is_filtered(v->interp))
        return fail(VT_EUNSUPPORTED, "the handle holds prefilter coefficients, not samples: correlate on a linear handle");
    if (n_refs != 0 && n_refs != 1 && n_refs != n) return fail(VT_EINVAL, "%d references for %d entries (1 or n)", n_refs, n);
    if ((refs != nullptr) == (ref_planes != nullptr)) return fail(VT_EINVAL, "exactly one of refs and ref_planes must be given");
    if (refs && n_refs == 0) return fail(VT_EINVAL, "0 host references");
    if (gh < 1 || gh > v->H || gw < 1 || gw > v->W) return fail(VT_EINVAL, "patch grid (%d,%d) for images of (%d,%d)", gh, gw, v->H, v->W);
    if (rh < 0 || rh > v->H - 1 || rw < 0 || rw > v->W - 1)
        return fail(VT_EINVAL, "shift window (%d,%d) for images of (%d,%d): at most (%d,%d)", rh, rw, v->H, v->W, v->H - 1, v->W - 1);
    // the bounds, before anything of the caller's arrays is read
    if (rh >= (1 << 30) || rw >= (1 << 30)) return fail(VT_EUNSUPPORTED, "output too large (a window of (%d,%d))", rh, rw);
    const CorrPlan cp = correlate_stack_plan(v->H, v->W, gh, gw, rh, rw);
    const int64_t nunv = (int64_t)cp.nu * cp.nv;                       // < 2^62
    const int64_t per = (int64_t)gh * gw;                              // patches per entry
    if (nunv > 0x7fffffffLL || per > 0x7fffffffLL || per * nunv > 0x7fffffffLL || per * nunv * n > 0x7fffffffLL)
        return fail(VT_EUNSUPPORTED, "output too large (%d entries x %lld patches x %lld shifts)", n, (long long)per, (long long)nunv);
    if (cp.unit_wgs > 0x7fffffffLL || cp.unit_part > 0x7fffffffLL)
        return fail(VT_EUNSUPPORTED, "%lld workgroups and %lld partial sums per patch", (long long)cp.unit_wgs, (long long)cp.unit_part);
    const size_t image = (size_t)v->H * v->W;
    if (refs && image * (size_t)n_refs > ((size_t)1 << 30)) return fail(VT_EUNSUPPORTED, "%d host references: more than 2^30 pixels", n_refs);
    if ((rc = select_device(v)) || (rc = check_planes(v, n, planes, ""))) return rc;
    if (ref_planes) {
        for (int i = 0; i < n; ++i)
            if (ref_planes[i] < 0 || ref_planes[i] >= v->D)
                return fail(VT_EINVAL, "reference plane index %d of entry %d outside [0, %d)", ref_planes[i], i, v->D);
    } else {
        for (size_t i = 0; i < image * (size_t)n_refs; ++i)
            if (!std::isfinite(refs[i])) return fail(VT_EINVAL, "pixel %zu of reference %zu is not finite", i % image, i / image);
    }

    // the call's tables in one staging vector: one CorrEntry per entry, then the host references as they came
    const size_t refs_at = (size_t)n, ref_dbl = refs ? (image * (size_t)n_refs + 1) / 2 : 0;
    if ((rc = begin_tables(v, refs_at + ref_dbl))) return rc;
    CorrEntry* const e = reinterpret_cast<CorrEntry*>(v->h_batch_m.data());
    for (int i = 0; i < n; ++i) {
        e[i].plane = planes ? planes[i] : i;
        e[i].ref = ref_planes ? ref_planes[i] : (n_refs == 1 ? 0 : i);
    }
    if (refs) std::memcpy(v->h_batch_m.data() + refs_at, refs, image * (size_t)n_refs * sizeof(float));

    // units per launch: their partials stay within the cap (one unit's partials at least), the grid within 2^31
    const int64_t units = per * n;
    int64_t per_launch = std::min<int64_t>(units, 0x7fffffffLL / cp.unit_wgs);
    if (cp.unit_part > 0)
        per_launch = std::min<int64_t>(per_launch, std::max<int64_t>(1, v->tune.dot_part_cap / (cp.unit_part * (int64_t)sizeof(double))));
    if (cp.unit_part > 0 && (rc = ensure_partials(v, (size_t)per_launch * (size_t)cp.unit_part * sizeof(double)))) return rc;
    if ((rc = upload_tables(v))) return rc;
    ResultScope res(v, out, (size_t)(units * nunv) * sizeof(double), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open())) return rc;

    const float* d_refs = refs ? reinterpret_cast<const float*>(v->d_batch_m + refs_at) : v->d_src;
    const int64_t src_plane = (int64_t)v->H * v->P, ref_plane = refs ? (int64_t)image : src_plane;
    int64_t last_cnt = 0;
    for (int64_t q0 = 0; q0 < units; q0 += per_launch) {
        last_cnt = std::min(per_launch, units - q0);
        VT_HIP(launch_correlate_stack(v->d_src, src_plane, v->P, d_refs, ref_plane, refs ? v->W : v->P,
                                      reinterpret_cast<const CorrEntry*>(v->d_batch_m), res.ptr<double>(), v->d_proj_part, q0, (int)last_cnt, cp,
                                      v->stream));
    }
    const int T[3] = {1, kCorrPiece, kCorrPiece};
    const int Lds[3] = {1, cp.lds_rows, cp.pitch};
    record_launch(v, 24, T, Lds, cp.lds_bytes, cp.unit_wgs * last_cnt);
    return res.finish();
}

// n x gh x gw x (2 rh + 1) x (2 rw + 1) x 2 float64: for entry i, patch (a, b) of the grid and shift (u, v), the sum and the sum of
// squares of image planes[i] under the patch displaced by (u - rh, v - rw), zeros outside the image (vt_kernels_momentsstack.hip has
// the expression and the order of additions).  Launches of kernel 25 over runs of entries whose row sums stay within the cap, each
// followed by the launch that adds the rows.  Does not read or change the handle's own output shape.
int do_moments_stack(vt_volume* v, int n, const int32_t* planes, int gh, int gw, int rh, int rw, double* out, int flags)
{
    if (!v || !out) return fail(VT_EINVAL, "NULL argument");
    int rc = check_batch_size(n);
    if (rc || (rc = check_whole_volume(v, "moments_stack"))) return rc;
    if (v->edge_pad) return fail(VT_EUNSUPPORTED, "moments_stack is not available on VT_EDGE_SCIPY handles");
    if (is_filtered(v->interp))
        return fail(VT_EUNSUPPORTED, "the handle holds prefilter coefficients, not samples: take moments on a linear handle");
    if (gh < 1 || gh > v->H || gw < 1 || gw > v->W) return fail(VT_EINVAL, "patch grid (%d,%d) for images of (%d,%d)", gh, gw, v->H, v->W);
    if (rh < 0 || rh > v->H - 1 || rw < 0 || rw > v->W - 1)
        return fail(VT_EINVAL, "shift window (%d,%d) for images of (%d,%d): at most (%d,%d)", rh, rw, v->H, v->W, v->H - 1, v->W - 1);
    // the bounds, before anything of the caller's arrays is read
    if (rh >= (1 << 29) || rw >= (1 << 29)) return fail(VT_EUNSUPPORTED, "output too large (a window of (%d,%d))", rh, rw);
    const MomPlan mp = moments_stack_plan(v->H, v->W, gh, gw, rh, rw);
    const int64_t nunv2 = (int64_t)mp.nu * mp.nv * 2;                  // < 2^62
    const int64_t per = (int64_t)gh * gw;                              // patches per entry
    if (nunv2 > 0x7fffffffLL || per > 0x7fffffffLL || per * nunv2 > 0x7fffffffLL || per * nunv2 * n > 0x7fffffffLL)
        return fail(VT_EUNSUPPORTED, "output too large (%d entries x %lld patches x %lld shifts x 2)", n, (long long)per,
                    (long long)(nunv2 / 2));
    if (mp.unit_wgs > 0x7fffffffLL || mp.unit_part > 0x7fffffffLL)
        return fail(VT_EUNSUPPORTED, "%lld workgroups and %lld row sums per entry", (long long)mp.unit_wgs, (long long)mp.unit_part);
    if ((rc = select_device(v)) || (rc = check_planes(v, n, planes, ""))) return rc;

    // the call's table: one MomEntry per entry
    if ((rc = begin_tables(v, (size_t)n))) return rc;
    MomEntry* const e = reinterpret_cast<MomEntry*>(v->h_batch_m.data());
    for (int i = 0; i < n; ++i) {
        e[i].plane = planes ? planes[i] : i;
        e[i].pad = 0;
    }
    // entries per launch: their row sums stay within the cap (one entry's at least), the grid within 2^31
    int64_t per_launch = std::min<int64_t>(n, 0x7fffffffLL / mp.unit_wgs);
    per_launch = std::min<int64_t>(per_launch, std::max<int64_t>(1, v->tune.dot_part_cap / (mp.unit_part * (int64_t)sizeof(double))));
    if ((rc = ensure_partials(v, (size_t)per_launch * (size_t)mp.unit_part * sizeof(double))) || (rc = upload_tables(v))) return rc;
    ResultScope res(v, out, (size_t)(per * nunv2 * n) * sizeof(double), !(flags & VT_OUT_DEVICE));
    if ((rc = res.open())) return rc;

    const int64_t src_plane = (int64_t)v->H * v->P;
    int64_t last_cnt = 0;
    for (int64_t e0 = 0; e0 < n; e0 += per_launch) {
        last_cnt = std::min<int64_t>(per_launch, n - e0);
        VT_HIP(launch_moments_stack(v->d_src, src_plane, v->P, reinterpret_cast<const MomEntry*>(v->d_batch_m), res.ptr<double>(),
                                    v->d_proj_part, e0, (int)last_cnt, mp, v->stream));
    }
    const int T[3] = {1, mp.rows_wg, kMomChunk};
    const int Lds[3] = {1, mp.rows_wg, mp.pitch};
    record_launch(v, 25, T, Lds, mp.lds_bytes, mp.unit_wgs * last_cnt);
    return res.finish();
}

// a float32 batch of n matrices in float64
std::vector<double> widened(const float* m4x4s, int n)
{
    std::vector<double> m((size_t)n * 16);
    for (size_t i = 0; i < m.size(); ++i) m[i] = (double)m4x4s[i];
    return m;
}

}  // namespace

extern "C" {

const char* vt_last_error(void) { return g_err; }
const char* vt_version(void) { return "voltools_amd 0.1.0 (gfx950)"; }

int vt_device_count(int* count)
{
    if (!count) return fail(VT_EINVAL, "NULL count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = (e == hipSuccess && n > 0) ? n : 0;     // "no device" is an answer, not an error
    return 0;
}

int vt_device_name(int dev, char* buf, int buflen)
{
    if (!buf || buflen <= 0) return fail(VT_EINVAL, "bad buffer");
    int rc = use_device(dev);
    if (rc) return rc;
    hipDeviceProp_t prop;
    VT_HIP(hipGetDeviceProperties(&prop, dev));
    snprintf(buf, (size_t)buflen, "%s (%s)", prop.name, prop.gcnArchName);
    return 0;
}

int vt_device_props(int dev, int* cu_count, int* lds_bytes_per_block, uint64_t* hbm_bytes)
{
    int rc = use_device(dev);
    if (rc) return rc;
    hipDeviceProp_t prop;
    VT_HIP(hipGetDeviceProperties(&prop, dev));
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (lds_bytes_per_block) *lds_bytes_per_block = (int)prop.sharedMemPerBlock;
    if (hbm_bytes) *hbm_bytes = (uint64_t)prop.totalGlobalMem;
    return 0;
}

int vt_device_synchronize(int dev)
{
    int rc = use_device(dev);
    if (rc) return rc;
    VT_HIP(hipDeviceSynchronize());
    return 0;
}

int vt_malloc(int dev, size_t bytes, void** dptr)
{
    if (!dptr || bytes == 0) return fail(VT_EINVAL, "bad arguments");
    int rc = use_device(dev);
    if (rc) return rc;
    VT_HIP(hipMalloc(dptr, bytes));
    return 0;
}

int vt_free(int dev, void* dptr)
{
    if (!dptr) return 0;
    int rc = use_device(dev);
    if (rc) return rc;
    VT_HIP(hipFree(dptr));
    return 0;
}

int vt_memset_zero(int dev, void* dptr, size_t bytes)
{
    if (!dptr) return fail(VT_EINVAL, "NULL pointer");
    int rc = use_device(dev);
    if (rc) return rc;
    VT_HIP(hipMemset(dptr, 0, bytes));
    return 0;
}

int vt_memcpy_h2d(int dev, void* dptr, const void* hptr, size_t bytes)
{
    if (!dptr || !hptr) return fail(VT_EINVAL, "NULL pointer");
    int rc = use_device(dev);
    if (rc) return rc;
    {
        PinnedScope pin(hptr, bytes);
        VT_HIP(pin.copy(dptr, hptr, bytes, hipMemcpyHostToDevice, nullptr));
        VT_HIP(hipStreamSynchronize(nullptr));
    }
    return 0;
}

int vt_memcpy_d2h(int dev, void* hptr, const void* dptr, size_t bytes)
{
    if (!dptr || !hptr) return fail(VT_EINVAL, "NULL pointer");
    int rc = use_device(dev);
    if (rc) return rc;
    {
        PinnedScope pin(hptr, bytes);
        VT_HIP(pin.copy(hptr, dptr, bytes, hipMemcpyDeviceToHost, nullptr));
        VT_HIP(hipStreamSynchronize(nullptr));
    }
    return 0;
}

int vt_memcpy_d2d(int dev, void* dst, const void* src, size_t bytes)
{
    if (!dst || !src) return fail(VT_EINVAL, "NULL pointer");
    int rc = use_device(dev);
    if (rc) return rc;
    VT_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
    return 0;
}

int vt_host_register(int dev, void* ptr, size_t bytes)
{
    if (!ptr || !bytes) return fail(VT_EINVAL, "NULL pointer or empty range");
    int rc = use_device(dev);
    if (rc) return rc;
    VT_HIP(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    PinnedScope::say("[vt pin] pool buffer [%p, %p) registered\n", ptr, (void*)((char*)ptr + bytes));
    return 0;
}

int vt_device_trim(int dev)
{
    if (dev < 0 || dev >= 64) return fail(VT_ENODEV, "device index %d", dev);
    int rc = use_device(dev);
    if (rc) return rc;
    std::vector<std::pair<size_t, void*>> drop, drop_small;
    {
        std::lock_guard<std::mutex> lk(g_cache[dev].mu);
        drop.swap(g_cache[dev].big);
        g_cache[dev].big_bytes = 0;
        drop_small.swap(g_cache[dev].bufs);
        g_cache[dev].buf_bytes = 0;
    }
    for (auto& d : drop) (void)hipFree(d.second);
    for (auto& d : drop_small) (void)hipFree(d.second);
    return 0;
}

int vt_host_unregister(int dev, void* ptr)
{
    if (!ptr) return 0;
    int rc = use_device(dev);
    if (rc) return rc;
    VT_HIP(hipHostUnregister(ptr));
    PinnedScope::say("[vt pin] pool buffer %p released\n", ptr);
    return 0;
}

int vt_volume_create(int dev, int depth, int height, int width, int interp, const float* data,
                     int create_flags, vt_volume_t** out)
{
    return create_common(dev, depth, height, width, interp, data, create_flags & (VT_SRC_DEVICE | VT_EDGE_SCIPY | VT_STACK),
                         0, depth, 0, depth, out);
}

int vt_volume_create_slab(int dev, int local_depth, int height, int width, int interp, const float* data,
                          int create_flags, int64_t plane0, int64_t global_depth, int64_t out_plane0,
                          int out_depth, vt_volume_t** out)
{
    return create_common(dev, local_depth, height, width, interp, data, create_flags,
                         plane0, global_depth, out_plane0, out_depth, out);
}

int vt_volume_upload_planes(vt_volume_t* v, int first_plane, int nplanes, const float* data, int flags)
{
    if (!v || !data) return fail(VT_EINVAL, "NULL argument");
    if (!v->deferred) return fail(VT_EINVAL, "planes can only be uploaded into a handle created with VT_SRC_DEFERRED, before vt_volume_finalize");
    if (first_plane < 0 || nplanes <= 0 || (int64_t)first_plane + nplanes > v->D)
        return fail(VT_EINVAL, "planes [%d, %d) outside the resident window of %d planes", first_plane, first_plane + nplanes, v->D);
    int rc = use_device(v->dev);
    if (rc) return rc;
    const bool src_dev = (flags & VT_SRC_DEVICE) != 0;
    const size_t rows = (size_t)nplanes * v->H;
    PinnedScope pin(src_dev ? nullptr : data, src_dev ? 0 : rows * v->W * sizeof(float));
    if (src_dev)
        VT_HIP(hipMemcpy2DAsync(v->d_src + (size_t)first_plane * v->H * v->P, (size_t)v->P * sizeof(float), data, (size_t)v->W * sizeof(float),
                                (size_t)v->W * sizeof(float), rows, hipMemcpyDeviceToDevice, v->stream));
    else
        VT_HIP(pin.copy2d(v->d_src + (size_t)first_plane * v->H * v->P, (size_t)v->P * sizeof(float), data, (size_t)v->W * sizeof(float), rows, true, v->stream));
    VT_HIP(hipStreamSynchronize(v->stream));
    return 0;
}

int vt_volume_finalize(vt_volume_t* v)
{
    if (!v) return fail(VT_EINVAL, "NULL handle");
    if (!v->deferred) return 0;
    int rc = use_device(v->dev);
    if (rc) return rc;
    return finalize_resident(v, v->lo_interior);
}

int vt_volume_destroy(vt_volume_t* v)
{
    if (!v) return 0;
    hipSetDevice(v->dev);
    if (v->stream) hipStreamSynchronize(v->stream);
    if (v->d_src) cached_free(v->dev, v->d_src, v->src_bytes);
    if (v->d_queue) hipFree(v->d_queue);
    if (v->d_tplan) hipFree(v->d_tplan);
    {
        LazyCopies::Released rel;
        v->lazy.release_all(rel);
        for (void* b : rel.bufs) hipFree(b);
    }
    if (v->d_scratch_out) cached_free(v->dev, v->d_scratch_out, v->scratch_elems * sizeof(float));
    if (v->d_proj_tmp) hipFree(v->d_proj_tmp);
    if (v->d_proj_part) cached_free(v->dev, v->d_proj_part, v->proj_part_bytes);
    if (v->d_batch_m) hipFree(v->d_batch_m);
    if (v->proj) { vt_volume_destroy(v->proj); v->proj = nullptr; }
    if (v->ev0) recycle_event(v->dev, v->ev0);
    if (v->ev1) recycle_event(v->dev, v->ev1);
    if (v->evc0) (void)hipEventDestroy(v->evc0);
    if (v->evc1) (void)hipEventDestroy(v->evc1);
    if (v->stream && v->owns_stream) recycle_stream(v->dev, v->stream);
    delete v;
    return 0;
}

// Free every resident copy a handle has built lazily besides its plain one (exchanged orientations, plane-quad and z-convolved
// plane-quad forms, the exchanged-result buffer) and the spare; `freed_bytes` is their sum.  They are rebuilt by the first call that
// needs them; results do not change.
int vt_volume_release_copies(vt_volume_t* v, uint64_t* freed_bytes)
{
    if (!v) return fail(VT_EINVAL, "NULL argument");
    int rc = use_device(v->dev);
    if (rc) return rc;
    VT_HIP(hipStreamSynchronize(v->stream));      // no launch may still be reading what is freed
    LazyCopies::Released rel;
    const uint64_t freed = v->lazy.release_all(rel);
    hipError_t e = hipSuccess;
    for (void* b : rel.bufs) if (hipError_t eb = hipFree(b)) e = eb;
    VT_HIP(e);
    if (freed_bytes) *freed_bytes = freed;
    return 0;
}

int vt_has_legacy_kernels(void)
{
#ifdef VT_LEGACY
    return 1;
#else
    return 0;
#endif
}

int vt_volume_info(const vt_volume_t* v, vt_volume_info_t* info)
{
    if (!v || !info) return fail(VT_EINVAL, "NULL argument");
    info->device = v->dev; info->interp = v->interp;
    // the caller's dims: a VT_EDGE_SCIPY handle keeps edge_pad mirrored voxels on every side of the resident copy (v->D/H/W)
    info->depth = v->D - 2 * v->edge_pad; info->height = v->H - 2 * v->edge_pad; info->width = v->W - 2 * v->edge_pad;
    info->out_depth = v->oD; info->out_height = v->oH; info->out_width = v->oW;
    info->last_kernel = v->last_kernel;
    for (int i = 0; i < 3; ++i) { info->last_tile[i] = v->last_tile[i]; info->last_lds_dims[i] = v->last_lds[i]; }
    info->last_lds_bytes = v->last_lds_bytes; info->last_grid = v->last_grid;
    info->prefilter_ms = v->prefilter_ms;
    info->resident_bytes = resident_now(v);
    info->copies_ms = v->copies_ms;
    info->copies_built = v->copies_built;
    info->copies_evicted = v->copies_evicted;
    info->max_resident_bytes = v->lazy.max_resident;
    return 0;
}

// Resident-memory budget of a handle (round 5; no reference counterpart: the reference keeps one CUDA array per StaticVolume,
// volume.py:37-45).  `bytes` counts what vt_volume_info.resident_bytes counts: the plain resident copy, the projection helper, every
// lazily built copy at the size of its allocation and the spare; 0 = no limit (the default unless VT_MAX_RESIDENT_GB is set).  The rules
// (vt_resident.h): a copy that would take the handle over its budget is built only after the least recently used copies have been
// released, never one the same call has touched (per-call pins); a copy that cannot fit beside the plain copy and the pinned ones is
// refused before anything is released, and the call runs on a kernel family that samples the plain layout.  A budget below the
// handle's present footprint releases copies at once (this runs outside a call: nothing is pinned).  Results never depend on the budget.
int vt_volume_set_max_resident(vt_volume_t* v, uint64_t bytes)
{
    if (!v) return fail(VT_EINVAL, "NULL argument");
    int rc = use_device(v->dev);
    if (rc) return rc;
    v->lazy.max_resident = bytes;
    LazyCopies::Released rel;
    v->lazy.trim(fixed_bytes(v), -1, rel);       // (outside a call: nothing is pinned)
    release(v, rel);
    v->lazy.clear_retries();
    return 0;
}

int vt_volume_stream(const vt_volume_t* v, void** hip_stream)
{
    if (!v || !hip_stream) return fail(VT_EINVAL, "NULL argument");
    *hip_stream = reinterpret_cast<void*>(v->stream);
    return 0;
}

int vt_volume_sync(vt_volume_t* v)
{
    if (!v) return fail(VT_EINVAL, "NULL handle");
    int rc = use_device(v->dev);
    if (rc) return rc;
    VT_HIP(hipStreamSynchronize(v->stream));
    return 0;
}

int vt_volume_set_output_shape(vt_volume_t* v, int od, int oh, int ow)
{
    if (!v) return fail(VT_EINVAL, "NULL handle");
    if (od <= 0 || oh <= 0 || ow <= 0) return fail(VT_EINVAL, "non-positive output dims");
    if ((int64_t)od * oh > 0x7fffffffLL || (int64_t)oh * ow > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "output too large");
    v->oD = od; v->oH = oh; v->oW = ow;
    return 0;
}

int vt_volume_affine(vt_volume_t* v, const float* m4x4, float* out, int flags)
{
    if (!m4x4) return fail(VT_EINVAL, "NULL matrix");
    double m[16];
    for (int i = 0; i < 16; ++i) m[i] = (double)m4x4[i];
    return do_affine(v, m, out, flags);
}

int vt_volume_affine_f64(vt_volume_t* v, const double* m4x4, float* out, int flags)
{
    return do_affine(v, m4x4, out, flags);
}

int vt_volume_affine_batch(vt_volume_t* v, int n, const float* m4x4s, float* out, int flags)
{
    if (!m4x4s || n <= 0) return fail(VT_EINVAL, "NULL matrices or empty batch");
    return do_affine_batch(v, n, widened(m4x4s, n).data(), out, flags);
}

int vt_volume_extract(vt_volume_t* v, int n, const float* m4x4s, int box_d, int box_h, int box_w, float* out, int flags)
{
    if (!v || !m4x4s || !out || n <= 0) return fail(VT_EINVAL, "NULL argument or empty batch");
    return do_extract(v, n, widened(m4x4s, n).data(), box_d, box_h, box_w, out, flags);
}

int vt_volume_extract_f64(vt_volume_t* v, int n, const double* m4x4s, int box_d, int box_h, int box_w, float* out, int flags)
{
    return do_extract(v, n, m4x4s, box_d, box_h, box_w, out, flags);
}

int vt_volume_extract_sum(vt_volume_t* v, int n, const float* m4x4s, const double* weights, int box_d, int box_h, int box_w, float* out,
                          int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (n <= 0) return fail(VT_EINVAL, "batch size %d", n);
    return do_extract_sum(v, n, widened(m4x4s, n).data(), weights, box_d, box_h, box_w, out, flags);
}

int vt_volume_extract_sum_f64(vt_volume_t* v, int n, const double* m4x4s, const double* weights, int box_d, int box_h, int box_w, float* out,
                              int flags)
{
    return do_extract_sum(v, n, m4x4s, weights, box_d, box_h, box_w, out, flags);
}

int vt_volume_extract_sum_multi(vt_volume_t* v, int n, const float* m4x4s, int g, const double* weights, int box_d, int box_h, int box_w,
                                float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (n <= 0) return fail(VT_EINVAL, "batch size %d", n);
    return do_extract_sum_multi(v, n, widened(m4x4s, n).data(), g, weights, box_d, box_h, box_w, out, flags);
}

int vt_volume_extract_sum_multi_f64(vt_volume_t* v, int n, const double* m4x4s, int g, const double* weights, int box_d, int box_h, int box_w,
                                    float* out, int flags)
{
    return do_extract_sum_multi(v, n, m4x4s, g, weights, box_d, box_h, box_w, out, flags);
}

int vt_volume_place(vt_volume_t* v, int n, const float* m4x4s, const double* weights, int out_d, int out_h, int out_w, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (n <= 0) return fail(VT_EINVAL, "batch size %d", n);
    return do_place(v, n, widened(m4x4s, n).data(), weights, out_d, out_h, out_w, out, flags);
}

int vt_volume_place_f64(vt_volume_t* v, int n, const double* m4x4s, const double* weights, int out_d, int out_h, int out_w, float* out,
                        int flags)
{
    return do_place(v, n, m4x4s, weights, out_d, out_h, out_w, out, flags);
}

int vt_volume_backproject(vt_volume_t* v, int n, const float* m4x4s, const int32_t* planes, const double* weights, int out_d, int out_h,
                          int out_w, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (n <= 0) return fail(VT_EINVAL, "batch size %d", n);
    return do_backproject(v, n, widened(m4x4s, n).data(), planes, weights, out_d, out_h, out_w, out, flags);
}

int vt_volume_backproject_f64(vt_volume_t* v, int n, const double* m4x4s, const int32_t* planes, const double* weights, int out_d, int out_h,
                              int out_w, float* out, int flags)
{
    return do_backproject(v, n, m4x4s, planes, weights, out_d, out_h, out_w, out, flags);
}

int vt_volume_backproject_boxes(vt_volume_t* v, int nb, int n, const float* m4x4s, const int32_t* planes, const double* weights, int box_d,
                                int box_h, int box_w, float* out, int flags)
{
    return do_backproject_boxes(v, nb, n, m4x4s, planes, weights, box_d, box_h, box_w, out, flags);
}

int vt_volume_backproject_boxes_f64(vt_volume_t* v, int nb, int n, const double* m4x4s, const int32_t* planes, const double* weights,
                                    int box_d, int box_h, int box_w, float* out, int flags)
{
    return do_backproject_boxes(v, nb, n, m4x4s, planes, weights, box_d, box_h, box_w, out, flags);
}

int vt_volume_affine_stack(vt_volume_t* v, int n, const float* m4x4s, const int32_t* planes, const double* weights, int out_h, int out_w,
                           float* out, int flags)
{
    return do_affine_stack(v, n, m4x4s, planes, weights, out_h, out_w, out, flags);
}

int vt_volume_affine_stack_f64(vt_volume_t* v, int n, const double* m4x4s, const int32_t* planes, const double* weights, int out_h, int out_w,
                               float* out, int flags)
{
    return do_affine_stack(v, n, m4x4s, planes, weights, out_h, out_w, out, flags);
}

int vt_volume_warp(vt_volume_t* v, const float* m4x4, const float* grid, int grid_d, int grid_h, int grid_w, int out_d, int out_h, int out_w,
                   float* out, int flags)
{
    double m[16];
    if (m4x4)
        for (int i = 0; i < 16; ++i) m[i] = (double)m4x4[i];
    return do_warp(v, m4x4 ? m : nullptr, grid, grid_d, grid_h, grid_w, out_d, out_h, out_w, out, flags);
}

int vt_volume_warp_f64(vt_volume_t* v, const double* m4x4, const float* grid, int grid_d, int grid_h, int grid_w, int out_d, int out_h,
                       int out_w, float* out, int flags)
{
    return do_warp(v, m4x4, grid, grid_d, grid_h, grid_w, out_d, out_h, out_w, out, flags);
}

int vt_volume_warp_stack_sum(vt_volume_t* v, int n, const float* m4x4s, const float* grids, int n_grids, int grid_h, int grid_w,
                             const int32_t* planes, int g, const double* weights, int out_h, int out_w, float* out, int flags)
{
    return do_warp_stack_sum(v, n, m4x4s, grids, n_grids, grid_h, grid_w, planes, g, weights, out_h, out_w, out, flags);
}

int vt_volume_warp_stack_sum_f64(vt_volume_t* v, int n, const double* m4x4s, const float* grids, int n_grids, int grid_h, int grid_w,
                                 const int32_t* planes, int g, const double* weights, int out_h, int out_w, float* out, int flags)
{
    return do_warp_stack_sum(v, n, m4x4s, grids, n_grids, grid_h, grid_w, planes, g, weights, out_h, out_w, out, flags);
}

int vt_volume_warp_stack(vt_volume_t* v, int n, const float* m4x4s, const float* grids, int n_grids, int grid_h, int grid_w,
                         const int32_t* planes, const double* weights, int out_h, int out_w, float* out, int flags)
{
    return do_warp_stack(v, n, m4x4s, grids, n_grids, grid_h, grid_w, planes, weights, out_h, out_w, out, flags);
}

int vt_volume_warp_stack_f64(vt_volume_t* v, int n, const double* m4x4s, const float* grids, int n_grids, int grid_h, int grid_w,
                             const int32_t* planes, const double* weights, int out_h, int out_w, float* out, int flags)
{
    return do_warp_stack(v, n, m4x4s, grids, n_grids, grid_h, grid_w, planes, weights, out_h, out_w, out, flags);
}

int vt_volume_filter_stack(vt_volume_t* v, int n, const int32_t* planes, const double* taps, int n_taps, int k, int axis, int pad,
                           const double* weights, float* out, int flags)
{
    return do_filter_stack(v, n, planes, taps, n_taps, k, axis, pad, weights, out, flags);
}

int vt_volume_correlate_stack(vt_volume_t* v, int n, const int32_t* planes, const float* refs, int n_refs, const int32_t* ref_planes,
                              int grid_h, int grid_w, int r_h, int r_w, double* out, int flags)
{
    return do_correlate_stack(v, n, planes, refs, n_refs, ref_planes, grid_h, grid_w, r_h, r_w, out, flags);
}

int vt_volume_moments_stack(vt_volume_t* v, int n, const int32_t* planes, int grid_h, int grid_w, int r_h, int r_w, double* out, int flags)
{
    return do_moments_stack(v, n, planes, grid_h, grid_w, r_h, r_w, out, flags);
}

int vt_volume_extract_dot(vt_volume_t* v, int n, const float* m4x4s, const float* tmpl, const float* mask, int box_d, int box_h, int box_w,
                          double* out, int flags)
{
    if (!v || !m4x4s || !tmpl || !out) return fail(VT_EINVAL, "NULL argument");
    if (n <= 0) return fail(VT_EINVAL, "batch size %d", n);
    return do_extract_dot(v, n, widened(m4x4s, n).data(), tmpl, mask, box_d, box_h, box_w, out, flags);
}

int vt_volume_extract_dot_f64(vt_volume_t* v, int n, const double* m4x4s, const float* tmpl, const float* mask, int box_d, int box_h, int box_w,
                              double* out, int flags)
{
    return do_extract_dot(v, n, m4x4s, tmpl, mask, box_d, box_h, box_w, out, flags);
}

int vt_volume_extract_dot_multi(vt_volume_t* v, int n, const float* m4x4s, int k, const float* tmpls, const float* mask, int box_d, int box_h,
                                int box_w, double* out, int flags)
{
    if (!v || !m4x4s || !tmpls || !out) return fail(VT_EINVAL, "NULL argument");
    if (n <= 0) return fail(VT_EINVAL, "batch size %d", n);
    return do_extract_dot_multi(v, n, widened(m4x4s, n).data(), k, tmpls, mask, box_d, box_h, box_w, out, flags);
}

int vt_volume_extract_dot_multi_f64(vt_volume_t* v, int n, const double* m4x4s, int k, const float* tmpls, const float* mask, int box_d,
                                    int box_h, int box_w, double* out, int flags)
{
    return do_extract_dot_multi(v, n, m4x4s, k, tmpls, mask, box_d, box_h, box_w, out, flags);
}

int vt_volume_project(vt_volume_t* v, const float* m4x4, float* out_hw, int flags)
{
    if (!m4x4) return fail(VT_EINVAL, "NULL matrix");
    double m[16];
    for (int i = 0; i < 16; ++i) m[i] = (double)m4x4[i];
    return do_project(v, m, out_hw, flags);
}

int vt_volume_project_f64(vt_volume_t* v, const double* m4x4, float* out_hw, int flags)
{
    return do_project(v, m4x4, out_hw, flags);
}

int vt_volume_project_batch(vt_volume_t* v, int n, const float* m4x4s, int depth, int height, int width, float* out, int flags)
{
    if (!v || !m4x4s || !out) return fail(VT_EINVAL, "NULL argument");
    if (n <= 0) return fail(VT_EINVAL, "batch size %d", n);
    return do_project_batch(v, n, widened(m4x4s, n).data(), depth, height, width, out, flags);
}

int vt_volume_project_batch_f64(vt_volume_t* v, int n, const double* m4x4s, int depth, int height, int width, float* out, int flags)
{
    return do_project_batch(v, n, m4x4s, depth, height, width, out, flags);
}

int vt_timer_start(vt_volume_t* v)
{
    if (!v) return fail(VT_EINVAL, "NULL handle");
    int rc = use_device(v->dev);
    if (rc) return rc;
    VT_HIP(hipEventRecord(v->ev0, v->stream));
    return 0;
}

int vt_timer_stop(vt_volume_t* v, float* ms)
{
    if (!v || !ms) return fail(VT_EINVAL, "NULL argument");
    int rc = use_device(v->dev);
    if (rc) return rc;
    VT_HIP(hipEventRecord(v->ev1, v->stream));
    VT_HIP(hipEventSynchronize(v->ev1));
    VT_HIP(hipEventElapsedTime(ms, v->ev0, v->ev1));
    return 0;
}

int vt_prefilter_inplace(int dev, float* d_volume, int D, int H, int W)
{
    if (!d_volume) return fail(VT_EINVAL, "NULL volume");
    if (D <= 0 || H <= 0 || W <= 0) return fail(VT_EINVAL, "non-positive dims");
    if ((int64_t)D * H > 0x7fffffffLL || (int64_t)H * W > 0x7fffffffLL) return fail(VT_EUNSUPPORTED, "volume too large");
    int rc = init_device(dev);
    if (rc) return rc;
    const size_t bytes = (size_t)D * H * W * sizeof(float);
    float* d_tmp = nullptr;
    VT_HIP(hipMalloc(reinterpret_cast<void**>(&d_tmp), bytes));
    float* res = nullptr;
    rc = run_prefilter(d_volume, d_tmp, D, H, W, W, false, nullptr, &res);
    if (!rc && res != d_volume) {
        hipError_t e = hipMemcpyAsync(d_volume, res, bytes, hipMemcpyDeviceToDevice, nullptr);
        if (e != hipSuccess) rc = fail((int)e, "copy back: %s", hipGetErrorString(e));
    }
    hipError_t es = hipStreamSynchronize(nullptr);
    hipFree(d_tmp);
    if (!rc && es != hipSuccess) rc = fail((int)es, "prefilter: %s", hipGetErrorString(es));
    return rc;
}

// One-shot transform of a host volume into a host buffer (transforms.py:164-226): upload, prefilter, transform, download.
// PCIe-bound (512^3: 2 x 9.4 ms of copies around < 1.5 ms of kernels).  Where the output planes only need nearby source
// planes (axis-0-separable matrices, no prefilter) the call is pipelined so that both PCIe directions run at once
// (oneshot_pipelined below); everything else is the plain sequence.
int vt_affine_oneshot(int dev, const float* h_volume, int D, int H, int W, int interp, const float* m4x4,
                      float* h_out, int flags, float* elapsed_ms)
{
    if (!h_volume || !m4x4 || !h_out) return fail(VT_EINVAL, "NULL argument");
    int rc = init_device(dev);
    if (rc) return rc;
    hipEvent_t t0, t1;
    VT_HIP(hipEventCreate(&t0));
    VT_HIP(hipEventCreate(&t1));
    hipEventRecord(t0, nullptr);
    vt_volume_t* v = nullptr;
    static const bool no_pipe = std::getenv("VT_ONESHOT_SEQ") != nullptr;      // A/B switch: always the plain sequence
    const bool edge = (flags & VT_ONESHOT_EDGE_SCIPY) != 0;
    flags &= ~VT_ONESHOT_EDGE_SCIPY;
    rc = (no_pipe || edge) ? 1 : oneshot_pipelined(dev, h_volume, D, H, W, interp, m4x4, h_out, flags & ~VT_OUT_DEVICE);
    if (rc == 1) {
        rc = vt_volume_create(dev, D, H, W, interp, h_volume, edge ? VT_EDGE_SCIPY : 0, &v);
        if (!rc) rc = vt_volume_affine(v, m4x4, h_out, flags & ~VT_OUT_DEVICE);
    }
    hipEventRecord(t1, nullptr);
    hipEventSynchronize(t1);
    if (elapsed_ms) hipEventElapsedTime(elapsed_ms, t0, t1);
    hipEventDestroy(t0);
    hipEventDestroy(t1);
    vt_volume_destroy(v);
    return rc;
}

}  // extern "C"

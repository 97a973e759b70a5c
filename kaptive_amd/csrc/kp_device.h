// kp_device.h -- owners of the device resources the C API holds: each frees what it holds when it goes away and cannot be
// copied.  None of them may have static storage duration: nothing calls into the HIP runtime while the process ends.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <utility>

extern std::atomic<long long> g_dev_allocs;  // re-allocations of device buffers since the process started
extern bool g_debug_alloc;                   // KAPTIVE_AMD_DEBUG_ALLOC (options_from_env): a line on stderr for each of them

// page-locked host memory, counted for kp_host_pinned_bytes (kp_ctx.hip)
hipError_t pinned_alloc(void **out, size_t bytes);
void pinned_free(void *p);

#define KP_MOVE_ONLY(T) /* moves like a unique_ptr: the source is left empty; declaring the moves deletes the copies */ \
    T() = default;                                                                                                         \
    T(T &&o) noexcept { swap(o); }                                                                                         \
    T &operator=(T &&o) noexcept { T t(std::move(o)); swap(t); return *this; }

template <class T>
struct DevBuf {  // growable device allocation
    T *p = nullptr;
    size_t n = 0;
    KP_MOVE_ONLY(DevBuf)
    ~DevBuf() { if (p) (void)hipFree(p); }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(n, o.n); }
    hipError_t reserve(size_t want) {
        if (want <= n) return hipSuccess;
        // hipFree / hipMalloc wait for the whole device: a buffer that grows while passes are in flight stalls the pipeline for
        // as long as those passes take (kp_device_allocations counts them, so that a caller can show a stream of batches does none)
        if (p) {
            g_dev_allocs.fetch_add(1, std::memory_order_relaxed);
            if (g_debug_alloc)
                std::fprintf(stderr, "[DevBuf] re-allocation: %zu -> %zu items of %zu bytes\n", n, want, sizeof(T));
            want += want / 8;  // a buffer that had to grow once gets head-room: sizes that creep by a per cent from batch to
                               // batch (the fullest assembly of a batch decides several of them) must not re-allocate each time
        }
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
        hipError_t e = hipMalloc((void **)&p, std::max<size_t>(want, 1) * sizeof(T));
        if (e == hipSuccess) n = want;
        return e;
    }
};

struct DevBlock {  // raw device block that its user allocates and grows (kp_sort_anchors)
    void *p = nullptr;
    size_t bytes = 0;
    KP_MOVE_ONLY(DevBlock)
    ~DevBlock() { if (p) (void)hipFree(p); }
    void swap(DevBlock &o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
};

struct PinnedBlock {  // page-locked host block that only grows (landing area of read-backs, staging of a batch's tables)
    uint8_t *p = nullptr;
    size_t bytes = 0;
    KP_MOVE_ONLY(PinnedBlock)
    ~PinnedBlock() { pinned_free(p); }
    void swap(PinnedBlock &o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
    // at least `need` bytes, `want` if it has to grow (contents are not kept; nothing may be in flight towards the old block)
    hipError_t reserve(size_t need, size_t want) {
        if (need <= bytes) return hipSuccess;
        pinned_free(p);
        p = nullptr; bytes = 0;
        const hipError_t e = pinned_alloc((void **)&p, want);
        if (e == hipSuccess) bytes = want;
        return e;
    }
};

template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    KP_MOVE_ONLY(Handle)
    ~Handle() { if (h) (void)Destroy(h); }
    void swap(Handle &o) { std::swap(h, o.h); }
    operator H() const { return h; }
};
// an owned stream: whatever is still queued on it runs to its end before the stream is destroyed
inline hipError_t kp_stream_drain_destroy(hipStream_t s) { (void)hipStreamSynchronize(s); return hipStreamDestroy(s); }
using Stream = Handle<hipStream_t, kp_stream_drain_destroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

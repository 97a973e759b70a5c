// kp_ctx.hip -- context of the C ABI (include/kaptive_amd.h): errors, page-locked host memory, options, creation, destruction.
#include <cctype>
#include <cstdlib>
#include <mutex>
#include <new>
#include <unordered_map>
#include <sys/mman.h>

#include "kp_host.h"

static std::mutex g_err_mutex;
static std::string g_global_error = "";

std::atomic<long long> g_dev_allocs{0};
bool g_debug_alloc = false;

// Page-locked host memory the library holds (kp_host_alloc and the batches' table staging), for kp_host_pinned_bytes.
// Two kinds: small blocks straight from hipHostMalloc; large ones (the callers' shard buffers) as anonymous memory
// advised to use huge pages and then registered -- locking 0.8 GB of 4 KB pages costs 139 ms and 84 ms to give back,
// of 2 MB pages 54 ms (51 of them the first touch, which a caller that fills the block before it locks it spreads over
// its own threads: kp_host_reserve / kp_host_lock) and 31 ms; a process that ends holding 3.2 GB leaves the kernel
// 410 ms of work against 168 (tools/microbench/pin_thp.cpp).
static std::mutex g_pin_mutex;
struct PinBlock { size_t bytes; bool mapped, locked; };
static std::unordered_map<void *, PinBlock> g_pin_blocks;
static size_t g_pin_bytes = 0;
constexpr size_t HUGE_PAGE = (size_t)2 << 20;
hipError_t pinned_alloc(void **out, size_t bytes) {
    // portable: usable by every device's context whichever thread (and current device) allocates it -- a reader thread of
    // the CLI takes page-locked buffers while the driving thread holds the context
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocPortable);
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_pin_mutex);
        g_pin_blocks[*out] = PinBlock{bytes, false, true};
        g_pin_bytes += bytes;
    }
    return e;
}
static void *mapped_alloc(size_t bytes) {  // 2 MB-aligned anonymous memory, huge pages where the system grants them on advice
    bytes = (bytes + HUGE_PAGE - 1) & ~(HUGE_PAGE - 1);
    char *raw = (char *)mmap(nullptr, bytes + HUGE_PAGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (raw == MAP_FAILED) return nullptr;
    char *p = (char *)(((uintptr_t)raw + HUGE_PAGE - 1) & ~(uintptr_t)(HUGE_PAGE - 1));
    if (p > raw) munmap(raw, (size_t)(p - raw));
    if (raw + HUGE_PAGE > p) munmap(p + bytes, (size_t)(raw + HUGE_PAGE - p));
    (void)madvise(p, bytes, MADV_HUGEPAGE);  // (refused where transparent huge pages are off: plain pages then)
    std::lock_guard<std::mutex> lk(g_pin_mutex);
    g_pin_blocks[p] = PinBlock{bytes, true, false};
    return p;
}
static hipError_t mapped_lock(void *p) {
    size_t bytes;
    {
        std::lock_guard<std::mutex> lk(g_pin_mutex);
        auto it = g_pin_blocks.find(p);
        if (it == g_pin_blocks.end() || !it->second.mapped) return hipErrorInvalidValue;
        if (it->second.locked) return hipSuccess;
        bytes = it->second.bytes;
    }
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_pin_mutex);
        g_pin_blocks[p].locked = true;
        g_pin_bytes += bytes;
    }
    return e;
}
void pinned_free(void *p) {
    if (!p) return;
    PinBlock b{0, false, true};
    {
        std::lock_guard<std::mutex> lk(g_pin_mutex);
        auto it = g_pin_blocks.find(p);
        if (it != g_pin_blocks.end()) {
            b = it->second;
            if (b.locked) g_pin_bytes -= b.bytes;
            g_pin_blocks.erase(it);
        }
    }
    if (b.mapped) {
        if (b.locked) (void)hipHostUnregister(p);
        munmap(p, b.bytes);
    } else {
        (void)hipHostFree(p);
    }
}

int kp_fail(kp_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->error = msg;
    else {
        std::lock_guard<std::mutex> lk(g_err_mutex);
        g_global_error = msg;
    }
    return code;
}

hipError_t create_priority_stream(hipStream_t *stream) {
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess) return e;
    return hipStreamCreateWithPriority(stream, hipStreamDefault, greatest);
}

static uint32_t env_u32(const char *name, uint32_t dflt) {
    const char *v = std::getenv(name);
    if (!v || !*v) return dflt;
    const long long x = std::atoll(v);
    return x > 0 ? (uint32_t)x : dflt;
}

// the environment is read here, once per context, and nowhere else
static void options_from_env(KpOptions &o) {
    o.anchor_cap = env_u32("KAPTIVE_AMD_ANCHOR_CAP", o.anchor_cap);
    o.tasks_per_asm = env_u32("KAPTIVE_AMD_TASKS_PER_ASM", o.tasks_per_asm);
    o.hit_cap = env_u32("KAPTIVE_AMD_HIT_CAP", o.hit_cap);
    o.trace_kb_per_asm = env_u32("KAPTIVE_AMD_TRACE_KB_PER_ASM", o.trace_kb_per_asm);
    o.trace_set = env_u32("KAPTIVE_AMD_TRACE_KB_PER_ASM", 0) != 0;
    o.cand_cap = env_u32("KAPTIVE_AMD_CAND_CAP", 0);
    o.group_cap = env_u32("KAPTIVE_AMD_GROUP_CAP", o.group_cap);
    o.join_cap = env_u32("KAPTIVE_AMD_JOIN_CAP", o.join_cap);
    o.occ_slots = env_u32("KAPTIVE_AMD_OCC_SLOTS", o.occ_slots);
    o.kept_cap = env_u32("KAPTIVE_AMD_KEPT_CAP", o.kept_cap);
    o.piece_cap = env_u32("KAPTIVE_AMD_PIECE_CAP", o.piece_cap);
    o.prot_cap = env_u32("KAPTIVE_AMD_PROT_CAP", o.prot_cap);
    o.scan_mode = (int)env_u32("KAPTIVE_AMD_SCAN_ABLATE", 0);
    o.library_sort = (int)env_u32("KAPTIVE_AMD_LIBRARY_SORT", 0);
    o.upload_piece_mb = std::max<uint32_t>(1, env_u32("KAPTIVE_AMD_UPLOAD_PIECE_MB", 4096));
    { const char *rb = getenv("KAPTIVE_AMD_READBACK"); o.readback_copy_engine = rb && std::string(rb) == "copy"; }
    o.spin_wait = (int)env_u32("KAPTIVE_AMD_SPIN_WAIT", 0);
    { const char *ts = std::getenv("KAPTIVE_AMD_TRACE_SUMMARY"); o.trace_summary = !(ts && std::string(ts) == "0"); }
    o.join_stats = std::getenv("KAPTIVE_AMD_JOIN_STATS") != nullptr;
    if (const char *e = std::getenv("KAPTIVE_AMD_JOIN_GRID")) std::sscanf(e, "%d,%d,%d,%d", &o.join.fill, &o.join.walk, &o.join.chain, &o.join.chain_large);
    if (const char *e = std::getenv("KAPTIVE_AMD_JOIN_PRIO")) o.join.prio = std::atoi(e);
    if (const char *e = std::getenv("KAPTIVE_AMD_SKIP_JOINS")) o.join.skip = std::atoi(e);
    g_debug_alloc = std::getenv("KAPTIVE_AMD_DEBUG_ALLOC") != nullptr;  // (process-wide: DevBuf knows no context)
}

// BLOSUM62 as the reference lays it out: 256x256 bytes, -128 outside ARNDCQEGHILKMFPSTWYVBJZX*
// (src/kaptive/core/pairwise.py:343-391)
static void fill_blosum(int8_t *m) {
    static const int8_t b[25][25] = {
        {4, -1, -2, -2, 0, -1, -1, 0, -2, -1, -1, -1, -1, -2, -1, 1, 0, -3, -2, 0, -2, -1, -1, -1, -4},
        {-1, 5, 0, -2, -3, 1, 0, -2, 0, -3, -2, 2, -1, -3, -2, -1, -1, -3, -2, -3, -1, -2, 0, -1, -4},
        {-2, 0, 6, 1, -3, 0, 0, 0, 1, -3, -3, 0, -2, -3, -2, 1, 0, -4, -2, -3, 4, -3, 0, -1, -4},
        {-2, -2, 1, 6, -3, 0, 2, -1, -1, -3, -4, -1, -3, -3, -1, 0, -1, -4, -3, -3, 4, -3, 1, -1, -4},
        {0, -3, -3, -3, 9, -3, -4, -3, -3, -1, -1, -3, -1, -2, -3, -1, -1, -2, -2, -1, -3, -1, -3, -1, -4},
        {-1, 1, 0, 0, -3, 5, 2, -2, 0, -3, -2, 1, 0, -3, -1, 0, -1, -2, -1, -2, 0, -2, 4, -1, -4},
        {-1, 0, 0, 2, -4, 2, 5, -2, 0, -3, -3, 1, -2, -3, -1, 0, -1, -3, -2, -2, 1, -3, 4, -1, -4},
        {0, -2, 0, -1, -3, -2, -2, 6, -2, -4, -4, -2, -3, -3, -2, 0, -2, -2, -3, -3, -1, -4, -2, -1, -4},
        {-2, 0, 1, -1, -3, 0, 0, -2, 8, -3, -3, -1, -2, -1, -2, -1, -2, -2, 2, -3, 0, -3, 0, -1, -4},
        {-1, -3, -3, -3, -1, -3, -3, -4, -3, 4, 2, -3, 1, 0, -3, -2, -1, -3, -1, 3, -3, 3, -3, -1, -4},
        {-1, -2, -3, -4, -1, -2, -3, -4, -3, 2, 4, -2, 2, 0, -3, -2, -1, -2, -1, 1, -4, 3, -3, -1, -4},
        {-1, 2, 0, -1, -3, 1, 1, -2, -1, -3, -2, 5, -1, -3, -1, 0, -1, -3, -2, -2, 0, -3, 1, -1, -4},
        {-1, -1, -2, -3, -1, 0, -2, -3, -2, 1, 2, -1, 5, 0, -2, -1, -1, -1, -1, 1, -3, 2, -1, -1, -4},
        {-2, -3, -3, -3, -2, -3, -3, -3, -1, 0, 0, -3, 0, 6, -4, -2, -2, 1, 3, -1, -3, 0, -3, -1, -4},
        {-1, -2, -2, -1, -3, -1, -1, -2, -2, -3, -3, -1, -2, -4, 7, -1, -1, -4, -3, -2, -2, -3, -1, -1, -4},
        {1, -1, 1, 0, -1, 0, 0, 0, -1, -2, -2, 0, -1, -2, -1, 4, 1, -3, -2, -2, 0, -2, 0, -1, -4},
        {0, -1, 0, -1, -1, -1, -1, -2, -2, -1, -1, -1, -1, -2, -1, 1, 5, -2, -2, 0, -1, -1, -1, -1, -4},
        {-3, -3, -4, -4, -2, -2, -3, -2, -2, -3, -2, -3, -1, 1, -4, -3, -2, 11, 2, -3, -4, -2, -2, -1, -4},
        {-2, -2, -2, -3, -2, -1, -2, -3, 2, -1, -1, -2, -1, 3, -3, -2, -2, 2, 7, -1, -3, -1, -2, -1, -4},
        {0, -3, -3, -3, -1, -2, -2, -3, -3, 3, 1, -2, 1, -1, -2, -2, 0, -3, -1, 4, -3, 2, -2, -1, -4},
        {-2, -1, 4, 4, -3, 0, 1, -1, 0, -3, -4, 0, -3, -3, -2, 0, -1, -4, -3, -3, 4, -3, 0, -1, -4},
        {-1, -2, -3, -3, -1, -2, -3, -4, -3, 3, 3, -3, 2, 0, -3, -2, -1, -2, -1, 2, -3, 3, -3, -1, -4},
        {-1, 0, 0, 1, -3, 4, 4, -2, 0, -3, -3, 1, -1, -3, -1, 0, -1, -2, -2, -2, 0, -3, 4, -1, -4},
        {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -4},
        {-4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, 1},
    };
    static const char alphabet[] = "ARNDCQEGHILKMFPSTWYVBJZX*";
    std::memset(m, KP_PROT_FILL, 256 * 256);
    for (int x = 0; x < 25; ++x)
        for (int y = 0; y < 25; ++y) m[(uint8_t)alphabet[x] * 256 + (uint8_t)alphabet[y]] = b[x][y];
}

extern "C" {

int kp_device_count(void) {
    int n_dev = 0;
    const hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess) return kp_fail(nullptr, KP_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return n_dev;
}

int kp_device_numa_node(int device_id) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device_id) != hipSuccess) return -1;
    for (char *c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);  // sysfs names are lower case
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    std::FILE *f = std::fopen(path.c_str(), "r");
    if (!f) return -1;
    int node = -1;
    if (std::fscanf(f, "%d", &node) != 1) node = -1;
    std::fclose(f);
    return node;
}

int kp_ctx_create(int device_id, kp_ctx **out) {
    if (!out) return kp_fail(nullptr, KP_EINVAL, "out is null");
    *out = nullptr;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev == 0)
        return kp_fail(nullptr, KP_EHIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= n_dev) return kp_fail(nullptr, KP_EINVAL, "device_id out of range");
    kp_ctx *ctx = new (std::nothrow) kp_ctx();
    if (!ctx) return kp_fail(nullptr, KP_ENOMEM, "out of host memory");
    ctx->device = device_id;
    options_from_env(ctx->opt);
    // The driving thread spends most of its time waiting for the device (scores, records): blocked on an interrupt it
    // leaves its core to the readers that feed the next shard (eight ranks and their ingest share one host); the
    // runtime's default spins.  (A device-wide flag: it has to be set before the device's streams exist.)
    if ((e = hipSetDevice(device_id)) == hipSuccess && !ctx->opt.spin_wait) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
    if (e != hipSuccess || (e = hipStreamCreate(&ctx->stream.h)) != hipSuccess || (e = hipStreamCreateWithFlags(&ctx->copy.h, hipStreamNonBlocking)) != hipSuccess ||
        (e = create_priority_stream(&ctx->post.h)) != hipSuccess || (e = create_priority_stream(&ctx->aux.h)) != hipSuccess) {
        delete ctx;
        return kp_fail(nullptr, KP_EHIP, std::string("device setup failed: ") + hipGetErrorString(e));
    }
    std::vector<int8_t> m(256 * 256);
    fill_blosum(m.data());
    std::vector<float> ln(KP_MAPQ_LN_HALF_SIZE + KP_MAPQ_LN_INT_SIZE, 0.0f);
    for (int i = 1; i < KP_MAPQ_LN_HALF_SIZE; ++i) ln[(size_t)i] = kp_mapq_ln((double)i / 2.0);
    for (int i = 1; i < KP_MAPQ_LN_INT_SIZE; ++i) ln[(size_t)KP_MAPQ_LN_HALF_SIZE + i] = kp_mapq_ln((double)i);
    if (upload(ctx, ctx->d_blosum, m.data(), m.size()) != KP_OK || upload(ctx, ctx->d_ln, ln.data(), ln.size()) != KP_OK || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        std::string msg = ctx->error;
        kp_ctx_destroy(ctx);
        return kp_fail(nullptr, KP_EHIP, "substitution table upload failed: " + msg);
    }
    *out = ctx;
    return KP_OK;
}

void kp_ctx_destroy(kp_ctx *ctx) {
    if (!ctx) return;
    // nothing is freed before the device is current and idle; the members then go in reverse order of declaration
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (kp_batch *b : ctx->batches) {  // batches that outlive their context keep nothing on the device
        b->in.reset();
        b->ctx = nullptr; b->w = nullptr; b->last_w = nullptr;
    }
    delete ctx;
}

const char *kp_last_error(const kp_ctx *ctx) {
    if (ctx) return ctx->error.c_str();
    std::lock_guard<std::mutex> lk(g_err_mutex);
    static thread_local std::string copy;
    copy = g_global_error;
    return copy.c_str();
}

void *kp_ctx_stream(kp_ctx *ctx) { return ctx ? (void *)ctx->stream.h : nullptr; }

int kp_ctx_set_option(kp_ctx *ctx, const char *name, int64_t value) {
    if (!ctx) return kp_fail(nullptr, KP_EINVAL, "null context");
    if (!name || value < 0) return kp_fail(ctx, KP_EINVAL, "bad option");
    const std::string n(name);
    KpOptions &o = ctx->opt;
    if (kp_caps_set_option(o, ctx->learnt, ctx->run_caps, n, value)) return KP_OK;
    if (kp_caps_set_cs_option(ctx->cs_caps, n, value)) return KP_OK;
    if (kp_caps_set_variants_option(ctx->var_caps, n, value)) return KP_OK;
    if (n == "scan_mode") o.scan_mode = (int)value;
    else if (n == "library_sort") o.library_sort = value != 0;
    else if (n == "cigar") o.cigar = value != 0;
    else if (n == "cs") o.cs = value != 0;
    else if (n == "variants") o.variants = value != 0;
    else if (n == "aligned") o.aligned = value != 0;
    else if (n == "rescue") o.rescue = value != 0;
    else if (n == "rescue_flank") {
        if (value > KP_RESCUE_FLANK_MAX) return kp_fail(ctx, KP_EINVAL, "rescue_flank must be within [0, 65535]");
        o.rescue_flank = (int)value;
    }
    else if (n == "upload_piece_mb") o.upload_piece_mb = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(value, 4096));
    else return kp_fail(ctx, KP_EINVAL, "unknown option: " + n);
    return KP_OK;
}

int kp_host_alloc(size_t bytes, void **out) {
    if (!out) return kp_fail(nullptr, KP_EINVAL, "out is null");
    *out = nullptr;
    if (bytes >= 4 * HUGE_PAGE) {
        int rc = kp_host_reserve(bytes, out);
        if (rc == KP_OK && (rc = kp_host_lock(*out)) == KP_OK) return KP_OK;
        if (*out) { pinned_free(*out); *out = nullptr; }  // (a host that will not register mapped memory: the runtime's own allocation)
    }
    const hipError_t e = pinned_alloc(out, std::max<size_t>(bytes, 1));
    if (e != hipSuccess) return kp_fail(nullptr, KP_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return KP_OK;
}

int kp_host_reserve(size_t bytes, void **out) {
    if (!out) return kp_fail(nullptr, KP_EINVAL, "out is null");
    *out = mapped_alloc(std::max<size_t>(bytes, 1));
    if (!*out) return kp_fail(nullptr, KP_ENOMEM, "mmap failed");
    return KP_OK;
}

int kp_host_lock(void *p) {
    const hipError_t e = mapped_lock(p);
    if (e == hipErrorInvalidValue) return kp_fail(nullptr, KP_EINVAL, "not a block of kp_host_reserve");
    if (e != hipSuccess) return kp_fail(nullptr, KP_ENOMEM, std::string("hipHostRegister: ") + hipGetErrorString(e));
    return KP_OK;
}

void kp_host_free(void *p) { pinned_free(p); }

int64_t kp_device_allocations(void) { return (int64_t)g_dev_allocs.load(std::memory_order_relaxed); }

int64_t kp_host_pinned_bytes(void) {
    std::lock_guard<std::mutex> lk(g_pin_mutex);
    return (int64_t)g_pin_bytes;
}

}  // extern "C"

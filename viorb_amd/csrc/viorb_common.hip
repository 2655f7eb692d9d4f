// viorb_amd/csrc/viorb_common.hip — the host-side runtime behind viorb_common.h and the C-ABI functions that belong to no feature:
// last error, device count, ABI version, device-to-device copy and the kernel profiler. No device code.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <mutex>
#include <string>
#include <vector>
#include "viorb_common.h"
#include "match_core.h"             // GRID_CELLS

namespace viorb {

static thread_local char g_err[512] = "";
char* last_error_buf() { return g_err; }
void set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}

int require_device() {
    if (viorb_device_count() >= 1) return VIORB_OK;
    set_error("no HIP device: libviorb_hip has no CPU fallback");
    return VIORB_ERR_NO_DEVICE;
}

// ---- kernel profiler (process-wide, single-threaded use) ----------------------------------------
namespace {
struct ProfRec { hipEvent_t a, b; int slot; };
struct Profiler {
    bool enabled = false;
    std::string only;                 // when not empty: only these kernels (comma-separated) are timed (an event pair costs ~8 us of stream time)
    std::vector<std::string> names;
    std::vector<ProfRec> recs;
    size_t used = 0;
} g_prof;
}
ProfScope::ProfScope(const char* name, hipStream_t s) : idx(-1), st(s) {
    if (!g_prof.enabled || !name) return;
    if (!g_prof.only.empty()) {                  // comma-separated list of kernel names
        const std::string key = "," + g_prof.only + ",", me = std::string(",") + name + ",";
        if (key.find(me) == std::string::npos) return;
    }
    if (g_prof.used >= g_prof.recs.size()) {
        if (g_prof.recs.size() >= 16384) return;
        ProfRec r; r.slot = -1;
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
        g_prof.recs.push_back(r);
    }
    int slot = -1;
    for (size_t i = 0; i < g_prof.names.size(); i++) if (g_prof.names[i] == name) slot = (int)i;
    if (slot < 0) { g_prof.names.push_back(name); slot = (int)g_prof.names.size() - 1; }
    idx = (int)g_prof.used++;
    g_prof.recs[idx].slot = slot;
    (void)hipEventRecord(g_prof.recs[idx].a, st);
}
bool prof_times_everything() { return g_prof.only.empty(); }
ProfScope::~ProfScope() { if (idx >= 0) (void)hipEventRecord(g_prof.recs[idx].b, st); }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the function object of the CURRENT device, so the cache is keyed by
// (device, kernel): a handle on a second device of the same process raises the limit there too. Lock-free fast path for the callers
// inside solver loops: a per-thread memo of the last (device, kernel, bytes) that succeeded.
hipError_t raise_dynamic_lds(const void* kernel, size_t bytes) {
    int dev = 0;
    hipError_t rc = hipGetDevice(&dev);
    if (rc != hipSuccess) return rc;
    struct Memo { int dev; const void* k; size_t bytes; };
    static thread_local Memo memo[4] = {{-1, nullptr, 0}, {-1, nullptr, 0}, {-1, nullptr, 0}, {-1, nullptr, 0}};
    for (const Memo& m : memo) if (m.dev == dev && m.k == kernel && bytes <= m.bytes) return hipSuccess;
    static std::mutex mu;
    struct Seen { int dev; const void* k; size_t bytes; };
    static std::vector<Seen> seen;
    std::lock_guard<std::mutex> lk(mu);
    Seen* hit = nullptr;
    for (auto& e : seen) if (e.dev == dev && e.k == kernel) hit = &e;
    if (!hit || bytes > hit->bytes) {
        rc = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (rc != hipSuccess) return rc;
        if (hit) hit->bytes = bytes; else { seen.push_back({dev, kernel, bytes}); hit = &seen.back(); }
    }
    static thread_local int next = 0;
    memo[next] = {dev, kernel, hit->bytes}; next = (next + 1) & 3;
    return hipSuccess;
}

// ---- the pool of stream contexts -------------------------------------------------------------------
namespace {
std::mutex g_ctx_mu;
std::vector<StreamCtx*> g_ctx_free;
}
StreamCtxLease::~StreamCtxLease() { if (c) { std::lock_guard<std::mutex> lk(g_ctx_mu); g_ctx_free.push_back(c); } }
bool StreamCtxLease::ready() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (!c) {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        for (size_t i = 0; i < g_ctx_free.size(); i++)
            if (g_ctx_free[i]->device == dev) { c = g_ctx_free[i]; g_ctx_free.erase(g_ctx_free.begin() + i); break; }
    }
    if (!c) {
        c = new StreamCtx();
        c->device = dev;
        if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess || hipHostMalloc(reinterpret_cast<void**>(&c->pinned), 64 * sizeof(double)) != hipSuccess) {
            delete c; c = nullptr; return false;
        }
    }
    return true;
}

int host_keyframe(DeviceBufs& B, const viorb_keypoint* kps, const uint8_t* desc, int n, int cap, const float* bounds4, viorb_s3m_keyframes& kf) {
    const size_t c = (size_t)cap;
    kf.cap = cap;
    kf.kps = B.up(kps, (size_t)n, c); kf.desc = B.up(desc, (size_t)n * 32, c * 32); kf.count = B.up(&n, 1);
    int32_t* cs = B.zeros<int32_t>(GRID_CELLS + 1); int32_t* ci = B.zeros<int32_t>(c);
    kf.cell_start = cs; kf.cell_idx = ci;
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    return viorb_keyframe_grid_device(kf.kps, kf.count, kf.cap, 1, bounds4, cs, ci, nullptr);
}

} // namespace viorb

using namespace viorb;

extern "C" {

int viorb_abi_version(void) { return 2; }   // 2: viorb_frontend_config.dist_coef

const char* viorb_last_error(void) { return viorb::last_error_buf(); }
int viorb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int viorb_memcpy_dtod_async(void* dst, const void* src, size_t bytes, void* stream) {
    VIORB_REQUIRE(dst && src, "null pointer");
    VIORB_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VIORB_OK;
}

int viorb_profile_enable(int on) {
    g_prof.enabled = on != 0;
    return VIORB_OK;
}
int viorb_profile_reset(void) {
    g_prof.used = 0;
    return VIORB_OK;
}
int viorb_profile_select(const char* kernel_name) {
    g_prof.only = kernel_name ? kernel_name : "";
    return VIORB_OK;
}
// Synchronises the device and sums the recorded intervals per kernel name. names_buf receives the
// names separated by '\n'.
int viorb_profile_read(char* names_buf, int names_cap, double* total_ms, int* calls, int cap, int* n) {
    VIORB_REQUIRE(names_buf && total_ms && calls && n, "null argument");
    VIORB_HIP_TRY(hipDeviceSynchronize());
    const int k = (int)g_prof.names.size();
    *n = k;
    std::string all;
    for (int i = 0; i < k; i++) { all += g_prof.names[i]; all += '\n'; }
    snprintf(names_buf, names_cap, "%s", all.c_str());
    for (int i = 0; i < k && i < cap; i++) { total_ms[i] = 0; calls[i] = 0; }
    for (size_t r = 0; r < g_prof.used; r++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, g_prof.recs[r].a, g_prof.recs[r].b) != hipSuccess) continue;
        const int slot = g_prof.recs[r].slot;
        if (slot >= 0 && slot < cap) { total_ms[slot] += ms; calls[slot]++; }
    }
    return VIORB_OK;
}
// Start / end of every recorded interval in milliseconds since the first record (the records of both streams share one clock),
// in recording order; slot[i] indexes the names of viorb_profile_read. A timeline without a tracer's per-launch host cost.
int viorb_profile_timeline(double* start_ms, double* end_ms, int* slot, int cap, int* n) {
    VIORB_REQUIRE(start_ms && end_ms && slot && n, "null argument");
    VIORB_HIP_TRY(hipDeviceSynchronize());
    *n = (int)g_prof.used;
    for (size_t r = 0; r < g_prof.used && (int)r < cap; r++) {
        float a = 0, b = 0;
        (void)hipEventElapsedTime(&a, g_prof.recs[0].a, g_prof.recs[r].a);
        (void)hipEventElapsedTime(&b, g_prof.recs[0].a, g_prof.recs[r].b);
        start_ms[r] = a; end_ms[r] = b; slot[r] = g_prof.recs[r].slot;
    }
    return VIORB_OK;
}

} // extern "C"

// viorb_amd/csrc/viorb_common.h — the host-side runtime shared by the C-ABI translation units: error plumbing, the device check, the
// kernel profiler and the timed launch, per-call device buffers, workspace layout and the pool of stream contexts (viorb_common.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/viorb.h"

namespace viorb {

// thread-local last-error text (viorb_last_error())
char* last_error_buf();
void set_error(const char* fmt, ...);

// VIORB_OK, or VIORB_ERR_NO_DEVICE with its text: the library has no CPU fallback. Entry points call it after their argument checks.
int require_device();

// Optional per-kernel timing with HIP events recorded on the stream the kernel is launched on
// (viorb_profile_* in include/viorb.h); used by bench.py for the roofline line. Off by default.
struct ProfScope {
    int idx;
    hipStream_t st;
    ProfScope(const char* name, hipStream_t s);
    ~ProfScope();
};
bool prof_times_everything();          // no kernel selection (viorb_profile_select(NULL)): every launch is timed

// hipFuncAttributeMaxDynamicSharedMemorySize is a process-wide, per-kernel setting: every handle asks for its own size, so the limit is
// only ever raised (a later, smaller handle must not lower it under a long-lived one's launches).
hipError_t raise_dynamic_lds(const void* kernel, size_t bytes);

// The device allocations of one call (the host-buffer form of an entry point) or of one handle: freed by the destructor or by release().
struct DeviceBufs {
    std::vector<void*> ptrs;
    bool ok = true;                    // sticky: after the first failure every later up() returns nullptr
    DeviceBufs() {}
    DeviceBufs(const DeviceBufs&) = delete;
    DeviceBufs& operator=(const DeviceBufs&) = delete;
    ~DeviceBufs() { release(); }
    void release() { for (void* p : ptrs) (void)hipFree(p); ptrs.clear(); }
    // max(n_alloc, n_src, 1) zeroed elements, the first n_src of them copied from src
    template <class T> T* up(const T* src, size_t n_src, size_t n_alloc = 0) {
        T* d = nullptr;
        n_alloc = std::max<size_t>(std::max(n_alloc, n_src), 1);
        if (!ok || hipMalloc((void**)&d, n_alloc * sizeof(T)) != hipSuccess) { ok = false; return nullptr; }
        ptrs.push_back(d);
        if (hipMemset(d, 0, n_alloc * sizeof(T)) != hipSuccess) ok = false;
        if (ok && src && n_src && hipMemcpy(d, src, n_src * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) ok = false;
        return d;
    }
    template <class T> T* zeros(size_t n) { return up<T>(nullptr, 0, n); }
};

// Lays arrays out in a workspace, each at a multiple of 256 bytes. base == nullptr: a size query (the pointers are offsets from 0).
struct WorkspaceLayout {
    size_t off = 0;
    uint8_t* base;
    explicit WorkspaceLayout(void* b) : base(static_cast<uint8_t*>(b)) {}
    template <class T> void take(T** p, size_t n) { off = end(); if (p) *p = reinterpret_cast<T*>(base + off); off += (n ? n : 1) * sizeof(T); }
    size_t end() const { return (off + 255) & ~(size_t)255; }      // the bytes laid out so far, rounded up to the next array's start
};

// A solve borrows a context (a HIP stream, a device arena, page-locked scalars) from one pool of the process, so that concurrent callers
// run on different streams and no call pays hipMalloc / hipFree (which synchronise the whole device) once its arena has grown. The pool
// owns the stream and `pinned`; when and by how much `arena` and `stage` grow is the borrower's business.
struct StreamCtx {
    hipStream_t st = nullptr; void* arena = nullptr; size_t bytes = 0;
    double* pinned = nullptr;           // 64 doubles of page-locked host memory
    uint8_t* stage = nullptr; size_t stage_bytes = 0;       // page-locked staging buffer (lives until the context's next borrower replaces it)
    int device = 0;
};
struct StreamCtxLease {
    StreamCtx* c = nullptr;
    StreamCtxLease() {}
    StreamCtxLease(const StreamCtxLease&) = delete;
    StreamCtxLease& operator=(const StreamCtxLease&) = delete;
    ~StreamCtxLease();                  // gives the context back; it does not wait for the stream
    bool ready();                       // a free context of the calling thread's current device, or a new one
};

// The device side of a host-form key frame: its arrays with `cap` >= max(n, 1) entries and its grid (viorb_keyframe_grid_device).
int host_keyframe(DeviceBufs& B, const viorb_keypoint* kps, const uint8_t* desc, int n, int cap, const float* bounds4, viorb_s3m_keyframes& kf);

} // namespace viorb

#define VIORB_HIP_TRY(expr)                                                                   \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            viorb::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                             __LINE__);                                                       \
            return VIORB_ERR_HIP;                                                             \
        }                                                                                     \
    } while (0)

#define VIORB_REQUIRE(cond, msg)                      \
    do {                                              \
        if (!(cond)) {                                \
            viorb::set_error("invalid argument: %s", msg); \
            return VIORB_ERR_INVALID_ARG;             \
        }                                             \
    } while (0)

// A caller's workspace: non-null, 256-byte aligned, at least `need` bytes, where `sizer` names the entry point that returns `need`
#define VIORB_REQUIRE_WORKSPACE(ws, bytes, need, sizer) \
    VIORB_REQUIRE((ws) && ((uintptr_t)(ws) & 255) == 0 && (bytes) >= (need), "workspace smaller than " sizer " or not 256-byte aligned")

// returns the status of x unless it is VIORB_OK
#define VIORB_TRY(x) do { int _rc = (x); if (_rc != VIORB_OK) return _rc; } while (0)

// A launch timed under the kernel's own name. grid / block: a dim3 or a count.
#define VIORB_LAUNCH(kernel, grid, block, lds, stream, ...)                                  \
    do {                                                                                      \
        {                                                                                     \
            viorb::ProfScope _ps(#kernel, stream);                                            \
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, stream, __VA_ARGS__);    \
        }                                                                                     \
        VIORB_HIP_TRY(hipGetLastError());                                                     \
    } while (0)

namespace viorb {

// n elements of a device array to the host form's output; a NULL output or n == 0 copies nothing
template <class T> int download(T* host, const T* dev, size_t n) {
    if (host && n) VIORB_HIP_TRY(hipMemcpy(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost));
    return VIORB_OK;
}

} // namespace viorb

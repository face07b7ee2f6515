// acmmp_ctx.h — the engine object behind the opaque `acmmp_ctx *` of
// include/acmmp.h, shared by the translation units of libacmmp_amd.so
// (acmmp_engine.hip: PatchMatch runs; acmmp_planar.hip: planar-prior
// construction). Not installed, not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/acmmp.h"
#include "acmmp_internal.h"

using namespace acmmp;
struct acmmp_ctx;

namespace acmmp {

// Device blocks (acmmp_engine.hip). hipFree synchronises the whole device —
// with two engines in flight it waits for the other one's kernels — and
// costs about a millisecond per block, so blocks freed where their engine's
// stream has just been synchronised (dfree_synced; every free of
// acmmp_destroy) go to a per-(device, size) cache that later allocations of
// the same size take from. ACMMP_DEVICE_POOL_MB caps it (default 8192; 0
// turns it off). Any other free goes to hipFree, as before.
hipError_t dev_alloc(void **p, size_t bytes);
void dev_free(void *p, bool synced);
extern thread_local bool g_frees_synced;  // set by acmmp_destroy after its stream sync

template <typename T>
inline void dfree(T *&p) {
    if (p) dev_free((void *)p, g_frees_synced);
    p = nullptr;
}

// for a block no queued work can still touch (its stream just synchronised)
template <typename T>
inline void dfree_synced(T *&p) {
    if (p) dev_free((void *)p, true);
    p = nullptr;
}

template <typename T>
inline hipError_t dalloc(T *&p, size_t count) {
    dfree(p);
    return dev_alloc((void **)&p, count * sizeof(T) > 0 ? count * sizeof(T) : 4);
}

// Device memory that lives for one call: freed on every way out of the
// scope. The destructor is the plain free (after a failure queued work may
// still touch the block); a call that has just synchronised its stream hands
// the block to the cache with release_synced() instead.
template <typename T>
class Scratch {
    T *p_ = nullptr;

public:
    Scratch() = default;
    Scratch(Scratch &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }  // move-only: this deletes the copies
    ~Scratch() { dfree(p_); }
    hipError_t alloc(size_t count) { return dalloc(p_, count); }
    void release_synced() { dfree_synced(p_); }
    operator T *() const { return p_; }
};

// One view's image or depth map, row pitch `pitch` floats: owned (uploaded
// from the host, pitched) or borrowed (the caller's device pointer, zero copy).
struct ViewPlane {
    const float *p = nullptr;  // what the kernels read: own, or the caller's
    float *own = nullptr;
    int pitch = 0, w = 0, h = 0;
};

// One view's padded footprint records (KViews::pad).
struct PadRecords {
    float *own = nullptr;        // owned buffer, kept across problems and only ever grown
    size_t bytes = 0;            // bytes allocated at own
    const float *use = nullptr;  // what KViews::pad points at: own, or a texture's records
    int pitch = 0;               // records per row
};

}  // namespace acmmp

// acmmp_texture_create: one view's padded footprint records, built once and
// borrowed by any engine on the device (~ a CUDA texture object,
// src/ACMMP.cpp:640-662). The image itself stays the caller's.
struct acmmp_texture {
    int device = 0;
    ViewPlane img;   // borrowed
    int form = 0;    // kTexelF32 / kTexelU8 / kTexelH16
    PadRecords pad;  // pad.use == pad.own
};

// The row-major results between runs. The depth channel of the planes is
// also kept as its own plane (written by k_finalize and the filters: the
// filters read 4 B per neighbour instead of a float4, and the depth export is
// a plain copy), which matches the planes' .w only after a full run. Every
// writable pointer comes from write(), which drops that claim, so no writer
// of the planes can leave a stale depth plane to be exported.
class Results {
    float4 *d_rm_plane = nullptr;
    float *d_rm_cost = nullptr;
    float *d_rm_depth = nullptr;
    uint32_t *d_rm_sv = nullptr;
    bool depth_ok = false;

public:
    struct Writable {
        float4 *plane;
        float *cost, *depth;
        uint32_t *sv;
    };
    const float4 *planes() const { return d_rm_plane; }
    const float *costs() const { return d_rm_cost; }
    const uint32_t *sv() const { return d_rm_sv; }
    Writable write() {
        depth_ok = false;
        return {d_rm_plane, d_rm_cost, d_rm_depth, d_rm_sv};
    }
    // the depth plane now matches .w at every pixel: a full run's finalize
    // and both filters, over the whole image, are queued
    void depth_plane_complete() { depth_ok = true; }
    // where an export copies the depths from, stride bytes apart: the depth
    // plane, else the .w channel of the planes
    const float *depth_source(size_t &stride) const {
        stride = depth_ok ? sizeof(float) : sizeof(float4);
        return depth_ok ? d_rm_depth : (const float *)d_rm_plane + 3;
    }
    // P zero-filled pixels (pin: the reference's never-written host fields,
    // src/ACMMP.cpp:797-804), the fill queued on ctx's stream
    int alloc(acmmp_ctx *ctx, size_t P);
    void release() {
        dfree(d_rm_plane);
        dfree(d_rm_cost);
        dfree(d_rm_depth);
        dfree(d_rm_sv);
        depth_ok = false;
    }
};

struct acmmp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    acmmp_params prm{};
    std::string err;

    int n = 0;
    int W = 0, H = 0, Wh = 0;
    acmmp_camera cams[ACMMP_MAX_IMAGES]{};

    std::vector<ViewPlane> img, dep;  // per view; dep is filled iff have_depths
    bool have_depths = false;
    std::vector<PadRecords> pad;       // per view, of one common form:
    int pad_texel = 0;                 // KViews::texel, kTexel*
    uint32_t *d_not_u8 = nullptr;      // device flag: a view does not fit the compact form

    float4 *d_cplane[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [colour][pingpong]
    float *d_ccost[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    uint32_t *d_csv[2] = {nullptr, nullptr};
    int cur[2] = {0, 0};
    Results res;
    float *d_pre_cost = nullptr;
    float4 *d_prior = nullptr;
    uint32_t *d_mask = nullptr;
    float4 *d_scaled = nullptr;
    size_t scaled_count = 0;
    float4 *d_seed = nullptr;
    bool have_prior = false, have_scaled = false, have_seed = false, have_state = false;

    // Per-run constant block. A ring of pinned host / device slots so an
    // asynchronous run never has its constants overwritten by the next
    // enqueue: slot k is refilled only after its previous copy completed
    // (event), and the device copy is stream-ordered behind the kernels that
    // read it.
    static constexpr int kSlots = 4;
    KViews *d_kv_ring[kSlots] = {};
    KViews *h_kv_ring[kSlots] = {};
    hipEvent_t kv_ev[kSlots] = {};
    bool kv_used[kSlots] = {};
    int kv_slot = 0;
    KViews *d_kv = nullptr;  // slot of the current enqueue
    KViews h_kv{};

    bool timing = false;
    acmmp_timing last_timing{};
    hipEvent_t ev[8] = {};
    bool events_made = false;

    // acmmp_wait_stream: recorded on a producer stream, waited on by `stream`
    hipEvent_t wait_ev = nullptr;
};

namespace acmmp {

inline int set_err(acmmp_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

// ctx may be NULL (entry points without an engine): the status alone is returned
#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return set_err(ctx, ACMMP_ERR_HIP, "%s failed: %s (%s:%d)", #expr,               \
                           hipGetErrorString(e_), __FILE__, __LINE__);                       \
    } while (0)

inline int pitch_of(int w) { return (w + 63) / 64 * 64; }

inline int check_ready(acmmp_ctx *ctx) {
    if (!ctx) return ACMMP_ERR_ARG;
    if (ctx->n < 2) return set_err(ctx, ACMMP_ERR_STATE, "no images set (acmmp_set_images)");
    return ACMMP_OK;
}

}  // namespace acmmp

inline int Results::alloc(acmmp_ctx *ctx, size_t P) {
    release();
    HIP_TRY(ctx, dalloc(d_rm_plane, P));
    HIP_TRY(ctx, dalloc(d_rm_cost, P));
    HIP_TRY(ctx, dalloc(d_rm_depth, P));
    HIP_TRY(ctx, dalloc(d_rm_sv, P));
    HIP_TRY(ctx, hipMemsetAsync(d_rm_plane, 0, P * sizeof(float4), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_rm_cost, 0, P * sizeof(float), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_rm_depth, 0, P * sizeof(float), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_rm_sv, 0, P * sizeof(uint32_t), ctx->stream));
    return ACMMP_OK;
}

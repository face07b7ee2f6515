// acmmp_fusion_dev.hip — fusion in Jacobi order on the device: one rule for a view, three carriers.
//
// The rule. The literal fusions (acmmp_fusion.cpp) walk a view's pixels one after the other because
// an approval masks source pixels that later pixels of the SAME view then skip. Here every pixel of
// view i reads the masks as they stood before view i's first pixel (its own mask bit and every
// source's, also when a view lists itself as a source); view i's mask writes become visible to view
// i + 1. Nothing else changes: view order, pixel order, the thresholds, the float expressions
// (world_point / project of acmmp_fusion_host.h, shared with the host). A view is then four
// data-parallel launches on one stream (enqueue_view):
//   test     a thread a pixel: per source slot the reference's tests against the masks
//            as they stand (nothing writes them meanwhile); out: the pixel's 32-bit hit mask (bit j
//            = source slot j passed) and its flag byte (approved, and what the carrier adds)
//   chunks   per chunk of kScanChunk pixels and slot: the chunk's last hit; per chunk: its approvals.
//   carry    Then across chunks: the last hit before each chunk per slot, and the exclusive prefix
//            of the approvals (the points' positions)
//   apply    its own launch after the test (fused, one pixel's write could reach another pixel's
//            test of the same view), a block a chunk: an approved pixel writes its point at its
//            position and sets mask bits of source pixels. Targets are not stored: recomputed by
//            the expression the test used. Atomic ORs of single bits: any thread order is the same.
// libm: acos / exp are the project's pinned dm_acosf / dm_expf (the literal fusions call the
// host's libm): same bits on host, device and in the tests' restatements. dm_acosf is NaN outside
// [-1, 1], so GetAngle's "NaN -> 0" gives angle 0 for a dot product just above 1.
// int(p + 0.5f): the host's conversion of a NaN, an infinity or a value outside int is INT_MIN,
// which the bounds test rejects; the device's saturates (NaN -> 0, in bounds). pixel_coord tests the
// range before converting: not finite or outside [-2^31, 2^31) is out of bounds.
//
// The carriers, and what each differs in:
//   acmmp_run_fusion_jacobi (RunFusion, src/acmmp_definitions.cpp:828-1043): k_fusion_test, and
//     k_fusion_apply<false>, which per slot sets the mask bit of the target of the last hit at or
//     before the approved pixel. That is used_list, which the reference never resets between
//     pixels: an unapproved pixel's hit is applied by the next approval unless a later hit on the
//     same slot replaced it.
//   acmmp_run_prior_aware_fusion_jacobi (RunPriorAwareFusion, :573-826): k_prior_test, both
//     hypotheses (0 = fusion_folder's maps, 1 = output_folder's, this run's priors) against both
//     maps of every source and the choice (:754-789); the hit mask is the chosen hypothesis's, the
//     flag byte and bit 31 of the point's pixel index name it. No used_list (declared at :679, never
//     used): in k_prior_apply an approved pixel masks the targets of its own hits (:814-818) and
//     nothing else, so the last-hit rows of chunks / carry are not read.
//   Both are folder calls (fuse_on_device): one upload of every view's maps, a stream of its own,
//     view i's 16-byte points copied back and collected (normal, colour: the host's) while view
//     i + 1's kernels run.
//   acmmp_fuse_views_jacobi (fuse_views_on_device): RunFusion's rule over views that already lie in
//     device memory: depth and normal read through strides (a float4 planes tensor serves as both),
//     byte masks packed by k_mask_pack, and k_fusion_apply<true>, which writes whole points (xyz,
//     normal, r g b) into the caller's arrays at the running total k_fusion_carry keeps on the
//     device + the position in the view, below the arrays' capacity. All on the caller's stream, no
//     wait between views, one at the end for the count.
#include <hip/hip_runtime.h>

#include "acmmp_fusion_host.h"
#include "../../include/acmmp_detmath.h"

namespace {

using namespace acmmp_fusion_host;

constexpr int kScanChunk = 1024;  // pixels a scan chunk = threads of an apply block
constexpr int kMaxSrc = 32;       // source slots: bits of a hit mask
constexpr int kCarrySeg = 16;     // k_fusion_carry: segments of chunks a row is scanned in

struct DevView {
    acmmp_camera cam;      // at the maps' size
    int W, H, nsrc;
    int src[kMaxSrc];      // [slot j]: the source's view index
    const float *depth;    // pixel q's depth at depth[q * dstride]
    const float *normal;   // ... its normal at normal[q * nstride + 0..2]
    long long dstride, nstride;  // the folder calls' maps: 1 and 3; float4 planes: 4 and 4
    const float *pdepth;   // the prior-aware fusion's second pair (this run's priors), else null
    const float *pnormal;  // (H x W and H x W x 3, no strides)
    const uint8_t *bgr;    // H x W x 3, the in-memory fusion's colours (null: 0, 0, 0); else unused
    uint32_t *mask;        // bit k & 31 of word k >> 5 (MaskBits' 64-bit words, little-endian)
};

__device__ inline float depth_at(const DevView &v, int q) { return v.depth[(long long)q * v.dstride]; }
__device__ inline const float *normal_at(const DevView &v, int q) { return v.normal + (long long)q * v.nstride; }

// where the in-memory fusion's apply step writes whole points (acmmp_cloud_buffers), and the running
// total k_fusion_carry keeps: total[0] = the points of the views before this one (this view's
// output base), total[1] = with this view's
struct DevCloud {
    float *xyz, *normal;
    uint8_t *rgb;
    long long capacity;
    const long long *total;
};

// an approved pixel: its world point and pixel index (normal, colour: the host's); bit 31 of q: the
// point is the prior-aware fusion's hypothesis 1 (pixel indices fit in 27 bits)
struct DevPoint {
    float x, y, z;
    uint32_t q;
};

// a pixel's flag byte, what a test kernel writes and the scan and apply kernels read: k_fusion_test
// writes 0 or kFlagApproved, k_prior_test also the hypothesis it chose
constexpr int kFlagApproved = 1;  // bit 0
constexpr int kFlagPickShift = 1; // bit 1: the prior-aware fusion's chosen hypothesis

__device__ inline bool mask_bit(const uint32_t *m, int k) { return (m[k >> 5] >> (k & 31)) & 1u; }

// int(p + 0.5f) inside [0, n), with the host's outcome for what int() cannot hold (see the top)
__device__ inline bool pixel_coord(float p, int n, int &out) {
    const float v = p + 0.5f;
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return false;  // NaN, +-inf, outside int
    out = (int)v;
    return out >= 0 && out < n;
}

// the pixel of source `vs` that world point X falls on; false: outside the source's maps
__device__ inline bool src_pixel(const F3 &X, const DevView &vs, int &sc, int &sr) {
    float px, py, proj_depth;
    project(X, vs.cam, px, py, proj_depth);
    const bool in_r = pixel_coord(py, vs.H, sr), in_c = pixel_coord(px, vs.W, sc);
    return in_r && in_c;
}

__device__ inline float get_angle(const float *a, const float *b) {  // GetAngle
    const float dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    const float angle = dm_acosf(dot);
    if (angle != angle) return 0.0f;
    return angle;
}

__global__ void __launch_bounds__(256)
k_fusion_test(const DevView *__restrict__ views, int i, int con_num_thresh, float consistency_scalar,
              uint32_t *__restrict__ hit, uint8_t *__restrict__ approved) {
    const DevView &vi = views[i];
    const int N = vi.W * vi.H;
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (q >= N) return;
    uint32_t hits = 0;
    bool ok = false;
    const float ref_depth = depth_at(vi, q);
    if (!mask_bit(vi.mask, q) && !(ref_depth <= 0.0f || ref_depth >= vi.cam.depth_max)) {
        const int r = q / vi.W, c = q - r * vi.W;
        const F3 X = world_point(c, r, ref_depth, vi.cam);
        int num_consistent = 0;
        float dynamic_consistency = 0;
        for (int j = 0; j < vi.nsrc; ++j) {
            const DevView &vs = views[vi.src[j]];
            int sc, sr;
            if (!src_pixel(X, vs, sc, sr)) continue;
            const int sp = sr * vs.W + sc;
            if (mask_bit(vs.mask, sp)) continue;
            const float src_depth = depth_at(vs, sp);
            if (src_depth <= 0.0f) continue;
            const F3 tmp_X = world_point(sc, sr, src_depth, vs.cam);
            float tx, ty, proj_depth;
            project(tmp_X, vi.cam, tx, ty, proj_depth);
            // as stage_reproject (acmmp_fusion.cpp): std::pow(v, 2) of a float is exact in double
            const double dx = (double)(c - tx), dy = (double)(r - ty);
            const float reproj_error = (float)sqrt(dx * dx + dy * dy);
            const float relative_depth_diff = fabsf(proj_depth - ref_depth) / ref_depth;
            if (!(reproj_error < 2.0f && relative_depth_diff < 0.01f)) continue;
            const float angle = get_angle(normal_at(vi, q), normal_at(vs, sp));
            if (angle < 0.174533f) {
                const float tmp_index = reproj_error + 200 * relative_depth_diff + angle * 10;
                hits |= 1u << j;
                dynamic_consistency += dm_expf(-tmp_index);
                num_consistent++;
            }
        }
        ok = num_consistent >= con_num_thresh && (dynamic_consistency > consistency_scalar * num_consistent);
    }
    hit[q] = hits;
    approved[q] = ok ? kFlagApproved : 0;
}

// 32 threads a chunk: thread j finds the chunk's last hit on slot j (-1: none; walks back from the
// chunk's end, so it stops early where hits are dense), and together they count its approvals.
__global__ void __launch_bounds__(256)
k_fusion_chunks(const uint32_t *__restrict__ hit, const uint8_t *__restrict__ approved, int N, int nchunks,
                int *__restrict__ chunk_last, int *__restrict__ chunk_count) {
    const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int chunk = t >> 5, j = t & 31;
    if (chunk >= nchunks) return;  // (all 32 threads of a chunk leave together)
    const int b = chunk * kScanChunk, e = min(N, b + kScanChunk);
    int last = -1;
    for (int p = e - 1; p >= b; --p)
        if ((hit[p] >> j) & 1u) {
            last = p;
            break;
        }
    chunk_last[chunk * kMaxSrc + j] = last;
    int cnt = 0;
    for (int p = b + j; p < e; p += 32) cnt += approved[p] & kFlagApproved;
    for (int o = 16; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 32);
    if (j == 0) chunk_count[chunk] = cnt;
}

// One block. Rows 0..31: per slot the exclusive running maximum of chunk_last over the chunks (the
// last hit before the chunk; pixel indices grow with the chunk, -1 = none). Row 32: the exclusive
// prefix sum of chunk_count, and the view's number of points (to view_points and / or added to the
// running total, either may be null). A row is scanned in kCarrySeg
// segments: each thread reduces its segment, then rescans it from what the segments before it hold.
constexpr int kCarryThreads = (kMaxSrc + 1) * kCarrySeg;

__global__ void __launch_bounds__(576)
k_fusion_carry(int nchunks, const int *__restrict__ chunk_last, const int *__restrict__ chunk_count,
               int *__restrict__ carry_last, int *__restrict__ chunk_base, int *__restrict__ view_points,
               long long *__restrict__ total) {
    __shared__ int seg_val[kMaxSrc + 1][kCarrySeg];
    const int tid = (int)threadIdx.x;
    const bool active = tid < kCarryThreads, counts = tid >= kMaxSrc * kCarrySeg;
    const int row = counts ? kMaxSrc : tid & (kMaxSrc - 1);
    const int seg = counts ? tid - kMaxSrc * kCarrySeg : tid >> 5;
    const int per = (nchunks + kCarrySeg - 1) / kCarrySeg;
    const int b = min(nchunks, seg * per), e = min(nchunks, b + per);
    if (active) {
        int acc = counts ? 0 : -1;
        for (int c = b; c < e; ++c) acc = counts ? acc + chunk_count[c] : max(acc, chunk_last[c * kMaxSrc + row]);
        seg_val[row][seg] = acc;
    }
    __syncthreads();
    if (!active) return;
    int run = counts ? 0 : -1;
    for (int s = 0; s < seg; ++s) run = counts ? run + seg_val[row][s] : max(run, seg_val[row][s]);
    for (int c = b; c < e; ++c) {
        if (counts) {
            chunk_base[c] = run;
            run += chunk_count[c];
        } else {
            carry_last[c * kMaxSrc + row] = run;
            run = max(run, chunk_last[c * kMaxSrc + row]);
        }
    }
    if (counts && seg == kCarrySeg - 1) {  // (the last segment ends at nchunks)
        if (view_points) *view_points = run;  // the folder calls: the host places the view's points
        if (total) {  // the in-memory fusion: the view's base is the total so far, which stays on the device
            const long long before = total[1];
            total[0] = before;
            total[1] = before + run;
        }
    }
}

// sets the mask bit of the pixel of source slot j that pixel p of view i falls on
__device__ inline void set_target(const DevView *views, const DevView &vi, int p, int j) {
    const int r = p / vi.W, c = p - r * vi.W;
    const F3 X = world_point(c, r, depth_at(vi, p), vi.cam);
    const DevView &vs = views[vi.src[j]];
    int sc, sr;
    if (!src_pixel(X, vs, sc, sr)) return;  // (a hit passed this very test in k_fusion_test)
    const int sp = sr * vs.W + sc;
    atomicOr(&vs.mask[sp >> 5], 1u << (sp & 31));
}

// kCloud: the in-memory fusion's apply step. The approved pixel writes its whole point (world point,
// its normal through the stride, its colour as r, g, b) into the caller's arrays at the running
// total + its position in the view, if that lies below the capacity: no byte of a point at or
// beyond it is written. The mask updates do not depend on the capacity. `out` is then unused.
template <bool kCloud>
__global__ void __launch_bounds__(kScanChunk)
k_fusion_apply(const DevView *__restrict__ views, int i, const uint32_t *__restrict__ hit,
               const uint8_t *__restrict__ approved, const int *__restrict__ chunk_last,
               const int *__restrict__ carry_last, const int *__restrict__ chunk_base, DevPoint *__restrict__ out,
               DevCloud cloud) {
    __shared__ uint32_t s_hit[kScanChunk];
    __shared__ int s_wave[kScanChunk / 64];
    __shared__ uint32_t s_present;  // slots with a hit somewhere in this chunk
    const DevView &vi = views[i];
    const int N = vi.W * vi.H;
    const int chunk = (int)blockIdx.x, tid = (int)threadIdx.x, q = chunk * kScanChunk + tid;
    const int lane = tid & 63, wave = tid >> 6;
    const bool ok = q < N && approved[q];
    s_hit[tid] = q < N ? hit[q] : 0u;
    const unsigned long long votes = __ballot(ok);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    if (wave == 0) {
        const unsigned long long present = __ballot(lane < kMaxSrc && chunk_last[chunk * kMaxSrc + (lane & 31)] >= 0);
        if (lane == 0) s_present = (uint32_t)present;
    }
    __syncthreads();
    if (!ok) return;
    int pos = chunk_base[chunk] + __popcll(votes & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += s_wave[w];
    const int r = q / vi.W, c = q - r * vi.W;
    const F3 X = world_point(c, r, depth_at(vi, q), vi.cam);
    if constexpr (kCloud) {
        const long long at = cloud.total[0] + pos;
        if (at < cloud.capacity) {
            const float *nrm = normal_at(vi, q);
            float *xyz = cloud.xyz + at * 3, *normal = cloud.normal + at * 3;
            uint8_t *rgb = cloud.rgb + at * 3;
            xyz[0] = X.x, xyz[1] = X.y, xyz[2] = X.z;
            normal[0] = nrm[0], normal[1] = nrm[1], normal[2] = nrm[2];
            const uint8_t *px = vi.bgr ? vi.bgr + (size_t)q * 3 : nullptr;
            rgb[0] = px ? px[2] : 0, rgb[1] = px ? px[1] : 0, rgb[2] = px ? px[0] : 0;
        }
    } else {
        out[pos] = DevPoint{X.x, X.y, X.z, (uint32_t)q};
    }
    const uint32_t slots = vi.nsrc >= kMaxSrc ? 0xffffffffu : (1u << vi.nsrc) - 1u;
    uint32_t need = slots & s_present;
    for (int p = tid; need && p >= 0; --p) {  // back to the chunk's start: the last hit per slot
        uint32_t h = s_hit[p] & need;
        need &= ~h;
        for (; h; h &= h - 1) set_target(views, vi, chunk * kScanChunk + p, __ffs((int)h) - 1);
    }
    for (uint32_t rest = (slots & ~s_present) | need; rest; rest &= rest - 1) {  // from earlier chunks
        const int j = __ffs((int)rest) - 1;
        const int p = carry_last[chunk * kMaxSrc + j];
        if (p >= 0) set_target(views, vi, p, j);
    }
}

// The in-memory fusion's initial mask: a view's N mask bytes (nonzero = masked) packed into its mask
// words, one ballot per 64 pixels (wave w of the grid holds pixels 64 w .. 64 w + 63 = words 2 w and
// 2 w + 1). N need be no multiple of 32 or 64: the bits past N are 0, and the words are allocated in
// pairs (MaskBits' 64-bit words), so a wave that holds a pixel writes both of its words in bounds.
__global__ void __launch_bounds__(256)
k_mask_pack(const uint8_t *__restrict__ bytes, int N, uint32_t *__restrict__ words) {
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const unsigned long long bits = __ballot(q < N && bytes[q] != 0);
    if ((threadIdx.x & 63) == 0 && q < N) {
        words[q >> 5] = (uint32_t)bits;
        words[(q >> 5) + 1] = (uint32_t)(bits >> 32);
    }
}

// ---- RunPriorAwareFusion (its kernels read a view's depth / normal as the folder calls lay them
// out, strides 1 and 3: fuse_on_device is their only caller)

// metric_of + the thresholds of get_consistency_metrics (:443-516) for one of a source's two maps:
// whether it passes, and then exp(-index) in dc (exp's value is used nowhere else)
__device__ inline bool prior_metric(const DevView &vi, int r, int c, float ref_depth, const float *ref_normal,
                                    const DevView &vs, int sr, int sc, float src_depth, const float *src_normal,
                                    float &dc) {
    if (!(src_depth > 0.0f)) return false;  // (all three metrics 1e6)
    const F3 tmp_X = world_point(sc, sr, src_depth, vs.cam);
    float tx, ty, proj_depth;
    project(tmp_X, vi.cam, tx, ty, proj_depth);
    const double dx = (double)(c - tx), dy = (double)(r - ty);
    const float reproj_err = (float)sqrt(dx * dx + dy * dy);
    const float relative_depth_diff = fabsf(proj_depth - ref_depth) / ref_depth;
    if (!(reproj_err < 2.0f && relative_depth_diff < 0.01f)) return false;
    const float angle = get_angle(ref_normal, src_normal);
    if (!(angle < 0.174533f)) return false;
    dc = dm_expf(-(reproj_err + 200 * relative_depth_diff + angle * 10));
    return true;
}

__global__ void __launch_bounds__(256)
k_prior_test(const DevView *__restrict__ views, int i, int num_consistent_thresh, int single_match_penalty,
             float consistency_scalar, uint32_t *__restrict__ hit, uint8_t *__restrict__ flag) {
    const DevView &vi = views[i];
    const int N = vi.W * vi.H;
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (q >= N) return;
    uint32_t hits[2] = {0, 0};
    int pick = 0;
    bool passing = false;
    const float ref_depth[2] = {vi.depth[q], vi.pdepth[q]};
    if (!mask_bit(vi.mask, q) && !(ref_depth[0] <= 0.0f && ref_depth[1] <= 0.0f)) {
        const int r = q / vi.W, c = q - r * vi.W;
        int nb[2] = {0, 0};
        bool t[2] = {false, false};
        for (int b = 0; b < 2; ++b) {
            if (!(ref_depth[b] > 0.0f)) continue;
            const float *ref_normal = (b ? vi.pnormal : vi.normal) + (size_t)q * 3;
            const F3 X = world_point(c, r, ref_depth[b], vi.cam);
            float d_cons = 0;
            for (int j = 0; j < vi.nsrc; ++j) {  // getCandidates (:520-571)
                const DevView &vs = views[vi.src[j]];
                int sc, sr;
                if (!src_pixel(X, vs, sc, sr)) continue;
                const int sp = sr * vs.W + sc;
                if (mask_bit(vs.mask, sp)) continue;
                float dc0 = 0, dc1 = 0;
                const bool t0 = prior_metric(vi, r, c, ref_depth[b], ref_normal, vs, sr, sc, vs.depth[sp],
                                             &vs.normal[(size_t)sp * 3], dc0);
                const bool t1 = prior_metric(vi, r, c, ref_depth[b], ref_normal, vs, sr, sc, vs.pdepth[sp],
                                             &vs.pnormal[(size_t)sp * 3], dc1);
                if (!t0 && !t1) continue;
                hits[b] |= 1u << j;
                nb[b]++;
                d_cons += t0 && t1 ? fmaxf(dc0, dc1) : t0 ? dc0 : dc1;
            }
            t[b] = nb[b] >= num_consistent_thresh && d_cons > consistency_scalar * nb[b];
        }
        if (t[0] && t[1]) {  // (:754-789)
            passing = true;
            pick = nb[1] >= nb[0] ? 1 : 0;
        } else if (t[1]) {
            passing = nb[1] >= num_consistent_thresh + single_match_penalty;
            pick = 1;
        } else {
            passing = t[0] && nb[0] >= num_consistent_thresh + single_match_penalty;
        }
    }
    hit[q] = passing ? hits[pick] : 0u;
    flag[q] = (uint8_t)((passing ? kFlagApproved : 0) | pick << kFlagPickShift);
}

__global__ void __launch_bounds__(kScanChunk)
k_prior_apply(const DevView *__restrict__ views, int i, const uint32_t *__restrict__ hit,
              const uint8_t *__restrict__ flag, const int *__restrict__ chunk_base, DevPoint *__restrict__ out) {
    __shared__ int s_wave[kScanChunk / 64];
    const DevView &vi = views[i];
    const int N = vi.W * vi.H;
    const int chunk = (int)blockIdx.x, tid = (int)threadIdx.x, q = chunk * kScanChunk + tid;
    const int lane = tid & 63, wave = tid >> 6;
    const int f = q < N ? flag[q] : 0;
    const bool ok = f & kFlagApproved;
    const unsigned long long votes = __ballot(ok);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    if (!ok) return;
    int pos = chunk_base[chunk] + __popcll(votes & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += s_wave[w];
    const int pick = f >> kFlagPickShift;
    const int r = q / vi.W, c = q - r * vi.W;
    const F3 X = world_point(c, r, pick ? vi.pdepth[q] : vi.depth[q], vi.cam);
    out[pos] = DevPoint{X.x, X.y, X.z, (uint32_t)q | (uint32_t)pick << 31};
    for (uint32_t h = hit[q]; h; h &= h - 1) {
        const DevView &vs = views[vi.src[__ffs((int)h) - 1]];
        int sc, sr;
        if (!src_pixel(X, vs, sc, sr)) continue;  // (a hit passed this very test in k_prior_test)
        const int sp = sr * vs.W + sc;
        atomicOr(&vs.mask[sp >> 5], 1u << (sp & 31));
    }
}

using Clock = std::chrono::steady_clock;
double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

#define FUSION_HIP_TRY(expr)                                                                               \
    do {                                                                                                   \
        const hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                              \
            return ffail(ACMMP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// What a call holds on the device and in pinned host memory, released on every way out: the stream
// drained, then the events, the memory, and the stream if it is the call's own. A caller's stream
// (borrowed: set `stream` and leave `owned`) is never destroyed, and waited for only while `pending`.
struct DevHold {
    std::vector<void *> dev, pinned;
    hipStream_t stream = nullptr;
    bool owned = false;    // created by own_stream
    bool pending = false;  // work is enqueued that the host has not waited for
    hipEvent_t copied[2] = {nullptr, nullptr};  // optional
    ~DevHold() {
        if (pending) (void)hipStreamSynchronize(stream);
        for (hipEvent_t e : copied)
            if (e) (void)hipEventDestroy(e);
        for (void *p : dev) (void)hipFree(p);
        for (void *p : pinned) (void)hipHostFree(p);
        if (owned) (void)hipStreamDestroy(stream);
    }
    hipError_t own_stream() {
        const hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        owned = pending = e == hipSuccess;  // (pending for good: every way out drains it)
        return e;
    }
    template <class T>
    hipError_t dev_alloc(T *&p, size_t count) {
        const hipError_t e = hipMalloc((void **)&p, std::max(count * sizeof(T), size_t(256)));
        if (e == hipSuccess) dev.push_back(p);
        return e;
    }
    template <class T>
    hipError_t pinned_alloc(T *&p, size_t count) {
        const hipError_t e = hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) pinned.push_back(p);
        return e;
    }
};

// what a view's launches hand to each other, sized for the call's largest view
struct ViewScratch {
    uint32_t *hit = nullptr;                            // [pixel]: its hit mask
    uint8_t *flag = nullptr;                            // [pixel]: its flag byte
    int *chunk_last = nullptr, *carry_last = nullptr;   // [chunk][slot]
    int *chunk_count = nullptr, *chunk_base = nullptr;  // [chunk]
};

int alloc_scratch(DevHold &hold, size_t max_pixels, ViewScratch &s) {
    const size_t max_chunks = (max_pixels + kScanChunk - 1) / kScanChunk;
    FUSION_HIP_TRY(hold.dev_alloc(s.hit, max_pixels));
    FUSION_HIP_TRY(hold.dev_alloc(s.flag, max_pixels));
    FUSION_HIP_TRY(hold.dev_alloc(s.chunk_last, max_chunks * kMaxSrc));
    FUSION_HIP_TRY(hold.dev_alloc(s.carry_last, max_chunks * kMaxSrc));
    FUSION_HIP_TRY(hold.dev_alloc(s.chunk_count, max_chunks));
    FUSION_HIP_TRY(hold.dev_alloc(s.chunk_base, max_chunks));
    return ACMMP_OK;
}

// a view's table entry but for what the carriers differ in: the pointers, strides, bgr and the
// prior pair (null here)
DevView dev_view(const acmmp_camera &cam, int W, int H, const int *src, int nsrc) {
    DevView v{cam, W, H, nsrc};  // (the other slots 0, the pointers null)
    for (int j = 0; j < nsrc; ++j) v.src[j] = src[j];
    return v;
}

// what the carriers' tests differ in
struct JacobiRule {
    bool prior;  // RunPriorAwareFusion's test and apply step, else RunFusion's
    float consistency_scalar;
    int num_consistent_thresh, single_match_penalty;
};

// View i's (N pixels) launches on the stream: test, chunks, carry, apply. The caller passes one of
// two pairs and leaves the other null / empty, and that picks the apply step: `out` (16-byte
// points) with `view_points` (the carry writes the view's count there): the folder calls,
// k_prior_apply if rule.prior, else k_fusion_apply<false>; or `cloud` (whole points) with `total`
// (the carry adds to the running total): the in-memory call, k_fusion_apply<true>, never with
// rule.prior. A view without pixels (the folder calls only) gets the carry alone: its count is 0.
void enqueue_view(hipStream_t stream, const DevView *d_views, int i, int N, const ViewScratch &s,
                  const JacobiRule &rule, DevPoint *out, const DevCloud &cloud, int *view_points, long long *total) {
    const int nchunks = (N + kScanChunk - 1) / kScanChunk;
    if (N > 0) {
        if (rule.prior)
            k_prior_test<<<(N + 255) / 256, 256, 0, stream>>>(d_views, i, rule.num_consistent_thresh,
                                                              rule.single_match_penalty, rule.consistency_scalar,
                                                              s.hit, s.flag);
        else
            k_fusion_test<<<(N + 255) / 256, 256, 0, stream>>>(d_views, i, rule.num_consistent_thresh,
                                                               rule.consistency_scalar, s.hit, s.flag);
        k_fusion_chunks<<<(nchunks * 32 + 255) / 256, 256, 0, stream>>>(s.hit, s.flag, N, nchunks, s.chunk_last,
                                                                        s.chunk_count);
    }
    k_fusion_carry<<<1, 576, 0, stream>>>(nchunks, s.chunk_last, s.chunk_count, s.carry_last, s.chunk_base,
                                          view_points, total);
    if (N <= 0) return;
    if (rule.prior)
        k_prior_apply<<<nchunks, kScanChunk, 0, stream>>>(d_views, i, s.hit, s.flag, s.chunk_base, out);
    else if (out)
        k_fusion_apply<false><<<nchunks, kScanChunk, 0, stream>>>(d_views, i, s.hit, s.flag, s.chunk_last,
                                                                  s.carry_last, s.chunk_base, out, DevCloud{});
    else
        k_fusion_apply<true><<<nchunks, kScanChunk, 0, stream>>>(d_views, i, s.hit, s.flag, s.chunk_last,
                                                                 s.carry_last, s.chunk_base, nullptr, cloud);
}

size_t align256(size_t n) { return (n + 255) / 256 * 256; }

// checked before any load: without a usable device nothing is launched and no file written
int need_device(const char *what, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
    if (device < 0 || device >= ndev)
        return ffail(ACMMP_ERR_HIP, "%s in Jacobi order needs a HIP device: device %d of %d asked for", what, device,
                     ndev);
    return ACMMP_OK;
}

// what the two folder calls differ in once their views are loaded
struct JacobiCall {
    JacobiRule rule;
    const std::vector<std::vector<float>> *pdepths, *pnormals;  // the prior-aware fusion's second pair, else null
    const char *tag;  // of the ACMMP_HOST_TIMING line
    std::string ply;
};

// The loaded views (masks assigned, sources resolved) through the device, view by view, into call.ply.
int fuse_on_device(Scene &sc, const JacobiCall &call, int device, Pool &pool, Clock::time_point t_start,
                   int *num_points) {
    const acmmp_problem *problems = sc.problems;
    const size_t n = sc.rows.size();
    const bool prior = call.rule.prior;
    const bool timing = std::getenv("ACMMP_HOST_TIMING") != nullptr;
    int rc = check_view_sizes(sc);
    if (rc) return rc;
    size_t max_pixels = 0;
    for (size_t i = 0; i < n; ++i) max_pixels = std::max(max_pixels, (size_t)sc.cols[i] * sc.rows[i]);
    const auto t_loaded = Clock::now();

    // ---- upload: every view's depth, normal and mask words, and the table of views, once
    FUSION_HIP_TRY(hipSetDevice(device));
    DevHold hold;
    FUSION_HIP_TRY(hold.own_stream());
    for (hipEvent_t &e : hold.copied) FUSION_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    size_t arena_bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t N = (size_t)sc.cols[i] * sc.rows[i];
        arena_bytes += (prior ? 2 : 1) * (align256(N * sizeof(float)) + align256(N * 3 * sizeof(float))) +
                       align256(sc.masks[i].w.size() * sizeof(uint64_t));
    }
    char *arena = nullptr;
    FUSION_HIP_TRY(hold.dev_alloc(arena, arena_bytes));
    std::vector<DevView> views(n);
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t N = (size_t)sc.cols[i] * sc.rows[i];
        DevView &v = views[i];
        v = dev_view(sc.cameras[i], sc.cols[i], sc.rows[i], sc.src_index[i].data(), problems[i].num_src_images);
        v.dstride = 1;
        v.nstride = 3;  // (bgr stays null: the colours stay with the host's collect)
        auto put = [&](const void *src, size_t bytes) -> char * {
            char *d = arena + at;
            at += align256(bytes);
            return hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, hold.stream) == hipSuccess ? d : nullptr;
        };
        v.depth = (const float *)put(sc.depths[i].data(), N * sizeof(float));
        v.normal = (const float *)put(sc.normals[i].data(), N * 3 * sizeof(float));
        v.mask = (uint32_t *)put(sc.masks[i].w.data(), sc.masks[i].w.size() * sizeof(uint64_t));
        v.pdepth = prior ? (const float *)put((*call.pdepths)[i].data(), N * sizeof(float)) : nullptr;
        v.pnormal = prior ? (const float *)put((*call.pnormals)[i].data(), N * 3 * sizeof(float)) : nullptr;
        if (!v.depth || !v.normal || !v.mask || (prior && (!v.pdepth || !v.pnormal)))
            return ffail(ACMMP_ERR_HIP, "upload of view %d failed: %s", problems[i].ref_image_id,
                         hipGetErrorString(hipGetLastError()));
    }
    DevView *d_views = nullptr;
    FUSION_HIP_TRY(hold.dev_alloc(d_views, n));
    FUSION_HIP_TRY(hipMemcpyAsync(d_views, views.data(), n * sizeof(DevView), hipMemcpyHostToDevice, hold.stream));
    ViewScratch scratch;
    if ((rc = alloc_scratch(hold, max_pixels, scratch))) return rc;
    int *d_view_points = nullptr, *h_view_points = nullptr;  // [i & 1], as the points: view i's count
    DevPoint *d_out[2] = {nullptr, nullptr}, *h_out[2] = {nullptr, nullptr};
    FUSION_HIP_TRY(hold.dev_alloc(d_view_points, 2));
    FUSION_HIP_TRY(hold.pinned_alloc(h_view_points, 2));
    for (int b = 0; b < 2; ++b) {
        FUSION_HIP_TRY(hold.dev_alloc(d_out[b], max_pixels));
        FUSION_HIP_TRY(hold.pinned_alloc(h_out[b], std::max(max_pixels, size_t(1))));
    }
    FUSION_HIP_TRY(hipStreamSynchronize(hold.stream));
    const auto t_uploaded = Clock::now();

    // ---- the views, in order. View i's points come back while view i + 1's kernels run, and the
    // host forms view i's cloud entries (normal and colour are the host's) beside them.
    std::vector<Point> cloud;
    cloud.reserve(sc.pixels());
    double t_wait = 0, t_copy_wait = 0, t_collect = 0;
    auto collect = [&](size_t i) -> int {  // view i's points, in pixel order, into the cloud
        const auto t0 = Clock::now();
        FUSION_HIP_TRY(hipEventSynchronize(hold.copied[i & 1]));
        t_copy_wait += secs(t0, Clock::now());
        const DevPoint *pts = h_out[i & 1];
        const int cnt = h_view_points[i & 1];
        const float *normal[2] = {sc.normals[i].data(), prior ? (*call.pnormals)[i].data() : nullptr};
        const uint8_t *img = sc.images[i].data();
        for (int k = 0; k < cnt; ++k) {
            const size_t q = pts[k].q & 0x7fffffffu;
            const float *nrm = normal[pts[k].q >> 31];  // the chosen hypothesis's map
            Point p;
            p.coord = F3{pts[k].x, pts[k].y, pts[k].z};
            p.normal = F3{nrm[q * 3], nrm[q * 3 + 1], nrm[q * 3 + 2]};
            p.color = F3{(float)img[q * 3], (float)img[q * 3 + 1], (float)img[q * 3 + 2]};
            cloud.push_back(p);
        }
        t_collect += secs(t0, Clock::now());
        return ACMMP_OK;
    };
    for (size_t i = 0; i < n; ++i) {
        const int N = sc.cols[i] * sc.rows[i];
        enqueue_view(hold.stream, d_views, (int)i, N, scratch, call.rule, d_out[i & 1], DevCloud{},
                     d_view_points + (i & 1), nullptr);
        FUSION_HIP_TRY(hipGetLastError());
        FUSION_HIP_TRY(hipMemcpyAsync(h_view_points + (i & 1), d_view_points + (i & 1), sizeof(int),
                                      hipMemcpyDeviceToHost, hold.stream));
        if (i > 0 && (rc = collect(i - 1))) return rc;  // beside view i's kernels
        const auto t1 = Clock::now();
        FUSION_HIP_TRY(hipStreamSynchronize(hold.stream));
        t_wait += secs(t1, Clock::now());
        const int cnt = h_view_points[i & 1];
        if (cnt < 0 || cnt > N)
            return ffail(ACMMP_ERR_HIP, "view %d: %d points of %d pixels", problems[i].ref_image_id, cnt, N);
        if (cnt > 0)
            FUSION_HIP_TRY(hipMemcpyAsync(h_out[i & 1], d_out[i & 1], (size_t)cnt * sizeof(DevPoint),
                                          hipMemcpyDeviceToHost, hold.stream));
        FUSION_HIP_TRY(hipEventRecord(hold.copied[i & 1], hold.stream));
    }
    if ((rc = collect(n - 1))) return rc;
    if (num_points) *num_points = (int)cloud.size();
    const auto t_fused = Clock::now();
    rc = store_ply(call.ply, cloud, &pool);
    if (timing)
        std::fprintf(stderr,
                     "[%s] load=%.3fs upload=%.3fs views=%.3fs (device_wait=%.3fs download_wait=%.3fs "
                     "collect=%.3fs) ply=%.3fs threads=%d map_bytes=%zu points=%zu\n",
                     call.tag, secs(t_start, t_loaded), secs(t_loaded, t_uploaded), secs(t_uploaded, t_fused), t_wait,
                     t_copy_wait, t_collect - t_copy_wait, secs(t_fused, Clock::now()), pool.size() + 1, arena_bytes,
                     cloud.size());
    return rc;
}

// The checked views through the device on the caller's stream (borrowed): mask words packed, then
// view by view; the carry adds the view's approvals to the running total and the apply step writes
// whole points at the total before the view + the position in it. No wait between views: the one
// at the end is for the count.
int fuse_views_on_device(int device, const acmmp_fusion_view *views, int count, float consistency_scalar,
                         int con_num_thresh, const acmmp_cloud_buffers *out, hipStream_t stream,
                         int64_t *num_points) {
    const size_t n = (size_t)count;
    FUSION_HIP_TRY(hipSetDevice(device));
    DevHold hold;
    hold.stream = stream;
    auto mask_bytes = [](size_t N) { return align256((N + 63) / 64 * sizeof(uint64_t)); };
    size_t max_pixels = 0, mask_arena_bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t N = (size_t)views[i].cam.width * views[i].cam.height;
        max_pixels = std::max(max_pixels, N);
        mask_arena_bytes += mask_bytes(N);
    }
    char *d_masks = nullptr;
    DevView *d_views = nullptr, *h_views = nullptr;
    ViewScratch scratch;
    long long *d_total = nullptr, *h_total = nullptr;
    FUSION_HIP_TRY(hold.dev_alloc(d_masks, mask_arena_bytes));
    FUSION_HIP_TRY(hold.dev_alloc(d_views, n));
    if (const int rc = alloc_scratch(hold, max_pixels, scratch)) return rc;
    FUSION_HIP_TRY(hold.dev_alloc(d_total, 2));
    FUSION_HIP_TRY(hold.pinned_alloc(h_views, n));  // pinned: the copies below do not wait
    FUSION_HIP_TRY(hold.pinned_alloc(h_total, 1));
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const acmmp_fusion_view &in = views[i];
        DevView &v = h_views[i];
        v = dev_view(in.cam, in.cam.width, in.cam.height, in.src, in.num_src);
        v.depth = in.d_depth;
        v.normal = in.d_normal;
        v.dstride = in.depth_stride;
        v.nstride = in.normal_stride;
        v.bgr = in.d_bgr;
        v.mask = (uint32_t *)(d_masks + at);
        at += mask_bytes((size_t)v.W * v.H);
    }
    hold.pending = true;
    FUSION_HIP_TRY(hipMemsetAsync(d_masks, 0, mask_arena_bytes, stream));
    FUSION_HIP_TRY(hipMemsetAsync(d_total, 0, 2 * sizeof(long long), stream));
    FUSION_HIP_TRY(hipMemcpyAsync(d_views, h_views, n * sizeof(DevView), hipMemcpyHostToDevice, stream));
    for (size_t i = 0; i < n; ++i) {  // every view's initial mask, before the first view's tests read a source's
        const int N = h_views[i].W * h_views[i].H;
        if (views[i].d_mask) k_mask_pack<<<(N + 255) / 256, 256, 0, stream>>>(views[i].d_mask, N, h_views[i].mask);
    }
    DevCloud cloud{};
    if (out && out->capacity > 0) cloud = DevCloud{out->d_xyz, out->d_normal, out->d_rgb, out->capacity, nullptr};
    cloud.total = d_total;
    const JacobiRule rule{false, consistency_scalar, con_num_thresh, 0};
    for (size_t i = 0; i < n; ++i)
        enqueue_view(stream, d_views, (int)i, h_views[i].W * h_views[i].H, scratch, rule, nullptr, cloud, nullptr,
                     d_total);
    FUSION_HIP_TRY(hipGetLastError());
    FUSION_HIP_TRY(hipMemcpyAsync(h_total, d_total + 1, sizeof(long long), hipMemcpyDeviceToHost, stream));
    FUSION_HIP_TRY(hipStreamSynchronize(stream));  // the call's one wait
    hold.pending = false;
    *num_points = *h_total;
    if (out && out->capacity > 0 && *h_total > out->capacity)
        return ffail(ACMMP_ERR_ARG, "the fusion produced %lld points, the cloud buffers hold %lld", *h_total,
                     (long long)out->capacity);
    return ACMMP_OK;
}

}  // namespace

extern "C" {

int acmmp_fusion_jacobi_scan_chunk(void) { return kScanChunk; }

int acmmp_fuse_views_jacobi(int device, const acmmp_fusion_view *views, int count, float consistency_scalar,
                            int con_num_thresh, const acmmp_cloud_buffers *out, void *stream, int64_t *num_points) {
    if (const int rc = check_fusion_views(views, count, out, num_points)) return rc;
    *num_points = 0;
    if (need_device("Fusing device-resident views", device)) return ACMMP_ERR_HIP;
    return fuse_views_on_device(device, views, count, consistency_scalar, con_num_thresh, out, (hipStream_t)stream,
                                num_points);
}

int acmmp_run_fusion_jacobi(const char *dense_folder, const char *output_folder, const acmmp_problem *problems,
                            int count, int geom_consistency, float consistency_scalar, int con_num_thresh,
                            const char *image_dir, const char *mask_folder, int device, int *num_points) {
    if (!dense_folder || !output_folder || !problems || count <= 0) return ffail(ACMMP_ERR_ARG, "bad args");
    if (need_device("RunFusion", device)) return ACMMP_ERR_HIP;
    const auto t_start = Clock::now();
    Scene sc(problems, (size_t)count);
    Pool pool;
    const int rc = load_fusion_views(sc, pool, dense_folder, output_folder, geom_consistency, image_dir, mask_folder);
    if (rc) return rc;
    const JacobiCall call{{false, consistency_scalar, con_num_thresh, 0}, nullptr, nullptr, "RunFusionJacobi",
                          std::string(output_folder) + "/ACMMP_model.ply"};
    return fuse_on_device(sc, call, device, pool, t_start, num_points);
}

int acmmp_run_prior_aware_fusion_jacobi(const char *dense_folder, const char *output_folder,
                                        const char *fusion_folder, const acmmp_problem *problems, int count,
                                        int geom_consistency, float consistency_scalar, int num_consistent_thresh,
                                        int single_match_penalty, int device, int *num_points) {
    if (!dense_folder || !output_folder || !fusion_folder || !problems || count <= 0)
        return ffail(ACMMP_ERR_ARG, "bad args");
    if (need_device("RunPriorAwareFusion", device)) return ACMMP_ERR_HIP;
    const std::string dense = dense_folder, out = output_folder, fus = fusion_folder;
    const auto t_start = Clock::now();
    FusionInputs in(problems, (size_t)count);
    Pool pool;
    int rc = pool_for(pool, count, [&](int i) -> int {  // the literal call's loads, on the pool
        const int load_rc = load_prior_view(in, (size_t)i, dense, out, fus, depth_suffix(geom_consistency));
        if (!load_rc) in.masks[(size_t)i].assign((size_t)in.cols[(size_t)i] * in.rows[(size_t)i]);
        return load_rc;
    });
    if (!rc) rc = resolve_sources(in);
    if (rc) return rc;
    const JacobiCall call{{true, consistency_scalar, num_consistent_thresh, single_match_penalty}, &in.pdepths,
                          &in.pnormals, "RunPriorAwareFusionJacobi", out + "/ACMMP_prior_model.ply"};
    return fuse_on_device(in, call, device, pool, t_start, num_points);
}

}  // extern "C"

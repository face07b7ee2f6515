// acmmp_kernels.hip — the plain (non-templated) MI355X kernels of
// ACMMP::RunPatchMatch and every kernel launcher. The templated PatchMatch
// kernels live in acmmp_kernels_tx.hip, one translation unit per texel form;
// launch_init / launch_sweep / launch_eval_costs pick the form and the patch
// policy here (tx_dispatch, gx_dispatch). Shared device helpers: acmmp_dev.h.
#include <type_traits>

#include "acmmp_dev.h"

namespace acmmp {

__global__ __launch_bounds__(256) void k_finalize(const KViews *__restrict__ kvp, KState st) {
    const KViews &kv = *kvp;
    const int px = blockIdx.x * 64 + threadIdx.x;
    const int py = (st.y0 / 4 + (int)blockIdx.y) * 4 + threadIdx.y;
    if (px >= kv.W || py < st.y0 || py >= st.y1) return;
    const int c = (px + py) & 1;
    const int ci = cs_index(kv, px, py);
    float4 h = st.plane[c][ci];
    h.w = plane_depth(kv.cam[0], h, px, py);
    h = to_world(kv.cam[0], h);
    const int center = py * kv.W + px;
    st.rm_plane[center] = h;
    st.rm_depth[center] = h.w;
    st.rm_cost[center] = st.cost[c][ci];
    st.rm_sv[center] = st.sv[c][ci];
}

// CheckerboardFilter (src/ACMMP.cu:1214-1328) on one colour, in place on the
// row-major planes: every read is of the opposite colour.
__global__ __launch_bounds__(256) void k_filter(const KViews *__restrict__ kvp, KState st, int colour) {
    const KViews &kv = *kvp;
    const int k = blockIdx.x * 64 + threadIdx.x;
    const int py = (st.y0 / 4 + (int)blockIdx.y) * 4 + threadIdx.y;
    const int width = kv.W, height = kv.H;
    if (py < st.y0 || py >= st.y1 || py >= kv.sweep_rows) return;
    const int px = 2 * k + ((py + colour) & 1);
    if (px >= width) return;
    // neighbours' depths from the depth plane (4 B each; the same values as
    // rm_plane[.].w, which the filter updates alongside)
    const float *ph = st.rm_depth;
    const int center = py * width + px;
    if (st.rm_cost[center] < 0.001f) return;
    float f[21];
    int n = 0;
    f[n++] = ph[center];
    const int left = center - 1, leftleft = center - 3;
    const int up = center - width, upup = center - 3 * width;
    const int down = center + width, downdown = center + 3 * width;
    const int right = center + 1, rightright = center + 3;
    if (py > 0) f[n++] = ph[up];
    if (py > 2) f[n++] = ph[upup];
    if (py > 4) f[n++] = ph[upup - width * 2];
    if (py < height - 1) f[n++] = ph[down];
    if (py < height - 3) f[n++] = ph[downdown];
    if (py < height - 5) f[n++] = ph[downdown + width * 2];
    if (px > 0) f[n++] = ph[left];
    if (px > 2) f[n++] = ph[leftleft];
    if (px > 4) f[n++] = ph[leftleft - 2];
    if (px < width - 1) f[n++] = ph[right];
    if (px < width - 3) f[n++] = ph[rightright];
    if (px < width - 5) f[n++] = ph[rightright + 2];
    if (py > 0 && px < width - 2) f[n++] = ph[up + 2];
    if (py < height - 1 && px < width - 2) f[n++] = ph[down + 2];
    if (py > 0 && px > 1) f[n++] = ph[up - 2];
    if (py < height - 1 && px > 1) f[n++] = ph[down - 2];
    if (px > 0 && py > 2) f[n++] = ph[left - width * 2];
    if (px < width - 1 && py > 2) f[n++] = ph[right - width * 2];
    if (px > 0 && py < height - 2) f[n++] = ph[left + width * 2];
    if (px < width - 1 && py < height - 2) f[n++] = ph[right + width * 2];
    for (int i = 1; i < n; i++) {  // sort_small
        const float tmp = f[i];
        int j;
        for (j = i; j >= 1 && tmp < f[j - 1]; j--) f[j] = f[j - 1];
        f[j] = tmp;
    }
    const int m = n / 2;
    const float med = (n % 2 == 0) ? (f[m - 1] + f[m]) / 2 : f[m];
    st.rm_depth[center] = med;
    st.rm_plane[center].w = med;
}

__global__ __launch_bounds__(256) void k_eval_geom(const KViews *__restrict__ kvp, const float4 *planes,
                                                   float *out) {
    const KViews &kv = *kvp;
    const int px = blockIdx.x * 64 + threadIdx.x;
    const int py = blockIdx.y * 4 + threadIdx.y;
    if (px >= kv.W || py >= kv.H) return;
    const int c = py * kv.W + px;
    for (int v = 0; v < kv.nsrc; ++v) out[(size_t)c * kv.nsrc + v] = geom_cost(kv, v + 1, planes[c], px, py);
}

// Padded copy of a source image (see KViews::pad).
// Row-paired clamp-to-edge copy of a source view for the NCC gathers:
// element (r, c), r < H + 2, c < W + 3, is the float pair
// (texel(clamp(c-1), clamp(r-1)), texel(clamp(c-1), clamp(r))); dpitch in pairs.
__global__ __launch_bounds__(256) void k_pad_image(const float *__restrict__ src, int spitch, int W, int H,
                                                   float *__restrict__ dst, int dpitch) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    const int r = blockIdx.y * 4 + threadIdx.y;
    if (c >= W + 3 || r >= H + 2) return;
    const int x = min(max(c - 1, 0), W - 1);
    const int y0 = min(max(r - 1, 0), H - 1), y1 = min(r, H - 1);
    reinterpret_cast<float2 *>(dst)[(size_t)r * dpitch + c] = make_float2(src[y0 * spitch + x], src[y1 * spitch + x]);
}

hipError_t launch_pad_image(const float *src, int spitch, int W, int H, float *dst, int dpitch, hipStream_t s) {
    dim3 block(64, 4), grid((W + 3 + 63) / 64, (H + 2 + 3) / 4);
    k_pad_image<<<grid, block, 0, s>>>(src, spitch, W, H, dst, dpitch);
    return hipGetLastError();
}

// u8 quad layout: element (r, c), r < H + 2, c < W + 2, packs the texels
// (clamp(c-1), clamp(r-1)), (clamp(c-1), clamp(r)), (clamp(c), clamp(r-1)),
// (clamp(c), clamp(r)) as bytes 0..3, so the record at (y0 + 1, x0 + 1) is
// the whole bilinear footprint of (x0, y0) (same record index as the fp32
// row-paired copy). Texel (clamp(c-1), clamp(r-1)) ranges over every texel,
// so checking it checks the view: -0.0f, NaN and non-integers are not u8.
__global__ __launch_bounds__(256) void k_pad_quad(const float *__restrict__ src, int spitch, int W, int H,
                                                  uint32_t *__restrict__ dst, int dpitch, uint32_t *not_u8) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    const int r = blockIdx.y * 4 + threadIdx.y;
    if (c >= W + 2 || r >= H + 2) return;
    const int xa = min(max(c - 1, 0), W - 1), xb = min(c, W - 1);
    const int ya = min(max(r - 1, 0), H - 1), yb = min(r, H - 1);
    const float t00 = src[ya * spitch + xa], t01 = src[yb * spitch + xa];
    const float t10 = src[ya * spitch + xb], t11 = src[yb * spitch + xb];
    const bool ok = t00 >= 0.0f && t00 <= 255.0f && t00 == dm_floor(t00) && (__float_as_uint(t00) >> 31) == 0u;
    if (!ok) *not_u8 = 1u;
    auto b = [](float t) -> uint32_t { return (t >= 0.0f && t <= 255.0f) ? (uint32_t)t : 0u; };
    dst[(size_t)r * dpitch + c] = b(t00) | (b(t01) << 8) | (b(t10) << 16) | (b(t11) << 24);
}

// f16 difference-quad layout: element (r, c), r < H + 2, c < W + 2, holds
// the halves (t00, t01, t10 - t00, t11 - t01) of the same clamped texels as
// the u8 quad, the differences formed in fp32 exactly as the lerp forms them
// (lerp_sample). Sets *not_h16 if any stored value is not exactly
// representable (non-finite, beyond +-65504, or more than 11 significant
// bits); the copy is then unusable and the fp32 form is built.
__global__ __launch_bounds__(256) void k_pad_h16(const float *__restrict__ src, int spitch, int W, int H,
                                                 uint2 *__restrict__ dst, int dpitch, uint32_t *not_h16) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    const int r = blockIdx.y * 4 + threadIdx.y;
    if (c >= W + 2 || r >= H + 2) return;
    const int xa = min(max(c - 1, 0), W - 1), xb = min(c, W - 1);
    const int ya = min(max(r - 1, 0), H - 1), yb = min(r, H - 1);
    const float t00 = src[ya * spitch + xa], t01 = src[yb * spitch + xa];
    const float t10 = src[ya * spitch + xb], t11 = src[yb * spitch + xb];
    const float v[4] = {t00, t01, t10 - t00, t11 - t01};
    _Float16 h[4];
    bool ok = true;
    for (int i = 0; i < 4; ++i) {
        h[i] = (_Float16)v[i];
        const float back = (float)h[i];
        ok = ok && __float_as_uint(back) == __float_as_uint(v[i]) && dm_fabs(v[i]) <= 65504.0f;
    }
    if (!ok) *not_h16 = 1u;
    dst[(size_t)r * dpitch + c] = make_uint2(__builtin_bit_cast(uint32_t, h2v{h[0], h[1]}),
                                             __builtin_bit_cast(uint32_t, h2v{h[2], h[3]}));
}

hipError_t launch_pad_h16(const float *src, int spitch, int W, int H, void *dst, int dpitch, uint32_t *not_h16,
                          hipStream_t s) {
    dim3 block(64, 4), grid((W + 2 + 63) / 64, (H + 2 + 3) / 4);
    k_pad_h16<<<grid, block, 0, s>>>(src, spitch, W, H, reinterpret_cast<uint2 *>(dst), dpitch, not_h16);
    return hipGetLastError();
}

hipError_t launch_pad_quad(const float *src, int spitch, int W, int H, uint32_t *dst, int dpitch, uint32_t *not_u8,
                           hipStream_t s) {
    dim3 block(64, 4), grid((W + 2 + 63) / 64, (H + 2 + 3) / 4);
    k_pad_quad<<<grid, block, 0, s>>>(src, spitch, W, H, dst, dpitch, not_u8);
    return hipGetLastError();
}

// Exhaustive check of recip_newton against IEEE 1/z over every float32 bit
// pattern inside recip_fast_window (grid-stride over all 2^32 patterns).
__global__ __launch_bounds__(256) void k_selftest_rcp(unsigned long long *mismatch,
                                                      unsigned long long *checked) {
    unsigned long long bad = 0, n = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < (1ull << 32); u += stride) {
        const float z = __uint_as_float((uint32_t)u);
        if (!recip_fast_window(z)) continue;
        ++n;
        const float a = recip_newton(z);
        volatile float one = 1.0f;
        const float b = one / z;
        if (__float_as_uint(a) != __float_as_uint(b)) ++bad;
    }
    atomicAdd(mismatch, bad);
    atomicAdd(checked, n);
}

hipError_t launch_selftest_rcp(unsigned long long *mismatch, unsigned long long *checked, hipStream_t s) {
    k_selftest_rcp<<<4096, 256, 0, s>>>(mismatch, checked);
    return hipGetLastError();
}

// JBU_cu (src/ACMMP.cu:1458-1516): joint-bilateral upsampling of a low-res
// depth map guided by the high-res reference image; one thread per high-res
// pixel. Texture reads at integer + 0.5 are exact texels (pin A4).
__global__ __launch_bounds__(256) void k_jbu(const float *__restrict__ img, int W, int H,
                                             const float *__restrict__ depth, int sw, int sh, int image_scale,
                                             float *__restrict__ out) {
    const int px = blockIdx.x * blockDim.x + threadIdx.x;
    const int py = blockIdx.y * blockDim.y + threadIdx.y;
    if (px >= W || py >= H) return;
    const float scale = (float)(1.0 * sw / W);
    const float sigmad = 0.50f, sigmar = 25.5f;
    const int nn = (image_scale * image_scale + 1) / 2;
    const float o_y = (float)py * scale;
    const float o_x = (float)px * scale;
    const float refPix = img[(size_t)py * W + px];
    float total_val = 0.0f, normalizing_factor = 0.0f;
    for (int j = -nn; j <= nn; ++j) {
        int r_y = (int)(o_y + (float)j);
        r_y = (r_y > 0 ? (r_y < sh ? r_y : sh - 1) : 0);
        int r_ys = py + j;
        r_ys = (r_ys > 0 ? (r_ys < H ? r_ys : H - 1) : 0);
        for (int i = -nn; i <= nn; ++i) {
            int r_x = (int)(o_x + (float)i);
            r_x = (r_x > 0 ? (r_x < sw ? r_x : sw - 1) : 0);
            const float srcPix = depth[(size_t)r_y * sw + r_x];
            int r_xs = px + i;
            r_xs = (r_xs > 0 ? (r_xs < W ? r_xs : W - 1) : 0);
            const float nb = img[(size_t)r_ys * W + r_xs];
            const float tg = spatial_gauss(o_x, o_y, (float)r_x, (float)r_y, sigmad) *
                             range_gauss(dm_fabs(refPix - nb), sigmar);
            normalizing_factor += tg;
            total_val += srcPix * tg;
        }
    }
    out[(size_t)py * W + px] = total_val / normalizing_factor;
}

// ---------------------------------------------------------------- launchers
// plane_hypotheses_host[center] = (0, 0, 0, depth) for the hierarchy init
// (src/ACMMP.cpp:797-804: x, y, z never written, pinned 0)
__global__ __launch_bounds__(256) void k_depth_planes(const float *__restrict__ depth, size_t n,
                                                      float4 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = make_float4(0.0f, 0.0f, 0.0f, depth[i]);
}

hipError_t launch_depth_planes(const float *depth, size_t n, float4 *out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    k_depth_planes<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(depth, n, out);
    return hipGetLastError();
}

// pSampler::GetPriorPlaneEstimate (src/acmmp_definitions.cpp:99-177): the
// seeded plane of output pixel (i, j) of a rows x cols view from the decoded
// 16-bit prior maps, one thread per pixel. The host loop of
// acmmp_prior_plane_estimate (acmmp_pipeline.cpp) restated: every operation a
// separate IEEE fp32 operation in the host's order (this unit builds with
// -ffp-contract=off; `/` and the square root are correctly rounded), so the
// planes are the host's bit for bit. The depth word is read at r*dw*dc + c
// (Mat_<float>::at(r, c) on a possibly multi-channel map), the normal words in
// B, G, R order as stored, and normVec3 multiplies by the norm: all kept.
// The launcher's caller has checked that the largest indices are in range.
__global__ __launch_bounds__(256) void k_seed_planes(const uint16_t *__restrict__ depth, int dw, int dc,
                                                     const uint16_t *__restrict__ normals, int nw, int scale,
                                                     acmmp_camera cam, int rows, int cols,
                                                     float4 *__restrict__ out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= cols || i >= rows) return;
    const size_t r = (size_t)i * (size_t)scale, c = (size_t)j * (size_t)scale;
    const size_t di = r * (size_t)dw * (size_t)dc + c;
    const size_t ni = (r * (size_t)nw + c) * 3;
    // Mat::convertTo(CV_32F, alpha, beta): src * alpha + beta in float
    const float dist = cam.depth_max - cam.depth_min;
    const float range = dist / 65535.0f;
    const float nalpha = (float)(2.0 / 65536.0), nbeta = -1.0f;
    const float d = (float)depth[di] * range + cam.depth_min;
    float nx = (float)normals[ni] * nalpha + nbeta;
    float ny = (float)normals[ni + 1] * nalpha + nbeta;
    float nz = (float)normals[ni + 2] * nalpha + nbeta;
    // depth_normal_to_plane (:72-89): getViewDirection, the flip, normVec3, distance_to_origin
    const float X0 = d * (j - cam.K[2]) / cam.K[0];
    const float X1 = d * (i - cam.K[5]) / cam.K[4];
    const float X2 = d;
    const float norm = dm_sqrt(X0 * X0 + X1 * X1 + X2 * X2);
    const float v0 = X0 / norm, v1 = X1 / norm, v2 = X2 / norm;
    const float dot = nx * v0 + ny * v1 + nz * v2;
    if (dot > 0.0f) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    const float n2 = nx * nx + ny * ny + nz * nz;
    const float s = dm_sqrt(n2);
    nx *= s;
    ny *= s;
    nz *= s;
    out[(size_t)i * cols + j] = make_float4(nx, ny, nz, -(nx * X0 + ny * X1 + nz * X2));
}

hipError_t launch_seed_planes(const uint16_t *depth, int dw, int dc, const uint16_t *normals, int nw, int scale,
                              const acmmp_camera &cam, int rows, int cols, float4 *out, hipStream_t stream) {
    dim3 block(64, 4), grid((cols + 63) / 64, (rows + 3) / 4);
    k_seed_planes<<<grid, block, 0, stream>>>(depth, dw, dc, normals, nw, scale, cam, rows, cols, out);
    return hipGetLastError();
}

hipError_t launch_jbu(const float *img, int W, int H, const float *depth, int sw, int sh, int image_scale,
                      float *out, hipStream_t stream) {
    dim3 block(64, 4), grid((W + 63) / 64, (H + 3) / 4);
    k_jbu<<<grid, block, 0, stream>>>(img, W, H, depth, sw, sh, image_scale, out);
    return hipGetLastError();
}

// KViews::wide -> the integer record index of views with 2^24 or more
// records; KViews::texel -> the texel form; texture_filter8 -> 8-bit fractions
static int tx_form(const KViews &h_kv) {
    return (h_kv.wide ? kTxWide : 0) | (h_kv.texel == kTexelU8 ? kTxU8 : 0) |
           (h_kv.texel == kTexelH16 ? kTxH16 : 0) | (h_kv.prm.texture_filter8 ? kTxFrac8 : 0);
}

// Calls f(std::integral_constant<int, TX>) for the texel form TX of h_kv, one
// case per form of ACMMP_TX_FORMS.
template <typename F>
static hipError_t tx_dispatch(const KViews &h_kv, F f) {
    switch (tx_form(h_kv)) {
#define ACMMP_TX_CASE(TX) \
    case TX: return f(std::integral_constant<int, TX>{});
        ACMMP_TX_FORMS(ACMMP_TX_CASE)
#undef ACMMP_TX_CASE
        default: return hipErrorNotSupported;  // texture_filter8 with a wide or f16 form
    }
}

// The same for the general-patch units (KViews::general), one case per form
// of ACMMP_GX_FORMS.
template <typename F>
static hipError_t gx_dispatch(const KViews &h_kv, F f) {
    switch (tx_form(h_kv)) {
#define ACMMP_GX_CASE(TX) \
    case TX: return f(std::integral_constant<int, TX>{});
        ACMMP_GX_FORMS(ACMMP_GX_CASE)
#undef ACMMP_GX_CASE
        default: return hipErrorNotSupported;  // texture_filter8 is an 11 / 2 mode
    }
}

// Colour-split grid over image rows [st.y0, st.y1): whole blocks of kBY
// rows from the block row holding y0 (the kernels skip rows outside).
static dim3 cs_grid(const KViews &kv, const KState &st, int colours) {
    const int by0 = st.y0 / kBY;
    return dim3((kv.Wh + kBX - 1) / kBX, (st.y1 - by0 * kBY + kBY - 1) / kBY, colours);
}
// 64 x 4 grid over rows [st.y0, st.y1) and `cols` columns
static dim3 row_grid(int cols, const KState &st) {
    return dim3((cols + 63) / 64, (st.y1 - (st.y0 / 4) * 4 + 3) / 4);
}

hipError_t launch_init(const KViews *d_kv, const KViews &h_kv, const KState &st, hipStream_t stream) {
    if (st.y1 <= st.y0) return hipSuccess;
    if (h_kv.general)
        return gx_dispatch(h_kv, [&](auto tx) {
            return gx_launch_init<decltype(tx)::value>(d_kv, h_kv.nsrc, cs_grid(h_kv, st, 2), stream, st);
        });
    return tx_dispatch(h_kv, [&](auto tx) {
        return tx_launch_init<decltype(tx)::value>(d_kv, h_kv.nsrc, cs_grid(h_kv, st, 2), stream, st);
    });
}

hipError_t launch_sweep(const KViews *d_kv, const KViews &h_kv, const KState &st, int colour, int iter,
                        hipStream_t stream) {
    if (st.y1 <= st.y0) return hipSuccess;
    if (h_kv.general)
        return gx_dispatch(h_kv, [&](auto tx) {
            return gx_launch_sweep<decltype(tx)::value>(d_kv, h_kv.nsrc, cs_grid(h_kv, st, 1), stream, st, colour,
                                                        iter);
        });
    return tx_dispatch(h_kv, [&](auto tx) {
        return tx_launch_sweep<decltype(tx)::value>(d_kv, h_kv.nsrc, cs_grid(h_kv, st, 1), stream, st, colour, iter);
    });
}

hipError_t launch_finalize(const KViews *d_kv, const KViews &h_kv, const KState &st, hipStream_t stream) {
    if (st.y1 <= st.y0) return hipSuccess;
    k_finalize<<<row_grid(h_kv.W, st), dim3(64, 4), 0, stream>>>(d_kv, st);
    return hipGetLastError();
}

hipError_t launch_filter(const KViews *d_kv, const KViews &h_kv, const KState &st, int colour,
                         hipStream_t stream) {
    if (st.y1 <= st.y0) return hipSuccess;
    k_filter<<<row_grid(h_kv.Wh, st), dim3(64, 4), 0, stream>>>(d_kv, st, colour);
    return hipGetLastError();
}

hipError_t launch_eval_costs(const KViews *d_kv, const KViews &h_kv, const float4 *planes, float *out,
                             float *out_init, uint32_t *out_views, hipStream_t stream) {
    KState all{};
    all.y1 = h_kv.H;
    if (h_kv.general)
        return gx_dispatch(h_kv, [&](auto tx) {
            return gx_launch_eval<decltype(tx)::value>(d_kv, h_kv.nsrc, cs_grid(h_kv, all, 2), stream, planes, out,
                                                       out_init, out_views);
        });
    return tx_dispatch(h_kv, [&](auto tx) {
        return tx_launch_eval<decltype(tx)::value>(d_kv, h_kv.nsrc, cs_grid(h_kv, all, 2), stream, planes, out,
                                                   out_init, out_views);
    });
}

hipError_t launch_eval_geom(const KViews *d_kv, const KViews &h_kv, const float4 *planes, float *out,
                            hipStream_t stream) {
    dim3 block(64, 4), grid((h_kv.W + 63) / 64, (h_kv.H + 3) / 4);
    k_eval_geom<<<grid, block, 0, stream>>>(d_kv, planes, out);
    return hipGetLastError();
}

}  // namespace acmmp

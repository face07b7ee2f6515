// acmmp_dev.h — device helpers shared by the MI355X (gfx950, CDNA4) kernels
// for ACMMP::RunPatchMatch: textures, geometry, RNG, the reference tile, the
// NCC rows, the geometric cost, the lane maps and the 11 / 2 patch policy
// (FastPatch; the policy of every other geometry is acmmp_general.h).
// Included by acmmp_kernels.hip (the plain kernels, every launcher, the
// texel-form dispatch) and by acmmp_kernels_tx.hip (the templated PatchMatch
// kernels, compiled once per texel form and patch policy).
//
// Reference semantics: rlav440/ACMMP src/ACMMP.cu:17-1352 (device code) with the
// pinned semantics of SURVEY.md Appendix A and the arithmetic pins P1-P4 listed
// in oracle/acmmp_oracle.c / DESIGN.md §4. The CPU oracle restates the
// reference literally; these files are the GPU design:
//
//  * one lane per pixel, 64-lane waves laid along a row of ONE checkerboard
//    colour (colour-split layout, acmmp_internal.h) so every state access of
//    a wave is a contiguous 256-B..1-KiB segment;
//  * the reference patch of a pixel (36 bilateral weights w and w*ref, the
//    normalised ref mean/variance) is invariant across the 14*(N-1)
//    ComputeBilateralNCC calls of a pixel-iteration: it is computed once per
//    pixel-iteration into VGPRs (exact: same operations, same order);
//  * NCC calls for views whose sampled view weight is 0 are skipped: the
//    reference multiplies their (finite, >= 0) cost by 0 and adds +0, so the
//    result is bit-identical (refinement at :751 skips them explicitly);
//  * stateless Philox RNG (no 48-B curandState traffic per pixel);
//  * all per-launch constants (cameras, homography camera terms, image
//    pointers) sit in one device struct read through scalar loads.
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "../../include/acmmp_detmath.h"
#include "acmmp_internal.h"

namespace acmmp {

#define DEV static __device__ __forceinline__

// Patch geometry of the fast path, the reference defaults (patch_size 11,
// increment 2: offsets {-5,-3,-1,1,3,5}^2, src/ACMMP.h:34,37). The engine
// sends every other geometry to the general kernels (acmmp_general.h).
constexpr int kTaps = 6;

// The kernel shapes below are the measured winners of the A/B experiments
// recorded in DESIGN.md §4 (the rejected variants live in git history only):
// 16 x 16 blocks of four 8 x 8-pixel waves (lanes column-major in 4 x 4
// quarters, lane_geom_of), candidate planes staged in LDS,
// refinement items packed across lanes, two software-pipelined patch rows,
// packed-pair u8 lerps, view selection in registers, 2 waves per SIMD.
constexpr int kWaveRows = 8;    // rows of pixels per wave (lane_geom_of)
constexpr int kSweepWaves = 2;  // __launch_bounds__ waves per SIMD of k_sweep

// ----------------------------------------------------------------- textures
// Through the global address space: a generic (flat) load would also count
// against lgkmcnt, so every later wait for a scalar or LDS load would drain
// it too (the geometric cost's depth fetch could never overlap anything).
typedef const __attribute__((address_space(1))) float gfloat;

DEV float texel(const float *img, int pitch, int W, int H, int x, int y) {
    x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
    y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
    return ((gfloat *)img)[y * pitch + x];
}

// pin P2 (tex2D linear, clamp; src/ACMMP.cu:394)
DEV float bilinear(const float *img, int pitch, int W, int H, float u, float v) {
    float xs = (u + 0.5f) - 0.5f;
    float ys = (v + 0.5f) - 0.5f;
    const float fw = (float)W, fh = (float)H;
    xs = (xs > -1.0f) ? xs : -1.0f;
    xs = (xs < fw) ? xs : fw;
    ys = (ys > -1.0f) ? ys : -1.0f;
    ys = (ys < fh) ? ys : fh;
    const float fx0 = dm_floor(xs), fy0 = dm_floor(ys);
    const float ax = xs - fx0, ay = ys - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int xa = x0 < 0 ? 0 : x0;
    const int xb = (x0 + 1) > (W - 1) ? (W - 1) : (x0 + 1);
    const int ya = y0 < 0 ? 0 : y0;
    const int yb = (y0 + 1) > (H - 1) ? (H - 1) : (y0 + 1);
    const int xa2 = xa > W - 1 ? W - 1 : xa;
    const int ya2 = ya > H - 1 ? H - 1 : ya;
    const int xb2 = xb < 0 ? 0 : xb;
    const int yb2 = yb < 0 ? 0 : yb;
    const float *r0 = img + ya2 * pitch;
    const float *r1 = img + yb2 * pitch;
    const float t00 = r0[xa2], t10 = r0[xb2];
    const float t01 = r1[xa2], t11 = r1[xb2];
    const float top = dm_fma(ax, t10 - t00, t00);
    const float bot = dm_fma(ax, t11 - t01, t01);
    return dm_fma(ay, bot - top, top);
}

// tex2D(depth, (int)x + 0.5, (int)y + 0.5) (src/ACMMP.cu:528)
DEV float tex_trunc(const float *img, int pitch, int W, int H, float u, float v) {
    const float fw = (float)W, fh = (float)H;
    u = (u > -1.0f) ? u : -1.0f;
    u = (u < fw) ? u : fw;
    v = (v > -1.0f) ? v : -1.0f;
    v = (v < fh) ? v : fh;
    return texel(img, pitch, W, H, (int)u, (int)v);
}

// ------------------------------------------------------------ geometry
// Get3DPoint (src/ACMMP.cu:123-128)
DEV void get3d(const acmmp_camera &c, int px, int py, float depth, float *X) {
    X[0] = depth * ((float)px - c.K[2]) / c.K[0];
    X[1] = depth * ((float)py - c.K[5]) / c.K[4];
    X[2] = depth;
}

// GetViewDirection (src/ACMMP.cu:130-142)
DEV float4 view_direction(const acmmp_camera &c, int px, int py, float depth) {
    float X[3];
    get3d(c, px, py, depth, X);
    const float norm = dm_sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
    return make_float4(X[0] / norm, X[1] / norm, X[2] / norm, 0.0f);
}

// GetDistance2Origin (src/ACMMP.cu:144-149)
DEV float distance_to_origin(const acmmp_camera &c, int px, int py, float depth, float4 n) {
    float X[3];
    get3d(c, px, py, depth, X);
    return -(n.x * X[0] + n.y * X[1] + n.z * X[2]);
}

// ComputeDepthfromPlaneHypothesis (src/ACMMP.cu:163-168)
DEV float plane_depth(const acmmp_camera &c, float4 h, int px, int py) {
    return -h.w * c.K[0] /
           (((float)px - c.K[2]) * h.x + (c.K[0] / c.K[4]) * ((float)py - c.K[5]) * h.y + c.K[0] * h.z);
}

// NormalizeVec3 (src/ACMMP.cu:98-105), rsqrt pinned to 1/sqrt
DEV void normalize3(float4 &v) {
    const float n2 = v.x * v.x + v.y * v.y + v.z * v.z;
    const float inv = dm_rsqrt(n2);
    v.x *= inv;
    v.y *= inv;
    v.z *= inv;
}

DEV float dot3(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// TransformNormal cam->world (src/ACMMP.cu:333-341)
DEV float4 to_world(const acmmp_camera &c, float4 h) {
    return make_float4(c.R[0] * h.x + c.R[3] * h.y + c.R[6] * h.z,
                       c.R[1] * h.x + c.R[4] * h.y + c.R[7] * h.z,
                       c.R[2] * h.x + c.R[5] * h.y + c.R[8] * h.z, h.w);
}

// TransformNormal2RefCam world->cam (src/ACMMP.cu:343-351)
DEV float4 to_cam(const acmmp_camera &c, float4 h) {
    return make_float4(c.R[0] * h.x + c.R[1] * h.y + c.R[2] * h.z,
                       c.R[3] * h.x + c.R[4] * h.y + c.R[5] * h.z,
                       c.R[6] * h.x + c.R[7] * h.y + c.R[8] * h.z, h.w);
}

// GenerateRandomNormal (src/ACMMP.cu:170-196)
DEV float4 random_normal(const acmmp_camera &c, int px, int py, dm_rng &rs, float depth) {
    float q1 = 1.0f, q2 = 1.0f, s = 2.0f;
    int guard = 0;
    while (s >= 1.0f && guard < 1000) {
        q1 = 2.0f * dm_rng_uniform(&rs) - 1.0f;
        q2 = 2.0f * dm_rng_uniform(&rs) - 1.0f;
        s = q1 * q1 + q2 * q2;
        ++guard;
    }
    const float sq = dm_sqrt(1.0f - s);
    float4 n = make_float4(2.0f * q1 * sq, 2.0f * q2 * sq, 1.0f - 2.0f * s, 0.0f);
    const float4 vd = view_direction(c, px, py, depth);
    if (n.x * vd.x + n.y * vd.y + n.z * vd.z > 0.0f) {
        n.x = -n.x;
        n.y = -n.y;
        n.z = -n.z;
    }
    normalize3(n);
    return n;
}

// GeneratePerturbedNormal (src/ACMMP.cu:198-233)
DEV float4 perturbed_normal(const acmmp_camera &c, int px, int py, float4 normal, dm_rng &rs,
                            float perturbation) {
    const float4 vd = view_direction(c, px, py, 1.0f);
    const float a1 = (dm_rng_uniform(&rs) - 0.5f) * perturbation;
    const float a2 = (dm_rng_uniform(&rs) - 0.5f) * perturbation;
    const float a3 = (dm_rng_uniform(&rs) - 0.5f) * perturbation;
    const float s1 = dm_sinf(a1), s2 = dm_sinf(a2), s3 = dm_sinf(a3);
    const float c1 = dm_cosf(a1), c2 = dm_cosf(a2), c3 = dm_cosf(a3);
    float R[9];
    R[0] = c2 * c3;
    R[1] = c3 * s1 * s2 - c1 * s3;
    R[2] = s1 * s3 + c1 * c3 * s2;
    R[3] = c2 * s3;
    R[4] = c1 * c3 + s1 * s2 * s3;
    R[5] = c1 * s2 * s3 - c3 * s1;
    R[6] = -s2;
    R[7] = c2 * s1;
    R[8] = c1 * c2;
    float4 np = make_float4(R[0] * normal.x + R[1] * normal.y + R[2] * normal.z,
                            R[3] * normal.x + R[4] * normal.y + R[5] * normal.z,
                            R[6] * normal.x + R[7] * normal.y + R[8] * normal.z, normal.w);
    if (dot3(np, vd) >= 0.0f) np = normal;
    normalize3(np);
    return np;
}

// Exactly rounded 1/z. The IEEE division sequence (v_div_scale / v_rcp /
// 4 fma / v_div_fmas / v_div_fixup) is the pinned semantics. Inside the
// exponent window below the sample loop replaces it by v_rcp_f32 + one fma
// Newton step, which acmmp_selftest_reciprocal() proves bit-identical for
// EVERY float in that window on this hardware.
DEV float recip_newton(float z) {
    const float r = __builtin_amdgcn_rcpf(z);
    const float e = dm_fma(-z, r, 1.0f);
    return dm_fma(e, r, r);
}
DEV bool recip_fast_window(float z) {
    const float az = dm_fabs(z);
    return az >= 0x1p-125f && az < 0x1p125f;
}
DEV float recip_exact(float z) { return 1.0f / z; }


// ------------------------------------------------------ homography + NCC
// ComputeHomography (src/ACMMP.cu:262-322) with the camera-only terms
// precomputed per view (ViewRel) and pin P4.
DEV void homography(const KViews &kv, int v, float4 h, float *H) {
    const ViewRel &r = kv.rel[v];
    const acmmp_camera &rc = kv.cam[0];
    const acmmp_camera &sc = kv.cam[v];
    const float inv_w = 1.0f / h.w;
    float G[9];
    G[0] = r.Rr[0] - (r.tr[0] * h.x) * inv_w;
    G[1] = r.Rr[1] - (r.tr[0] * h.y) * inv_w;
    G[2] = r.Rr[2] - (r.tr[0] * h.z) * inv_w;
    G[3] = r.Rr[3] - (r.tr[1] * h.x) * inv_w;
    G[4] = r.Rr[4] - (r.tr[1] * h.y) * inv_w;
    G[5] = r.Rr[5] - (r.tr[1] * h.z) * inv_w;
    G[6] = r.Rr[6] - (r.tr[2] * h.x) * inv_w;
    G[7] = r.Rr[7] - (r.tr[2] * h.y) * inv_w;
    G[8] = r.Rr[8] - (r.tr[2] * h.z) * inv_w;
    const float ik0 = kv.inv_k0, ik4 = kv.inv_k4;
    float t[9];
    t[0] = G[0] * ik0;
    t[1] = G[1] * ik4;
    t[2] = ((-G[0] * rc.K[2]) * ik0 - (G[1] * rc.K[5]) * ik4) + G[2];
    t[3] = G[3] * ik0;
    t[4] = G[4] * ik4;
    t[5] = ((-G[3] * rc.K[2]) * ik0 - (G[4] * rc.K[5]) * ik4) + G[5];
    t[6] = G[6] * ik0;
    t[7] = G[7] * ik4;
    t[8] = ((-G[6] * rc.K[2]) * ik0 - (G[7] * rc.K[5]) * ik4) + G[8];
    H[0] = sc.K[0] * t[0] + sc.K[2] * t[6];
    H[1] = sc.K[0] * t[1] + sc.K[2] * t[7];
    H[2] = sc.K[0] * t[2] + sc.K[2] * t[8];
    H[3] = sc.K[4] * t[3] + sc.K[5] * t[6];
    H[4] = sc.K[4] * t[4] + sc.K[5] * t[7];
    H[5] = sc.K[4] * t[5] + sc.K[5] * t[8];
    H[6] = sc.K[8] * t[6];
    H[7] = sc.K[8] * t[7];
    H[8] = sc.K[8] * t[8];
}

// ComputeCorrespondingPoint (src/ACMMP.cu:324-331), pin P1
DEV float2 project(const float *H, float x, float y) {
    const float px = dm_fma(H[1], y, dm_fma(H[0], x, H[2]));
    const float py = dm_fma(H[4], y, dm_fma(H[3], x, H[5]));
    const float pz = dm_fma(H[7], y, dm_fma(H[6], x, H[8]));
    const float inv = recip_exact(pz);
    return make_float2(px * inv, py * inv);
}

// Texel modes of the gather kernels (template parameter TX):
//   bit 0 (kTxWide): record index by integer multiply-add (views of 2^24+
//          records), else exactly in fp32;
//   bit 1 (kTxU8):   the padded source views hold u8 texel quads (every view
//          of the problem is integer-valued in [0, 255], which 8-bit JPEG
//          input at native size is): one 4-byte record per bilinear
//          footprint instead of 16 bytes; v_cvt_f32_ubyte* restores the exact
//          fp32 texel values, so the arithmetic is unchanged.
//   bit 2 (kTxH16):  the padded source views hold f16 "difference quads"
//          (t00, t01, t10 - t00, t11 - t01) for views whose every stored value
//          is exact in f16 (8-bit input is): 8 bytes per footprint, and the
//          two row lerps are v_fma_mix_f32 straight from the f16 halves (the
//          f16 -> f32 widening is exact, the fma is the pinned fp32 fma).
//   bit 3 (kTxFrac8): acmmp_params::texture_filter8 — the bilinear fractions
//                    rounded to the CUDA texture unit's 1.8 fixed point
//                    (instantiated for the non-wide u8 and fp32 forms)
constexpr int kTxWide = 1, kTxU8 = 2, kTxH16 = 4, kTxFrac8 = 8;

// Source-image sampler: one buffer resource (SRD) per view over the padded
// copy (KViews::pad), built from wave-uniform values (the view index is a
// uniform loop counter) so the loads are index-addressed (`idxen`) buffer
// loads with the record stride in the descriptor.
struct SrcImage {
    __amdgpu_buffer_rsrc_t rsrc;
    int pitch, W, H;
    float fpitch, fp1;  // pitch and pitch + 1 as floats (exact: < 2^24)
};

template <int TX>
DEV SrcImage src_image(const KViews &kv, int v) {
    SrcImage s;
    s.pitch = kv.ppitch[v];
    s.W = kv.cam[v].width;
    s.H = kv.cam[v].height;
    // structured view, indexed loads (idxen): 8-byte records (one fp32 row
    // pair) or 4-byte records (one u8 2x2 quad)
    s.rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)kv.pad[v], (short)((TX & kTxU8) ? 4 : 8), s.pitch * (s.H + 2),
                                               0x00020000);
    s.fp1 = (float)(s.pitch + 1);
    s.fpitch = (float)s.pitch;
    return s;
}


typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------- ref-image tile
// A block covers kBX colour-split columns (k0..k0+kBX-1) x kBY rows of ONE
// colour c (256 threads). Both patch offsets i, j are odd, so every
// reference sample of a colour-c pixel is itself a colour-c pixel: the
// block's whole reference footprint is a (kBX + 6) x (kBY + 10) window of the
// colour-c plane, staged once in LDS (clamp-to-edge baked in); the address
// of a sample is a compile-time offset from the lane's base.
//
// kBX = 16 colour-split columns x 16 rows packs a block's four waves (8 x 8
// colour-split pixels each, kWaveRows) 2 x 2, so they share most
// source-view rows of their patches in the CU's L1, and keeps the ragged
// last block column narrow (Wh = 800 at 1600 px: 50 x 75 blocks). cfg2, ms
// per k_sweep launch (profiles/r02_block_shape.md): 64 x 4 blocks of
// 16 x 4 waves 4.66, 32 x 8 4.41, 16 x 16 4.28, 16 x 16 of 8 x 8 waves
// 4.19, 8 x 32 4.18.
constexpr int kBX = 16, kBY = 16;
constexpr int kTileW = kBX + 6, kTileH = kBY + 10;

DEV void load_ref_tile(const KViews &kv, float *tile, int k0, int y0, int colour) {
    const float *img = kv.img[0];
    const int pitch = kv.ipitch[0], W = kv.W, H = kv.H;
    // all of a thread's texels loaded before any is stored; a thread past the
    // end repeats the last element (same value, same address), so no load
    // sits in a conditional block waited on alone
    constexpr int kN = kTileW * kTileH, kIt = (kN + kBX * kBY - 1) / (kBX * kBY);
    float v[kIt];
    int at[kIt];
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
        int e = threadIdx.y * kBX + threadIdx.x + it * kBX * kBY;
        e = e < kN ? e : kN - 1;
        const int r = e / kTileW, kk = e - r * kTileW;
        const int yy = y0 - 5 + r;
        const int kc = k0 - 3 + kk;
        const int par = (yy + colour) & 1;
        const int xx = 2 * kc + par;
        at[it] = e;
        v[it] = texel(img, pitch, W, H, xx, yy);
    }
#pragma unroll
    for (int it = 0; it < kIt; ++it) tile[at[it]] = v[it];
}

// Reference-side invariants of ComputeBilateralNCC (src/ACMMP.cu:372-421):
// the 36 bilateral weights (ComputeBilateralWeight :353-358) and the
// normalised ref mean / variance — identical for all 14*(N-1) calls of a
// pixel-iteration, so computed once (same operations, same order).
//
// The source side of the NCC runs on PAIRS of patch columns (2p, 2p+1) held
// as packed-FP32 lanes (SoA): one v_pk_* instruction does the same IEEE
// operation for both samples of a pair, and the pair's weights come from LDS
// as one float2 (w_a, w_b), the reference pair from the tile, so no register
// shuffling is needed to feed the packed ops. LDS slot of (column pair p,
// patch row jj): jj * 3 + p, in the order the row loop reads them.
constexpr int kPairs = kTaps / 2;
constexpr int kSlots = kPairs * kTaps;
DEV int wslot(int p, int jj) { return jj * kPairs + p; }
typedef float2 WSlot;

struct PixPatch {
    WSlot *w;        // LDS: slot k of this lane at [k * kThreads]
    const float *rt; // LDS: this lane's first reference sample in the tile (tile + tb)
    int wo;          // this lane's offset into the weight array (w = wbase + wo)
    float mean;      // sum_ref * inv_bilateral_weight_sum
    float var;       // var_ref
    float inv_wsum;  // inv_bilateral_weight_sum
};

// 18 float2 rows of 256 lanes: 36 KB + the 3.9 KB tile per 256-thread block,
// so four blocks (16 waves) fit a CU's 160 KB of LDS. A wave's read of one
// slot is a conflict-free ds_read_b64 and costs no VGPRs between NCC calls;
// the matching reference pair comes from the tile (ds_read2_b32).
constexpr int kThreads = kBX * kBY;

DEV float bilateral_weight(float xd, float yd, float pix, float cpix, float ss, float sc) {
    const float spatial = dm_sqrt(xd * xd + yd * yd);
    const float color = dm_fabs(pix - cpix);
    return dm_expf(-spatial / (2.0f * ss * ss) - color / (2.0f * sc * sc));
}

// The bilateral-weight table (KViews::wlut) staged in LDS by the block
// (kernels of the u8 texel form, whose reference texels are all integers in
// [0, 255]); the caller's __syncthreads publishes it.
DEV void load_wlut(const KViews &kv, float *wl) {
    const int t = threadIdx.y * kBX + threadIdx.x;
    for (int i = t; i < kWlutClasses * 256; i += kBX * kBY) wl[i] = (&kv.wlut[0][0])[i];
}

// tb = tile index of sample (ii=0, jj=0) of this lane: ty*kTileW + tx + s.
// wlut: the LDS weight table (u8 texel form) or nullptr (weights computed).
DEV void pixel_patch(const KViews &kv, const float *tile, int tb, int s, PixPatch &pp, const float *wlut = nullptr) {
    const float ss = kv.prm.sigma_spatial, sc = kv.prm.sigma_color;
    const float center = tile[tb - s + 5 * kTileW + 3];
    float sum_ref = 0.0f, sum_rr = 0.0f, bw = 0.0f;
#pragma unroll
    for (int ii = 0; ii < kTaps; ++ii) {
        float r_ref = 0.0f, r_rr = 0.0f, r_w = 0.0f;
#pragma unroll
        for (int jj = 0; jj < kTaps; ++jj) {
            const float r = tile[tb + ii + 2 * kTileW * jj];
            // |I - I_c| of integer texels in [0, 255]: the table holds the
            // weight this expression gives for it (bit-identical)
            const float w = wlut ? wlut[wlut_class((ii < 3 ? 5 - 2 * ii : 2 * ii - 5) / 2,
                                                   (jj < 3 ? 5 - 2 * jj : 2 * jj - 5) / 2) * 256 +
                                        (int)dm_fabs(r - center)]
                                 : bilateral_weight((float)(-5 + 2 * ii), (float)(-5 + 2 * jj), r, center, ss, sc);
            const float wr = w * r;
            r_ref = dm_fma(w, r, r_ref);  // nvcc's contraction of `sum += w * r` (pin P3)
            r_rr = dm_fma(wr, r, r_rr);
            r_w += w;
            float *slot = reinterpret_cast<float *>(&pp.w[wslot(ii >> 1, jj) * kThreads]);
            slot[ii & 1] = w;
        }
        sum_ref += r_ref;
        sum_rr += r_rr;
        bw += r_w;
    }
    const float inv = 1.0f / bw;
    sum_ref *= inv;
    pp.mean = sum_ref;
    pp.var = dm_fma(sum_rr, inv, -(sum_ref * sum_ref));  // `rr * inv - m * m` contracted (pin P3)
    pp.inv_wsum = inv;
}

typedef float f2v __attribute__((ext_vector_type(2)));
// texture_filter8: a bilinear fraction in [0, 1) rounded to the texture
// unit's 1.8 fixed point (1/256 steps, 1.0 representable), exactly: x * 256
// and the scale back are exact, rint is round-half-even.
DEV f2v frac8(f2v a) {
    return f2v{__builtin_rintf(a.x * 256.0f), __builtin_rintf(a.y * 256.0f)} * 0.00390625f;
}
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// llvm.amdgcn.struct.ptr.buffer.load: the idxen form of buffer_load
// (address = base + vindex * stride + voffset); clang has no builtin for it.
__device__ u32x4 amdgcn_struct_buffer_load_b128(__amdgpu_buffer_rsrc_t rsrc, int vindex, int voffset, int soffset,
                                                int aux) __asm("llvm.amdgcn.struct.ptr.buffer.load.v4i32");
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
__device__ u32x2 amdgcn_struct_buffer_load_b64(__amdgpu_buffer_rsrc_t rsrc, int vindex, int voffset, int soffset,
                                               int aux) __asm("llvm.amdgcn.struct.ptr.buffer.load.v2i32");
__device__ unsigned amdgcn_struct_buffer_load_b32(__amdgpu_buffer_rsrc_t rsrc, int vindex, int voffset, int soffset,
                                                  int aux) __asm("llvm.amdgcn.struct.ptr.buffer.load.i32");

DEV f2v fma2(f2v a, f2v b, f2v c) { return __builtin_elementwise_fma(a, b, c); }
DEV f2v splat(float v) { return f2v{v, v}; }

// Bilinear value of one fetched sample t = (t00, t01, t10, t11) (pin P2's
// lerp order): top = fma(ax, t10 - t00, t00), bot = fma(ax, t11 - t01, t01)
// as one packed pair, then fma(ay, bot - top, top).
DEV float lerp_sample(u32x4 t, float ax, float ay) {
    const f2v lo = f2v{__uint_as_float(t.x), __uint_as_float(t.y)};
    const f2v hi = f2v{__uint_as_float(t.z), __uint_as_float(t.w)};
    const f2v tb = fma2(splat(ax), hi - lo, lo);
    return dm_fma(ay, tb.y - tb.x, tb.x);
}

// One patch row's gathers in flight: the fetched footprints (in the form
// of TX) and the bilinear fractions of the row's 6 samples.
template <int TX>
struct RowFetch {
    u32x4 t[kTaps];   // fp32 row pairs
    unsigned q[kTaps];  // u8 quads
    u32x2 hq[kTaps];  // f16 difference quads
    f2v ax[kPairs], ay[kPairs];
};

// Projection, clamp, fractions and record index of patch row jj, and its 6
// loads issued (not waited for).
template <bool FAST, int TX>
DEV void fetch_row(const SrcImage &im, const float *H, const f2v *cx, const f2v *cy, const f2v *cz, int py, int jj,
                   RowFetch<TX> &rf) {
    constexpr bool WIDE = (TX & kTxWide) != 0, U8 = (TX & kTxU8) != 0, H16 = (TX & kTxH16) != 0;
    constexpr bool F8 = (TX & kTxFrac8) != 0;
    const f2v fw = splat((float)im.W), fh = splat((float)im.H);
    const f2v y = splat((float)(py - 5 + 2 * jj));
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
        const f2v hx = fma2(splat(H[1]), y, cx[p]);
        const f2v hy = fma2(splat(H[4]), y, cy[p]);
        const f2v hz = fma2(splat(H[7]), y, cz[p]);
        f2v inv;
        if (FAST) {  // v_rcp + one Newton step == IEEE 1/z in the window
            const f2v r = f2v{__builtin_amdgcn_rcpf(hz.x), __builtin_amdgcn_rcpf(hz.y)};
            inv = fma2(fma2(-hz, r, splat(1.0f)), r, r);
        } else {
            inv = f2v{1.0f / hz.x, 1.0f / hz.y};
        }
        f2v u = hx * inv, v = hy * inv;
        u = (u + 0.5f) - 0.5f;
        v = (v + 0.5f) - 0.5f;
        // clamp to [-1, W] x [-1, H]. FAST: every value is finite or +-inf
        // (finite homography, |hz| inside the reciprocal window), where
        // v_med3 equals max-then-min. Otherwise v_max/v_min (NaN -> -1;
        // bounds are never +-0) == the oracle's selects.
        f2v xs, ys;
        if (FAST) {
            xs = f2v{__builtin_amdgcn_fmed3f(u.x, -1.0f, fw.x), __builtin_amdgcn_fmed3f(u.y, -1.0f, fw.x)};
            ys = f2v{__builtin_amdgcn_fmed3f(v.x, -1.0f, fh.x), __builtin_amdgcn_fmed3f(v.y, -1.0f, fh.x)};
        } else {
            xs = f2v{fminf(fmaxf(u.x, -1.0f), fw.x), fminf(fmaxf(u.y, -1.0f), fw.x)};
            ys = f2v{fminf(fmaxf(v.x, -1.0f), fh.x), fminf(fmaxf(v.y, -1.0f), fh.x)};
        }
        const f2v flx = f2v{dm_floor(xs.x), dm_floor(xs.y)};
        const f2v fly = f2v{dm_floor(ys.x), dm_floor(ys.y)};
        rf.ax[p] = xs - flx;
        rf.ay[p] = ys - fly;
        if (F8) {
            rf.ax[p] = frac8(rf.ax[p]);
            rf.ay[p] = frac8(rf.ay[p]);
        }
        // record index (y0 + 1) * pitch + x0 + 1
        unsigned ia, ib;
        if (!WIDE) {
            // = fma(y0, pitch, x0 + pitch + 1): integers below 2^24, so
            // exact in fp32 (the engine selects WIDE otherwise)
            const f2v idx = fma2(fly, splat(im.fpitch), flx + im.fp1);
            ia = (unsigned)idx.x;
            ib = (unsigned)idx.y;
        } else {
            // views of 2^24 records or more: integer multiply-add (24-bit
            // operands, 32-bit result)
            const f2v q = flx + 1.0f, r = fly + 1.0f;
            ia = __umul24((unsigned)r.x, (unsigned)im.pitch) + (unsigned)q.x;
            ib = __umul24((unsigned)r.y, (unsigned)im.pitch) + (unsigned)q.y;
        }
        if (H16) {
            rf.hq[2 * p] = amdgcn_struct_buffer_load_b64(im.rsrc, (int)ia, 0, 0, 0);
            rf.hq[2 * p + 1] = amdgcn_struct_buffer_load_b64(im.rsrc, (int)ib, 0, 0, 0);
        } else if (U8) {
            rf.q[2 * p] = amdgcn_struct_buffer_load_b32(im.rsrc, (int)ia, 0, 0, 0);
            rf.q[2 * p + 1] = amdgcn_struct_buffer_load_b32(im.rsrc, (int)ib, 0, 0, 0);
        } else {
            rf.t[2 * p] = amdgcn_struct_buffer_load_b128(im.rsrc, (int)ia, 0, 0, 0);
            rf.t[2 * p + 1] = amdgcn_struct_buffer_load_b128(im.rsrc, (int)ib, 0, 0, 0);
        }
    }
}

// Bilinear values of a fetched row and their weighted sums into the
// per-column accumulators (w from the LDS weight slots, ref from the tile).
template <int TX>
DEV void reduce_row(const RowFetch<TX> &rf, const WSlot *wl, const float *rt, int wstride, int jj, f2v *acc_s,
                    f2v *acc_ss, f2v *acc_rs) {
    constexpr bool U8 = (TX & kTxU8) != 0, H16 = (TX & kTxH16) != 0;
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
        f2v sv;
        if (H16) {
            // row lerps fma(ax, t1x - t0x, t0x) as v_fma_mix_f32 on the
            // halves, then the column lerp of both samples packed (words
            // copied out first: clang's __builtin_bit_cast of a
            // vector-element lvalue reads element 0)
            const unsigned wa0 = rf.hq[2 * p].x, wa1 = rf.hq[2 * p].y;
            const unsigned wb0 = rf.hq[2 * p + 1].x, wb1 = rf.hq[2 * p + 1].y;
            const h2v ta = __builtin_bit_cast(h2v, wa0), da = __builtin_bit_cast(h2v, wa1);
            const h2v tb = __builtin_bit_cast(h2v, wb0), db = __builtin_bit_cast(h2v, wb1);
            const f2v r0 = f2v{__builtin_fmaf(rf.ax[p].x, (float)da.x, (float)ta.x),
                               __builtin_fmaf(rf.ax[p].y, (float)db.x, (float)tb.x)};
            const f2v r1 = f2v{__builtin_fmaf(rf.ax[p].x, (float)da.y, (float)ta.y),
                               __builtin_fmaf(rf.ax[p].y, (float)db.y, (float)tb.y)};
            sv = fma2(rf.ay[p], r1 - r0, r0);
        } else if (U8) {
            // lerp_sample's operations with the pair's two samples in the two
            // components (sample a in .x, b in .y, as ax / ay already are):
            // top = fma(ax, t10 - t00, t00), bot = fma(ax, t11 - t01, t01),
            // fma(ay, bot - top, top) — 6 packed ops per pair instead of 8
            const unsigned qa = rf.q[2 * p], qb = rf.q[2 * p + 1];
            const f2v t00 = f2v{(float)(qa & 0xffu), (float)(qb & 0xffu)};
            const f2v t01 = f2v{(float)((qa >> 8) & 0xffu), (float)((qb >> 8) & 0xffu)};
            const f2v t10 = f2v{(float)((qa >> 16) & 0xffu), (float)((qb >> 16) & 0xffu)};
            const f2v t11 = f2v{(float)(qa >> 24), (float)(qb >> 24)};
            const f2v top = fma2(rf.ax[p], t10 - t00, t00);
            const f2v bot = fma2(rf.ax[p], t11 - t01, t01);
            sv = fma2(rf.ay[p], bot - top, top);
        } else {
            sv = f2v{lerp_sample(rf.t[2 * p], rf.ax[p].x, rf.ay[p].x),
                     lerp_sample(rf.t[2 * p + 1], rf.ax[p].y, rf.ay[p].y)};
        }
        // w from the weight slots, ref from the tile: w * ref is the same
        // IEEE product pixel_patch formed, so re-forming it is exact
        const WSlot w = wl[wslot(p, jj) * wstride];
        const float *rr = rt + 2 * kTileW * jj + 2 * p;
        const f2v wv = f2v{w.x, w.y};
        const f2v wr = wv * f2v{rr[0], rr[1]};
        const f2v ws = wv * sv;
        acc_s[p] = fma2(wv, sv, acc_s[p]);  // `sum += w * s` contracted (pin P3)
        acc_ss[p] = fma2(ws, sv, acc_ss[p]);
        acc_rs[p] = fma2(wr, sv, acc_rs[p]);
    }
}

// Source-sample reduction of ComputeBilateralNCC (src/ACMMP.cu:382-412).
//
// Per sample: projection (pin P1, the x-terms hoisted per column), the
// coordinate clamp of pin P2, and ONE load of the 2x2 bilinear footprint
// from the padded source view (KViews::pad) at record (y0 + 1, x0 + 1).
//
// Rows are gathered one at a time (a lane's 6 samples of a row sit in the
// same one or two cache lines) and accumulated into per-column partial
// sums: within a column the rows are still added in order jj = 0..5,
// columns are summed at the end in order ii — the pinned order
// (src/ACMMP.cu:382-412). The row loop is software-pipelined: row jj + 1's
// loads are issued before row jj is reduced, so a row's gather latency
// overlaps the previous row's arithmetic.
template <bool FAST, int TX>
DEV void ncc_sums_rows(const SrcImage &im, const float *H, const WSlot *wl, const float *rt, int wstride, int px,
                       int py, float &sum_src, float &sum_ss, float &sum_rs) {
    f2v cx[kPairs], cy[kPairs], cz[kPairs];
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
        const f2v x = f2v{(float)(px - 5 + 4 * p), (float)(px - 3 + 4 * p)};
        cx[p] = fma2(splat(H[0]), x, splat(H[2]));
        cy[p] = fma2(splat(H[3]), x, splat(H[5]));
        cz[p] = fma2(splat(H[6]), x, splat(H[8]));
    }
    f2v acc_s[kPairs], acc_ss[kPairs], acc_rs[kPairs];
#pragma unroll
    for (int p = 0; p < kPairs; ++p) acc_s[p] = acc_ss[p] = acc_rs[p] = splat(0.0f);
    // two rows per trip (ping-pong fetch buffers, no register copies)
    RowFetch<TX> ra, rb;
    fetch_row<FAST, TX>(im, H, cx, cy, cz, py, 0, ra);
#pragma unroll 1
    for (int jj = 0; jj < kTaps; jj += 2) {
        fetch_row<FAST, TX>(im, H, cx, cy, cz, py, jj + 1, rb);
        reduce_row<TX>(ra, wl, rt, wstride, jj, acc_s, acc_ss, acc_rs);
        if (jj + 2 < kTaps) fetch_row<FAST, TX>(im, H, cx, cy, cz, py, jj + 2, ra);
        reduce_row<TX>(rb, wl, rt, wstride, jj + 1, acc_s, acc_ss, acc_rs);
    }
    sum_src = 0.0f;
    sum_ss = 0.0f;
    sum_rs = 0.0f;
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
        sum_src += acc_s[p].x;
        sum_src += acc_s[p].y;
        sum_ss += acc_ss[p].x;
        sum_ss += acc_ss[p].y;
        sum_rs += acc_rs[p].x;
        sum_rs += acc_rs[p].y;
    }
}

// Source-sample reduction of ComputeBilateralNCC (src/ACMMP.cu:382-412):
// returns the three weighted sums (ncc_sums_rows above).
template <bool FAST, int TX>
DEV void ncc_sums(const SrcImage &im, const float *H, const PixPatch &pp, int px, int py, float &sum_src,
                  float &sum_ss, float &sum_rs) {
    // re-read weights from LDS each call rather than caching them in VGPRs
    // (launder the integer offset, not the pointer, so the LDS address space
    // stays visible and the reads are ds_read, not flat)
    int wo = pp.wo;
    asm volatile("" : "+v"(wo));
    const WSlot *wl = pp.w - pp.wo + wo;
    ncc_sums_rows<FAST, TX>(im, H, wl, pp.rt, kThreads, px, py, sum_src, sum_ss, sum_rs);
}

constexpr float kNccCostMax = 2.0f, kNccMinVar = 1e-5f;

// ComputeBilateralNCC (src/ACMMP.cu:360-432) for source view v (1-based,
// wave-uniform). Reference samples come from the LDS tile, source samples
// through ncc_sums.
template <int TX>
DEV float bilateral_ncc(const KViews &kv, const PixPatch &pp, int v, int px, int py, float4 h) {
    const float cost_max = kNccCostMax;
    const float kMinVar = kNccMinVar;
    // var_ref is invariant: when it is below kMinVar (or the centre maps
    // outside the source) every call returns cost_max.
    if (pp.var < kMinVar) return cost_max;
    const SrcImage im = src_image<TX>(kv, v);
    float H[9];
    homography(kv, v, h, H);
    const float2 pt = project(H, (float)px, (float)py);
    if (pt.x >= (float)im.W || pt.x < 0.0f || pt.y >= (float)im.H || pt.y < 0.0f) return cost_max;
    float sum_src, sum_ss, sum_rs;
    // hz is affine in the sample position, so its values over the patch lie
    // between the four corner values (up to rounding: the window test uses a
    // 2x margin). Inside the window the Newton reciprocal is bit-identical to
    // IEEE 1/z (exhaustive proof: acmmp_selftest_reciprocal).
    const float xl = (float)(px - 5), xr = (float)(px + 5), yt = (float)(py - 5), yb = (float)(py + 5);
    const float z00 = dm_fma(H[7], yt, dm_fma(H[6], xl, H[8]));
    const float z10 = dm_fma(H[7], yt, dm_fma(H[6], xr, H[8]));
    const float z01 = dm_fma(H[7], yb, dm_fma(H[6], xl, H[8]));
    const float z11 = dm_fma(H[7], yb, dm_fma(H[6], xr, H[8]));
    const float zmin = fminf(fminf(z00, z10), fminf(z01, z11));
    const float zmax = fmaxf(fmaxf(z00, z10), fmaxf(z01, z11));
    const bool fast = (zmin >= 0x1p-124f && zmax < 0x1p124f) || (zmax <= -0x1p-124f && zmin > -0x1p124f);
    if (fast) ncc_sums<true, TX>(im, H, pp, px, py, sum_src, sum_ss, sum_rs);
    else ncc_sums<false, TX>(im, H, pp, px, py, sum_src, sum_ss, sum_rs);
    sum_src *= pp.inv_wsum;
    const float var_src = dm_fma(sum_ss, pp.inv_wsum, -(sum_src * sum_src));  // pin P3
    if (var_src < kMinVar) return cost_max;
    const float covar = dm_fma(sum_rs, pp.inv_wsum, -(pp.mean * sum_src));
    const float var_rs = dm_sqrt(pp.var * var_src);
    float c = 1.0f - covar / var_rs;
    c = (c < cost_max) ? c : cost_max;
    c = (c > 0.0f) ? c : 0.0f;
    return c;
}

// ComputeMultiViewInitialCostandSelectedViews (src/ACMMP.cu:434-471)
template <int NS, typename P>
DEV float initial_cost(const KViews &kv, const typename P::Pix &pp, int px, int py, float4 h, uint32_t &sel) {
    const int nsrc = kv.nsrc;
    float cv[NS];
    float cs[NS];
    int num_valid = 0;
    for (int i = 0; i < nsrc; ++i) {
        const float c = P::ncc(kv, pp, i + 1, px, py, h);
        cv[i] = c;
        cs[i] = c;
        if (c < 2.0f) num_valid++;
    }
    for (int i = 1; i < nsrc; i++) {  // sort_small (src/ACMMP.cu:24-33)
        const float tmp = cs[i];
        int j;
        for (j = i; j >= 1 && tmp < cs[j - 1]; j--) cs[j] = cs[j - 1];
        cs[j] = tmp;
    }
    sel = 0;
    const int top_k = num_valid < kv.prm.top_k ? num_valid : kv.prm.top_k;
    if (top_k > 0) {
        float cost = 0.0f;
        for (int i = 0; i < top_k; ++i) cost += cs[i];
        const float thr = cs[top_k - 1];
        for (int i = 0; i < nsrc; ++i)
            if (cv[i] <= thr) sel |= (1u << i);
        return cost / (float)top_k;
    }
    return 2.0f;
}

// ComputeGeomConsistencyCost (src/ACMMP.cu:518-543), split so the view-
// independent half is formed once per hypothesis: geom_ref is the world
// point of the hypothesis at the pixel (ComputeDepthfromPlaneHypothesis +
// Get3DPointonWorld_cu :480-504), geom_cost_at projects it into source v,
// fetches the source depth and measures the reprojection error. Same
// operations in the same order as the unsplit function (the camera offsets
// -(R^T t) come precomputed in KViews::cw, formed by the same expression).
struct GeomRef {
    float Wp[3];
};

// -(R^T t) of camera v, component k. The product takes it from KViews::cw
// (formed on the host by the same expression: bit-identical without
// contraction); the fidelity-study build (ACMMP_CUDA_NUMERICS) forms it here
// so the device's FMA contraction and FTZ apply to it as nvcc's --fmad does
// to Get3DPointonWorld_cu (src/ACMMP.cu:490-504).
DEV float cam_offset(const KViews &kv, int v, int k) {
#ifdef ACMMP_CUDA_NUMERICS
    const acmmp_camera &c = kv.cam[v];
    return -(c.R[k] * c.t[0] + c.R[3 + k] * c.t[1] + c.R[6 + k] * c.t[2]);
#else
    return kv.cw[v][k];
#endif
}

DEV GeomRef geom_ref(const KViews &kv, float4 h, int px, int py) {
    const acmmp_camera &rc = kv.cam[0];
    const float depth = plane_depth(rc, h, px, py);
    float X[3];
    X[0] = depth * ((float)px - rc.K[2]) / rc.K[0];
    X[1] = depth * ((float)py - rc.K[5]) / rc.K[4];
    X[2] = depth;
    GeomRef g;
    g.Wp[0] = (rc.R[0] * X[0] + rc.R[3] * X[1] + rc.R[6] * X[2]) + cam_offset(kv, 0, 0);
    g.Wp[1] = (rc.R[1] * X[0] + rc.R[4] * X[1] + rc.R[7] * X[2]) + cam_offset(kv, 0, 1);
    g.Wp[2] = (rc.R[2] * X[0] + rc.R[5] * X[1] + rc.R[8] * X[2]) + cam_offset(kv, 0, 2);
    return g;
}

// geom_cost_at in two halves, so a caller can issue the source-depth
// fetches of several views (or one ahead of an NCC) before it consumes them:
// geom_fetch projects into source v and loads the depth (always in bounds:
// tex_trunc clamps, NaN included), geom_finish is the rest.
struct GeomFetch {
    float sx, sy, dep;
};

DEV GeomFetch geom_fetch(const KViews &kv, int v, const GeomRef &g) {
    const acmmp_camera &sc = kv.cam[v];
    const float *Wp = g.Wp;
    // ProjectonCamera_cu (:506-516)
    float T[3];
    T[0] = sc.R[0] * Wp[0] + sc.R[1] * Wp[1] + sc.R[2] * Wp[2] + sc.t[0];
    T[1] = sc.R[3] * Wp[0] + sc.R[4] * Wp[1] + sc.R[5] * Wp[2] + sc.t[1];
    T[2] = sc.R[6] * Wp[0] + sc.R[7] * Wp[1] + sc.R[8] * Wp[2] + sc.t[2];
    const float sd = sc.K[6] * T[0] + sc.K[7] * T[1] + sc.K[8] * T[2];
    GeomFetch f;
    f.sx = (sc.K[0] * T[0] + sc.K[1] * T[1] + sc.K[2] * T[2]) / sd;
    f.sy = (sc.K[3] * T[0] + sc.K[4] * T[1] + sc.K[5] * T[2]) / sd;
    f.dep = tex_trunc(kv.dep[v], kv.dpitch[v], kv.dw[v], kv.dh[v], f.sx, f.sy);
    return f;
}

DEV float geom_finish(const KViews &kv, int v, const GeomFetch &f, int px, int py) {
    const float max_cost = 3.0f;
    const acmmp_camera &rc = kv.cam[0];
    const acmmp_camera &sc = kv.cam[v];
    const float sx = f.sx, sy = f.sy, src_depth = f.dep;
    if (src_depth == 0.0f) return max_cost;
    float Y[3];
    Y[0] = src_depth * (sx - sc.K[2]) / sc.K[0];
    Y[1] = src_depth * (sy - sc.K[5]) / sc.K[4];
    Y[2] = src_depth;
    float Wq[3];
    Wq[0] = (sc.R[0] * Y[0] + sc.R[3] * Y[1] + sc.R[6] * Y[2]) + cam_offset(kv, v, 0);
    Wq[1] = (sc.R[1] * Y[0] + sc.R[4] * Y[1] + sc.R[7] * Y[2]) + cam_offset(kv, v, 1);
    Wq[2] = (sc.R[2] * Y[0] + sc.R[5] * Y[1] + sc.R[8] * Y[2]) + cam_offset(kv, v, 2);
    float U[3];
    U[0] = rc.R[0] * Wq[0] + rc.R[1] * Wq[1] + rc.R[2] * Wq[2] + rc.t[0];
    U[1] = rc.R[3] * Wq[0] + rc.R[4] * Wq[1] + rc.R[5] * Wq[2] + rc.t[1];
    U[2] = rc.R[6] * Wq[0] + rc.R[7] * Wq[1] + rc.R[8] * Wq[2] + rc.t[2];
    const float rd = rc.K[6] * U[0] + rc.K[7] * U[1] + rc.K[8] * U[2];
    const float bx = (rc.K[0] * U[0] + rc.K[1] * U[1] + rc.K[2] * U[2]) / rd;
    const float by = (rc.K[3] * U[0] + rc.K[4] * U[1] + rc.K[5] * U[2]) / rd;
    const float dc = (float)px - bx;
    const float dr = (float)py - by;
    const float e = dm_sqrt(dc * dc + dr * dr);
    return (e < max_cost) ? e : max_cost;
}

DEV float geom_cost_at(const KViews &kv, int v, const GeomRef &g, int px, int py) {
    return geom_finish(kv, v, geom_fetch(kv, v, g), px, py);
}

DEV float geom_cost(const KViews &kv, int v, float4 h, int px, int py) {
    return geom_cost_at(kv, v, geom_ref(kv, h, px, py), px, py);
}

DEV dm_rng make_rng(const KViews &kv, int center, uint32_t phase) {
    dm_rng g;
    g.k0 = kv.prm.seed_lo;
    g.k1 = kv.prm.seed_hi;
    g.pix = (uint32_t)center;
    g.phase = phase;
    g.stream = kv.prm.rng_stream;
    g.draw = 0;
    g.blk = dm_u32x4{0u, 0u, 0u, 0u};
    return g;
}

DEV int cs_index(const KViews &kv, int x, int y) { return y * kv.Wh + (x >> 1); }

// SpatialGauss / RangeGauss (src/ACMMP.cu:151-161), pow(v,2) pinned to v*v.
DEV float spatial_gauss(float x1, float y1, float x2, float y2, float sigma) {
    const float dis = (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) - 0.0f;
    return dm_expf((float)(-1.0 * (double)dis / (double)(2 * sigma * sigma)));
}
DEV float range_gauss(float x, float sigma) {
    const float xp = x - 0.0f;
    return dm_expf((float)(-1.0 * (double)(xp * xp) / (double)(2 * sigma * sigma)));
}

// upscale_normal (src/ACMMP.cu:548-607)
DEV float4 upscale_normal(const KViews &kv, const KState &st, int px, int py, float sigmad,
                          float sigmar, int nn, float o_y, float o_x, float refPix, float &cost_out) {
    const int scols = (int)kv.prm.scaled_cols, srows = (int)kv.prm.scaled_rows;
    float c_total = 0.0f, norm = 0.0f;
    float4 n_total = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int j = -nn; j <= nn; ++j) {
        int r_y = (int)(o_y + (float)j);
        r_y = (r_y > 0 ? (r_y < srows ? r_y : srows - 1) : 0);
        const int r_ys = py + j;
        for (int i = -nn; i <= nn; ++i) {
            int r_x = (int)(o_x + (float)i);
            r_x = (r_x > 0 ? (r_x < scols ? r_x : scols - 1) : 0);
            const float4 sn = st.scaled[r_y * scols + r_x];
            const float nb = texel(kv.img[0], kv.ipitch[0], kv.W, kv.H, px + i, r_ys);
            const float tg = spatial_gauss(o_x, o_y, (float)r_x, (float)r_y, sigmad) *
                             range_gauss(dm_fabs(refPix - nb), sigmar);
            norm += tg;
            c_total += sn.w * tg;
            n_total.x = n_total.x + sn.x * tg;
            n_total.y = n_total.y + sn.y * tg;
            n_total.z = n_total.z + sn.z * tg;
        }
    }
    cost_out = c_total / norm;
    n_total.x = n_total.x / norm;
    n_total.y = n_total.y / norm;
    n_total.z = n_total.z / norm;
    normalize3(n_total);
    return n_total;
}

// ------------------------------------------------------ colour-split lanes
// Every PatchMatch kernel maps a 64x4 block onto 64 colour-split columns x 4
// rows of ONE checkerboard colour: lane (tx, ty) of block (bx, by) handles
// pixel x = 2k + s, y, with k = 64 bx + tx, y = 4 by + ty, s = (y + colour) & 1.
struct LaneGeom {
    int k, px, py, s, tb;
};

// XCD-aware block order (cdna_hip_programming.md T1): workgroups are dealt
// round-robin to the 8 XCDs, so consecutive (x, y) blocks would land on 8
// different L2s. Remap the dispatch index so XCD j processes one contiguous
// run of blocks (a band of rows): its L2 then holds the source-image
// footprint of that band only. Bijective for any block count; affects speed
// only (dispatch placement is not guaranteed).
struct BlockXY {
    int bx, by;
};

DEV BlockXY xcd_block(int by0 = 0) {  // by0: block row of the grid's first row (row bands)
    const int gx = gridDim.x;
    const int T = gx * gridDim.y;
    const int L = blockIdx.y * gx + blockIdx.x;
    const int xcd = L & 7, i = L >> 3;
    const int q = T >> 3, r = T & 7;
    const int nl = (xcd < r) ? xcd * (q + 1) + i : r * (q + 1) + (xcd - r) * q + i;
    BlockXY b;
    b.by = nl / gx;
    b.bx = nl - b.by * gx;
    b.by += by0;
    return b;
}

// kWaveRows = R rows per wave: each wave covers 64/R columns x R rows of the
// block instead of one 64-column row, so its gathers for neighbouring patch
// rows overlap in the source image (L1 reuse within a wave).
DEV LaneGeom lane_geom_of(int colour, BlockXY b, int tid) {
    LaneGeom g;
    // waves of C columns x R rows, kBX / C of them side by side per block row
    constexpr int R = kWaveRows, C = 64 / R, WPR = kBX / C;
    static_assert(kWaveRows == 8 && kBX % 8 == 0 && kBY % 8 == 0, "8 x 8-pixel waves tile the block");
    const int w = tid >> 6, l = tid & 63;
    // Which pixel of its C x R patch each lane takes. A gather costs one TD
    // cycle per L1 access, and an access serves one 64-B line for one group
    // of 8 lanes: the even or the odd lanes of a 16-lane quarter-wave
    // (profiles/r04_td_addressing.md). A quarter is 4 columns x 4 rows, lanes
    // column-major inside, so each 8-lane group is 4 adjacent colour-split
    // columns of 2 rows (rows r, r + 2): 36 accesses per k_sweep gather
    // against 46 for row-major lanes (8 columns x 2 rows per quarter, groups
    // of every other column), bench +2 % (profiles/r04_lanemap2_pmc.txt).
    // Each lane still computes its own pixel, so the map changes no result.
    // lane -> (column, row) inside the wave's C x R pixels
    const int lc = ((l >> 2) & 3) + 4 * ((l >> 4) & 1);
    const int lr = (l & 3) + 4 * (l >> 5);
    const int tx = (w % WPR) * C + lc, ty = (w / WPR) * R + lr;
    g.k = b.bx * kBX + tx;
    g.py = b.by * kBY + ty;
    g.s = (g.py + colour) & 1;
    g.px = 2 * g.k + g.s;
    g.tb = ty * kTileW + tx + g.s;
    return g;
}

DEV LaneGeom lane_geom(int colour, BlockXY b) { return lane_geom_of(colour, b, threadIdx.y * kBX + threadIdx.x); }

// ---------------------------------------------------------- patch policies
// The PatchMatch kernels (init, sweep, refinement, eval; acmmp_kernels_tx.hip)
// are written once over a patch policy P, which owns everything that depends
// on the patch geometry:
//   P::kTileFloats / kWeightSlots / kLutFloats   sizes of the block's LDS arrays
//   P::Pix                a pixel's handle: LDS addresses + wo (the lane's index
//                         in the block), mean, var, inv_wsum, which the bodies read
//   P::stage(...)         stage the block's reference window (caller syncs)
//   P::lane(...)          the handle of lane `tid` of the block (any lane)
//   P::invariants(...)    form a pixel's reference invariants
//   P::ncc(...)           NCC of plane h against source view v
// FastPatch is the 11 / 2 code of this file; GeneralPatch (acmmp_general.h)
// takes radius and increment from KViews::prm.
struct PatchLds {
    float *tile;  // the reference window
    WSlot *w;     // per-lane weight slots
    float *wlut;  // the u8-form weight table
};

template <int TX>
struct FastPatch {
    static constexpr int kTx = TX;
    static constexpr int kTileFloats = kTileW * kTileH;
    static constexpr int kWeightSlots = kSlots * kThreads;
    static constexpr int kLutFloats = (TX & kTxU8) ? kWlutClasses * 256 : 1;
    typedef PixPatch Pix;

    // lut: take the bilateral weights from the table (the u8 form's init and sweep)
    static __device__ __forceinline__ void stage(const KViews &kv, const PatchLds &l, BlockXY blk, int colour,
                                                 bool lut) {
        load_ref_tile(kv, l.tile, blk.bx * kBX, blk.by * kBY, colour);
        if (lut) load_wlut(kv, l.wlut);
    }
    static __device__ __forceinline__ Pix lane(const PatchLds &l, const LaneGeom &g, BlockXY, int tid) {
        Pix pp;
        pp.wo = tid;
        pp.w = l.w + tid;
        pp.rt = l.tile + g.tb;
        return pp;
    }
    static __device__ __forceinline__ void invariants(const KViews &kv, const PatchLds &l, const LaneGeom &g, Pix &pp,
                                                      bool lut) {
        pixel_patch(kv, l.tile, g.tb, g.s, pp, lut ? l.wlut : nullptr);
    }
    static __device__ __forceinline__ float ncc(const KViews &kv, const Pix &pp, int v, int px, int py, float4 h) {
        return bilateral_ncc<TX>(kv, pp, v, px, py, h);
    }
};

// ------------------------------------------------------- texel-form units
// The templated kernels (k_init, k_sweep_f, k_eval_costs) are instantiated
// per texel form (a kTx* bit set) in their own translation unit:
// acmmp_kernels_tx.hip compiled once per form (Makefile), 5 source-count
// buckets each, so the build compiles the forms in parallel. These three
// functions per form are the units' entry points; acmmp_kernels.hip picks
// the form. ACMMP_TX_FORMS is the list of forms that exist (the Makefile's
// TX_FORMS repeats it: a form missing there fails to link).
#define ACMMP_TX_FORMS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(8) X(10)
template <int TX> hipError_t tx_launch_init(const KViews *d_kv, int nsrc, dim3 grid, hipStream_t s, KState st);
template <int TX>
hipError_t tx_launch_sweep(const KViews *d_kv, int nsrc, dim3 grid, hipStream_t s, KState st, int colour, int iter);
template <int TX>
hipError_t tx_launch_eval(const KViews *d_kv, int nsrc, dim3 grid, hipStream_t s, const float4 *planes, float *out,
                          float *out_init, uint32_t *out_views);
#define ACMMP_TX_DECL(TX)                                                                                      \
    template <> hipError_t tx_launch_init<TX>(const KViews *, int, dim3, hipStream_t, KState);                  \
    template <> hipError_t tx_launch_sweep<TX>(const KViews *, int, dim3, hipStream_t, KState, int, int);       \
    template <> hipError_t tx_launch_eval<TX>(const KViews *, int, dim3, hipStream_t, const float4 *, float *,  \
                                              float *, uint32_t *);
ACMMP_TX_FORMS(ACMMP_TX_DECL)
#undef ACMMP_TX_DECL

// The general-patch kernels (k_init_g, k_sweep_g, k_eval_costs_g) are the same
// file compiled with -DACMMP_GENERAL_UNIT, again one unit per form (the
// Makefile's GX_FORMS): every form but the texture_filter8 ones.
#define ACMMP_GX_FORMS(X) X(0) X(1) X(2) X(3) X(4) X(5)
template <int TX> hipError_t gx_launch_init(const KViews *d_kv, int nsrc, dim3 grid, hipStream_t s, KState st);
template <int TX>
hipError_t gx_launch_sweep(const KViews *d_kv, int nsrc, dim3 grid, hipStream_t s, KState st, int colour, int iter);
template <int TX>
hipError_t gx_launch_eval(const KViews *d_kv, int nsrc, dim3 grid, hipStream_t s, const float4 *planes, float *out,
                          float *out_init, uint32_t *out_views);
#define ACMMP_GX_DECL(TX)                                                                                      \
    template <> hipError_t gx_launch_init<TX>(const KViews *, int, dim3, hipStream_t, KState);                  \
    template <> hipError_t gx_launch_sweep<TX>(const KViews *, int, dim3, hipStream_t, KState, int, int);       \
    template <> hipError_t gx_launch_eval<TX>(const KViews *, int, dim3, hipStream_t, const float4 *, float *,  \
                                              float *, uint32_t *);
ACMMP_GX_FORMS(ACMMP_GX_DECL)
#undef ACMMP_GX_DECL

}  // namespace acmmp

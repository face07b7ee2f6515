// acmmp_general.h — the general patch policy of the PatchMatch kernels: any
// patch_size / radius_increment of the engine's envelope (radius 1..10,
// increment 1..2 * radius), read from KViews::prm at run time. Included only
// by the general units (acmmp_kernels_tx.hip compiled with
// -DACMMP_GENERAL_UNIT); the 11 / 2 fast path (FastPatch, acmmp_dev.h) never
// sees this file.
//
// It is ComputeBilateralNCC's loop as written (src/ACMMP.cu:382-412): x offset
// outer, y offset inner, offsets -radius, -radius + inc, ... <= radius. The
// offsets need not be symmetric or contain 0 (8 / 3: {-4, -1, 2}), and an even
// offset lands on the other checkerboard colour, so the block's reference
// window is a full-pixel tile. What the fast path keeps per pixel-iteration in
// LDS (36 weights) is recomputed here per tap and per call: bilateral_weight
// is the same function of the same inputs (offsets, tile texel, centre texel,
// sigmas), hence bit-identical, and its arithmetic sits between the issue of a
// group's gathers and their first use. Mean, variance and 1 / sum(w) of the
// reference side are still formed once per pixel-iteration (invariants).
#pragma once

#include "acmmp_dev.h"

namespace acmmp {

constexpr int kGMaxRadius = 10;  // patch_size <= 21 (the engine's envelope)
// Full-pixel reference window of a block: pixels x in [2 k0 - R, 2 k0 + 2 kBX
// - 1 + R], y in [y0 - R, y0 + kBY - 1 + R], sized (and always staged) for
// R = kGMaxRadius so every tile address is a compile-time pitch: 7.3 KB.
constexpr int kGTileW = 2 * kBX + 2 * kGMaxRadius, kGTileH = kBY + 2 * kGMaxRadius;
// Gathers of one patch column kept in flight per lane: the column's rows go
// out in groups of this many loads, issued before the group's weights are
// computed and the first of them is used.
constexpr int kGGroup = 4;

// radius, increment and taps per axis: wave-uniform (scalar loads of KViews)
struct PatchGeom {
    int radius, inc, taps;
};
DEV PatchGeom patch_geom(const KViews &kv) {
    PatchGeom g;
    g.radius = kv.prm.patch_size / 2;
    g.inc = kv.prm.radius_increment;
    g.taps = (2 * g.radius) / g.inc + 1;  // offsets -radius + k * inc <= radius
    return g;
}

DEV void load_ref_window(const KViews &kv, float *tile, int k0, int y0) {
    const float *img = kv.img[0];
    const int pitch = kv.ipitch[0], W = kv.W, H = kv.H;
    // as load_ref_tile: every texel of a thread loaded before any is stored,
    // a thread past the end repeats the last element
    constexpr int kN = kGTileW * kGTileH, kIt = (kN + kThreads - 1) / kThreads;
    float v[kIt];
    int at[kIt];
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
        int e = threadIdx.y * kBX + threadIdx.x + it * kThreads;
        e = e < kN ? e : kN - 1;
        const int r = e / kGTileW, c = e - r * kGTileW;
        at[it] = e;
        v[it] = texel(img, pitch, W, H, 2 * k0 - kGMaxRadius + c, y0 - kGMaxRadius + r);  // clamp-to-edge baked in
    }
#pragma unroll
    for (int it = 0; it < kIt; ++it) tile[at[it]] = v[it];
}

// bilateral_ncc's reciprocal-window test for any patch corners (that function
// keeps its own copy: k_sweep_f's register allocation moved when it called
// this one). hz is affine in the sample position, so its values over a patch
// lie between the values at the patch's four corners (up to rounding: the
// test uses a 2x margin). Inside the window the Newton reciprocal is
// bit-identical to IEEE 1/z (exhaustive proof: acmmp_selftest_reciprocal).
DEV bool recip_window_holds(const float *H, float xl, float xr, float yt, float yb) {
    const float z00 = dm_fma(H[7], yt, dm_fma(H[6], xl, H[8]));
    const float z10 = dm_fma(H[7], yt, dm_fma(H[6], xr, H[8]));
    const float z01 = dm_fma(H[7], yb, dm_fma(H[6], xl, H[8]));
    const float z11 = dm_fma(H[7], yb, dm_fma(H[6], xr, H[8]));
    const float zmin = fminf(fminf(z00, z10), fminf(z01, z11));
    const float zmax = fmaxf(fmaxf(z00, z10), fmaxf(z01, z11));
    return (zmin >= 0x1p-124f && zmax < 0x1p124f) || (zmax <= -0x1p-124f && zmin > -0x1p124f);
}

// bilateral_ncc's epilogue, likewise: the cost of ComputeBilateralNCC from
// its three source-side sums and the reference-side invariants
// (src/ACMMP.cu:414-431, the fused moments of pin P3).
DEV float ncc_from_sums(float mean, float var, float inv_wsum, float sum_src, float sum_ss, float sum_rs) {
    sum_src *= inv_wsum;
    const float var_src = dm_fma(sum_ss, inv_wsum, -(sum_src * sum_src));  // pin P3
    if (var_src < kNccMinVar) return kNccCostMax;
    const float covar = dm_fma(sum_rs, inv_wsum, -(mean * sum_src));
    const float var_rs = dm_sqrt(var * var_src);
    float c = 1.0f - covar / var_rs;
    c = (c < kNccCostMax) ? c : kNccCostMax;
    c = (c > 0.0f) ? c : 0.0f;
    return c;
}

// A pixel's handle: its centre in the tile and the reference-side invariants.
struct GenPix {
    int wo;           // this lane's index in the block
    const float *rc;  // LDS: the pixel itself in the tile; sample (i, j) at rc[j * kGTileW + i]
    float mean;       // sum_ref * inv_bilateral_weight_sum
    float var;        // var_ref
    float inv_wsum;   // inv_bilateral_weight_sum
};

// pixel_patch for any geometry: the reference half of the loop.
DEV void general_invariants(const KViews &kv, GenPix &pp) {
    const PatchGeom pg = patch_geom(kv);
    const float ss = kv.prm.sigma_spatial, sc = kv.prm.sigma_color;
    const float center = pp.rc[0];
    float sum_ref = 0.0f, sum_rr = 0.0f, bw = 0.0f;
#pragma unroll 1
    for (int i = 0; i < pg.taps; ++i) {
        const int xo = -pg.radius + i * pg.inc;
        float r_ref = 0.0f, r_rr = 0.0f, r_w = 0.0f;
#pragma unroll 1
        for (int j = 0; j < pg.taps; ++j) {
            const int yo = -pg.radius + j * pg.inc;
            const float r = pp.rc[yo * kGTileW + xo];
            const float w = bilateral_weight((float)xo, (float)yo, r, center, ss, sc);
            const float wr = w * r;
            r_ref = dm_fma(w, r, r_ref);  // pin P3, as pixel_patch
            r_rr = dm_fma(wr, r, r_rr);
            r_w += w;
        }
        sum_ref += r_ref;
        sum_rr += r_rr;
        bw += r_w;
    }
    const float inv = 1.0f / bw;
    sum_ref *= inv;
    pp.mean = sum_ref;
    pp.var = dm_fma(sum_rr, inv, -(sum_ref * sum_ref));
    pp.inv_wsum = inv;
}

// One gathered source sample: the fetched footprint (in the form of TX) and
// its bilinear fractions.
template <int TX>
struct TapFetch {
    u32x4 t;     // fp32 row pairs
    unsigned q;  // u8 quad
    u32x2 hq;    // f16 difference quad
    float ax, ay;
};

// fetch_row's arithmetic for one sample (same IEEE operations, unpacked):
// reciprocal, clamp of pin P2, fractions, record index, and the load issued
// (not waited for).
template <bool FAST, int TX>
DEV void fetch_tap(const SrcImage &im, float hx, float hy, float hz, TapFetch<TX> &f) {
    constexpr bool WIDE = (TX & kTxWide) != 0, U8 = (TX & kTxU8) != 0, H16 = (TX & kTxH16) != 0;
    static_assert((TX & kTxFrac8) == 0, "texture_filter8 is built for the 11 / 2 kernels only");
    const float fw = (float)im.W, fh = (float)im.H;
    const float inv = FAST ? recip_newton(hz) : 1.0f / hz;
    float u = hx * inv, v = hy * inv;
    u = (u + 0.5f) - 0.5f;
    v = (v + 0.5f) - 0.5f;
    float xs, ys;
    if (FAST) {  // finite or +-inf: v_med3 equals max-then-min (fetch_row)
        xs = __builtin_amdgcn_fmed3f(u, -1.0f, fw);
        ys = __builtin_amdgcn_fmed3f(v, -1.0f, fh);
    } else {
        xs = fminf(fmaxf(u, -1.0f), fw);
        ys = fminf(fmaxf(v, -1.0f), fh);
    }
    const float flx = dm_floor(xs), fly = dm_floor(ys);
    f.ax = xs - flx;
    f.ay = ys - fly;
    unsigned idx;  // record (y0 + 1) * pitch + x0 + 1
    if (!WIDE) idx = (unsigned)dm_fma(fly, im.fpitch, flx + im.fp1);
    else idx = __umul24((unsigned)(fly + 1.0f), (unsigned)im.pitch) + (unsigned)(flx + 1.0f);
    if (H16) f.hq = amdgcn_struct_buffer_load_b64(im.rsrc, (int)idx, 0, 0, 0);
    else if (U8) f.q = amdgcn_struct_buffer_load_b32(im.rsrc, (int)idx, 0, 0, 0);
    else f.t = amdgcn_struct_buffer_load_b128(im.rsrc, (int)idx, 0, 0, 0);
}

// Bilinear value of a fetched sample (reduce_row's lerps, one sample).
template <int TX>
DEV float tap_value(const TapFetch<TX> &f) {
    constexpr bool U8 = (TX & kTxU8) != 0, H16 = (TX & kTxH16) != 0;
    if (H16) {
        const unsigned w0 = f.hq.x, w1 = f.hq.y;
        const h2v t = __builtin_bit_cast(h2v, w0), d = __builtin_bit_cast(h2v, w1);
        const float r0 = __builtin_fmaf(f.ax, (float)d.x, (float)t.x);
        const float r1 = __builtin_fmaf(f.ax, (float)d.y, (float)t.y);
        return dm_fma(f.ay, r1 - r0, r0);
    } else if (U8) {
        const unsigned q = f.q;
        const float t00 = (float)(q & 0xffu), t01 = (float)((q >> 8) & 0xffu);
        const float t10 = (float)((q >> 16) & 0xffu), t11 = (float)(q >> 24);
        const float top = dm_fma(f.ax, t10 - t00, t00);
        const float bot = dm_fma(f.ax, t11 - t01, t01);
        return dm_fma(f.ay, bot - top, top);
    } else {
        return lerp_sample(f.t, f.ax, f.ay);
    }
}

// Source-sample reduction of ComputeBilateralNCC for any geometry: per patch
// column the partial sums over its rows in order, the columns added in order
// (the pinned order, as ncc_sums_rows). A column's rows go out kGGroup
// gathers at a time; a group's slots past the last row repeat that row's
// load (same address) and are not accumulated.
template <bool FAST, int TX>
DEV void general_sums(const KViews &kv, const SrcImage &im, const float *H, const GenPix &pp, int px, int py,
                      float &sum_src, float &sum_ss, float &sum_rs) {
    const PatchGeom pg = patch_geom(kv);
    const float ss = kv.prm.sigma_spatial, sc = kv.prm.sigma_color;
    const float center = pp.rc[0];
    sum_src = 0.0f;
    sum_ss = 0.0f;
    sum_rs = 0.0f;
#pragma unroll 1
    for (int i = 0; i < pg.taps; ++i) {
        const int xo = -pg.radius + i * pg.inc;
        const float x = (float)(px + xo);
        const float cx = dm_fma(H[0], x, H[2]);  // pin P1, the x-terms per column
        const float cy = dm_fma(H[3], x, H[5]);
        const float cz = dm_fma(H[6], x, H[8]);
        float c_s = 0.0f, c_ss = 0.0f, c_rs = 0.0f;
#pragma unroll 1
        for (int j0 = 0; j0 < pg.taps; j0 += kGGroup) {
            TapFetch<TX> f[kGGroup];
            float w[kGGroup], r[kGGroup];
#pragma unroll
            for (int g = 0; g < kGGroup; ++g) {
                const int j = (j0 + g < pg.taps) ? j0 + g : pg.taps - 1;
                const float y = (float)(py - pg.radius + j * pg.inc);
                fetch_tap<FAST, TX>(im, dm_fma(H[1], y, cx), dm_fma(H[4], y, cy), dm_fma(H[7], y, cz), f[g]);
            }
#pragma unroll
            for (int g = 0; g < kGGroup; ++g) {
                const int j = (j0 + g < pg.taps) ? j0 + g : pg.taps - 1;
                const int yo = -pg.radius + j * pg.inc;
                r[g] = pp.rc[yo * kGTileW + xo];
                w[g] = bilateral_weight((float)xo, (float)yo, r[g], center, ss, sc);
            }
#pragma unroll
            for (int g = 0; g < kGGroup; ++g) {
                if (j0 + g < pg.taps) {  // wave-uniform
                    const float sv = tap_value<TX>(f[g]);
                    const float wr = w[g] * r[g];
                    const float ws = w[g] * sv;
                    c_s = dm_fma(w[g], sv, c_s);  // pin P3, as reduce_row
                    c_ss = dm_fma(ws, sv, c_ss);
                    c_rs = dm_fma(wr, sv, c_rs);
                }
            }
        }
        sum_src += c_s;
        sum_ss += c_ss;
        sum_rs += c_rs;
    }
}

// The patch policy (see FastPatch, acmmp_dev.h, for the operations).
template <int TX>
struct GeneralPatch {
    static constexpr int kTx = TX;
    static constexpr int kTileFloats = kGTileW * kGTileH;
    static constexpr int kWeightSlots = 1;  // no per-lane weight slots: weights are recomputed
    static constexpr int kLutFloats = 1;    // no weight table: KViews::wlut covers the 11 / 2 classes only
    typedef GenPix Pix;

    static __device__ __forceinline__ void stage(const KViews &kv, const PatchLds &l, BlockXY blk, int, bool) {
        load_ref_window(kv, l.tile, blk.bx * kBX, blk.by * kBY);
    }
    static __device__ __forceinline__ Pix lane(const PatchLds &l, const LaneGeom &g, BlockXY blk, int tid) {
        Pix pp;
        pp.wo = tid;
        const int tx = g.k - blk.bx * kBX, ty = g.py - blk.by * kBY;
        pp.rc = l.tile + (ty + kGMaxRadius) * kGTileW + 2 * tx + g.s + kGMaxRadius;
        return pp;
    }
    static __device__ __forceinline__ void invariants(const KViews &kv, const PatchLds &, const LaneGeom &, Pix &pp,
                                                      bool) {
        general_invariants(kv, pp);
    }
    static __device__ __forceinline__ float ncc(const KViews &kv, const Pix &pp, int v, int px, int py, float4 h) {
        if (pp.var < kNccMinVar) return kNccCostMax;
        const SrcImage im = src_image<TX>(kv, v);
        float H[9];
        homography(kv, v, h, H);
        const float2 pt = project(H, (float)px, (float)py);
        if (pt.x >= (float)im.W || pt.x < 0.0f || pt.y >= (float)im.H || pt.y < 0.0f) return kNccCostMax;
        // the reciprocal window's z-range test over the patch's actual corners
        // (the last offset is -radius + (taps - 1) * inc, not always +radius)
        const PatchGeom pg = patch_geom(kv);
        const int last = -pg.radius + (pg.taps - 1) * pg.inc;
        const bool fast = recip_window_holds(H, (float)(px - pg.radius), (float)(px + last), (float)(py - pg.radius),
                                             (float)(py + last));
        float sum_src, sum_ss, sum_rs;
        if (fast) general_sums<true, TX>(kv, im, H, pp, px, py, sum_src, sum_ss, sum_rs);
        else general_sums<false, TX>(kv, im, H, pp, px, py, sum_src, sum_ss, sum_rs);
        return ncc_from_sums(pp.mean, pp.var, pp.inv_wsum, sum_src, sum_ss, sum_rs);
    }
};

}  // namespace acmmp

// acmmp_kernels_tx.hip — the templated PatchMatch kernels of ONE texel form
// and ONE patch policy: compiled once per form with -DACMMP_TX_UNIT=<form> (a
// kTx* bit set, acmmp_dev.h; the Makefile's TX_FORMS) for the 11 / 2 fast path
// (k_init, k_sweep_f, k_eval_costs over FastPatch), and once more per form with
// -DACMMP_GENERAL_UNIT (GX_FORMS) for every other patch geometry (k_init_g,
// k_sweep_g, k_eval_costs_g over GeneralPatch), 5 source-count buckets each.
// The kernel bodies (init_body, sweep_body, refine_costs_compact, eval_body)
// are written once over the policy. The three tx_launch_* (gx_launch_*)
// functions at the end are the unit's entry points; acmmp_kernels.hip picks
// the form and the policy.
#ifndef ACMMP_TX_UNIT
#error "compile with -DACMMP_TX_UNIT=<texel form> (see the Makefile's TX_FORMS)"
#endif

#include "acmmp_dev.h"
#ifdef ACMMP_GENERAL_UNIT
#include "acmmp_general.h"
#endif

namespace acmmp {

// The block's LDS arrays of policy P (reference window, weight slots, weight
// table), declared in the calling body.
#define ACMMP_PATCH_LDS(P, lds)                            \
    __shared__ float tile[P::kTileFloats];                 \
    __shared__ WSlot wlds[P::kWeightSlots];                \
    __shared__ float wlut[P::kLutFloats];                  \
    const PatchLds lds = {tile, wlds, wlut}

// ------------------------------------------------------------------ init
// RandomInitialization (src/ACMMP.cu:609-705). Reads the row-major state,
// writes the colour-split "current" buffers. blockIdx.z = colour.
template <int NS, typename P>
DEV void init_body(const KViews *__restrict__ kvp, KState st) {
    ACMMP_PATCH_LDS(P, lds);
    constexpr bool kLut = P::kLutFloats > 1;  // bilateral weights from the u8-form table (KViews::wlut)
    const KViews &kv = *kvp;
    const int colour = blockIdx.z;
    const BlockXY blk = xcd_block(st.y0 / kBY);
    P::stage(kv, lds, blk, colour, kLut);
    __syncthreads();
    const LaneGeom g = lane_geom(colour, blk);
    const int px = g.px, py = g.py;
    if (px >= kv.W || py < st.y0 || py >= st.y1) return;
    const acmmp_params &prm = kv.prm;
    const acmmp_camera &c0 = kv.cam[0];
    const int center = py * kv.W + px;
    dm_rng rs = make_rng(kv, center, 0u);
    typename P::Pix pp = P::lane(lds, g, blk, threadIdx.y * kBX + threadIdx.x);
    P::invariants(kv, lds, g, pp, kLut);
    float4 plane;
    float cost;
    uint32_t sel = 0;
    if (!prm.geom_consistency && !prm.hierarchy && !prm.seeded) {
        const float depth = dm_rng_uniform(&rs) * (prm.depth_max - prm.depth_min) + prm.depth_min;
        plane = random_normal(c0, px, py, rs, depth);
        plane.w = distance_to_origin(c0, px, py, depth, plane);
        cost = initial_cost<NS, P>(kv, pp, px, py, plane, sel);
    } else if (prm.seeded) {
        plane = st.seed[center];
        cost = initial_cost<NS, P>(kv, pp, px, py, plane, sel);
    } else if (prm.planar_prior) {
        if (st.mask[center] > 0 && st.rm_cost[center] >= 0.1f) {
            const float perturbation = 0.02f;
            const float4 h = st.prior[center];
            float dp = h.w;
            const float dmin = (1 - 3 * perturbation) * dp;
            const float dmax = (1 + 3 * perturbation) * dp;
            dp = dm_rng_uniform(&rs) * (dmax - dmin) + dmin;
            plane = perturbed_normal(c0, px, py, h, rs, kv.pert3_pi);
            plane.w = dp;
        } else {
            plane = st.rm_plane[center];
            plane.w = distance_to_origin(c0, px, py, plane.w, plane);
        }
        cost = initial_cost<NS, P>(kv, pp, px, py, plane, sel);
    } else if (prm.upsample) {
        const float scale = (float)(1.0 * (double)prm.scaled_cols / (double)kv.W);
        const float sigmad = 0.50f, sigmar = 25.5f;
        const float a = (float)kv.W / prm.scaled_cols, b = (float)kv.H / prm.scaled_rows;
        const int Imagescale = (int)(a > b ? a : b);
        const int nn = (Imagescale * Imagescale + 1) / 2;
        const float o_y = (float)py * scale, o_x = (float)px * scale;
        const float refPix = texel(kv.img[0], kv.ipitch[0], kv.W, kv.H, px, py);
        float ucost;
        const float4 n_total = upscale_normal(kv, st, px, py, sigmad, sigmar, nn, o_y, o_x, refPix, ucost);
        const float4 prev = st.rm_plane[center];
        st.pre_cost[center] = initial_cost<NS, P>(kv, pp, px, py, prev, sel);
        plane = to_cam(c0, n_total);
        plane.w = distance_to_origin(c0, px, py, prev.w, plane);
        cost = initial_cost<NS, P>(kv, pp, px, py, plane, sel);
    } else {
        float4 h = prm.hierarchy ? st.scaled[center] : st.rm_plane[center];
        h = to_cam(c0, h);
        h.w = distance_to_origin(c0, px, py, h.w, h);
        plane = h;
        cost = initial_cost<NS, P>(kv, pp, px, py, plane, sel);
    }
    const int ci = py * kv.Wh + g.k;
    st.plane[colour][ci] = plane;
    st.cost[colour][ci] = cost;
    st.sv[colour][ci] = sel;
}

// Packed per-view sample counts (view_weights of the reference, src/ACMMP.cu:995):
// 15 draws, so every count fits 4 bits; 32 views -> two 64-bit words.
struct ViewCounts {
    uint64_t lo = 0, hi = 0;
    __device__ __forceinline__ void add(int j) {
        if (j < 16) lo += (uint64_t)1 << (4 * j);
        else hi += (uint64_t)1 << (4 * (j - 16));
    }
    __device__ __forceinline__ int get(int j) const { return (int)(((j < 16) ? (lo >> (4 * j)) : (hi >> (4 * (j - 16)))) & 15u); }
};

// ------------------------------------------------- compacted refinement
// The candidate-plane slots (cand_lds: 8 float4 per lane, slot d of lane i at
// [d * kThreads + i]) are dead after the t = 0 accept and are reused, each
// lane only within its OWN 8 slots (waves progress independently, so a
// lane's slots may still hold live candidates of another wave's t = 0 step
// — nothing may spill across lanes of different waves):
//   slots 0..4 = the 5 refinement planes; slot 5 = results of planes 0..3;
//   slot 6 = (result of plane 4, mean, var, inv_wsum); slots 7 of the wave's
//   64 lanes (1024 contiguous bytes) = the wave's item list of one view.
DEV float &cmp_res(float4 *lds, int t, int lane) {
    return reinterpret_cast<float *>(lds)[4 * ((5 + (t >> 2)) * kThreads + lane) + (t & 3)];
}
DEV float &cmp_pd(float4 *lds, int k, int lane) {  // k = 1 mean, 2 var, 3 inv_wsum
    return reinterpret_cast<float *>(lds)[4 * (6 * kThreads + lane) + k];
}
// Item k of the wave whose first lane is wbase: (t << 6) | owner lane. At most
// 5 * 64 = 320 items of 2 bytes (t = 4 does not fit a byte): 640 of the 1024.
DEV uint16_t &cmp_item(float4 *lds, int wbase, int k) {
    return reinterpret_cast<uint16_t *>(lds + 7 * kThreads + wbase)[k];
}
// Set bits of the wave mask m below this lane.
DEV int rank_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

DEV void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The 5 refinement hypotheses of PlaneHypothesisRefinement (src/ACMMP.cu:
// 743-783) cost sum_j w_j * (NCC_j (+ 0.2 geom_j)) over the lane's sampled
// views j. Their planes are fixed before any of them is evaluated, so all 5
// sums are formed here, view-major, and the sequential accept of the caller
// then consumes them in order t = 1..5 (same operations, same order per
// (lane, t): j ascending). Instead of one pass per (t, view with any lane
// sampling it), the wave packs the live (owner lane, t) items of view j into
// ceil(items / active lanes) passes: a lane evaluates another lane's item
// with that lane's pixel, LDS patch weights, tile offset and plane, and
// returns the cost through LDS. The view stays wave-uniform (scalar SRD and
// cameras). Result: cmp_res(t, lane) = sum_t, or a prefix of it (below).
//
// Dead hypotheses. Outside the planar-prior branch the caller uses sum_t only
// in `sum_t / weight_norm < cost_now`, and cost_now only falls while it
// consumes t = 1..5. Every term w_j * c_j is >= 0 or NaN (w_j >= 1, c_j an
// NCC in [0, 2] plus 0.2 * a non-negative geometric cost), so the running sum
// never decreases under round-to-nearest, and x / weight_norm is monotone in
// x. With `bound` the lane's cost_now on entry: once a prefix satisfies
// prefix / weight_norm >= bound, sum_t / weight_norm >= bound >= cost_now
// holds for whatever the remaining views cost (or sum_t is NaN), and the
// caller's comparison is false. Such a (lane, t) is dead: its remaining items
// are not packed, and cmp_res(t, lane) is left at the prefix, for which the
// caller's comparison is false by the same inequality. A NaN prefix or bound
// makes the test false, so nothing is dropped there. Planar-prior lanes, whose
// accept rule is another one, come with `prunable` false (a flag rather than
// a NaN bound: the select's extra VGPR put the NS 9 kernel 16 B of scratch
// over what tests/test_isa_guards.py allows).
template <typename P, typename RD, typename RN>
DEV void refine_costs_compact(const KViews &kv, const PatchLds &plds, float4 *lds, const typename P::Pix &pp,
                              const ViewCounts &vw, int nsrc, int colour, BlockXY blk, RD ref_depth,
                              RN ref_normal, int px, int py, float weight_norm, float bound, bool prunable) {
    const acmmp_camera &c0 = kv.cam[0];
    const int tid = pp.wo;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        float4 h = ref_normal(t);
        h.w = distance_to_origin(c0, px, py, ref_depth(t), h);
        lds[t * kThreads + tid] = h;
    }
    cmp_pd(lds, 1, tid) = pp.mean;
    cmp_pd(lds, 2, tid) = pp.var;
    cmp_pd(lds, 3, tid) = pp.inv_wsum;
    const int lane = tid & 63, wbase = tid & ~63;
    const uint64_t act = __ballot(1);
    const int nact = __popcll(act), arank = rank_below(act);
    float acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t alive = 31u;  // bit t: hypothesis t of this lane can still win
    wave_sync();
    for (int j = 0; j < nsrc; ++j) {
        const float wj = (float)vw.get(j);
        // the view's items, t-major: every count and offset comes from a
        // ballot, so the pass loop and the wave_sync()s stay wave-uniform
        uint64_t mt[5];
        int off[6];
        off[0] = 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            mt[t] = __ballot(wj > 0 && ((alive >> t) & 1u));
            off[t + 1] = off[t] + __popcll(mt[t]);
        }
        const int n = off[5];
        if (n == 0) continue;
        if (wj > 0) {
#pragma unroll
            for (int t = 0; t < 5; ++t)
                if ((alive >> t) & 1u) cmp_item(lds, wbase, off[t] + rank_below(mt[t])) = (uint16_t)((t << 6) | lane);
        }
        wave_sync();
        for (int base = 0; base < n; base += nact) {
            const int k = base + arank;
            if (k < n) {
                const int item = cmp_item(lds, wbase, k);
                const int t = item >> 6;
                const int otid = wbase + (item & 63);
                const LaneGeom og = lane_geom_of(colour, blk, otid);
                typename P::Pix op = P::lane(plds, og, blk, otid);
                op.mean = cmp_pd(lds, 1, otid);
                op.var = cmp_pd(lds, 2, otid);
                op.inv_wsum = cmp_pd(lds, 3, otid);
                const float4 h = lds[t * kThreads + otid];
                // the geometric depth fetch goes out ahead of the NCC's gathers
                GeomFetch gf = {};
                if (kv.prm.geom_consistency) gf = geom_fetch(kv, j + 1, geom_ref(kv, h, og.px, og.py));
                const float cc = P::ncc(kv, op, j + 1, og.px, og.py, h);
                cmp_res(lds, t, otid) =
                    kv.prm.geom_consistency ? cc + 0.2f * geom_finish(kv, j + 1, gf, og.px, og.py) : cc;
            }
        }
        wave_sync();
        if (wj > 0) {
            // (a dead t's result slot is stale: read, not used. The test is
            // the caller's own expression, tc / weight_norm)
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const float a = acc[t] + wj * cmp_res(lds, t, tid);
                const bool live = (alive >> t) & 1u;
                acc[t] = live ? a : acc[t];
                if (live && prunable && a / weight_norm >= bound) alive &= ~(1u << t);
            }
        }
        wave_sync();
    }
    // a dead t hands over its prefix: prefix / weight_norm >= bound >= the
    // caller's cost_now, so `tc < cost_now` is false, as it is for the full sum
#pragma unroll
    for (int t = 0; t < 5; ++t) cmp_res(lds, t, tid) = acc[t];
    wave_sync();
}

// ------------------------------------------------------------- the sweep
// CheckerboardPropagation (src/ACMMP.cu:786-1173) for the pixels of one colour.
// Neighbour state is read from the colour-split "current" buffers (the
// half-sweep snapshot); own state lives in registers and is written to the
// "next" buffer of this colour. (A device function rather than the kernel
// body: measured 4.15 -> 4.05 ms per launch)
template <int NS, typename P>
DEV void sweep_body(const KViews *__restrict__ kvp, KState st, int colour, int iter) {
    ACMMP_PATCH_LDS(P, lds);
    __shared__ float4 cand_lds[8 * kThreads];
    constexpr bool kLut = P::kLutFloats > 1;  // bilateral weights from the u8-form table (KViews::wlut)
    const KViews &kv = *kvp;
    const BlockXY blk = xcd_block(st.y0 / kBY);
    P::stage(kv, lds, blk, colour, kLut);
    __syncthreads();
    const LaneGeom g = lane_geom(colour, blk);
    const int px = g.px, py = g.py;
    const int width = kv.W, height = kv.H;
    if (py < st.y0 || py >= st.y1 || px >= width) return;  // rows [y0, y1) of the image (a band or all)
    const int oc = colour ^ 1;
    const int Wh = kv.Wh;
    const int my = py * Wh + g.k;
    const float4 *plane_same = st.plane[colour];
    const float4 *plane_opp = st.plane[oc];
    const float *cost_same = st.cost[colour];
    const float *cost_opp = st.cost[oc];
    float4 my_plane = plane_same[my];
    float my_cost = cost_same[my];
    uint32_t my_sv = st.sv[colour][my];
    if (py >= kv.sweep_rows) {  // rows the reference grid never reaches
        st.plane_nx[colour][my] = my_plane;
        st.cost_nx[colour][my] = my_cost;
        return;
    }
    const acmmp_params &prm = kv.prm;
    const acmmp_camera &c0 = kv.cam[0];
    const int nsrc = kv.nsrc;
    const int center = py * width + px;
#define CS(x, y) ((y) * Wh + ((x) >> 1))

    // ---- adaptive checkerboard sampling (:813-991). cidx[d]: colour-split
    // index of direction d's winner; bit d of `same`: it is this colour.
    // Each search reads all its costs first, unconditionally (a step outside
    // the image reads the search's first, always valid, position instead),
    // then runs the reference's comparison chain over them in the same order
    // under the same conditions: one memory latency per search instead of
    // one per step (a load inside a condition is issued and waited alone).
    int cidx[8];
    uint32_t flags = 0, same = 0;
    // Far lines d = 0..3 (up, down, left, right; bit 2d + 1): 11 steps of 2
    // from distance 3 in the opposite colour; right_far's reversed comparison
    // keeps the max (:879). Near "V"s d = 0..3 (bit 2d): the base point is
    // the opposite colour, arm k = 2 i + side is this colour (snapshot reads,
    // pin A2). A step off the image (or a direction that does not apply)
    // reads a valid stand-in: CS(px, py) of the opposite colour, `my` of
    // this one; its value is never compared.
    auto far_valid = [&](int d, int i) -> bool {
        return d == 0 ? py > 2 + 2 * i : d == 1 ? py < height - 3 - 2 * i : d == 2 ? px > 2 + 2 * i : px < width - 3 - 2 * i;
    };
    auto far_at = [&](int d, int i) -> int {
        return d == 0 ? CS(px, py - 3 - 2 * i)
             : d == 1 ? CS(px, py + 3 + 2 * i)
             : d == 2 ? CS(px - 3 - 2 * i, py)
                      : CS(px + 3 + 2 * i, py);
    };
    auto near_valid = [&](int d, int k) -> bool {
        const int i = k >> 1, sd = k & 1;
        return d == 0 ? py > 1 + i && (sd ? px < width - 1 - i : px > i)
             : d == 1 ? py < height - 2 - i && (sd ? px < width - 1 - i : px > i)
             : d == 2 ? px > 1 + i && (sd ? py < height - 1 - i : py > i)
                      : px < width - 2 - i && (sd ? py < height - 1 - i : py > i);
    };
    auto near_at = [&](int d, int k) -> int {
        const int i = k >> 1, sd = k & 1;
        return d == 0 ? CS(sd ? px + i : px - i, py - 2 - i)
             : d == 1 ? CS(sd ? px + i : px - i, py + 2 + i)
             : d == 2 ? CS(px - 2 - i, sd ? py + i : py - i)
                      : CS(px + 2 + i, sd ? py + i : py - i);
    };
    const bool near_on[4] = {py > 0, py < height - 1, px > 0, px < width - 1};
    const int near_base[4] = {CS(px, py - 1), CS(px, py + 1), CS(px - 1, py), CS(px + 1, py)};
    // every cost of the 8 searches is loaded before any comparison: one
    // memory latency for all of them (a load inside a condition is issued
    // and waited alone)
    float cf[4][11], cn[4][6], cb[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
#pragma unroll
        for (int i = 0; i < 11; ++i) cf[d][i] = cost_opp[far_valid(d, i) ? far_at(d, i) : CS(px, py)];
        cb[d] = cost_opp[near_on[d] ? near_base[d] : CS(px, py)];
#pragma unroll
        for (int k = 0; k < 6; ++k) cn[d][k] = cost_same[near_valid(d, k) ? near_at(d, k) : my];
    }
    // the reference's comparison chains, same order, same conditions
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (far_valid(d, 0)) {
            flags |= 1u << (2 * d + 1);
            int b = 0;
            float m = cf[d][0];
#pragma unroll
            for (int i = 1; i < 11; ++i)
                if (far_valid(d, i) && (d == 3 ? (m < cf[d][i]) : (cf[d][i] < m))) { m = cf[d][i]; b = i; }
            cidx[2 * d + 1] = far_at(d, b);
        }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (near_on[d]) {
            flags |= 1u << (2 * d);
            int bi = near_base[d];
            bool bs = false;
            float m = cb[d];
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (near_valid(d, k) && cn[d][k] < m) { m = cn[d][k]; bi = near_at(d, k); bs = true; }
            cidx[2 * d] = bi;
            same |= (uint32_t)bs << (2 * d);
        }
    }
#undef CS
    // the 8 winners' planes, fetched once into this lane's LDS slots (the
    // NCC prologues then read them at LDS latency, not L2's)
    float4 *cand_slot = cand_lds + threadIdx.y * kBX + threadIdx.x;
    // (all 8 loads issued together, and stored unconditionally so none is
    // sunk into a conditional block and waited alone: an unflagged
    // direction's slot gets the own plane, and every reader of a slot
    // checks its flag first)
    float4 cpl[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const bool f = (flags >> d) & 1u;
        cpl[d] = ((f && !((same >> d) & 1u)) ? plane_opp : plane_same)[f ? cidx[d] : my];
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) cand_slot[d * kThreads] = cpl[d];
    auto cand = [&](int d) -> float4 { return cand_slot[d * kThreads]; };

    typename P::Pix pp = P::lane(lds, g, blk, threadIdx.y * kBX + threadIdx.x);
    P::invariants(kv, lds, g, pp, kLut);

    // cost_array[8][32] = {2.0f}: only [0][0] is 2, the rest 0 (:805)
    float cost_array[8][NS];
    // view-selection inputs (:994-1032), folded into the view-major candidate
    // loop so each view's 8 costs are consumed from registers
    float probs[NS];
    uint32_t nb[4];
    {
        const uint32_t *sv_opp = st.sv[oc];
        // (x, y+-1) are colour-split column (x >> 1); (x+-1, y) are k - 1 + s, k + s
        nb[0] = (py > 0) ? sv_opp[(py - 1) * Wh + (px >> 1)] : 0u;
        nb[1] = (py < height - 1) ? sv_opp[(py + 1) * Wh + (px >> 1)] : 0u;
        nb[2] = (px > 0) ? sv_opp[py * Wh + ((px - 1) >> 1)] : 0u;
        nb[3] = (px < width - 1) ? sv_opp[py * Wh + ((px + 1) >> 1)] : 0u;
    }
    const float cost_threshold = (float)(0.8 * (double)dm_expf((float)(iter * iter) / (-90.0f)));
    // view-major: the 8 candidates of one source view gather from nearly the
    // same footprint, back to back (results are independent)
    for (int v = 0; v < nsrc; ++v) {
        // one NCC call site: the candidate loop stays rolled (d is wave-uniform,
        // the candidate's index is picked by selects), and the sampling
        // statistics of :1013-1024 are accumulated in the same j = 0..7 order
        float count = 0;
        int count_false = 0;
        float tmpw = 0;
#pragma unroll 1
        for (int d = 0; d < 8; ++d) {
            float c;
            if ((flags >> d) & 1u) c = P::ncc(kv, pp, v + 1, px, py, cand(d));
            else c = (d == 0 && v == 0) ? 2.0f : 0.0f;
            cost_array[d][v] = c;
            if (c < cost_threshold) {
                // exp(c * c / -0.18f) (:1017): c is 0 or in [2^-24, 2] (an NCC is 1 - q rounded,
                // clamped to [0, 2]), so c * c is 0 or in [2^-48, 4] and the quotient in
                // [-22.3, 0], where the Markstein quotient and dm_expf_nonpos are the IEEE
                // quotient and dm_expf bit for bit (exhaustive: tests/test_detmath.py)
                tmpw += dm_expf_nonpos(dm_div_neg018(c * c));
                count++;
            }
            if (c > 1.2f) count_false++;
        }
        float vsp = 0.0f;
        for (int n = 0; n < 4; ++n)
            if ((flags >> (2 * n)) & 1u) vsp += ((nb[n] >> v) & 1u) ? 0.9f : 0.1f;
        float pr = 0.0f;
        if (count > 2 && count_false < 3) pr = tmpw / count;
        else if (count_false < 3) pr = dm_expf(cost_threshold * cost_threshold / (-0.32f));
        probs[v] = pr * vsp;
    }

    // ---- multi-hypothesis joint view selection (:994-1056)
    // CDF in registers (static indices over NS, predicated on i < nsrc): the
    // 15 draws then need no dependent scratch loads. The CDF is
    // nondecreasing (non-negative terms; once NaN it stays NaN), so the
    // reference's "first i with cdf[i] > r" (:1036-1041) is the count of
    // entries <= r, taken only if that entry is > r (a NaN or all-<= r CDF
    // selects nothing, as in the reference).
    float cdf[NS];
    {  // TransformPDFToCDF (:107-121), same operations and order
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            cdf[i] = i < nsrc ? probs[i] : 0.0f;
            if (i < nsrc) sum += cdf[i];
        }
        const float inv = 1.0f / sum;
        float cum = 0.0f;
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (i < nsrc) {
                cum += cdf[i] * inv;
                cdf[i] = cum;
            }
    }
    dm_rng rs = make_rng(kv, center, 1u + (uint32_t)iter);
    ViewCounts vw;
#pragma unroll 1
    for (int sample = 0; sample < 15; ++sample) {
        const float rand_prob = dm_rng_uniform(&rs) - FLT_EPSILON;
        int idx = 0;
        float at = cdf[0];
#pragma unroll
        for (int i = 0; i < NS; ++i) idx += (i < nsrc && cdf[i] <= rand_prob) ? 1 : 0;
#pragma unroll
        for (int i = 1; i < NS; ++i) at = idx == i ? cdf[i] : at;
        if (idx < nsrc && at > rand_prob) vw.add(idx);
    }
    uint32_t temp_sv = 0;
    float weight_norm = 0;
    for (int i = 0; i < nsrc; ++i) {
        const int c = vw.get(i);
        if (c > 0) { temp_sv |= (1u << i); weight_norm += (float)c; }
    }
    float final_costs[8];
    if (!prm.geom_consistency) {
        // photometric: the NS cost loads of a candidate issued together
        // (static offsets), unsampled views add +0 (costs are finite and
        // >= 0, fc >= +0: the same sum as skipping them)
        for (int i = 0; i < 8; ++i) {
            float fc = 0.0f;
#pragma unroll
            for (int j = 0; j < NS; ++j)
                if (j < nsrc) {
                    const float wj = (float)vw.get(j);
                    fc += wj > 0 ? wj * cost_array[i][j] : 0.0f;
                }
            final_costs[i] = fc / weight_norm;
        }
    } else if (NS <= 9) {
        // (the 9-view bucket only: with 16-32 views the batch of fetches
        // costs more than the latency it hides, geometric launch +0.2 / +0.6
        // / +1.1 % at nsrc 16 / 20 / 21, profiles/r05_geom_ahead_ns.jsonl;
        // those buckets take the per-view loop below)
        // views sampled by some lane of the wave (bit j; nsrc <= 32, so
        // padding slots j >= nsrc never appear)
        uint32_t wave_views = 0;
        for (int j = 0; j < nsrc; ++j) wave_views |= (__ballot(vw.get(j) > 0) != 0 ? 1u : 0u) << j;
        // geometric: a flagged candidate's source-depth fetches for all views
        // are issued before any is consumed (one memory latency per
        // candidate, not one per view); the sum is the same ops in the same
        // order, with unsampled views adding +0 as above. Only the nsrc real
        // views are fetched and read (j < nsrc is wave-uniform, so the loads
        // still go out together; padding slots j >= nsrc are never written)
        for (int i = 0; i < 8; ++i) {
            float fc = 0.0f;
            const bool fl = (flags >> i) & 1u;
            // the candidate's cost row read whole and unconditionally (one
            // batch of scratch loads, not one load and wait per sampled view)
            float ci[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) ci[j] = j < nsrc ? cost_array[i][j] : 0.0f;
            if (fl) {
                // views no lane of the wave sampled add +0 for every lane:
                // their geometric cost is not finished (wave-uniform skip;
                // the fetches stay unconditional, one batch per candidate)
                const GeomRef gi = geom_ref(kv, cand(i), px, py);
                GeomFetch gf[NS];
#pragma unroll
                for (int j = 0; j < NS; ++j) gf[j] = j < nsrc ? geom_fetch(kv, j + 1, gi) : GeomFetch{};
#pragma unroll
                for (int j = 0; j < NS; ++j)
                    if ((wave_views >> j) & 1u) {
                        const float wj = (float)vw.get(j);
                        const float gc = geom_finish(kv, j + 1, gf[j], px, py);
                        fc += wj > 0 ? wj * (ci[j] + 0.2f * gc) : 0.0f;
                    }
            } else {
#pragma unroll
                for (int j = 0; j < NS; ++j)
                    if (j < nsrc) {
                        const float wj = (float)vw.get(j);
                        fc += wj > 0 ? wj * (ci[j] + 0.1f * 3.0f) : 0.0f;
                    }
            }
            final_costs[i] = fc / weight_norm;
        }
    } else
    for (int i = 0; i < 8; ++i) {
        float fc = 0.0f;
        const bool fl = (flags >> i) & 1u;
        GeomRef gi = {};
        if (prm.geom_consistency && fl) gi = geom_ref(kv, cand(i), px, py);  // once per candidate
        for (int j = 0; j < nsrc; ++j) {
            const float wj = (float)vw.get(j);
            if (wj > 0) {
                if (prm.geom_consistency) {
                    const float cij = cost_array[i][j];
                    if (fl) fc += wj * (cij + 0.2f * geom_cost_at(kv, j + 1, gi, px, py));
                    else fc += wj * (cij + 0.1f * 3.0f);
                } else {
                    fc += wj * cost_array[i][j];
                }
            }
        }
        final_costs[i] = fc / weight_norm;
    }
    int min_cost_idx = 0;
    {
        float m = final_costs[0];
        for (int i = 1; i < 8; ++i)
            if (final_costs[i] <= m) { m = final_costs[i]; min_cost_idx = i; }
    }

    // ---- current hypothesis (:1080-1093) + refinement (:707-784): one NCC
    // site. t = 0 evaluates the current plane; t = 1..5 the refinement planes.
    const bool has_prior = prm.planar_prior && st.mask[center] > 0;
    float4 prior_plane = make_float4(0.f, 0.f, 0.f, 0.f);
    if (prm.planar_prior) prior_plane = st.prior[center];
    float cost_now = 0.0f, depth_now = 0.0f, restricted_cost = 0.0f, depth_prior = 0.0f;
    float4 plane_now = my_plane;
    // the 5 refinement hypotheses (:735-740) take their depths and normals
    // from 3 values each: (depth, normal) of t = 1..5 is
    // (rnd, now), (gen, rnd), (rnd, rnd), (gen, pert), (pert, now), with
    // gen / now the depth / plane at generation time (held apart: the
    // accepts below move depth_now and plane_now). Picked by wave-uniform
    // selects (a dynamically indexed array would live in scratch).
    float rd_rnd = 0.0f, rd_gen = 0.0f, rd_pert = 0.0f;
    float4 rn_now = my_plane, rn_rnd = my_plane, rn_pert = my_plane;
    auto ref_depth = [&](int k) -> float { return k == 4 ? rd_pert : ((k & 1) ? rd_gen : rd_rnd); };
    auto ref_normal = [&](int k) -> float4 {
        return (k == 0 || k == 4) ? rn_now : (k == 3 ? rn_pert : rn_rnd);
    };
    const float gamma = 0.5f;
    const float depth_sigma = (prm.depth_max - prm.depth_min) / 64.0f;
    const float two_dss = 2 * depth_sigma * depth_sigma;
    const float two_ass = 2 * kv.angle_sigma * kv.angle_sigma;
    const float beta = 0.18f;

    for (int t = 0; t < 6; ++t) {
        // all 5 refinement costs at once (their planes go to LDS slots 0..4).
        // cost_now is final for t = 0 here and only falls from here on: it
        // bounds what a refinement plane may cost and still be accepted. A
        // planar-prior lane accepts by exp(-c^2 / beta) * prior instead and
        // may raise cost_now: it keeps all its hypotheses
        if (t == 1)
            refine_costs_compact<P>(kv, lds, cand_lds, pp, vw, nsrc, colour, blk, ref_depth, ref_normal, px, py,
                                    weight_norm, cost_now, !has_prior);
        float4 h;
        if (t == 0) h = my_plane;
        else h = cand_lds[(t - 1) * kThreads + pp.wo];  // stored by refine_costs_compact
        // views with a zero sampled weight contribute +0 in the reference
        // (weight 0 * finite cost), so their NCC is skipped: bit-identical
        float tc = 0.0f;
        if (t >= 1) {
            tc = cmp_res(cand_lds, t - 1, pp.wo);
        } else {
            GeomRef gnow = {};
            if (prm.geom_consistency) gnow = geom_ref(kv, h, px, py);  // once for the current plane
            for (int j = 0; j < nsrc; ++j) {
                const float wj = (float)vw.get(j);
                if (wj > 0) {
                    // the geometric depth fetch goes out ahead of the NCC's gathers
                    GeomFetch gf = {};
                    if (prm.geom_consistency) gf = geom_fetch(kv, j + 1, gnow);
                    const float c = P::ncc(kv, pp, j + 1, px, py, h);
                    if (prm.geom_consistency) tc += wj * (c + 0.2f * geom_finish(kv, j + 1, gf, px, py));
                    else tc += wj * c;
                }
            }
        }
        tc /= weight_norm;
        if (t == 0) {
            cost_now = tc;
            my_cost = cost_now;  // costs[center] = cost_now (:1092)
            depth_now = plane_depth(c0, my_plane, px, py);
            if (prm.planar_prior) {
                depth_prior = plane_depth(c0, prior_plane, px, py);
                if (st.mask[center] > 0) {
                    float rfc[8];
                    for (int i = 0; i < 8; i++) {
                        rfc[i] = 0.0f;
                        if ((flags >> i) & 1u) {
                            const float4 ci = cand(i);
                            const float dn = plane_depth(c0, ci, px, py);
                            const float dd = dn - depth_prior;
                            const float ad = dm_acosf(dot3(prior_plane, ci));
                            const float prior = gamma + dm_expf(-dd * dd / two_dss) * dm_expf(-ad * ad / two_ass);
                            rfc[i] = dm_expf(-final_costs[i] * final_costs[i] / beta) * prior;
                        }
                    }
                    int max_idx = 0;
                    {
                        float m = rfc[0];
                        for (int i = 1; i < 8; ++i)
                            if (rfc[i] >= m) { m = rfc[i]; max_idx = i; }
                    }
                    const float dn = plane_depth(c0, my_plane, px, py);
                    const float dd = dn - depth_prior;
                    const float ad = dm_acosf(dot3(prior_plane, my_plane));
                    const float prior = gamma + dm_expf(-dd * dd / two_dss) * dm_expf(-ad * ad / two_ass);
                    const float rcn = dm_expf(-cost_now * cost_now / beta) * prior;
                    if ((flags >> max_idx) & 1u) {
                        const float4 cm = cand(max_idx);
                        const float db = plane_depth(c0, cm, px, py);
                        if (db >= prm.depth_min && db <= prm.depth_max && rfc[max_idx] > rcn) {
                            // the reference assigns a shadowing local here (:1119/:1130):
                            // the outer depth_now is NOT updated
                            my_plane = cm;
                            my_cost = final_costs[max_idx];
                            restricted_cost = rfc[max_idx];
                            my_sv = temp_sv;
                        }
                    }
                } else if ((flags >> min_cost_idx) & 1u) {
                    const float4 cm = cand(min_cost_idx);
                    const float db = plane_depth(c0, cm, px, py);
                    if (db >= prm.depth_min && db <= prm.depth_max && final_costs[min_cost_idx] < cost_now) {
                        depth_now = db;
                        my_plane = cm;
                        my_cost = final_costs[min_cost_idx];
                    }
                }
            }
            plane_now = my_plane;  // pin A3
            if (!prm.planar_prior && ((flags >> min_cost_idx) & 1u)) {
                const float4 cm = cand(min_cost_idx);
                const float db = plane_depth(c0, cm, px, py);
                if (db >= prm.depth_min && db <= prm.depth_max && final_costs[min_cost_idx] < cost_now) {
                    depth_now = db;
                    plane_now = cm;
                    cost_now = final_costs[min_cost_idx];
                    my_sv = temp_sv;
                }
            }
            // PlaneHypothesisRefinement: candidate generation (:718-741)
            float depth_rand;
            float4 plane_rand;
            if (has_prior) {
                const float dpri = plane_depth(c0, prior_plane, px, py);
                depth_prior = dpri;
                depth_rand = dm_rng_uniform(&rs) * 6 * depth_sigma + (dpri - 3 * depth_sigma);
                plane_rand = perturbed_normal(c0, px, py, prior_plane, rs, kv.angle_sigma);
            } else {
                depth_rand = dm_rng_uniform(&rs) * (prm.depth_max - prm.depth_min) + prm.depth_min;
                plane_rand = random_normal(c0, px, py, rs, depth_now);
            }
            const float perturbation = 0.02f;
            float depth_perturbed = depth_now;
            const float dmin_p = (1 - perturbation) * depth_perturbed;
            const float dmax_p = (1 + perturbation) * depth_perturbed;
            do {
                depth_perturbed = dm_rng_uniform(&rs) * (dmax_p - dmin_p) + dmin_p;
            } while (depth_perturbed < prm.depth_min && depth_perturbed > prm.depth_max);
            const float4 plane_perturbed = perturbed_normal(c0, px, py, plane_now, rs, kv.pert_pi);
            rd_rnd = depth_rand;
            rd_gen = depth_now;
            rd_pert = depth_perturbed;
            rn_now = plane_now;
            rn_rnd = plane_rand;
            rn_pert = plane_perturbed;
        } else {
            const float depth_before = plane_depth(c0, h, px, py);
            if (has_prior) {
                const float dd = ref_depth(t - 1) - depth_prior;
                const float ad = dm_acosf(dot3(prior_plane, h));
                const float prior = gamma + dm_expf(-dd * dd / two_dss) * dm_expf(-ad * ad / two_ass);
                const float rtc = dm_expf(-tc * tc / beta) * prior;
                if (depth_before >= prm.depth_min && depth_before <= prm.depth_max && rtc > restricted_cost) {
                    depth_now = depth_before;
                    plane_now = h;
                    cost_now = tc;
                    restricted_cost = rtc;
                }
            } else {
                if (depth_before >= prm.depth_min && depth_before <= prm.depth_max && tc < cost_now) {
                    depth_now = depth_before;
                    plane_now = h;
                    cost_now = tc;
                }
            }
        }
    }
    // hierarchy gate (:1163-1172)
    if (prm.hierarchy) {
        if (cost_now < st.pre_cost[center] - 0.1f) {
            my_cost = cost_now;
            my_plane = plane_now;
        }
    } else {
        my_cost = cost_now;
        my_plane = plane_now;
    }
    st.plane_nx[colour][my] = my_plane;
    st.cost_nx[colour][my] = my_cost;
    st.sv[colour][my] = my_sv;
}

// T1 kernel: costs of a given plane per pixel against every source view
// (same NCC code path as the sweep; blockIdx.z = colour).
template <int NS, typename P>
DEV void eval_body(const KViews *__restrict__ kvp, const float4 *planes, float *out, float *out_init,
                   uint32_t *out_views) {
    ACMMP_PATCH_LDS(P, lds);
    const KViews &kv = *kvp;
    const int colour = blockIdx.z;
    const BlockXY blk = xcd_block();
    P::stage(kv, lds, blk, colour, false);  // (weights computed, not from the table)
    __syncthreads();
    const LaneGeom g = lane_geom(colour, blk);
    if (g.px >= kv.W || g.py >= kv.H) return;
    const int c = g.py * kv.W + g.px;
    typename P::Pix pp = P::lane(lds, g, blk, threadIdx.y * kBX + threadIdx.x);
    P::invariants(kv, lds, g, pp, false);
    const float4 h = planes[c];
    if (out)
        for (int v = 0; v < kv.nsrc; ++v) out[(size_t)c * kv.nsrc + v] = P::ncc(kv, pp, v + 1, g.px, g.py, h);
    if (out_init) {
        uint32_t sel = 0;
        out_init[c] = initial_cost<NS, P>(kv, pp, g.px, g.py, h, sel);
        if (out_views) out_views[c] = sel;
    }
}

// ------------------------------------------------------------ the kernels
#ifndef ACMMP_GENERAL_UNIT
template <int NS, int TX>
__global__ __launch_bounds__(kThreads) void k_init(const KViews *__restrict__ kvp, KState st) {
    init_body<NS, FastPatch<TX>>(kvp, st);
}
template <int NS, int TX>
__global__ __launch_bounds__(kThreads, kSweepWaves) void k_sweep_f(const KViews *__restrict__ kvp, KState st,
                                                                   int colour, int iter) {
    sweep_body<NS, FastPatch<TX>>(kvp, st, colour, iter);
}
template <int NS, int TX>
__global__ __launch_bounds__(kThreads) void k_eval_costs(const KViews *__restrict__ kvp, const float4 *planes,
                                                         float *out, float *out_init, uint32_t *out_views) {
    eval_body<NS, FastPatch<TX>>(kvp, planes, out, out_init, out_views);
}
#define ACMMP_K_INIT k_init
#define ACMMP_K_SWEEP k_sweep_f
#define ACMMP_K_EVAL k_eval_costs
#define ACMMP_LAUNCH(name) tx_launch_##name
#else
template <int NS, int TX>
__global__ __launch_bounds__(kThreads) void k_init_g(const KViews *__restrict__ kvp, KState st) {
    init_body<NS, GeneralPatch<TX>>(kvp, st);
}
template <int NS, int TX>
__global__ __launch_bounds__(kThreads, kSweepWaves) void k_sweep_g(const KViews *__restrict__ kvp, KState st,
                                                                   int colour, int iter) {
    sweep_body<NS, GeneralPatch<TX>>(kvp, st, colour, iter);
}
template <int NS, int TX>
__global__ __launch_bounds__(kThreads) void k_eval_costs_g(const KViews *__restrict__ kvp, const float4 *planes,
                                                           float *out, float *out_init, uint32_t *out_views) {
    eval_body<NS, GeneralPatch<TX>>(kvp, planes, out, out_init, out_views);
}
#define ACMMP_K_INIT k_init_g
#define ACMMP_K_SWEEP k_sweep_g
#define ACMMP_K_EVAL k_eval_costs_g
#define ACMMP_LAUNCH(name) gx_launch_##name
#endif

// Source-view count -> array capacity of the templated kernels.
static int ns_bucket(int nsrc) {
    if (nsrc <= 4) return 4;
    if (nsrc <= 9) return 9;
    if (nsrc <= 16) return 16;
    if (nsrc <= 20) return 20;
    return 32;
}

#define ACMMP_NS_SWITCH(KERNEL, GRID, STREAM, ...)                                                         \
    switch (ns_bucket(nsrc)) {                                                                              \
        case 4: KERNEL<4, ACMMP_TX_UNIT><<<GRID, dim3(kBX, kBY), 0, STREAM>>>(__VA_ARGS__); break;          \
        case 9: KERNEL<9, ACMMP_TX_UNIT><<<GRID, dim3(kBX, kBY), 0, STREAM>>>(__VA_ARGS__); break;          \
        case 16: KERNEL<16, ACMMP_TX_UNIT><<<GRID, dim3(kBX, kBY), 0, STREAM>>>(__VA_ARGS__); break;        \
        case 20: KERNEL<20, ACMMP_TX_UNIT><<<GRID, dim3(kBX, kBY), 0, STREAM>>>(__VA_ARGS__); break;        \
        default: KERNEL<32, ACMMP_TX_UNIT><<<GRID, dim3(kBX, kBY), 0, STREAM>>>(__VA_ARGS__); break;        \
    }

template <>
hipError_t ACMMP_LAUNCH(init)<ACMMP_TX_UNIT>(const KViews *d_kv, int nsrc, dim3 grid, hipStream_t s, KState st) {
    ACMMP_NS_SWITCH(ACMMP_K_INIT, grid, s, d_kv, st);
    return hipGetLastError();
}
template <>
hipError_t ACMMP_LAUNCH(sweep)<ACMMP_TX_UNIT>(const KViews *d_kv, int nsrc, dim3 grid, hipStream_t s, KState st,
                                              int colour, int iter) {
    ACMMP_NS_SWITCH(ACMMP_K_SWEEP, grid, s, d_kv, st, colour, iter);
    return hipGetLastError();
}
template <>
hipError_t ACMMP_LAUNCH(eval)<ACMMP_TX_UNIT>(const KViews *d_kv, int nsrc, dim3 grid, hipStream_t s,
                                             const float4 *planes, float *out, float *out_init,
                                             uint32_t *out_views) {
    ACMMP_NS_SWITCH(ACMMP_K_EVAL, grid, s, d_kv, planes, out, out_init, out_views);
    return hipGetLastError();
}

}  // namespace acmmp

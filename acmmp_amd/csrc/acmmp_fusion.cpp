// acmmp_fusion.cpp — RunFusion (src/acmmp_definitions.cpp:828-1043), SURVEY §8f rank 3:
// depth/normal maps of all views -> one coloured point cloud (<out>/ACMMP_model.ply,
// StoreColorPlyFileBinaryPointCloud src/ACMMP.cpp:382-424), and RunPriorAwareFusion (:573-826,
// <out>/ACMMP_prior_model.ply).
//
// Host code, literal: the reference's fusion is order-dependent (a pixel's approval masks pixels of
// other views that later pixels then skip, and used_list is never reset between pixels), so
// approvals run sequentially in the reference's order with the reference's float expression order
// (Get3DPointonWorld / ProjectonCamera src/ACMMP.cpp:203-251, GetAngle :253-262). Only the
// per-pixel projections and tests before an approval run on other threads. That is exact because
// masks only ever go 0 -> 1 and depths do not change: a source or pixel found masked stays masked,
// so the candidate stage may read the masks as they stand at any moment, and the walk re-checks
// what passed against the masks as they stand at approval.
//
// What the Jacobi-order device fusion (acmmp_fusion_dev.hip) needs as well lives in
// acmmp_fusion_host.h: world_point / project, CacheDomain, Pool, pool_for, MaskBits, Scene,
// FusionInputs, the loaders (load_view .. load_prior_view: both orders of a fusion load the same
// way), check_view_sizes, store_ply, the error string. This file builds without HIP.
//
// The file, in order (RunFusion unless said otherwise):
//   get_angle .. stage_reproject     the reference's float expressions, vectorised stages
//   candidates_row  (pool workers, a row each; InFlight holds the job and waits
//                   on every way out) a view's live pixels and their hits:
//                   (source slot, source pixel, exp(-index)), source-major
//   walk_view       (calling thread, the masks' only writer) the reference's
//                   pixel order over those hits: points out, mask bits set;
//                   view i + 1's candidates run beside it into the other ViewHits
//   metric_of .. candidates          the prior-aware fusion's per-pixel tests
//   acmmp_run_fusion                 load, resolve, wait i / start i + 1 / walk i, PLY
//   acmmp_run_prior_aware_fusion     the same two steps per band of 32 rows, byte masks
//
// Deviations: no cv::imshow (:897-900); the PLY is written in point order (the reference's
// OpenMP-critical writes make its order arbitrary); a colour image whose size differs from its
// depth map is resized with a float bilinear filter (cv::resize's 8-bit fixed-point path is
// unpinned).
#include "acmmp_fusion_host.h"

namespace {

using namespace acmmp_fusion_host;

float get_angle(const float *a, const float *b) {  // GetAngle
    const float dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    const float angle = std::acos(dot);
    if (angle != angle) return 0.0f;
    return angle;
}

// The two arithmetic stages of RunFusion's candidates_row: branch-free
// loops the vectoriser turns into AVX2 where the host has it. Each is built
// twice (target_clones: an AVX2 clone and a baseline x86-64 clone, picked by
// the loader from the running CPU), so the library never executes an AVX2
// instruction on a host without it. AVX2 without FMA, and this file builds
// with -ffp-contract=off: both clones perform the same IEEE operations, so
// the PLY does not depend on the host.
__attribute__((target_clones("avx2", "default")))
void stage_project(const F3 *X, size_t nl, const acmmp_camera &cs, int *scp, int *srp) {
    for (size_t k = 0; k < nl; ++k) {
        float ptx, pty, proj_depth;
        project(X[k], cs, ptx, pty, proj_depth);
        srp[k] = int(pty + 0.5f);
        scp[k] = int(ptx + 0.5f);
    }
}

// reprojection of candidate q's source pixel into view i (row r): error and
// relative depth difference
__attribute__((target_clones("avx2", "default")))
void stage_reproject(size_t nc, int r, const int *__restrict__ col, const int *__restrict__ scp,
                     const int *__restrict__ srp, const float *__restrict__ cd, const float *__restrict__ cr,
                     float *__restrict__ re, float *__restrict__ rd, const acmmp_camera cs, const acmmp_camera ci) {
    for (size_t q = 0; q < nc; ++q) {
        const float ref_depth = cr[q];
        float tx, ty, proj_depth;
        const F3 tmp_X = world_point(scp[q], srp[q], cd[q], cs);
        project(tmp_X, ci, tx, ty, proj_depth);
        // std::pow(v, 2) of a float v is exact in double: v * v
        const double dx = (double)(col[q] - tx), dy = (double)(r - ty);
        re[q] = (float)std::sqrt(dx * dx + dy * dy);
        rd[q] = std::fabs(proj_depth - ref_depth) / ref_depth;
    }
}

// ---- RunFusion's two stages per view (see the top for why they are exact).
// A hit = (source slot j, source pixel sp) packed in 32 bits; its
// exp(-tmp_index) is kept beside it, and every live pixel's sum of them
// (ascending j, as the walk adds) is precomputed: the walk reads the
// per-hit values only for pixels where some hit became masked.
constexpr int kSpBits = 27;
constexpr uint32_t kSpMask = (1u << kSpBits) - 1;
constexpr uint32_t kNoHit = 0xffffffffu;

struct ViewHits {
    std::vector<std::vector<uint32_t>> hit;    // hits of row r, pixel order: j << kSpBits | sp
    std::vector<std::vector<float>> ex;        // their exp(-tmp_index)
    // per live pixel of row r (the candidate stage's order: ascending column)
    // -- the walk visits only these (a pixel not live then stays so:
    // masks only go 0 -> 1 and depths do not change)
    std::vector<std::vector<int>> live;        // its column
    std::vector<std::vector<uint16_t>> nhit;   // its number of hits
    std::vector<std::vector<float>> sum;       // sum of its hits' ex, ascending j
    std::vector<std::vector<F3>> X;            // its world point
    void resize(size_t rows) {
        hit.resize(rows), ex.resize(rows), live.resize(rows), nhit.resize(rows), sum.resize(rows), X.resize(rows);
    }
};

struct RowScratch {
    std::vector<F3> X;
    std::vector<int> live;           // columns of the live pixels
    std::vector<uint32_t> sp;        // [live k][j]: source pixel of a hit, or kNoHit
    std::vector<float> e;            // [live k][j]: its exp(-tmp_index)
    // one source's pass over the row, in stages (see candidates_row)
    std::vector<int> src_c, src_r;   // [live k]: the projected source pixel
    std::vector<int> cand;           // live indices whose source pixel is in bounds, unmasked, depth > 0
    std::vector<int> ccol, csc, csr; // ... its column and source pixel
    std::vector<float> cdepth, cref; // ... its source depth and reference depth
    std::vector<float> rerr, rdiff;  // [cand q]: reprojection error, relative depth difference
};

// Row r of view i: every pixel's per-source projections and consistency tests against the masks as
// they stand. Source-major inside the row: every live pixel's world point first, then one source at
// a time over the row (its depth/normal/mask reads follow the row's projection into that source
// instead of hopping between 20 sources per pixel), then each pixel's hits in ascending j as the
// reference adds them (same values, same order).
void candidates_row(const Scene &sc, size_t i, int r, ViewHits &vh) {
    thread_local RowScratch rs;
    const int W = sc.cols[i];
    const int num_ngb = sc.problems[i].num_src_images;
    const float depth_max = sc.cameras[i].depth_max;
    std::vector<uint32_t> &h = vh.hit[(size_t)r];
    std::vector<float> &hx = vh.ex[(size_t)r];
    std::vector<uint16_t> &nh = vh.nhit[(size_t)r];
    std::vector<float> &sum = vh.sum[(size_t)r];
    std::vector<F3> &X = vh.X[(size_t)r];
    h.clear();
    hx.clear();
    rs.live.clear();
    rs.X.clear();
    for (int c = 0; c < W; ++c) {
        const size_t pc = (size_t)r * W + c;
        if (sc.masks[i].get(pc)) continue;
        const float ref_depth = sc.depths[i][pc];
        if (ref_depth <= 0.0 || ref_depth >= depth_max) continue;
        rs.live.push_back(c);
        rs.X.push_back(world_point(c, r, ref_depth, sc.cameras[i]));
    }
    const size_t nl = rs.live.size();
    const size_t nj = (size_t)std::max(num_ngb, 1);
    rs.sp.assign(nl * nj, kNoHit);
    rs.e.resize(nl * nj);
    nh.resize(nl);
    sum.resize(nl);
    rs.src_c.resize(nl);
    rs.src_r.resize(nl);
    for (int j = 0; j < num_ngb; ++j) {
        const int s = sc.src_index[i][j];
        const int src_cols = sc.cols[s], src_rows = sc.rows[s];
        // Per source, the reference's per-pixel test in four stages over
        // the row's live pixels (the same operations on the same values:
        // the two arithmetic stages are branch-free loops the compiler
        // vectorises; the gathers and the mask reads stay scalar).
        // (1) the projection into the source
        stage_project(rs.X.data(), nl, sc.cameras[s], rs.src_c.data(), rs.src_r.data());
        // (2) in bounds, unmasked, positive source depth: the candidates,
        // with what stage 3 reads, in contiguous arrays
        rs.cand.resize(nl);
        rs.ccol.resize(nl);
        rs.csc.resize(nl);
        rs.csr.resize(nl);
        rs.cdepth.resize(nl);
        rs.cref.resize(nl);
        size_t nc = 0;
        const float *dref = sc.depths[i].data() + (size_t)r * W;
        for (size_t k = 0; k < nl; ++k) {
            const int src_r = rs.src_r[k], src_c = rs.src_c[k];
            if (!(src_c >= 0 && src_c < src_cols && src_r >= 0 && src_r < src_rows)) continue;
            const size_t sp = (size_t)src_r * src_cols + src_c;
            if (sc.masks[s].get(sp)) continue;
            const float src_depth = sc.depths[s][sp];
            if (src_depth <= 0.0) continue;
            rs.cand[nc] = (int)k;
            rs.ccol[nc] = rs.live[k];
            rs.csc[nc] = src_c;
            rs.csr[nc] = src_r;
            rs.cdepth[nc] = src_depth;
            rs.cref[nc] = dref[rs.live[k]];
            ++nc;
        }
        // (3) the reprojection into view i: error and relative depth difference
        rs.rerr.resize(nc);
        rs.rdiff.resize(nc);
        stage_reproject(nc, r, rs.ccol.data(), rs.csc.data(), rs.csr.data(), rs.cdepth.data(), rs.cref.data(),
                        rs.rerr.data(), rs.rdiff.data(), sc.cameras[s], sc.cameras[i]);
        // (4) the reference evaluates all three before the test; acos is
        // pure, so the angle is only formed where the first two pass
        for (size_t q = 0; q < nc; ++q) {
            const float reproj_error = rs.rerr[q], relative_depth_diff = rs.rdiff[q];
            if (!(reproj_error < 2.0f && relative_depth_diff < 0.01f)) continue;
            const int k = rs.cand[q];
            const size_t pc = (size_t)r * W + rs.ccol[q];
            const size_t sp = (size_t)rs.csr[q] * src_cols + rs.csc[q];
            const float angle = get_angle(&sc.normals[i][pc * 3], &sc.normals[s][sp * 3]);
            if (angle < 0.174533f) {
                const float tmp_index = reproj_error + 200 * relative_depth_diff + angle * 10;
                rs.sp[(size_t)k * nj + (size_t)j] = (uint32_t)sp;
                rs.e[(size_t)k * nj + (size_t)j] = std::exp(-tmp_index);
            }
        }
    }
    for (size_t k = 0; k < nl; ++k) {
        const size_t k0 = h.size();
        float total = 0;
        for (int j = 0; j < num_ngb; ++j) {
            const uint32_t sp = rs.sp[k * nj + (size_t)j];
            if (sp == kNoHit) continue;
            const float e = rs.e[k * nj + (size_t)j];
            h.push_back((uint32_t)j << kSpBits | sp);
            hx.push_back(e);
            total += e;
        }
        nh[k] = (uint16_t)(h.size() - k0);
        sum[k] = total;
    }
    // the walk emits an approved pixel's point from here (the same
    // world_point call the reference makes at approval, :1012)
    X.swap(rs.X);
    vh.live[(size_t)r].swap(rs.live);
}

// A view's candidate job on the pool. Its rows read the scene and write a
// ViewHits buffer, so it must be over before either dies: declare this after
// both, and every way out of the scope waits first.
struct InFlight {
    Pool &pool;
    std::shared_ptr<Pool::Job> job;
    ~InFlight() { wait(); }
    void start(const Scene &sc, size_t i, ViewHits &vh) {
        vh.resize((size_t)sc.rows[i]);
        job = pool.submit(sc.rows[i], [&sc, &vh, i](int r) { candidates_row(sc, i, r, vh); });
    }
    void wait() {
        if (job) pool.wait(job);
        job.reset();
    }
};

struct WalkStats {
    size_t n_live = 0, n_hits = 0, n_masked = 0;
    double t_wait = 0, t_walk = 0;
};

// The approval walk of view i, in the reference's pixel order: the sources that passed in the
// candidate stage are re-checked against the current masks and accumulated in ascending j (same exp
// values, same sum order), then points are emitted and masks / used_list updated. `approved`, if
// not null, is the view's W x H debug image.
void walk_view(Scene &sc, size_t i, const ViewHits &vh, int con_num_thresh, float consistency_scalar,
               std::vector<Point> &cloud, uint8_t *approved, WalkStats &stats) {
    const int W = sc.cols[i], H = sc.rows[i];
    const int num_ngb = sc.problems[i].num_src_images;
    size_t n_live = 0, n_hits = 0, n_masked = 0;
    // per source: its mask words; used_list as mask indices (-1 unset)
    std::vector<uint64_t *> mw((size_t)std::max(num_ngb, 1));
    for (int j = 0; j < num_ngb; ++j) mw[(size_t)j] = sc.masks[(size_t)sc.src_index[i][j]].w.data();
    std::vector<int64_t> used_sp((size_t)std::max(num_ngb, 1), -1);
    uint32_t dirty = 0;  // used_sp entries written since the last approval
    for (int r = 0; r < H; ++r) {
        const uint32_t *h = vh.hit[(size_t)r].data();
        const float *hx = vh.ex[(size_t)r].data();
        const std::vector<int> &lv = vh.live[(size_t)r];
        const uint16_t *nhr = vh.nhit[(size_t)r].data();
        const float *sumr = vh.sum[(size_t)r].data();
        const F3 *xr = vh.X[(size_t)r].data();
        const size_t nl = lv.size();
        for (size_t k = 0; k < nl; ++k) {  // the pixels live in the candidate stage, in column order
            const int c = lv[k];
            const size_t pc = (size_t)r * W + c;
            const int nh = nhr[k];
            const uint32_t *hp = h;
            const float *hxp = hx;
            const F3 *xp = xr + k;
            h += nh;
            hx += nh;
            // re-read: view i - 1's walk (beside view i's candidate stage) and,
            // if i is its own source, view i's own approvals set bits
            if (sc.masks[i].get(pc)) continue;
            int num_consistent = 0;
            bool masked = false;
            for (int q = 0; q < nh; ++q) {
                const uint32_t j = hp[q] >> kSpBits, sp = hp[q] & kSpMask;
                if (MaskBits::bit(mw[j], sp)) {
                    masked = true;
                    continue;
                }
                used_sp[j] = sp;
                dirty |= 1u << j;
                num_consistent++;
            }
            float dynamic_consistency = sumr[k];
            n_live++;
            n_hits += (size_t)nh;
            n_masked += masked;
            if (masked) {  // re-add the unmasked ones, ascending j
                dynamic_consistency = 0;
                for (int q = 0; q < nh; ++q)
                    if (!MaskBits::bit(mw[hp[q] >> kSpBits], hp[q] & kSpMask)) dynamic_consistency += hxp[q];
            }
            if (num_consistent >= con_num_thresh && (dynamic_consistency > consistency_scalar * num_consistent)) {
                const float *ref_normal = &sc.normals[i][pc * 3];
                const uint8_t *bgr = &sc.images[i][pc * 3];
                Point p;
                p.coord = *xp;  // world_point(c, r, depths[i][pc], cameras[i]), formed in the candidate stage
                p.normal = F3{ref_normal[0], ref_normal[1], ref_normal[2]};
                p.color = F3{(float)bgr[0], (float)bgr[1], (float)bgr[2]};
                cloud.push_back(p);
                // used_list is not reset per pixel in the reference: stale
                // entries apply too. An entry unchanged since the last
                // approval was set then (masks only go 0 -> 1), so only
                // the entries written since are applied.
                for (; dirty; dirty &= dirty - 1) {
                    const int j = __builtin_ctz(dirty);
                    const int64_t sp = used_sp[(size_t)j];
                    const int s = sc.src_index[i][j];
                    sc.masks[s].set((size_t)sp);
                    if (approved) {
                        // `approved` is this view's W x H image indexed by source coordinates (:1030)
                        const int ux = (int)(sp % sc.cols[s]), uy = (int)(sp / sc.cols[s]);
                        if (uy < H && ux < W) approved[(size_t)uy * W + ux] = 255;
                    }
                }
            }
        }
    }
    stats.n_live += n_live, stats.n_hits += n_hits, stats.n_masked += n_masked;
}

using Clock = std::chrono::steady_clock;
double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// ---- prior-aware fusion helpers (src/acmmp_definitions.cpp:443-571)
struct CInfo {  // struct c_info
    float dynamic_consistency = 0;
    int x = 0, y = 0;
    bool below_thresh = false;
    int im_num = -1;
};

struct CMetric {  // struct cmetric
    float reproj_err = 1e6, relative_depth_diff = 1e6, angle = 1e6;
};

CMetric metric_of(const FusionInputs &in, size_t i, int r, int c, float ref_depth, const float *ref_normal, int src,
                  int src_r, int src_c, float src_depth, const float *src_normal) {
    CMetric m;
    if (src_depth > 0) {
        const F3 tmp_X = world_point(src_c, src_r, src_depth, in.cameras[src]);
        float tx, ty, proj_depth;
        project(tmp_X, in.cameras[i], tx, ty, proj_depth);
        const double dx = (double)(c - tx), dy = (double)(r - ty);  // std::pow(v, 2), exact as v * v
        m.reproj_err = (float)std::sqrt(dx * dx + dy * dy);
        m.relative_depth_diff = std::fabs(proj_depth - ref_depth) / ref_depth;
        m.angle = get_angle(ref_normal, src_normal);
    }
    return m;
}

// get_consistency_metrics (:443-516)
CInfo consistency_metrics(const FusionInputs &in, size_t i, int r, int c, float ref_depth, const float *ref_normal,
                          int src, int src_r, int src_c) {
    const size_t sp = (size_t)src_r * in.cols[src] + src_c;
    const CMetric res0 = metric_of(in, i, r, c, ref_depth, ref_normal, src, src_r, src_c, in.depths[src][sp],
                                   &in.normals[src][sp * 3]);
    const CMetric res1 = metric_of(in, i, r, c, ref_depth, ref_normal, src, src_r, src_c, in.pdepths[src][sp],
                                   &in.pnormals[src][sp * 3]);
    const bool t0 = res0.reproj_err < 2.0f && res0.relative_depth_diff < 0.01f && res0.angle < 0.174533f;
    const bool t1 = res1.reproj_err < 2.0f && res1.relative_depth_diff < 0.01f && res1.angle < 0.174533f;
    CInfo out;
    out.x = src_c;
    out.y = src_r;
    const float dc0 = std::exp(-(res0.reproj_err + 200 * res0.relative_depth_diff + res0.angle * 10));
    const float dc1 = std::exp(-(res1.reproj_err + 200 * res1.relative_depth_diff + res1.angle * 10));
    if (t0 && t1) {
        out.dynamic_consistency = std::fmax(dc0, dc1);
        out.below_thresh = true;
        out.im_num = src;
    } else if (t0) {
        out.dynamic_consistency = dc0;
        out.below_thresh = true;
        out.im_num = src;
    } else if (t1) {
        out.dynamic_consistency = dc1;
        out.below_thresh = true;
        out.im_num = src;
    }
    return out;
}

// getCandidates (:520-571)
void candidates(const FusionInputs &in, const std::vector<std::vector<uint8_t>> &masks, const std::vector<int> &srcs,
                size_t i, int r, int c, float ref_depth, const float *ref_normal, std::vector<CInfo> &out) {
    out.clear();
    for (const int s : srcs) {
        const F3 PointX = world_point(c, r, ref_depth, in.cameras[i]);
        float px, py, proj_depth;
        project(PointX, in.cameras[s], px, py, proj_depth);
        const int src_r = int(py + 0.5f);
        const int src_c = int(px + 0.5f);
        if (src_c >= 0 && src_c < in.cols[s] && src_r >= 0 && src_r < in.rows[s]) {
            if (masks[s][(size_t)src_r * in.cols[s] + src_c] == 1) continue;
            out.push_back(consistency_metrics(in, i, r, c, ref_depth, ref_normal, s, src_r, src_c));
        }
    }
}

}  // namespace

extern "C" {

const char *acmmp_fusion_last_error(void) { return f_err.c_str(); }

// the host ends of the in-memory fusion (acmmp_fuse_views_jacobi, acmmp_fusion_dev.hip): in this
// unit, which needs no HIP, so the sanitizer tier builds them with a plain C++ compiler
int acmmp_write_ply_points(const char *path, const float *xyz, const float *normal, const uint8_t *rgb, int64_t n) {
    if (!path || n < 0 || (n > 0 && (!xyz || !normal || !rgb)))
        return ffail(ACMMP_ERR_ARG, "acmmp_write_ply_points: null path or array, or n below 0");
    if (n > INT32_MAX) return ffail(ACMMP_ERR_ARG, "acmmp_write_ply_points: %lld points exceed the header's int", (long long)n);
    Pool pool;
    return store_ply_arrays(path, xyz, normal, rgb, (size_t)n, &pool);
}

int acmmp_resize_bilinear_u8(const uint8_t *src, int sw, int sh, int channels, uint8_t *dst, int dw, int dh) {
    if (!src || !dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || channels < 1 || channels > 4)
        return ffail(ACMMP_ERR_ARG, "acmmp_resize_bilinear_u8: null image, empty size or channels outside 1..4");
    resize_u8(src, sw, sh, channels, dst, dw, dh);
    return ACMMP_OK;
}

int acmmp_run_fusion(const char *dense_folder, const char *output_folder, const acmmp_problem *problems, int count,
                     int geom_consistency, float consistency_scalar, int con_num_thresh, const char *image_dir,
                     const char *mask_folder, int write_debug_images, int *num_points) {
    if (!dense_folder || !output_folder || !problems || count <= 0) return ffail(ACMMP_ERR_ARG, "bad args");
    const std::string dense = dense_folder, out = output_folder;
    const size_t n = (size_t)count;
    const bool timing = std::getenv("ACMMP_HOST_TIMING") != nullptr;
    const auto t_start = Clock::now();
    Scene sc(problems, n);
    // The threads are confined to one last-level-cache domain BEFORE the loads, and the loads run on
    // that domain's pool: maps, images and masks are then first touched (allocated) on the memory node
    // of the walk's core, which reads them. (Loaded by threads all over a 2-socket host, part of them
    // lay on the other node: walk 0.85 or 1.3 s from run to run, profiles/r05_fusion_walk_ab3.jsonl.)
    CacheDomain dom;
    Pool pool(&dom);
    int rc = load_fusion_views(sc, pool, dense_folder, output_folder, geom_consistency, image_dir, mask_folder);
    if (!rc) rc = check_view_sizes(sc);  // (a hit packs the pixel in kSpBits = 27 bits, the slot in 5)
    if (rc) return rc;
    std::vector<Point> cloud;  // reserved once (pages are committed as points arrive): no copies in the walk
    cloud.reserve(sc.pixels());
    ViewHits vhits[2];
    WalkStats stats;
    const auto t_loaded = Clock::now();
    InFlight job{pool, nullptr};  // declared after all its rows touch: sc, vhits
    job.start(sc, 0, vhits[0]);
    for (size_t i = 0; i < n; ++i) {
        const int W = sc.cols[i], H = sc.rows[i];
        std::vector<uint8_t> approved(write_debug_images ? (size_t)W * H : 0, 0);
        const auto t0 = Clock::now();
        job.wait();
        const auto t1 = Clock::now();
        if (i + 1 < n) job.start(sc, i + 1, vhits[(i + 1) & 1]);
        walk_view(sc, i, vhits[i & 1], con_num_thresh, consistency_scalar, cloud,
                  write_debug_images ? approved.data() : nullptr, stats);
        stats.t_wait += secs(t0, t1);
        stats.t_walk += secs(t1, Clock::now());
        if (write_debug_images) {
            const std::string dbg = dense + "/approved_pixels_cam_" + std::to_string(i) + ".png";
            if (acmmp_internal_write_png(dbg.c_str(), W, H, 1, approved.data()))
                return ffail(ACMMP_ERR_IO, "cannot write %s", dbg.c_str());
        }
    }
    if (num_points) *num_points = (int)cloud.size();
    const auto t_walked = Clock::now();
    rc = store_ply(out + "/ACMMP_model.ply", cloud, &pool);
    if (timing)
        std::fprintf(stderr,
                     "[RunFusion] load=%.2fs candidates_wait=%.2fs walk=%.2fs ply=%.2fs threads=%d "
                     "walked_pixels=%zu hits=%zu pixels_with_masked_hits=%zu points=%zu pinned=%d\n",
                     secs(t_start, t_loaded), stats.t_wait, stats.t_walk, secs(t_walked, Clock::now()),
                     pool.size() + 1, stats.n_live, stats.n_hits, stats.n_masked, cloud.size(), (int)dom.pinned());
    return rc;
}

int acmmp_run_prior_aware_fusion(const char *dense_folder, const char *output_folder, const char *fusion_folder,
                                 const acmmp_problem *problems, int count, int geom_consistency,
                                 float consistency_scalar, int num_consistent_thresh, int single_match_penalty,
                                 int *num_points) {
    if (!dense_folder || !output_folder || !fusion_folder || !problems || count <= 0)
        return ffail(ACMMP_ERR_ARG, "bad args");
    const std::string dense = dense_folder, out = output_folder, fus = fusion_folder;
    const size_t n = (size_t)count;
    FusionInputs in(problems, n);
    std::vector<std::vector<uint8_t>> &images = in.images, masks(n);
    for (size_t i = 0; i < n; ++i) {  // one after the other, on the calling thread
        if (const int rc = load_prior_view(in, i, dense, out, fus, depth_suffix(geom_consistency))) return rc;
        masks[i].assign((size_t)in.cols[i] * in.rows[i], 0);
    }
    const int src_rc = resolve_sources(in);
    if (src_rc) return src_rc;
    std::vector<Point> cloud;
    cloud.reserve(in.pixels());  // at most one point per pixel (see RunFusion)
    Pool pool;
    // RunFusion's two steps per band of rows: candidates (projection + metrics of both maps) on host
    // threads against the current masks, then the reference's pixel order with every approval re-checked
    struct Ok {  // a below-threshold candidate: the only kind that counts or masks
        int im, x, y;
        float dc;
    };
    const int band = 32;
    for (size_t i = 0; i < n; ++i) {
        const int W = in.cols[i], H = in.rows[i];
        const std::vector<int> &srcs = in.src_index[i];
        const int ns = std::max((int)srcs.size(), 1);
        // per pixel: bit 0 live, bit 1 map 0 evaluated, bit 2 map 1 evaluated
        std::vector<uint8_t> state((size_t)band * W);
        std::vector<uint8_t> cnt((size_t)band * W * 2);
        std::vector<Ok> oks((size_t)band * W * 2 * ns);
        for (int r0 = 0; r0 < H; r0 += band) {
            const int r1 = std::min(H, r0 + band);
            pool.wait(pool.submit(r1 - r0, [&](int rr) {
                const int r = r0 + rr;
                std::vector<CInfo> cand;
                for (int c = 0; c < W; ++c) {
                    const size_t pc = (size_t)r * W + c, q = (size_t)rr * W + c;
                    state[q] = 0;
                    if (masks[i][pc] == 1) continue;
                    const float ref_depth = in.depths[i][pc], ref_p_depth = in.pdepths[i][pc];
                    if (ref_depth <= 0.0 && ref_p_depth <= 0.0) continue;
                    uint8_t st = 1;
                    for (int b = 0; b < 2; ++b) {
                        const float d = b ? ref_p_depth : ref_depth;
                        cnt[2 * q + b] = 0;
                        if (!(d > 0.0)) continue;
                        st |= (uint8_t)(2 << b);
                        candidates(in, masks, srcs, i, r, c, d, b ? &in.pnormals[i][pc * 3] : &in.normals[i][pc * 3],
                                   cand);
                        Ok *o = &oks[(2 * q + b) * ns];
                        int k = 0;
                        for (const CInfo &ci : cand)
                            if (ci.below_thresh) o[k++] = Ok{ci.im_num, ci.x, ci.y, ci.dynamic_consistency};
                        cnt[2 * q + b] = (uint8_t)k;
                    }
                    state[q] = st;
                }
            }));
            for (int r = r0; r < r1; ++r) {
                for (int c = 0; c < W; ++c) {
                    const size_t pc = (size_t)r * W + c, q = (size_t)(r - r0) * W + c;
                    if (!state[q] || masks[i][pc] == 1) continue;
                    const float ref_depth = in.depths[i][pc], ref_p_depth = in.pdepths[i][pc];
                    const float *ref_normal = &in.normals[i][pc * 3], *ref_p_normal = &in.pnormals[i][pc * 3];
                    float d_cons[2] = {0, 0};
                    int nb[2] = {0, 0};
                    bool t[2] = {false, false};
                    for (int b = 0; b < 2; ++b) {
                        if (!(state[q] & (2 << b))) continue;
                        Ok *o = &oks[(2 * q + b) * ns];
                        int keep = 0;
                        for (int k = 0; k < cnt[2 * q + b]; ++k) {
                            if (masks[o[k].im][(size_t)o[k].y * in.cols[o[k].im] + o[k].x] == 1) continue;
                            nb[b]++;
                            d_cons[b] += o[k].dc;
                            o[keep++] = o[k];
                        }
                        cnt[2 * q + b] = (uint8_t)keep;
                        t[b] = (nb[b] >= num_consistent_thresh) && (d_cons[b] > consistency_scalar * nb[b]);
                    }
                    int pick = 0;
                    bool passing = false;
                    float g_depth = 0;
                    const float *g_normal = ref_normal;
                    if (t[0] && t[1]) {  // (:754-769)
                        passing = true;
                        pick = nb[1] >= nb[0] ? 1 : 0;
                    } else if (t[1]) {
                        passing = nb[1] >= (num_consistent_thresh + single_match_penalty);
                        pick = 1;
                    } else {
                        passing = t[0] && nb[0] >= (num_consistent_thresh + single_match_penalty);
                        pick = 0;
                    }
                    g_depth = pick ? ref_p_depth : ref_depth;
                    g_normal = pick ? ref_p_normal : ref_normal;
                    if (passing) {
                        Point p;
                        p.coord = world_point(c, r, g_depth, in.cameras[i]);
                        p.normal = F3{g_normal[0], g_normal[1], g_normal[2]};
                        const uint8_t *bgr = &images[i][pc * 3];
                        p.color = F3{(float)bgr[0], (float)bgr[1], (float)bgr[2]};
                        cloud.push_back(p);
                        const Ok *o = &oks[(2 * q + pick) * ns];
                        for (int k = 0; k < cnt[2 * q + pick]; ++k)
                            masks[o[k].im][(size_t)o[k].y * in.cols[o[k].im] + o[k].x] = 1;
                    }
                }
            }
        }
    }
    if (num_points) *num_points = (int)cloud.size();
    return store_ply(out + "/ACMMP_prior_model.ply", cloud);
}

}  // extern "C"

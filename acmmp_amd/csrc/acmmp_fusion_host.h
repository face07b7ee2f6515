// acmmp_fusion_host.h — what the fusions' host code shares (internal, all inline):
// acmmp_fusion.cpp (RunFusion literal, RunPriorAwareFusion) and acmmp_fusion_dev.hip
// (both fusions in Jacobi order on the device). No HIP in here: acmmp_fusion.cpp builds
// with a plain C++ compiler.
//   f_err, ffail                     the message behind acmmp_fusion_last_error (one per thread)
//   world_point, project             the reference's float expressions (host and device)
//   CacheDomain, Pool, pool_for      one L3 domain: the caller walks, workers do the rest
//   MaskBits, Scene, FusionInputs    a fusion's inputs; masks one bit a pixel
//   load_view .. resolve_sources     one view loader and source lookup for all fusions
//   check_view_sizes                 2^27 pixels / 32 sources: RunFusion (both orders), the device folder calls
//   load_fusion_views                RunFusion's inputs from its raw arguments (both orders)
//   load_prior_view                  a view of RunPriorAwareFusion, both map pairs (both orders)
//   store_ply, store_ply_arrays      27-byte records in chunks (pool or caller)
//   check_fusion_views               acmmp_fuse_views_jacobi's argument checks
#ifndef ACMMP_FUSION_HOST_H_
#define ACMMP_FUSION_HOST_H_

#include <sched.h>
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/acmmp.h"
#include "acmmp_dense.h"
#include "acmmp_hostio.h"

namespace acmmp_fusion_host {

using acmmp_dense::camera_path;
using acmmp_dense::id8;
using acmmp_dense::result_folder;

#if defined(__HIPCC__)
#define ACMMP_FUSION_HD __host__ __device__
#else
#define ACMMP_FUSION_HD
#endif

inline thread_local std::string f_err;

inline int ffail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    f_err = buf;
    return code;
}

struct F3 {
    float x, y, z;
};

ACMMP_FUSION_HD inline F3 world_point(int x, int y, float depth, const acmmp_camera &c) {  // Get3DPointonWorld
    F3 p;
    p.x = depth * (x - c.K[2]) / c.K[0];
    p.y = depth * (y - c.K[5]) / c.K[4];
    p.z = depth;
    F3 t;
    t.x = c.R[0] * p.x + c.R[3] * p.y + c.R[6] * p.z;
    t.y = c.R[1] * p.x + c.R[4] * p.y + c.R[7] * p.z;
    t.z = c.R[2] * p.x + c.R[5] * p.y + c.R[8] * p.z;
    F3 C;
    C.x = -(c.R[0] * c.t[0] + c.R[3] * c.t[1] + c.R[6] * c.t[2]);
    C.y = -(c.R[1] * c.t[0] + c.R[4] * c.t[1] + c.R[7] * c.t[2]);
    C.z = -(c.R[2] * c.t[0] + c.R[5] * c.t[1] + c.R[8] * c.t[2]);
    p.x = t.x + C.x;
    p.y = t.y + C.y;
    p.z = t.z + C.z;
    return p;
}

ACMMP_FUSION_HD inline void project(const F3 &X, const acmmp_camera &c, float &px, float &py,
                                    float &depth) {  // ProjectonCamera
    F3 t;
    t.x = c.R[0] * X.x + c.R[1] * X.y + c.R[2] * X.z + c.t[0];
    t.y = c.R[3] * X.x + c.R[4] * X.y + c.R[5] * X.z + c.t[1];
    t.z = c.R[6] * X.x + c.R[7] * X.y + c.R[8] * X.z + c.t[2];
    depth = c.K[6] * t.x + c.K[7] * t.y + c.K[8] * t.z;
    px = (c.K[0] * t.x + c.K[1] * t.y + c.K[2] * t.z) / depth;
    py = (c.K[3] * t.x + c.K[4] * t.y + c.K[5] * t.z) / depth;
}

// RunFusion's threads kept on ONE last-level-cache domain (on a many-CCD
// host a view's candidate lists, written by the pool, and the masks, written
// by the walk, otherwise cross between L3s on every access; the walk, which
// is sequential, measured ~1.4 s or 5-7 s for cfg4 depending on where the
// scheduler happened to put the threads, profiles/r03_fusion_ab.jsonl):
// the calling thread is confined to the physical core it runs on, the
// workers to the rest of that core's L3 domain (within the allowed CPUs).
// Restored when RunFusion returns. ACMMP_FUSION_PIN=0 turns it off.
class CacheDomain {
  public:
    CacheDomain() : threads_(acmmp_host_threads()) {  // the budget before any pinning
        if (const char *e = std::getenv("ACMMP_FUSION_PIN"))
            if (std::atoi(e) == 0) return;
        const int cpu = sched_getcpu();
        if (cpu < 0 || sched_getaffinity(0, sizeof saved_, &saved_)) return;
        cpu_set_t l3 = cpus_of(cpu, "cache/index3/shared_cpu_list"), core = cpus_of(cpu, "topology/thread_siblings_list");
        CPU_AND(&l3, &l3, &saved_);
        CPU_AND(&core, &core, &saved_);
        if (!CPU_ISSET(cpu, &core)) return;
        CPU_XOR(&workers_, &l3, &core);  // l3 without the walk's core
        CPU_AND(&workers_, &workers_, &l3);
        if (CPU_COUNT(&workers_) < 1 || CPU_EQUAL(&l3, &saved_)) return;  // one domain already
        if (sched_setaffinity(0, sizeof core, &core)) return;
        pinned_ = true;
    }
    ~CacheDomain() {
        if (pinned_) (void)sched_setaffinity(0, sizeof saved_, &saved_);
    }
    bool pinned() const { return pinned_; }
    int threads() const { return threads_; }
    // worker threads: confine themselves (0 = no limit)
    int workers() const { return pinned_ ? CPU_COUNT(&workers_) : 0; }
    void confine_worker() const {
        if (pinned_) (void)sched_setaffinity(0, sizeof workers_, &workers_);
    }

  private:
    static cpu_set_t cpus_of(int cpu, const char *what) {
        cpu_set_t set;
        CPU_ZERO(&set);
        char path[160];
        std::snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/%s", cpu, what);
        FILE *f = std::fopen(path, "r");
        if (!f) return set;
        char buf[4096];
        const size_t n = std::fread(buf, 1, sizeof buf - 1, f);
        std::fclose(f);
        buf[n] = 0;
        for (char *p = buf; *p;) {  // "a-b,c,..."
            char *end = nullptr;
            const long a = std::strtol(p, &end, 10);
            if (end == p) break;
            long b = a;
            p = end;
            if (*p == '-') {
                b = std::strtol(p + 1, &end, 10);
                p = end;
            }
            for (long k = a; k <= b && k < CPU_SETSIZE; ++k)
                if (k >= 0) CPU_SET((int)k, &set);
            while (*p == ',' || *p == '\n' || *p == ' ') ++p;
        }
        return set;
    }
    int threads_;
    cpu_set_t saved_{}, workers_{};
    bool pinned_ = false;
};

// A persistent pool of acmmp_host_threads() - 1 workers: `submit` hands out
// indices 0..n-1 of a job to whichever worker is free (dynamic rows), `wait`
// blocks until a job is done. The caller's thread stays free for the
// sequential approval walk, which overlaps the next view's candidate phase.
class Pool {
  public:
    struct Job {
        std::function<void(int)> fn;
        int n = 0;
        std::atomic<int> next{0}, done{0};
    };
    explicit Pool(const CacheDomain *dom = nullptr) {
        int nw = std::max(1, (dom ? dom->threads() : acmmp_host_threads()) - 1);
        if (dom && dom->workers() > 0) nw = std::min(nw, dom->workers());
        for (int t = 0; t < nw; ++t)
            workers_.emplace_back([this, dom] {
                if (dom) dom->confine_worker();
                loop();
            });
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    int size() const { return (int)workers_.size(); }
    std::shared_ptr<Job> submit(int n, std::function<void(int)> fn) {
        auto j = std::make_shared<Job>();
        j->fn = std::move(fn);
        j->n = n;
        {
            std::lock_guard<std::mutex> g(mu_);
            jobs_.push_back(j);
        }
        cv_.notify_all();
        return j;
    }
    void wait(const std::shared_ptr<Job> &j) {
        std::unique_lock<std::mutex> g(mu_);
        done_cv_.wait(g, [&] { return j->done.load() == j->n; });
    }

  private:
    void loop() {
        for (;;) {
            std::shared_ptr<Job> j;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return stop_ || !jobs_.empty(); });
                if (stop_ && jobs_.empty()) return;
                j = jobs_.front();
            }
            int i;
            bool any = false;
            while ((i = j->next.fetch_add(1)) < j->n) {
                j->fn(i);
                any = true;
                if (j->done.fetch_add(1) + 1 == j->n) {
                    std::lock_guard<std::mutex> g(mu_);
                    done_cv_.notify_all();
                }
            }
            if (!any) {  // exhausted: retire it from the queue
                std::lock_guard<std::mutex> g(mu_);
                if (!jobs_.empty() && jobs_.front() == j) jobs_.pop_front();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::deque<std::shared_ptr<Job>> jobs_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    bool stop_ = false;
};

// RunFusion's per-view masks as bitsets: a view's ~20 sources' masks then
// stay cache-resident during the approval walk (1 bit instead of 1 byte a
// pixel). The walk is their only writer; the next view's candidate phase
// reads them meanwhile (any value read is exact, see the top): relaxed
// atomic words.
struct MaskBits {
    std::vector<uint64_t> w;
    void assign(size_t n) { w.assign((n + 63) / 64, 0ull); }
    static bool bit(const uint64_t *w, size_t k) {
        return (__atomic_load_n(&w[k >> 6], __ATOMIC_RELAXED) >> (k & 63)) & 1ull;
    }
    bool get(size_t k) const { return bit(w.data(), k); }
    void set(size_t k) {  // single writer
        const uint64_t v = __atomic_load_n(&w[k >> 6], __ATOMIC_RELAXED) | (1ull << (k & 63));
        __atomic_store_n(&w[k >> 6], v, __ATOMIC_RELAXED);
    }
};

// Runs fn(0..n-1) on the pool's workers (the caller waits); returns the
// status of the lowest failing index with its message (what the sequential
// loop reports first).
template <class Fn>
int pool_for(Pool &pool, int n, Fn fn) {
    std::vector<int> rc((size_t)std::max(n, 0), ACMMP_OK);
    std::vector<std::string> msg(rc.size());
    pool.wait(pool.submit(n, [&](int i) {
        rc[(size_t)i] = fn(i);
        if (rc[(size_t)i]) msg[(size_t)i] = f_err;
    }));
    for (int i = 0; i < n; ++i)
        if (rc[(size_t)i]) {
            f_err = msg[(size_t)i];
            return rc[(size_t)i];
        }
    return ACMMP_OK;
}

// Float bilinear resize of an 8-bit multi-channel image (half-pixel centres,
// edge clamp, round to nearest) — the unpinned stand-in for cv::resize.
inline void resize_u8(const uint8_t *src, int sw, int sh, int C, uint8_t *dst, int dw, int dh) {
    for (int y = 0; y < dh; ++y) {
        float fy = (float)((y + 0.5) * sh / dh - 0.5);
        int y0 = (int)std::floor(fy);
        float ay = fy - y0;
        if (y0 < 0) { y0 = 0; ay = 0; }
        if (y0 >= sh - 1) { y0 = sh - 1; ay = 0; }
        const int y1 = std::min(y0 + 1, sh - 1);
        for (int x = 0; x < dw; ++x) {
            float fx = (float)((x + 0.5) * sw / dw - 0.5);
            int x0 = (int)std::floor(fx);
            float ax = fx - x0;
            if (x0 < 0) { x0 = 0; ax = 0; }
            if (x0 >= sw - 1) { x0 = sw - 1; ax = 0; }
            const int x1 = std::min(x0 + 1, sw - 1);
            for (int k = 0; k < C; ++k) {
                auto at = [&](int yy, int xx) { return (float)src[((size_t)yy * sw + xx) * C + k]; };
                const float top = at(y0, x0) * (1 - ax) + at(y0, x1) * ax;
                const float bot = at(y1, x0) * (1 - ax) + at(y1, x1) * ax;
                const float v = top * (1 - ay) + bot * ay;
                dst[((size_t)y * dw + x) * C + k] = (uint8_t)std::min(255.0f, std::max(0.0f, std::nearbyint(v)));
            }
        }
    }
}

inline void resize_u8(const std::vector<uint8_t> &src, int sw, int sh, int C, std::vector<uint8_t> &dst, int dw, int dh) {
    dst.resize((size_t)dw * dh * C);
    resize_u8(src.data(), sw, sh, C, dst.data(), dw, dh);
}

// A fusion's inputs, per view. The stages read it; walk_view alone writes (mask bits only).
struct Scene {
    const acmmp_problem *problems;
    std::vector<std::vector<uint8_t>> images;  // BGR, at the maps' size
    std::vector<acmmp_camera> cameras;         // ... and so are their intrinsics
    std::vector<std::vector<float>> depths, normals;
    std::vector<int> rows, cols;
    std::vector<MaskBits> masks;              // RunFusion's (the prior-aware fusion keeps bytes)
    std::vector<std::vector<int>> src_index;  // [view][source slot j]: the source's view index
    Scene(const acmmp_problem *p, size_t n)
        : problems(p), images(n), cameras(n), depths(n), normals(n), rows(n), cols(n), masks(n), src_index(n) {}
    size_t pixels() const {  // of all views: a cloud has at most one point per pixel
        size_t total = 0;
        for (size_t i = 0; i < rows.size(); ++i) total += (size_t)cols[i] * rows[i];
        return total;
    }
};

struct FusionInputs : Scene {  // the prior-aware fusions': with the second map pair, this run's priors
    std::vector<std::vector<float>> pdepths, pnormals;
    FusionInputs(const acmmp_problem *p, size_t n) : Scene(p, n), pdepths(n), pnormals(n) {}
};

// depths[_geom].dmb and normals.dmb of view `id` in `folder`: one size, 1 and 3 bands
inline int read_maps(const std::string &folder, const char *suffix, int id, std::vector<float> &depth,
              std::vector<float> &normal, int &h, int &w) {
    int nb = 0, h2 = 0, w2 = 0, nb2 = 0;
    const std::string dpath = folder + suffix, npath = folder + "/normals.dmb";
    if (acmmp_hostio::read_dmb(dpath, depth, h, w, nb)) return ffail(ACMMP_ERR_IO, "cannot read %s", dpath.c_str());
    if (acmmp_hostio::read_dmb(npath, normal, h2, w2, nb2)) return ffail(ACMMP_ERR_IO, "cannot read %s", npath.c_str());
    if (nb != 1 || nb2 != 3 || h2 != h || w2 != w) return ffail(ACMMP_ERR_IO, "bad maps for view %d", id);
    return ACMMP_OK;
}

// View i of a fusion (both fusions; one index per thread): its colour image,
// camera and the maps in `maps_folder`, image and intrinsics brought to the
// maps' size (RescaleImageAndCamera, src/ACMMP.cpp:181-201).
inline int load_view(Scene &sc, size_t i, const std::string &image_folder, const std::string &dense,
              const std::string &maps_folder, const char *suffix) {
    const int id = sc.problems[i].ref_image_id;
    const std::string ipath = image_folder + "/" + id8(id) + ".jpg";
    int iw = 0, ih = 0, h = 0, w = 0;
    std::vector<uint8_t> img;
    int rc = acmmp_internal_read_image_bgr(ipath.c_str(), img, iw, ih);
    if (rc) return ffail(rc, "cannot read image %s", ipath.c_str());
    const std::string cpath = camera_path(dense, id);
    acmmp_camera &cam = sc.cameras[i];
    if (acmmp_read_camera(cpath.c_str(), &cam)) return ffail(ACMMP_ERR_IO, "cannot read %s", cpath.c_str());
    rc = read_maps(maps_folder, suffix, id, sc.depths[i], sc.normals[i], h, w);
    if (rc) return rc;
    sc.rows[i] = h;
    sc.cols[i] = w;
    if (w == iw && h == ih) {
        sc.images[i] = std::move(img);
    } else {
        resize_u8(img, iw, ih, 3, sc.images[i], w, h);
        acmmp_dense::scale_intrinsics(cam, w / static_cast<float>(iw), h / static_cast<float>(ih));
        cam.width = w;
        cam.height = h;
    }
    return ACMMP_OK;
}

// RunFusion's mask folder (:881-905): mask = (resize(mask) < 128) / 255 as bits of `mask` (w x h, all 0)
inline int load_initial_mask(const std::string &mpath, int w, int h, MaskBits &mask) {
    int mw = 0, mh = 0, mc = 0, bd = 0;
    std::vector<uint16_t> m16;
    if (acmmp_hostio::read_png(mpath, m16, mw, mh, mc, bd))
        return ffail(ACMMP_ERR_IO, "Couldn't find mask image %s", mpath.c_str());
    // cv::imread(path, -1) keeps the file's depth and channels (colour as
    // B, G, R[, A], as acmmp_read_png returns them too); `(temp_mask < 128) /
    // 255` keeps the channels, and the walk reads and writes the mask with
    // at<uchar>(r, c): byte c of row r. For a 1-channel mask that is pixel
    // (r, c); for a colour one it is channel c % C of pixel c / C, reproduced
    // here. (2-channel gray+alpha masks use the gray value: unpinned.)
    const bool same = mw == w && mh == h;
    if (bd != 8 && !same) return ffail(ACMMP_ERR_UNSUPPORTED, "16-bit mask %s needs resizing", mpath.c_str());
    const int C = mc == 2 ? 1 : mc;
    std::vector<uint16_t> px((size_t)mw * mh * C);
    for (size_t k = 0; k < (size_t)mw * mh; ++k)
        for (int ch = 0; ch < C; ++ch) px[k * C + ch] = m16[k * mc + ch];
    std::vector<uint16_t> mr;
    if (same) {
        mr.swap(px);
    } else {
        std::vector<uint8_t> m8(px.begin(), px.end()), r8;
        resize_u8(m8, mw, mh, C, r8, w, h);
        mr.assign(r8.begin(), r8.end());
    }
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c)
            if (mr[(size_t)r * w * C + c] < 128) mask.set((size_t)r * w + c);
    return ACMMP_OK;
}

// src_index from the problems' image ids: every source must be a problem itself
inline int resolve_sources(Scene &sc) {
    std::map<int, int> image_id_2_index;
    for (size_t i = 0; i < sc.rows.size(); ++i) image_id_2_index[sc.problems[i].ref_image_id] = (int)i;
    for (size_t i = 0; i < sc.rows.size(); ++i)
        for (int j = 0; j < sc.problems[i].num_src_images; ++j) {
            const auto it = image_id_2_index.find(sc.problems[i].src_image_ids[j]);
            if (it == image_id_2_index.end())
                return ffail(ACMMP_ERR_ARG, "source %d of view %d is not a problem", sc.problems[i].src_image_ids[j],
                             sc.problems[i].ref_image_id);
            sc.src_index[i].push_back(it->second);
        }
    return ACMMP_OK;
}

// what a hit's pixel bits, the kernels' pixel indices and a hit mask's bits hold
inline int check_view_sizes(const Scene &sc) {
    for (size_t i = 0; i < sc.rows.size(); ++i)
        if ((size_t)sc.cols[i] * sc.rows[i] > (size_t(1) << 27) || sc.problems[i].num_src_images > 32)
            return ffail(ACMMP_ERR_ARG, "view %d: fusion supports images up to 2^27 pixels and 32 sources",
                         sc.problems[i].ref_image_id);
    return ACMMP_OK;
}

inline const char *depth_suffix(int geom_consistency) { return geom_consistency ? "/depths_geom.dmb" : "/depths.dmb"; }

// RunFusion's inputs (both orders), from the call's raw arguments: the views load independently on
// the pool (JPEG decode, two .dmb reads from output_folder, the mask if a mask folder is given), then
// the sources
inline int load_fusion_views(Scene &sc, Pool &pool, const char *dense_folder, const char *output_folder,
                             int geom_consistency, const char *image_dir, const char *mask_folder) {
    const std::string dense = dense_folder, out = output_folder;
    const std::string image_folder = dense + (image_dir ? image_dir : "/images");
    const bool use_masks = mask_folder && std::string(mask_folder) != " " && mask_folder[0] != 0;
    const char *suffix = depth_suffix(geom_consistency);
    const int rc = pool_for(pool, (int)sc.rows.size(), [&](int vi) -> int {
        const size_t i = (size_t)vi;
        const int id = sc.problems[i].ref_image_id;
        const int load_rc = load_view(sc, i, image_folder, dense, result_folder(out, id), suffix);
        if (load_rc) return load_rc;
        sc.masks[i].assign((size_t)sc.cols[i] * sc.rows[i]);
        if (!use_masks) return (int)ACMMP_OK;
        return load_initial_mask(dense + "/" + mask_folder + "/" + id8(id) + ".png", sc.cols[i], sc.rows[i],
                                 sc.masks[i]);
    });
    return rc ? rc : resolve_sources(sc);
}

// View i of RunPriorAwareFusion (both orders): load_view with the maps of the other reconstruction
// (fusion_folder), and this run's (output_folder), the priors, as the second pair of the same size.
// The masks are the caller's: mask files give 255/0 here (:654-661), never the 1 the checks test,
// so they start all zero and only approvals mask pixels.
inline int load_prior_view(FusionInputs &in, size_t i, const std::string &dense, const std::string &out,
                           const std::string &fus, const char *suffix) {
    const int id = in.problems[i].ref_image_id;
    int rc = load_view(in, i, dense + "/images", dense, result_folder(fus, id), suffix);
    int h = 0, w = 0;
    if (!rc) rc = read_maps(result_folder(out, id), suffix, id, in.pdepths[i], in.pnormals[i], h, w);
    if (rc) return rc;
    if (h != in.rows[i] || w != in.cols[i]) return ffail(ACMMP_ERR_IO, "map sizes of view %d disagree", id);
    return ACMMP_OK;
}

struct Point {
    F3 coord, normal, color;
};

// StoreColorPlyFileBinaryPointCloud. The 27-byte records (6 floats + r, g, b)
// are formed in chunks of 2^18 points, each written at its own offset: on
// the pool's workers when one is given (RunFusion's pool is idle by then),
// else in order on the caller. Same bytes either way. (ACMMP_PLY_CHUNK_POINTS
// sets the chunk size, so tests reach the chunk boundaries on small clouds.)
constexpr size_t kPlyRec = 6 * sizeof(float) + 3;

inline size_t ply_chunk_points() {
    const char *e = std::getenv("ACMMP_PLY_CHUNK_POINTS");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? (size_t)v : size_t(1) << 18;
}

inline int pwrite_all(int fd, const char *p, size_t n, off_t at) {
    while (n) {
        const ssize_t w = ::pwrite(fd, p, n, at);
        if (w <= 0) return -1;
        p += w, n -= (size_t)w, at += w;
    }
    return 0;
}

// n records, record k formed by fill(k, o) at o: the header, then the chunks
template <class Fill>
int store_ply_records(const std::string &path, size_t n, Pool *pool, Fill fill) {
    char hdr[512];
    const int hl = std::snprintf(hdr, sizeof(hdr),
                                 "ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
                                 "property float x\nproperty float y\nproperty float z\n"
                                 "property float nx\nproperty float ny\nproperty float nz\n"
                                 "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n",
                                 (int)n);
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return ffail(ACMMP_ERR_IO, "cannot write %s", path.c_str());
    const size_t per = ply_chunk_points();
    const int nchunks = (int)((n + per - 1) / per);
    auto chunk = [&](int c) -> int {
        const size_t b = (size_t)c * per, e = std::min(n, b + per);
        std::vector<char> buf((e - b) * kPlyRec);
        char *o = buf.data();
        for (size_t k = b; k < e; ++k, o += kPlyRec) fill(k, o);
        if (pwrite_all(fd, buf.data(), buf.size(), (off_t)(hl + b * kPlyRec)))
            return ffail(ACMMP_ERR_IO, "cannot write %s", path.c_str());
        return ACMMP_OK;
    };
    int rc = pwrite_all(fd, hdr, (size_t)hl, 0) ? ffail(ACMMP_ERR_IO, "cannot write %s", path.c_str()) : ACMMP_OK;
    if (rc == ACMMP_OK && pool) rc = pool_for(*pool, nchunks, chunk);
    for (int c = 0; rc == ACMMP_OK && !pool && c < nchunks; ++c) rc = chunk(c);
    if (::close(fd) != 0 && rc == ACMMP_OK) rc = ffail(ACMMP_ERR_IO, "cannot write %s", path.c_str());
    return rc;
}

// a record's coordinate: one that is not finite is written as 0, 0, 0
inline F3 ply_coord(F3 X) {
    if (!(X.x < FLT_MAX && X.x > -FLT_MAX) || !(X.y < FLT_MAX && X.y > -FLT_MAX) ||
        !(X.z < FLT_MAX && X.z >= -FLT_MAX)) {
        X.x = X.y = X.z = 0.0f;
    }
    return X;
}

inline int store_ply(const std::string &path, const std::vector<Point> &pc, Pool *pool = nullptr) {
    return store_ply_records(path, pc.size(), pool, [&](size_t k, char *o) {
        const Point &p = pc[k];
        const F3 X = ply_coord(p.coord);
        const float v[6] = {X.x, X.y, X.z, p.normal.x, p.normal.y, p.normal.z};
        std::memcpy(o, v, sizeof(v));
        o[24] = (char)(int)p.color.z;  // colour is stored b, g, r; written r, g, b
        o[25] = (char)(int)p.color.y;
        o[26] = (char)(int)p.color.x;
    });
}

// the same file from a cloud held as arrays (acmmp_write_ply_points): n x 3 floats, floats, bytes r, g, b
inline int store_ply_arrays(const std::string &path, const float *xyz, const float *normal, const uint8_t *rgb,
                            size_t n, Pool *pool = nullptr) {
    return store_ply_records(path, n, pool, [&](size_t k, char *o) {
        const F3 X = ply_coord(F3{xyz[k * 3], xyz[k * 3 + 1], xyz[k * 3 + 2]});
        const float v[6] = {X.x, X.y, X.z, normal[k * 3], normal[k * 3 + 1], normal[k * 3 + 2]};
        std::memcpy(o, v, sizeof(v));
        std::memcpy(o + 24, rgb + k * 3, 3);
    });
}

// acmmp_fuse_views_jacobi's arguments, all of them before any device call: ACMMP_OK or ACMMP_ERR_ARG
// with the message. The limits are what the kernels index with: 32 source slots (a hit mask's
// bits), source indices into views[], pixel indices below 2^27.
inline int check_fusion_views(const acmmp_fusion_view *views, int count, const acmmp_cloud_buffers *out,
                              const int64_t *num_points) {
    if (count <= 0) return ffail(ACMMP_ERR_ARG, "count %d: at least one view is needed", count);
    if (!views) return ffail(ACMMP_ERR_ARG, "null views");
    if (!num_points) return ffail(ACMMP_ERR_ARG, "null num_points");
    for (int i = 0; i < count; ++i) {
        const acmmp_fusion_view &v = views[i];
        if (v.num_src < 0 || v.num_src > 32)
            return ffail(ACMMP_ERR_ARG, "view %d: num_src %d outside 0..32", i, v.num_src);
        for (int j = 0; j < v.num_src; ++j)
            if (v.src[j] < 0 || v.src[j] >= count)
                return ffail(ACMMP_ERR_ARG, "view %d: source slot %d is view %d of %d", i, j, v.src[j], count);
        const long long pixels = (long long)v.cam.width * v.cam.height;
        if (v.cam.width <= 0 || v.cam.height <= 0 || pixels > (1ll << 27))
            return ffail(ACMMP_ERR_ARG, "view %d: %d x %d maps, fusion supports 1 to 2^27 pixels", i, v.cam.width,
                         v.cam.height);
        if (!v.d_depth || !v.d_normal) return ffail(ACMMP_ERR_ARG, "view %d: null d_depth or d_normal", i);
        if (v.depth_stride < 1 || v.normal_stride < 3)
            return ffail(ACMMP_ERR_ARG, "view %d: depth_stride %lld (at least 1) or normal_stride %lld (at least 3)", i,
                         (long long)v.depth_stride, (long long)v.normal_stride);
    }
    if (out && (out->capacity < 0 || (out->capacity > 0 && (!out->d_xyz || !out->d_normal || !out->d_rgb))))
        return ffail(ACMMP_ERR_ARG, "cloud buffers: capacity %lld with a null array or below 0",
                     (long long)out->capacity);
    return ACMMP_OK;
}

}  // namespace acmmp_fusion_host

#endif  // ACMMP_FUSION_HOST_H_

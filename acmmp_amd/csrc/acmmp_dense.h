// acmmp_dense.h — what every host driver of a dense folder shares: the
// reference's file layout, its image rescale rule, the per-scale size step,
// one view's .dmb outputs and the index-parallel worker loop. Header-only and
// inline over include/acmmp.h's C-ABI, so the library sources and the tools
// that link against the library (acmmp_main.cpp, acmmp_vp.cpp) use one copy.
#pragma once

#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "../../include/acmmp.h"

namespace acmmp_dense {

// ---- folder layout (src/ACMMP.cpp:536-557, src/acmmp_definitions.cpp:254-258)
inline std::string id8(int id) {
    char b[32];
    std::snprintf(b, sizeof(b), "%08d", id);
    return b;
}

// images/<id>.jpg; .pgm / .pfm are accepted when no .jpg exists
inline std::string image_path(const std::string &dense, int id) {
    const std::string base = dense + "/images/" + id8(id);
    for (const char *ext : {".jpg", ".pgm", ".pfm"}) {
        struct stat st;
        if (::stat((base + ext).c_str(), &st) == 0) return base + ext;
    }
    return base + ".jpg";
}

inline std::string camera_path(const std::string &dense, int id) { return dense + "/cams/" + id8(id) + "_cam.txt"; }

inline std::string result_folder(const std::string &out, int ref_id) { return out + "/2333_" + id8(ref_id); }

// ---- the rescale rule of InputInitialization (src/ACMMP.cpp:578-583) and
// JointBilateralUpsampling (src/acmmp_definitions.cpp:428-433): float factor,
// std::round (halves away from zero).
inline void rescaled_size(int w, int h, int size, int *nw, int *nh) {
    const float factor_x = static_cast<float>(size) / w;
    const float factor_y = static_cast<float>(size) / h;
    const float factor = std::min(factor_x, factor_y);
    *nw = (int)std::round(w * factor);
    *nh = (int)std::round(h * factor);
}

// InputInitialization's use of it: an image with both sides <= max_image_size
// keeps its size (src/ACMMP.cpp:574-576; JointBilateralUpsampling has no such test)
inline void scaled_size(int w, int h, int max_image_size, int *nw, int *nh) {
    *nw = w;
    *nh = h;
    if (w > max_image_size || h > max_image_size) rescaled_size(w, h, max_image_size, nw, nh);
}

// the camera of an image resized by (sx, sy): K rows 0 and 1 (src/ACMMP.cpp:193-196, :590-593)
inline void scale_intrinsics(acmmp_camera &cam, float sx, float sy) {
    cam.K[0] *= sx, cam.K[2] *= sx;
    cam.K[4] *= sy, cam.K[5] *= sy;
}

// cur_image_size of every problem for the next scale (src/main_ACMMP.cpp:99-106)
inline void scale_step(acmmp_problem *problems, int n) {
    for (int i = 0; i < n; ++i)
        if (problems[i].num_downscale >= 0) {
            problems[i].cur_image_size = (int)(problems[i].max_image_size / std::pow(2, problems[i].num_downscale));
            problems[i].num_downscale--;
        }
}

// One view's maps (src/acmmp_definitions.cpp:381-401): H x W float4 planes
// (normal xyz, depth) split into depths[_geom].dmb and normals.dmb, plus
// costs.dmb, in `folder`.
inline int write_view_maps(const std::string &folder, bool geom, int H, int W, const float *planes4,
                           const float *costs) {
    const size_t P = (size_t)W * H;
    std::vector<float> depths(P), normals(P * 3);
    for (size_t i = 0; i < P; ++i) {
        normals[3 * i] = planes4[4 * i];
        normals[3 * i + 1] = planes4[4 * i + 1];
        normals[3 * i + 2] = planes4[4 * i + 2];
        depths[i] = planes4[4 * i + 3];
    }
    if (acmmp_write_dmb((folder + (geom ? "/depths_geom.dmb" : "/depths.dmb")).c_str(), H, W, 1, depths.data()) ||
        acmmp_write_dmb((folder + "/normals.dmb").c_str(), H, W, 3, normals.data()) ||
        acmmp_write_dmb((folder + "/costs.dmb").c_str(), H, W, 1, costs))
        return ACMMP_ERR_IO;
    return ACMMP_OK;
}

// Runs fn(0..n-1) on `workers` threads (clamped to [1, n]; the calling thread
// is one of them). Returns the status of the lowest failing index and leaves
// in `message` what last_message(i) returned on the thread that ran it, so the
// caller sees what the sequential loop would have reported first. With
// stop_on_first_error no index is started after a failure.
template <class Fn, class Msg>
int parallel_index(int n, int workers, Fn fn, Msg last_message, std::string &message,
                   bool stop_on_first_error = false) {
    std::vector<int> rc((size_t)std::max(n, 0), ACMMP_OK);
    std::vector<std::string> msg(rc.size());
    std::atomic<int> next{0};
    std::atomic<bool> failed{false};
    auto work = [&]() {
        for (int i; !(stop_on_first_error && failed.load()) && (i = next.fetch_add(1)) < n;) {
            rc[(size_t)i] = fn(i);
            if (rc[(size_t)i]) {
                msg[(size_t)i] = last_message(i);
                failed = true;
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < std::min(workers, n); ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    for (int i = 0; i < n; ++i)
        if (rc[(size_t)i]) {
            message = msg[(size_t)i];
            return rc[(size_t)i];
        }
    return ACMMP_OK;
}

}  // namespace acmmp_dense

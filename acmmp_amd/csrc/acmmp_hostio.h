// acmmp_hostio.h — host-side helpers shared by the host modules
// (acmmp_image.cpp defines the first two; acmmp_pipeline.cpp and
// acmmp_fusion.cpp use them all). Not part of the C-ABI.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/acmmp.h"

// 8-bit PNG (channels 1 = gray, 3 = RGB), one IDAT, zlib at best speed.
// ACMMP_OK / ACMMP_ERR_ARG / ACMMP_ERR_IO.
int acmmp_internal_write_png(const char *path, int w, int h, int channels, const uint8_t *px);

// acmmp_read_image_bgr in one pass: decodes into `bgr` (W*H*3, BGR) and sets
// the size, without the C-ABI's size-query call (which decodes the file too).
// ACMMP_OK / ACMMP_ERR_IO / ACMMP_ERR_UNSUPPORTED.
int acmmp_internal_read_image_bgr(const char *path, std::vector<uint8_t> &bgr, int &width, int &height);

// k_seed_planes on `stream` of `device` (acmmp_engine.hip), for
// acmmp_seed_planes_device, which has validated every index first.
// ACMMP_OK / ACMMP_ERR_HIP.
extern "C" int acmmp_internal_launch_seed_planes(int device, const uint16_t *d_depth, int dw, int dc,
                                                 const uint16_t *d_normals, int nw, int scale,
                                                 const acmmp_camera *cam, int rows, int cols, float *d_planes4,
                                                 void *stream);

namespace acmmp_hostio {

// The C-ABI's two-call readers (size query, then data) as one call. Status only: each module words its message.
inline int read_dmb(const std::string &path, std::vector<float> &data, int &h, int &w, int &nb) {
    int32_t hh = 0, ww = 0, bb = 0;
    const int rc = acmmp_read_dmb(path.c_str(), &hh, &ww, &bb, nullptr, 0);
    if (rc != ACMMP_OK && rc != ACMMP_ERR_ARG) return ACMMP_ERR_IO;
    data.resize((size_t)hh * ww * bb);
    if (acmmp_read_dmb(path.c_str(), &hh, &ww, &bb, data.data(), data.size())) return ACMMP_ERR_IO;
    h = hh, w = ww, nb = bb;
    return ACMMP_OK;
}

// (the size query of a readable PNG answers ACMMP_ERR_ARG: no buffer)
inline int read_png(const std::string &path, std::vector<uint16_t> &px, int &w, int &h, int &c, int &bit_depth) {
    const int rc = acmmp_read_png(path.c_str(), nullptr, 0, &w, &h, &c, &bit_depth);
    if (rc != ACMMP_ERR_ARG) return rc ? rc : ACMMP_ERR_IO;
    px.resize((size_t)w * h * c);
    return acmmp_read_png(path.c_str(), px.data(), px.size(), &w, &h, &c, &bit_depth);
}

// ---- pSampler's inputs (src/acmmp_definitions.cpp:8-177): the 16-bit depth
// and normal PNGs of a camera under <dense>priors/{depths,normals}/%08d.png
// (the reference concatenates "priors" to dense_folder without a separator).
inline std::string prior_path(const std::string &dense, const char *kind, int cam) {
    char b[32];
    std::snprintf(b, sizeof(b), "%08d", cam);
    return dense + "priors/" + kind + "/" + b + ".png";
}

struct PriorMaps {
    std::vector<uint16_t> depth, normals;  // decoded words: depth dh x dw x dc, normals nh x nw x 3 (B, G, R)
    int dw = 0, dh = 0, dc = 0, nw = 0, nh = 0;
};

// The one loader of a camera's prior maps (GetPriorPlaneEstimate :99-124) for
// the host estimate and the resident drivers. On failure the status and, in
// `message`, what acmmp_prior_plane_estimate reports.
inline int read_prior_maps(const std::string &dense, int cam_num, PriorMaps &m, std::string &message) {
    const std::string dp = prior_path(dense, "depths", cam_num), np = prior_path(dense, "normals", cam_num);
    int nc = 0, bits = 0;
    if (read_png(dp, m.depth, m.dw, m.dh, m.dc, bits) != ACMMP_OK ||
        read_png(np, m.normals, m.nw, m.nh, nc, bits) != ACMMP_OK) {
        message = "failed to load prior images: " + std::to_string(cam_num) + " (" + dp + ")";
        return ACMMP_ERR_IO;
    }
    if (nc != 3) {
        message = "prior normal map " + np + " has " + std::to_string(nc) + " channels";
        return ACMMP_ERR_UNSUPPORTED;
    }
    return ACMMP_OK;
}

}  // namespace acmmp_hostio

// acmmp_hostio.h — host-side helpers shared by the host modules
// (acmmp_image.cpp defines the first two; acmmp_pipeline.cpp and
// acmmp_fusion.cpp use them all). Not part of the C-ABI.
#pragma once

#include <cstdint>
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

}  // namespace acmmp_hostio

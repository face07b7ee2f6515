// Sanitizer driver for the host side of the in-memory fusion (acmmp_fuse_views_jacobi,
// DESIGN.md §8): the argument checks (check_fusion_views, what the entry point runs before any
// device call), acmmp_write_ply_points and acmmp_resize_bilinear_u8. Host code only, built with
// ASan + UBSan by Makefile.fuse_views and run by tests/test_asan_fuse_views.py.
//   fuse_views_driver <folder to write PLY files in>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../acmmp_amd/csrc/acmmp_fusion_host.h"

using acmmp_fusion_host::check_fusion_views;

static int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);    \
            ++fails;                                                   \
        }                                                              \
    } while (0)

static std::vector<acmmp_fusion_view> valid_views(int n) {
    static float somewhere[4];
    std::vector<acmmp_fusion_view> v((size_t)n);
    for (int i = 0; i < n; ++i) {
        v[i] = acmmp_fusion_view{};
        v[i].cam.width = 40, v[i].cam.height = 30;
        v[i].num_src = n - 1;
        for (int j = 0, s = 0; s < n; ++s)
            if (s != i) v[i].src[j++] = s;
        v[i].d_depth = v[i].d_normal = somewhere;  // never read on the host
        v[i].depth_stride = 1, v[i].normal_stride = 3;
    }
    return v;
}

static void checks() {
    int64_t n = 0;
    auto v = valid_views(3);
    EXPECT(check_fusion_views(v.data(), 3, nullptr, &n) == ACMMP_OK);
    EXPECT(check_fusion_views(v.data(), 0, nullptr, &n) == ACMMP_ERR_ARG);
    EXPECT(check_fusion_views(nullptr, 3, nullptr, &n) == ACMMP_ERR_ARG);
    EXPECT(check_fusion_views(v.data(), 3, nullptr, nullptr) == ACMMP_ERR_ARG);
    auto bad = [&](auto change) {
        auto w = valid_views(3);
        change(w);
        const int rc = check_fusion_views(w.data(), 3, nullptr, &n);
        return rc == ACMMP_ERR_ARG && acmmp_fusion_last_error()[0] != 0;
    };
    EXPECT(bad([](auto &w) { w[1].num_src = -1; }));
    EXPECT(bad([](auto &w) { w[1].num_src = 33; }));  // (its sources are not read: src has 32 entries)
    EXPECT(bad([](auto &w) { w[2].src[1] = 3; }));
    EXPECT(bad([](auto &w) { w[0].src[0] = std::numeric_limits<int32_t>::min(); }));
    EXPECT(bad([](auto &w) { w[1].cam.width = 0; }));
    EXPECT(bad([](auto &w) { w[1].cam.width = w[1].cam.height = std::numeric_limits<int32_t>::max(); }));
    EXPECT(bad([](auto &w) { w[1].cam.width = (1 << 27) / 30 + 1; }));
    EXPECT(bad([](auto &w) { w[1].d_depth = nullptr; }));
    EXPECT(bad([](auto &w) { w[1].d_normal = nullptr; }));
    EXPECT(bad([](auto &w) { w[1].depth_stride = 0; }));
    EXPECT(bad([](auto &w) { w[1].normal_stride = std::numeric_limits<int64_t>::min(); }));
    v[0].num_src = 32;
    for (int j = 0; j < 32; ++j) v[0].src[j] = j % 3;
    v[1].cam.width = 1 << 14, v[1].cam.height = 1 << 13;
    acmmp_cloud_buffers out{};
    EXPECT(check_fusion_views(v.data(), 3, &out, &n) == ACMMP_OK);
    out.capacity = 4;
    EXPECT(check_fusion_views(v.data(), 3, &out, &n) == ACMMP_ERR_ARG);
    out.capacity = -1;
    EXPECT(check_fusion_views(v.data(), 3, &out, &n) == ACMMP_ERR_ARG);
}

static void ply(const std::string &folder) {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> u(-100.0f, 100.0f);
    const float odd[] = {INFINITY, -INFINITY, NAN, std::numeric_limits<float>::max(), -std::numeric_limits<float>::max()};
    for (const char *chunk : {"", "1", "7", "1000000"}) {
        ::setenv("ACMMP_PLY_CHUNK_POINTS", chunk, 1);
        for (int n : {0, 1, 6, 7, 8, 1001}) {
            std::vector<float> xyz((size_t)n * 3), nrm((size_t)n * 3);
            std::vector<uint8_t> rgb((size_t)n * 3);
            for (auto &x : xyz) x = u(rng);
            for (auto &x : nrm) x = u(rng);
            for (auto &x : rgb) x = (uint8_t)rng();
            for (int k = 0; k < n; k += 3) xyz[(size_t)k * 3 + k % 3] = odd[k % 5];
            const std::string path = folder + "/cloud.ply";
            EXPECT(acmmp_write_ply_points(path.c_str(), xyz.data(), nrm.data(), rgb.data(), n) == ACMMP_OK);
            FILE *f = std::fopen(path.c_str(), "rb");
            EXPECT(f != nullptr);
            if (!f) continue;
            std::fseek(f, 0, SEEK_END);
            const long size = std::ftell(f);
            std::fclose(f);
            char hdr[512];
            const int hl = std::snprintf(hdr, sizeof hdr, "%d", n);
            EXPECT(size == (long)(228 + hl + (long)n * 27));  // the header's text without the count: 228 bytes
        }
    }
    EXPECT(acmmp_write_ply_points(nullptr, nullptr, nullptr, nullptr, 0) == ACMMP_ERR_ARG);
    EXPECT(acmmp_write_ply_points((folder + "/x.ply").c_str(), nullptr, nullptr, nullptr, 2) == ACMMP_ERR_ARG);
    EXPECT(acmmp_write_ply_points((folder + "/x.ply").c_str(), nullptr, nullptr, nullptr, -2) == ACMMP_ERR_ARG);
    EXPECT(acmmp_write_ply_points((folder + "/none/x.ply").c_str(), nullptr, nullptr, nullptr, 0) == ACMMP_ERR_IO);
}

static void resize() {
    std::mt19937 rng(5);
    const int sizes[][2] = {{1, 1}, {2, 1}, {1, 3}, {131, 67}, {100, 50}, {140, 70}, {7, 300}};
    for (const auto &s : sizes)
        for (const auto &d : sizes)
            for (int c = 1; c <= 4; ++c) {
                std::vector<uint8_t> src((size_t)s[0] * s[1] * c), dst((size_t)d[0] * d[1] * c);
                for (auto &x : src) x = (uint8_t)rng();
                EXPECT(acmmp_resize_bilinear_u8(src.data(), s[0], s[1], c, dst.data(), d[0], d[1]) == ACMMP_OK);
                if (s[0] == d[0] && s[1] == d[1]) EXPECT(src == dst);
            }
    uint8_t px[4] = {1, 2, 3, 4};
    EXPECT(acmmp_resize_bilinear_u8(px, 1, 1, 0, px, 1, 1) == ACMMP_ERR_ARG);
    EXPECT(acmmp_resize_bilinear_u8(px, 1, 1, 5, px, 1, 1) == ACMMP_ERR_ARG);
    EXPECT(acmmp_resize_bilinear_u8(px, 0, 1, 1, px, 1, 1) == ACMMP_ERR_ARG);
    EXPECT(acmmp_resize_bilinear_u8(nullptr, 1, 1, 1, px, 1, 1) == ACMMP_ERR_ARG);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <folder>\n", argv[0]);
        return 2;
    }
    checks();
    ply(argv[1]);
    resize();
    if (fails) return 1;
    std::puts("fuse_views host ok");
    return 0;
}

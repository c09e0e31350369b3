// include/spt_bake.h on the host (spt_host_bake_rays) and the lightmap rasteriser (spt_host_lightmap_points), compiled into this
// stand-alone program from csrc/host/bake.cpp under AddressSanitizer + UBSan, over scene files the loader of libspt_host.so reads.
// Every output array has exactly the documented size, so a write past it is a report.  `make bake-check` builds it;
// tests/test_bake_host.py runs it.  usage: bake_check scene.json [instance names ...] [scene.json ...]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/spt_bake.h"
#include "../include/spt_host.h"

namespace {

int g_failures = 0;

#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (++g_failures <= 20) {                        \
                std::printf("CHECK failed: %s: ", #cond);    \
                std::printf(__VA_ARGS__);                    \
                std::printf("\n");                           \
            }                                                \
        }                                                    \
    } while (0)

uint32_t g_state = 12345u;
float rnd() {   // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * 5.9604644775390625e-8f;
}

void check_rays(const spt_scene_desc* d, const std::vector<spt_bake_point>& pts, uint32_t flags) {
    const uint32_t S = 5;
    const size_t n = pts.size(), nl = d->n_lights;
    std::vector<spt_path_ray> rays(n * S);
    std::vector<float> pos(3 * n), nrm(3 * n), li(3 * n * nl);
    std::vector<spt_ray> shadow(n * nl);
    CHECK(spt_host_bake_rays(d, SPT_BAKE_POINTS_SURFACE, flags, n, pts.data(), S, 99, 0xfffffffeu, 7, rays.data(), pos.data(), nrm.data(), shadow.data(),
                             li.data()) == SPT_OK,
          "%s", spt_host_last_error());
    for (size_t i = 0; i < n; ++i) {
        const float* N = &nrm[3 * i];
        for (uint32_t k = 0; k < S; ++k) {
            const spt_path_ray& r = rays[i * S + k];
            const double len = std::sqrt((double)r.d[0] * r.d[0] + (double)r.d[1] * r.d[1] + (double)r.d[2] * r.d[2]);
            CHECK(std::fabs(len - 1.0) < 1e-6, "point %zu sample %u: |d| = %.9g", i, k, len);
            CHECK(r.d[0] * N[0] + r.d[1] * N[1] + r.d[2] * N[2] > 0.0f, "point %zu sample %u leaves into the surface", i, k);
            CHECK(r.stream_a == 0xfffffffeu + (uint32_t)i && r.stream_b == 7 + k && r.t_min > 0.0f, "point %zu sample %u: streams", i, k);
            CHECK(std::memcmp(r.o, &pos[3 * i], 12) == 0, "point %zu: origin", i);
        }
        for (size_t l = 0; l < nl; ++l) {
            const float* c = &li[3 * (i * nl + l)];
            const spt_ray& s = shadow[i * nl + l];
            const bool lit = c[0] != 0.0f || c[1] != 0.0f || c[2] != 0.0f;
            CHECK(lit == (s.t_max != 0.0f), "point %zu light %zu: li and shadow ray disagree", i, l);
            CHECK(!lit || d->lights[l].type <= SPT_LIGHT_SPOT, "point %zu light %zu: not a delta light", i, l);
        }
    }
    // every output is optional
    CHECK(spt_host_bake_rays(d, SPT_BAKE_POINTS_SURFACE, flags, n, pts.data(), S, 99, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SPT_OK, "null outputs");
    // a refusal writes nothing
    std::vector<spt_bake_point> bad(pts);
    bad.back().instance = d->n_instances;
    std::vector<float> sentinel(3 * n, -7.0f);
    CHECK(spt_host_bake_rays(d, SPT_BAKE_POINTS_SURFACE, flags, n, bad.data(), S, 99, 0, 0, nullptr, sentinel.data(), nullptr, nullptr, nullptr) == SPT_ERR_INVALID_ARG,
          "instance == n_instances was accepted");
    for (float v : sentinel) CHECK(v == -7.0f, "a refused call wrote");
    bad = pts;
    bad[0].v = std::nanf("");
    CHECK(spt_host_bake_rays(d, SPT_BAKE_POINTS_SURFACE, flags, n, bad.data(), S, 99, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SPT_ERR_INVALID_ARG, "NaN v was accepted");
    // WORLD points: the resolved points fed back give the same rays
    std::vector<spt_bake_world_point> wp(n);
    for (size_t i = 0; i < n; ++i) {
        std::memset(&wp[i], 0, sizeof wp[i]);
        std::memcpy(wp[i].p, &pos[3 * i], 12);
        std::memcpy(wp[i].n, &nrm[3 * i], 12);
    }
    std::vector<spt_path_ray> rays2(n * S);
    CHECK(spt_host_bake_rays(d, SPT_BAKE_POINTS_WORLD, 0, n, wp.data(), S, 99, 0xfffffffeu, 7, rays2.data(), nullptr, nullptr, nullptr, nullptr) == SPT_OK, "%s",
          spt_host_last_error());
    CHECK(std::memcmp(rays.data(), rays2.data(), rays.size() * sizeof(spt_path_ray)) == 0, "WORLD points made from resolved SURFACE points give other rays");
}

void check_lightmap(const spt_host_scene* hs, const spt_scene_desc* d, const char* name) {
    const uint32_t sizes[][2] = {{17, 9}, {1, 1}, {64, 3}};
    for (const auto& wh : sizes) {
        uint64_t n = 0, n2 = 0;
        CHECK(spt_host_lightmap_points(hs, name, wh[0], wh[1], nullptr, nullptr, 0, &n) == SPT_OK, "%s", spt_host_last_error());
        CHECK(n <= (uint64_t)wh[0] * wh[1], "%s: more points than texels", name);
        std::vector<spt_bake_point> pts(n);
        std::vector<uint32_t> texels(n);
        CHECK(spt_host_lightmap_points(hs, name, wh[0], wh[1], pts.data(), texels.data(), n, &n2) == SPT_OK && n2 == n, "%s: second call", name);
        for (uint64_t i = 0; i < n; ++i) {
            CHECK(spt_bake_point_ok(&pts[i], d->n_instances, &d->instances[0].prim_type, 48u, d->n_meshes, d->meshes), "%s: texel %u is not a valid point", name, texels[i]);
            CHECK(i == 0 || texels[i] > texels[i - 1], "%s: texels out of order", name);
            CHECK(texels[i] < wh[0] * wh[1], "%s: texel index", name);
        }
        if (n > 1) {   // a short capacity
            std::vector<spt_bake_point> few(n / 2);
            std::vector<uint32_t> idx(n / 2);
            CHECK(spt_host_lightmap_points(hs, name, wh[0], wh[1], few.data(), idx.data(), n / 2, &n2) == SPT_OK && n2 == n, "%s: short capacity", name);
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    spt_host_scene* hs = nullptr;
    const spt_scene_desc* d = nullptr;
    int scenes = 0;
    for (int a = 1; a < argc; ++a) {
        const std::string arg = argv[a];
        if (arg.size() > 5 && arg.compare(arg.size() - 5, 5, ".json") == 0) {
            if (hs) spt_host_scene_free(hs);
            hs = nullptr;
            if (spt_host_load_scene(argv[a], &hs) != SPT_OK) { std::printf("cannot load %s: %s\n", argv[a], spt_host_last_error()); return 2; }
            d = spt_host_scene_desc(hs);
            ++scenes;
            std::vector<spt_bake_point> pts;
            for (uint32_t i = 0; i < d->n_instances; ++i) {
                if (d->instances[i].prim_type != SPT_PRIM_MESH) continue;
                const spt_mesh& m = d->meshes[d->instances[i].prim_id];
                for (int k = 0; k < 40; ++k) {
                    float v = rnd(), w = rnd();
                    if (v + w > 1.0f) { v = 1.0f - v; w = 1.0f - w; }
                    if (k == 0) { v = 0.0f; w = 0.0f; }
                    if (k == 1) { v = 1.0f; w = 0.0f; }
                    if (k == 2) { v = 0.0f; w = 1.0f; }
                    pts.push_back(spt_bake_point{i, m.tri_first + (uint32_t)(rnd() * (float)m.tri_count) % m.tri_count, v, w});
                }
            }
            CHECK(!pts.empty(), "%s has no mesh instance", argv[a]);
            if (!pts.empty()) {
                check_rays(d, pts, 0);
                check_rays(d, pts, SPT_BAKE_FLIP);
            }
        } else if (hs) {
            check_lightmap(hs, d, argv[a]);
        }
    }
    if (hs) spt_host_scene_free(hs);
    if (g_failures || scenes == 0) { std::printf("bake_check FAILED: %d checks, %d scenes\n", g_failures, scenes); return 1; }
    std::printf("bake_check ok: %d scenes\n", scenes);
    return 0;
}

// include/spt_probe.h and the host entry points of csrc/host/probe.cpp over degenerate inputs, as a stand-alone host program under
// AddressSanitizer + UBSan (`make probe-check`; tests/test_probe_host.py runs it).  Prints "probe_check ok" when every check held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "spt_host.h"
#include "spt_probe.h"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "probe_check: %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_bad; } } while (0)

static bool unit(const float* d) {
    const double len = std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
    return std::isfinite(len) && std::fabs(len - 1.0) < 1e-6;
}

int main() {
    // 1. the sphere map at the ends of the draws' range: rx = 0 (the north pole, r = 0), rx = 1 - ulp (the south pole, where
    //    1 - z*z may round below 0 without the max), ry at both ends
    const float one_less = std::nextafter(1.0f, 0.0f);
    const float ends[] = {0.0f, std::numeric_limits<float>::min(), 0.25f, 0.5f, 0.75f, one_less};
    for (float rx : ends)
        for (float ry : ends) {
            float d[3];
            spt_probe_map(rx, ry, d);
            CHECK(unit(d));
            float Y[SPT_PROBE_COEFFS];
            spt_probe_basis(d, Y);
            for (uint32_t j = 0; j < SPT_PROBE_COEFFS; ++j) CHECK(std::isfinite(Y[j]) && Y[j] == spt_probe_basis_j(d, j));
        }
    {
        float d[3];
        spt_probe_map(0.0f, 0.0f, d);
        CHECK(d[0] == 0.0f && d[1] == 0.0f && d[2] == 1.0f);
        spt_probe_map(one_less, 0.0f, d);
        CHECK(d[2] < -0.999999f);
    }
    // 2. streams at the ends of their ranges
    for (uint32_t a : {0u, 1u, 0xffffffffu})
        for (uint32_t b : {0u, 0xffffffffu}) {
            float d[3];
            spt_probe_sample(0xffffffffffffffffull, a, b, d);
            CHECK(unit(d));
        }
    // 3. the predicate and the host entry points: non-finite points are refused and nothing is written
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<spt_probe_point> pts(5);
    for (size_t i = 0; i < pts.size(); ++i) { pts[i].p[0] = (float)i; pts[i].p[1] = -1.0f; pts[i].p[2] = 0.5f; pts[i].pad = nan; }   // (pad is not read)
    for (const auto& pt : pts) CHECK(spt_probe_ok(&pt));
    const uint32_t S = 3;
    std::vector<spt_path_ray> rays(pts.size() * S);
    std::vector<float> weights(pts.size() * S * 9);
    // zero lights: null light pointers and null delta outputs
    CHECK(spt_host_probe_rays(0, nullptr, pts.size(), pts.data(), S, 7, 0xfffffffeu, 0xffffffffu, rays.data(), weights.data(), nullptr, nullptr, nullptr) == SPT_OK);
    for (size_t i = 0; i < pts.size(); ++i)
        for (uint32_t k = 0; k < S; ++k) {
            const spt_path_ray& r = rays[i * S + k];
            CHECK(unit(r.d) && r.t_min == SPT_BAKE_T_EPS && r.o[0] == pts[i].p[0]);
            CHECK(r.stream_a == 0xfffffffeu + (uint32_t)i && r.stream_b == 0xffffffffu + k);   // (u32 wrap)
            float Y[9];
            spt_probe_basis(r.d, Y);
            CHECK(std::memcmp(Y, &weights[(i * S + k) * 9], sizeof Y) == 0);
        }
    CHECK(spt_host_probe_rays(0, nullptr, 0, nullptr, S, 7, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SPT_OK);
    CHECK(spt_host_probe_rays(0, nullptr, pts.size(), pts.data(), 0, 7, 0, 0, rays.data(), weights.data(), nullptr, nullptr, nullptr) == SPT_OK);   // no samples
    for (float bad : {inf, -inf, nan}) {
        std::vector<spt_probe_point> q = pts;
        q[3].p[1] = bad;
        CHECK(!spt_probe_ok(&q[3]));
        std::vector<spt_path_ray> untouched(q.size() * S);
        std::memset(untouched.data(), 0x5a, untouched.size() * sizeof(spt_path_ray));
        CHECK(spt_host_probe_rays(0, nullptr, q.size(), q.data(), S, 7, 0, 0, untouched.data(), nullptr, nullptr, nullptr, nullptr) == SPT_ERR_INVALID_ARG);
        CHECK(std::strstr(spt_host_last_error(), "point 3 ") != nullptr);
        const unsigned char* bytes = reinterpret_cast<const unsigned char*>(untouched.data());
        bool same = true;
        for (size_t b = 0; b < untouched.size() * sizeof(spt_path_ray); ++b) same = same && bytes[b] == 0x5a;
        CHECK(same);
    }
    // 4. delta lights: every type, a black light, a light of an area type, a point light on the probe itself
    std::vector<spt_light> lights(6);
    std::memset(lights.data(), 0, lights.size() * sizeof(spt_light));
    lights[0].type = SPT_LIGHT_DIRECTIONAL; lights[0].dir[1] = -1.0f; lights[0].strength[0] = 2.0f;
    lights[1].type = SPT_LIGHT_POINT; lights[1].pos[1] = 4.0f; lights[1].strength[1] = 8.0f;
    lights[2].type = SPT_LIGHT_SPOT; lights[2].pos[1] = 4.0f; lights[2].dir[1] = -1.0f; lights[2].cos_inner = 0.9f; lights[2].cos_outer = 0.9f; lights[2].strength[2] = 1.0f;
    lights[3].type = SPT_LIGHT_POINT;                     // black: skipped
    lights[4].type = 0x7fffffffu;                         // not a delta type: skipped
    lights[5].type = SPT_LIGHT_POINT; lights[5].pos[0] = pts[1].p[0]; lights[5].pos[1] = pts[1].p[1]; lights[5].pos[2] = pts[1].p[2]; lights[5].strength[0] = 1.0f;
    const uint32_t nl = (uint32_t)lights.size();
    std::vector<spt_ray> drays(pts.size() * nl);
    std::vector<float> dli(pts.size() * nl * 3), dy(pts.size() * nl * 9);
    CHECK(spt_host_probe_rays(nl, lights.data(), pts.size(), pts.data(), S, 7, 0, 0, nullptr, nullptr, drays.data(), dli.data(), dy.data()) == SPT_OK);
    for (size_t i = 0; i < pts.size(); ++i) {
        CHECK(dli[(i * nl + 0) * 3] == 2.0f && drays[i * nl].d[1] == 1.0f && drays[i * nl].t_max == SPT_F32_MAX);
        CHECK(dli[(i * nl + 1) * 3 + 1] > 0.0f && unit(drays[i * nl + 1].d));
        CHECK(dli[(i * nl + 3) * 3] == 0.0f && drays[i * nl + 3].t_max == 0.0f && dy[(i * nl + 3) * 9] == 0.0f);
        CHECK(dli[(i * nl + 4) * 3] == 0.0f && drays[i * nl + 4].t_max == 0.0f);
    }
    CHECK(spt_host_probe_rays(nl, nullptr, pts.size(), pts.data(), S, 7, 0, 0, nullptr, nullptr, drays.data(), nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    // 5. the basis entry point
    const float dirs[6] = {0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};   // a unit vector and the zero vector (used as given)
    float out[18];
    CHECK(spt_host_probe_basis(2, dirs, out) == SPT_OK);
    CHECK(out[0] == 0.282094792f && out[2] == 0.488602512f && out[9] == 0.282094792f && out[9 + 6] == -0.315391565f);
    CHECK(spt_host_probe_basis(0, nullptr, nullptr) == SPT_OK);
    CHECK(spt_host_probe_basis(1, nullptr, out) == SPT_ERR_INVALID_ARG);
    CHECK(spt_probe_weight(1) == 4.0f * SPT_PI);
    if (g_bad) return 1;
    std::printf("probe_check ok\n");
    return 0;
}

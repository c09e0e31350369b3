// spt_host_probe_rays and spt_host_probe_basis (include/spt_host.h): include/spt_probe.h evaluated on the host.
#include <cstring>
#include <string>

#include "../../../include/spt_probe.h"
#include "../../../include/spt_host.h"

namespace spt_host {
void set_error(const std::string& m);
}
using spt_host::set_error;

extern "C" {

spt_status spt_host_probe_rays(uint32_t n_lights, const spt_light* lights, uint64_t n_points, const spt_probe_point* points, uint32_t samples, uint64_t seed,
                               uint32_t first_point, uint32_t first_sample, spt_path_ray* rays_out, float* weights_out, spt_ray* delta_rays_out,
                               float* delta_li_out, float* delta_basis_out) {
    if ((n_points != 0 && !points) || (n_lights != 0 && !lights)) { set_error("probe_rays: null argument"); return SPT_ERR_INVALID_ARG; }
    for (uint64_t i = 0; i < n_points; ++i)   // the whole list first: a refusal writes nothing
        if (!spt_probe_ok(points + i)) {
            set_error("probe_rays: point " + std::to_string(i) + " has a non-finite p");
            return SPT_ERR_INVALID_ARG;
        }
    const bool want_delta = delta_rays_out || delta_li_out || delta_basis_out;
    for (uint64_t i = 0; i < n_points; ++i) {
        const float* const p = points[i].p;
        for (uint32_t l = 0; l < n_lights && want_delta; ++l) {
            float dir[3] = {0.0f, 0.0f, 0.0f}, li[3] = {0.0f, 0.0f, 0.0f}, t_max = 0.0f;
            const bool want = spt_probe_delta(lights + l, p, dir, li, &t_max);
            const size_t at = (size_t)i * n_lights + l;
            if (delta_rays_out) {
                spt_ray& r = delta_rays_out[at];
                std::memset(&r, 0, sizeof r);
                if (want) {
                    for (int c = 0; c < 3; ++c) { r.o[c] = p[c]; r.d[c] = dir[c]; }
                    r.t_min = SPT_BAKE_T_EPS;
                    r.t_max = t_max;
                }
            }
            if (delta_li_out)
                for (int c = 0; c < 3; ++c) delta_li_out[3 * at + c] = want ? li[c] : 0.0f;
            if (delta_basis_out) {
                float Y[SPT_PROBE_COEFFS];
                spt_probe_basis(dir, Y);
                for (uint32_t j = 0; j < SPT_PROBE_COEFFS; ++j) delta_basis_out[SPT_PROBE_COEFFS * at + j] = want ? Y[j] : 0.0f;
            }
        }
        if (!rays_out && !weights_out) continue;
        const uint32_t a = first_point + (uint32_t)i;   // (u32 wrap)
        for (uint32_t k = 0; k < samples; ++k) {
            const size_t at = (size_t)i * samples + k;
            float d[3];
            spt_probe_sample(seed, a, first_sample + k, d);
            if (rays_out) {
                spt_path_ray& r = rays_out[at];
                std::memset(&r, 0, sizeof r);
                for (int c = 0; c < 3; ++c) { r.o[c] = p[c]; r.d[c] = d[c]; }
                r.t_min = SPT_BAKE_T_EPS;
                r.stream_a = a;
                r.stream_b = first_sample + k;
            }
            if (weights_out) spt_probe_basis(d, weights_out + SPT_PROBE_COEFFS * at);
        }
    }
    return SPT_OK;
}

spt_status spt_host_probe_basis(uint64_t n, const float* dirs, float* out) {
    if (n != 0 && (!dirs || !out)) { set_error("probe_basis: null argument"); return SPT_ERR_INVALID_ARG; }
    for (uint64_t i = 0; i < n; ++i) spt_probe_basis(dirs + 3 * i, out + SPT_PROBE_COEFFS * i);
    return SPT_OK;
}

}  // extern "C"

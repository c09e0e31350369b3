// spt_host_bake_rays and spt_host_lightmap_points (include/spt_host.h): include/spt_bake.h evaluated on the host, and the
// texel-centre rasteriser that names lightmap texels as bake points.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/spt_bake.h"
#include "../../../include/spt_host.h"

namespace spt_host {
void set_error(const std::string& m);
}
using spt_host::set_error;

extern "C" {

spt_status spt_host_bake_rays(const spt_scene_desc* desc, uint32_t kind, uint32_t flags, uint64_t n_points, const void* points, uint32_t samples,
                              uint64_t seed, uint32_t first_point, uint32_t first_sample, spt_path_ray* rays_out, float* pos_out, float* nrm_out,
                              spt_ray* delta_rays_out, float* delta_li_out) {
    if (!desc || (n_points != 0 && !points)) { set_error("bake_rays: null argument"); return SPT_ERR_INVALID_ARG; }
    if (kind > SPT_BAKE_POINTS_WORLD) { set_error("bake_rays: unknown kind of points"); return SPT_ERR_INVALID_ARG; }
    if (flags & ~(uint32_t)SPT_BAKE_FLIP) { set_error("bake_rays: unknown flags"); return SPT_ERR_INVALID_ARG; }
    const bool world = kind == SPT_BAKE_POINTS_WORLD;
    const uint32_t stride = (uint32_t)(sizeof(spt_instance) / sizeof(uint32_t));
    for (uint64_t i = 0; i < n_points; ++i) {   // the whole list first: a refusal writes nothing
        const bool ok = world ? spt_bake_world_ok(static_cast<const spt_bake_world_point*>(points) + i)
                              : spt_bake_point_ok(static_cast<const spt_bake_point*>(points) + i, desc->n_instances,
                                                  desc->n_instances ? &desc->instances[0].prim_type : nullptr, stride, desc->n_meshes, desc->meshes);
        if (!ok) {
            set_error("bake_rays: point " + std::to_string(i) +
                      (world ? " has a non-finite p or n or an all-zero n" : " does not name a triangle of a mesh instance (instance, prim) or has a non-finite v or w"));
            return SPT_ERR_INVALID_ARG;
        }
    }
    for (uint64_t i = 0; i < n_points; ++i) {
        float p[3], n[3];
        if (world) {
            const spt_bake_world_point& wp = static_cast<const spt_bake_world_point*>(points)[i];
            for (int c = 0; c < 3; ++c) { p[c] = wp.p[c]; n[c] = wp.n[c]; }
        } else {
            const spt_bake_point& pt = static_cast<const spt_bake_point*>(points)[i];
            spt_bake_resolve(&pt, desc->instances + pt.instance, desc->tri_pos + pt.prim, desc->tri_attr + pt.prim, p, n);
        }
        if (flags & SPT_BAKE_FLIP) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        if (pos_out) std::memcpy(pos_out + 3 * i, p, sizeof p);
        if (nrm_out) std::memcpy(nrm_out + 3 * i, n, sizeof n);
        for (uint32_t l = 0; l < desc->n_lights && (delta_rays_out || delta_li_out); ++l) {
            float dir[3], li[3], t_min, t_max;
            const bool want = spt_bake_delta(desc->lights + l, p, n, dir, li, &t_min, &t_max);
            const size_t at = (size_t)i * desc->n_lights + l;
            if (delta_rays_out) {
                spt_ray& r = delta_rays_out[at];
                std::memset(&r, 0, sizeof r);
                if (want) {
                    for (int c = 0; c < 3; ++c) { r.o[c] = p[c]; r.d[c] = dir[c]; }
                    r.t_min = t_min;
                    r.t_max = t_max;
                }
            }
            if (delta_li_out)
                for (int c = 0; c < 3; ++c) delta_li_out[3 * at + c] = want ? li[c] : 0.0f;
        }
        if (!rays_out) continue;
        float tg[3], bt[3];
        spt_bake_frame(n, tg, bt);
        const uint32_t a = first_point + (uint32_t)i;   // (u32 wrap)
        for (uint32_t k = 0; k < samples; ++k) {
            spt_path_ray& r = rays_out[(size_t)i * samples + k];
            std::memset(&r, 0, sizeof r);
            spt_bake_sample(seed, a, first_sample + k, n, tg, bt, r.d, &r.t_min);
            for (int c = 0; c < 3; ++c) r.o[c] = p[c];
            r.stream_a = a;
            r.stream_b = first_sample + k;
        }
    }
    return SPT_OK;
}

spt_status spt_host_lightmap_points(const spt_host_scene* scene, const char* instance_name, uint32_t width, uint32_t height, spt_bake_point* points_out,
                                    uint32_t* texels_out, uint64_t capacity, uint64_t* n_out) {
    if (!scene || !instance_name || !n_out) { set_error("lightmap_points: null argument"); return SPT_ERR_INVALID_ARG; }
    if (width == 0 || height == 0 || (uint64_t)width * height > 0xffffffffull) { set_error("lightmap_points: bad size"); return SPT_ERR_INVALID_ARG; }
    if (capacity != 0 && (!points_out || !texels_out)) { set_error("lightmap_points: null output with a capacity"); return SPT_ERR_INVALID_ARG; }
    uint32_t inst = 0;
    if (const spt_status e = spt_host_scene_instance_index(scene, instance_name, &inst)) return e;
    const spt_scene_desc* d = spt_host_scene_desc(scene);
    if (!d || inst >= d->n_instances || d->instances[inst].prim_type != SPT_PRIM_MESH || d->instances[inst].prim_id >= d->n_meshes) {
        set_error(std::string("lightmap_points: '") + instance_name + "' is not a triangle-mesh instance");
        return SPT_ERR_INVALID_ARG;
    }
    const spt_mesh& m = d->meshes[d->instances[inst].prim_id];
    const size_t n_texels = (size_t)width * height;
    const uint32_t none = 0xffffffffu;
    std::vector<uint32_t> owner(n_texels, none);
    std::vector<float> vw(2 * n_texels, 0.0f);
    const double W = (double)width, H = (double)height;
    for (uint32_t t = 0; t < m.tri_count; ++t) {   // triangle order: the lowest index keeps a texel
        const spt_tri_attr& a = d->tri_attr[m.tri_first + t];
        const double x0 = a.uv[0][0], y0 = a.uv[0][1], x1 = a.uv[1][0], y1 = a.uv[1][1], x2 = a.uv[2][0], y2 = a.uv[2][1];
        const double area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
        if (!(area != 0.0) || !std::isfinite(area)) continue;   // zero-area (or non-finite) uv triangles are skipped
        const double lo_x = std::fmin(x0, std::fmin(x1, x2)), hi_x = std::fmax(x0, std::fmax(x1, x2));
        const double lo_y = std::fmin(y0, std::fmin(y1, y2)), hi_y = std::fmax(y0, std::fmax(y1, y2));
        if (hi_x < 0.0 || hi_y < 0.0 || lo_x > 1.0 || lo_y > 1.0) continue;
        // the texels whose centres can lie inside, one texel of slack on every side
        const uint32_t i0 = (uint32_t)std::fmax(0.0, std::floor(lo_x * W) - 1.0), i1 = (uint32_t)std::fmin(W - 1.0, std::ceil(hi_x * W) + 1.0);
        const uint32_t j0 = (uint32_t)std::fmax(0.0, std::floor(lo_y * H) - 1.0), j1 = (uint32_t)std::fmin(H - 1.0, std::ceil(hi_y * H) + 1.0);
        for (uint32_t j = j0; j <= j1; ++j)
            for (uint32_t i = i0; i <= i1; ++i) {
                const size_t at = (size_t)j * width + i;
                if (owner[at] != none) continue;
                const double px = ((double)i + 0.5) / W, py = ((double)j + 0.5) / H;
                const double b0 = ((x2 - x1) * (py - y1) - (y2 - y1) * (px - x1)) / area;
                const double b1 = ((x0 - x2) * (py - y2) - (y0 - y2) * (px - x2)) / area;
                const double b2 = ((x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)) / area;
                if (!(b0 >= 0.0 && b1 >= 0.0 && b2 >= 0.0)) continue;
                owner[at] = m.tri_first + t;
                vw[2 * at] = (float)b1;
                vw[2 * at + 1] = (float)b2;
            }
    }
    uint64_t n = 0;
    for (size_t at = 0; at < n_texels; ++at) {
        if (owner[at] == none) continue;
        if (n < capacity) {
            points_out[n].instance = inst;
            points_out[n].prim = owner[at];
            points_out[n].v = vw[2 * at];
            points_out[n].w = vw[2 * at + 1];
            texels_out[n] = (uint32_t)at;
        }
        ++n;
    }
    *n_out = n;
    return SPT_OK;
}

}  // extern "C"

// C entry points of libspt_host.so (see include/spt_host.h for the reference
// counterparts of each function).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../../include/spt_block_cand.h"
#include "../../../include/spt_camera_models.h"
#include "../../../include/spt_origin_cand.h"
#include "host_scene.hpp"
#include "json.hpp"

namespace spt_host {

static thread_local std::string g_error;
void set_error(const std::string& m) { g_error = m; }

}  // namespace spt_host

using namespace spt_host;

struct spt_host_scene {
    HostScene* hs;
};

struct spt_host_animation {
    Animation* an;
};

// The body of an entry point that edits a scene: a HostError becomes its status and message
template <class Body>
static spt_status host_guarded(const char* who, Body&& body) {
    try {
        body();
        return SPT_OK;
    } catch (const HostError& e) {
        set_error(e.msg);
        return e.code;
    } catch (const std::exception& e) {
        set_error(std::string(who) + ": " + e.what());
        return SPT_HOST_ERR_PARSE;
    }
}

static Affine affine_of(const float* f) {
    Affine a;
    a.m.c0 = {f[0], f[1], f[2]};
    a.m.c1 = {f[3], f[4], f[5]};
    a.m.c2 = {f[6], f[7], f[8]};
    a.t = {f[9], f[10], f[11]};
    return a;
}

extern "C" {

const char* spt_host_last_error(void) { return g_error.c_str(); }

spt_status spt_host_catmull_clark(const char* ply_path, uint32_t fas_times, uint32_t* n_patches, float** control_points_out) {
    if (!ply_path || !n_patches || !control_points_out) { set_error("catmull_clark: null argument"); return SPT_ERR_INVALID_ARG; }
    *n_patches = 0;
    *control_points_out = nullptr;
    try {
        const std::vector<float> cps = catmull_clark_patches(ply_path, fas_times);
        float* out = static_cast<float*>(std::malloc(std::max<size_t>(cps.size(), 1) * sizeof(float)));
        if (!out) { set_error("catmull_clark: out of memory"); return SPT_ERR_OUT_OF_MEMORY; }
        std::memcpy(out, cps.data(), cps.size() * sizeof(float));
        *n_patches = (uint32_t)(cps.size() / 48);
        *control_points_out = out;
        return SPT_OK;
    } catch (const HostError& e) {
        set_error(e.msg);
        return e.code;
    } catch (const std::exception& e) {
        set_error(std::string("catmull_clark: ") + e.what());
        return SPT_HOST_ERR_PARSE;
    }
}

spt_status spt_host_load_scene(const char* scene_json_path, spt_host_scene** out) {
    if (!scene_json_path || !out) { set_error("load_scene: null argument"); return SPT_ERR_INVALID_ARG; }
    *out = nullptr;
    try {
        HostScene* hs = load_scene_file(scene_json_path);
        *out = new spt_host_scene{hs};
        return SPT_OK;
    } catch (const HostError& e) {
        set_error(e.msg);
        return e.code;
    } catch (const std::exception& e) {
        set_error(std::string("load_scene: ") + e.what());
        return SPT_HOST_ERR_PARSE;
    }
}

// (the records of meshes spt_host_scene_set_mesh_vertices left pending are made here: a reader of the descriptor sees none missing)
const spt_scene_desc* spt_host_scene_desc(const spt_host_scene* scene) {
    if (!scene) return nullptr;
    try {
        scene->hs->materialize();
    } catch (...) {   // (nothing set_mesh_vertices lets through is known to get here)
        return nullptr;
    }
    return &scene->hs->desc;
}

spt_status spt_host_scene_set_bezier_newton(spt_host_scene* scene, int32_t newton) {
    if (!scene) { set_error("scene_set_bezier_newton: null argument"); return SPT_ERR_INVALID_ARG; }
    for (spt_bezier_patch& bp : scene->hs->bezier_patches) bp.cp[0][0][3] = newton ? SPT_BEZIER_NEWTON : 0.0f;   // the desc points at this array
    return SPT_OK;
}

spt_status spt_host_scene_instance_index(const spt_host_scene* scene, const char* name, uint32_t* index) {
    if (!scene || !name || !index) { set_error("scene_instance_index: null argument"); return SPT_ERR_INVALID_ARG; }
    auto it = scene->hs->inst_index.find(name);
    if (it == scene->hs->inst_index.end()) { set_error(std::string("There is no instance named '") + name + "'"); return SPT_HOST_ERR_SCHEMA; }
    *index = it->second;
    return SPT_OK;
}

spt_status spt_host_scene_set_transforms(spt_host_scene* scene, uint32_t n, const char* const* names, const float* fwd) {
    if (!scene || (n && (!names || !fwd))) { set_error("scene_set_transforms: null argument"); return SPT_ERR_INVALID_ARG; }
    return host_guarded("scene_set_transforms", [&] {
        std::vector<std::pair<std::string, Affine>> moves;
        for (uint32_t i = 0; i < n; ++i) {
            if (!names[i]) throw HostError(SPT_ERR_INVALID_ARG, "scene_set_transforms: null name");
            moves.emplace_back(names[i], affine_of(fwd + 12 * (size_t)i));
        }
        scene->hs->set_transforms(moves);
    });
}

spt_status spt_host_scene_set_light(spt_host_scene* scene, const char* name, const spt_light* light) {
    if (!scene || !name || !light) { set_error("scene_set_light: null argument"); return SPT_ERR_INVALID_ARG; }
    return host_guarded("scene_set_light", [&] { scene->hs->set_light(name, *light); });
}

spt_status spt_host_scene_mesh_index(const spt_host_scene* scene, const char* primitive_name, uint32_t* mesh) {
    if (!scene || !primitive_name || !mesh) { set_error("scene_mesh_index: null argument"); return SPT_ERR_INVALID_ARG; }
    return host_guarded("scene_mesh_index", [&] { *mesh = scene->hs->mesh_source(primitive_name).mesh; });
}

spt_status spt_host_scene_mesh_positions(const spt_host_scene* scene, const char* primitive_name, uint32_t* n_vertices, float* out) {
    if (!scene || !primitive_name || !n_vertices) { set_error("scene_mesh_positions: null argument"); return SPT_ERR_INVALID_ARG; }
    return host_guarded("scene_mesh_positions", [&] {
        const MeshSource& src = scene->hs->mesh_source(primitive_name);
        *n_vertices = (uint32_t)src.pos.size();
        for (size_t i = 0; out && i < src.pos.size(); ++i) { out[3 * i] = src.pos[i].x; out[3 * i + 1] = src.pos[i].y; out[3 * i + 2] = src.pos[i].z; }
    });
}

spt_status spt_host_scene_set_mesh_positions(spt_host_scene* scene, const char* primitive_name, uint32_t n_vertices, const float* positions, const float* normals) {
    if (!scene || !primitive_name || !positions) { set_error("scene_set_mesh_positions: null argument"); return SPT_ERR_INVALID_ARG; }
    return host_guarded("scene_set_mesh_positions", [&] { scene->hs->set_mesh_positions(primitive_name, n_vertices, positions, normals); });
}

spt_status spt_host_scene_mesh_topology(const spt_host_scene* scene, const char* primitive_name, spt_mesh_topology* out) {
    if (!scene || !primitive_name || !out) { set_error("scene_mesh_topology: null argument"); return SPT_ERR_INVALID_ARG; }
    return host_guarded("scene_mesh_topology", [&] {
        const MeshSource& src = scene->hs->mesh_source(primitive_name);
        static_assert(sizeof(V3) == 3 * sizeof(float), "MeshSource::nrm is handed out as 3 floats per vertex");
        std::memset(out, 0, sizeof *out);
        out->size = (uint32_t)sizeof(spt_mesh_topology);
        out->mesh = src.mesh;
        out->n_vertices = (uint32_t)src.pos.size();
        out->tri_count = (uint32_t)(src.idx.size() / 3);
        out->indices = src.idx.data();
        out->face_of_tri = src.order.data();
        out->uv = src.uv.data();
        out->normals = &src.nrm.data()->x;
    });
}

spt_status spt_host_scene_set_mesh_vertices(spt_host_scene* scene, const char* primitive_name, uint32_t n_vertices, const float* positions, const float* normals) {
    if (!scene || !primitive_name || !positions) { set_error("scene_set_mesh_vertices: null argument"); return SPT_ERR_INVALID_ARG; }
    return host_guarded("scene_set_mesh_vertices", [&] { scene->hs->set_mesh_vertices(primitive_name, n_vertices, positions, normals); });
}

spt_status spt_host_scene_dynamic(const spt_host_scene* scene, spt_scene_update_desc* out) {
    if (!scene || !out) { set_error("scene_dynamic: null argument"); return SPT_ERR_INVALID_ARG; }
    const spt_scene_desc& d = scene->hs->desc;   // (no materialize: none of the four arrays depends on a pending mesh's records)
    std::memset(out, 0, sizeof *out);
    out->size = (uint32_t)sizeof(spt_scene_update_desc);
    out->n_tlas_nodes = d.n_tlas_nodes; out->tlas_nodes = d.tlas_nodes;
    out->n_instances = d.n_instances; out->instances = d.instances;
    out->n_lights = d.n_lights; out->lights = d.lights;
    out->light_alias = d.light_alias;
    return SPT_OK;
}

spt_status spt_host_animation_load(const char* path, const spt_host_scene* scene, spt_host_animation** out) {
    if (!path || !scene || !out) { set_error("animation_load: null argument"); return SPT_ERR_INVALID_ARG; }
    *out = nullptr;
    return host_guarded("animation_load", [&] { *out = new spt_host_animation{load_animation(path, *scene->hs)}; });
}

uint32_t spt_host_animation_frames(const spt_host_animation* animation) { return animation ? (uint32_t)animation->an->frames.size() : 0u; }

spt_status spt_host_animation_apply(const spt_host_animation* animation, uint32_t frame, spt_host_scene* scene) {
    if (!animation || !scene) { set_error("animation_apply: null argument"); return SPT_ERR_INVALID_ARG; }
    if (frame >= animation->an->frames.size()) { set_error("animation_apply: no such frame"); return SPT_ERR_INVALID_ARG; }
    return host_guarded("animation_apply", [&] { scene->hs->set_transforms(animation->an->frames[frame]); });
}

void spt_host_animation_free(spt_host_animation* animation) {
    if (!animation) return;
    delete animation->an;
    delete animation;
}

// Scene::get_camera (src/core/scene.rs:29-41): by name, or the only one
spt_status spt_host_scene_camera(const spt_host_scene* scene, const char* name, spt_camera* out) {
    if (!scene || !out) { set_error("scene_camera: null argument"); return SPT_ERR_INVALID_ARG; }
    const HostScene& hs = *scene->hs;
    if (name) {
        auto it = hs.camera_index.find(name);
        if (it == hs.camera_index.end()) { set_error(std::string("There is no camera names ") + name); return SPT_HOST_ERR_SCHEMA; }
        *out = hs.cameras[it->second];
        return SPT_OK;
    }
    if (hs.cameras.size() == 1) { *out = hs.cameras[0]; return SPT_OK; }
    set_error("There are multiple cameras so a name must be given");
    return SPT_HOST_ERR_SCHEMA;
}

void spt_host_scene_free(spt_host_scene* scene) {
    if (!scene) return;
    delete scene->hs;
    delete scene;
}

// loader::load_renderer (src/loader/json.rs:19-51) + create_sampler_from_params
// (src/pixel_sampler/mod.rs:28-43) + create_filter_from_params (src/filter/mod.rs:19-32).
// filter == nullptr: spt_host_load_renderer, which knows the reference's box only; else spt_host_load_renderer_filter, which also
// takes the weighted filters of spt_film_filter and returns the desc.
static spt_status load_renderer(const char* path, spt_render_params* params, float* filter_radius, spt_filter_desc* filter) {
    try {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw HostError(SPT_HOST_ERR_IO, std::string("cannot open '") + path + "'");
        std::stringstream ss;
        ss << f.rdbuf();
        std::string text = ss.str();
        JsonValue root;
        try { root = JsonParser(text).parse(); } catch (const std::runtime_error& e) { throw HostError(SPT_HOST_ERR_PARSE, e.what()); }
        const JsonValue* md = root.get("max_depth");
        if (!md) throw HostError(SPT_HOST_ERR_SCHEMA, "renderer - There is no 'max_depth' field");
        if (md->kind != JsonValue::Int) throw HostError(SPT_HOST_ERR_SCHEMA, "renderer - 'max_depth' shoule be integer");
        const JsonValue* sv = root.get("sampler");
        if (!sv || sv->kind != JsonValue::Object) throw HostError(SPT_HOST_ERR_SCHEMA, "renderer - There is no 'sampler' field");
        auto need = [&](const JsonValue* o, const char* key, JsonValue::Kind kind, const char* owner, const char* hint) {
            const JsonValue* v = o->get(key);
            if (!v) throw HostError(SPT_HOST_ERR_SCHEMA, std::string(owner) + " - there is no '" + key + "' field");
            if (v->kind != kind) throw HostError(SPT_HOST_ERR_SCHEMA, std::string(owner) + " - '" + key + "' should be " + hint);
            return v;
        };
        std::string sty = need(sv, "type", JsonValue::String, "sampler", "string")->s;
        uint32_t sampler, spp, dx = 0, dy = 0;
        if (sty == "random" || sty == "recurrence") {
            sampler = sty == "random" ? SPT_SAMPLER_RANDOM : SPT_SAMPLER_RECURRENCE;
            spp = (uint32_t)need(sv, "spp", JsonValue::Int, ("sampler-" + sty).c_str(), "integer")->i;
        } else if (sty == "jittered") {
            sampler = SPT_SAMPLER_JITTERED;
            dx = (uint32_t)need(sv, "division_x", JsonValue::Int, "sampler-jittered", "integer")->i;
            dy = (uint32_t)need(sv, "division_y", JsonValue::Int, "sampler-jittered", "integer")->i;
            spp = dx * dy;
        } else {
            throw HostError(SPT_HOST_ERR_SCHEMA, "sampler: unknown type '" + sty + "'");
        }
        const JsonValue* fv = root.get("filter");
        if (!fv || fv->kind != JsonValue::Object) throw HostError(SPT_HOST_ERR_SCHEMA, "renderer - There is no 'filter' field");
        std::string fty = need(fv, "type", JsonValue::String, "filter", "string")->s;
        spt_filter_desc fd{};
        fd.size = (uint32_t)sizeof(spt_filter_desc);
        // a number that may be left out; like every float of the loader, an integer literal is a schema error
        auto opt = [&](const char* key, const char* owner, float dflt) {
            return fv->get(key) ? (float)need(fv, key, JsonValue::Float, owner, "float")->f : dflt;
        };
        float radius;
        if (fty == "box") {
            fd.type = SPT_FILTER_BOX;
            radius = (float)need(fv, "radius", JsonValue::Float, "filter-box", "float")->f;
        } else if (filter && fty == "tent") {
            fd.type = SPT_FILTER_TENT;
            radius = (float)need(fv, "radius", JsonValue::Float, "filter-tent", "float")->f;
        } else if (filter && fty == "gaussian") {
            fd.type = SPT_FILTER_GAUSSIAN;
            radius = (float)need(fv, "radius", JsonValue::Float, "filter-gaussian", "float")->f;
            fd.p0 = opt("alpha", "filter-gaussian", 2.0f);
        } else if (filter && fty == "mitchell") {
            fd.type = SPT_FILTER_MITCHELL;
            radius = opt("radius", "filter-mitchell", 2.0f);
            fd.p0 = opt("b", "filter-mitchell", 1.0f / 3.0f);
            fd.p1 = opt("c", "filter-mitchell", 1.0f / 3.0f);
        } else {
            throw HostError(SPT_HOST_ERR_SCHEMA, "filter: unknown type '" + fty + "'");
        }
        fd.radius = radius;
        const JsonValue* ty = root.get("type");
        if (!ty) throw HostError(SPT_HOST_ERR_SCHEMA, "renderer - There is no 'type' field");
        if (ty->kind != JsonValue::String) throw HostError(SPT_HOST_ERR_SCHEMA, "renderer - 'type' shoule be string");
        if (ty->s != "pt") throw HostError(SPT_HOST_ERR_SCHEMA, "renderer - unknown type '" + ty->s + "'");
        params->max_depth = (uint32_t)md->i;
        params->sampler = sampler;
        params->spp = spp;
        params->division_x = dx;
        params->division_y = dy;
        // BoxFilter::new (src/filter/boxf.rs:11-14): any radius; 0.5 is the plain per-pixel mean.  (A weighted filter's radius
        // decides the halo a sample-keeping film stores.)
        params->filter_radius = radius;
        if (radius != 0.5f) params->flags |= SPT_RENDER_BOX_RADIUS;
        if (filter_radius) *filter_radius = radius;
        if (filter) *filter = fd;
        return SPT_OK;
    } catch (const HostError& e) {
        set_error(e.msg);
        return e.code;
    }
}

spt_status spt_host_block_candidates(const spt_camera* cam, uint32_t width, uint32_t height, uint32_t shard_index, uint32_t shard_count,
                                     uint32_t strip_rows, uint32_t rows, uint32_t block, const float* inv, const float* fwd, uint32_t n_tris,
                                     const float* tri_pos, uint64_t* mask_out) {
    if (!cam || !inv || !fwd || !mask_out || (n_tris != 0u && !tri_pos)) { g_error = "block_candidates: null argument"; return SPT_ERR_INVALID_ARG; }
    if (width == 0u || height == 0u || shard_count == 0u || shard_index >= shard_count || strip_rows == 0u || n_tris > SPT_BC_MAX_TRIS) {
        g_error = "block_candidates: empty image, bad shard layout or more than 64 triangles";
        return SPT_ERR_INVALID_ARG;
    }
    // the camera and image terms as the device forms them (plan_ctx of spt_hip.hip, k_primary)
    spt_bc_view v;
    for (int k = 0; k < 3; ++k) {
        v.fwd_hc[k] = cam->forward[k] * cam->half_cot_half_fov;
        v.right[k] = cam->right[k]; v.up[k] = cam->up[k]; v.fwd[k] = cam->forward[k];
    }
    v.aspect = (float)width / (float)height;
    v.width_inv = 1.0f / (float)width;
    v.height_inv = 1.0f / (float)height;
    v.width = width; v.height = height;
    const spt_bc_layout l{shard_index, shard_count, strip_rows, 0u, rows};
    // the object-space eye of the eye-relative copy (make_eye_blob: xf_point(inv, eye))
    float oo[3];
    for (int k = 0; k < 3; ++k) oo[k] = ((inv[k] * cam->eye[0] + inv[3 + k] * cam->eye[1]) + inv[6 + k] * cam->eye[2]) + inv[9 + k];
    uint64_t mask = 0ull;
    uint32_t i0, i1, row;
    if (spt_bc_block_pixels(&v, &l, block, &i0, &i1, &row)) {
        const uint32_t row_end = std::min(row + SPT_BC_ROWS, rows);
        uint32_t j0, j1;
        while (spt_bc_next_run(&l, &row, row_end, &j0, &j1)) {
            spt_bc_cone cone;
            spt_bc_cone_make(&v, i0, i1, j0, j1, inv, fwd, &cone);
            for (uint32_t t = 0; t < n_tris; ++t) {
                const float* p = tri_pos + 9u * t;
                float s[3], e1[3], e2[3];
                for (int k = 0; k < 3; ++k) { s[k] = oo[k] - p[k]; e1[k] = p[3 + k] - p[k]; e2[k] = p[6 + k] - p[k]; }
                if (spt_bc_keep(&cone, s, e1, e2)) mask |= 1ull << t;
            }
        }
    }
    *mask_out = mask;
    return SPT_OK;
}

spt_status spt_host_origin_candidates(uint32_t n_instances, const float* inv, const float* fwd, const float* nrm, uint32_t n_tris,
                                      const uint32_t* tri_instance, const float* tri_pos, const float* tri_nrm, uint64_t* words_out,
                                      double* info_out) {
    if (!inv || !fwd || !nrm || !tri_instance || !tri_pos || !tri_nrm || !words_out || !info_out) { g_error = "origin_candidates: null argument"; return SPT_ERR_INVALID_ARG; }
    std::vector<spt_oc_instance> in(n_instances);
    for (uint32_t i = 0; i < n_instances; ++i) {
        std::memcpy(in[i].inv, inv + 12u * i, sizeof in[i].inv);
        std::memcpy(in[i].fwd, fwd + 12u * i, sizeof in[i].fwd);
        std::memcpy(in[i].nrm, nrm + 9u * i, sizeof in[i].nrm);
    }
    std::vector<spt_oc_triangle> tr(n_tris);
    for (uint32_t k = 0; k < n_tris; ++k) {
        const float* p = tri_pos + 9u * k;
        for (int a = 0; a < 3; ++a) { tr[k].p0[a] = p[a]; tr[k].e1[a] = p[3 + a] - p[a]; tr[k].e2[a] = p[6 + a] - p[a]; }   // the blob's f32 differences
        std::memcpy(tr[k].n, tri_nrm + 9u * k, sizeof tr[k].n);
        tr[k].instance = tri_instance[k];
        tr[k].id = k;
    }
    uint64_t words[SPT_OC_WORDS * SPT_OC_MAX_TRIS];
    spt_oc_info info;
    if (!spt_oc_build(in.data(), n_instances, tr.data(), n_tris, words, &info)) {
        g_error = "origin_candidates: no triangle, more than 64, a bad instance index or a singular transform";
        return SPT_ERR_INVALID_ARG;
    }
    std::memcpy(words_out, words, sizeof(uint64_t) * SPT_OC_WORDS * n_tris);
    const double out[8] = {info.center[0], info.center[1], info.center[2], info.radius, info.reach, info.delta, info.delta_scene, (double)info.tight};
    std::memcpy(info_out, out, sizeof out);
    return SPT_OK;
}

spt_status spt_host_camera_rays(const spt_camera_model* model, const spt_render_params* plan, uint32_t first, uint32_t count, spt_path_ray* rays,
                                spt_ray_aux* aux) {
    if (!plan || (count != 0 && !rays)) { g_error = "camera_rays: null argument"; return SPT_ERR_INVALID_ARG; }
    if (const char* why = spt_cm_check(model)) { g_error = std::string("camera_rays: ") + why; return SPT_ERR_INVALID_ARG; }
    const spt_render_params& p = *plan;
    if (p.width == 0 || p.height == 0 || p.spp == 0 || p.sampler > SPT_SAMPLER_RECURRENCE || (uint64_t)first + count > p.spp) {
        g_error = "camera_rays: bad plan (width, height, spp > 0, a known sampler) or samples past the plan's spp";
        return SPT_ERR_INVALID_ARG;
    }
    if (p.sampler == SPT_SAMPLER_JITTERED && (p.division_x == 0 || p.division_y == 0)) { g_error = "camera_rays: jittered sampler without divisions"; return SPT_ERR_INVALID_ARG; }
    // what plan_ctx of the device library makes once per plan (pt.rs:239, 250-254, 272-275)
    const float aspect = (float)p.width / (float)p.height, width_inv = 1.0f / (float)p.width, height_inv = 1.0f / (float)p.height;
    const float spp_sqrt_inv = 1.0f / std::sqrt((float)p.spp);
    const float aux_dx = aspect * width_inv * spp_sqrt_inv, aux_dy = height_inv * spp_sqrt_inv;
    const spt_cm_plan pl = spt_cm_plan_make(model, p.width, p.height);
    size_t k = 0;
    for (uint32_t s = first; s < first + count; ++s)
        for (uint32_t j = 0; j < p.height; ++j)
            for (uint32_t i = 0; i < p.width; ++i, ++k) {
                const uint32_t pixel = j * p.width + i;
                float ox, oy;
                if (p.sampler == SPT_SAMPLER_RECURRENCE) {
                    spt_r2_offset(pixel, p.spp, s, &ox, &oy);
                } else {
                    spt_rng rng = spt_rng_seed(p.seed, pixel, s);
                    const float a = spt_rng_f32(&rng), b = spt_rng_f32(&rng);
                    if (p.sampler == SPT_SAMPLER_JITTERED) {
                        ox = ((float)(s % p.division_x) + a) * (1.0f / (float)p.division_x);
                        oy = ((float)(s / p.division_x) + b) * (1.0f / (float)p.division_y);
                    } else { ox = a; oy = b; }
                }
                float x, y, lx = 0.0f, ly = 0.0f;
                spt_cm_screen(i, j, p.height, ox, oy, width_inv, height_inv, aspect, &x, &y);
                if (model->type == SPT_CAMERA_THIN_LENS) spt_cm_lens_point(p.seed, pixel, s, &lx, &ly);
                spt_path_ray& r = rays[k];
                std::memset(&r, 0, sizeof r);
                spt_cm_ray(model, &pl, x, y, lx, ly, r.o, r.d);
                r.t_min = SPT_CM_T_MIN;
                r.stream_a = pixel;
                r.stream_b = s;
                if (aux) {
                    spt_ray_aux& a = aux[k];
                    std::memset(&a, 0, sizeof a);
                    spt_cm_ray(model, &pl, x + aux_dx, y, lx, ly, a.rx_o, a.rx_d);
                    spt_cm_ray(model, &pl, x, y + aux_dy, lx, ly, a.ry_o, a.ry_d);
                }
            }
    return SPT_OK;
}

spt_status spt_host_load_renderer(const char* path, spt_render_params* params, float* filter_radius) {
    if (!path || !params) { set_error("load_renderer: null argument"); return SPT_ERR_INVALID_ARG; }
    return load_renderer(path, params, filter_radius, nullptr);
}

spt_status spt_host_load_renderer_filter(const char* path, spt_render_params* params, spt_filter_desc* filter) {
    if (!path || !params || !filter) { set_error("load_renderer_filter: null argument"); return SPT_ERR_INVALID_ARG; }
    return load_renderer(path, params, nullptr, filter);
}

}  // extern "C"

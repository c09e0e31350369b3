// The scene builder: everything spt_scene_create and spt_scene_update derive from a descriptor on the host - the checks of the
// descriptor, the device-side BLAS and TLAS (binned SAH), the wide and the compressed 4-wide node forms, the traversal blob and its
// layout, the kernel choices that follow from the scene, the texture programs.  Plain host vectors in, plain host vectors out: no
// HIP runtime call, no kernel header, no read of the environment outside BuildOptions::from_env().  spt_hip.hip opens the device,
// uploads what comes out of here and schedules the kernels; tests/scene_build_check.cpp runs this unit alone, on the CPU.
#pragma once
#include <hip/hip_vector_types.h>   // float4, uint4, uint2, float2

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/spt_abi.h"
#include "abi_error.h"
#include "scene_consts.h"
#include "scene_refit.h"

namespace scene_build {

// What the environment asks of the builder, read once per spt_scene_create / spt_scene_update (from_env) and passed down.  The
// defaults are what an empty environment gives.
struct BuildOptions {
    // tuning knobs of the BLAS builder (defaults measured on cfg2 / cfg5; the environment overrides exist for that measurement only)
    uint32_t bvh_max_leaf = 4;           // SPT_BVH_MAX_LEAF, clamped to 1 .. 15
    float bvh_traversal_cost = 1.2f;     // SPT_BVH_TRAVERSAL_COST: one wide-node visit (two slab tests) relative to one triangle test
    bool debug_bvh = false;              // SPT_DEBUG_BVH: a line per device-built tree on stderr
    bool stream = true;                  // SPT_NO_STREAM unset: the streaming walker serves a scene whose tables could be built
    uint64_t flat_budget = kFlatBudget;  // SPT_FLAT_BUDGET: triangle tests per ray up to which a scene is walked exhaustively, 0 = never
    bool eye_blob = true;                // SPT_NO_EYE_BLOB unset: the eye-relative copy of an LDS-resident scene (eye.h)
    bool reference_bvh = false;          // SPT_REFERENCE_BVH: walk the caller's trees instead of the device-built ones (creation only)
    bool lds_geo = true;                 // SPT_NO_LDS_GEO unset; false drives small scenes through the large-scene form (creation only)
    bool bez_lds = false;                // SPT_BEZ_LDS: LDS-resident nested walkers for scenes with patches too (creation only)
    bool with_bezier = false;            // not of the environment: the library has the Bezier-patch primitive compiled in
    static BuildOptions from_env();
};

// What spt_scene_update needs again of the descriptor a scene was created from, and of what spt_scene_create derived from the
// part of it that an update keeps: the scene's own copy, nothing of the caller's memory.
struct SceneFixed {
    uint32_t aggregate = 0, light_sampler = 0, n_instances = 0, n_lights = 0, n_meshes = 0, n_spheres = 0, n_surfaces = 0, n_bezier_patches = 0, n_tris = 0;
    int32_t env_light_index = -1;
    uint32_t env_light_type = 0;      // the type of lights[env_light_index] at creation
    bool has_env = false;
    bool own_bvh = true;              // SPT_REFERENCE_BVH was not set
    bool n4 = false;                  // the large-scene form: compressed 4-wide BLAS nodes, dynamic sections behind the static ones
    uint32_t blas_depth = 0;          // of the caller's BLAS trees
    uint32_t own_blas_depth = 0;      // of the device-built ones
    uint32_t max_blas_need = 0;       // pending entries of a walk of the 4-wide BLAS
    uint32_t blas_f4 = 0;             // the BLAS nodes of the form in use, in float4
    size_t tables_bytes = 0;          // what the shading tables add behind an LDS-resident blob
    bool simple_fixed = false, fused_fixed = false;   // spt_scene::simple / ::fused but for the lights' types
    std::vector<uint32_t> mesh_tris;                  // triangle count per mesh
    std::vector<uint32_t> mesh_first;                 // ... and its first triangle (ABI index and leaf-order slot alike)
    std::vector<uint32_t> mesh_depth;                 // depth of the device-built tree per mesh (own_bvh)
    // n4, per mesh: its first 4-wide node, its nodes and the height of its root node (spt_scene_deform refits level by level)
    std::vector<std::array<uint32_t, 3>> n4_nodes;
    std::vector<spt_sphere> spheres;
    std::vector<uint8_t> surf_class, surf_emissive;   // per surface: the shade class of its material, luminance of its emission > 0
    std::vector<std::array<double, 6>> mesh_box;      // object-space bounds of every mesh's vertices (lo, hi)
    std::vector<float4> mesh_rec;                     // the blob's mesh records of the form in use
    // LDS-resident scenes only (<= 32 KB): the static sections of the blob, which an update writes again with the dynamic ones
    std::vector<float4> wblas, tri_sec, attr_sec, surf_sec, mat_sec;
    uint32_t tail_first = 0, tail_cap = 0;            // n4: where the dynamic sections start in the blob and what the allocation holds of them (float4)
};

// The four arrays an update replaces, as spt_scene_create and spt_scene_update both read them (the caller's memory)
struct DynView {
    uint32_t aggregate, light_sampler;
    uint32_t n_tlas_nodes, n_instances, n_lights, n_spheres, n_meshes, n_bezier_patches, n_surfaces;
    bool has_env;
    const spt_bvh_node* tlas_nodes;
    const spt_instance* instances;
    const spt_light* lights;
    spt_alias_table light_alias;
    const uint8_t* surf_emissive;
};

// Everything of a scene that depends on where its instances and lights are: built on the host from a DynView, then committed
struct SceneDynamic {
    uint32_t tlas_root = 0, s_root = 0, n_tlas_nodes = 0, stack_cap = 0, flat = 0;
    float tlas_lo[3] = {0, 0, 0}, tlas_hi[3] = {0, 0, 0};
    uint32_t o_sinst = 0, o_tlas = 0, o_inst = 0, o_mesh = 0, o_sph = 0, o_blas = 0, o_tri = 0, o_tord = 0, o_attr = 0, o_surf = 0, o_mat = 0, o_light = 0;
    uint32_t geo_f4 = 0;
    size_t plain_f4 = 0;              // the blob without the shading tables (what has to fit LDS for the LDS-resident form)
    uint32_t tail_first = 0;          // large-scene form: where the sections an update rewrites start (dyn_layout)
    bool swalk = false, lds_tables = false, fused = false, simple = false, eye_ok = false;
    std::vector<uint8_t> cls;
    std::vector<uint32_t> tlas_order;
    std::vector<float4> wtlas, stlas, sinst;
    std::vector<float4> blob;         // the whole blob (LDS-resident scenes, creation) or the dynamic sections from SceneFixed::tail_first
    double bs_center[3] = {0, 0, 0}, bs_radius = 0, world_lo[3] = {0, 0, 0}, world_hi[3] = {0, 0, 0};
    bool bs_valid = false;
    std::vector<std::array<double, 24>> hull_corners;
};

// The static sections of the blob as spt_scene_create has them at hand (a large scene's are not kept)
struct StaticSections {
    const float4* wblas;
    const void* tri;
};

// The postfix programs of a scene's textures (shading.h, "textures"): per texture (first instruction, count) in `prog`; an image
// leaf's chain of input modifiers in `chain`
struct TexturePools {
    std::vector<uint4> prog;
    std::vector<uint2> roots;
    std::vector<uint32_t> chain;
};

// Everything of a scene that an update keeps, as spt_scene_create uploads it (build_static)
struct StaticBuild {
    SceneFixed fixed;
    bool lds_geo = false;                 // the traversal geometry is small enough to live in LDS: the blob's LDS-resident form
    std::vector<spt_tri_pos> tri_blob;    // the triangles in leaf order of the tree that is walked: (p0, e1, e2), ABI index in the first pad lane
    std::vector<float4> wblas;            // the BLAS nodes of the form in use (fixed.n4)
    std::vector<std::pair<uint32_t, uint32_t>> blas_range;   // LDS-resident form, per mesh: its wide nodes [first, end) in units of 4 float4
    std::vector<float4> env_px;           // per env texel (r, g, b, alias prop)
    std::vector<uint2> env_uk;            // ... and (alias u as bits, alias k)
    std::vector<float2> ss_cdf;           // the BSSRDF radius table (`subsurface` only)
    TexturePools tex;                     // (`textured` only)
    bool textured = false, subsurface = false, has_probe = false, has_pndf = false, bez_newton = false;   // see spt_scene (spt_hip.hip)
    StaticSections sections() const { return StaticSections{wblas.data(), tri_blob.data()}; }
};

DynView dyn_view(const spt_scene_desc& s, const uint8_t* surf_emissive);
void validate_instances(const DynView& s, const BuildOptions& opt, const char* who);
void validate_lights(const DynView& s, const char* who);
void validate_light_alias(const DynView& s, const char* who);
void validate(const spt_scene_desc& s, const BuildOptions& opt);
// whether a blob of plain_f4 float4 (+ extra bytes behind it) fits LDS next to the traversal stack
bool lds_fits(size_t plain_f4, size_t extra_bytes = 0);
// The part of a (validated) scene that an update keeps.  The LDS decision needs the size of the dynamic sections, so the trees
// over the instances are built here once for it.
StaticBuild build_static(const spt_scene_desc& s, const BuildOptions& opt);
// The part that depends on the instances and the lights: dyn_trees -> dyn_layout -> dyn_decide -> dyn_fill -> dyn_bounds.  `st`:
// the static sections, with which the whole blob is written (a creation; every update of the LDS-resident form); nullptr: the
// blob from fx.tail_first on (an update of the large-scene form, which keeps no copy of its static sections).
SceneDynamic build_dynamic(const SceneFixed& fx, const DynView& s, const BuildOptions& opt, bool lds_geo, size_t n_blas_ranges, const StaticSections* st);

// spt_scene_deform.  The checks of the named meshes against the scene (every refusal that needs no build).
void validate_deform(const SceneFixed& fx, uint32_t n_meshes, const spt_mesh_deform* meshes);
// Large-scene form: what the host keeps of a named mesh - its object-space box and its record with pad(bounds of the whole
// mesh), which contains every box the refit kernels make (scene_refit.h).  Returns that box per named mesh.
std::vector<RefitBox> deform_fixed_n4(SceneFixed& fx, uint32_t n_meshes, const spt_mesh_deform* meshes);
// The same from the raw bounds of the named meshes' vertices (spt_scene_deform_vertices, whose records are made on the device)
std::vector<RefitBox> deform_fixed_n4_raw(SceneFixed& fx, uint32_t n_meshes, const uint32_t* mesh_ids, const RefitBox* raw);
// LDS-resident form: the named meshes' static sections built again with the creation's functions (binned-SAH tree, wide nodes,
// leaf-order triangles, attributes, record, box, depth), the other meshes' nodes moved to where they now start.
void deform_fixed_lds(SceneFixed& fx, std::vector<std::pair<uint32_t, uint32_t>>& blas_range, uint32_t n_meshes, const spt_mesh_deform* meshes,
                      const BuildOptions& opt);

}  // namespace scene_build

// Owning storage behind a spt_scene_desc (the arrays a Rust `Scene::flatten()`
// would own on the reference side).
#pragma once
#include <array>
#include <map>
#include <string>
#include <vector>

#include "../../../include/spt_host.h"
#include "hmath.hpp"

namespace spt_host {

struct HostError {
    spt_status code;
    std::string msg;
    HostError(spt_status c, std::string m) : code(c), msg(std::move(m)) {}
};

// One instance as the loader made it (Instance::new), with what making it again under another transform needs
struct InstRec { spt_instance inst; Affine trans; std::string name; Box prim_box; };
InstRec make_instance_rec(const std::string& name, const Affine& trans, uint32_t prim_type, uint32_t prim_id, const Box& prim_box, uint32_t surf);

// A trimesh primitive of a JSON scene as the OBJ loader made it (single-index vertices), with the triangle order its BLAS build
// chose: what spt_host_scene_set_mesh_positions makes the mesh's records from again
struct MeshSource {
    uint32_t mesh = 0;                  // index in HostScene::meshes
    std::vector<V3> pos, nrm;
    std::vector<float> uv;              // 2 per vertex
    std::vector<uint32_t> idx;          // 3 per face
    std::vector<uint32_t> order;        // triangle k of the mesh's range is face order[k]
    // spt_host_scene_set_mesh_vertices: pos / nrm are newer than the mesh's tri_pos / tri_attr / blas_nodes ranges, which
    // HostScene::materialize makes from them
    bool pending = false;
    std::vector<uint8_t> named;         // per vertex: some face names it (made by the first set_mesh_vertices)
};

// A mesh as the OBJ loader makes it (single-index vertices), and the loader's two functions over it: the vertex tangents
// (TriMesh::calc_tangents) and the two records of face t (TriMesh::new).  include/spt_mesh_assemble.h restates them for the device;
// tests/mesh_assemble_check.cpp compares the two.
struct ObjMesh {
    std::vector<V3> pos, nrm, tan, bit;
    std::vector<float> uv;  // 2 per vertex
    std::vector<uint32_t> idx;
};
void calc_tangents(ObjMesh& m);
void face_records(const ObjMesh& m, uint32_t t, spt_tri_pos& tp, spt_tri_attr& ta);

struct HostScene {
    std::vector<spt_bvh_node> tlas_nodes, blas_nodes;
    std::vector<spt_instance> instances;
    std::vector<spt_mesh> meshes;
    std::vector<spt_tri_pos> tri_pos;
    std::vector<spt_tri_attr> tri_attr;
    std::vector<spt_sphere> spheres;
    std::vector<spt_bezier_patch> bezier_patches;
    std::vector<spt_pndf> pndfs;                 // position-normal distributions (pndf.cpp)
    std::vector<spt_pndf_term> pndf_terms;
    std::vector<spt_pndf_node> pndf_nodes;
    std::vector<uint32_t> pndf_refs, pndf_roots;
    std::vector<spt_surface> surfaces;
    std::vector<spt_material> materials;
    std::vector<spt_medium> mediums;
    std::vector<spt_texture> textures;
    std::vector<spt_image> images;
    std::vector<spt_image_level> image_levels;
    std::vector<uint32_t> texels;
    std::vector<spt_material_recipe> material_recipes;
    std::vector<spt_light> lights;
    std::vector<float> light_props, light_u;
    std::vector<uint32_t> light_k;
    std::vector<float> env_texels, env_props, env_u;
    std::vector<uint32_t> env_k;
    uint32_t env_w = 0, env_h = 0;
    float env_scale[3] = {1, 1, 1};
    uint32_t aggregate = SPT_AGGREGATE_BVH, light_sampler = SPT_LIGHT_SAMPLER_UNIFORM;
    int32_t env_light_index = -1;
    std::vector<spt_camera> cameras;
    std::map<std::string, size_t> camera_index;
    spt_scene_desc desc;
    void finalize_desc();
    // What the part of the descriptor that depends on the instances' transforms and the named lights is made from (kept for
    // spt_host_scene_set_transforms / _set_light): the instances and the named lights by name, the average emission per surface
    std::map<std::string, InstRec> inst_recs;         // name-sorted (Q7: reference order is HashMap order)
    std::map<std::string, spt_light> named_lights;
    std::vector<V3> avg_emissive;
    std::map<std::string, uint32_t> inst_index;       // name -> index in `instances` as they stand
    float instance_area(const InstRec& r) const;
    // tlas_nodes, instances (in TLAS leaf order), lights, the light alias table and desc from the three members above
    void finalize_dynamic();
    void set_transforms(const std::vector<std::pair<std::string, Affine>>& moves);   // all or nothing (HostError)
    void set_light(const std::string& name, const spt_light& light);
    // spt_host_scene_mesh_positions / _set_mesh_positions: the trimesh primitives by name; the names of the meshes that cannot
    // be edited (glTF primitives, Catmull-Clark surfaces)
    std::map<std::string, MeshSource> mesh_sources;
    std::map<std::string, std::string> fixed_meshes;   // name -> why not
    const MeshSource& mesh_source(const std::string& name) const;   // HostError: unknown name, a mesh that cannot be edited
    MeshSource& mesh_source(const std::string& name);
    void set_mesh_positions(const std::string& name, uint32_t n_vertices, const float* positions, const float* normals);   // all or nothing
    // spt_host_scene_set_mesh_vertices: set_mesh_positions with the mesh's records deferred (MeshSource::pending) unless an
    // emissive instance needs them; materialize() makes the records of every pending mesh (every reader of tri_pos / tri_attr /
    // blas_nodes calls it first: spt_host_scene_desc does)
    void set_mesh_vertices(const std::string& name, uint32_t n_vertices, const float* positions, const float* normals);   // all or nothing
    void materialize();
};

HostScene* load_scene_file(const std::string& path);
struct Animation { std::vector<std::vector<std::pair<std::string, Affine>>> frames; };
Animation* load_animation(const std::string& path, const HostScene& hs);
// pndf.cpp: the Gaussian terms and trees of one pndf_conductor material (PndfConductor::new), appended to the scene
uint32_t build_pndf(HostScene& hs, uint32_t base_normal_texture, float sigma_r, float h, const std::string& label);
// catmull.cpp: 16 control points (x, y, z) per bicubic patch of the Catmull-Clark surface of an ASCII PLY control mesh
std::vector<float> catmull_clark_patches(const std::string& ply_path, uint32_t fas_times);
void read_png_rgba8(const std::string& path, uint32_t* width, uint32_t* height, std::vector<uint32_t>* texels);
void decode_png_rgba8(const std::vector<uint8_t>& bytes, const std::string& label, uint32_t* width, uint32_t* height, std::vector<uint32_t>* texels);   // PNG or JPEG (by content)
void decode_jpeg_rgba8(const std::vector<uint8_t>& bytes, const std::string& label, uint32_t* width, uint32_t* height, std::vector<uint32_t>* texels);
void encode_jpeg_rgb8(const uint8_t* rgb, uint32_t w, uint32_t h, int quality, std::vector<uint8_t>* out);

// exr_piz.cpp: one PIZ-compressed block of an OpenEXR scanline file -> the bytes of the uncompressed block
void exr_piz_decode(const uint8_t* src, size_t size, const std::vector<int>& words_per_pixel, int64_t width, int64_t lines, uint8_t* raw, size_t raw_bytes);

}  // namespace spt_host

// The kernels of spt_scene_deform on a scene of the large-scene form (inst_deform.hip defines them, spt_hip.hip launches them):
// one mesh's triangles rewritten in the traversal blob, then its compressed 4-wide BLAS nodes refitted level by level over the
// topology the creation built.  A launch covers one mesh and one height; stream order is the only synchronisation.
#pragma once
#include <hip/hip_runtime.h>

#include "scene_refit.h"

#include "../../../include/spt_mesh_assemble.h"

// One mesh of one spt_scene_deform_vertices call on a large scene, as the kernels of inst_assemble.hip see it: the registration's
// device arrays and the call's vertices (m), the vertex frames between the two launches, and the scene's ABI-order triangle arrays
struct AssembleMesh {
    spt_ma_mesh m;
    float* tan;               // 3 floats per vertex, written by k_vertex_frames, read by k_assemble_tris
    float* bit;
    float4* tri_pos;          // 3 float4 per triangle
    float4* tri_attr;         // 9 float4 per triangle
    uint32_t tri_first;       // the mesh's first triangle in them
    uint32_t n_tris;          // their length
};

// one thread per vertex: the tangent and bitangent of the vertex from the faces that name it, in table order (spt_mesh_assemble.h)
__global__ void k_vertex_frames(AssembleMesh a);
// one thread per triangle k of the mesh's range: the two records of face face_of_tri[k] into tri_pos / tri_attr[tri_first + k]
__global__ void k_assemble_tris(AssembleMesh a);

constexpr uint8_t kRefitUnknown = 255;   // a node whose height is not known yet (k_refit_heights)

// One mesh of one spt_scene_deform call, as its kernels see it
struct DeformMesh {
    float4* geo;              // the traversal blob
    const float4* tri_pos;    // the scene's triangles in ABI order, 3 float4 each (the call's copies land here first)
    RefitBox* raw;            // raw bounds per BLAS node (index: node behind o_blas)
    uint8_t* height;          // height per BLAS node: 0 = every child is a leaf
    uint32_t o_tri, o_blas, o_mesh;
    uint32_t mesh;
    uint32_t tri_first, tri_count;      // the mesh's triangles: ABI indices and leaf-order slots alike
    uint32_t node_first, node_count;    // its 4-wide nodes
    float root_lo[3], root_hi[3];       // pad(bounds of the whole mesh), made on the host: the box of the mesh record
};

// leaf-order slot -> (p0, p1 - p0, p2 - p0, ABI index) from the new ABI-order record; thread 0 writes the mesh record's box
__global__ void k_deform_tris(DeformMesh m);
// level == kRefitUnknown: marks the nodes of height 0 and the others unknown; else: the unknown nodes whose children are all
// lower than `level` get height `level` (a node of height h is found by exactly the launch of level h)
__global__ void k_refit_heights(DeformMesh m, uint32_t level);
// the nodes of height `level`: raw bounds from the children (leaf: its triangles; node: the level below), then refit_node
__global__ void k_refit_level(DeformMesh m, uint32_t level);

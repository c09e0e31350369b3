/* From vertex arrays to triangle records: the arithmetic of spt_scene_deform_vertices, once, for the host and the device.
 *
 * It restates what the loader does for a trimesh primitive (calc_tangents and face_records of csrc/host/scene.cpp, the
 * reference's TriMesh::calc_tangents and TriMesh::new): the tangent frame of a face from its positions and uvs, the frame of a
 * vertex as the normalised mean of the frames of the corners that name it, summed in increasing (face, corner) order, and the
 * two records of a triangle gathered from its three vertices.  The kernels of inst_assemble.hip, the library's host path for
 * LDS-resident scenes and tests/mesh_assemble_check.cpp compile this one text; the check program proves it equal to the loader's
 * own functions bit for bit.
 *
 * Only f32 + - * / and sqrt, one rounded operation each (-ffp-contract=off -fno-fast-math on both compilers): equal bits on x86-64
 * and gfx950, except for which NaN a 0 / 0 produces (a collapsed face whose uv determinant is not 0 normalises a zero vector).
 */
#ifndef SPT_MESH_ASSEMBLE_H
#define SPT_MESH_ASSEMBLE_H

#include <stddef.h>
#include <stdint.h>

#include "spt_abi.h"
#include "spt_detmath.h"

/* One registered mesh as the assembly reads it.  corner_first has n_vertices + 1 entries; corners[corner_first[v] ..
 * corner_first[v + 1]) are the corners that name vertex v as 3 * face + corner, in increasing order. */
typedef struct spt_ma_mesh {
    uint32_t n_vertices, tri_count;
    const uint32_t* indices;       /* 3 per face */
    const uint32_t* face_of_tri;   /* triangle k of the mesh's range is face face_of_tri[k] */
    const uint32_t* corner_first;
    const uint32_t* corners;
    const float* uv;               /* 2 per vertex */
    const float* positions;        /* 3 per vertex */
    const float* normals;          /* 3 per vertex */
} spt_ma_mesh;

/* hmath.hpp's dot: (x * x + y * y) + z * z */
SPT_HD float spt_ma_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

/* a / sqrt(dot(a, a)): three divisions */
SPT_HD void spt_ma_normalize(const float* a, float* o) {
    const float len = spt_sqrt(spt_ma_dot(a, a));
    o[0] = a[0] / len; o[1] = a[1] / len; o[2] = a[2] / len;
}

/* The frame of one face from its three positions and uvs.  False: det == 0, the face contributes to no vertex. */
SPT_HD bool spt_ma_face_frame(const float* p0, const float* p1, const float* p2, const float* uv0, const float* uv1, const float* uv2,
                              float* tg, float* bt) {
    const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const float e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const float u1x = uv1[0] - uv0[0], u1y = uv1[1] - uv0[1];
    const float u2x = uv2[0] - uv0[0], u2y = uv2[1] - uv0[1];
    float det = u1x * u2y - u1y * u2x;
    if (!(det != 0.0f)) return false;
    det = 1.0f / det;
    float t[3], b[3];
    for (int k = 0; k < 3; ++k) {
        t[k] = (e1[k] * u2y - e2[k] * u1y) * det;
        b[k] = (e2[k] * u1x - e1[k] * u2x) * det;
    }
    spt_ma_normalize(t, tg);
    spt_ma_normalize(b, bt);
    return true;
}

/* The frame of face `face` of a mesh.  False: det == 0, or an index out of range (a registration admits none). */
SPT_HD bool spt_ma_mesh_face_frame(const spt_ma_mesh* m, uint32_t face, float* tg, float* bt) {
    if (face >= m->tri_count) return false;
    const uint32_t i0 = m->indices[3u * face], i1 = m->indices[3u * face + 1u], i2 = m->indices[3u * face + 2u];
    if (i0 >= m->n_vertices || i1 >= m->n_vertices || i2 >= m->n_vertices) return false;
    return spt_ma_face_frame(m->positions + 3u * (size_t)i0, m->positions + 3u * (size_t)i1, m->positions + 3u * (size_t)i2,
                             m->uv + 2u * (size_t)i0, m->uv + 2u * (size_t)i1, m->uv + 2u * (size_t)i2, tg, bt);
}

/* The frame of vertex v: the sums over its corners in table order, starting from 0, then normalize(sum * (1 / (float)deg)).  A
 * vertex without a contributing corner keeps (1, 0, 0) and (0, 1, 0). */
SPT_HD void spt_ma_vertex_frame(const spt_ma_mesh* m, uint32_t v, float* tan_out, float* bit_out) {
    float ts[3] = {0.0f, 0.0f, 0.0f}, bs[3] = {0.0f, 0.0f, 0.0f};
    uint32_t deg = 0;
    const uint32_t first = m->corner_first[v], end = m->corner_first[v + 1u];
    for (uint32_t c = first; c < end && c < 3u * m->tri_count; ++c) {
        float tg[3], bt[3];
        if (!spt_ma_mesh_face_frame(m, m->corners[c] / 3u, tg, bt)) continue;
        for (int k = 0; k < 3; ++k) { ts[k] = ts[k] + tg[k]; bs[k] = bs[k] + bt[k]; }
        ++deg;
    }
    if (deg == 0u) {
        tan_out[0] = 1.0f; tan_out[1] = 0.0f; tan_out[2] = 0.0f;
        bit_out[0] = 0.0f; bit_out[1] = 1.0f; bit_out[2] = 0.0f;
        return;
    }
    const float inv = 1.0f / (float)deg;
    for (int k = 0; k < 3; ++k) { ts[k] = ts[k] * inv; bs[k] = bs[k] * inv; }
    spt_ma_normalize(ts, tan_out);
    spt_ma_normalize(bs, bit_out);
}

/* The two records of triangle k of the mesh's range (face face_of_tri[k]) from the vertex arrays and the vertex frames (3 floats
 * per vertex each).  Pad lanes and pad[3] are zero.  False, nothing written: an index out of range. */
SPT_HD bool spt_ma_triangle(const spt_ma_mesh* m, const float* tan, const float* bit, uint32_t k, spt_tri_pos* tp, spt_tri_attr* ta) {
    if (k >= m->tri_count) return false;
    const uint32_t face = m->face_of_tri[k];
    if (face >= m->tri_count) return false;
    uint32_t vi[3];
    for (int c = 0; c < 3; ++c) {
        vi[c] = m->indices[3u * face + (uint32_t)c];
        if (vi[c] >= m->n_vertices) return false;
    }
    float* pp[3] = {tp->p0, tp->p1, tp->p2};
    for (int c = 0; c < 3; ++c) {
        const size_t v = vi[c];
        for (int j = 0; j < 3; ++j) {
            pp[c][j] = m->positions[3u * v + j];
            ta->n[c][j] = m->normals[3u * v + j];
            ta->t[c][j] = tan[3u * v + j];
            ta->b[c][j] = bit[3u * v + j];
        }
        ta->uv[c][0] = m->uv[2u * v]; ta->uv[c][1] = m->uv[2u * v + 1u];
    }
    tp->pad0 = 0.0f; tp->pad1 = 0.0f; tp->pad2 = 0.0f;
    ta->pad[0] = 0.0f; ta->pad[1] = 0.0f; ta->pad[2] = 0.0f;
    return true;
}

#endif

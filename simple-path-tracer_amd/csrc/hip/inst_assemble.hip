// spt_scene_deform_vertices' kernels (deform_kernels.h): a mesh's triangle records made from its vertex arrays with the loader's
// arithmetic (include/spt_mesh_assemble.h), in front of k_deform_tris and the refit.  One thread per item, plain global loads and
// 16-byte stores, no atomics: a vertex sums the frames of its faces itself, in the table's order, so a face's frame is computed
// once per corner (arithmetic, not bandwidth).  Every index is checked against the mesh's own counts before it is used (the
// header's functions do, for the table and the index arrays; the kernels for their own item and the scene's arrays).
#include "deform_kernels.h"

__global__ void k_vertex_frames(AssembleMesh a) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.m.n_vertices) return;
    float tg[3], bt[3];
    spt_ma_vertex_frame(&a.m, v, tg, bt);
    float* t = a.tan + 3u * (size_t)v;
    float* b = a.bit + 3u * (size_t)v;
    t[0] = tg[0]; t[1] = tg[1]; t[2] = tg[2];
    b[0] = bt[0]; b[1] = bt[1]; b[2] = bt[2];
}

__global__ void k_assemble_tris(AssembleMesh a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.m.tri_count) return;
    if (a.tri_first >= a.n_tris || k >= a.n_tris - a.tri_first) return;   // (never: the host checked the range)
    spt_tri_pos tp;
    spt_tri_attr ta;
    if (!spt_ma_triangle(&a.m, a.tan, a.bit, k, &tp, &ta)) return;   // (never: a registration admits no index out of range)
    float4* dp = a.tri_pos + 3u * ((size_t)a.tri_first + k);
    dp[0] = make_float4(tp.p0[0], tp.p0[1], tp.p0[2], tp.pad0);
    dp[1] = make_float4(tp.p1[0], tp.p1[1], tp.p1[2], tp.pad1);
    dp[2] = make_float4(tp.p2[0], tp.p2[1], tp.p2[2], tp.pad2);
    // the 36 floats of the attribute record in memory order: n[3][3], t[3][3], b[3][3], uv[3][2], pad[3]
    float f[36];
    for (int c = 0; c < 3; ++c)
        for (int j = 0; j < 3; ++j) {
            f[3 * c + j] = ta.n[c][j];
            f[9 + 3 * c + j] = ta.t[c][j];
            f[18 + 3 * c + j] = ta.b[c][j];
        }
    for (int c = 0; c < 3; ++c) { f[27 + 2 * c] = ta.uv[c][0]; f[28 + 2 * c] = ta.uv[c][1]; }
    f[33] = ta.pad[0]; f[34] = ta.pad[1]; f[35] = ta.pad[2];
    float4* da = a.tri_attr + 9u * ((size_t)a.tri_first + k);
#pragma unroll
    for (int q = 0; q < 9; ++q) da[q] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
}

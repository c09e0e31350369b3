// spt_scene_deform's kernels (deform_kernels.h).  They move at most 240 bytes per triangle and 88 per node: one thread per item,
// plain global loads and stores, every index checked against the mesh's own ranges before it is used.
#include "deform_kernels.h"

namespace {

__device__ inline void node_refs(const float4* f, uint32_t refs[4]) {
    refs[0] = __float_as_uint(f[2].z); refs[1] = __float_as_uint(f[2].w);
    refs[2] = __float_as_uint(f[3].x); refs[3] = __float_as_uint(f[3].y);
}

__device__ inline bool own_node(const DeformMesh& m, uint32_t ref) { return ref >= m.node_first && ref - m.node_first < m.node_count; }

}  // namespace

__global__ void k_deform_tris(DeformMesh m) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0u) {
        float4* rec = m.geo + m.o_mesh + 2u * (size_t)m.mesh;   // (the root ref and the flat range in the w lanes stay)
        rec[0].x = m.root_lo[0]; rec[0].y = m.root_lo[1]; rec[0].z = m.root_lo[2];
        rec[1].x = m.root_hi[0]; rec[1].y = m.root_hi[1]; rec[1].z = m.root_hi[2];
    }
    if (k >= m.tri_count) return;
    float4* dst = m.geo + m.o_tri + 3u * ((size_t)m.tri_first + k);
    const uint32_t abi = __float_as_uint(dst[0].w);
    if (abi < m.tri_first || abi - m.tri_first >= m.tri_count) return;   // (never: the creation wrote the index)
    const float4* src = m.tri_pos + 3u * (size_t)abi;
    const float4 p0 = src[0], p1 = src[1], p2 = src[2];
    dst[0] = make_float4(p0.x, p0.y, p0.z, __uint_as_float(abi));
    dst[1] = make_float4(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z, p1.w);
    dst[2] = make_float4(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z, p2.w);
}

__global__ void k_refit_heights(DeformMesh m, uint32_t level) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m.node_count) return;
    const uint32_t node = m.node_first + k;
    if (level != kRefitUnknown && m.height[node] != kRefitUnknown) return;
    const float4* f = m.geo + m.o_blas + 4u * (size_t)node;
    uint32_t refs[4];
    node_refs(f, refs);
    const uint32_t n = min(__float_as_uint(f[0].w) >> 24, 4u);
    bool ready = true;
    for (uint32_t c = 0; c < n; ++c) {
        if (refs[c] & kLeaf) continue;
        // a child found by this very launch reads as unknown or as `level`: not ready either way
        ready = ready && level != kRefitUnknown && own_node(m, refs[c]) && m.height[refs[c]] < level;
    }
    if (level == kRefitUnknown) m.height[node] = ready ? (uint8_t)0 : kRefitUnknown;
    else if (ready) m.height[node] = (uint8_t)level;
}

__global__ void k_refit_level(DeformMesh m, uint32_t level) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m.node_count) return;
    const uint32_t node = m.node_first + k;
    if (m.height[node] != level) return;
    float4* fp = m.geo + m.o_blas + 4u * (size_t)node;
    float4 f[4] = {fp[0], fp[1], fp[2], fp[3]};
    uint32_t refs[4];
    node_refs(f, refs);
    const uint32_t n = min(__float_as_uint(f[0].w) >> 24, 4u);
    RefitBox child[4];
    for (uint32_t c = 0; c < n; ++c) {
        child[c] = refit_empty();
        if (refs[c] & kLeaf) {
            const uint32_t first = refs[c] & 0x07ffffffu, cnt = (refs[c] >> 27) & 15u;
            for (uint32_t t = 0; t < cnt; ++t) {
                const uint32_t slot = first + t;
                if (slot < m.tri_first || slot - m.tri_first >= m.tri_count) continue;
                const uint32_t abi = __float_as_uint(m.geo[m.o_tri + 3u * (size_t)slot].w);
                if (abi < m.tri_first || abi - m.tri_first >= m.tri_count) continue;
                const float4* tp = m.tri_pos + 3u * (size_t)abi;
                const float4 p0 = tp[0], p1 = tp[1], p2 = tp[2];
                const float a[3] = {p0.x, p0.y, p0.z}, b[3] = {p1.x, p1.y, p1.z}, cc[3] = {p2.x, p2.y, p2.z};
                refit_grow_tri(child[c], a, b, cc);
            }
        } else if (own_node(m, refs[c])) {
            child[c] = m.raw[refs[c]];
        }
    }
    m.raw[node] = refit_node(f, child, n);
    fp[0] = f[0];
    fp[1] = f[1];
    fp[2] = f[2];   // (the refs in its z, w lanes as they were read; f[3] holds refs only)
}

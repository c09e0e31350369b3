// spt_occluded and spt_ao (include/spt_abi.h, "visibility along caller rays and at surface points"): any-hit walks without a path.
// Both are built on first_any (first_segment.h), the walker of k_trace_any* for the three geometry forms, and need nothing of the
// wavefront pipeline: no queue, no radiance slot, no bounce.
//
//   k_occluded : one lane per ray of the pass.  The record is loaded as two 16-byte words; the lane stores its byte, or - PACKED - the
//                wave's ballot goes out as one u64 from its first lane.  A pass starts at a multiple of 64 rays, a workgroup at a
//                multiple of 256, so wave w of the pass owns word w.
//   k_ao       : one lane per point of the pass, bake_intake's shape (bake_kernels.h).  The lane resolves its point once per launch
//                (include/spt_bake.h); the sample loop is block-uniform; sum and count stay in registers and leave as two 16-byte
//                words.  A call whose samples are cut into several launches carries sum and count through the out record, so the
//                additions keep their k order; open and bent are made behind the last chunk.
//
// Whole waves: every lane of a wave calls first_any inside wave-uniform code (flat_any and the streaming walker's ballot need
// them).  A lane past `n`, or one whose point failed the predicate, passes want = false.
#pragma once
#include "first_segment.h"
#include "../../../include/spt_bake.h"

struct OccludedJob {
    const float4* rays;   // 2 float4 per ray of the pass: (o, t_min), (d, t_max)
    void* out;            // the pass' bytes, or its u64 words
    uint32_t n;           // rays in the pass
    uint32_t packed;
};

// kWalk: see first_segment.h
template <int kWalk>
SPT_DEV void occluded_lane(const DScene& sc, const OccludedJob& job) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < job.n;
    [[maybe_unused]] uint2 spill_mem[kSpillStack];
    const size_t at = active ? i : 0u;
    const float4 a = job.rays[2u * at], b = job.rays[2u * at + 1u];
    DRay r;
    r.o = mk3(a.x, a.y, a.z); r.t_min = a.w;
    r.d = mk3(b.x, b.y, b.z);
    const bool occ = first_any<kWalk>(sc, r, b.w, active, spill_mem);
    if (job.packed) {
        const uint64_t word = __ballot(active && occ);
        if (active && (threadIdx.x & 63u) == 0u) static_cast<uint64_t*>(job.out)[i >> 6] = word;
    } else if (active) {
        static_cast<uint8_t*>(job.out)[i] = occ ? 1 : 0;
    }
}

struct AoJob {
    const float4* points;    // 1 float4 per SURFACE point of the pass, 2 per WORLD point
    float4* out;             // 2 float4 per point of the pass: (sum, open), (bent, count)
    uint64_t seed;
    float t_max;             // max_distance, or f32::MAX
    float inv;               // 1.0f / (float)S
    uint32_t n;              // points in the pass
    uint32_t reps;           // samples in this chunk
    uint32_t k_first;        // the chunk's first sample: 0 starts from nothing, else from the out record
    uint32_t last;           // the chunk is the call's last: open and bent are made
    uint32_t stream_a;       // first_point + the pass' first point
    uint32_t stream_b;       // first_sample
    uint32_t kind, flip;
};

template <int kWalk>
SPT_DEV void ao_lane(const DScene& sc, const AoJob& job) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < job.n;
    [[maybe_unused]] uint2 spill_mem[kSpillStack];
    float p[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 1.0f, 0.0f};
    bool live = false;
    if (active) {   // (bake_intake's resolution of its point)
        if (job.kind == SPT_BAKE_POINTS_WORLD) {
            const float4 a = job.points[2u * (size_t)i], b = job.points[2u * (size_t)i + 1u];
            spt_bake_world_point wp;
            wp.p[0] = a.x; wp.p[1] = a.y; wp.p[2] = a.z; wp.pad0 = 0.0f;
            wp.n[0] = b.x; wp.n[1] = b.y; wp.n[2] = b.z; wp.pad1 = 0.0f;
            live = spt_bake_world_ok(&wp);
            if (live) { p[0] = wp.p[0]; p[1] = wp.p[1]; p[2] = wp.p[2]; n[0] = wp.n[0]; n[1] = wp.n[1]; n[2] = wp.n[2]; }
        } else {
            const float4 a = job.points[i];
            spt_bake_point pt;
            pt.instance = __float_as_uint(a.x); pt.prim = __float_as_uint(a.y); pt.v = a.z; pt.w = a.w;
            const spt_instance* const inst = reinterpret_cast<const spt_instance*>(sc.instances);
            live = spt_bake_point_ok(&pt, sc.n_instances, &inst->prim_type, (uint32_t)(sizeof(spt_instance) / sizeof(uint32_t)), sc.n_meshes,
                                     reinterpret_cast<const spt_mesh*>(sc.meshes));
            if (live)
                spt_bake_resolve(&pt, inst + pt.instance, reinterpret_cast<const spt_tri_pos*>(sc.tri_pos) + pt.prim,
                                 reinterpret_cast<const spt_tri_attr*>(sc.tri_attr) + pt.prim, p, n);
        }
        if (live && job.flip) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    }
    const f3 origin = mk3(p[0], p[1], p[2]);

    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    uint32_t count = 0u;
    if (live && job.k_first != 0u) {   // what the earlier chunks left
        const float4 s = job.out[2u * (size_t)i], c = job.out[2u * (size_t)i + 1u];
        sum = mk3(s.x, s.y, s.z);
        count = __float_as_uint(c.w);
    }

    float tg[3], bt[3];
    spt_bake_frame(n, tg, bt);
    const uint32_t sa = job.stream_a + i;
    for (uint32_t k = 0; k < job.reps; ++k) {   // (block-uniform: every lane walks the same samples)
        const uint32_t sb = job.stream_b + job.k_first + k;
        float d[3], t_min;
        spt_bake_sample(job.seed, sa, sb, n, tg, bt, d, &t_min);
        DRay ray;
        ray.o = origin;
        ray.d = mk3(d[0], d[1], d[2]);
        ray.t_min = t_min;
        const bool occ = first_any<kWalk>(sc, ray, job.t_max, live, spill_mem);
        if (live && !occ) {
            sum = sum + ray.d;
            ++count;
        }
    }
    if (!active) return;

    float4 w0, w1;
    if (!live) {
        const float q = __uint_as_float(SPT_BAKE_NAN_BITS);
        w0 = make_float4(q, q, q, q);
        w1 = make_float4(q, q, q, __uint_as_float(0xffffffffu));
    } else {
        float open = 0.0f, bent[3] = {0.0f, 0.0f, 0.0f};
        if (job.last) {
            open = (float)count * job.inv;
            if (count > 0u && !(sum.x == 0.0f && sum.y == 0.0f && sum.z == 0.0f)) spt_cm_normalize(sum.x, sum.y, sum.z, bent);
        }
        w0 = make_float4(sum.x, sum.y, sum.z, open);
        w1 = make_float4(bent[0], bent[1], bent[2], __uint_as_float(count));
    }
    job.out[2u * (size_t)i] = w0;
    job.out[2u * (size_t)i + 1u] = w1;
}

// geometry in LDS or in memory
template <bool kLds>
__global__ void __launch_bounds__(256) k_occluded(DScene sc, OccludedJob job) {
    stage_geometry<kLds>(sc);
    occluded_lane<kLds ? 0 : 1>(sc, job);
}
template <bool kLds>
__global__ void __launch_bounds__(256) k_ao(DScene sc, AoJob job) {
    stage_geometry<kLds>(sc);
    ao_lane<kLds ? 0 : 1>(sc, job);
}
// the streaming walker (scenes that do not fit LDS)
__global__ void __launch_bounds__(256) k_occluded_stream(DScene sc, OccludedJob job);
__global__ void __launch_bounds__(256) k_ao_stream(DScene sc, AoJob job);

#if defined(SPT_INSTANTIATE_GROUP_VISIBILITY)
__global__ void __launch_bounds__(256) k_occluded_stream(DScene sc, OccludedJob job) { occluded_lane<2>(sc, job); }
__global__ void __launch_bounds__(256) k_ao_stream(DScene sc, AoJob job) { ao_lane<2>(sc, job); }
template __global__ void k_occluded<true>(DScene, OccludedJob);
template __global__ void k_occluded<false>(DScene, OccludedJob);
template __global__ void k_ao<true>(DScene, AoJob);
template __global__ void k_ao<false>(DScene, AoJob);
#else
extern template __global__ void k_occluded<true>(DScene, OccludedJob);
extern template __global__ void k_occluded<false>(DScene, OccludedJob);
extern template __global__ void k_ao<true>(DScene, AoJob);
extern template __global__ void k_ao<false>(DScene, AoJob);
#endif

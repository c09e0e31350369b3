// spt_bake (include/spt_abi.h, "irradiance at surface points"): the front and the back end that put gather rays made on the device
// through the wavefront pipeline of kernels.h.
//
//   intake : one lane per point of the pass.  The lane resolves its point once (include/spt_bake.h) through the global instance and
//            triangle records, as instance_sample reads them.  In the chunk with k_first == 0 it sums the unoccluded delta lights
//            into D (first_any, first_segment.h), and stores D and the point's validity in planes of their own.  Per sample of the
//            chunk it then makes the gather ray, traces its first segment and files the path at slot k * n + i (first_closest,
//            first_file).  The ray and its hit differ per k, so the trace sits inside the sample loop; the loop is wave-uniform.
//   bounces: the loop of spt_radiance.
//   finish : k_ray_finish plus D: acc += x(i, k) in k order, behind the last chunk acc * (1 / S), then D + acc.  A point that failed
//            the predicate gets the quiet NaN SPT_BAKE_NAN_BITS and has indexed nothing.
#pragma once
#include "first_segment.h"
#include "../../../include/spt_bake.h"

static_assert(kTMinEps == SPT_BAKE_T_EPS, "the gather ray's epsilon is the integrator's");

struct BakeJob {
    const float4* points;    // 1 float4 per SURFACE point of the pass, 2 per WORLD point
    float* rgb_out;          // 3 floats per point of the pass (k_bake_finish)
    float* d_planes;         // 4 planes of `n` floats: D.x, D.y, D.z, valid (1 or 0)
    uint64_t seed;
    uint32_t n;              // points in the pass
    uint32_t reps;           // samples in this chunk
    uint32_t k_first;        // the chunk's first sample
    uint32_t stream_a;       // first_point + the pass' first point
    uint32_t stream_b;       // first_sample
    uint32_t kind, flip;
};

// kWalk: see first_segment.h
template <int kWalk>
SPT_DEV void bake_intake(const DScene& sc, const RenderCtx& rc, const BakeJob& job) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < job.n;
    [[maybe_unused]] uint2 spill_mem[kSpillStack];
    float p[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 1.0f, 0.0f};
    bool live = false;
    if (active) {
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

    if (job.k_first == 0u) {   // D, once per point
        f3 D = mk3(0.0f, 0.0f, 0.0f);
        for (uint32_t l = 0; l < sc.n_lights; ++l) {   // (wave-uniform)
            float dir[3] = {0.0f, 1.0f, 0.0f}, li[3] = {0.0f, 0.0f, 0.0f}, t_min = kTMinEps, t_max = 0.0f;
            const bool want = live && spt_bake_delta(sc.lights + l, p, n, dir, li, &t_min, &t_max);
            if (__ballot(want) == 0ull) continue;
            DRay sr;
            sr.o = origin; sr.d = mk3(dir[0], dir[1], dir[2]); sr.t_min = t_min;
            const bool occ = first_any<kWalk>(sc, sr, t_max, want, spill_mem);
            if (want && !occ) D = D + mk3(li[0], li[1], li[2]);
        }
        if (active) {
            job.d_planes[i] = D.x;
            job.d_planes[(size_t)job.n + i] = D.y;
            job.d_planes[2u * (size_t)job.n + i] = D.z;
            job.d_planes[3u * (size_t)job.n + i] = live ? 1.0f : 0.0f;
        }
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
        const DHit h = first_closest<kWalk>(sc, ray, live, spill_mem);
        first_file<kWalk>(sc, rc, ray, h, active, live, k * job.n + i, job.reps, k, [&] {
            DRng rng;
            rng.s = spt_rng_seed(job.seed, sa, sb);
            return rng;
        });
    }
}

// geometry in LDS or in memory
template <bool kLds>
__global__ void __launch_bounds__(256) k_bake_intake(DScene sc, RenderCtx rc, BakeJob job) {
    stage_geometry<kLds>(sc);
    bake_intake<kLds ? 0 : 1>(sc, rc, job);
}
// the streaming walker (scenes that do not fit LDS)
__global__ void __launch_bounds__(256) k_bake_intake_stream(DScene sc, RenderCtx rc, BakeJob job);

// out_i = D + ((0 + x(i, 0)) + x(i, 1) + ...) * inv: the chunk's samples in k order onto what the earlier chunks left in rgb_out
// (`first`: nothing, start from 0), times 1 / S and plus D behind the last one (`last`)
__global__ void __launch_bounds__(256) k_bake_finish(RenderCtx rc, BakeJob job, uint32_t first, uint32_t last, float inv);

#if defined(SPT_INSTANTIATE_GROUP_BAKE)
__global__ void __launch_bounds__(256) k_bake_intake_stream(DScene sc, RenderCtx rc, BakeJob job) { bake_intake<2>(sc, rc, job); }

__global__ void __launch_bounds__(256) k_bake_finish(RenderCtx rc, BakeJob job, uint32_t first, uint32_t last, float inv) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= job.n) return;
    float* const out = job.rgb_out + 3u * (size_t)i;
    if (job.d_planes[3u * (size_t)job.n + i] == 0.0f) {
        if (last) { out[0] = __uint_as_float(SPT_BAKE_NAN_BITS); out[1] = __uint_as_float(SPT_BAKE_NAN_BITS); out[2] = __uint_as_float(SPT_BAKE_NAN_BITS); }
        return;
    }
    f3 acc = first ? mk3(0.0f, 0.0f, 0.0f) : mk3(out[0], out[1], out[2]);
    const size_t plane = rc.rad_plane;
    for (uint32_t k = 0; k < job.reps; ++k) {
        const size_t s = (size_t)k * job.n + i;
        acc = acc + mk3(rc.rad[s], rc.rad[plane + s], rc.rad[2 * plane + s]);
    }
    if (last) acc = mk3(job.d_planes[i], job.d_planes[(size_t)job.n + i], job.d_planes[2u * (size_t)job.n + i]) + acc * inv;
    out[0] = acc.x; out[1] = acc.y; out[2] = acc.z;
}
template __global__ void k_bake_intake<true>(DScene, RenderCtx, BakeJob);
template __global__ void k_bake_intake<false>(DScene, RenderCtx, BakeJob);
#else
extern template __global__ void k_bake_intake<true>(DScene, RenderCtx, BakeJob);
extern template __global__ void k_bake_intake<false>(DScene, RenderCtx, BakeJob);
#endif

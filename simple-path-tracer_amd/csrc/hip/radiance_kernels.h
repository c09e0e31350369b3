// spt_radiance (include/spt_abi.h): the front and the back end that put caller rays through the wavefront pipeline of kernels.h.
//
//   intake : one lane per ray of the pass.  It loads the 48-byte record (three 16-byte loads), traces the first segment
//            (first_segment.h), writes the hit out, and files one path per repetition k of the chunk at slot k * n + i, so the finish
//            kernel's loads are coalesced and a path's ray is slot % n.  The ray and its hit are the same for every k; the paths
//            differ in their RNG stream (stream_b + k).
//   bounces: the loop of trace_window from bounce 0 with the non-first shade instances (k_shade<., kFirst = false> shades a vertex
//            from its 72-byte record whatever made it), the bounce-0 launch of a textured scene with auxiliary rays being the
//            kAux instance.
//   finish : acc += x(i, k) in k order per ray, then acc * (1 / S).
#pragma once
#include "first_segment.h"

struct RayJob {
    const float4* rays;      // 3 float4 per ray of the pass (spt_path_ray)
    spt_hit* hits_out;       // per ray of the pass; null: not asked for (or written by an earlier chunk of repetitions)
    float* rgb_out;          // 3 floats per ray of the pass (k_ray_finish)
    uint64_t seed;
    uint32_t n;              // rays in the pass
    uint32_t reps;           // repetitions in this chunk
    uint32_t k_first;        // the chunk's first repetition
    uint32_t rng_skip;
};

// kWalk: see first_segment.h
template <int kWalk>
SPT_DEV void ray_intake(const DScene& sc, const RenderCtx& rc, const RayJob& job) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < job.n;
    [[maybe_unused]] uint2 spill_mem[kSpillStack];
    const size_t at = 3u * (size_t)(active ? i : 0u);
    const float4 a = job.rays[at], b = job.rays[at + 1u], c = job.rays[at + 2u];
    DRay ray;
    ray.o = mk3(a); ray.t_min = a.w;
    ray.d = mk3(b);
    const uint32_t stream_a = __float_as_uint(b.w), stream_b = __float_as_uint(c.x);
    const DHit h = first_closest<kWalk>(sc, ray, active, spill_mem);
    if (active && job.hits_out != nullptr) {
        const bool hit = h.inst >= 0;
        spt_hit out;
        out.t = hit ? h.t : SPT_F32_MAX;
        out.instance = h.inst;
        out.prim = hit ? h.prim : -1;
        out.v = hit ? h.v : 0.0f;
        out.w = hit ? h.w : 0.0f;
        job.hits_out[i] = out;
    }
    const f3 miss = first_miss(sc, ray, active && h.inst < 0);
    for (uint32_t k = 0; k < job.reps; ++k)   // (block-uniform)
        first_file_as<kWalk>(sc, rc, ray, h, miss, active, active, k * job.n + i, job.reps, k, [&] {
            DRng rng;
            rng.s = spt_rng_seed(job.seed, stream_a, stream_b + job.k_first + k);
            for (uint32_t j = 0; j < job.rng_skip; ++j) (void)rng.next();
            return rng;
        });
}

// geometry in LDS or in memory
template <bool kLds>
__global__ void __launch_bounds__(256) k_ray_intake(DScene sc, RenderCtx rc, RayJob job) {
    stage_geometry<kLds>(sc);
    ray_intake<kLds ? 0 : 1>(sc, rc, job);
}
// the streaming walker (scenes that do not fit LDS)
__global__ void __launch_bounds__(256) k_ray_intake_stream(DScene sc, RenderCtx rc, RayJob job) { ray_intake<2>(sc, rc, job); }

// out_i = ((0 + x(i, 0)) + x(i, 1) + ...) * inv: the chunk's repetitions in k order onto what the earlier chunks left in rgb_out
// (`first`: nothing, start from 0), times 1 / S behind the last one (`last`)
__global__ void __launch_bounds__(256) k_ray_finish(RenderCtx rc, RayJob job, uint32_t first, uint32_t last, float inv) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= job.n) return;
    float* const out = job.rgb_out + 3u * (size_t)i;
    f3 acc = first ? mk3(0.0f, 0.0f, 0.0f) : mk3(out[0], out[1], out[2]);
    const size_t plane = rc.rad_plane;
    for (uint32_t k = 0; k < job.reps; ++k) {
        const size_t s = (size_t)k * job.n + i;
        acc = acc + mk3(rc.rad[s], rc.rad[plane + s], rc.rad[2 * plane + s]);
    }
    if (last) acc = acc * inv;
    out[0] = acc.x; out[1] = acc.y; out[2] = acc.z;
}

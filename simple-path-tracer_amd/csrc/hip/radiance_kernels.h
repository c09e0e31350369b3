// spt_radiance (include/spt_abi.h): the front and the back end that put caller rays through the wavefront pipeline of kernels.h.
//
//   intake : one lane per ray of the pass.  It loads the 48-byte record (three 16-byte loads), traces the first segment as
//            k_trace_closest* do, writes the hit out, and per repetition k either writes the path's whole result - a miss: the
//            environment term of depth 0, or 0 - into the path's radiance slot, or zeroes the slot and appends a full path record
//            (store_path) with its hit to the hit queue of bounce 0.
//   bounces: the loop of trace_window from bounce 0 with the non-first shade instances (k_shade<., kFirst = false> shades a vertex
//            from its 72-byte record whatever made it), the bounce-0 launch of a textured scene with auxiliary rays being the
//            kAux instance.  They ADD to the slots, which is why the intake zeroes them.
//   finish : acc += x(i, k) in k order per ray, then acc * (1 / S).
//
// Slots: path (ray i of the pass, repetition k of the chunk) owns slot k * n + i of the three planes, so the finish kernel's loads are
// coalesced and a path's ray is slot % n.  Queue shards: workgroup g appends to shard g % kShards only, (lane, repetition) pairs are
// distinct paths, so a shard receives at most ceil(ceil(n / 256) / kShards) * 256 * reps records whatever the rays hit; the later
// generations of a shard are subsets of its first.
#pragma once
#include "kernels.h"

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

// What a lane does with its ray once the first segment is traced.  Every lane of the wave calls it (`active`: the lane has a ray).
template <bool kLds>
SPT_DEV void ray_intake_finish(const DScene& sc, const RenderCtx& rc, const RayJob& job, uint32_t i, bool active, const DRay& ray, uint32_t stream_a,
                               uint32_t stream_b, const DHit& h) {
    const bool hit = active && h.inst >= 0;
    if (active && job.hits_out != nullptr) {
        spt_hit out;
        out.t = hit ? h.t : SPT_F32_MAX;
        out.instance = h.inst;
        out.prim = hit ? h.prim : -1;
        out.v = hit ? h.v : 0.0f;
        out.w = hit ? h.w : 0.0f;
        job.hits_out[i] = out;
    }
    f3 miss = mk3(0.0f, 0.0f, 0.0f);
    if (active && !hit && sc.env_w != 0u) {  // pt.rs:98-110 at depth 0: weight 1
        f3 env;
        float env_pdf;
        env_strength_pdf(sc, ray.d, &env, &env_pdf);
        miss = mk3(0, 0, 0) + (gray(1.0f) * env) * 1.0f;
    }
    const uint32_t shard = blockIdx.x % kShards;
    const uint32_t qbase = shard * rc.shard_cap;
    for (uint32_t k = 0; k < job.reps; ++k) {
        if (active) rad_store(rc, k * job.n + i, miss);   // (a hit: the 0 the shade stages add to)
        const uint32_t slot = rc.n_classes > 1u ? hit_push<kLds>(sc, rc, hit, h.inst, 0u, shard) : qbase + wave_push(hit, q_count(rc.counts, 0, Q_HIT, shard));
        if (hit) {
            // class queues: the hit sits in its class' sub-queue, the record (as after k_extend) at an index of its own inside the shard
            const uint32_t rec = rc.n_classes > 1u ? qbase + ((blockIdx.x / kShards) * blockDim.x + threadIdx.x) * job.reps + k : slot;
            DRng rng;
            rng.s = spt_rng_seed(job.seed, stream_a, stream_b + job.k_first + k);
            for (uint32_t j = 0; j < job.rng_skip; ++j) (void)rng.next();
            store_path(rc.qa, rec, ray, 0.0f, gray(1.0f), k * job.n + i, mk3(0, 0, 0), pack_meta(0u, -1), rng);
            rc.hits.t_v_w_prim[slot] = make_float4(h.t, h.v, h.w, __int_as_float(h.prim));
            rc.hits.inst_src[slot] = make_uint2((uint32_t)h.inst, rec);
        }
    }
}

SPT_DEV void ray_load(const RayJob& job, uint32_t i, DRay* ray, uint32_t* stream_a, uint32_t* stream_b) {
    const float4 a = job.rays[3u * (size_t)i], b = job.rays[3u * (size_t)i + 1u], c = job.rays[3u * (size_t)i + 2u];
    ray->o = mk3(a); ray->t_min = a.w;
    ray->d = mk3(b);
    *stream_a = __float_as_uint(b.w);
    *stream_b = __float_as_uint(c.x);
}

// geometry in LDS or in memory: the walkers of k_trace_closest
template <bool kLds>
__global__ void __launch_bounds__(256) k_ray_intake(DScene sc, RenderCtx rc, RayJob job) {
    stage_geometry<kLds>(sc);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < job.n;
    DRay ray;
    uint32_t sa, sb;
    ray_load(job, active ? i : 0u, &ray, &sa, &sb);
    DHit h;
    h.inst = -1; h.t = SPT_F32_MAX; h.prim = -1; h.v = 0.0f; h.w = 0.0f;
    if (kLds && sc.flat) h = flat_closest(sc, ray, SPT_F32_MAX, active);   // (whole waves, see flat.h)
    else if (active) h = trace_closest<kLds>(sc, ray, SPT_F32_MAX);
    ray_intake_finish<kLds>(sc, rc, job, i, active, ray, sa, sb, h);
}

// the streaming walker (scenes that do not fit LDS): one ray per lane, no refill, as k_trace_closest_stream
__global__ void __launch_bounds__(256) k_ray_intake_stream(DScene sc, RenderCtx rc, RayJob job) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < job.n;
    uint2 spill_mem[kSpillStack];
    SWalker<true, false> wk;
    wk.done = true;
    wk.cur = kNoRef;
    wk.h.inst = -1; wk.h.t = SPT_F32_MAX; wk.h.prim = -1; wk.h.v = 0.0f; wk.h.w = 0.0f;
    DRay ray;
    uint32_t sa, sb;
    ray_load(job, active ? i : 0u, &ray, &sa, &sb);
    if (active) wk.begin(sc, ray, SPT_F32_MAX);
    for (uint32_t guard = 0; guard < (1u << 20) && __ballot(!wk.done) != 0ull; ++guard) wk.run(sc, 8u, spill_mem);
    ray_intake_finish<false>(sc, rc, job, i, active, ray, sa, sb, wk.h);
}

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

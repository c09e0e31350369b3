// The first segment of a path that no pinhole k_primary made: what k_ray_intake* (radiance_kernels.h), k_bake_intake* (bake_kernels.h),
// k_probe_intake* (probe_kernels.h) and k_primary_cam (camera_kernels.h) do between making a ray and the bounce loop of trace_window.
// Each of them brings its ray source and its finish kernel; the walkers and the filing of the path are here, once.
//
// kWalk: 0 geometry in LDS (the flat layout included), 1 geometry from memory, 2 the streaming walker (scenes that do not fit LDS).
// Every lane of a wave calls these functions inside wave-uniform loops: flat_closest / flat_any, the streaming walker's ballot and
// the queue pushes need whole waves.  A lane without a ray says so (`live`, `want`, `traced`) and gets "no hit".
//
// Slots: a path owns one radiance slot `ri` of the three planes (rc.rad, rc.rad_plane apart).  The first segment writes the path's
// whole result there when it misses (the environment term of depth 0, or 0) and 0 when it hits: the shade stages ADD to the slot.
// Queue shards: workgroup g appends to shard g % kShards only, and a lane files at most `stride` paths per launch, so a shard
// receives at most ceil(G / kShards) * 256 * stride records (G workgroups), which is what the host sizes it for (ItemRun::cut,
// cam_chunks); the later generations of a shard are subsets of its first.  With class queues the hit sits in its class' sub-queue
// and the path record (as after k_extend) at an index of its own inside the shard: (workgroup of the shard, lane, index < stride).
#pragma once
#include "kernels.h"

// the closest hit of `ray`, as k_trace_closest* find it
template <int kWalk>
SPT_DEV DHit first_closest(const DScene& sc, const DRay& ray, bool live, [[maybe_unused]] uint2* spill_mem) {
    DHit h;
    h.inst = -1; h.t = SPT_F32_MAX; h.prim = -1; h.v = 0.0f; h.w = 0.0f;
    if constexpr (kWalk == 2) {
        SWalker<true, false> wk;
        wk.done = true;
        wk.cur = kNoRef;
        wk.h = h;
        if (live) wk.begin(sc, ray, SPT_F32_MAX);
        for (uint32_t guard = 0; guard < (1u << 20) && __ballot(!wk.done) != 0ull; ++guard) wk.run(sc, 8u, spill_mem);
        h = wk.h;
    } else {
        constexpr bool kLds = kWalk == 0;
        if (kLds && sc.flat) h = flat_closest(sc, ray, SPT_F32_MAX, live);   // (whole waves, see flat.h)
        else if (live) h = trace_closest<kLds>(sc, ray, SPT_F32_MAX);
    }
    return h;
}

// whether anything lies on `ray` before t_max, as k_trace_any* find it
template <int kWalk>
SPT_DEV bool first_any(const DScene& sc, const DRay& ray, float t_max, bool want, [[maybe_unused]] uint2* spill_mem) {
    bool occ = false;
    if constexpr (kWalk == 2) {
        SWalker<false, false> wk;
        wk.done = true;
        wk.cur = kNoRef;
        wk.h.inst = -1; wk.h.t = SPT_F32_MAX; wk.h.prim = -1; wk.h.v = 0.0f; wk.h.w = 0.0f;
        if (want) wk.begin(sc, ray, t_max);
        for (uint32_t guard = 0; guard < (1u << 20) && __ballot(!wk.done) != 0ull; ++guard) wk.run(sc, 8u, spill_mem);
        occ = wk.h.inst >= 0;
    } else {
        constexpr bool kLds = kWalk == 0;
        if (kLds && sc.flat) occ = flat_any(sc, ray, t_max, want);   // (whole waves, see flat.h)
        else if (want) occ = trace_any<kLds>(sc, ray, t_max);
    }
    return occ;
}

// what a traced first segment that hit nothing contributes: the environment term of depth 0, or 0
SPT_DEV f3 first_miss(const DScene& sc, const DRay& ray, bool missed) {
    f3 miss = mk3(0.0f, 0.0f, 0.0f);
    if (missed && sc.env_w != 0u) {  // pt.rs:98-110 at depth 0: weight 1
        f3 env;
        float env_pdf;
        env_strength_pdf(sc, ray.d, &env, &env_pdf);
        miss = mk3(0, 0, 0) + (gray(1.0f) * env) * 1.0f;
    }
    return miss;
}

// Files the path of slot `ri`: `miss` (a hit: the 0 the shade stages add to) into the slot when the lane `stores` it, and on a hit
// (`traced`: the lane had a ray) the full path record - throughput 1, last_pdf 0, depth 0, the RNG that `make_rng` yields, which is
// called on a hit only - with its hit record to the hit queue of bounce 0.  The lane files path `idx` of its `stride`.
// Returns whether the path goes on: `traced && h.inst >= 0`, the `hit` a caller may have computed for itself (probe_intake does, for
// its segment word, before it knows whether it files at all), since the shard guard below never fails.  That expression is the one
// definition of a hit; first_file repeats it for the miss term.
template <int kWalk, class MakeRng>
SPT_DEV bool first_file_as(const DScene& sc, const RenderCtx& rc, const DRay& ray, const DHit& h, const f3& miss, bool stores, bool traced, uint32_t ri,
                           uint32_t stride, uint32_t idx, MakeRng make_rng) {
    const bool hit = traced && h.inst >= 0;
    const uint32_t shard = blockIdx.x % kShards;
    const uint32_t qbase = shard * rc.shard_cap;
    if (stores) rad_store(rc, ri, miss);
    const uint32_t slot = rc.n_classes > 1u ? hit_push<kWalk == 0>(sc, rc, hit, h.inst, 0u, shard) : qbase + wave_push(hit, q_count(rc.counts, 0, Q_HIT, shard));
    const uint32_t rec = rc.n_classes > 1u ? qbase + ((blockIdx.x / kShards) * blockDim.x + threadIdx.x) * stride + idx : slot;
    const bool filed = hit && rec < qbase + rc.shard_cap;   // (== hit: the host sizes a shard for its workgroups' paths; nothing is ever written past it)
    if (filed) {
        store_path(rc.qa, rec, ray, 0.0f, gray(1.0f), ri, mk3(0, 0, 0), pack_meta(0u, -1), make_rng());
        rc.hits.t_v_w_prim[slot] = make_float4(h.t, h.v, h.w, __int_as_float(h.prim));
        rc.hits.inst_src[slot] = make_uint2((uint32_t)h.inst, rec);
    }
    return filed;
}

// The same with the miss term made here, for a segment that is filed once.  (spt_radiance files one segment `reps` times: it makes
// the term once and calls first_file_as.  `traced && !hit` is written with the `hit` of the filing on purpose: the compiler keeps
// one lane mask for both, where a comparison of its own costs two more spilled SGPRs in every caller.)
template <int kWalk, class MakeRng>
SPT_DEV bool first_file(const DScene& sc, const RenderCtx& rc, const DRay& ray, const DHit& h, bool stores, bool traced, uint32_t ri, uint32_t stride,
                        uint32_t idx, MakeRng make_rng) {
    const bool hit = traced && h.inst >= 0;
    return first_file_as<kWalk>(sc, rc, ray, h, first_miss(sc, ray, traced && !hit), stores, traced, ri, stride, idx, make_rng);
}

// Shadow and extension rays of the fused simple shade kernels against per-origin-triangle candidate sets.
//
// The table (include/spt_origin_cand.h, made on the host once per scene state) holds four 64-bit words per triangle: the slots
// of the staged blob a ray may hit that leaves the triangle upwards / downwards, loose and tight.  A lane picks its word from
// the side its ray leaves on (origin_word), the wave ORs its lanes' words (wave_or64) and every lane tests exactly the union's
// triangles in two scalar loops, as eye_cand_closest (eye.h) does for camera rays: one to_object per instance with set bits, no
// reciprocal, no box test, no stack.  A superset is harmless: the closest hit is the minimum over (t, instance, primitive) and
// any-hit is order-free, and tri_test_edges and the acceptance expressions are those of instance_closest / instance_any
// (trace.h), so the film keeps the walk's bits.  A union of 0 - every ray of a convex body - is no trace at all.
#pragma once
#include "trace.h"
#include "../../../include/spt_origin_cand.h"

static_assert(kTMinEps == (float)SPT_OC_TMIN_EPS, "the table's heights are derived from kTMinEps");

// the extra argument of k_shade<0, ., kFused, ..., OriginCand>: two uint4 per triangle (row = the hit record's triangle id):
// (loose up, loose down), (tight up, tight down), 64 bits each as (low, high)
struct OriginCand {
    const uint4* table;
};

// The word of a ray with z component wz in the shading frame; z_flipped: the frame's z axis is -it.normal (a double-sided
// surface hit from behind).  Below z0 - or NaN - the sign says nothing about the side: both loose words.
SPT_DEV uint64_t origin_word(uint4 loose, uint4 tight, float wz, bool z_flipped) {
    const bool down = (wz < 0.0f) != z_flipped;
    const uint32_t lo = spt_abs(wz) >= SPT_OC_Z0 ? (down ? tight.z : tight.x) : (loose.x | loose.z);
    const uint32_t hi = spt_abs(wz) >= SPT_OC_Z0 ? (down ? tight.w : tight.y) : (loose.y | loose.w);
    return ((uint64_t)hi << 32) | lo;
}

// OR of `w` over the wave (lanes without a ray pass 0; called by whole waves).  One round per distinct contribution: the lanes
// whose word the union already covers drop out, so a wave on one face of a body takes one round, a union of 0 none.
SPT_DEV uint64_t wave_or64(uint64_t w) {
    uint64_t un = 0ull;
    unsigned long long rem = __ballot(w != 0ull);
    while (rem != 0ull) {
        const uint32_t lane = (uint32_t)__builtin_ctzll(rem);
        const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)w, lane), hi = __builtin_amdgcn_readlane((uint32_t)(w >> 32), lane);
        un |= ((uint64_t)hi << 32) | lo;
        rem = __ballot((w & ~un) != 0ull);
    }
    return un;
}

// the slots of `cand` (wave-uniform) inside instance `inst`'s mesh: its first slot and the bits relative to it
SPT_DEV uint64_t origin_mesh_bits(const DScene& sc, uint32_t inst, uint64_t cand, uint32_t* first) {
    const uint32_t I = sc.o_inst + 12u * inst;
    const uint32_t prim_id = __builtin_amdgcn_readfirstlane(__float_as_uint(geo_ld<true>(sc, I + 8u).z));
    const uint32_t range = __builtin_amdgcn_readfirstlane(__float_as_uint(geo_ld<true>(sc, sc.o_mesh + 2u * prim_id + 1u).w));
    const uint32_t count = range >> 16;
    *first = range & 0xffffu;
    return *first < 64u ? (cand >> *first) & (count >= 64u ? ~0ull : ((1ull << count) - 1ull)) : 0ull;
}

// trace_any<true> over the slots of `cand`; lanes without `want` carry no ray and return false
SPT_DEV bool origin_cand_any(const DScene& sc, uint64_t cand, bool want, const DRay& ray, float t_max) {
    bool occluded = false;
    for (uint32_t inst = 0; inst < sc.n_instances; ++inst) {
        uint32_t first;
        uint64_t m = origin_mesh_bits(sc, inst, cand, &first);
        if (m == 0ull) continue;
        if (__ballot(want && !occluded) == 0ull) break;   // every ray of the wave has its answer
        if (want) {
            uint32_t prim_type, prim_id;
            const DRay orr = to_object<true>(sc, inst, ray, &prim_type, &prim_id);
            do {
                const uint32_t i = first + (uint32_t)__builtin_ctzll(m);
                m &= m - 1ull;
                float t, v, w;
                int32_t id;
                if (tri_test_geo<true>(sc, i, orr, &t, &v, &w, &id) && t > orr.t_min && t < t_max) occluded = true;
            } while (m != 0ull);
        }
    }
    return occluded;
}

// trace_closest<true> over the slots of `cand`; lanes without `want` return a miss
SPT_DEV DHit origin_cand_closest(const DScene& sc, uint64_t cand, bool want, const DRay& ray, float t_max) {
    DHit h;
    h.t = t_max; h.inst = -1; h.prim = -1; h.v = 0.0f; h.w = 0.0f;
    for (uint32_t inst = 0; inst < sc.n_instances; ++inst) {
        uint32_t first;
        uint64_t m = origin_mesh_bits(sc, inst, cand, &first);
        if (m == 0ull) continue;
        if (want) {
            uint32_t prim_type, prim_id;
            const DRay orr = to_object<true>(sc, inst, ray, &prim_type, &prim_id);
            do {
                const uint32_t i = first + (uint32_t)__builtin_ctzll(m);
                m &= m - 1ull;
                float t, v, w;
                int32_t id;
                const bool ok = tri_test_geo<true>(sc, i, orr, &t, &v, &w, &id);
                if (ok && t > orr.t_min && (t < h.t || (t == h.t && h.inst >= 0 && key_less((int32_t)inst, id, h)))) {  // triangle.rs:187
                    h.t = t; h.inst = (int32_t)inst; h.prim = id; h.v = v; h.w = w;
                }
            } while (m != 0ull);
        }
    }
    return h;
}

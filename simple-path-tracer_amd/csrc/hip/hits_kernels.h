// spt_hits (include/spt_abi.h, "all hits along caller rays"): the K nearest crossings of each caller segment and the count of all of them.
//
//   k_hits<kLds, kAll> : one lane per ray of the pass; the record is loaded as two 16-byte words, as in k_occluded.  The walk is the
//                nested one of trace.h - walk_tree over the TLAS (or the GROUP loop), per instance to_object and walk_tree over the
//                BLAS: wide nodes in LDS after stage_geometry (kLds), 4-wide nodes from memory otherwise - with a leaf functor of
//                its own.  The flat loops, the streaming walker and first_segment.h are not used: nothing here needs whole waves.
//
// The list.  A lane's sorted list IS its output: max_hits consecutive 32-byte records that no other lane touches, read and written
// as 16-byte words (they stay in L2 while the lane works).  A crossing is inserted when the list is not full or when its key
// (t, instance, prim, backfacing) is below the last record's key; the records behind its place move up by one and the last one
// drops out.  The count, the counters, the cull limit and the last record's key stay in registers; the records past the last crossing
// are filled with the miss record at the end.  No private array is indexed by a run-time value, so the list costs no scratch.
//
// The limit.  walk_tree reads `limit` on every box test.  It is t_max until the list is full - under kAll always, every crossing
// of the segment is counted - and the last record's t afterwards; boxes are culled with the closest-hit rule t0 <= limit, so a
// crossing that ties the K-th key in t is still seen and the result does not depend on the visit order.
#pragma once
#include "trace.h"

struct HitsJob {
    const float4* rays;   // 2 float4 per ray of the pass: (o, t_min), (d, t_max)
    float4* hits;         // 2 float4 per record, max_hits records per ray of the pass (unused when max_hits == 0)
    uint2* counts;        // (total, back) per ray of the pass
    uint32_t n;           // rays in the pass
    uint32_t max_hits;    // K
};

#if !SPT_WITH_BEZIER   // (the patch test yields one root by construction: spt_hits refuses scenes with patches, and libspt_hip_bez.so compiles no k_hits)

// one lane's list and counters
template <bool kAll>
struct HitList {
    float4* rec;                // the lane's records: word 0 (t, instance, prim, flags), word 1 (v, w, 0, 0)
    uint32_t cap;               // K
    uint32_t n = 0;             // records in the list
    uint32_t total = 0, back = 0;
    float limit;                // what the walk culls against
    float t_max;
    // the key of record cap - 1 once the list is full
    float last_t = 0.0f;
    int32_t last_inst = 0, last_prim = 0;
    uint32_t last_back = 0;

    // (t, instance, prim, backfacing) of a crossing below the key in the first word of a record
    static SPT_DEV bool below(float t, int32_t inst, int32_t prim, uint32_t bk, float pt, int32_t pi, int32_t pp, uint32_t pb) {
        if (t != pt) return t < pt;
        if (inst != pi) return inst < pi;
        if (prim != pp) return prim < pp;
        return bk < pb;
    }

    // a crossing: t_min < t < t_max holds
    SPT_DEV void add(float t, int32_t inst, int32_t prim, uint32_t prim_type, uint32_t bk, float v, float w) {
        if (kAll) { ++total; back += bk; }
        if (cap == 0u) return;
        const bool full = n == cap;
        if (full && !below(t, inst, prim, bk, last_t, last_inst, last_prim, last_back)) return;
        if (!kAll) {
            if (full) back -= last_back;   // the last record drops out
            back += bk;
        }
        uint32_t j = full ? cap - 1u : n;  // the place that is free
        while (j > 0u) {
            const float4 p = rec[2u * (j - 1u)];
            if (!below(t, inst, prim, bk, p.x, __float_as_int(p.y), __float_as_int(p.z), __float_as_uint(p.w) & SPT_HIT_BACKFACING)) break;
            rec[2u * j] = p;
            rec[2u * j + 1u] = rec[2u * (j - 1u) + 1u];
            --j;
        }
        rec[2u * j] = make_float4(t, __int_as_float(inst), __int_as_float(prim), __uint_as_float(bk | (prim_type << 8)));
        rec[2u * j + 1u] = make_float4(v, w, 0.0f, 0.0f);
        if (!full) ++n;
        if (n == cap) {
            const float4 p = rec[2u * (cap - 1u)];
            last_t = p.x; last_inst = __float_as_int(p.y); last_prim = __float_as_int(p.z); last_back = __float_as_uint(p.w) & SPT_HIT_BACKFACING;
            if (!kAll) limit = last_t;
        }
    }
};

// the crossings of one instance
template <bool kLds, bool kAll>
SPT_DEV void instance_hits(const DScene& sc, uint32_t inst, const DRay& ray, HitList<kAll>& hl, TStack& st) {
    uint32_t prim_type, prim_id;
    DRay orr = to_object<kLds>(sc, inst, ray, &prim_type, &prim_id);
    if (prim_type == SPT_PRIM_SPHERE) {   // both roots, each judged on its own
        float mn, mx;
        if (sphere_roots(geo_ld<kLds>(sc, sc.o_sph + prim_id), orr, &mn, &mx)) {
            if (orr.t_min < mn && mn < hl.t_max) hl.add(mn, (int32_t)inst, (int32_t)prim_id, prim_type, 0u, 0.0f, 0.0f);
            if (orr.t_min < mx && mx < hl.t_max) hl.add(mx, (int32_t)inst, (int32_t)prim_id, prim_type, SPT_HIT_BACKFACING, 0.0f, 0.0f);
        }
        return;
    }
    if (prim_type != SPT_PRIM_MESH) return;
    const float4 rlo = geo_ld<kLds>(sc, sc.o_mesh + 2u * prim_id), rhi = geo_ld<kLds>(sc, sc.o_mesh + 2u * prim_id + 1u);
    const uint32_t root = __float_as_uint(rlo.w);
    const f3 inv_o = recip3(sc, orr.d);
    if (!root_hit<true>(rlo, rhi, orr.o, inv_o, orr.t_min, hl.limit)) return;
    walk_tree<kLds, true, !kLds, false>(sc, sc.o_blas, root, orr.o, inv_o, orr.t_min, hl.limit, st, nullptr, [&](uint32_t first, uint32_t count) {
        for (uint32_t i = first; i < first + count; ++i) {
            const uint32_t o = sc.o_tri + 3u * i;
            const float4 a = geo_ld_tri<kLds>(sc, o), b = geo_ld_tri<kLds>(sc, o + 1u), c = geo_ld_tri<kLds>(sc, o + 2u);
            float t, v, w;
            const bool ok = tri_test_edges(a, b, c, orr, &t, &v, &w);
            if (ok && t > orr.t_min && t < hl.t_max) {
                const float det = dot(mk3(b), cross(orr.d, mk3(c)));   // tri_test_edges' det: < 0, the ray leaves through the face e1 x e2
                hl.add(t, (int32_t)inst, __float_as_int(a.w), prim_type, det < 0.0f ? (uint32_t)SPT_HIT_BACKFACING : 0u, v, w);
            }
        }
        return false;
    });
}

template <bool kLds, bool kAll>
__global__ void __launch_bounds__(256) k_hits(DScene sc, HitsJob job) {
    stage_geometry<kLds>(sc);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= job.n) return;
    const float4 a = job.rays[2u * (size_t)i], b = job.rays[2u * (size_t)i + 1u];
    DRay r;
    r.o = mk3(a.x, a.y, a.z); r.t_min = a.w;
    r.d = mk3(b.x, b.y, b.z);
    HitList<kAll> hl;
    hl.cap = job.max_hits;
    hl.rec = job.hits + 2u * (size_t)i * job.max_hits;
    hl.t_max = b.w;
    hl.limit = b.w;
    uint2 spill_mem[kSpillStack];
    TStack st;
    st.spill = spill_mem;
    if (sc.aggregate == SPT_AGGREGATE_GROUP) {
        for (uint32_t k = 0; k < sc.n_instances; ++k) instance_hits<kLds, kAll>(sc, k, r, hl, st);
    } else if (sc.n_tlas_nodes > 0) {
        const f3 inv_w = recip3(sc, r.d);
        const float4 tlo = make_float4(sc.tlas_lo[0], sc.tlas_lo[1], sc.tlas_lo[2], 0.0f), thi = make_float4(sc.tlas_hi[0], sc.tlas_hi[1], sc.tlas_hi[2], 0.0f);
        if (root_hit<true>(tlo, thi, r.o, inv_w, r.t_min, hl.limit))
            walk_tree<kLds, true, false, false>(sc, sc.o_tlas, sc.tlas_root, r.o, inv_w, r.t_min, hl.limit, st, nullptr, [&](uint32_t first, uint32_t count) {
                for (uint32_t k = first; k < first + count; ++k) instance_hits<kLds, kAll>(sc, tlas_instance<kLds>(sc, k), r, hl, st);
                return false;
            });
    }
    for (uint32_t j = hl.n; j < hl.cap; ++j) {   // the miss record
        hl.rec[2u * j] = make_float4(SPT_F32_MAX, __int_as_float(-1), __int_as_float(-1), 0.0f);
        hl.rec[2u * j + 1u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    job.counts[i] = kAll ? make_uint2(hl.total, hl.back) : make_uint2(hl.n, hl.back);
}

#if defined(SPT_INSTANTIATE_GROUP_HITS)
template __global__ void k_hits<true, false>(DScene, HitsJob);
template __global__ void k_hits<true, true>(DScene, HitsJob);
template __global__ void k_hits<false, false>(DScene, HitsJob);
template __global__ void k_hits<false, true>(DScene, HitsJob);
#else
extern template __global__ void k_hits<true, false>(DScene, HitsJob);
extern template __global__ void k_hits<true, true>(DScene, HitsJob);
extern template __global__ void k_hits<false, false>(DScene, HitsJob);
extern template __global__ void k_hits<false, true>(DScene, HitsJob);
#endif

#endif   // !SPT_WITH_BEZIER

// spt_probe (include/spt_abi.h, "spherical-harmonic light probes"): the front and the back end that put uniform sphere rays made on
// the device through the wavefront pipeline of kernels.h, and project what the paths return onto nine SH coefficients per probe.
//
//   intake : one lane per probe of the pass.  In the chunk with k_first == 0 it sums the unoccluded delta lights (first_any,
//            first_segment.h), each times the basis of its direction, into D[9][3], and stores D and the probe's validity in planes
//            of their own.  Per sample of the chunk it makes the gather ray from the header (include/spt_probe.h), traces its first
//            segment and files the path at slot k * n + i (first_closest, first_file).  The first segment's t, with the backface
//            bit in its sign, goes to a plane of its own at the same slot (kProbeMiss: no hit).  The loops are wave-uniform.
//   bounces: the loop of spt_radiance.
//   finish : one lane per (coefficient j, probe i), i fastest: the three plane loads per k are coalesced, and a job of few probes
//            and many samples still fills the device nine times better than a lane per probe.  The lane rebuilds d_k from the stream
//            (two draws, one sincos, one sqrt) rather than read nine stored weights per path, and adds x(i, k) * Y_j(d_k) in k order
//            onto what the earlier chunks left in sh_out; behind the last chunk D + acc * w.  The lanes with j == 0 reduce the
//            visibility record; hit and backface counts are carried between chunks as integers in planes of their own.
//
// Stores and the sizes the host computed for them (ProbeJob): the D, validity and carry planes at i < n <= plane_cap (the planes'
// stride); the segment plane at k * n + i < seg_cap; the radiance planes at the same slot < rc.rad_plane (reps * n); the queue
// record at rec < qbase + rc.shard_cap; sh_out / aux_out at i < n of the pass' slice of the caller's (or the staging) array.
#pragma once
#include "first_segment.h"
#include "../../../include/spt_probe.h"

static_assert(kTMinEps == SPT_BAKE_T_EPS, "the gather ray's epsilon is the integrator's");

constexpr uint32_t kProbeMiss = 0xffffffffu;   // segment plane: no hit (a hit is the bits of t > 0, sign set when backfacing)
constexpr uint32_t kProbePlanes = 32u;         // 27 of D, validity, then the carry: hits, backfacing (u32), sum of t, smallest t

struct ProbeJob {
    const float4* points;    // 1 float4 per probe of the pass
    float* sh_out;           // 27 floats per probe of the pass (k_probe_finish)
    float* aux_out;          // 4 floats per probe of the pass, or null
    float* planes;           // kProbePlanes planes of `plane_cap` words
    uint32_t* seg;           // the first segments of the chunk's paths, slot k * n + i, `seg_cap` words
    uint64_t seed;
    uint32_t n;              // probes in the pass
    uint32_t reps;           // samples in this chunk
    uint32_t k_first;        // the chunk's first sample
    uint32_t stream_a;       // first_point + the pass' first probe
    uint32_t stream_b;       // first_sample
    uint32_t plane_cap, seg_cap;
    uint32_t paths;          // 0: max_depth == 0, the segments are traced for the visibility record only and every x is 0
};

// kWalk: see first_segment.h
template <int kWalk>
SPT_DEV void probe_intake(const DScene& sc, const RenderCtx& rc, const ProbeJob& job) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < job.n && i < job.plane_cap;
    [[maybe_unused]] uint2 spill_mem[kSpillStack];
    float p[3] = {0.0f, 0.0f, 0.0f};
    bool live = false;
    if (active) {
        const float4 a = job.points[i];
        spt_probe_point pt;
        pt.p[0] = a.x; pt.p[1] = a.y; pt.p[2] = a.z; pt.pad = 0.0f;
        live = spt_probe_ok(&pt);
        if (live) { p[0] = pt.p[0]; p[1] = pt.p[1]; p[2] = pt.p[2]; }
    }
    const f3 origin = mk3(p[0], p[1], p[2]);
    const size_t cap = job.plane_cap;

    if (job.k_first == 0u) {   // D, once per probe
        float D[SPT_PROBE_SH_WORDS];
#pragma unroll
        for (uint32_t q = 0; q < SPT_PROBE_SH_WORDS; ++q) D[q] = 0.0f;
        for (uint32_t l = 0; l < sc.n_lights; ++l) {   // (wave-uniform)
            float dir[3] = {0.0f, 1.0f, 0.0f}, li[3] = {0.0f, 0.0f, 0.0f}, t_max = 0.0f;
            const bool want = live && spt_probe_delta(sc.lights + l, p, dir, li, &t_max);
            if (__ballot(want) == 0ull) continue;
            DRay sr;
            sr.o = origin; sr.d = mk3(dir[0], dir[1], dir[2]); sr.t_min = SPT_BAKE_T_EPS;
            const bool occ = first_any<kWalk>(sc, sr, t_max, want, spill_mem);
            if (want && !occ) {
#pragma unroll
                for (uint32_t j = 0; j < SPT_PROBE_COEFFS; ++j) {
                    const float Y = spt_probe_basis_j(dir, j);
                    D[3u * j] = D[3u * j] + li[0] * Y;
                    D[3u * j + 1u] = D[3u * j + 1u] + li[1] * Y;
                    D[3u * j + 2u] = D[3u * j + 2u] + li[2] * Y;
                }
            }
        }
        if (active) {
#pragma unroll
            for (uint32_t q = 0; q < SPT_PROBE_SH_WORDS; ++q) job.planes[q * cap + i] = D[q];
            job.planes[27u * cap + i] = live ? 1.0f : 0.0f;
        }
    }

    const uint32_t sa = job.stream_a + i;
    const spt_instance* const inst = reinterpret_cast<const spt_instance*>(sc.instances);
    for (uint32_t k = 0; k < job.reps; ++k) {   // (block-uniform: every lane walks the same samples)
        const uint32_t sb = job.stream_b + job.k_first + k;
        float d[3];
        spt_probe_sample(job.seed, sa, sb, d);
        DRay ray;
        ray.o = origin;
        ray.d = mk3(d[0], d[1], d[2]);
        ray.t_min = SPT_BAKE_T_EPS;
        const DHit h = first_closest<kWalk>(sc, ray, live, spill_mem);
        const bool hit = live && h.inst >= 0;
        const uint32_t ri = k * job.n + i;
        uint32_t seg = kProbeMiss;
        if (hit && (uint32_t)h.inst < sc.n_instances) {
            const bool mesh = inst[h.inst].prim_type == SPT_PRIM_MESH;   // (h.prim indexes the triangle records of a mesh instance only)
            const bool back = mesh && spt_probe_backfacing(inst + h.inst, (uint32_t)h.inst, (uint32_t)h.prim, h.v, h.w,
                                                           reinterpret_cast<const spt_tri_pos*>(sc.tri_pos) + h.prim,
                                                           reinterpret_cast<const spt_tri_attr*>(sc.tri_attr) + h.prim, d);
            seg = (__float_as_uint(h.t) & 0x7fffffffu) | (back ? 0x80000000u : 0u);
        }
        if (active && ri < job.seg_cap) job.seg[ri] = seg;
        if (job.paths == 0u) {   // (job-uniform) max_depth == 0: no path runs, x = 0
            if (active) rad_store(rc, ri, mk3(0.0f, 0.0f, 0.0f));
            continue;
        }
        first_file<kWalk>(sc, rc, ray, h, active, live, ri, job.reps, k, [&] {
            DRng rng;
            rng.s = spt_rng_seed(job.seed, sa, sb);
            return rng;
        });
    }
}

// geometry in LDS or in memory
template <bool kLds>
__global__ void __launch_bounds__(256) k_probe_intake(DScene sc, RenderCtx rc, ProbeJob job) {
    stage_geometry<kLds>(sc);
    probe_intake<kLds ? 0 : 1>(sc, rc, job);
}
// the streaming walker (scenes that do not fit LDS)
__global__ void __launch_bounds__(256) k_probe_intake_stream(DScene sc, RenderCtx rc, ProbeJob job);

// Lane (j, i) = (g / n, g % n): sh[j][c] of probe i.  `first`: start from 0, else from what sh_out holds; `last`: D + acc * w, the
// visibility record, and the NaN words of an invalid probe.  inv = 1 / S.
__global__ void __launch_bounds__(256) k_probe_finish(RenderCtx rc, ProbeJob job, uint32_t first, uint32_t last, float w, float inv);

#if defined(SPT_INSTANTIATE_GROUP_PROBE)
__global__ void __launch_bounds__(256) k_probe_intake_stream(DScene sc, RenderCtx rc, ProbeJob job) { probe_intake<2>(sc, rc, job); }

__global__ void __launch_bounds__(256) k_probe_finish(RenderCtx rc, ProbeJob job, uint32_t first, uint32_t last, float w, float inv) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = g / job.n, i = g - j * job.n;
    if (j >= SPT_PROBE_COEFFS || i >= job.plane_cap) return;
    const size_t cap = job.plane_cap;
    float* const out = job.sh_out + SPT_PROBE_SH_WORDS * (size_t)i + 3u * j;
    float* const aux = job.aux_out != nullptr && j == 0u ? job.aux_out + SPT_PROBE_AUX_WORDS * (size_t)i : nullptr;
    const float nan = __uint_as_float(SPT_BAKE_NAN_BITS);
    if (job.planes[27u * cap + i] == 0.0f) {
        if (last) {
            out[0] = nan; out[1] = nan; out[2] = nan;
            if (aux) { aux[0] = nan; aux[1] = nan; aux[2] = nan; aux[3] = nan; }
        }
        return;
    }
    f3 acc = first ? mk3(0.0f, 0.0f, 0.0f) : mk3(out[0], out[1], out[2]);
    const size_t plane = rc.rad_plane;
    const uint32_t sa = job.stream_a + i;
    uint32_t* const carry_n = reinterpret_cast<uint32_t*>(job.planes + 28u * cap);
    uint32_t* const carry_b = reinterpret_cast<uint32_t*>(job.planes + 29u * cap);
    uint32_t hits = 0u, backs = 0u;
    float t_sum = 0.0f, t_min = SPT_F32_MAX;
    if (aux && !first) { hits = carry_n[i]; backs = carry_b[i]; t_sum = job.planes[30u * cap + i]; t_min = job.planes[31u * cap + i]; }
    for (uint32_t k = 0; k < job.reps; ++k) {
        const size_t s = (size_t)k * job.n + i;
        if (s >= job.seg_cap) break;   // (never: the host sized the planes for reps * n)
        float d[3];
        spt_probe_sample(job.seed, sa, job.stream_b + job.k_first + k, d);
        const float Y = spt_probe_basis_j(d, j);
        acc = mk3(acc.x + rc.rad[s] * Y, acc.y + rc.rad[plane + s] * Y, acc.z + rc.rad[2 * plane + s] * Y);
        if (aux) {
            const uint32_t seg = job.seg[s];
            if (seg != kProbeMiss) {
                const float t = __uint_as_float(seg & 0x7fffffffu);
                hits += 1u;
                backs += seg >> 31;
                t_sum = t_sum + t;
                t_min = t < t_min ? t : t_min;
            }
        }
    }
    if (last) acc = mk3(job.planes[(3u * j) * cap + i] + acc.x * w, job.planes[(3u * j + 1u) * cap + i] + acc.y * w, job.planes[(3u * j + 2u) * cap + i] + acc.z * w);
    out[0] = acc.x; out[1] = acc.y; out[2] = acc.z;
    if (aux) {
        if (last) {
            aux[0] = (float)hits * inv;
            aux[1] = (float)backs * inv;
            aux[2] = hits ? t_sum / (float)hits : 0.0f;
            aux[3] = t_min;
        } else {
            carry_n[i] = hits; carry_b[i] = backs; job.planes[30u * cap + i] = t_sum; job.planes[31u * cap + i] = t_min;
        }
    }
}
template __global__ void k_probe_intake<true>(DScene, RenderCtx, ProbeJob);
template __global__ void k_probe_intake<false>(DScene, RenderCtx, ProbeJob);
#else
extern template __global__ void k_probe_intake<true>(DScene, RenderCtx, ProbeJob);
extern template __global__ void k_probe_intake<false>(DScene, RenderCtx, ProbeJob);
#endif

// spt_gbuffer (include/spt_abi.h, "first-hit surface records"): the stage behind spt_radiance's intake kernels that turns a pass of
// caller rays and their closest hits into spt_gbuffer_rec records.
//
//   intake   : k_ray_intake<kLds> / k_ray_intake_stream (radiance_kernels.h) with reps == 0: they trace the first segments, file no
//              path and write one spt_hit per ray of the pass.
//   k_gbuffer: one lane per ray.  It loads the 48-byte ray record (three 16-byte loads), the 20-byte hit and, on a scene that
//              samples textures and with auxiliary rays given, the 64-byte aux record (four 16-byte loads); rebuilds the hit
//              (reconstruct_hit) and its texture footprint (calc_differential), evaluates the material record at the hit
//              (material_at, one call site) and stores the record as four 16-byte words, so a wave writes 4 KiB contiguous.  A miss
//              lane stores the miss record.  k_shade_albedo (kernels.h) is the same arithmetic on the pinhole's compact records.
//              No LDS, no atomics, no queue: the shading tables come from memory.
//
// Stores: out[4 * i + 0 .. 3] for i < n, n the rays of the pass, `out` the pass' slice of the caller's (or the staging) array.
#pragma once
#include "shading.h"

struct GBufferJob {
    const float4* rays;      // 3 float4 per ray of the pass (spt_path_ray)
    const spt_hit* hits;     // per ray of the pass, as the intake kernel left them
    const float4* aux;       // 4 float4 per ray of the pass (spt_ray_aux), or null: no differentials
    float4* out;             // 4 float4 per ray of the pass (spt_gbuffer_rec)
    uint32_t n;              // rays in the pass
};

// kTex: texcoords, the differentials of the auxiliary rays and the per-hit recipes; kPndf: the glint footprint walk of material_at
template <bool kTex, bool kPndf>
__global__ void __launch_bounds__(256) k_gbuffer(DScene sc, GBufferJob job) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= job.n) return;
    const size_t at = 3u * (size_t)i;
    const float4 a = job.rays[at], b = job.rays[at + 1u];
    const spt_hit hr = job.hits[i];
    DRay ray;
    ray.o = mk3(a); ray.t_min = a.w;
    ray.d = mk3(b);
    float4 w0 = make_float4(0.0f, 0.0f, 0.0f, SPT_F32_MAX), w1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)),
           w2 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)), w3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (hr.instance >= 0) {
        DHit h;
        h.t = hr.t; h.v = hr.v; h.w = hr.w; h.prim = hr.prim; h.inst = hr.instance;
        DInter it = reconstruct_hit<kTex, false>(sc, ray, h);
        if (kTex && job.aux != nullptr) {   // the footprint from the caller's auxiliary rays, as k_shade<., kAux = true>
            const float4* const ar = job.aux + 4u * (size_t)i;
            calc_differential(it, ray, h.t, mk3(ar[0]), mk3(ar[1]), mk3(ar[2]), mk3(ar[3]));
        }
        const spt_surface sf = load_surface<false>(sc, it.surface);
        const DMat mt = material_at<kTex, false, kPndf>(sc, sf.material, it);
        const f3 albedo = mat_albedo(mt);
        uint32_t flags = it.prim_type << 8;
        if (dot(it.normal, ray.d) > 0.0f) flags |= (uint32_t)SPT_GBUF_BACKFACING;
        if (it.light >= 0) flags |= (uint32_t)SPT_GBUF_LIGHT;
        w0 = make_float4(it.position.x, it.position.y, it.position.z, h.t);
        w1 = make_float4(it.normal.x, it.normal.y, it.normal.z, __int_as_float(h.inst));
        w2 = make_float4(albedo.x, albedo.y, albedo.z, __int_as_float(h.prim));
        w3 = make_float4(h.v, h.w, __uint_as_float(it.surface), __uint_as_float(flags));
    }
    float4* const out = job.out + 4u * (size_t)i;
    out[0] = w0; out[1] = w1; out[2] = w2; out[3] = w3;
}

// spt_camera_rays and spt_camera_gbuffer (include/spt_abi.h, "camera rays and first-hit images made on the device"): a plan's camera
// rays written out as records, and first-hit records added into per-pixel sums.
//
// A job's rays are numbered q = (s - first) * n_pixels + pixel, the order of spt_host_camera_rays' arrays; a pass is the n rays from
// q0 = s0 * n_pixels + p0 on (p0 < n_pixels).  The host keeps p0 + n below 2^32 (n_pixels <= 2^31, n < 2^31), so a lane finds its
// sample and pixel with one 32-bit division.
//
//   k_camera_rays           : one lane per ray of the pass.  It makes the pixel offset, the screen point, the lens point and the ray as
//                             k_primary_cam does (camera_kernels.h; include/spt_camera_models.h) and stores the spt_path_ray as three
//                             16-byte words - (o, t_min), (d, stream_a = pixel), (stream_b = plan index, +0, +0, +0) - and, when `aux` is
//                             given, the spt_ray_aux as four, padding words +0.  A wave writes 3 KiB + 4 KiB contiguous.  No LDS, no
//                             atomics, no geometry.
//   k_gbuffer_image         : behind k_camera_rays and spt_radiance's intake kernels with reps == 0 (radiance_kernels.h), which leave
//                             the pass' rays and hits in the workspace.  One lane per PIXEL the pass touches (min(n, n_pixels) lanes):
//                             the lane walks its pixel's rays of the pass, i = lane, lane + n_pixels, ..., which is plan-sample order,
//                             and adds k_gbuffer's albedo, normal and t (gbuffer_kernels.h: the same reconstruct_hit,
//                             calc_differential and material_at) to the pixel's sums.  Passes follow each other on one stream, so every
//                             sum grows in sample order and nothing is atomic.  A miss adds +0 to sums that are never -0: it is skipped.
//   k_gbuffer_image_finish  : one lane per pixel, behind the last pass: the sums times 1 / count, T / K and K / count, stored into
//                             whichever of the four images are asked for.
//
// Sums: two 16-byte words per pixel, (A.x, A.y, A.z, T) and (N.x, N.y, N.z, K as its u32 bits), zeroed before the first pass.
#pragma once
#include "kernels.h"
#include "gbuffer_kernels.h"
#include "../../../include/spt_camera_models.h"

struct CamRaysJob {
    spt_camera_model model;
    spt_cm_plan plan;
    float4* rays;        // 3 float4 per ray of the pass (spt_path_ray)
    float4* aux;         // 4 float4 per ray of the pass (spt_ray_aux), or null
    uint32_t n;          // rays in the pass
    uint32_t p0;         // the pixel of the pass' first ray
    uint32_t s0;         // the plan sample of the pass' first ray
};

// rc: plan_ctx of the whole image (n_pixels = width * height); only its plan constants are read
__global__ void __launch_bounds__(256) k_camera_rays(RenderCtx rc, CamRaysJob job);

struct GBufferImageJob {
    const float4* rays;      // 3 float4 per ray of the pass, as k_camera_rays left them
    const spt_hit* hits;     // per ray of the pass, as the intake kernel left them
    const float4* aux;       // 4 float4 per ray of the pass, or null: no differentials
    float4* sums;            // 2 float4 per pixel of the image
    uint32_t n;              // rays in the pass
    uint32_t p0;             // the pixel of the pass' first ray
    uint32_t n_pixels;
};

// kTex, kPndf: k_gbuffer's
template <bool kTex, bool kPndf>
__global__ void __launch_bounds__(256) k_gbuffer_image(DScene sc, GBufferImageJob job) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= min(job.n, job.n_pixels)) return;
    const uint32_t pixel = (job.p0 + lane) % job.n_pixels;
    float4 s0 = job.sums[2u * (size_t)pixel], s1 = job.sums[2u * (size_t)pixel + 1u];
    uint32_t hits = __float_as_uint(s1.w);
    for (uint64_t i = lane; i < job.n; i += job.n_pixels) {
        const spt_hit hr = job.hits[i];
        if (hr.instance < 0) continue;
        const float4 a = job.rays[3u * i], b = job.rays[3u * i + 1u];
        DRay ray;
        ray.o = mk3(a); ray.t_min = a.w;
        ray.d = mk3(b);
        DHit h;
        h.t = hr.t; h.v = hr.v; h.w = hr.w; h.prim = hr.prim; h.inst = hr.instance;
        DInter it = reconstruct_hit<kTex, false>(sc, ray, h);
        if (kTex && job.aux != nullptr) {
            const float4* const ar = job.aux + 4u * i;
            calc_differential(it, ray, h.t, mk3(ar[0]), mk3(ar[1]), mk3(ar[2]), mk3(ar[3]));
        }
        const spt_surface sf = load_surface<false>(sc, it.surface);
        const DMat mt = material_at<kTex, false, kPndf>(sc, sf.material, it);
        const f3 albedo = mat_albedo(mt);
        s0.x += albedo.x; s0.y += albedo.y; s0.z += albedo.z;
        s1.x += it.normal.x; s1.y += it.normal.y; s1.z += it.normal.z;
        s0.w += h.t;
        ++hits;
    }
    s1.w = __uint_as_float(hits);
    job.sums[2u * (size_t)pixel] = s0;
    job.sums[2u * (size_t)pixel + 1u] = s1;
}

struct GBufferImageOut {
    const float4* sums;      // 2 float4 per pixel
    float* albedo;           // [n_pixels][3], or null
    float* normal;           // [n_pixels][3], or null
    float* depth;            // [n_pixels], or null
    float* coverage;         // [n_pixels], or null
    uint32_t n_pixels;
    float count;             // (float)count
    float inv;               // 1.0f / (float)count
};

__global__ void __launch_bounds__(256) k_gbuffer_image_finish(GBufferImageOut job);

#if defined(SPT_INSTANTIATE_GROUP_CAMERA_DEVICE)
__global__ void __launch_bounds__(256) k_camera_rays(RenderCtx rc, CamRaysJob job) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= job.n) return;
    const uint32_t q = job.p0 + lane;
    const uint32_t s_rel = q / rc.n_pixels;
    const uint32_t pixel = q - s_rel * rc.n_pixels;
    const uint32_t gs = job.s0 + s_rel;
    const uint32_t j = pixel / rc.width, i = pixel - j * rc.width;
    DRng rng;
    rng.s.state = 0ull;
    if (rc.sampler != SPT_SAMPLER_RECURRENCE) rng.s = spt_rng_seed(rc.seed, pixel, gs);   // (the R2 sampler draws nothing)
    float ox, oy, x, y, lx = 0.0f, ly = 0.0f;
    pixel_offset(rc, pixel, gs, rng, &ox, &oy);
    spt_cm_screen(i, j, rc.height, ox, oy, rc.width_inv, rc.height_inv, rc.aspect, &x, &y);
    if (job.model.type == SPT_CAMERA_THIN_LENS) spt_cm_lens_point(rc.seed, pixel, gs, &lx, &ly);
    float o[3], d[3];
    spt_cm_ray(&job.model, &job.plan, x, y, lx, ly, o, d);
    float4* const r = job.rays + 3u * (size_t)lane;
    r[0] = make_float4(o[0], o[1], o[2], SPT_CM_T_MIN);
    r[1] = make_float4(d[0], d[1], d[2], __uint_as_float(pixel));
    r[2] = make_float4(__uint_as_float(gs), 0.0f, 0.0f, 0.0f);
    if (job.aux != nullptr) {   // the same model at (x + aux_dx, y) and (x, y + aux_dy) with the same lens point
        float ao[3], ad[3];
        float4* const ar = job.aux + 4u * (size_t)lane;
        spt_cm_ray(&job.model, &job.plan, x + rc.aux_dx, y, lx, ly, ao, ad);
        ar[0] = make_float4(ao[0], ao[1], ao[2], 0.0f);
        ar[1] = make_float4(ad[0], ad[1], ad[2], 0.0f);
        spt_cm_ray(&job.model, &job.plan, x, y + rc.aux_dy, lx, ly, ao, ad);
        ar[2] = make_float4(ao[0], ao[1], ao[2], 0.0f);
        ar[3] = make_float4(ad[0], ad[1], ad[2], 0.0f);
    }
}

__global__ void __launch_bounds__(256) k_gbuffer_image_finish(GBufferImageOut job) {
    const uint32_t pixel = blockIdx.x * blockDim.x + threadIdx.x;
    if (pixel >= job.n_pixels) return;
    const float4 s0 = job.sums[2u * (size_t)pixel], s1 = job.sums[2u * (size_t)pixel + 1u];
    const uint32_t hits = __float_as_uint(s1.w);
    if (job.albedo != nullptr) {
        float* const out = job.albedo + 3u * (size_t)pixel;
        out[0] = s0.x * job.inv; out[1] = s0.y * job.inv; out[2] = s0.z * job.inv;
    }
    if (job.normal != nullptr) {
        float* const out = job.normal + 3u * (size_t)pixel;
        out[0] = s1.x * job.inv; out[1] = s1.y * job.inv; out[2] = s1.z * job.inv;
    }
    if (job.depth != nullptr) job.depth[pixel] = hits > 0u ? s0.w / (float)hits : 0.0f;
    if (job.coverage != nullptr) job.coverage[pixel] = (float)hits / job.count;
}

template __global__ void k_gbuffer_image<false, false>(DScene, GBufferImageJob);
template __global__ void k_gbuffer_image<true, false>(DScene, GBufferImageJob);
template __global__ void k_gbuffer_image<true, true>(DScene, GBufferImageJob);
#else
extern template __global__ void k_gbuffer_image<false, false>(DScene, GBufferImageJob);
extern template __global__ void k_gbuffer_image<true, false>(DScene, GBufferImageJob);
extern template __global__ void k_gbuffer_image<true, true>(DScene, GBufferImageJob);
#endif

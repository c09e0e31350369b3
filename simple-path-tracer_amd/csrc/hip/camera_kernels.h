// spt_render_camera / spt_film_create_camera (include/spt_abi.h, "camera models"): the primary kernel of a camera model.
//
//   k_primary_cam : one launch per pass.  Blocks are k_primary's 16x16 pixel tiles times sample chunks (blockIdx = tile + n_tiles * chunk),
//                   so the lanes of a wave cover a compact pixel block and the samples of the chunk are the loop.  Per sample a lane makes
//                   its ray in registers (include/spt_camera_models.h; and its two auxiliary rays when the scene samples textures),
//                   traces the first segment and files the path (first_segment.h) with film semantics: slot s * n_pixels + lp, the RNG
//                   seeded from the path stream and advanced past the pixel-offset draws.  No ray record goes through memory.
//   bounces       : the loop of trace_window from bounce 0 with the non-first shade instances (k_shade<., kFirst = false>), as for
//                   spt_radiance; a textured scene's bounce-0 launch is the kAux instance, fed from the records written here per slot.
//   resolve       : every sample of a live pixel owns its slot (first_slot = 0, as after a `collect` pass), so the resolve is the
//                   plain k_resolve / k_resolve_buckets<false> (rc.slot_bits stays null).  A pixel an adaptive film has retired traces
//                   nothing and has first_slot == pass_samples.
//
// Queue shards (first_segment.h): a lane files at most chunk_samples paths per launch, which is what the host sizes a shard for
// (cam_chunks, grow_workspace).
#pragma once
#include "first_segment.h"
#include "../../../include/spt_camera_models.h"

static_assert(kTMinEps == SPT_CM_T_MIN, "the camera models' t_min is the pinhole's");

struct CamJob {
    spt_camera_model model;
    spt_cm_plan plan;
    float4* aux_out;     // 4 float4 (spt_ray_aux) per radiance slot of the pass; null: the scene samples no texture
    FilmMask mask;       // an adaptive film's active set; pixel == null: every pixel
};

// kWalk: see first_segment.h
template <int kWalk>
__global__ void __launch_bounds__(256) k_primary_cam(DScene sc, RenderCtx rc, CamJob job) {
    const bool masked = job.mask.pixel != nullptr;
    if (masked && mask_tile_idle(rc, job.mask)) return;   // the whole block: mask.tile[tile] is one value per block
    stage_geometry<kWalk == 0>(sc);
    const uint32_t tile = blockIdx.x % rc.n_tiles, chunk = blockIdx.x / rc.n_tiles;
    const uint32_t tx = tile % rc.tiles_x, ty = tile / rc.tiles_x;
    const uint32_t i = tx * kTile + (threadIdx.x % kTile);
    const uint32_t row_local = ty * kTile + (threadIdx.x / kTile);
    const bool valid = (i < rc.width) && (row_local < rc.rows);
    const uint32_t lp = valid ? row_local * rc.width + i : 0u;
    const uint32_t j = valid ? global_row(rc, row_local) : 0u;
    const uint32_t pixel = valid ? j * rc.width + i : 0u;
    bool live = valid;
    if (masked) live = live && job.mask.pixel[lp] != 0u;   // a retired pixel traces nothing, environment or not
    const bool lazy_rng = rc.sampler == SPT_SAMPLER_RECURRENCE;   // the R2 sampler draws nothing: seed hits only
    const bool thin = job.model.type == SPT_CAMERA_THIN_LENS;
    const uint32_t s_begin = chunk * rc.chunk_samples;
    const uint32_t s_end = min(s_begin + rc.chunk_samples, rc.pass_samples);   // (block-uniform: every lane walks the same samples)
    [[maybe_unused]] uint2 spill_mem[kSpillStack];
    for (uint32_t s = s_begin; s < s_end; ++s) {
        const uint32_t gs = rc.pass_first + s;
        DRng rng;
        rng.s.state = 0ull;
        if (!lazy_rng) rng.s = spt_rng_seed(rc.seed, pixel, gs);
        float ox, oy, x, y, lx = 0.0f, ly = 0.0f;
        pixel_offset(rc, pixel, gs, rng, &ox, &oy);
        spt_cm_screen(i, j, rc.height, ox, oy, rc.width_inv, rc.height_inv, rc.aspect, &x, &y);
        if (thin) spt_cm_lens_point(rc.seed, pixel, gs, &lx, &ly);
        float o[3], d[3];
        spt_cm_ray(&job.model, &job.plan, x, y, lx, ly, o, d);
        DRay ray;
        ray.o = mk3(o[0], o[1], o[2]);
        ray.d = mk3(d[0], d[1], d[2]);
        ray.t_min = kTMinEps;
        const DHit h = first_closest<kWalk>(sc, ray, live, spill_mem);
        const uint32_t ri = s * rc.n_pixels + lp;
        const bool filed = first_file<kWalk>(sc, rc, ray, h, live, live, ri, rc.chunk_samples, s - s_begin, [&] {
            if (lazy_rng) rng.s = spt_rng_seed(rc.seed, pixel, gs);   // (else: the stream stands behind the two pixel-offset draws)
            return rng;
        });
        if (filed && job.aux_out != nullptr) {   // the same model at (x + aux_dx, y) and (x, y + aux_dy) with the same lens point
            float ao[3], ad[3];
            float4* const ar = job.aux_out + 4u * (size_t)ri;
            spt_cm_ray(&job.model, &job.plan, x + rc.aux_dx, y, lx, ly, ao, ad);
            ar[0] = make_float4(ao[0], ao[1], ao[2], 0.0f);
            ar[1] = make_float4(ad[0], ad[1], ad[2], 0.0f);
            spt_cm_ray(&job.model, &job.plan, x, y + rc.aux_dy, lx, ly, ao, ad);
            ar[2] = make_float4(ao[0], ao[1], ao[2], 0.0f);
            ar[3] = make_float4(ad[0], ad[1], ad[2], 0.0f);
        }
    }
    if (valid && chunk == 0u) rc.first_slot[lp] = live ? 0u : rc.pass_samples;
}

#if defined(SPT_INSTANTIATE_GROUP_CAMERA)
template __global__ void k_primary_cam<0>(DScene, RenderCtx, CamJob);
template __global__ void k_primary_cam<1>(DScene, RenderCtx, CamJob);
template __global__ void k_primary_cam<2>(DScene, RenderCtx, CamJob);
#else
extern template __global__ void k_primary_cam<0>(DScene, RenderCtx, CamJob);
extern template __global__ void k_primary_cam<1>(DScene, RenderCtx, CamJob);
extern template __global__ void k_primary_cam<2>(DScene, RenderCtx, CamJob);
#endif

// Every instantiation of the heavy kernel templates of kernels.h, grouped by the translation unit that compiles it
// (csrc/hip/inst_*.hip define SPT_INSTANTIATE_GROUP_x and get explicit instantiation DEFINITIONS; spt_hip.hip, which
// only launches them, gets explicit instantiation DECLARATIONS so that it compiles none of them).  One monolithic
// .hip took ~4 minutes per library build; split this way the groups compile side by side.
// (inst_deform.hip is a unit of the same kind without templates: spt_scene_deform's kernels, declared in deform_kernels.h.)
// (inst_bake.hip: spt_bake's kernels, bake_kernels.h - k_bake_intake<true>, k_bake_intake<false>, k_bake_intake_stream, k_bake_finish.)
// (inst_probe.hip: spt_probe's kernels, probe_kernels.h - k_probe_intake<true>, k_probe_intake<false>, k_probe_intake_stream, k_probe_finish.)
// (inst_camera.hip: the camera models' k_primary_cam<0|1|2>, camera_kernels.h.  spt_radiance's k_ray_intake<true>, k_ray_intake<false>,
//  k_ray_intake_stream and k_ray_finish, radiance_kernels.h, are compiled in spt_hip.hip itself.)
// (inst_gbuffer.hip: spt_gbuffer's k_gbuffer<kTex, kPndf>, gbuffer_kernels.h, the stage behind spt_radiance's intake kernels.)
// (inst_visibility.hip: spt_occluded's and spt_ao's kernels, visibility_kernels.h - k_occluded<true>, k_occluded<false>, k_occluded_stream,
//  k_ao<true>, k_ao<false>, k_ao_stream: any-hit walks over first_segment.h's first_any, without a path.)
// (inst_camera_device.hip: spt_camera_rays' and spt_camera_gbuffer's kernels, camera_device_kernels.h - k_camera_rays,
//  k_gbuffer_image<false, false>, k_gbuffer_image<true, false>, k_gbuffer_image<true, true>, k_gbuffer_image_finish.)
// (inst_hits.hip: spt_hits' kernels, hits_kernels.h - k_hits<true, false>, k_hits<true, true>, k_hits<false, false>, k_hits<false, true>:
//  the K nearest crossings and the crossing counts, over trace.h's nested walkers with a leaf functor of their own; compiled into
//  libspt_hip.so only.)
// (These four front ends trace and file their first segments with first_segment.h, which the four kernel headers include.)
#pragma once
#include "kernels.h"
#include "gbuffer_kernels.h"

#define SPT_UNPAREN(...) __VA_ARGS__
#define SPT_DECLARE_KERNEL(NAME, ARGS) extern template __global__ void SPT_UNPAREN NAME ARGS;
#define SPT_DEFINE_KERNEL(NAME, ARGS) template __global__ void SPT_UNPAREN NAME ARGS;

#define SPT_ARGS_PRIMARY (DScene, RenderCtx)
#define SPT_ARGS_BOUNCE (DScene, RenderCtx, uint32_t)
#define SPT_ARGS_PRIMARY_MASK (DScene, RenderCtx, FilmMask)

// k_primary<kLds, kChunked, kCount, kEye, kMask, M...>  (kMask: adaptive films, chunked only; M: the types of the extra arguments)
#define SPT_KERNELS_PRIMARY(X)                          \
    X((k_primary<true, false, false>), SPT_ARGS_PRIMARY)  \
    X((k_primary<true, true, false>), SPT_ARGS_PRIMARY)   \
    X((k_primary<true, false, false, true>), SPT_ARGS_PRIMARY)  \
    X((k_primary<true, true, false, true>), SPT_ARGS_PRIMARY)   \
    X((k_primary<false, false, false>), SPT_ARGS_PRIMARY) \
    X((k_primary<false, true, false>), SPT_ARGS_PRIMARY)  \
    X((k_primary<false, false, true>), SPT_ARGS_PRIMARY)  \
    X((k_primary<false, true, true>), SPT_ARGS_PRIMARY)   \
    X((k_primary<true, true, false, true, true, FilmMask>), SPT_ARGS_PRIMARY_MASK)  \
    X((k_primary<true, true, false, false, true, FilmMask>), SPT_ARGS_PRIMARY_MASK) \
    X((k_primary<false, true, false, false, true, FilmMask>), SPT_ARGS_PRIMARY_MASK)

// k_primary<true, kChunked, false, kEye = true, kMask, [FilmMask,] BlockCand>: camera rays against per-block candidate masks, and the
// kernel that makes the masks
#define SPT_ARGS_PRIMARY_CAND (DScene, RenderCtx, BlockCand)
#define SPT_ARGS_PRIMARY_MASK_CAND (DScene, RenderCtx, FilmMask, BlockCand)
#define SPT_ARGS_BLOCK_CAND (DScene, RenderCtx, uint64_t*, uint32_t)
#define SPT_KERNELS_PRIMARY_CAND(X)                                                   \
    X((k_block_candidates<SPT_BC_MAX_TRIS>), SPT_ARGS_BLOCK_CAND)                     \
    X((k_primary<true, false, false, true, false, BlockCand>), SPT_ARGS_PRIMARY_CAND) \
    X((k_primary<true, true, false, true, false, BlockCand>), SPT_ARGS_PRIMARY_CAND)  \
    X((k_primary<true, true, false, true, true, FilmMask, BlockCand>), SPT_ARGS_PRIMARY_MASK_CAND)

// k_shadow / k_extend <kLds, kCount, kFlat>, refilling variants <kCount>
#define SPT_KERNELS_RAYS(X)                          \
    X((k_shadow<true, false>), SPT_ARGS_BOUNCE)      \
    X((k_shadow<true, false, true>), SPT_ARGS_BOUNCE) \
    X((k_shadow<false, false>), SPT_ARGS_BOUNCE)     \
    X((k_shadow<false, true>), SPT_ARGS_BOUNCE)      \
    X((k_extend<true, false>), SPT_ARGS_BOUNCE)      \
    X((k_extend<true, false, true>), SPT_ARGS_BOUNCE) \
    X((k_extend<false, false>), SPT_ARGS_BOUNCE)     \
    X((k_extend<false, true>), SPT_ARGS_BOUNCE)      \
    X((k_shadow_dyn<false>), SPT_ARGS_BOUNCE)        \
    X((k_shadow_dyn<true>), SPT_ARGS_BOUNCE)         \
    X((k_extend_dyn<false>), SPT_ARGS_BOUNCE)        \
    X((k_extend_dyn<true>), SPT_ARGS_BOUNCE)

// streaming kernels (stream.h): k_shadow_stream / k_extend_stream <kCount>, k_primary_stream<kChunked, kCount, kMask>
#define SPT_KERNELS_STREAM(X)                             \
    X((k_shadow_stream<false>), SPT_ARGS_BOUNCE)          \
    X((k_shadow_stream<true>), SPT_ARGS_BOUNCE)           \
    X((k_extend_stream<false>), SPT_ARGS_BOUNCE)          \
    X((k_extend_stream<true>), SPT_ARGS_BOUNCE)           \
    X((k_primary_stream<false, false>), SPT_ARGS_PRIMARY) \
    X((k_primary_stream<true, false>), SPT_ARGS_PRIMARY)  \
    X((k_primary_stream<false, true>), SPT_ARGS_PRIMARY)  \
    X((k_primary_stream<true, true>), SPT_ARGS_PRIMARY)   \
    X((k_primary_stream<true, false, true, FilmMask>), SPT_ARGS_PRIMARY_MASK)

// k_shade<kFeat, kFirst, kFused, kTab, kGeoLds>
#define SPT_KERNELS_SHADE0(X)                                        \
    X((k_shade<0, true, true, true, true>), SPT_ARGS_BOUNCE)         \
    X((k_shade<0, false, true, true, true>), SPT_ARGS_BOUNCE)        \
    X((k_shade<0, false, true, true, true, true>), SPT_ARGS_BOUNCE)  \
    X((k_shade<0, true, false, true, true>), SPT_ARGS_BOUNCE)        \
    X((k_shade<0, false, false, true, true>), SPT_ARGS_BOUNCE)       \
    X((k_shade<0, true, false, false, false>), SPT_ARGS_BOUNCE)      \
    X((k_shade<0, false, false, false, false>), SPT_ARGS_BOUNCE)
// k_shade<0, kFirst, true, true, true, kLoop, false, OriginCand>: the fused simple kernels with per-origin-triangle candidate sets
// (origin.h) instead of the two tree walks: bounce 0, bounce >= 1 and the tail loop
#define SPT_ARGS_BOUNCE_ORIGIN (DScene, RenderCtx, uint32_t, OriginCand)
#define SPT_KERNELS_SHADE0_ORIGIN(X)                                                             \
    X((k_shade<0, true, true, true, true, false, false, OriginCand>), SPT_ARGS_BOUNCE_ORIGIN)    \
    X((k_shade<0, false, true, true, true, false, false, OriginCand>), SPT_ARGS_BOUNCE_ORIGIN)   \
    X((k_shade<0, false, true, true, true, true, false, OriginCand>), SPT_ARGS_BOUNCE_ORIGIN)
#define SPT_KERNELS_SHADE1(X)                                        \
    X((k_shade<1, true, false, true, true>), SPT_ARGS_BOUNCE)        \
    X((k_shade<1, false, false, true, true>), SPT_ARGS_BOUNCE)       \
    X((k_shade<1, true, false, false, false>), SPT_ARGS_BOUNCE)      \
    X((k_shade<1, false, false, false, false>), SPT_ARGS_BOUNCE)
#define SPT_KERNELS_SHADE2(X)                                        \
    X((k_shade<2, true, false, true, true>), SPT_ARGS_BOUNCE)        \
    X((k_shade<2, false, false, true, true>), SPT_ARGS_BOUNCE)       \
    X((k_shade<2, true, false, false, false>), SPT_ARGS_BOUNCE)      \
    X((k_shade<2, false, false, false, false>), SPT_ARGS_BOUNCE)
#define SPT_KERNELS_SHADE3A(X)                                       \
    X((k_shade<3, true, false, true, true>), SPT_ARGS_BOUNCE)        \
    X((k_shade<3, false, false, true, true>), SPT_ARGS_BOUNCE)       \
    X((k_shade<3, true, false, false, false>), SPT_ARGS_BOUNCE)
#define SPT_KERNELS_SHADE3B(X)                                       \
    X((k_shade<3, false, false, false, false>), SPT_ARGS_BOUNCE)     \
    X((k_shade<3, true, false, false, true>), SPT_ARGS_BOUNCE)       \
    X((k_shade<3, false, false, false, true>), SPT_ARGS_BOUNCE)

// k_shade<4, .>: position-normal distributions without a BSSRDF probe (kGeoLds plays no role: two table variants)
#define SPT_KERNELS_SHADE4(X)                                        \
    X((k_shade<4, true, false, true, true>), SPT_ARGS_BOUNCE)        \
    X((k_shade<4, false, false, true, true>), SPT_ARGS_BOUNCE)       \
    X((k_shade<4, true, false, false, false>), SPT_ARGS_BOUNCE)      \
    X((k_shade<4, false, false, false, false>), SPT_ARGS_BOUNCE)
// k_shade<5, .>: both
#define SPT_KERNELS_SHADE5A(X)                                       \
    X((k_shade<5, true, false, true, true>), SPT_ARGS_BOUNCE)        \
    X((k_shade<5, false, false, true, true>), SPT_ARGS_BOUNCE)       \
    X((k_shade<5, true, false, false, false>), SPT_ARGS_BOUNCE)
#define SPT_KERNELS_SHADE5B(X)                                       \
    X((k_shade<5, false, false, false, false>), SPT_ARGS_BOUNCE)     \
    X((k_shade<5, true, false, false, true>), SPT_ARGS_BOUNCE)       \
    X((k_shade<5, false, false, false, true>), SPT_ARGS_BOUNCE)

// k_shade_albedo<kTex, kPndf>: the bounce-0 stage of an albedo plan (SPT_RENDER_AOV_ALBEDO)
#define SPT_KERNELS_ALBEDO(X)                                        \
    X((k_shade_albedo<false, false>), SPT_ARGS_BOUNCE)               \
    X((k_shade_albedo<true, false>), SPT_ARGS_BOUNCE)                \
    X((k_shade_albedo<true, true>), SPT_ARGS_BOUNCE)

// k_shade<kFeat, false, false, kTab, kGeoLds, false, kAux = true, RayAux>: bounce 0 of spt_radiance with auxiliary rays, the textured levels
#define SPT_ARGS_BOUNCE_AUX (DScene, RenderCtx, uint32_t, RayAux)
#define SPT_KERNELS_SHADE2X(X)                                                                \
    X((k_shade<2, false, false, true, true, false, true, RayAux>), SPT_ARGS_BOUNCE_AUX)       \
    X((k_shade<2, false, false, false, false, false, true, RayAux>), SPT_ARGS_BOUNCE_AUX)
#define SPT_KERNELS_SHADE3X(X)                                                                \
    X((k_shade<3, false, false, true, true, false, true, RayAux>), SPT_ARGS_BOUNCE_AUX)       \
    X((k_shade<3, false, false, false, false, false, true, RayAux>), SPT_ARGS_BOUNCE_AUX)     \
    X((k_shade<3, false, false, false, true, false, true, RayAux>), SPT_ARGS_BOUNCE_AUX)
#define SPT_KERNELS_SHADE4X(X)                                                                \
    X((k_shade<4, false, false, true, true, false, true, RayAux>), SPT_ARGS_BOUNCE_AUX)       \
    X((k_shade<4, false, false, false, false, false, true, RayAux>), SPT_ARGS_BOUNCE_AUX)
#define SPT_KERNELS_SHADE5X(X)                                                                \
    X((k_shade<5, false, false, true, true, false, true, RayAux>), SPT_ARGS_BOUNCE_AUX)       \
    X((k_shade<5, false, false, false, false, false, true, RayAux>), SPT_ARGS_BOUNCE_AUX)     \
    X((k_shade<5, false, false, false, true, false, true, RayAux>), SPT_ARGS_BOUNCE_AUX)

// k_gbuffer<kTex, kPndf>: first-hit records along caller rays (spt_gbuffer), chosen like k_shade_albedo's instances
#define SPT_ARGS_GBUFFER (DScene, GBufferJob)
#define SPT_KERNELS_GBUFFER(X)                                       \
    X((k_gbuffer<false, false>), SPT_ARGS_GBUFFER)                   \
    X((k_gbuffer<true, false>), SPT_ARGS_GBUFFER)                    \
    X((k_gbuffer<true, true>), SPT_ARGS_GBUFFER)

#if defined(SPT_INSTANTIATE_GROUP_PRIMARY)
SPT_KERNELS_PRIMARY(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_PRIMARY_CAND)
SPT_KERNELS_PRIMARY_CAND(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_RAYS)
SPT_KERNELS_RAYS(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_STREAM)
SPT_KERNELS_STREAM(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE0)
SPT_KERNELS_SHADE0(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE0_ORIGIN)
SPT_KERNELS_SHADE0_ORIGIN(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE1)
SPT_KERNELS_SHADE1(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE2)
SPT_KERNELS_SHADE2(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE3A)
SPT_KERNELS_SHADE3A(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE3B)
SPT_KERNELS_SHADE3B(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE4)
SPT_KERNELS_SHADE4(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE5A)
SPT_KERNELS_SHADE5A(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE5B)
SPT_KERNELS_SHADE5B(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_ALBEDO)
SPT_KERNELS_ALBEDO(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE2X)
SPT_KERNELS_SHADE2X(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE3X)
SPT_KERNELS_SHADE3X(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE4X)
SPT_KERNELS_SHADE4X(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_SHADE5X)
SPT_KERNELS_SHADE5X(SPT_DEFINE_KERNEL)
#elif defined(SPT_INSTANTIATE_GROUP_GBUFFER)
SPT_KERNELS_GBUFFER(SPT_DEFINE_KERNEL)
#else
SPT_KERNELS_PRIMARY(SPT_DECLARE_KERNEL)
SPT_KERNELS_PRIMARY_CAND(SPT_DECLARE_KERNEL)
SPT_KERNELS_RAYS(SPT_DECLARE_KERNEL)
SPT_KERNELS_STREAM(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE0(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE0_ORIGIN(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE1(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE2(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE3A(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE3B(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE4(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE5A(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE5B(SPT_DECLARE_KERNEL)
SPT_KERNELS_ALBEDO(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE2X(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE3X(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE4X(SPT_DECLARE_KERNEL)
SPT_KERNELS_SHADE5X(SPT_DECLARE_KERNEL)
SPT_KERNELS_GBUFFER(SPT_DECLARE_KERNEL)
#endif

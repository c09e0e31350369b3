/*
 * spt_host.h — C ABI of the host side (libspt_host.so): the stand-in for the
 * reference's Rust host that the north star keeps (scene JSON loader, camera,
 * surface/material plumbing, image write-out).  No Rust toolchain exists in the
 * build image, so this side is C++ behind a C ABI; it produces exactly the POD
 * `spt_scene_desc` a Rust `Scene::flatten()` would hand to libspt_hip.so.
 *
 * Reference counterparts:
 *   spt_host_load_scene     loader::load_scene      src/loader/json.rs:53-199
 *                           SceneResources::to_scene src/core/scene_resources.rs:29-138
 *   spt_host_load_renderer  loader::load_renderer   src/loader/json.rs:19-51
 *   spt_host_scene_camera   Scene::get_camera       src/core/scene.rs:29-41
 *   spt_host_film_to_rgb8   color_to_rgb            src/core/film.rs:94-99
 *   spt_host_write_png      image.save              src/renderer/pt.rs:290-294
 * Errors are returned as status codes + spt_host_last_error() where the reference
 * returns anyhow::Error (load) or panics (get_camera).
 */
#ifndef SPT_HOST_H
#define SPT_HOST_H

#include "spt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spt_host_scene spt_host_scene; /* owns every array the desc points to */

enum {
    SPT_HOST_ERR_IO = 100,       /* file missing / unreadable */
    SPT_HOST_ERR_PARSE = 101,    /* JSON / OBJ / EXR syntax */
    SPT_HOST_ERR_SCHEMA = 102,   /* missing or mistyped field, unknown name/type (anyhow::bail! sites) */
    SPT_HOST_ERR_UNSUPPORTED = 103 /* valid reference feature outside the hot-path scope */
};

spt_status spt_host_load_scene(const char* scene_json_path, spt_host_scene** out);
const spt_scene_desc* spt_host_scene_desc(const spt_host_scene* scene);
/* name == NULL: the scene must have exactly one camera (reference panics otherwise). */
spt_status spt_host_scene_camera(const spt_host_scene* scene, const char* name, spt_camera* out);
void spt_host_scene_free(spt_host_scene* scene);
/* Which routine intersects the scene's Bezier patches (Catmull-Clark surfaces included): 0 = Bezier clipping, the reference's
 * default build; 1 = Newton's iteration, the reference built with `--features bezier_ni` (Cargo.toml:34-36, bezier.rs:58-103).
 * Sets spt_bezier_patch::cp[0][0][3] of every patch of THIS scene (call it before spt_scene_create); without the call the
 * process-wide default applies (clipping, or Newton when the environment variable SPT_BEZIER_NI is set to a non-zero value). */
spt_status spt_host_scene_set_bezier_newton(spt_host_scene* scene, int32_t newton);

/* Animating a loaded scene (the arrays spt_scene_update takes).  The loader is the only place that knows how an instance record
 * follows from a transform (Instance::new), what a shape light's power is under it, how the TLAS orders the instances and what
 * the alias table over the lights' powers is: these calls run that same finalisation again.  After a call that returns SPT_OK,
 * spt_host_scene_desc is the descriptor spt_host_load_scene would produce for the same scene file with the new transforms (or
 * light) written into it: tlas_nodes, instances (their order too), lights and light_alias, bit for bit; every other array is
 * untouched and keeps its address.  The four arrays may move: read the descriptor again.  A refused call leaves the scene as
 * it was. */
/* The index of the instance called `name` in the CURRENT descriptor (the order changes with the transforms).
 * SPT_HOST_ERR_SCHEMA: no such instance. */
spt_status spt_host_scene_instance_index(const spt_host_scene* scene, const char* name, uint32_t* index);
/* New object-to-world transforms of n named instances: fwd holds n x 12 floats in the layout of spt_instance::fwd (the three
 * columns of the 3x3 part, then the translation).  SPT_HOST_ERR_SCHEMA: an unknown name; SPT_ERR_INVALID_ARG: a transform that is
 * not invertible or yields a box that is not finite, or a name given twice. */
spt_status spt_host_scene_set_transforms(spt_host_scene* scene, uint32_t n, const char* const* names, const float* fwd);
/* Replaces the directional, point or spot light called `name` (the type must stay; `power` is set from the strength as the
 * loader sets it, `instance` is ignored). */
spt_status spt_host_scene_set_light(spt_host_scene* scene, const char* name, const spt_light* light);
/* Deforming a loaded mesh (spt_scene_deform takes the result to a live device scene).  `primitive_name` names a `trimesh`
 * primitive of a JSON scene; its vertices are in the OBJ loader's single-index order (one vertex per distinct v/vt/vn tuple, in
 * first-seen order).  SPT_HOST_ERR_SCHEMA: no such primitive; SPT_HOST_ERR_UNSUPPORTED: a glTF primitive or a Catmull-Clark
 * surface.
 *   _mesh_index: the primitive's index in the descriptor's meshes[] (a helper for callers that name meshes to spt_scene_deform,
 *     such as the Python binding; nothing else depends on it).
 *   _mesh_positions: n_vertices, and 3 floats per vertex into `out` unless it is NULL.
 *   _set_mesh_positions: new positions (and normals; NULL keeps them).  Tangents are computed again, the mesh's tri_pos /
 *     tri_attr range is rewritten in place (triangle k stays the same face), the boxes of its blas_nodes are refitted over the
 *     unchanged topology, and every instance of it, the TLAS, the shape lights' power and the alias table follow as in
 *     spt_host_scene_set_transforms.  SPT_ERR_INVALID_ARG: a wrong count or a value that is not finite; the scene is unchanged.
 *     Setting the file's own positions again gives the loaded descriptor back byte for byte. */
spt_status spt_host_scene_mesh_index(const spt_host_scene* scene, const char* primitive_name, uint32_t* mesh);
spt_status spt_host_scene_mesh_positions(const spt_host_scene* scene, const char* primitive_name, uint32_t* n_vertices, float* out /* may be NULL */);
spt_status spt_host_scene_set_mesh_positions(spt_host_scene* scene, const char* primitive_name, uint32_t n_vertices, const float* positions,
                                             const float* normals /* NULL: keep */);
/* Deforming a loaded mesh from vertex arrays, its records made only when somebody reads them (spt_scene_deform_vertices takes the
 * vertices to a live device scene, which makes its own records).
 *   _mesh_topology: fills *out for spt_scene_mesh_topology with pointers into the scene - the OBJ loader's indices in face order,
 *     the triangle order the BLAS build chose as face_of_tri, uv, the normals in force, the counts, `mesh` as _mesh_index gives
 *     it.  The pointers stay valid until spt_host_scene_free (the normals' contents follow later edits).
 *   _set_mesh_vertices: the checks and refusals of _set_mesh_positions.  The vertices are stored, the mesh's root box is the
 *     min / max over the vertices some face names, its instances, the TLAS, the lights and the alias table are made again from
 *     that box - and the mesh is left PENDING: its tri_pos / tri_attr / blas_nodes ranges are made by the next
 *     spt_host_scene_desc (or any other entry that reads them), which therefore returns exactly what _set_mesh_positions would
 *     have left.  A mesh with an emissive instance needs its triangles for the light's power: it is made at once.
 *     _set_mesh_positions on a pending mesh supersedes it.
 *   _dynamic: the four arrays spt_scene_update takes, as they stand, WITHOUT making any pending mesh. */
spt_status spt_host_scene_mesh_topology(const spt_host_scene* scene, const char* primitive_name, spt_mesh_topology* out);
spt_status spt_host_scene_set_mesh_vertices(spt_host_scene* scene, const char* primitive_name, uint32_t n_vertices, const float* positions,
                                            const float* normals /* NULL: keep */);
spt_status spt_host_scene_dynamic(const spt_host_scene* scene, spt_scene_update_desc* out);
/* `spt --animate FILE`: {"frames": [ {"<instance name>": <transform object in the scene file's own syntax: matrix, scale, rotate,
 * translate>, ...}, ... ]}, checked against `scene` (SPT_HOST_ERR_SCHEMA: a malformed file, an unknown instance).
 * spt_host_animation_apply hands frame `frame`'s transforms to spt_host_scene_set_transforms; instances a frame does not name
 * keep the transform they have. */
typedef struct spt_host_animation spt_host_animation;
spt_status spt_host_animation_load(const char* path, const spt_host_scene* scene, spt_host_animation** out);
uint32_t spt_host_animation_frames(const spt_host_animation* animation);
spt_status spt_host_animation_apply(const spt_host_animation* animation, uint32_t frame, spt_host_scene* scene);
void spt_host_animation_free(spt_host_animation* animation);

/* Fills max_depth, spp, sampler, division_x/y of *params (other fields untouched)
 * and the box-filter radius. */
spt_status spt_host_load_renderer(const char* renderer_json_path, spt_render_params* params,
                                  float* filter_radius);
/* spt_host_load_renderer that also takes the weighted filters of spt_film_filter (spt_abi.h), which the function above refuses
 * as unknown types.  "filter" is one of
 *     {"type": "box", "radius": r}      {"type": "gaussian", "radius": r, "alpha": a}          alpha optional, 2.0
 *     {"type": "tent", "radius": r}     {"type": "mitchell", "radius": r, "b": B, "c": C}      radius optional, 2.0; b, c 1/3
 * (numbers are floats: an integer literal is a schema error).  *filter receives the desc to hand to spt_film_filter;
 * params->filter_radius is r, with SPT_RENDER_BOX_RADIUS when r != 0.5: the halo a sample-keeping film stores. */
spt_status spt_host_load_renderer_filter(const char* renderer_json_path, spt_render_params* params,
                                         spt_filter_desc* filter);

/* u8 = (clamp(c*255, 0, 255)) as u8 — truncation, no gamma (src/core/film.rs:94-99). */
void spt_host_film_to_rgb8(const float* rgb_mean, uint64_t n_pixels, uint8_t* rgb8_out);
spt_status spt_host_write_png(const char* path, const uint8_t* rgb8, uint32_t width, uint32_t height);
/* baseline JPEG, 4:4:4, IJG quality scale (the image crate's JpegEncoder default is 75) */
spt_status spt_host_write_jpeg(const char* path, const uint8_t* rgb8, uint32_t width, uint32_t height, int32_t quality);
/* `image.save(path)` (src/renderer/pt.rs:292-294): the extension picks the format - png, jpg / jpeg */
spt_status spt_host_write_image(const char* path, const uint8_t* rgb8, uint32_t width, uint32_t height);

/* The conservative block-versus-triangle test of include/spt_block_cand.h on the host, for checking it without a device.  A block
 * is the 16 columns x 4 local rows one wave of the primary kernel owns in the shard (shard_index, shard_count, strip_rows; `rows`
 * local rows): block = 4 * (tile_x + tiles_x * tile_y) + wave.  `inv` / `fwd` are the instance's spt_instance matrices, tri_pos
 * 9 floats (p0, p1, p2, object space) per triangle, at most 64.  Bit k of *mask_out is set unless no camera ray of the block's
 * pixels can hit triangle k. */
spt_status spt_host_block_candidates(const spt_camera* cam, uint32_t width, uint32_t height, uint32_t shard_index, uint32_t shard_count,
                                     uint32_t strip_rows, uint32_t rows, uint32_t block, const float* inv, const float* fwd, uint32_t n_tris,
                                     const float* tri_pos, uint64_t* mask_out);

/* The rays of a camera model (include/spt_abi.h, "camera models"; include/spt_camera_models.h, which the device kernel includes too)
 * for the samples [first, first + count) of a plan: rays[count][height][width], streams (pixel, plan index), t_min 0.0001f; aux (or
 * NULL) the auxiliary rays in the same order.  rays == radiance input: spt_radiance over them with the plan's seed and max_depth and
 * rng_skip = the pixel-offset draws of the plan's sampler (2, recurrence 0) returns the samples a film of the model holds.  All four
 * model types; SPT_ERR_INVALID_ARG for what spt_render_camera refuses of a model, a bad plan or samples past its spp. */
spt_status spt_host_camera_rays(const spt_camera_model* model, const spt_render_params* plan, uint32_t first, uint32_t count,
                                spt_path_ray* rays, spt_ray_aux* aux /* or NULL */);

/* spt_bake's specification (include/spt_abi.h, "irradiance at surface points"; include/spt_bake.h, which the device kernel includes
 * too) evaluated on the host over a descriptor, so that callers and tests can reproduce a bake from spt_radiance and spt_trace_any.
 * `points`: n_points spt_bake_point (kind SPT_BAKE_POINTS_SURFACE) or spt_bake_world_point; flags: SPT_BAKE_FLIP or 0.  Every output
 * may be NULL:
 *   rays_out        n_points * samples gather rays in (i, k) order, streams (first_point + i, first_sample + k): spt_radiance input
 *   pos_out, nrm_out  3 floats per point, the resolved world position and (flipped) normal
 *   delta_rays_out  per point and light of desc->lights, [i * n_lights + l]: the shadow ray, all zero where the light is skipped
 *   delta_li_out    3 floats at the same index: li, zeros where skipped
 * SPT_ERR_INVALID_ARG: what spt_bake refuses of a host point (the message names the first index), an unknown kind or flag. */
spt_status spt_host_bake_rays(const spt_scene_desc* desc, uint32_t kind, uint32_t flags, uint64_t n_points, const void* points, uint32_t samples,
                              uint64_t seed, uint32_t first_point, uint32_t first_sample, spt_path_ray* rays_out, float* pos_out, float* nrm_out,
                              spt_ray* delta_rays_out, float* delta_li_out);
/* The texels of a width x height lightmap of the mesh instance called `instance_name`, as bake points.  The centre of texel (x, y) is
 * uv ((x + 0.5) / W, (y + 0.5) / H), no wrap, no flip.  It is tested against the uv triangles of the instance's mesh in triangle
 * order: E(a, b, p) = (b.x - a.x) * (p.y - a.y) - (b.y - a.y) * (p.x - a.x) in double, area = E(uv0, uv1, uv2), b0 = E(uv1, uv2, p) / area,
 * b1 = E(uv2, uv0, p) / area, b2 = E(uv0, uv1, p) / area; inside when all three are >= 0; zero-area uv triangles are skipped; the lowest
 * triangle index wins.  Emits {instance (its current index), prim, (float)b1, (float)b2} and the texel's linear index y * W + x, in
 * texel order; uncovered texels are omitted.  *n_out is the number of covered texels; at most `capacity` records are written
 * (capacity == 0 only counts, the outputs may then be NULL).  No dilation, no conservative coverage. */
spt_status spt_host_lightmap_points(const spt_host_scene* scene, const char* instance_name, uint32_t width, uint32_t height,
                                    spt_bake_point* points_out, uint32_t* texels_out, uint64_t capacity, uint64_t* n_out);

/* spt_probe's specification (include/spt_abi.h, "spherical-harmonic light probes"; include/spt_probe.h, which the device kernels
 * include too) evaluated on the host, so that callers and tests can reproduce a probe from spt_radiance and spt_trace_any.  `lights`
 * are n_lights records of a descriptor (may be NULL with n_lights == 0).  Every output may be NULL:
 *   rays_out        n_points * samples gather rays in (i, k) order, streams (first_point + i, first_sample + k): spt_radiance input
 *   weights_out     9 floats per (i, k): spt_probe_basis of the ray's direction
 *   delta_rays_out  per probe and light, [i * n_lights + l]: the shadow ray, all zero where the light is skipped
 *   delta_li_out    3 floats at the same index: li, zeros where skipped
 *   delta_basis_out 9 floats at the same index: spt_probe_basis of the shadow ray's direction, zeros where skipped
 * SPT_ERR_INVALID_ARG: a probe whose p is not finite (the message names the first index). */
spt_status spt_host_probe_rays(uint32_t n_lights, const spt_light* lights, uint64_t n_points, const spt_probe_point* points, uint32_t samples, uint64_t seed,
                               uint32_t first_point, uint32_t first_sample, spt_path_ray* rays_out, float* weights_out, spt_ray* delta_rays_out,
                               float* delta_li_out, float* delta_basis_out);
/* spt_probe_basis over n directions (3 floats each, used as given): 9 floats per direction */
spt_status spt_host_probe_basis(uint64_t n, const float* dirs, float* out);

/* The per-origin-triangle candidate table of include/spt_origin_cand.h on the host, for checking it without a device.  Instance i
 * has the spt_instance matrices inv / fwd (12 floats each) and the normal matrix nrm (9 floats); triangle k (at most 64) belongs
 * to instance tri_instance[k], with tri_pos 9 floats (p0, p1, p2, object space) and tri_nrm its 3 vertex normals; its slot and its
 * row are both k.  words_out receives 4 words per triangle (loose up, loose down, tight up, tight down; bit u = triangle u),
 * info_out 8 doubles: the scene's centre (3) and radius, reach, delta(reach), delta_scene, tight (0 / 1). */
spt_status spt_host_origin_candidates(uint32_t n_instances, const float* inv, const float* fwd, const float* nrm, uint32_t n_tris,
                                      const uint32_t* tri_instance, const float* tri_pos, const float* tri_nrm, uint64_t* words_out,
                                      double* info_out);

/* OpenEXR scanline I/O (RGB f32 / f16; reads NO_COMPRESSION / RLE / ZIPS / ZIP / PIZ / PXR24, writes uncompressed) for
 * `environment {type: "exr"}` (get_exr_image, src/core/loader.rs:374-390). */
spt_status spt_host_read_exr(const char* path, uint32_t* width, uint32_t* height, float** rgb_out);
spt_status spt_host_write_exr(const char* path, const float* rgb, uint32_t width, uint32_t height);
/* PNG -> RGBA8 texels (r | g<<8 | b<<16 | a<<24) the way `image::open` + `get_pixel` present an
 * `image_file` texture (get_image, src/core/loader.rs:366-371); free with spt_host_free. */
spt_status spt_host_read_png(const char* path, uint32_t* width, uint32_t* height, uint32_t** rgba8_out);
/* the same for a PNG or a JPEG file (told apart by content; baseline / progressive Huffman, IJG arithmetic) */
spt_status spt_host_read_image(const char* path, uint32_t* width, uint32_t* height, uint32_t** rgba8_out);
/* The Catmull-Clark front end on its own (CatmullClark::load, src/primitive/catmull.rs:93-101): the bicubic patches of an
 * ASCII PLY control mesh after `fas_times` rounds of feature-adaptive subdivision, 16 control points (x, y, z) per patch;
 * free with spt_host_free.  (A scene's `catmull_clark` primitive goes through the same code.) */
spt_status spt_host_catmull_clark(const char* ply_path, uint32_t fas_times, uint32_t* n_patches, float** control_points_out);
void spt_host_free(void* p);

/* ---- one call, N devices, one film -------------------------------------------------------------------------------------
 * The reference's `render` fans the image rows out over all of its worker threads and assembles ONE film
 * (PathTracer::render, src/renderer/pt.rs:243-287; UnsafeFilm, src/core/film.rs:101-116).  The counterpart here: one
 * worker thread per device, each with a full scene replica (spt_scene_create on its device), device k rendering the
 * interleaved row strips (j / strip_rows) % n == k of the image straight into the caller's film (out_strip_stride: one
 * strided DMA per device, no host-side scatter, no collective).  Seeds depend on (pixel, sample) only, so the film is
 * bit-identical for every n.  The device entry points arrive as a table, so that the fan-out (this library has no HIP in
 * it) can be driven with libspt_hip.so's functions - what `spt --gpus N` and the Python binding do - or with stand-ins. */
typedef struct spt_device_api {
    spt_status (*scene_create)(const spt_scene_desc* desc, int32_t device, spt_scene** out);
    void (*scene_destroy)(spt_scene* scene);
    spt_status (*render)(const spt_scene* scene, const spt_camera* cam, const spt_render_params* params, float* rgb_mean_out,
                         spt_render_stats* stats);
    const char* (*last_error)(void);
    /* optional (NULL: the film is handed to `render` as it is): page-lock / unlock the caller's film once, so that every
     * device's copy-out is a DMA */
    spt_status (*pin_host)(void* p, uint64_t bytes);
    void (*unpin_host)(void* p);
} spt_device_api;

typedef struct spt_host_multi spt_host_multi;
/* Creates one scene replica per entry of `devices` (concurrently, one thread each; an index may repeat: two workers then
 * share that device).  Fails as a whole if any replica fails. */
spt_status spt_host_multi_create(const spt_scene_desc* desc, const spt_device_api* api, uint32_t n_devices, const int32_t* devices,
                                 spt_host_multi** out);
/* Renders the full image of `params` (its shard fields are overwritten: shard k of n_devices, `strip_rows` rows per strip, 0 = a
 * default that keeps the shares even) into film[height][width][3].  stats: NULL or n_devices entries (one per device; each
 * is written with params->stats_size bytes as spt_render does).  Synchronous: the film is complete on return.
 * Lifetime of `film`: with api->pin_host set, the film stays page-locked AFTER the call returns, so that a caller who renders
 * into one buffer frame after frame pays for one registration.  The registration is dropped by the next spt_host_multi_render
 * with another pointer or size (before it pins the new film) and by spt_host_multi_destroy.  Until one of the two, the film
 * must stay mapped at that address: do not free or unmap it earlier. */
spt_status spt_host_multi_render(spt_host_multi* m, const spt_camera* cam, const spt_render_params* params, uint32_t strip_rows,
                                 float* film, spt_render_stats* stats);
uint32_t spt_host_multi_device_count(const spt_host_multi* m);
void spt_host_multi_destroy(spt_host_multi* m);

/* ---- a progressive film over the replicas of a spt_host_multi (additive: detect it by symbol) -----------------------------------
 * A multi film is one shard film per replica - shard k of n, the interleaved strips of spt_host_multi_render - driven as one.
 * A sample depends on (seed, pixel, plan index) only, so a shard film's S, Q, buckets, mask and counts are the rows of the whole
 * film's, and every per-pixel call (render, adapt, the read-outs) is the same call on every shard, run side by side on the
 * persistent workers of the spt_host_multi.  Every read-out returns the FULL image, height x width: each worker reads its shard's
 * packed rows into a buffer the multi film owns and scatters the strips to their rows itself, so the scatter of one shard runs
 * beside the device read of another.  The one call that needs neighbours, the denoiser, gathers SPT_FILM_MEAN and
 * SPT_FILM_VAR_OF_MEAN of the film (and of the guide and albedo multi films) into full-image arrays the multi film owns and runs
 * ONE denoise_image on replica 0's scene.  Every read-out and the denoised image have the bits of the same plan's single-device
 * film, for every number of devices and every strip_rows, repeated device indices and shards without rows included.
 * The film entry points arrive as a second table, so that stand-ins can drive the fan-out.  `size` is sizeof of the table as the
 * caller was compiled (the table only grows at its tail); an entry that is NULL or lies behind `size` makes the multi call that
 * needs it return SPT_ERR_UNSUPPORTED. */
typedef struct spt_device_film_api {
    uint32_t size, pad;
    spt_status (*film_create)(const spt_scene* scene, const spt_camera* cam, const spt_render_params* params, uint32_t first_sample,
                              uint32_t film_flags, spt_film** out);
    void (*film_destroy)(spt_film* film);
    spt_status (*film_render)(spt_film* film, uint32_t n_samples);
    spt_status (*film_samples)(const spt_film* film, uint32_t* done);
    spt_status (*film_read)(spt_film* film, uint32_t what, float* out);
    spt_status (*film_read_counts)(spt_film* film, uint32_t* out);
    spt_status (*film_adapt)(spt_film* film, float rel_error, float abs_floor, uint32_t min_samples, uint32_t* active_out);
    spt_status (*film_buckets)(spt_film* film, uint32_t n_buckets);
    spt_status (*film_read_robust)(spt_film* film, uint32_t estimator, float* out);
    spt_status (*film_read_rgb8)(spt_film* film, uint32_t source, spt_film* guide, const spt_denoise_params* dn, uint8_t* out);
    spt_status (*denoise_image)(const spt_scene* scene, const spt_image_denoise_job* job, void* out);
    const char* (*last_error)(void);
} spt_device_film_api;

typedef struct spt_host_multi_film spt_host_multi_film;
/* Creates shard film k of n on replica k, for every k (side by side on the workers).  `params` is the plan (its shard fields are
 * overwritten; `strip_rows` as in spt_host_multi_render, 0 = its default; the plan's flags pass through, so a guide or albedo multi
 * film is the same call with SPT_RENDER_DEBUG_NORMAL / SPT_RENDER_AOV_ALBEDO); first_sample and film_flags as in spt_film_create;
 * n_buckets != 0: spt_film_buckets on every shard.  Refused as a whole, with no film left behind: null arguments, width or height 0,
 * a plan with SPT_RENDER_ASYNC / PROFILE / COUNT_VISITS or an out_strip_stride (SPT_ERR_INVALID_ARG), and whatever a shard refuses
 * (its status, its message behind "device D (shard k of n): ").  Destroy the multi film before its spt_host_multi; a multi film
 * that is still alive at spt_host_multi_destroy loses its shard films there, refuses every later call (SPT_ERR_INVALID_ARG) and
 * is still released by spt_host_multi_film_destroy. */
spt_status spt_host_multi_film_create(spt_host_multi* m, const spt_device_film_api* film_api, const spt_camera* cam,
                                      const spt_render_params* params, uint32_t strip_rows, uint32_t first_sample, uint32_t film_flags,
                                      uint32_t n_buckets, spt_host_multi_film** out);
/* spt_film_render / spt_film_adapt on every shard.  *active_out (may be NULL) is the sum over the shards.  When every shard
 * refuses, the call is refused with the first shard's status and message and the multi film is as it was.  When some shards fail
 * and others do not, the shards are out of step and the multi film is BROKEN: every later call except destroy returns
 * SPT_ERR_INVALID_ARG with a message that says so and repeats the first error. */
spt_status spt_host_multi_film_render(spt_host_multi_film* f, uint32_t n_samples);
spt_status spt_host_multi_film_adapt(spt_host_multi_film* f, float rel_error, float abs_floor, uint32_t min_samples, uint32_t* active_out);
spt_status spt_host_multi_film_samples(const spt_host_multi_film* f, uint32_t* done);
/* The full image, height * width (* 3): spt_film_read / _read_counts / _read_robust / _read_rgb8 of every shard, scattered to its
 * rows.  read_rgb8 takes SPT_READ_MEAN, SPT_READ_ROBUST_MON and SPT_READ_ROBUST_GMON; SPT_READ_DENOISED is SPT_ERR_INVALID_ARG
 * (a shard cannot filter: spt_host_multi_film_denoise with SPT_DENOISE_OUT_RGB8 returns those bytes). */
spt_status spt_host_multi_film_read(spt_host_multi_film* f, uint32_t what, float* image);
spt_status spt_host_multi_film_read_counts(spt_host_multi_film* f, uint32_t* image);
spt_status spt_host_multi_film_read_robust(spt_host_multi_film* f, uint32_t estimator, float* image);
spt_status spt_host_multi_film_read_rgb8(spt_host_multi_film* f, uint32_t source, uint8_t* image);
/* spt_denoise_job with multi films: the guide and the albedo film are multi films of the same spt_host_multi, width, height and
 * strip layout (anything else: SPT_ERR_INVALID_ARG), both may be NULL. */
typedef struct spt_host_multi_film_denoise_job {
    uint32_t size, flags;             /* sizeof(spt_host_multi_film_denoise_job) as the caller was compiled; SPT_DENOISE_* */
    spt_host_multi_film* guide;
    spt_host_multi_film* albedo;
    const spt_denoise_params* params; /* may be NULL: the defaults */
    float k_albedo, eps_albedo, eps_demod;   /* the defaults 1, 1e-2, 1e-2 when size ends before them */
    uint32_t pad;
} spt_host_multi_film_denoise_job;
/* image: height * width * 3 f32, or u8 with SPT_DENOISE_OUT_RGB8.  Gathers mean and variance of the mean of the film, the guide
 * and the albedo film (every worker reads and scatters its shards' rows), then runs denoise_image on replica 0's scene: the bits of
 * spt_film_denoise_job on the single-device films.  The films are read only. */
spt_status spt_host_multi_film_denoise(spt_host_multi_film* f, const spt_host_multi_film_denoise_job* job, void* image);
void spt_host_multi_film_destroy(spt_host_multi_film* f);   /* before spt_host_multi_destroy of its spt_host_multi (see above) */

const char* spt_host_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SPT_HOST_H */

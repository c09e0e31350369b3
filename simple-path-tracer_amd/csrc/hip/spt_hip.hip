// libspt_hip.so — C ABI (include/spt_abi.h) over the gfx950 kernels.
// Host code here only validates descriptors, moves the flattened scene into HBM
// and enqueues kernels on one HIP stream; there is no CPU rendering path.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "kernel_list.h"   // the heavy kernel templates: declared here, compiled in inst_*.hip
#include "film_kernels.h"
#include "radiance_kernels.h"
#include "bake_kernels.h"
#include "visibility_kernels.h"   // spt_occluded's and spt_ao's kernels: declared here, compiled in inst_visibility.hip
#include "hits_kernels.h"   // spt_hits' kernels: declared here, compiled in inst_hits.hip
#include "probe_kernels.h"
#include "camera_kernels.h"   // k_primary_cam: declared here, compiled in inst_camera.hip
#include "camera_device_kernels.h"   // spt_camera_rays' and spt_camera_gbuffer's kernels: declared here, compiled in inst_camera_device.hip
#include "deform_kernels.h"   // spt_scene_deform's kernels: declared here, compiled in inst_deform.hip
#include "abi_error.h"     // AbiError, fail
#include "scene_build.h"   // everything a scene derives from its descriptor on the host

using namespace scene_build;

namespace {

thread_local std::string g_error;

#define HIP_CHECK(expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            fail(e_ == hipErrorOutOfMemory ? SPT_ERR_OUT_OF_MEMORY : SPT_ERR_HIP,                    \
                 std::string(#expr) + ": " + hipGetErrorString(e_));                                 \
    } while (0)

int usable_device_count() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

struct DeviceBuffer {   // owning: freed with the scene object (the owner selects the device first)
    void* p = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { release(); }
    void alloc(size_t n) {
        release();
        if (n == 0) n = 16;
        HIP_CHECK(hipMalloc(&p, n));
        bytes = n;
    }
    void ensure(size_t n) {
        if (n > bytes) alloc(n);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    void swap(DeviceBuffer& o) {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
    }
    template <class T>
    void upload(const T* src, size_t count) {
        alloc(std::max<size_t>(count * sizeof(T), 16));
        if (count) HIP_CHECK(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

struct PinnedBuffer {   // owning, page-locked host memory: freed with the scene object, like a DeviceBuffer
    void* p = nullptr;
    size_t bytes = 0;
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() { release(); }
    void ensure(size_t n) {
        if (n <= bytes) return;
        release();
        HIP_CHECK(hipHostMalloc(&p, n, hipHostMallocDefault));
        bytes = n;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

}  // namespace

// Scenes with Bezier patches are served by libspt_hip_bez.so: this same source compiled with SPT_WITH_BEZIER=1 (the
// patch test of csrc/hip/bezier.h keeps a 16-frame subdivision stack in scratch memory, and a kernel that can call it
// pays for that scratch on every wave whether or not the scene has patches).  spt_scene_create of the plain library
// opens the other one next to itself and every later call on that scene is passed through.
struct BezierLib {
    void* handle = nullptr;
    decltype(&spt_scene_create) create = nullptr;
    decltype(&spt_scene_destroy) destroy = nullptr;
    decltype(&spt_render) render = nullptr;
    decltype(&spt_render_wait) render_wait = nullptr;
    decltype(&spt_film_create) film_create = nullptr;
    decltype(&spt_film_render) film_render = nullptr;
    decltype(&spt_film_samples) film_samples = nullptr;
    decltype(&spt_film_read) film_read = nullptr;
    decltype(&spt_film_destroy) film_destroy = nullptr;
    decltype(&spt_film_adapt) film_adapt = nullptr;
    decltype(&spt_film_read_counts) film_read_counts = nullptr;
    decltype(&spt_film_denoise) film_denoise = nullptr;
    decltype(&spt_film_denoise_job) film_denoise_job = nullptr;
    decltype(&spt_film_buckets) film_buckets = nullptr;
    decltype(&spt_film_read_buckets) film_read_buckets = nullptr;
    decltype(&spt_film_read_robust) film_read_robust = nullptr;
    decltype(&spt_film_read_rgb8) film_read_rgb8 = nullptr;
    decltype(&spt_film_read_samples) film_read_samples = nullptr;
    decltype(&spt_film_filter) film_filter = nullptr;   // (resolved if present: a library without it serves every other call)
    decltype(&spt_denoise_image) denoise_image = nullptr;
    decltype(&spt_trace_closest) trace_closest = nullptr;
    decltype(&spt_trace_any) trace_any = nullptr;
    decltype(&spt_radiance) radiance = nullptr;
    decltype(&spt_scene_update) scene_update = nullptr;   // (resolved if present, like film_filter)
    decltype(&spt_scene_deform) scene_deform = nullptr;   // (the same)
    decltype(&spt_scene_mesh_topology) scene_mesh_topology = nullptr;       // (the same)
    decltype(&spt_scene_deform_vertices) scene_deform_vertices = nullptr;   // (the same)
    decltype(&spt_scene_read_triangles) scene_read_triangles = nullptr;     // (the same)
    decltype(&spt_render_camera) render_camera = nullptr;             // (the same)
    decltype(&spt_film_create_camera) film_create_camera = nullptr;   // (the same)
    decltype(&spt_bake) bake = nullptr;                               // (the same)
    decltype(&spt_probe) probe = nullptr;                             // (the same)
    decltype(&spt_gbuffer) gbuffer = nullptr;                         // (the same)
    decltype(&spt_occluded) occluded = nullptr;                       // (the same)
    decltype(&spt_ao) ao = nullptr;                                   // (the same)
    decltype(&spt_camera_rays) camera_rays = nullptr;                 // (the same)
    decltype(&spt_camera_gbuffer) camera_gbuffer = nullptr;           // (the same)
    decltype(&spt_debug_bxdf) debug_bxdf = nullptr;
    decltype(&spt_debug_render_info) debug_render_info = nullptr;
    decltype(&spt_last_error) last_error = nullptr;
};


struct spt_scene {
    const BezierLib* fwd = nullptr;   // set: `inner` lives in libspt_hip_bez.so and nothing below is used
    spt_scene* inner = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;            // side stream: k_shadow(b) next to k_extend(b) (see bounce); a fused plan's pass pipeline: its bounce launches (trace_window)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // SPT_RENDER_ASYNC: the film stream.  It carries the film's D2H copy next to the following render's kernels and, on the
    // overlapped schedule (trace_window), the tail-loop shade launch, the resolve and the finish kernel of every pass next
    // to the following pass's k_primary.  (No fourth stream: a process gets four hardware queues, the null stream included.)
    hipStream_t stream_film = nullptr;
    hipEvent_t ev_out_ready = nullptr, ev_copy_done = nullptr;
    bool copy_pending = false;                // an asynchronous copy-out of `out` may still be in flight
    // the overlapped schedule, per set of doubled pass buffers (consecutive passes alternate between the sets): "the main stream has finished its part
    // of the pass" and "the film stream has finished the pass"; ev_film_idle: everything queued on the film stream so far
    hipEvent_t ev_main[2] = {nullptr, nullptr}, ev_film[2] = {nullptr, nullptr}, ev_film_idle = nullptr;
    bool film_recorded[2] = {false, false};   // ev_film[k] has been recorded: the set may still be read by the film stream
    uint32_t next_set = 0;                    // the set the next overlapped pass takes: they alternate from pass to pass, across renders too
    int tail_set = -1;                        // >= 0: ev_film[tail_set] covers a tail-loop launch that may still read qb / hit_*_next
    bool film_pending = false;                // the main stream is not yet behind the film-stream kernels of an overlapped render (film_join)
    bool film_inflight = false;               // ... and the host has not waited for them since (grow)
    // the pass pipeline (trace_window): the bounce launches of a pass on stream2 beside the next pass's k_primary on the main stream.  ev_prim[k]: "the
    // main stream has traced the camera rays of the pass in set k"; ev_shade_idle: everything queued on stream2 so far (shade_join)
    hipEvent_t ev_prim[2] = {nullptr, nullptr}, ev_shade_idle = nullptr;
    bool shade_pending = false;               // the main stream is not yet behind the shade stage of a pipelined render (shade_join)
    int ov_mode = 0;                          // the schedule of the overlapped passes still in flight: 1 two streams, 2 the pass pipeline (0: none yet)
    uint64_t passes_film = 0, passes_single = 0;   // spt_debug_render_info: passes resolved on the film stream / on the main stream
    uint64_t passes_pipe = 0;                      // ... and passes whose shade stage ran on stream2 (counted under passes_film too)
    uint64_t passes_cam = 0;                       // ... and passes whose camera rays came from k_primary_cam (camera_kernels.h)
    uint64_t frames_direct = 0;                    // ... and frames whose finish kernel stored into the caller's buffer (no copy-out)
    // ... and what the kernels of a sample-keeping film's last read-out (k_film_filter_box, k_film_filter_weighted) took on the device, in ns, between the
    // two events below (made by the first such film)
    uint64_t keep_read_ns = 0;
    hipEvent_t ev_keep[2] = {nullptr, nullptr};
    bool bez_newton = false;                  // some patch asks for Newton's iteration (the pair kernel only clips)
    // what the last pass with a counter readback saw at bounce 1 (path vertices in all shards); ~0: never seen.  A hint
    // only: it picks between two kernels that compute the same film (k_shade's kLoop)
    uint64_t tail_vertices = ~0ull;
    DScene d{};
    DeviceBuffer tri_pos, tri_attr, instances, meshes, spheres, bezier, surfaces, materials, mediums, lights;
    DeviceBuffer light_props, light_u, light_k, env_px, env_uk, geo;
    bool lds_geo = false;   // traversal geometry small enough to live in LDS (k_*<true>)
    bool swalk = false;     // the streaming walker's tables (stream.h) were built: k_*_stream serve the scene
    size_t lds_bytes = 0;   // dynamic LDS per 256-thread block: traversal stack (+ geometry)
    // render workspace (grown on demand, reused between calls)
    // (counts, rad, first_slot, slot_bits: what the film stream reads of pass p while the main stream writes pass p + 1; set 1
    //  of these four is made by the first overlapped render, or with set 1 of the queues, below: already by the first spt_render of a fused plan)
    DeviceBuffer qa[5], qb[5], hit_f4, hit_inst, hit_f4_next, hit_inst_next, sh[3], counts[2], rad[2], film, first_slot[2], slot_bits[2], out;
    // the pass pipeline's set 1 of the path and hit queues of a fused plan (set 0: the buffers above), made by the first spt_render of such a plan:
    // k_primary of pass p + 1 fills one set while the shade kernels of pass p read and write the other
    DeviceBuffer qa_1[5], qb_1[5], hit_f4_1, hit_inst_1, hit_f4_next_1, hit_inst_next_1;
    bool pipe_warm = false;                   // stream2 and the film stream have run a first command (trace_window)
    uint64_t pipe_refused_bytes = 0;         // != 0: a set of this many bytes was refused (no memory, or the limit): not asked for again at this size or above
    DeviceBuffer trace_in, trace_out, visits, inst_class;
    // spt_denoise_image's workspace, made by its first call and reused: the up to six input images (planar RGB f32) and the
    // page-locked staging buffer they go up through, the records of the a-trous kernels (two colour arrays, guide, albedo), the
    // filtered image and its bytes.  No render and no film touches them
    DeviceBuffer img_in[6], img_color[2], img_guide, img_albedo, img_out, img_out8;
    PinnedBuffer img_stage;
    // spt_radiance's own buffers, made by its first call and reused: the rays (and auxiliary rays) of a pass on the device and the
    // two page-locked slots they go up through, the results of a call with host pointers, and the events that say a slot's copy is done
    DeviceBuffer ray_in, ray_aux_in, ray_rgb, ray_hits;
    DeviceBuffer cam_aux;   // k_primary_cam on a textured scene: the auxiliary rays of a pass, one spt_ray_aux per radiance slot
    PinnedBuffer ray_stage[2];
    hipEvent_t ev_ray[2] = {nullptr, nullptr};
    std::mutex mu;
    double bs_center[3] = {0, 0, 0}, bs_radius = 0;  // bounding sphere of all instance boxes
    double world_lo[3] = {0, 0, 0}, world_hi[3] = {0, 0, 0};   // their union
    bool bs_valid = false;
    // per-row screen-space spans (spt_render): the 8 world-space corners of every instance's OBJECT-space box, the spans of
    // the last camera / image size and their device copy
    std::vector<std::array<double, 24>> hull_corners;
    std::vector<int32_t> span_host;          // 2 per image row: first / last pixel that can see an instance (lo > hi: none)
    std::vector<double> span_key;            // camera + image size the spans were made for
    DeviceBuffer row_span;
    // eye-relative copy of the LDS-resident geometry for k_primary<.., kEye> (eye.h): the plain blob and where its parts are
    // (kept on the host), the copy made for the last camera position and the DScene that describes it
    std::vector<float4> host_blob;
    std::vector<std::pair<uint32_t, uint32_t>> blas_range;   // per mesh: its wide nodes [first, end) in units of 4 float4 behind o_blas
    uint32_t wtlas_f4 = 0;
    bool eye_ok = false, eye_valid = false;
    float eye_key[3] = {0, 0, 0};
    DeviceBuffer eye_geo;
    DScene eye_d{};
    size_t eye_lds_bytes = 0;
    // per-block candidate masks of that copy (k_block_candidates, include/spt_block_cand.h): the copy qualifies when every instance
    // is a triangle mesh and it holds at most 64 triangle slots; the masks of the last window, remade by every render
    bool cand_ok = false;
    DeviceBuffer block_cand;
    // per-origin-triangle candidate sets of the fused simple shade kernels (origin.h, include/spt_origin_cand.h): made on the host
    // from the blob of every committed scene state (origin_table), the device copy always 4 x 64 words; origin_ok: the scene qualifies
    bool origin_ok = false;
    std::vector<uint64_t> origin_words;
    spt_oc_info origin_info{};
    DeviceBuffer origin_cand;
    uint64_t origin_build_ns = 0;   // what the last origin_table took on the host
    bool simple = false;  // Lambert + delta lights only, no emission / environment / media (k_shade<0, .>)
    bool lds_tables = false;  // the shading tables fit LDS behind the geometry (k_shade<.., kTab>)
    bool fused = false;     // k_shade<0, ., kFused> can run: lds_tables and a simple scene
    bool subsurface = false;  // the heavy shade levels are needed: some material has a Subsurface substrate (probe) and / or glints
    bool has_probe = false;   // ... a Subsurface substrate: k_shade<3 | 5, .> (the BSSRDF probe walks the BVH inside the shade kernel)
    bool has_pndf = false;    // ... a position-normal distribution: k_shade<4 | 5, .> (tree walks with private stacks)
    DeviceBuffer ss_cdf;
    DeviceBuffer pndfs, pndf_terms, pndf_nodes, pndf_refs, pndf_roots;   // position-normal distributions (k_shade<3, .> too)
    bool textured = false;  // a material recipe, normal map or emissive map samples textures per hit (k_shade<2, .>)
    DeviceBuffer textures, tex_prog, tex_root, tex_chain, images, image_levels, texels, recipes;
    std::vector<hipEvent_t> events;
    // spt_scene_update: the creation's fixed part, the films alive on the scene, the page-locked slot the dynamic part goes up
    // through and the event that says the slot's copies are done; what spt_debug_render_info reports of the updates
    SceneFixed fixed;
    uint32_t live_films = 0;
    PinnedBuffer upd_stage;
    hipEvent_t ev_upd = nullptr;
    bool upd_recorded = false;
    uint64_t updates = 0, update_bytes = 0;
    // spt_scene_deform on a large scene, made by its first call: the refit's raw bounds and height per BLAS node, and per mesh
    // whether its nodes' heights have been derived (k_refit_heights)
    DeviceBuffer refit_raw, refit_height;
    std::vector<uint8_t> refit_heights_known;
    hipEvent_t ev_deform[2] = {nullptr, nullptr};   // around the copies and kernels of the last call that named meshes (counter 6)
    bool deform_timed = false;
    // spt_scene_mesh_topology: per mesh its registration (null: none) - the host copy the checks and an LDS-resident scene's
    // host assembly read, and the device arrays the kernels of inst_assemble.hip read and write
    struct MeshTopology {
        uint32_t n_vertices = 0, tri_count = 0;
        std::vector<uint32_t> indices, face_of_tri, corner_first, corners;
        std::vector<uint8_t> named;       // per vertex: some face names it (an empty row of the table; the bounds pass reads it)
        std::vector<float> uv, normals;   // normals: the ones in force (the registration's, then the last ones a deformation gave)
        DeviceBuffer d_indices, d_face_of_tri, d_corner_first, d_corners, d_uv, d_normals, d_positions, d_tan, d_bit;
    };
    std::vector<std::unique_ptr<MeshTopology>> topology;
    ~spt_scene() {
        if (fwd) { fwd->destroy(inner); return; }
        (void)hipSetDevice(device);
        for (auto e : events) (void)hipEventDestroy(e);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (ev_out_ready) (void)hipEventDestroy(ev_out_ready);
        if (ev_copy_done) (void)hipEventDestroy(ev_copy_done);
        for (auto e : {ev_main[0], ev_main[1], ev_film[0], ev_film[1], ev_film_idle, ev_prim[0], ev_prim[1], ev_shade_idle, ev_keep[0], ev_keep[1], ev_ray[0], ev_ray[1], ev_upd, ev_deform[0], ev_deform[1]})
            if (e) (void)hipEventDestroy(e);
        if (stream_film) (void)hipStreamDestroy(stream_film);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// A film object (spt_film_*, ABI v14): one shard's running sums of a fixed plan on the scene's device, which every
// spt_film_render extends by the next samples.  Its buffers are its own: spt_render's film / out (which an asynchronous
// copy-out may still be reading) are never touched, the render workspace is shared under the scene's lock.
struct spt_film {
    const BezierLib* fwd = nullptr;   // set: `inner` is a film of libspt_hip_bez.so and nothing below is used
    spt_film* inner = nullptr;
    spt_scene* sc = nullptr;
    spt_camera cam{};
    spt_camera_model model{};         // type != SPT_CAMERA_PERSPECTIVE: the film's camera model (spt_film_create_camera); cam == model.base
    spt_render_params plan{};
    uint32_t first = 0, done = 0;     // covers the plan's samples [first, first + done)
    uint32_t flags = 0;               // SPT_FILM_*
    uint32_t rows = 0;                // image rows of the shard
    float radius = 0.5f;
    int32_t R = 0;                    // ceil(radius - 0.5) <= 0
    DeviceBuffer sum, sq, out;        // S, Q (SPT_FILM_MOMENTS) and the read-out staging buffer, rows * width * 3 f32 each
    DeviceBuffer out8;                // spt_film_read_rgb8: the bytes of the staging buffer (k_pack_rgb8), rows * width * 3 u8
    // adaptive sampling (spt_film_adapt), made by its first call that can retire pixels; until then the film is a plain one
    bool adaptive = false;
    DeviceBuffer mask;                // per pixel u8: 1 active, 0 retired
    DeviceBuffer counts;              // per pixel u32: the samples a retired pixel covers (n_p; an active pixel covers `done`)
    DeviceBuffer tile_active;         // per 16x16 tile of the shard (k_primary's numbering) u32: active pixels after the last adapt
    DeviceBuffer totals;              // 2 u32 of k_film_adapt: active pixels, tiles with any
    DeviceBuffer inv;                 // (spp + 1) f32: inv[k] = 1.0f / (float)k as the host rounds it (inv[0] = 0, never read)
    uint32_t active = 0, active_tiles = 0;
    // spt_film_denoise's workspace, made by its first call: two colour arrays (ping-pong) and the guide array, one float4 per pixel;
    // the albedo array by the first spt_film_denoise_job with an albedo film
    DeviceBuffer dn_color[2], dn_guide, dn_albedo;
    // bucket sums (spt_film_buckets): n_buckets planes of rows * width * 3 f32, and the reciprocal table of the robust read-outs
    uint32_t n_buckets = 0;           // K; 0: a film without buckets
    DeviceBuffer buckets;             // B_j, j = 0 .. K - 1
    DeviceBuffer b_inv;               // (spp + 1) f32: inv[k] = 1.0f / (float)k as the host rounds it (inv[0] = 0, never read)
    // a film that keeps its samples (SPT_FILM_KEEP_SAMPLES): no running sums; per run of consecutive own rows the radiance of every
    // covered sample of the run's stored rows (own rows + R halo rows each way, clipped to the image), one chunk per wavefront pass
    struct KeptRun {
        uint32_t j0 = 0, j1 = 0;      // own image rows [j0, j1)
        uint32_t b0 = 0, b1 = 0;      // stored image rows [b0, b1)
        size_t out_row = 0;           // the run's first own row in the shard's packed rows
        std::vector<std::unique_ptr<DeviceBuffer>> chunks;   // 3 planes [c][sample in pass][stored pixel] each
        std::vector<KeptChunk> table;                        // what the kernels read of them, and its device copy
        DeviceBuffer table_dev;
    };
    std::deque<KeptRun> runs;       // (a KeptRun does not move: it owns device buffers)
    // the reconstruction filter of the read-outs (spt_film_filter); SPT_FILTER_BOX: the reference's box at the plan's radius
    uint32_t filter_type = SPT_FILTER_BOX;
    float filter_radius = 0.5f;       // r
    int32_t filter_R = 0;             // Rf = max(ceil(r - 0.5), 0) <= max(R, 0)
    FilterCoef filter_coef{};
};

namespace {

// The host side of a committed SceneDynamic: the DScene fields, the kernel choices and the caches that depend on the instances
// (the device copies are the caller's business: spt_scene_create uploads, spt_scene_update queues copies on the render stream)
void dyn_commit_host(spt_scene* sc, SceneDynamic& dy, bool lds_geo) {
    DScene& d = sc->d;
    d.n_tlas_nodes = dy.n_tlas_nodes;
    d.stack_cap = dy.stack_cap;
    d.tlas_root = dy.tlas_root;
    d.s_root = dy.s_root;
    d.flat = dy.flat;
    for (int k = 0; k < 3; ++k) { d.tlas_lo[k] = dy.tlas_lo[k]; d.tlas_hi[k] = dy.tlas_hi[k]; }
    d.o_sinst = dy.o_sinst; d.o_tlas = dy.o_tlas; d.o_inst = dy.o_inst; d.o_mesh = dy.o_mesh; d.o_sph = dy.o_sph; d.o_blas = dy.o_blas;
    d.o_tri = dy.o_tri; d.o_tord = dy.o_tord; d.o_attr = dy.o_attr; d.o_surf = dy.o_surf; d.o_mat = dy.o_mat; d.o_light = dy.o_light;
    d.geo_f4 = dy.geo_f4;
    d.lds_f4 = lds_geo ? d.geo_f4 : 0u;   // large scene: global fetches only (see trace.h)
    sc->lds_bytes = kStackBytes + (size_t)d.lds_f4 * 16;
    sc->swalk = dy.swalk;
    sc->lds_tables = dy.lds_tables;
    sc->fused = dy.fused;
    sc->simple = dy.simple;
    sc->eye_ok = dy.eye_ok;
    sc->eye_valid = false;      // (its key is the eye position alone)
    sc->span_key.clear();       // (... the camera and the image size)
    if (dy.eye_ok) {
        sc->host_blob = dy.blob;
        sc->wtlas_f4 = (uint32_t)dy.wtlas.size();
    } else {
        sc->host_blob.clear();
    }
    for (int k = 0; k < 3; ++k) { sc->bs_center[k] = dy.bs_center[k]; sc->world_lo[k] = dy.world_lo[k]; sc->world_hi[k] = dy.world_hi[k]; }
    sc->bs_radius = dy.bs_radius;
    sc->bs_valid = dy.bs_valid;
    sc->hull_corners = std::move(dy.hull_corners);
}

// The origin-candidate table of the scene state `dy` (include/spt_origin_cand.h), from the blob the device stages: the instances'
// matrices, the slots' (p0, e1, e2, id) and the vertex normals of the shading tables behind the geometry.  False - no table - unless
// the state is served by the fused simple kernels with an eye-relative copy (every mesh used by one instance, so a triangle id names
// one world triangle), every instance is a triangle mesh and the blob holds at most 64 slots: the preconditions of the block masks.
bool origin_table(const SceneDynamic& dy, uint32_t n_instances, uint32_t n_meshes, std::vector<uint64_t>& words, spt_oc_info& info) {
    if (!dy.fused || !dy.simple || !dy.eye_ok || dy.o_attr == 0u || n_instances == 0u || dy.blob.size() < dy.geo_f4) return false;
    const float4* const b = dy.blob.data();
    auto as_u = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    std::vector<spt_oc_instance> inst(n_instances);
    std::vector<spt_oc_triangle> tri;
    std::vector<uint8_t> mesh_used(n_meshes, 0);
    for (uint32_t i = 0; i < n_instances; ++i) {
        float rec[48];
        std::memcpy(rec, &b[dy.o_inst + 12u * i], sizeof(rec));
        std::memcpy(inst[i].inv, rec, sizeof inst[i].inv);
        std::memcpy(inst[i].fwd, rec + 12, sizeof inst[i].fwd);
        std::memcpy(inst[i].nrm, rec + 24, sizeof inst[i].nrm);
        const uint32_t prim_type = as_u(rec[33]), mesh = as_u(rec[34]);
        if (prim_type != SPT_PRIM_MESH || mesh >= n_meshes || mesh_used[mesh]) return false;
        mesh_used[mesh] = 1;
        const uint32_t range = as_u(b[dy.o_mesh + 2u * mesh + 1u].w);
        const uint32_t first = range & 0xffffu, count = range >> 16;
        if (first + count > SPT_OC_MAX_TRIS) return false;
        if (tri.size() < first + count) tri.resize(first + count, spt_oc_triangle{{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, ~0u, ~0u});
        for (uint32_t k = first; k < first + count; ++k) {
            const float4 a = b[dy.o_tri + 3u * k], e1 = b[dy.o_tri + 3u * k + 1u], e2 = b[dy.o_tri + 3u * k + 2u];
            spt_oc_triangle& t = tri[k];
            t.p0[0] = a.x; t.p0[1] = a.y; t.p0[2] = a.z;
            t.e1[0] = e1.x; t.e1[1] = e1.y; t.e1[2] = e1.z;
            t.e2[0] = e2.x; t.e2[1] = e2.y; t.e2[2] = e2.z;
            t.instance = i;
            t.id = as_u(a.w);
            if (t.id >= SPT_OC_MAX_TRIS || (size_t)dy.o_attr + 9u * t.id + 3u > dy.blob.size()) return false;
            std::memcpy(t.n, &b[dy.o_attr + 9u * t.id], sizeof t.n);   // spt_tri_attr: the three vertex normals come first
        }
    }
    for (const spt_oc_triangle& t : tri)
        if (t.instance == ~0u) return false;   // a slot of a mesh no instance uses
    words.assign((size_t)SPT_OC_WORDS * SPT_OC_MAX_TRIS, 0ull);
    return spt_oc_build(inst.data(), n_instances, tri.data(), (uint32_t)tri.size(), words.data(), &info);
}

// ... installed as the scene's (host side; the caller copies sc->origin_words to sc->origin_cand where origin_ok)
void origin_install(spt_scene* sc, const SceneDynamic& dy, uint32_t n_instances, uint32_t n_meshes) {
    const auto t0 = std::chrono::steady_clock::now();
    sc->origin_ok = origin_table(dy, n_instances, n_meshes, sc->origin_words, sc->origin_info);
    sc->origin_build_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}
constexpr size_t kOriginBytes = (size_t)SPT_OC_WORDS * SPT_OC_MAX_TRIS * sizeof(uint64_t);

uint32_t shard_row_count(const spt_render_params& p) {
    uint32_t sc = p.shard_count ? p.shard_count : 1u, sr = p.strip_rows ? p.strip_rows : 1u;
    uint32_t rows = 0;
    for (uint32_t j = 0; j < p.height; ++j)
        if ((j / sr) % sc == p.shard_index) ++rows;
    return rows;
}

// Grid of the queue kernels (grid-stride over a queue shard).  Sizing it to exactly the resident workgroups of
// each kernel (hipOccupancyMaxActiveBlocksPerMultiprocessor: 768 for the 144-VGPR fused shade kernel) was MEASURED
// no better (cfg2 60.5 / 61.8 / 62.1 Gsamples/s for 1 / 2 / 3 resident rounds vs 62.4 with this fixed grid, cfg4 4.49
// vs 4.61): items cost very different amounts, so more, smaller work shares balance better than an exact fit.
constexpr uint32_t kPersistentBlocks = 2048;
// bounce-1 vertices per pass below which the fused pipeline stops launching per bounce (a lane that loops over its path
// wastes the lanes whose paths ended; with this few vertices that costs microseconds, the launches it saves ~0.1 ms)
constexpr uint64_t kTailLoopBelow = 4ull << 20;

}  // namespace

extern "C" uint32_t spt_abi_version(void);

#if !SPT_WITH_BEZIER
namespace {
const BezierLib* bezier_lib() {
    static BezierLib lib;
    static std::once_flag once;
    static std::string err;
    std::call_once(once, [] {
        Dl_info info;
        if (!dladdr(reinterpret_cast<void*>(&spt_abi_version), &info) || !info.dli_fname) { err = "dladdr failed"; return; }
        std::string path(info.dli_fname);
        const size_t slash = path.find_last_of('/');
        path = (slash == std::string::npos ? std::string() : path.substr(0, slash + 1)) + "libspt_hip_bez.so";
        void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) { const char* e = dlerror(); err = e ? e : "dlopen failed"; return; }
        auto sym = [h](auto& fn, const char* name) {   // true: the library exports `name`
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name));
            return fn != nullptr;
        };
        decltype(&spt_abi_version) version = nullptr;
        const bool all = sym(lib.create, "spt_scene_create") && sym(lib.destroy, "spt_scene_destroy") && sym(lib.render, "spt_render") &&
                         sym(lib.render_wait, "spt_render_wait") && sym(lib.film_create, "spt_film_create") && sym(lib.film_render, "spt_film_render") &&
                         sym(lib.film_samples, "spt_film_samples") && sym(lib.film_read, "spt_film_read") && sym(lib.film_destroy, "spt_film_destroy") &&
                         sym(lib.film_adapt, "spt_film_adapt") && sym(lib.film_read_counts, "spt_film_read_counts") &&
                         sym(lib.film_denoise, "spt_film_denoise") && sym(lib.film_denoise_job, "spt_film_denoise_job") && sym(lib.film_buckets, "spt_film_buckets") &&
                         sym(lib.film_read_buckets, "spt_film_read_buckets") && sym(lib.film_read_robust, "spt_film_read_robust") &&
                         sym(lib.film_read_rgb8, "spt_film_read_rgb8") && sym(lib.film_read_samples, "spt_film_read_samples") &&
                         sym(lib.denoise_image, "spt_denoise_image") &&
                         sym(lib.trace_closest, "spt_trace_closest") && sym(lib.trace_any, "spt_trace_any") && sym(lib.radiance, "spt_radiance") && sym(lib.debug_bxdf, "spt_debug_bxdf") &&
                         sym(lib.debug_render_info, "spt_debug_render_info") &&
                         sym(lib.last_error, "spt_last_error") && sym(version, "spt_abi_version");
        (void)sym(lib.film_filter, "spt_film_filter");
        (void)sym(lib.scene_update, "spt_scene_update");
        (void)sym(lib.scene_deform, "spt_scene_deform");
        (void)sym(lib.scene_mesh_topology, "spt_scene_mesh_topology");
        (void)sym(lib.scene_deform_vertices, "spt_scene_deform_vertices");
        (void)sym(lib.scene_read_triangles, "spt_scene_read_triangles");
        (void)sym(lib.render_camera, "spt_render_camera");
        (void)sym(lib.film_create_camera, "spt_film_create_camera");
        (void)sym(lib.bake, "spt_bake");
        (void)sym(lib.probe, "spt_probe");
        (void)sym(lib.gbuffer, "spt_gbuffer");
        (void)sym(lib.occluded, "spt_occluded");
        (void)sym(lib.ao, "spt_ao");
        (void)sym(lib.camera_rays, "spt_camera_rays");
        (void)sym(lib.camera_gbuffer, "spt_camera_gbuffer");
        if (!all || version() != SPT_ABI_VERSION) {
            err = path + " does not export ABI version " + std::to_string(SPT_ABI_VERSION);
            return;
        }
        lib.handle = h;
    });
    if (!lib.handle) fail(SPT_ERR_UNSUPPORTED, "the scene has Bezier patches and libspt_hip_bez.so could not be loaded: " + err);
    return &lib;
}
}  // namespace
#endif

namespace {
// The body of a C entry point: an AbiError becomes its status and message, any other exception (std::bad_alloc of a host
// buffer, ...) SPT_ERR_OUT_OF_MEMORY with "<who>: what()".  Nothing leaves through the C ABI.
template <class Body>
spt_status guarded(const char* who, Body&& body) {
    try {
        return body();
    } catch (const AbiError& e) {
        g_error = e.msg;
        return e.code;
    } catch (const std::exception& e) {
        g_error = std::string(who) + ": " + e.what();
        return SPT_ERR_OUT_OF_MEMORY;
    }
}

// The status of a call passed through to libspt_hip_bez.so (see BezierLib), whose message becomes this library's on failure
spt_status forwarded(const BezierLib* lib, spt_status st) {
    if (st != SPT_OK) g_error = lib->last_error();
    return st;
}

// What the environment asks of the scene builder, and what this library was compiled with
BuildOptions build_options() {
    BuildOptions opt = BuildOptions::from_env();
    opt.with_bezier = SPT_WITH_BEZIER != 0;
    return opt;
}

// spt_scene_create of a scene with patch instances in the plain library: the scene of libspt_hip_bez.so behind a forwarding
// object (see BezierLib); nullptr: the scene is this library's own
spt_scene* forward_to_bezier_lib(const spt_scene_desc& desc, int32_t device) {
#if !SPT_WITH_BEZIER
    bool has_patch_instance = false;   // a patch that no instance uses (a primitives library) does not count
    if (desc.n_bezier_patches > 0 && desc.instances)
        for (uint32_t i = 0; i < desc.n_instances && !has_patch_instance; ++i) has_patch_instance = desc.instances[i].prim_type == SPT_PRIM_BEZIER;
    if (has_patch_instance) {
        const BezierLib* lib = bezier_lib();
        spt_scene* inner = nullptr;
        const spt_status st = lib->create(&desc, device, &inner);
        if (st != SPT_OK) fail(st, lib->last_error());
        auto sc = std::make_unique<spt_scene>();
        sc->fwd = lib;
        sc->inner = inner;
        return sc.release();
    }
#else
    (void)desc; (void)device;
#endif
    return nullptr;
}

// A scene object on `device` with its streams and events and nothing else
std::unique_ptr<spt_scene> open_device(int32_t device) {
    int n = usable_device_count();
    if (n <= 0) fail(SPT_ERR_NO_DEVICE, "no HIP device is visible: libspt_hip has no CPU fallback");
    if (device < 0 || device >= n) fail(SPT_ERR_NO_DEVICE, "device index out of range");
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        fail(SPT_ERR_NO_DEVICE, std::string("device is '") + prop.gcnArchName + "', the kernels are built for gfx950 only");
    HIP_CHECK(hipSetDevice(device));
    auto sc = std::make_unique<spt_scene>();
    sc->device = device;
    HIP_CHECK(hipStreamCreateWithFlags(&sc->stream, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&sc->stream2, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&sc->stream_film, hipStreamNonBlocking));
    for (hipEvent_t* e : {&sc->ev_main[0], &sc->ev_main[1], &sc->ev_film[0], &sc->ev_film[1], &sc->ev_film_idle, &sc->ev_out_ready, &sc->ev_copy_done,
                          &sc->ev_fork, &sc->ev_join, &sc->ev_prim[0], &sc->ev_prim[1], &sc->ev_shade_idle})
        HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return sc;
}

// The traversal blob: allocated for what an update may write, filled with what the creation built
void upload_geometry(spt_scene* sc, const spt_scene_desc& s, StaticBuild& sb, const SceneDynamic& dy) {
    SceneFixed& fx = sb.fixed;
    // the allocation holds what an update may write: 64 KB of an LDS-resident blob; behind a large scene's static sections
    // the dynamic ones of any tree over n instances (4-wide TLAS <= 4 (n - 1), entries 6 n, 2-wide TLAS <= 4 n + 4,
    // records 12 n, order n / 4 float4), or what the caller's tree takes now if that is more
    if (fx.n4) {
        const size_t n = s.n_instances;
        fx.tail_cap = (uint32_t)std::min<size_t>(0x7fffffffu, std::max<size_t>((size_t)dy.geo_f4 - fx.tail_first, 4 * n + 6 * n + 4 * n + 4 + 12 * n + (n + 3) / 4));
    }
    const size_t geo_bytes = fx.n4 ? ((size_t)fx.tail_first + fx.tail_cap) * 16 : std::max<size_t>(dy.blob.size() * 16, 64u * 1024u);
    sc->geo.alloc(std::max<size_t>(geo_bytes, 16));
    if (!dy.blob.empty()) HIP_CHECK(hipMemcpy(sc->geo.p, dy.blob.data(), dy.blob.size() * 16, hipMemcpyHostToDevice));
    sc->d.geo = sc->geo.as<float4>();
}

// The tables only some scenes' shade kernels read: position-normal distributions, the BSSRDF radius table, textures
void upload_shading_tables(spt_scene* sc, const spt_scene_desc& s, const StaticBuild& sb) {
    DScene& d = sc->d;
    if (sb.has_pndf) {
        sc->pndfs.upload(s.pndfs, s.n_pndfs);
        sc->pndf_terms.upload(s.pndf_terms, s.n_pndf_terms);
        sc->pndf_nodes.upload(s.pndf_nodes, s.n_pndf_nodes);
        sc->pndf_refs.upload(s.pndf_refs, s.n_pndf_refs);
        sc->pndf_roots.upload(s.pndf_roots, s.n_pndf_roots);
        d.pndfs = sc->pndfs.as<spt_pndf>();
        d.pndf_terms = sc->pndf_terms.as<spt_pndf_term>();
        d.pndf_nodes = sc->pndf_nodes.as<spt_pndf_node>();
        d.pndf_refs = sc->pndf_refs.as<uint32_t>();
        d.pndf_roots = sc->pndf_roots.as<uint32_t>();
    }
    if (sb.subsurface) {
        sc->ss_cdf.upload(sb.ss_cdf.data(), sb.ss_cdf.size());
        d.ss_cdf = sc->ss_cdf.as<float2>();
    }
    if (sb.textured) {
        sc->textures.upload(s.textures, s.n_textures);
        sc->tex_prog.upload(sb.tex.prog.data(), sb.tex.prog.size());
        sc->tex_root.upload(sb.tex.roots.data(), sb.tex.roots.size());
        sc->tex_chain.upload(sb.tex.chain.data(), sb.tex.chain.size());
        sc->images.upload(s.images, s.n_images);
        sc->image_levels.upload(s.image_levels, s.n_image_levels);
        sc->texels.upload(s.texels, s.n_texels);
        sc->recipes.upload(s.material_recipes, s.n_material_recipes);
        d.textures = sc->textures.as<float4>();
        d.tex_prog = sc->tex_prog.as<uint4>();
        d.tex_root = sc->tex_root.as<uint2>();
        d.tex_chain = sc->tex_chain.as<uint32_t>();
        d.images = sc->images.as<uint2>();
        d.image_levels = sc->image_levels.as<uint4>();
        d.texels = sc->texels.as<uint32_t>();
        d.recipes = sc->recipes.as<uint4>();
    }
}

// Everything of a new scene that lives on the device: every array of the descriptor and of the two builds goes up, every DScene
// pointer and count is set (the offsets and choices that follow the instances: dyn_commit_host).  Takes sb.fixed into the scene.
void upload_scene(spt_scene* sc, const spt_scene_desc& s, StaticBuild& sb, const SceneDynamic& dy) {
    DScene& d = sc->d;
    sc->tri_pos.upload(s.tri_pos, s.n_tris);
    sc->tri_attr.upload(s.tri_attr, s.n_tris);
    sc->instances.upload(s.instances, s.n_instances);
    sc->meshes.upload(s.meshes, s.n_meshes);
    sc->spheres.upload(s.spheres, s.n_spheres);
    sc->bezier.upload(s.bezier_patches, s.n_bezier_patches);
    sc->surfaces.upload(s.surfaces, s.n_surfaces);
    sc->materials.upload(s.materials, s.n_materials);
    sc->mediums.upload(s.mediums, s.n_mediums);
    sc->lights.upload(s.lights, s.n_lights);
    const bool pis = s.light_sampler == SPT_LIGHT_SAMPLER_POWER_IS;
    sc->light_props.upload(s.light_alias.props, pis ? s.n_lights : 0);
    sc->light_u.upload(s.light_alias.u, pis ? s.n_lights : 0);
    sc->light_k.upload(s.light_alias.k, pis ? s.n_lights : 0);
    sc->env_px.upload(sb.env_px.data(), sb.env_px.size());
    sc->env_uk.upload(sb.env_uk.data(), sb.env_uk.size());
    sc->inst_class.upload(dy.cls.data(), dy.cls.size());
    d.tri_pos = sc->tri_pos.as<float4>();
    d.tri_attr = sc->tri_attr.as<float4>();
    d.instances = sc->instances.as<float4>();
    d.meshes = sc->meshes.as<uint4>();
    d.spheres = sc->spheres.as<float4>();
    d.bez = sc->bezier.as<float4>();
    d.surfaces = sc->surfaces.as<spt_surface>();
    d.materials = sc->materials.as<spt_material>();
    d.mediums = sc->mediums.as<spt_medium>();
    d.lights = sc->lights.as<spt_light>();
    d.light_props = sc->light_props.as<float>();
    d.light_u = sc->light_u.as<float>();
    d.light_k = sc->light_k.as<uint32_t>();
    d.env_px = sc->env_px.as<float4>();
    d.env_uk = sc->env_uk.as<uint2>();
    d.inst_class = sc->inst_class.as<uint8_t>();
    d.n_instances = s.n_instances;
    d.n_lights = s.n_lights;
    d.n_meshes = s.n_meshes;
    d.aggregate = s.aggregate;
    d.light_sampler = s.light_sampler;
    d.env_light_index = s.env_light_index;
    d.env_w = s.env.width;
    d.env_h = s.env.height;
    for (int i = 0; i < 3; ++i) d.env_scale[i] = s.env.scale[i];
    d.fast_slab = sb.fixed.own_bvh ? 1u : 0u;
    upload_geometry(sc, s, sb, dy);
    upload_shading_tables(sc, s, sb);
    sc->lds_geo = sb.lds_geo;
    sc->blas_range = std::move(sb.blas_range);
    sc->bez_newton = sb.bez_newton;
    sc->subsurface = sb.subsurface;
    sc->has_probe = sb.has_probe;
    sc->has_pndf = sb.has_pndf;
    sc->textured = sb.textured;
    sc->fixed = std::move(sb.fixed);
}
}  // namespace

extern "C" {

const char* spt_last_error(void) { return g_error.c_str(); }
uint32_t spt_abi_version(void) { return SPT_ABI_VERSION; }

spt_status spt_device_count(int32_t* count) {
    if (!count) { g_error = "device_count: null argument"; return SPT_ERR_INVALID_ARG; }
    *count = usable_device_count();
    return SPT_OK;
}

spt_status spt_shard_rows(const spt_render_params* params, uint32_t* rows) {
    if (!params || !rows) { g_error = "shard_rows: null argument"; return SPT_ERR_INVALID_ARG; }
    *rows = shard_row_count(*params);
    return SPT_OK;
}

spt_status spt_scene_create(const spt_scene_desc* desc, int32_t device, spt_scene** out) {
    if (!desc || !out) { g_error = "scene_create: null argument"; return SPT_ERR_INVALID_ARG; }
    *out = nullptr;
    return guarded("scene_create", [&] {
        if (spt_scene* passed_on = forward_to_bezier_lib(*desc, device)) {
            *out = passed_on;
            return SPT_OK;
        }
        const BuildOptions opt = build_options();
        validate(*desc, opt);
        std::unique_ptr<spt_scene> sc = open_device(device);
        StaticBuild sb = build_static(*desc, opt);
        const StaticSections st = sb.sections();
        SceneDynamic dy = build_dynamic(sb.fixed, dyn_view(*desc, sb.fixed.surf_emissive.data()), opt, sb.lds_geo, sb.blas_range.size(), &st);
        upload_scene(sc.get(), *desc, sb, dy);
        origin_install(sc.get(), dy, desc->n_instances, desc->n_meshes);
        sc->origin_cand.alloc(kOriginBytes);
        if (sc->origin_ok) HIP_CHECK(hipMemcpy(sc->origin_cand.p, sc->origin_words.data(), kOriginBytes, hipMemcpyHostToDevice));
        dyn_commit_host(sc.get(), dy, sc->lds_geo);
        *out = sc.release();
        return SPT_OK;
    });
}

void spt_scene_destroy(spt_scene* scene) {
    if (!scene) return;
    (void)hipSetDevice(scene->device);
    (void)hipStreamSynchronize(scene->stream);
    if (scene->stream2) (void)hipStreamSynchronize(scene->stream2);
    if (scene->stream_film) (void)hipStreamSynchronize(scene->stream_film);
    // every DeviceBuffer member frees itself (a list here used to miss the buffers added later)
    delete scene;
}

}  // extern "C"

// eye.h: the copy of the LDS-resident geometry relative to the camera position `eye` (every value by the f32 operations, in the
// order, in which the walkers of trace.h compute it per ray - this file is compiled with FP contraction off like the kernels),
// uploaded behind the work already queued on the scene's stream.
static void make_eye_blob(spt_scene* sc, const float eye[3]) {
    const DScene& d = sc->d;
    std::vector<float4> eb = sc->host_blob;
    auto sub3 = [](float4& v, const float o[3]) { v.x = v.x - o[0]; v.y = v.y - o[1]; v.z = v.z - o[2]; };
    auto as_u = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    uint32_t n_tris = 0;
    for (uint32_t m = 0; m < d.n_meshes; ++m) {
        const uint32_t range = as_u(eb[d.o_mesh + 2u * m + 1u].w);
        n_tris = std::max(n_tris, (range & 0xffffu) + (range >> 16));
    }
    const uint32_t o_eye = (uint32_t)eb.size();
    eb.resize(eb.size() + n_tris, make_float4(0, 0, 0, 0));
    sc->cand_ok = n_tris <= SPT_BC_MAX_TRIS && d.n_instances > 0u;
    for (uint32_t i = 0; i < sc->wtlas_f4; ++i) sub3(eb[d.o_tlas + i], eye);                 // TLAS nodes: world space
    for (uint32_t i = 0; i < d.n_instances; ++i) {
        float rec[48];
        std::memcpy(rec, &eb[d.o_inst + 12u * i], sizeof(rec));
        const float* m = rec;                                                                 // spt_instance::inv
        const uint32_t prim_type = as_u(rec[33]), prim_id = as_u(rec[34]);
        if (prim_type != SPT_PRIM_MESH) sc->cand_ok = false;
        float oo[3];                                                                          // xf_point(inv, eye)
        for (int k = 0; k < 3; ++k) oo[k] = ((m[k] * eye[0] + m[3 + k] * eye[1]) + m[6 + k] * eye[2]) + m[9 + k];
        if (prim_type == SPT_PRIM_SPHERE) {                                                   // oc = o' - c, in pad[1..3] of the instance record
            const float4 sp = eb[d.o_sph + prim_id];
            float4& pad = eb[d.o_inst + 12u * i + 11u];
            pad.x = oo[0] - sp.x; pad.y = oo[1] - sp.y; pad.z = oo[2] - sp.z;
            continue;
        }
        sub3(eb[d.o_mesh + 2u * prim_id], oo);                                                // root box of the BLAS
        sub3(eb[d.o_mesh + 2u * prim_id + 1u], oo);
        for (uint32_t n = 4u * sc->blas_range[prim_id].first; n < 4u * sc->blas_range[prim_id].second; ++n) sub3(eb[d.o_blas + n], oo);
        const uint32_t range = as_u(eb[d.o_mesh + 2u * prim_id + 1u].w);
        for (uint32_t k = range & 0xffffu; k < (range & 0xffffu) + (range >> 16); ++k) {
            float4& a = eb[d.o_tri + 3u * k];
            const float4 e1 = eb[d.o_tri + 3u * k + 1u], e2 = eb[d.o_tri + 3u * k + 2u];
            const float sx = oo[0] - a.x, sy = oo[1] - a.y, sz = oo[2] - a.z;                 // s = o' - p0
            const float rx = sy * e1.z - sz * e1.y, ry = sz * e1.x - sx * e1.z, rz = sx * e1.y - sy * e1.x;   // cross(s, e1)
            const float c = (e2.x * rx + e2.y * ry) + e2.z * rz;                              // dot(e2, s x e1)
            a.x = sx; a.y = sy; a.z = sz;
            eb[o_eye + k] = make_float4(rx, ry, rz, c);
        }
    }
    sc->eye_geo.ensure(eb.size() * 16);
    HIP_CHECK(hipMemcpyAsync(sc->eye_geo.p, eb.data(), eb.size() * 16, hipMemcpyHostToDevice, sc->stream));
    HIP_CHECK(hipStreamSynchronize(sc->stream));   // `eb` is pageable; once per camera position
    sc->eye_d = sc->d;
    sc->eye_d.geo = sc->eye_geo.as<float4>();
    sc->eye_d.geo_f4 = sc->eye_d.lds_f4 = (uint32_t)eb.size();
    sc->eye_d.o_eye = o_eye;
    for (int k = 0; k < 3; ++k) { sc->eye_d.tlas_lo[k] = sc->d.tlas_lo[k] - eye[k]; sc->eye_d.tlas_hi[k] = sc->d.tlas_hi[k] - eye[k]; }
    sc->eye_lds_bytes = sc->lds_bytes - (size_t)sc->d.lds_f4 * 16 + eb.size() * 16;
    for (int k = 0; k < 3; ++k) sc->eye_key[k] = eye[k];
    sc->eye_valid = true;
}

namespace {

uint32_t env_u32(const char* name, uint32_t dflt) { const char* v = std::getenv(name); return v ? (uint32_t)std::atoi(v) : dflt; }

// The samples one run of the pass loop adds, and where it adds them: spt_render sums [0, spp) of its plan into the scene's
// workspace film, zeroed first; a film object (spt_film_render) adds its next increment to its own sums as they stand.
struct SampleTarget {
    uint32_t first, count;   // the plan's samples [first, first + count)
    float* sum;              // window pixels * 3 running sums on the device; null: the scene's workspace film (sc->film)
    float* sq;               // SPT_FILM_MOMENTS: the running sums of the squares (k_resolve*<., true>); null: none
    bool zero;               // zero the sums before the first pass
    // an adaptive film (spt_film_adapt): only its active pixels are traced (k_primary*<..., kMask>); null: every pixel
    FilmMask mask{nullptr, nullptr};
    uint32_t mask_tiles = 0;  // tiles with an active pixel after the last adapt: what the primary chunk count is sized for
    // a bucketed film (spt_film_buckets): its K bucket sums, `bucket_plane` floats apart (k_resolve_buckets); null: none
    float* buckets = nullptr;
    uint32_t n_buckets = 0;
    size_t bucket_plane = 0;
    // a sample-keeping film (collect): the radiance chunk of every pass of this call, sized by pass_samples_of and zeroed by the
    // caller; the passes write there, not to the scene's sc->rad.  null: the scene's workspace
    float* const* keep = nullptr;
};

// One call of the render loop: its plan, the kernel choices made once per call (run_setup), the profiling spans and the
// counters that become spt_render_stats (spt_render with stats only).
struct RenderRun {
    spt_scene* sc = nullptr;
    const spt_camera* cam = nullptr;
    const spt_camera_model* model = nullptr;   // a non-perspective camera model (cam == &model->base); null: the pinhole
    const spt_render_params* params = nullptr;
    spt_render_stats* stats = nullptr;
    hipStream_t st = nullptr;
    bool profile = false, count = false, overlap = false, L = false, use_eye = false, dyn_shadow = false, dyn_extend = false;
    bool use_cand = false;       // k_primary<..., BlockCand>: camera rays against the per-block candidate masks of the eye-relative copy
    bool fused = false;          // k_shade<0, ., kFused>: shade, shadow and extend of a bounce in one kernel, one hit queue class
    bool use_origin = false;     // ... its OriginCand instances: the two rays of a vertex against the scene's origin-candidate table
    bool class_queues = false;   // the general shade kernels' hit queue may be binned by BxDF class (kClasses)
    bool tab = false;            // the general shade kernels read the shading tables from LDS (k_shade<.., kTab>)
    bool tail_loop = false;      // the fused pipeline may take bounce 1 and every later one in one launch (kTailLoopBelow)
    bool pack_first = false;     // RenderCtx::pack_first for the passes of at most 4096 samples
    bool pixel_cull = false, row_spans = false;   // k_primary's screen-space rectangle, and the per-row spans inside it
    bool stream_p = false, stream_s = false, stream_e = false;   // the streaming walker serves primary / shadow / extension rays
    bool resolve32 = false;      // k_resolve_bits<32u> instead of <16u>
    bool film_stream = false;    // the overlapped schedule is allowed (no SPT_NO_FILM_STREAM)
    bool film_overlap = false;   // ... and this render takes it: tail launch, resolve, finish and copy-out on the film stream
    bool pass_pipeline = false;  // an overlapped render of a fused plan may run its bounce launches on stream2 (no SPT_NO_PASS_PIPELINE)
    bool pipe_plan = false;      // ... and this is an spt_render of such a plan: its overlapped form takes the pass pipeline (trace_window)
    uint64_t pipe_max_bytes = ~0ull;   // ... unless its second queue set would hold more than this (SPT_PASS_PIPELINE_MAX_BYTES)
    bool direct_out = false;     // k_finish_host may store into a pinned rgb_mean_out (no SPT_NO_DIRECT_OUT)
    uint32_t direct_grid = 0;    // ... over this many workgroups at the most (kFinishHostGrid, or SPT_DIRECT_OUT_GRID for A/B runs)
    bool debug_spans = false;    // per-launch HIP-event times on stderr (profile mode)
    bool general = false;        // the camera rays come from k_primary_cam (a camera model, or SPT_CAMERA_GENERAL=1): full path records at bounce 0, as `rays`
    CamJob cam_job{};            // ... and what it takes besides the scene and the pass
    uint32_t ray_aux_wrap = 0;   // RayAux::wrap of `ray_aux` below
    bool rays = false;           // spt_radiance: no camera, every bounce shaded from full path records (k_shade<., kFirst = false>)
    const float4* ray_aux = nullptr;   // ... and the auxiliary rays of the pass for the bounce-0 launch of a textured scene (kAux); null: none
    bool albedo = false;         // SPT_RENDER_AOV_ALBEDO: paths end at their first surface, and the kernels get the scene without its environment
    bool env = false;            // the scene the kernels see has an environment
    uint32_t primary_chunks = 0;   // sample chunks per primary tile; 0: sized to the busy tiles
    uint64_t box_band_bytes = 0;   // kept radiance per band of a wide box filter
    size_t lds = 0;
    uint32_t kDynBlocks = 0, dyn_refill_below = 0, dyn_steps = 0, stream_rounds = 0, stream_refill_below = 0;
    const int2* row_span_dev = nullptr;
    struct Span { int cls; size_t e0; };
    std::vector<Span> spans;
    size_t ev_used = 0;
    std::vector<uint32_t> h_counts;
    uint64_t seg_closest = 0, seg_shadow = 0, primary_hits = 0, path_vertices = 0, shadow_first = 0, vertices_second = 0;
    uint64_t samples_traced = 0, live_samples = 0;
    hipEvent_t get_event() {
        if (ev_used == sc->events.size()) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreate(&e));
            sc->events.push_back(e);
        }
        return sc->events[ev_used++];
    }
    void begin(int cls) {
        if (!profile) return;
        spans.push_back(Span{cls, ev_used});
        HIP_CHECK(hipEventRecord(get_event(), st));
    }
    void end() {
        if (!profile) return;
        HIP_CHECK(hipEventRecord(get_event(), st));
    }
};

// The kernel choices of one call (the scene's lock is held and its device selected): every environment switch of the render
// loop is read here, once.
void run_setup(RenderRun& run) {
    spt_scene* const sc = run.sc;
    const spt_render_params& p = *run.params;
    const spt_camera* const cam = run.cam;
    run.st = sc->stream;
    run.profile = (p.flags & SPT_RENDER_PROFILE) != 0;
    run.albedo = (p.flags & SPT_RENDER_AOV_ALBEDO) != 0;
    run.env = sc->d.env_w != 0u && !run.albedo;
    // visit counters: only the kernels that fetch their geometry from memory count (an LDS-resident scene is read once
    // per workgroup whatever the rays do)
    run.count = (p.flags & SPT_RENDER_COUNT_VISITS) != 0 && !sc->lds_geo;
    sc->visits.ensure(12 * sizeof(unsigned long long));
    if (run.count) HIP_CHECK(hipMemsetAsync(sc->visits.p, 0, 12 * sizeof(unsigned long long), sc->stream));
    // per-kernel event timing needs one stream; so does a scene with an environment (see bounce)
    run.overlap = !run.profile && !run.env && std::getenv("SPT_NO_OVERLAP") == nullptr;
    run.lds = sc->lds_bytes;
    run.L = sc->lds_geo;
    // a camera model - or, for A/B runs, the pinhole under SPT_CAMERA_GENERAL=1 (plans that count visits or ask for the albedo keep the
    // pinhole kernels) - takes k_primary_cam: nothing below that is derived from a pinhole eye applies to it
    run.general = !run.rays && (run.model != nullptr || (env_u32("SPT_CAMERA_GENERAL", 0u) != 0u && !run.albedo && !(p.flags & SPT_RENDER_COUNT_VISITS)));
    // primary rays of an LDS-resident scene through the eye-relative copy of its geometry (eye.h), remade when the eye has moved
    run.use_eye = !run.rays && !run.general && run.L && !run.count && sc->eye_ok && std::getenv("SPT_NO_EYE_BLOB") == nullptr;
    if (run.use_eye && (!sc->eye_valid || std::memcmp(sc->eye_key, cam->eye, sizeof(sc->eye_key)) != 0)) make_eye_blob(sc, cam->eye);
    // ... and, when that copy is at most 64 triangles of meshes only, against the triangles k_block_candidates leaves per wave
    run.use_cand = run.use_eye && sc->cand_ok && std::getenv("SPT_NO_BLOCK_CANDIDATES") == nullptr;
    // refilling persistent waves for large scenes: on for shadow rays (any-hit walks end at very
    // different times: 10.9 -> 8.8 ms on the 1 M-triangle scene), off for extension rays (28 vs 20 ms)
    run.dyn_shadow = !run.L && std::getenv("SPT_NO_DYN_SHADOW") == nullptr;
    // (with the 2-wide nodes the refilling extension kernel was slower, 28 vs 20 ms; with the 4-wide nodes it is
    //  faster, 16.0 vs 17.7 ms on cfg5 - measured - and on by default)
    run.dyn_extend = !run.L && std::getenv("SPT_NO_DYN_EXTEND") == nullptr;
    run.kDynBlocks = env_u32("SPT_DYN_BLOCKS", 2048);   // persistent blocks that pull work
    run.dyn_refill_below = env_u32("SPT_DYN_REFILL", kRefillBelow);
    run.dyn_steps = env_u32("SPT_DYN_STEPS", kStepsPerCheck);
    // which kernel classes the streaming walker serves (1 primary, 2 shadow, 4 extend).  Measured on cfg5, one box
    // (gpurun_out r2j): extension rays 93.5 ms refilling state machine -> 87.4 ms streaming if-if; primary rays
    // 8.8 -> 12.4 ms and shadow rays 9.8 -> 11.3 ms (coherent / short walks: the state machine's tighter loop wins)
    const bool stream = sc->swalk && !run.L;
    const uint32_t stream_mask = env_u32("SPT_STREAM_MASK", SPT_WITH_BEZIER ? 6u : 4u);   // (patch scenes: shadow rays too, 214 -> 197 ms on t_catmull.json)
    run.stream_p = stream && (stream_mask & 1u);
    run.stream_s = stream && (stream_mask & 2u);
    run.stream_e = stream && (stream_mask & 4u);
    // rays of a path tracer are short (cfg5: ~4 node + ~2 triangle + ~1 instance records per segment = 2 - 3 rounds):
    // a finished lane that waits several rounds for its wave costs more than the refill check
    // if-if with 4 rounds per check: 87.4 ms; 8 rounds 95.2; while-while (SPT_STREAM_IFIF=0) 100 - 121 ms
    run.stream_rounds = std::max(1u, std::min(255u, env_u32("SPT_STREAM_ROUNDS", 4u))) | (env_u32("SPT_STREAM_IFIF", 1u) ? 0x100u : 0u);
    run.stream_refill_below = std::max(1u, std::min(64u, env_u32("SPT_STREAM_REFILL", 40u)));
    // see k_shade<.., kFused>.  Only the lean k_shade<0> variant gains: with the general kernel's 220+ VGPRs
    // the two traversals run at 2 waves / SIMD and cfg4 is faster un-fused (4.30 vs 4.00 Gsamples/s, measured)
    run.fused = sc->fused && sc->simple && std::getenv("SPT_NO_FUSED") == nullptr;
    // ... with the candidate sets of the triangle a vertex lies on instead of the two walks, for a camera whose eye is within the
    // table's reach (the error bound of a bounce-0 origin grows with the camera's distance; caller rays start anywhere)
    run.use_origin = run.fused && sc->origin_ok && !run.rays && !run.general && !run.count && cam != nullptr && std::getenv("SPT_NO_ORIGIN_CANDIDATES") == nullptr;
    if (run.use_origin) {
        double d2 = 0.0;
        for (int k = 0; k < 3; ++k) d2 += ((double)cam->eye[k] - sc->origin_info.center[k]) * ((double)cam->eye[k] - sc->origin_info.center[k]);
        run.use_origin = std::sqrt(d2) <= sc->origin_info.reach;   // (a NaN eye fails the comparison)
    }
    run.class_queues = std::getenv("SPT_NO_CLASS_QUEUES") == nullptr;
    run.tab = sc->lds_tables && std::getenv("SPT_NO_LDS_TABLES") == nullptr;   // shading tables from LDS (tab_ld)
    run.tail_loop = std::getenv("SPT_NO_TAIL_LOOP") == nullptr;
    run.pack_first = sc->d.n_instances < (1u << 20) && std::getenv("SPT_NO_PACK_FIRST") == nullptr;
    run.pixel_cull = !run.general && std::getenv("SPT_NO_PIXEL_CULL") == nullptr;
    run.row_spans = run.pixel_cull && std::getenv("SPT_NO_ROW_SPANS") == nullptr;
    if (const char* v = std::getenv("SPT_PRIMARY_CHUNKS")) run.primary_chunks = (uint32_t)std::max(1, std::atoi(v));
    run.resolve32 = env_u32("SPT_RESOLVE_BATCH", 16u) == 32u;
    run.film_stream = env_u32("SPT_NO_FILM_STREAM", 0u) == 0u;
    run.pass_pipeline = !run.general && env_u32("SPT_NO_PASS_PIPELINE", 0u) == 0u;
    if (const char* v = std::getenv("SPT_PASS_PIPELINE_MAX_BYTES")) run.pipe_max_bytes = std::strtoull(v, nullptr, 10);
    run.direct_out = env_u32("SPT_NO_DIRECT_OUT", 0u) == 0u;
    run.direct_grid = std::max(1u, env_u32("SPT_DIRECT_OUT_GRID", kFinishHostGrid));
    run.box_band_bytes = 8ull << 30;
    if (const char* v = std::getenv("SPT_BOX_BAND_BYTES")) run.box_band_bytes = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
    run.debug_spans = std::getenv("SPT_DEBUG_SPANS") != nullptr;
    if (run.general) {
        spt_camera_model& m = run.cam_job.model;
        if (run.model != nullptr) m = *run.model;
        else { m = spt_camera_model{}; m.type = SPT_CAMERA_PERSPECTIVE; m.base = *cam; }
        m.size = (uint32_t)sizeof(spt_camera_model);
        run.cam_job.plan = spt_cm_plan_make(&m, p.width, p.height);
    }
}

void run_spans(RenderRun& run) {
    spt_scene* const sc = run.sc;
    const spt_render_params& p = *run.params;
    const spt_camera* const cam = run.cam;
    const int2*& row_span_dev = run.row_span_dev;

    // Per-row screen-space spans: every instance's object-space box (8 world-space corners, spt_scene_create) is
    // projected, the convex hull of the 8 image points is the exact silhouette of the box, and row j keeps the pixels
    // from the leftmost to the rightmost hull point within one row of slack above and below, plus one pixel each side.
    // A pixel outside its row's span cannot see any instance with any sample (k_primary's `in_bounds`): the rotated
    // cube of the headline scene fills 19 % of the image, its world-space AABB's rectangle 25 %.
    if (!sc->hull_corners.empty() && !run.env && run.row_spans) {
        std::vector<double> key = {(double)p.width, (double)p.height, (double)cam->half_cot_half_fov};
        for (int k = 0; k < 3; ++k) { key.push_back(cam->eye[k]); key.push_back(cam->forward[k]); key.push_back(cam->up[k]); key.push_back(cam->right[k]); }
        if (key != sc->span_key) {
            sc->span_key.clear();
            std::vector<int32_t>& sp = sc->span_host;
            sp.assign((size_t)p.height * 2, 0);
            for (uint32_t j = 0; j < p.height; ++j) { sp[2 * j] = (int32_t)p.width; sp[2 * j + 1] = -1; }
            const double W = (double)p.width, H = (double)p.height, aspect = W / H;
            bool ok = true;
            for (const auto& cn : sc->hull_corners) {
                double px[8], py[8];
                for (int c = 0; c < 8 && ok; ++c) {
                    double z = 0, xr = 0, yu = 0, n2 = 0;
                    for (int k = 0; k < 3; ++k) {
                        const double v = cn[3 * c + k] - (double)cam->eye[k];
                        z += v * (double)cam->forward[k]; xr += v * (double)cam->right[k]; yu += v * (double)cam->up[k]; n2 += v * v;
                    }
                    if (!(z > 1e-6 * std::sqrt(n2)) || !(z > 0)) { ok = false; break; }   // beside / behind the eye: no finite silhouette
                    const double x = (double)cam->half_cot_half_fov * xr / z, y = (double)cam->half_cot_half_fov * yu / z;
                    px[c] = (x / aspect + 0.5) * W;                 // pixel i covers [i, i + 1)
                    py[c] = H - (y + 0.5) * H;                     // row j covers (j, j + 1]  (k_primary: y = ((H - j - 1) + oy) / H - 0.5)
                    ok = std::isfinite(px[c]) && std::isfinite(py[c]) && std::fabs(px[c]) < 1e9 && std::fabs(py[c]) < 1e9;
                }
                if (!ok) break;
                // convex hull (monotone chain)
                int idx[8];
                for (int c = 0; c < 8; ++c) idx[c] = c;
                std::sort(idx, idx + 8, [&](int a, int b) { return px[a] < px[b] || (px[a] == px[b] && py[a] < py[b]); });
                int hull[17], hn = 0;
                auto crs = [&](int o, int a, int b) { return (px[a] - px[o]) * (py[b] - py[o]) - (py[a] - py[o]) * (px[b] - px[o]); };
                for (int c = 0; c < 8; ++c) { while (hn >= 2 && crs(hull[hn - 2], hull[hn - 1], idx[c]) <= 0) --hn; hull[hn++] = idx[c]; }
                for (int c = 6, lower = hn + 1; c >= 0; --c) { while (hn >= lower && crs(hull[hn - 2], hull[hn - 1], idx[c]) <= 0) --hn; hull[hn++] = idx[c]; }
                if (hn > 1) --hn;      // the last point repeats the first
                double ymin = 1e300, ymax = -1e300;
                for (int c = 0; c < hn; ++c) { ymin = std::min(ymin, py[hull[c]]); ymax = std::max(ymax, py[hull[c]]); }
                const int64_t j0 = std::max<int64_t>(0, (int64_t)std::floor(ymin) - 2), j1 = std::min<int64_t>((int64_t)p.height - 1, (int64_t)std::floor(ymax) + 2);
                for (int64_t j = j0; j <= j1; ++j) {
                    const double ya = (double)j - 1.0, yb = (double)j + 2.0;    // the row's own band (j, j + 1] and one row of slack each way
                    double xmin = 1e300, xmax = -1e300;
                    for (int c = 0; c < hn; ++c) {
                        const int a = hull[c], b = hull[(c + 1) % hn];
                        double xa = px[a], yA = py[a], xb = px[b], yB = py[b];
                        if (yA > yB) { std::swap(xa, xb); std::swap(yA, yB); }
                        if (yB < ya || yA > yb) continue;
                        double x0 = xa, x1 = xb;
                        if (yB > yA) {      // clip the edge to the band
                            const double t0 = std::max(0.0, (ya - yA) / (yB - yA)), t1 = std::min(1.0, (yb - yA) / (yB - yA));
                            x0 = xa + (xb - xa) * t0; x1 = xa + (xb - xa) * t1;
                        }
                        xmin = std::min({xmin, x0, x1}); xmax = std::max({xmax, x0, x1});
                    }
                    if (xmin > xmax) continue;
                    const int32_t lo = (int32_t)std::max(-1.0, std::min(W, std::floor(xmin) - 1.0)), hi = (int32_t)std::max(-1.0, std::min(W, std::floor(xmax) + 1.0));
                    sp[2 * j] = std::min(sp[2 * j], lo);
                    sp[2 * j + 1] = std::max(sp[2 * j + 1], hi);
                }
            }
            if (ok) {
                sc->row_span.ensure((size_t)p.height * 2 * sizeof(int32_t));
                HIP_CHECK(hipMemcpyAsync(sc->row_span.p, sp.data(), (size_t)p.height * 2 * sizeof(int32_t), hipMemcpyHostToDevice, sc->stream));
                HIP_CHECK(hipStreamSynchronize(sc->stream));   // `sp` is pageable; once per camera
                sc->span_key = key;
            } else {
                sp.clear();
            }
        }
        if (!sc->span_key.empty()) row_span_dev = sc->row_span.as<int2>();
    }
}

// What spt_render and spt_film_create both check of a plan; `who` prefixes the messages.
void check_plan(const spt_render_params& p, const char* who) {
    const std::string w(who);
    if (p.width == 0 || p.height == 0 || p.spp == 0) fail(SPT_ERR_INVALID_ARG, w + ": width, height and spp must be > 0");
    if (p.max_depth > 255) fail(SPT_ERR_UNSUPPORTED, w + ": max_depth > 255");
    if (p.sampler > SPT_SAMPLER_RECURRENCE) fail(SPT_ERR_INVALID_ARG, w + ": unknown sampler");
    if (p.sampler == SPT_SAMPLER_JITTERED && (p.division_x == 0 || p.division_y == 0 || p.division_x * p.division_y != p.spp))
        fail(SPT_ERR_INVALID_ARG, w + ": jittered sampler needs spp == division_x * division_y");
    const uint32_t shard_count = p.shard_count ? p.shard_count : 1u;
    if (p.shard_index >= shard_count) fail(SPT_ERR_INVALID_ARG, w + ": shard_index >= shard_count");
    if ((uint64_t)p.width * p.height > 0xffffffffull) fail(SPT_ERR_UNSUPPORTED, w + ": more than 2^32 pixels");
    if ((p.flags & SPT_RENDER_DEBUG_NORMAL) && (p.flags & SPT_RENDER_AOV_ALBEDO))
        fail(SPT_ERR_INVALID_ARG, w + ": SPT_RENDER_DEBUG_NORMAL and SPT_RENDER_AOV_ALBEDO exclude each other (a path has one colour)");
}

// BoxFilter (src/filter/boxf.rs:11-14): radius_int = ceil(radius - 0.5) neighbour pixels each way
float plan_radius(const spt_render_params& p, const char* who) {
    const float radius = (p.flags & SPT_RENDER_BOX_RADIUS) ? p.filter_radius : 0.5f;
    if (!(radius == radius) || std::fabs(radius) > 64.0f) fail(SPT_ERR_UNSUPPORTED, std::string(who) + ": box filter radius must be finite and at most 64");
    return radius;
}

// The plan and camera part of the RenderCtx of `rows` image rows: the strip formula of the ABI (w_index, w_count, w_strip)
// from image row row_base.  A film read's k_finish_box gets its context from here too.
RenderCtx plan_ctx(const spt_render_params& p, const spt_camera& cam, uint32_t row_base, uint32_t rows, uint32_t w_index, uint32_t w_count,
                   uint32_t w_strip) {
    RenderCtx rc{};
    rc.cam.eye = f3{cam.eye[0], cam.eye[1], cam.eye[2]};
    rc.cam.forward = f3{cam.forward[0], cam.forward[1], cam.forward[2]};
    rc.cam.up = f3{cam.up[0], cam.up[1], cam.up[2]};
    rc.cam.right = f3{cam.right[0], cam.right[1], cam.right[2]};
    rc.cam.half_cot = cam.half_cot_half_fov;
    rc.width = p.width; rc.height = p.height; rc.spp = p.spp; rc.max_depth = p.max_depth;
    rc.sampler = p.sampler; rc.division_x = p.division_x; rc.division_y = p.division_y;
    rc.seed = p.seed;
    rc.shard_index = w_index; rc.shard_count = w_count; rc.strip_rows = w_strip;
    rc.row_base = row_base;
    rc.n_pixels = rows * p.width;
    rc.rows = rows;
    rc.aspect = (float)p.width / (float)p.height;   // pt.rs:239
    rc.width_inv = 1.0f / (float)p.width;           // pt.rs:250-251
    rc.height_inv = 1.0f / (float)p.height;
    rc.spp_inv = 1.0f / (float)p.spp;
    {   // pt.rs:253-254, 272-275
        const float spp_sqrt_inv = 1.0f / std::sqrt((float)p.spp);
        rc.aux_dx = rc.aspect * rc.width_inv * spp_sqrt_inv;
        rc.aux_dy = rc.height_inv * spp_sqrt_inv;
    }
    rc.debug_normal = (p.flags & SPT_RENDER_DEBUG_NORMAL) ? 1u : ((p.flags & SPT_RENDER_AOV_ALBEDO) ? 2u : 0u);
    return rc;
}

// The main stream waits for whatever a pipelined render left on stream2 (its shade stage reads the scene and the path and hit queues).
void shade_join(spt_scene* sc) {
    if (!sc->shade_pending) return;
    HIP_CHECK(hipEventRecord(sc->ev_shade_idle, sc->stream2));
    HIP_CHECK(hipStreamWaitEvent(sc->stream, sc->ev_shade_idle, 0));
    sc->shade_pending = false;
}

// Every entry point that queues work on sc->stream and is not the overlapped schedule itself starts here: the main stream
// waits for whatever an overlapped render left on the film stream and on stream2 (the scene's lock is held, its device selected).
void film_join(spt_scene* sc) {
    shade_join(sc);
    if (!sc->film_pending) return;
    HIP_CHECK(hipEventRecord(sc->ev_film_idle, sc->stream_film));
    HIP_CHECK(hipStreamWaitEvent(sc->stream, sc->ev_film_idle, 0));
    sc->film_pending = false;
    sc->film_recorded[0] = sc->film_recorded[1] = false;   // (the main stream is behind both sets' film-stream work now)
    sc->tail_set = -1;
}

// Grows a workspace buffer (or `out`).  The old allocation may still be in use by an overlapped render on either stream:
// both are drained first (growth is rare: the first render of a size).
void grow(spt_scene* sc, DeviceBuffer& b, size_t n) {
    if (n <= b.bytes) return;
    if (sc->film_inflight) {
        HIP_CHECK(hipStreamSynchronize(sc->stream));
        HIP_CHECK(hipStreamSynchronize(sc->stream2));
        HIP_CHECK(hipStreamSynchronize(sc->stream_film));
        sc->film_inflight = sc->film_pending = sc->copy_pending = sc->shade_pending = false;
        sc->film_recorded[0] = sc->film_recorded[1] = false;
        sc->tail_set = -1;
    }
    b.alloc(n);
}

// k_pack_rgb8 over the n_floats floats of `in`, on `st` behind the kernel that wrote them.
void launch_pack_rgb8(uint32_t n_floats, const float* in, uint8_t* out, hipStream_t st) {
    const uint32_t lanes = (n_floats + 3u) / 4u;
    hipLaunchKernelGGL(k_pack_rgb8, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n_floats, in, out);
    HIP_CHECK(hipGetLastError());
}

// The passes of one window: their size, and the queues and counters they use.
struct PassShape {
    uint32_t spp_pass;       // samples per pass
    size_t counts_words;     // the pass counters, [bounce][Q_KINDS][kShards] 128-B lines
    uint64_t rad_slots;      // per-sample radiance slots per colour plane
};

// Sizes the passes of the window of rc (plan_ctx) that add `n_samples` samples, grows the scene's workspace to them and binds
// it and the window's tiles into rc.  sum: the running sums the passes add to (null: the scene's workspace film).
// collect: every sample of the window is kept (wide box filter), else only the samples of one pass.
// samples per pass of a window of n_pix pixels that adds n_samples: keep the queues around a few million entries
uint32_t pass_samples_of(const spt_render_params& p, uint32_t n_pix, uint32_t n_samples) {
    uint32_t spp_pass = p.samples_per_pass;
    if (spp_pass == 0) {
        const uint64_t target = 128ull << 20;
        spp_pass = (uint32_t)std::max<uint64_t>(1, target / n_pix);
    }
    return std::min(spp_pass, n_samples);   // (a film's increment: what is left of it)
}

// The path, hit and shadow queues and the pass counters of passes whose queue shards hold shard_cap entries (cap = kShards * shard_cap
// in all), grown and bound into rc: what a window of pixels (grow_workspace) and a pass of caller rays (spt_radiance) share.
// compact_first: the bounce-0 records are k_primary's compact ones, which sit at their hit's index in every class of the hit queue.
// Returns the words of the pass counters.
size_t grow_queues(spt_scene* sc, size_t cap, uint32_t shard_cap, uint32_t max_depth, bool fused, bool class_queues, bool compact_first, RenderCtx& rc) {
    // the hit queue is binned by BxDF class for the general shade kernels (kernels.h, kClasses): class c lives c * cap
    // entries further.  Memory is what MI355X has (24 B x cap x 8 classes = 26 GB for a 128 M-sample pass)
    const uint32_t n_classes = (!fused && max_depth > 1 && cap * (uint64_t)kClasses <= 0xffffffffull && class_queues) ? kClasses : 1u;
    for (int k = 0; k < 4; ++k) { grow(sc, sc->qa[k], cap * 16 * (k == 1 && compact_first ? n_classes : 1u)); grow(sc, sc->qb[k], cap * 16); }
    grow(sc, sc->qa[4], cap * 8);
    grow(sc, sc->qb[4], cap * 8);
    grow(sc, sc->hit_f4, cap * 16 * n_classes);
    grow(sc, sc->hit_inst, cap * 8 * n_classes);
    if (fused) {
        grow(sc, sc->hit_f4_next, cap * 16);
        grow(sc, sc->hit_inst_next, cap * 8);
    }
    for (int k = 0; k < 3; ++k) grow(sc, sc->sh[k], cap * 16);
    const size_t counts_words = (size_t)(max_depth + 1) * Q_KINDS * kShards * 32;
    grow(sc, sc->counts[0], counts_words * sizeof(uint32_t));
    rc.qa = PathQueue{sc->qa[0].as<float4>(), sc->qa[1].as<float4>(), sc->qa[2].as<float4>(), sc->qa[3].as<float4>(), sc->qa[4].as<uint2>()};
    rc.qb = PathQueue{sc->qb[0].as<float4>(), sc->qb[1].as<float4>(), sc->qb[2].as<float4>(), sc->qb[3].as<float4>(), sc->qb[4].as<uint2>()};
    rc.hits = HitQueue{sc->hit_f4.as<float4>(), sc->hit_inst.as<uint2>()};
    rc.hits_next = HitQueue{sc->hit_f4_next.as<float4>(), sc->hit_inst_next.as<uint2>()};
    rc.shadow = ShadowQueue{sc->sh[0].as<float4>(), sc->sh[1].as<float4>(), sc->sh[2].as<float4>()};
    rc.counts = sc->counts[0].as<uint32_t>();
    rc.shard_cap = shard_cap;
    rc.n_classes = n_classes;
    rc.class_cap = (uint32_t)cap;
    return counts_words;
}

// The sample chunks of a k_primary_cam pass of pass_samples samples over n_tiles tiles: about 6144 workgroups, as primary_pass aims at
struct CamChunks { uint32_t chunk_samples, chunks; };
CamChunks cam_chunks(uint32_t n_tiles, uint32_t pass_samples) {
    const uint32_t want = std::max(1u, std::min({64u, (6144u + n_tiles - 1u) / std::max(n_tiles, 1u), pass_samples}));
    const uint32_t chunk_samples = (pass_samples + want - 1u) / want;
    return CamChunks{chunk_samples, (pass_samples + chunk_samples - 1u) / chunk_samples};
}

// general: the passes are k_primary_cam's (camera_kernels.h), whose queue shards belong to workgroups, not to tiles, and whose bounce-0
// records are full path records
PassShape grow_workspace(spt_scene* sc, const spt_render_params& p, uint32_t n_samples, bool collect, bool fused, bool class_queues, float* sum,
                         bool own_rad, bool general, bool cam_aux, RenderCtx& rc) {
    const uint32_t n_pix = rc.n_pixels;
    PassShape ps{};
    ps.spp_pass = pass_samples_of(p, n_pix, n_samples);
    // queue shards: shard s holds what the primary tiles mapped to it can emit, which also bounds
    // every later generation of that shard
    const uint32_t tiles_y = (rc.rows + kTile - 1) / kTile;
    rc.tiles_x = (p.width + kTile - 1) / kTile;
    rc.n_tiles = rc.tiles_x * tiles_y;
    uint32_t max_tiles = 0;
    {
        std::vector<uint32_t> per(kShards, 0u);
        for (uint32_t ty = 0; ty < tiles_y; ++ty)
            for (uint32_t tx = 0; tx < rc.tiles_x; ++tx) max_tiles = std::max(max_tiles, ++per[(tx + 9u * ty) % kShards]);
    }
    uint64_t shard_cap64 = (uint64_t)max_tiles * kBlock * ps.spp_pass;
    if (general) {   // the passes come in two sizes, the full one and the rest behind the last full one: a shard holds either
        shard_cap64 = 0;
        for (const uint32_t pass_samples : {ps.spp_pass, n_samples % ps.spp_pass}) {
            if (pass_samples == 0u) continue;
            const CamChunks cc = cam_chunks(rc.n_tiles, pass_samples);
            shard_cap64 = std::max(shard_cap64, (((uint64_t)rc.n_tiles * cc.chunks + kShards - 1) / kShards) * kBlock * cc.chunk_samples);
        }
    }
    const uint64_t cap64 = shard_cap64 * kShards;
    if (cap64 > 0x7fffffffull) fail(SPT_ERR_UNSUPPORTED, "render: pass too large (lower samples_per_pass)");
    const size_t cap = (size_t)cap64;
    ps.rad_slots = (uint64_t)n_pix * (collect ? p.spp : ps.spp_pass);

    ps.counts_words = grow_queues(sc, cap, (uint32_t)shard_cap64, p.max_depth, fused, class_queues, !general, rc);
    if (cam_aux) grow(sc, sc->cam_aux, (size_t)n_pix * ps.spp_pass * sizeof(spt_ray_aux));
    if (!own_rad) grow(sc, sc->rad[0], (size_t)ps.rad_slots * 3 * sizeof(float));   // (own_rad: the passes write the caller's chunks, SampleTarget::keep)
    float* const film_sum = sum ? sum : (grow(sc, sc->film, (size_t)n_pix * 3 * sizeof(float)), sc->film.as<float>());
    grow(sc, sc->first_slot[0], (size_t)n_pix * sizeof(uint32_t));
    grow(sc, sc->slot_bits[0], (size_t)n_pix * ((ps.spp_pass + 7u) / 8u));

    rc.rad = sc->rad[0].as<float>();
    rc.film = film_sum;
    rc.first_slot = sc->first_slot[0].as<uint32_t>();
    return ps;
}

// The second set of the doubled pass buffers, sized like the first (grow_workspace).  False: no memory for it (the render
// keeps the single-stream schedule).
bool grow_second_set(spt_scene* sc) {
    try {
        grow(sc, sc->counts[1], sc->counts[0].bytes);
        grow(sc, sc->rad[1], sc->rad[0].bytes);
        grow(sc, sc->first_slot[1], sc->first_slot[0].bytes);
        grow(sc, sc->slot_bits[1], sc->slot_bits[0].bytes);
    } catch (const AbiError& e) {
        if (e.code != SPT_ERR_OUT_OF_MEMORY) throw;
        (void)hipGetLastError();
        return false;
    }
    return true;
}

// Set 1 of the path and hit queues of a fused plan, sized like set 0 (grow_queues) and bound into q: what the pass pipeline needs on top of
// grow_second_set.  False: no memory for it (the render keeps the two-stream schedule).
struct QueueSet {
    PathQueue qa, qb;
    HitQueue hits, hits_next;
};
// max_bytes: the set is refused, as if the device had no memory for it, once it would hold more than this (SPT_PASS_PIPELINE_MAX_BYTES).
// A refusal frees what the set holds - a part of it is of no use and would be missing for the film, `out` or kept chunks - and is
// remembered for the size it was refused at (sc->pipe_refused_bytes), so that the frames that follow neither drain the streams
// nor ask the device again.
bool grow_pipeline_set(spt_scene* sc, uint64_t max_bytes, QueueSet& q) {
    std::pair<DeviceBuffer*, const DeviceBuffer*> bufs[14];
    for (int k = 0; k < 5; ++k) { bufs[2 * k] = {&sc->qa_1[k], &sc->qa[k]}; bufs[2 * k + 1] = {&sc->qb_1[k], &sc->qb[k]}; }
    bufs[10] = {&sc->hit_f4_1, &sc->hit_f4};
    bufs[11] = {&sc->hit_inst_1, &sc->hit_inst};
    bufs[12] = {&sc->hit_f4_next_1, &sc->hit_f4_next};
    bufs[13] = {&sc->hit_inst_next_1, &sc->hit_inst_next};
    uint64_t need = 0;
    for (const auto& b : bufs) need += b.second->bytes;
    if (sc->pipe_refused_bytes != 0 && need >= sc->pipe_refused_bytes) return false;
    try {
        uint64_t held = 0;
        for (const auto& b : bufs) {
            held += std::max(b.first->bytes, b.second->bytes);
            if (held > max_bytes) fail(SPT_ERR_OUT_OF_MEMORY, "render: the second queue set is above SPT_PASS_PIPELINE_MAX_BYTES");
            grow(sc, *b.first, b.second->bytes);
        }
    } catch (const AbiError& e) {
        if (e.code != SPT_ERR_OUT_OF_MEMORY) throw;
        (void)hipGetLastError();
        // (a buffer that had to grow drained the streams first, grow; a set that only failed the limit may still be in use)
        if (sc->film_inflight) {
            HIP_CHECK(hipStreamSynchronize(sc->stream));
            HIP_CHECK(hipStreamSynchronize(sc->stream2));
            HIP_CHECK(hipStreamSynchronize(sc->stream_film));
        }
        for (const auto& b : bufs) b.first->release();
        sc->pipe_refused_bytes = need;
        return false;
    }
    sc->pipe_refused_bytes = 0;
    q.qa = PathQueue{sc->qa_1[0].as<float4>(), sc->qa_1[1].as<float4>(), sc->qa_1[2].as<float4>(), sc->qa_1[3].as<float4>(), sc->qa_1[4].as<uint2>()};
    q.qb = PathQueue{sc->qb_1[0].as<float4>(), sc->qb_1[1].as<float4>(), sc->qb_1[2].as<float4>(), sc->qb_1[3].as<float4>(), sc->qb_1[4].as<uint2>()};
    q.hits = HitQueue{sc->hit_f4_1.as<float4>(), sc->hit_inst_1.as<uint2>()};
    q.hits_next = HitQueue{sc->hit_f4_next_1.as<float4>(), sc->hit_inst_next_1.as<uint2>()};
    return true;
}

// k_primary's early-outs for the camera: the bounding sphere of the instances relative to the eye, and the rectangle of the
// image their world box projects to (the whole image without pixel_cull or a finite bound)
void screen_bound(const spt_scene* sc, const spt_render_params& p, const spt_camera& cam, bool pixel_cull, RenderCtx& rc) {
    double oc[3], d2 = 0;
    for (int k = 0; k < 3; ++k) { oc[k] = sc->bs_center[k] - (double)cam.eye[k]; d2 += oc[k] * oc[k]; }
    rc.bs_oc = f3{(float)oc[0], (float)oc[1], (float)oc[2]};
    // a little extra slack for the f32 rounding of oc and of the test itself
    rc.bs_c = (float)((d2 - sc->bs_radius * sc->bs_radius) * (1.0 - 1e-5));
    rc.bs_valid = sc->bs_valid ? 1u : 0u;
    // screen-space bound: project the 8 corners of the union of the instance boxes (double precision).
    // A point P is seen through image coordinates (u, v) = ((x / aspect + 0.5) W, (y + 0.5) H) with
    // x = half_cot * (P - eye).right / (P - eye).forward, y likewise with up (k_primary: pt.rs:269-271).
    rc.cull_i0 = 0; rc.cull_i1 = (int32_t)p.width - 1; rc.cull_j0 = 0; rc.cull_j1 = (int32_t)p.height - 1;
    if (!sc->bs_valid || !pixel_cull) return;
    double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300;
    bool ok = true;
    const double ext = std::max({sc->world_hi[0] - sc->world_lo[0], sc->world_hi[1] - sc->world_lo[1], sc->world_hi[2] - sc->world_lo[2], 1e-30});
    for (int c = 0; c < 8 && ok; ++c) {
        double v[3], z = 0, xr = 0, yu = 0;
        for (int k = 0; k < 3; ++k) {
            const double pad = 1e-4 * ext;   // covers the (tiny) padding of the device-side boxes
            v[k] = (((c >> k) & 1) ? sc->world_hi[k] + pad : sc->world_lo[k] - pad) - (double)cam.eye[k];
            z += v[k] * (double)cam.forward[k];
            xr += v[k] * (double)cam.right[k];
            yu += v[k] * (double)cam.up[k];
        }
        if (!(z > 1e-6 * ext)) { ok = false; break; }   // a corner beside / behind the eye: no finite bound
        const double x = (double)cam.half_cot_half_fov * xr / z, y = (double)cam.half_cot_half_fov * yu / z;
        const double u = (x / ((double)p.width / (double)p.height) + 0.5) * (double)p.width, w = (y + 0.5) * (double)p.height;
        umin = std::min(umin, u); umax = std::max(umax, u);
        vmin = std::min(vmin, w); vmax = std::max(vmax, w);
    }
    if (ok && std::isfinite(umin) && std::isfinite(umax) && std::isfinite(vmin) && std::isfinite(vmax)) {
        // pixel i covers u in [i, i + 1); row j covers v in [H - 1 - j, H - j); one pixel of slack each side
        const double H = (double)p.height;
        auto clampi = [](double x, double lo, double hi) { return (int32_t)std::max(lo, std::min(hi, x)); };
        rc.cull_i0 = clampi(std::floor(umin) - 1.0, -1.0, (double)p.width);
        rc.cull_i1 = clampi(std::floor(umax) + 1.0, -1.0, (double)p.width);
        rc.cull_j0 = clampi(std::floor(H - 1.0 - vmax) - 1.0, -1.0, H);
        rc.cull_j1 = clampi(std::floor(H - 1.0 - vmin) + 2.0, -1.0, H);
    }
}

// The pixels of rc's window inside the screen-space bound (and the row spans, when rc has them) and the tiles that
// intersect it; every pixel and tile with an environment
struct LiveCount {
    uint32_t active_tiles;
    uint64_t live_pixels;
};
LiveCount count_live(const spt_scene* sc, bool env, const RenderCtx& rc) {
    if (env) return LiveCount{rc.n_tiles, rc.n_pixels};
    auto image_row = [&rc](uint32_t r) {   // global_row of kernels.h
        const uint32_t strip = r / rc.strip_rows;
        return (int32_t)(rc.row_base + (strip * rc.shard_count + rc.shard_index) * rc.strip_rows + (r - strip * rc.strip_rows));
    };
    LiveCount live{0u, 0u};
    for (uint32_t r = 0; r < rc.rows; ++r) {
        const int32_t j = image_row(r);
        if (j >= rc.cull_j0 && j <= rc.cull_j1) {
            int32_t i0 = std::max(rc.cull_i0, 0), i1 = std::min(rc.cull_i1, (int32_t)rc.width - 1);
            if (rc.row_span) { i0 = std::max(i0, sc->span_host[2 * (size_t)j]); i1 = std::min(i1, sc->span_host[2 * (size_t)j + 1]); }
            live.live_pixels += (uint64_t)std::max(0, i1 - i0 + 1);
        }
    }
    for (uint32_t ty = 0; ty < rc.n_tiles / rc.tiles_x; ++ty)
        for (uint32_t tx = 0; tx < rc.tiles_x; ++tx) {
            const int32_t i_lo = (int32_t)(tx * kTile), i_hi = (int32_t)std::min(rc.width, (tx + 1) * kTile) - 1;
            bool rows_in = false;
            for (uint32_t r = ty * kTile; r < std::min(rc.rows, (ty + 1) * kTile) && !rows_in; ++r) {
                const int32_t j = image_row(r);
                rows_in = j >= rc.cull_j0 && j <= rc.cull_j1 && i_hi >= rc.cull_i0 && i_lo <= rc.cull_i1;
                if (rows_in && rc.row_span) rows_in = i_hi >= sc->span_host[2 * (size_t)j] && i_lo <= sc->span_host[2 * (size_t)j + 1];
            }
            if (rows_in) ++live.active_tiles;
        }
    return live;
}

// The scene as the primary kernel of this run sees it: an albedo plan (SPT_RENDER_AOV_ALBEDO) hides the environment, so a miss is
// black and every host-side choice that asks "is there an environment" (run.env) agrees with the kernel.
DScene run_scene(const RenderRun& run, bool eye) {
    DScene d = eye ? run.sc->eye_d : run.sc->d;
    if (run.albedo) d.env_w = d.env_h = 0u;
    return d;
}

// The primary kernel of a pass over `blocks` workgroups (one per tile, or per tile and sample chunk: kChunked).  The mask
// argument (FilmMask) makes it an adaptive film's k_*<..., kMask>, which exists chunked and without visit counting only.
template <bool kChunked, class... M>
void launch_primary(const RenderRun& run, uint32_t blocks, const RenderCtx& rc, M... mask) {
    constexpr bool kMask = sizeof...(M) != 0;
    const spt_scene* const sc = run.sc;
    void (*fn)(DScene, RenderCtx, M...);
    if (run.stream_p) fn = k_primary_stream<kChunked, false, kMask, M...>;
    else if (run.use_eye) fn = k_primary<true, kChunked, false, true, kMask, M...>;
    else if (run.L) fn = k_primary<true, kChunked, false, false, kMask, M...>;
    else fn = k_primary<false, kChunked, false, false, kMask, M...>;
    if constexpr (!kMask) {   // (visits are only counted outside LDS, so never through the eye-relative copy)
        if (run.count) fn = run.stream_p ? k_primary_stream<kChunked, true> : k_primary<false, kChunked, true>;
    }
    if constexpr (kChunked || !kMask) {
        if (run.use_cand && !run.stream_p && !run.count) {   // (use_cand implies use_eye; the masks are those of this window, see trace_window)
            hipLaunchKernelGGL((k_primary<true, kChunked, false, true, kMask, M..., BlockCand>), dim3(blocks), dim3(kBlock), sc->eye_lds_bytes, run.st,
                               run_scene(run, true), rc, mask..., BlockCand{sc->block_cand.as<uint64_t>()});
            return;
        }
    }
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(kBlock), run.use_eye ? sc->eye_lds_bytes : run.lds, run.st, run_scene(run, run.use_eye), rc, mask...);
}

// The sample chunks per tile and the primary kernel of one pass.  Returns whether the kernel was a chunked one (which
// marks the samples that own a radiance slot in rc.slot_bits for the resolve).
bool primary_pass(const RenderRun& run, RenderCtx& rc, const SampleTarget& tgt, uint32_t active_tiles, bool collect, uint8_t* slot_bits) {
    spt_scene* const sc = run.sc;
    if (run.general) {   // every sample of a live pixel owns its slot and the film is touched by the resolve only: the plain k_resolve follows
        const CamChunks cc = cam_chunks(rc.n_tiles, rc.pass_samples);
        rc.chunk_samples = cc.chunk_samples;
        rc.primary_chunks = cc.chunks;
        rc.slot_bits = nullptr;
        CamJob job = run.cam_job;
        job.mask = tgt.mask;
        job.aux_out = run.ray_aux != nullptr ? sc->cam_aux.as<float4>() : nullptr;
        const bool stream = sc->swalk && !sc->lds_geo;   // the walkers of spt_trace_closest, as spt_radiance's intake
        hipLaunchKernelGGL(stream ? k_primary_cam<2> : sc->lds_geo ? k_primary_cam<0> : k_primary_cam<1>, dim3(rc.n_tiles * cc.chunks), dim3(kBlock),
                           sc->lds_bytes, run.st, run_scene(run, false), rc, job);
        ++sc->passes_cam;
        return false;
    }
    // sample chunks per tile: aim at ~6144 busy workgroups (24 per CU; 4096 .. 8192 measured within 2 %) given the tiles inside the screen bound
    // (an adaptive film: the tiles its last adapt left active; chunking does not change bits)
    const uint32_t busy_tiles = tgt.mask.pixel ? std::min(active_tiles, tgt.mask_tiles) : active_tiles;
    uint32_t want = std::min<uint32_t>(64u, (6144u + busy_tiles - 1u) / std::max(busy_tiles, 1u));
    if (run.primary_chunks) want = run.primary_chunks;
    want = std::max(1u, std::min(want, rc.pass_samples));
    rc.chunk_samples = (rc.pass_samples + want - 1u) / want;
    rc.chunk_samples = (rc.chunk_samples + 7u) / 8u * 8u;   // slot_bits: a group of 8 samples belongs to one chunk
    rc.primary_chunks = (rc.pass_samples + rc.chunk_samples - 1u) / rc.chunk_samples;
    // collect: every sample owns a slot, which is what the chunked kernel does.  Moments of a scene with an environment: the
    // un-chunked kernel adds the misses before a pixel's first hit straight into its sum, past k_resolve<true>'s Q
    // An adaptive film takes the chunked path only (its masked instances), whatever the chunk count.
    // Buckets of a scene with an environment: the same, those misses would pass k_resolve_buckets.
    const bool all_slots = collect || ((tgt.sq != nullptr || tgt.buckets != nullptr) && run.env) || tgt.mask.pixel != nullptr;
    const bool chunked = rc.primary_chunks > 1u || all_slots;
    rc.slot_bits = chunked ? slot_bits : nullptr;
    if (!chunked && run.film_overlap) {   // the un-chunked kernel adds into rc.film itself: behind the film memset and every earlier resolve
        HIP_CHECK(hipEventRecord(sc->ev_film_idle, sc->stream_film));
        HIP_CHECK(hipStreamWaitEvent(run.st, sc->ev_film_idle, 0));
    }
    if (tgt.mask.pixel != nullptr) {
        if (run.count) fail(SPT_ERR_INVALID_ARG, "render: an adaptive film does not count visits");
        launch_primary<true>(run, rc.n_tiles * rc.primary_chunks, rc, tgt.mask);
    } else if (chunked) {
        launch_primary<true>(run, rc.n_tiles * rc.primary_chunks, rc);
    } else {
        launch_primary<false>(run, rc.n_tiles, rc);
    }
    return chunked;
}

using BounceFn = void (*)(DScene, RenderCtx, uint32_t);

// k_shade<kFeat, kFirst, false, kTab, kGeoLds> of the general pipeline: the shading tables and the geometry from LDS, or
// neither, or - levels 3 and 5 with the geometry in LDS and the tables not - the BSSRDF probe walking the LDS copy (kGeoLds)
template <int kFeat>
BounceFn shade_level(bool first, bool tab, bool geo_lds) {
    if (tab) return first ? k_shade<kFeat, true, false, true, true> : k_shade<kFeat, false, false, true, true>;
    if constexpr (kFeat == 3 || kFeat == 5)
        if (geo_lds) return first ? k_shade<kFeat, true, false, false, true> : k_shade<kFeat, false, false, false, true>;
    return first ? k_shade<kFeat, true, false, false, false> : k_shade<kFeat, false, false, false, false>;
}

// The shade kernel of bounce b.  tail_loop: the fused kernel that takes bounce 1 and every later one in one launch.
BounceFn shade_kernel(const RenderRun& run, uint32_t b, bool tail_loop) {
    const spt_scene* const sc = run.sc;
    const bool first = b == 0 && !run.rays && !run.general;   // (caller rays and camera models: bounce 0 has full path records too, radiance_kernels.h)
    if (run.fused) return first ? k_shade<0, true, true, true, true> : tail_loop ? k_shade<0, false, true, true, true, true> : k_shade<0, false, true, true, true>;
    if (sc->simple) return shade_level<0>(first, run.tab, false);
    if (!sc->textured) return shade_level<1>(first, run.tab, false);
    if (!sc->subsurface) return shade_level<2>(first, run.tab, false);
    if (!sc->has_probe) return shade_level<4>(first, run.tab, false);   // glints only: no probe, so the geometry's place does not matter
    return sc->has_pndf ? shade_level<5>(first, run.tab, run.L) : shade_level<3>(first, run.tab, run.L);
}

// ... and its OriginCand instance, which run.use_origin launches in its place
using BounceOriginFn = void (*)(DScene, RenderCtx, uint32_t, OriginCand);
BounceOriginFn shade_origin_kernel(uint32_t b, bool tail_loop) {
    return b == 0 ? k_shade<0, true, true, true, true, false, false, OriginCand>
                  : tail_loop ? k_shade<0, false, true, true, true, true, false, OriginCand> : k_shade<0, false, true, true, true, false, false, OriginCand>;
}

// k_shade<kFeat, false, false, kTab, kGeoLds, false, kAux = true>: bounce 0 of spt_radiance with auxiliary rays on a textured scene, chosen
// as shade_level / shade_kernel choose the plain instances
using BounceAuxFn = void (*)(DScene, RenderCtx, uint32_t, RayAux);
template <int kFeat>
BounceAuxFn shade_aux_level(bool tab, bool geo_lds) {
    if (tab) return k_shade<kFeat, false, false, true, true, false, true, RayAux>;
    if constexpr (kFeat == 3 || kFeat == 5)
        if (geo_lds) return k_shade<kFeat, false, false, false, true, false, true, RayAux>;
    return k_shade<kFeat, false, false, false, false, false, true, RayAux>;
}
BounceAuxFn shade_aux_kernel(const RenderRun& run) {
    const spt_scene* const sc = run.sc;
    if (!sc->subsurface) return shade_aux_level<2>(run.tab, false);
    if (!sc->has_probe) return shade_aux_level<4>(run.tab, false);
    return sc->has_pndf ? shade_aux_level<5>(run.tab, run.L) : shade_aux_level<3>(run.tab, run.L);
}

// The shadow or the extension rays of a bounce: the kernels of one ray kind, [kCount] where visit counting makes two
struct RayKernels {
    BounceFn stream[2];     // the streaming walker (stream.h)
    BounceFn dyn[2];        // persistent waves that refill
    BounceFn mem[2];        // persistent waves, geometry from memory
    BounceFn lds, lds_flat;   // geometry in LDS; kFlat: the scene's flat layout (flat.h)
};
const RayKernels kShadowRays{{k_shadow_stream<false>, k_shadow_stream<true>}, {k_shadow_dyn<false>, k_shadow_dyn<true>},
                             {k_shadow<false, false>, k_shadow<false, true>}, k_shadow<true, false>, k_shadow<true, false, true>};
const RayKernels kExtendRays{{k_extend_stream<false>, k_extend_stream<true>}, {k_extend_dyn<false>, k_extend_dyn<true>},
                             {k_extend<false, false>, k_extend<false, true>}, k_extend<true, false>, k_extend<true, false, true>};

void launch_rays(const RenderRun& run, const RayKernels& k, bool stream, bool dyn, hipStream_t s, const RenderCtx& ru, uint32_t b) {
    const spt_scene* const sc = run.sc;
    BounceFn fn = k.mem[run.count];
    uint32_t blocks = kPersistentBlocks;
    if (stream) { fn = k.stream[run.count]; blocks = run.kDynBlocks; }
    else if (run.L) fn = sc->d.flat ? k.lds_flat : k.lds;
    else if (dyn) { fn = k.dyn[run.count]; blocks = run.kDynBlocks; }
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(kBlock), run.lds, s, sc->d, ru, b);
}

// One bounce of a pass: shade, then shadow and extension rays.  Returns true when the fused pipeline's tail loop took every
// later bounce along.
// few vertices left after bounce 0 (seen by the previous pass with a counter readback): bounce 1 and
// everything after it in ONE launch, each lane following its path to the end (k_shade's kLoop)
bool takes_tail_loop(const RenderRun& run, uint32_t b) {
    return run.fused && b == 1 && run.tail_loop && run.sc->tail_vertices <= kTailLoopBelow;
}

// `st`: the stream of the shade launch (the film stream for the tail-loop launch of the overlapped schedule, else run.st).
bool bounce(RenderRun& run, const RenderCtx& rc, uint32_t b, hipStream_t st) {
    spt_scene* const sc = run.sc;
    const uint32_t max_depth = run.params->max_depth;
    // the fused kernel: shade + shadow + extend of this bounce in one kernel; vertices of bounce b live in (qa, hits) for even
    // b and in (qb, hits_next) for odd b.  Un-fused: the shade stage of bounce b reads the path records its predecessor
    // wrote (ru.qa) through the hits' source indices and writes the next ones to ru.qb, which the extend stage traces: the
    // two path queues swap roles every bounce, the hit queue is one buffer
    RenderCtx ru = rc;
    if (b & 1u) {
        std::swap(ru.qa, ru.qb);
        if (run.fused) std::swap(ru.hits, ru.hits_next);
    }
    const bool tail_loop = takes_tail_loop(run, b);
    // LDS: the traversal stack and geometry, also for the BSSRDF probe, which walks the BVH inside k_shade<3 | 5>
    const size_t shade_lds = (run.fused || run.tab || sc->has_probe) ? run.lds : 0;
    run.begin(b == 0 ? SPT_K_SHADE_FIRST : SPT_K_SHADE);
    if (run.albedo) {   // every path ends in k_shade_albedo: no shadow ray, no extension ray (trace_window launches bounce 0 only)
        const bool pndf = sc->textured && sc->subsurface && sc->has_pndf;   // the scenes whose shade kernel is k_shade<4 | 5>
        const BounceFn fn = pndf ? k_shade_albedo<true, true> : sc->textured ? k_shade_albedo<true, false> : k_shade_albedo<false, false>;
        hipLaunchKernelGGL(fn, dim3(kPersistentBlocks), dim3(kBlock), 0, st, sc->d, ru, b);
        run.end();
        return false;
    }
    if (run.ray_aux != nullptr && b == 0u && sc->textured && !sc->simple && !run.fused)
        hipLaunchKernelGGL(shade_aux_kernel(run), dim3(kPersistentBlocks), dim3(kBlock), shade_lds, st, sc->d, ru, b, RayAux{run.ray_aux, run.ray_aux_wrap});
    else if (run.use_origin)
        hipLaunchKernelGGL(shade_origin_kernel(b, tail_loop), dim3(kPersistentBlocks), dim3(kBlock), shade_lds, st, sc->d, ru, b, OriginCand{sc->origin_cand.as<uint4>()});
    else
        hipLaunchKernelGGL(shade_kernel(run, b, tail_loop), dim3(kPersistentBlocks), dim3(kBlock), shade_lds, st, sc->d, ru, b);
    run.end();
    if (run.fused) return tail_loop;
    // k_shadow(b) and k_extend(b) are independent unless the scene has an environment (then a missing
    // extension ray adds its term to the same radiance slot the shadow ray of that vertex adds to, and
    // the reference's order of the two additions has to be kept): without one, the shadow kernel runs on
    // a side stream next to the extension kernel and is joined before the next stage reads the slots.
    const bool side = run.overlap && b + 1 < max_depth;
    const hipStream_t ss = side ? sc->stream2 : run.st;
    if (side) {
        HIP_CHECK(hipEventRecord(sc->ev_fork, run.st));
        HIP_CHECK(hipStreamWaitEvent(ss, sc->ev_fork, 0));
    }
    run.begin(SPT_K_SHADOW);
    launch_rays(run, kShadowRays, run.stream_s, run.dyn_shadow, ss, ru, b);
    run.end();
    if (side) HIP_CHECK(hipEventRecord(sc->ev_join, ss));
    if (b + 1 < max_depth) {
        run.begin(SPT_K_EXTEND);
        launch_rays(run, kExtendRays, run.stream_e, run.dyn_extend, run.st, ru, b);
        run.end();
    }
    if (side) HIP_CHECK(hipStreamWaitEvent(run.st, sc->ev_join, 0));
    return false;
}

// The resolve of a pass: k_resolve_bits after a chunked primary (rc.slot_bits), k_resolve after an un-chunked one; sq: the
// sums of the squares too (SPT_FILM_MOMENTS)
void launch_resolve(const RenderRun& run, const RenderCtx& rc, float* sq, hipStream_t st) {
    const dim3 grid(rc.n_tiles), block(kBlock);
    if (sq != nullptr) {
        void (*const fn)(RenderCtx, float*) = rc.slot_bits ? k_resolve_bits<16u, true, float*> : k_resolve<true, float*>;
        hipLaunchKernelGGL(fn, grid, block, 0, st, rc, sq);
    } else {
        void (*const fn)(RenderCtx) = rc.slot_bits ? (run.resolve32 ? k_resolve_bits<32u> : k_resolve_bits<16u>) : k_resolve<>;
        hipLaunchKernelGGL(fn, grid, block, 0, st, rc);
    }
}

// The bucket sums of a bucketed film, after the resolve of the same pass: the same slots once more, every sample into the bucket of
// its plan index
void launch_resolve_buckets(const RenderRun& run, const RenderCtx& rc, const SampleTarget& tgt) {
    const dim3 grid(rc.n_tiles), block(kBlock);
    void (*const fn)(RenderCtx, uint32_t, float*, size_t) = rc.slot_bits ? k_resolve_buckets<true> : k_resolve_buckets<false>;
    hipLaunchKernelGGL(fn, grid, block, 0, run.st, rc, tgt.n_buckets, tgt.buckets, tgt.bucket_plane);
}

// The pass counters of one pass into the call's statistics; the vertices of bounce 1 become the scene's tail-loop hint
void read_counters(RenderRun& run, const RenderCtx& rc, size_t counts_words) {
    const uint32_t max_depth = run.params->max_depth;
    const std::vector<uint32_t>& h = run.h_counts;
    run.h_counts.resize(counts_words);
    HIP_CHECK(hipMemcpyAsync(run.h_counts.data(), rc.counts, counts_words * sizeof(uint32_t), hipMemcpyDeviceToHost, run.st));
    HIP_CHECK(hipStreamSynchronize(run.st));
    run.seg_closest += (uint64_t)rc.n_pixels * rc.pass_samples;
    auto qsum = [&](uint32_t b, uint32_t q) {
        uint64_t t = 0;
        for (uint32_t s = 0; s < kShards; ++s) t += h[((size_t)(b * Q_KINDS + q) * kShards + s) * 32];
        if (q == Q_HIT)     // the hit queue's other classes (bounce >= 1 of the general pipeline)
            for (uint32_t c = 1; c < kClasses; ++c)
                for (uint32_t s = 0; s < kShards; ++s) t += h[((size_t)(b * Q_KINDS + Q_HIT_CLASS1 + c - 1u) * kShards + s) * 32];
        return t;
    };
    if (max_depth > 1) run.sc->tail_vertices = qsum(1, Q_HIT);
    run.primary_hits += qsum(0, Q_HIT);
    run.shadow_first += qsum(0, Q_SHADOW);
    if (max_depth > 1) run.vertices_second += qsum(1, Q_HIT);
    for (uint32_t b = 0; b < max_depth; ++b) {
        run.path_vertices += qsum(b, Q_HIT);
        run.seg_shadow += qsum(b, Q_SHADOW);
        if (b + 1 < max_depth) run.seg_closest += qsum(b, Q_EXT);
    }
}

// One window of whole image rows through the wavefront pipeline.  A shard is one window (row_base 0, the
// strip formula of the ABI); a wide box filter renders bands of consecutive rows (w_count = w_strip = 1).
// collect: keep every sample's radiance (3 planes [c][sample][pixel] in sc->rad) instead of summing it into
// the film.  tgt: the samples of the plan this call adds and the sums they go to (see SampleTarget).  Returns the
// context the resolve kernels of the caller need.
RenderCtx trace_window(RenderRun& run, uint32_t row_base, uint32_t rows, uint32_t w_index, uint32_t w_count, uint32_t w_strip, bool collect,
                       const SampleTarget& tgt) {
    spt_scene* const sc = run.sc;
    const spt_render_params& p = *run.params;
    if ((uint64_t)rows * p.width > 0x7fffffffull) fail(SPT_ERR_UNSUPPORTED, "render: window larger than 2^31 pixels");
    RenderCtx rc = plan_ctx(p, *run.cam, row_base, rows, w_index, w_count, w_strip);
    const uint32_t n_pix = rc.n_pixels;
    // a camera model on a scene that samples textures: the kernel leaves the auxiliary rays of the pass for the kAux bounce-0 launch
    const bool cam_aux = run.general && sc->textured && !sc->simple && !run.fused && p.max_depth > 0u;
    const PassShape ps = grow_workspace(sc, p, tgt.count, collect && tgt.keep == nullptr, run.fused, run.class_queues, tgt.sum, tgt.keep != nullptr,
                                        run.general, cam_aux, rc);
    if (cam_aux) run.ray_aux = sc->cam_aux.as<float4>();
    if (run.general) {   // no pinhole eye: no bounding-sphere early-out, no screen bound
        rc.bs_valid = 0u;
        rc.cull_i0 = 0; rc.cull_i1 = (int32_t)p.width - 1; rc.cull_j0 = 0; rc.cull_j1 = (int32_t)p.height - 1;
    } else screen_bound(sc, p, *run.cam, run.pixel_cull, rc);
    rc.dyn_refill_below = run.dyn_refill_below;
    rc.dyn_steps = run.dyn_steps;
    rc.stream_rounds = run.stream_rounds;
    rc.stream_refill_below = run.stream_refill_below;
    rc.visits = sc->visits.as<unsigned long long>();
    rc.row_span = run.row_span_dev;
    const LiveCount live = count_live(sc, run.env || run.general, rc);
    // The candidate masks of this window's blocks: every render, ahead of its first k_primary on the same stream (whose earlier launches read the
    // masks before this one overwrites them, by stream order).  Here, with the rest of the workspace: a growing buffer drains both streams and
    // resets the overlap state, which the lines below set for this render.
    if (run.use_cand && p.max_depth != 0u && rc.n_tiles != 0u) {
        const uint32_t n_blocks = rc.n_tiles * 4u;
        grow(sc, sc->block_cand, (size_t)n_blocks * sizeof(uint64_t));
        run.begin(SPT_K_OTHER);
        hipLaunchKernelGGL((k_block_candidates<SPT_BC_MAX_TRIS>), dim3((n_blocks + 63u) / 64u), dim3(64), 0, run.st, run_scene(run, true), rc,
                           sc->block_cand.as<uint64_t>(), n_blocks);
        HIP_CHECK(hipGetLastError());
        run.end();
    }
    // The overlapped schedule (run.film_overlap, asked for by spt_render): the main stream traces pass p + 1 into one set of
    // the doubled pass buffers while the film stream finishes pass p from the other - its tail-loop shade launch when that
    // kernel is chosen, and its resolve.  Neither needs the vector ALU that k_primary keeps busy.  Without memory for the
    // second set the render stays on the main stream.
    if (run.film_overlap && !grow_second_set(sc)) {
        run.film_overlap = false;
        film_join(sc);
    }
    const bool ov = run.film_overlap;
    const hipStream_t st_film = ov ? sc->stream_film : run.st;
    // The pass pipeline, for the overlapped renders of a fused plan: a third stage between the two.  The main stream only fills the counters
    // and traces the camera rays of a pass (ev_prim[set]); stream2 - never the shadow side stream of a fused plan - runs the bounce launches
    // behind that event (ev_main[set]); the film stream does what it did.  k_primary of pass p + 1 then runs beside the bounce-0 shade kernel
    // of pass p, and nothing on the main stream waits for the film stream's tail launch any more, because the path and hit queues a pass
    // writes exist once per set too (grow_pipeline_set): whoever writes a set next is behind ev_film[set].  Without memory for them the
    // render keeps the two-stream schedule.
    // The second set is made by a scene's first spt_render of such a plan, synchronous or not (run.pipe_plan): allocating it takes up to
    // seconds at the headline's size (profiles/r08_experiments.md), which belongs with the first render's workspace growth, not in the first
    // asynchronous frame behind a synchronous warm-up.  A caller that only ever renders synchronously holds that memory for nothing:
    // SPT_NO_PASS_PIPELINE=1 or SPT_PASS_PIPELINE_MAX_BYTES is for them.
    QueueSet q1{};
    const bool pipe_ready = run.pipe_plan && !collect && tgt.keep == nullptr && grow_pipeline_set(sc, run.pipe_max_bytes, q1);
    // ... and so does everything else that only a first overlapped frame would do (measured: 30 - 36 ms inside the first frame queued behind a
    // synchronous warm-up, in most processes): set 1 of the doubled pass buffers, and the first command on stream2 and on the film stream, with
    // which the runtime makes their hardware queues.  (Nothing has used queue set 1 before pipe_warm is set.)
    if (pipe_ready) {
        (void)grow_second_set(sc);
        if (!sc->pipe_warm && sc->hit_inst_1.bytes >= 4 && sc->hit_f4_1.bytes >= 4) {
            HIP_CHECK(hipMemsetAsync(sc->hit_inst_1.p, 0, 4, sc->stream2));
            HIP_CHECK(hipMemsetAsync(sc->hit_f4_1.p, 0, 4, sc->stream_film));
            HIP_CHECK(hipStreamSynchronize(sc->stream2));
            HIP_CHECK(hipStreamSynchronize(sc->stream_film));
            sc->pipe_warm = true;
        }
    }
    const bool pipe = ov && pipe_ready;
    const QueueSet q0{rc.qa, rc.qb, rc.hits, rc.hits_next};
    // a switch between the two schedules with passes in flight (SPT_NO_PASS_PIPELINE changed): they order the shared queues differently, so
    // this render starts behind all of it
    if (ov && sc->film_pending && sc->ov_mode != (pipe ? 2 : 1)) film_join(sc);
    if (ov) {
        sc->ov_mode = pipe ? 2 : 1;
        sc->film_pending = sc->film_inflight = true;
        // the film stream starts behind what the main stream holds so far (an earlier single-stream render's use of the film)
        HIP_CHECK(hipEventRecord(sc->ev_main[1], run.st));
        HIP_CHECK(hipStreamWaitEvent(st_film, sc->ev_main[1], 0));
    }
    if (tgt.zero) {   // (overlapped: behind the previous frame's k_finish, ahead of this frame's first resolve, by stream order)
        HIP_CHECK(hipMemsetAsync(rc.film, 0, (size_t)n_pix * 3 * sizeof(float), st_film));
        if (tgt.sq) HIP_CHECK(hipMemsetAsync(tgt.sq, 0, (size_t)n_pix * 3 * sizeof(float), st_film));
    }
    if (collect && tgt.keep == nullptr) HIP_CHECK(hipMemsetAsync(sc->rad[0].p, 0, (size_t)ps.rad_slots * 3 * sizeof(float), run.st));   // pixels outside the screen bound write no slots
    bool chunked_any = false;
    // max_depth 0: `while curr_depth < self.max_depth` (pt.rs:48) never runs, every sample is black - environment included.
    // Nothing is traced: the film (and, for a wide box filter, the kept samples) stay at the zeros written above.  (The
    // passes below would mark the hits' radiance slots as owned and no shade launch would ever write them.)
    // Passes start anywhere in the plan (a film's increment at its first uncovered sample): the slot bits, the chunks and the
    // packed sample index of k_primary count from the pass's first sample, only the sampler sees the plan's index pass_first + s.
    const uint32_t s_end = tgt.first + tgt.count;
    for (uint32_t s0 = tgt.first; s0 < (p.max_depth == 0u ? tgt.first : s_end); s0 += ps.spp_pass) {
        // (the sets alternate across renders too: a shard whose frame is ONE pass still traces beside the previous frame's resolve)
        const uint32_t set = ov ? sc->next_set : 0u;
        if (ov) sc->next_set ^= 1u;
        rc.counts = sc->counts[set].as<uint32_t>();
        rc.first_slot = sc->first_slot[set].as<uint32_t>();
        if (pipe) {
            const QueueSet& q = set ? q1 : q0;
            rc.qa = q.qa; rc.qb = q.qb; rc.hits = q.hits; rc.hits_next = q.hits_next;
        }
        // the film stream may still read this set: the pass before the previous one, of this render or an earlier one (pipelined: and that
        // pass's shade stage, which its film stage waited for)
        if (ov && sc->film_recorded[set]) HIP_CHECK(hipStreamWaitEvent(run.st, sc->ev_film[set], 0));
        rc.pass_first = s0;
        rc.pass_samples = std::min(ps.spp_pass, s_end - s0);
        rc.rad_plane = collect ? (size_t)p.spp * n_pix : (size_t)rc.pass_samples * n_pix;
        rc.pack_first = (run.pack_first && !run.general && rc.pass_samples <= 4096u) ? 1u : 0u;
        run.ray_aux_wrap = cam_aux ? rc.pass_samples * n_pix : 0u;
        if (tgt.keep != nullptr) {   // a sample-keeping film: the pass's own chunk, laid out like a pass that is not kept
            rc.rad_plane = (size_t)rc.pass_samples * n_pix;
            rc.rad = tgt.keep[(s0 - tgt.first) / ps.spp_pass];
        } else {
            rc.rad = sc->rad[set].as<float>() + (collect ? (size_t)(s0 - tgt.first) * n_pix : 0);
        }
        run.begin(SPT_K_OTHER);
        HIP_CHECK(hipMemsetAsync(rc.counts, 0, ps.counts_words * sizeof(uint32_t), run.st));
        run.end();
        run.begin(SPT_K_PRIMARY);
        chunked_any |= primary_pass(run, rc, tgt, live.active_tiles, collect, sc->slot_bits[set].as<uint8_t>());
        run.end();
        const hipStream_t st_shade = pipe ? sc->stream2 : run.st;   // the stream of the bounce launches
        if (pipe) {
            HIP_CHECK(hipEventRecord(sc->ev_prim[set], run.st));
            HIP_CHECK(hipStreamWaitEvent(st_shade, sc->ev_prim[set], 0));
            sc->shade_pending = true;
        }
        bool handed_over = false;   // the film stream waits for the main stream's (pipelined: the shade stage's) part of this pass
        auto hand_over = [&] {
            HIP_CHECK(hipEventRecord(sc->ev_main[set], st_shade));
            HIP_CHECK(hipStreamWaitEvent(st_film, sc->ev_main[set], 0));
            handed_over = true;
        };
        bool tail_on_film = false;
        const uint32_t n_bounces = run.albedo ? std::min(p.max_depth, 1u) : p.max_depth;   // an albedo plan's paths end at their first surface
        for (uint32_t b = 0; b < n_bounces; ++b) {
            if (ov && takes_tail_loop(run, b)) {   // reads qb / hit_*_next and this set; the next k_primary writes neither
                hand_over();
                (void)bounce(run, rc, b, st_film);
                tail_on_film = true;
                break;
            }
            // bounce 0 writes qb / hit_*_next (un-fused: and the shadow queue), which a tail-loop launch still on the film
            // stream reads; the later bounces of a pass without that launch ping-pong through the queues on the main stream
            // (pipelined: that launch reads its own set's queues, and the bounces ping-pong on stream2)
            if (ov && !pipe && b == 0u && sc->tail_set >= 0) {
                HIP_CHECK(hipStreamWaitEvent(run.st, sc->ev_film[sc->tail_set], 0));
                sc->tail_set = -1;
            }
            if (bounce(run, rc, b, st_shade)) break;
        }
        if (!collect) {
            if (ov && !handed_over) hand_over();
            run.begin(SPT_K_RESOLVE);
            launch_resolve(run, rc, tgt.sq, st_film);
            if (tgt.buckets != nullptr) launch_resolve_buckets(run, rc, tgt);
            run.end();
            if (ov) {
                HIP_CHECK(hipEventRecord(sc->ev_film[set], st_film));
                sc->film_recorded[set] = true;
                if (tail_on_film) sc->tail_set = (int)set;   // (pipelined: for spt_scene_update only, the launch reads the scene)
                ++sc->passes_film;
                if (pipe) ++sc->passes_pipe;
            }
        }
        if (!ov) ++sc->passes_single;
        if (run.stats) read_counters(run, rc, ps.counts_words);
    }
    run.samples_traced += (uint64_t)n_pix * tgt.count;
    if (chunked_any) run.live_samples += live.live_pixels * tgt.count;
    return rc;
}

// ---- sample-keeping films (SPT_FILM_KEEP_SAMPLES) ----
// The device time between the scene's two ev_keep events, both reached (spt_debug_render_info)
uint64_t keep_elapsed_ns(spt_scene* sc) {
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, sc->ev_keep[0], sc->ev_keep[1]));
    return (uint64_t)((double)ms * 1e6);
}

// The runs of a new film: every run of consecutive own rows with max(R, 0) halo rows each way, as spt_render's band loop cuts them
// (a run is never split: the store is what the film is for).  The scene's lock is held.
void make_kept_runs(spt_film* f) {
    spt_scene* const sc = f->sc;
    const spt_render_params& p = f->plan;
    const uint32_t shard_count = p.shard_count ? p.shard_count : 1u, strip_rows = p.strip_rows ? p.strip_rows : 1u;
    const uint32_t halo = (uint32_t)std::max(f->R, 0);
    std::vector<uint32_t> own;
    for (uint32_t j = 0; j < p.height; ++j)
        if ((j / strip_rows) % shard_count == p.shard_index) own.push_back(j);
    uint64_t stored = 0;
    for (size_t k = 0; k < own.size();) {
        size_t e = k + 1;
        while (e < own.size() && own[e] == own[e - 1] + 1u) ++e;
        spt_film::KeptRun& r = f->runs.emplace_back();
        r.j0 = own[k]; r.j1 = own[e - 1] + 1u;
        r.b0 = r.j0 >= halo ? r.j0 - halo : 0u;
        r.b1 = (uint32_t)std::min<uint64_t>(p.height, (uint64_t)r.j1 + halo);
        r.out_row = k;
        stored += (uint64_t)(r.b1 - r.b0) * p.width;
        k = e;
    }
    if (stored > 0x7fffffffull) fail(SPT_ERR_UNSUPPORTED, "film_create: a sample-keeping film of more than 2^31 - 1 stored pixels (own rows and halo rows)");
    for (hipEvent_t& e : sc->ev_keep)
        if (!e) HIP_CHECK(hipEventCreate(&e));
}

// One increment of a sample-keeping film: per run, the chunks of its passes are allocated and zeroed (collect mode writes no slot
// for a black sample or a pixel outside the screen bound), one trace_window in collect mode fills them.  The film changes only after
// every run has worked: an increment that fails (no memory for a chunk) leaves it as it was.
void kept_render(spt_film* f, RenderRun& run, uint32_t n_samples) {
    const spt_render_params& p = f->plan;
    const uint32_t s_first = f->first + f->done;
    struct NewChunks {
        std::vector<std::unique_ptr<DeviceBuffer>> bufs;
        std::vector<KeptChunk> table;
        DeviceBuffer table_dev;
    };
    std::vector<NewChunks> fresh(f->runs.size());
    for (size_t k = 0; k < f->runs.size(); ++k) {
        spt_film::KeptRun& r = f->runs[k];
        NewChunks& nc = fresh[k];
        const uint32_t n_band = (r.b1 - r.b0) * p.width;
        const uint32_t spp_pass = pass_samples_of(p, n_band, n_samples);
        std::vector<float*> ptrs;
        for (uint32_t s0 = 0; s0 < n_samples; s0 += spp_pass) {
            const uint32_t n = std::min(spp_pass, n_samples - s0);
            auto buf = std::make_unique<DeviceBuffer>();
            buf->alloc((size_t)n * n_band * 3 * sizeof(float));
            HIP_CHECK(hipMemsetAsync(buf->p, 0, buf->bytes, run.st));
            ptrs.push_back(buf->as<float>());
            nc.table.push_back(KeptChunk{buf->as<float>(), s_first + s0, n});
            nc.bufs.push_back(std::move(buf));
        }
        SampleTarget inc{s_first, n_samples, nullptr, nullptr, false};
        inc.keep = ptrs.data();
        (void)trace_window(run, r.b0, r.b1 - r.b0, 0u, 1u, 1u, true, inc);
        HIP_CHECK(hipGetLastError());
        // the chunk table the read-outs will take: the old entries and the new ones
        std::vector<KeptChunk> table = r.table;
        table.insert(table.end(), nc.table.begin(), nc.table.end());
        nc.table.swap(table);
        nc.table_dev.alloc(nc.table.size() * sizeof(KeptChunk));
        HIP_CHECK(hipMemcpyAsync(nc.table_dev.p, nc.table.data(), nc.table.size() * sizeof(KeptChunk), hipMemcpyHostToDevice, run.st));
    }
    HIP_CHECK(hipStreamSynchronize(run.st));   // (the tables are pageable; every trace has worked)
    for (size_t k = 0; k < f->runs.size(); ++k) {
        spt_film::KeptRun& r = f->runs[k];
        for (auto& b : fresh[k].bufs) r.chunks.push_back(std::move(b));
        r.table.swap(fresh[k].table);
        r.table_dev.swap(fresh[k].table_dev);
    }
}

// What the kernels of a sample-keeping film read of one of its runs; `out`: the run's first own row in a packed buffer
KeptJob kept_job(const spt_film* f, const spt_film::KeptRun& r, float* out, bool mean) {
    return KeptJob{r.table_dev.as<KeptChunk>(), (uint32_t)r.table.size(), r.b0, r.b1 - r.b0, r.j0, r.j1 - r.j0, out, f->R, f->radius, mean ? 1u : 0u};
}

// The read-out of one run under the film's weighted filter (spt_film_filter): the job of the box with Rf and r in the place of the
// plan's R and radius.  Samples requested together per lane: kFilterBatch ("Reconstruction filters").
constexpr uint32_t kFilterBatch = 4u;
void launch_filter_weighted(const spt_film* f, dim3 grid, hipStream_t st, const RenderCtx& rc, KeptJob job) {
    job.R = f->filter_R;
    job.radius = f->filter_radius;
    auto* k = k_film_filter_weighted<SPT_FILTER_TENT, kFilterBatch>;
    if (f->filter_type == SPT_FILTER_GAUSSIAN) k = k_film_filter_weighted<SPT_FILTER_GAUSSIAN, kFilterBatch>;
    if (f->filter_type == SPT_FILTER_MITCHELL) k = k_film_filter_weighted<SPT_FILTER_MITCHELL, kFilterBatch>;
    hipLaunchKernelGGL(k, grid, dim3(kBlock), 0, st, rc, job, f->filter_coef);
}

// The device-visible address of spt_render's destination when k_finish_host may store into it, else nullptr (the frame then
// takes the runtime's copy): the first and the last byte of the span the shard writes must both be mapped for the device, exactly
// that span apart - pageable memory, a buffer pinned only in part and two unrelated mappings all fail one of the three.  Asked anew
// for every call: the caller may unpin or free the buffer between two renders.
float* direct_destination(const spt_render_params& p, uint32_t own_rows, uint32_t strip_rows, float* host, OutLayout* lay) {
    if (((uintptr_t)host & 3u) != 0u || (p.out_strip_stride & 3u) != 0u) return nullptr;
    void *d_first = nullptr, *d_last = nullptr;
    if (hipHostGetDevicePointer(&d_first, host, 0) != hipSuccess || !d_first) { (void)hipGetLastError(); return nullptr; }
    *lay = out_layout(own_rows, p.width, strip_rows, p.out_strip_stride, (uint64_t)(uintptr_t)d_first);
    const uint64_t span = out_layout_span(*lay) * sizeof(float);
    if (span == 0u) return nullptr;
    if (hipHostGetDevicePointer(&d_last, (char*)host + (span - 1u), 0) != hipSuccess || !d_last) { (void)hipGetLastError(); return nullptr; }
    if ((uintptr_t)d_last - (uintptr_t)d_first != span - 1u) return nullptr;
    return (float*)d_first;
}

// spt_scene_update and spt_scene_deform under the scene's lock (`who` names the call in the messages; n_meshes == 0: an update).
// Everything of the scene that depends on its instances and lights is built again on the host from the new arrays (build_dynamic
// of scene_build.h, the function spt_scene_create runs), then committed: the device copies through one page-locked slot, by copies
// queued on the render stream behind the kernels of the frames queued so far, the host side last.  A deformation first makes the
// fixed part of the named meshes again, in a copy (scene_build.h, deform_fixed_*): on a large scene that is a box per mesh, and the
// call queues the triangles' copies and the refit kernels (deform_kernels.h) in front of the dynamic sections' copies; an
// LDS-resident scene's blob is written whole as by any update.  Nothing of the scene is touched before the first copy is queued,
// so a refused call leaves it as it was.
// spt_scene_deform_vertices on a large scene: one named mesh, checked by the caller (vertices_locked) - what goes up instead of
// records, and the raw bounds of the vertices some face names
struct VertexEdit {
    uint32_t mesh;
    const float* positions;
    const float* normals;   // or null: the ones on the device stay
    RefitBox raw;
};

spt_status update_locked(spt_scene* sc, const spt_scene_update_desc* u, uint32_t n_meshes, const spt_mesh_deform* meshes, const char* who,
                         const VertexEdit* verts = nullptr) {
    const std::string w(who);
    return guarded(who, [&] {
        const BuildOptions opt = build_options();
        if (u->flags != 0u) fail(SPT_ERR_INVALID_ARG, w + ": unknown flags");
        if (sc->live_films != 0u) fail(SPT_ERR_INVALID_ARG, w + ": destroy the scene's films first (a film accumulates samples of one scene)");
        if (u->n_instances != sc->fixed.n_instances) fail(SPT_ERR_INVALID_ARG, w + ": n_instances differs from the scene's (objects cannot appear or vanish)");
        if (u->n_lights != sc->fixed.n_lights) fail(SPT_ERR_INVALID_ARG, w + ": n_lights differs from the scene's");
        if ((u->n_tlas_nodes && !u->tlas_nodes) || (u->n_instances && !u->instances) || (u->n_lights && !u->lights)) fail(SPT_ERR_INVALID_ARG, w + ": null array");
        if (u->n_instances && sc->fixed.aggregate == SPT_AGGREGATE_BVH && u->n_tlas_nodes == 0) fail(SPT_ERR_INVALID_ARG, w + ": bvh aggregate without TLAS nodes");
        if (!verts) validate_deform(sc->fixed, n_meshes, meshes);
        // a deformation: the fixed part with the named meshes made again, committed with the rest
        SceneFixed deformed;
        std::vector<std::pair<uint32_t, uint32_t>> blas_range = sc->blas_range;
        std::vector<RefitBox> root_box;
        if (n_meshes) {
            deformed = sc->fixed;
            if (verts) {
                std::vector<uint32_t> ids(n_meshes);
                std::vector<RefitBox> raw(n_meshes);
                for (uint32_t i = 0; i < n_meshes; ++i) { ids[i] = verts[i].mesh; raw[i] = verts[i].raw; }
                root_box = deform_fixed_n4_raw(deformed, n_meshes, ids.data(), raw.data());
            } else if (deformed.n4) root_box = deform_fixed_n4(deformed, n_meshes, meshes);
            else deform_fixed_lds(deformed, blas_range, n_meshes, meshes, opt);
        }
        const SceneFixed& fx = n_meshes ? deformed : sc->fixed;
        const DynView view{fx.aggregate, fx.light_sampler, u->n_tlas_nodes, u->n_instances, u->n_lights, fx.n_spheres, fx.n_meshes, fx.n_bezier_patches, fx.n_surfaces,
                           fx.has_env, u->tlas_nodes, u->instances, u->lights, u->light_alias, fx.surf_emissive.data()};
        validate_instances(view, opt, who);
        validate_lights(view, who);
        if (fx.env_light_index >= 0 && u->lights[fx.env_light_index].type != fx.env_light_type)
            fail(SPT_ERR_INVALID_ARG, w + ": the light at env_light_index may not change its type");
        validate_light_alias(view, who);
        // the new state, on the host (nothing of it is committed before the refusals below)
        const StaticSections st{fx.wblas.data(), fx.tri_sec.data()};
        SceneDynamic dy = build_dynamic(fx, view, opt, sc->lds_geo, blas_range.size(), fx.n4 ? nullptr : &st);
        if (sc->lds_geo && !lds_fits(dy.plain_f4))
            fail(SPT_ERR_UNSUPPORTED, w + ": the traversal geometry would no longer fit LDS, where the scene's BLAS nodes are laid out for: recreate the scene");
        if (fx.n4 && (size_t)dy.geo_f4 - fx.tail_first > fx.tail_cap)
            fail(SPT_ERR_UNSUPPORTED, w + ": the caller's TLAS needs more room than the scene reserved: recreate the scene");
        // the slot: [triangles and attributes of the named meshes | instances | classes | lights | alias props, u, k | blob]
        const bool pis = fx.light_sampler == SPT_LIGHT_SAMPLER_POWER_IS && fx.n_lights != 0;
        struct Part { void* dst; const void* src; size_t bytes, at; };
        std::vector<Part> parts;
        size_t total = 0;
        auto part = [&](void* dst, const void* src, size_t bytes) {
            if (!bytes) return;
            parts.push_back(Part{dst, src, bytes, total});
            total += (bytes + 15) / 16 * 16;
        };
        for (uint32_t i = 0; verts && i < n_meshes; ++i) {   // the vertex arrays the kernels of inst_assemble.hip make those records from
            spt_scene::MeshTopology& tp = *sc->topology[verts[i].mesh];
            part(tp.d_positions.p, verts[i].positions, (size_t)tp.n_vertices * 3 * sizeof(float));
            if (verts[i].normals) part(tp.d_normals.p, verts[i].normals, (size_t)tp.n_vertices * 3 * sizeof(float));
        }
        for (uint32_t i = 0; !verts && i < n_meshes; ++i) {   // the ABI-order arrays the shade kernels (and the refit kernels) read
            const spt_mesh_deform& e = meshes[i];
            part(sc->tri_pos.as<spt_tri_pos>() + fx.mesh_first[e.mesh], e.tri_pos, (size_t)e.tri_count * sizeof(spt_tri_pos));
            if (e.tri_attr) part(sc->tri_attr.as<spt_tri_attr>() + fx.mesh_first[e.mesh], e.tri_attr, (size_t)e.tri_count * sizeof(spt_tri_attr));
        }
        const size_t geometry_parts = parts.size();
        part(sc->instances.p, u->instances, (size_t)fx.n_instances * sizeof(spt_instance));
        part(sc->inst_class.p, dy.cls.data(), fx.n_instances);
        part(sc->lights.p, u->lights, (size_t)fx.n_lights * sizeof(spt_light));
        if (pis) {
            part(sc->light_props.p, u->light_alias.props, (size_t)fx.n_lights * sizeof(float));
            part(sc->light_u.p, u->light_alias.u, (size_t)fx.n_lights * sizeof(float));
            part(sc->light_k.p, u->light_alias.k, (size_t)fx.n_lights * sizeof(uint32_t));
        }
        part(sc->geo.as<float4>() + (fx.n4 ? fx.tail_first : 0u), dy.blob.data(), dy.blob.size() * 16);
        // the origin-candidate table of the new state (instances moved, vertices deformed: both are in dy.blob), behind the blob
        std::vector<uint64_t> origin_words;
        spt_oc_info origin_info{};
        const auto origin_t0 = std::chrono::steady_clock::now();
        const bool origin_ok = origin_table(dy, fx.n_instances, fx.n_meshes, origin_words, origin_info);
        const uint64_t origin_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - origin_t0).count();
        if (origin_ok) part(sc->origin_cand.p, origin_words.data(), kOriginBytes);
        if ((fx.n4 ? (size_t)fx.tail_first * 16 : 0) + dy.blob.size() * 16 > sc->geo.bytes) fail(SPT_ERR_UNSUPPORTED, w + ": the geometry blob outgrew its allocation: recreate the scene");
        HIP_CHECK(hipSetDevice(sc->device));
        if (!sc->ev_upd) HIP_CHECK(hipEventCreateWithFlags(&sc->ev_upd, hipEventDisableTiming));
        if (sc->upd_recorded) HIP_CHECK(hipEventSynchronize(sc->ev_upd));   // the previous update's copies still read the slot
        sc->upd_recorded = false;
        sc->upd_stage.ensure(std::max<size_t>(total, 16));
        // the refit's scratch, made by the first deformation of a large scene: raw bounds and a height per BLAS node
        const bool refit = n_meshes != 0 && fx.n4;
        const size_t n_nodes = fx.blas_f4 / 4u;
        if (refit && n_nodes != 0 && !sc->refit_raw.p) {
            sc->refit_raw.alloc(n_nodes * sizeof(RefitBox));
            sc->refit_height.alloc(n_nodes);
            sc->refit_heights_known.assign(fx.n_meshes, 0);
        }
        if (n_meshes && !sc->ev_deform[0])
            for (hipEvent_t& e : sc->ev_deform) HIP_CHECK(hipEventCreate(&e));
        for (const Part& pt : parts) std::memcpy(static_cast<char*>(sc->upd_stage.p) + pt.at, pt.src, pt.bytes);
        // Of what an overlapped render leaves on the film stream only a tail-loop launch reads the scene (the resolves, the finish
        // kernel and the copy-out read the render workspace): the copies go behind that launch, as the next frame's bounce 0 would,
        // and the copy-out of the previous frame goes on beside them and beside the next frame's kernels
        // A pipelined render's bounce launches on stream2 read the scene as well: behind them too.
        if (sc->tail_set >= 0) {
            HIP_CHECK(hipStreamWaitEvent(sc->stream, sc->ev_film[sc->tail_set], 0));
            sc->tail_set = -1;
        }
        shade_join(sc);
        auto queue_copy = [&](const Part& pt) {
            HIP_CHECK(hipMemcpyAsync(pt.dst, static_cast<const char*>(sc->upd_stage.p) + pt.at, pt.bytes, hipMemcpyHostToDevice, sc->stream));
        };
        // the named meshes' triangles, then (large scene) their kernels, then the dynamic sections: the streaming walker's entries
        // carry the mesh records' new boxes, so a frame sees either all of a deformation or none of it
        if (n_meshes) HIP_CHECK(hipEventRecord(sc->ev_deform[0], sc->stream));
        for (size_t k = 0; k < geometry_parts; ++k) queue_copy(parts[k]);
        for (uint32_t i = 0; refit && i < n_meshes; ++i) {
            const uint32_t mesh = verts ? verts[i].mesh : meshes[i].mesh;
            if (verts) {   // the mesh's records from the vertex arrays the copies above brought, where k_deform_tris reads them
                const spt_scene::MeshTopology& tp = *sc->topology[mesh];
                AssembleMesh am{};
                am.m.n_vertices = tp.n_vertices; am.m.tri_count = tp.tri_count;
                am.m.indices = tp.d_indices.as<uint32_t>(); am.m.face_of_tri = tp.d_face_of_tri.as<uint32_t>();
                am.m.corner_first = tp.d_corner_first.as<uint32_t>(); am.m.corners = tp.d_corners.as<uint32_t>();
                am.m.uv = tp.d_uv.as<float>(); am.m.positions = tp.d_positions.as<float>(); am.m.normals = tp.d_normals.as<float>();
                am.tan = tp.d_tan.as<float>(); am.bit = tp.d_bit.as<float>();
                am.tri_pos = sc->tri_pos.as<float4>(); am.tri_attr = sc->tri_attr.as<float4>();
                am.tri_first = fx.mesh_first[mesh]; am.n_tris = fx.n_tris;
                hipLaunchKernelGGL(k_vertex_frames, dim3((tp.n_vertices + kBlock - 1u) / kBlock), dim3(kBlock), 0, sc->stream, am);
                hipLaunchKernelGGL(k_assemble_tris, dim3((tp.tri_count + kBlock - 1u) / kBlock), dim3(kBlock), 0, sc->stream, am);
            }
            DeformMesh dm{};
            dm.geo = sc->geo.as<float4>();
            dm.tri_pos = sc->tri_pos.as<float4>();
            dm.raw = sc->refit_raw.as<RefitBox>();
            dm.height = sc->refit_height.as<uint8_t>();
            dm.o_tri = sc->d.o_tri; dm.o_blas = sc->d.o_blas; dm.o_mesh = sc->d.o_mesh;   // (static sections: no update moves them)
            dm.mesh = mesh;
            dm.tri_first = fx.mesh_first[mesh]; dm.tri_count = fx.mesh_tris[mesh];
            dm.node_first = fx.n4_nodes[mesh][0]; dm.node_count = fx.n4_nodes[mesh][1];
            for (int k = 0; k < 3; ++k) { dm.root_lo[k] = root_box[i].lo[k]; dm.root_hi[k] = root_box[i].hi[k]; }
            const uint32_t levels = fx.n4_nodes[mesh][2] + 1u;
            const dim3 tri_grid((dm.tri_count + kBlock - 1u) / kBlock), node_grid((dm.node_count + kBlock - 1u) / kBlock);
            hipLaunchKernelGGL(k_deform_tris, tri_grid, dim3(kBlock), 0, sc->stream, dm);
            if (dm.node_count == 0u) continue;   // the root is a leaf: the mesh record's box is all there is
            if (!sc->refit_heights_known[mesh]) {
                hipLaunchKernelGGL(k_refit_heights, node_grid, dim3(kBlock), 0, sc->stream, dm, (uint32_t)kRefitUnknown);
                for (uint32_t level = 1; level < levels; ++level) hipLaunchKernelGGL(k_refit_heights, node_grid, dim3(kBlock), 0, sc->stream, dm, level);
                sc->refit_heights_known[mesh] = 1;
            }
            for (uint32_t level = 0; level < levels; ++level) hipLaunchKernelGGL(k_refit_level, node_grid, dim3(kBlock), 0, sc->stream, dm, level);
        }
        if (refit) HIP_CHECK(hipGetLastError());
        for (size_t k = geometry_parts; k < parts.size(); ++k) queue_copy(parts[k]);
        HIP_CHECK(hipEventRecord(sc->ev_upd, sc->stream));
        sc->upd_recorded = true;
        if (n_meshes) {
            HIP_CHECK(hipEventRecord(sc->ev_deform[1], sc->stream));
            sc->deform_timed = true;
            sc->fixed = std::move(deformed);
            sc->blas_range = std::move(blas_range);
        }
        dyn_commit_host(sc, dy, sc->lds_geo);
        sc->origin_ok = origin_ok;
        sc->origin_words = std::move(origin_words);
        sc->origin_info = origin_info;
        sc->origin_build_ns = origin_ns;
        ++sc->updates;
        sc->update_bytes = 0;
        for (const Part& pt : parts) sc->update_bytes += pt.bytes;
        return SPT_OK;
    });
}

// spt_scene_mesh_topology under the scene's lock: the checks, the vertex -> corner table, the synchronous uploads.  The new
// registration replaces the old one only when all of it stands.
spt_status topology_locked(spt_scene* sc, const spt_mesh_topology* t) {
    return guarded("scene_mesh_topology", [&] {
        const SceneFixed& fx = sc->fixed;
        if (!fx.own_bvh) fail(SPT_ERR_UNSUPPORTED, "scene_mesh_topology: the scene walks the caller's trees (SPT_REFERENCE_BVH): the library owns none to refit");
        if (t->mesh >= fx.n_meshes) fail(SPT_ERR_INVALID_ARG, "scene_mesh_topology: mesh index out of range");
        if (t->tri_count == 0u || t->tri_count != fx.mesh_tris[t->mesh]) fail(SPT_ERR_INVALID_ARG, "scene_mesh_topology: tri_count differs from the mesh's");
        if (t->n_vertices == 0u || !t->indices || !t->uv || !t->normals) fail(SPT_ERR_INVALID_ARG, "scene_mesh_topology: null array");
        if ((uint64_t)fx.mesh_first[t->mesh] + t->tri_count > fx.n_tris) fail(SPT_ERR_INVALID_ARG, "scene_mesh_topology: the mesh's range leaves the scene's triangles");
        const size_t nv = t->n_vertices, nt = t->tri_count;
        for (size_t i = 0; i < 3 * nt; ++i)
            if (t->indices[i] >= t->n_vertices) fail(SPT_ERR_INVALID_ARG, "scene_mesh_topology: a vertex index is out of range");
        for (size_t i = 0; i < 2 * nv; ++i)
            if (!std::isfinite(t->uv[i])) fail(SPT_ERR_INVALID_ARG, "scene_mesh_topology: a texture coordinate is not finite");
        for (size_t i = 0; i < 3 * nv; ++i)
            if (!std::isfinite(t->normals[i])) fail(SPT_ERR_INVALID_ARG, "scene_mesh_topology: a normal is not finite");
        auto tp = std::make_unique<spt_scene::MeshTopology>();
        tp->n_vertices = t->n_vertices;
        tp->tri_count = t->tri_count;
        tp->face_of_tri.resize(nt);
        std::vector<uint8_t> seen(nt, 0);
        for (size_t k = 0; k < nt; ++k) {
            const uint32_t face = t->face_of_tri ? t->face_of_tri[k] : (uint32_t)k;
            if (face >= t->tri_count || seen[face]++) fail(SPT_ERR_INVALID_ARG, "scene_mesh_topology: face_of_tri is no permutation of the faces");
            tp->face_of_tri[k] = face;
        }
        tp->indices.assign(t->indices, t->indices + 3 * nt);
        tp->uv.assign(t->uv, t->uv + 2 * nv);
        tp->normals.assign(t->normals, t->normals + 3 * nv);
        // the corners that name a vertex, in increasing (face, corner) order: the order calc_tangents adds them in
        tp->corner_first.assign(nv + 1, 0u);
        for (size_t i = 0; i < 3 * nt; ++i) ++tp->corner_first[tp->indices[i] + 1u];
        tp->named.resize(nv);
        for (size_t v = 0; v < nv; ++v) {
            tp->named[v] = tp->corner_first[v + 1] != 0u;
            tp->corner_first[v + 1] += tp->corner_first[v];
        }
        tp->corners.resize(3 * nt);
        std::vector<uint32_t> at(tp->corner_first.begin(), tp->corner_first.end() - 1);
        for (size_t i = 0; i < 3 * nt; ++i) tp->corners[at[tp->indices[i]]++] = (uint32_t)i;
        HIP_CHECK(hipSetDevice(sc->device));
        tp->d_indices.upload(tp->indices.data(), tp->indices.size());
        tp->d_face_of_tri.upload(tp->face_of_tri.data(), tp->face_of_tri.size());
        tp->d_corner_first.upload(tp->corner_first.data(), tp->corner_first.size());
        tp->d_corners.upload(tp->corners.data(), tp->corners.size());
        tp->d_uv.upload(tp->uv.data(), tp->uv.size());
        tp->d_normals.upload(tp->normals.data(), tp->normals.size());
        tp->d_positions.alloc(3 * nv * sizeof(float));
        tp->d_tan.alloc(3 * nv * sizeof(float));
        tp->d_bit.alloc(3 * nv * sizeof(float));
        if (sc->topology.size() != fx.n_meshes) sc->topology.resize(fx.n_meshes);
        // (the old registration's arrays: freeing them waits for the kernels of a deformation still in flight)
        sc->topology[t->mesh] = std::move(tp);
        return SPT_OK;
    });
}

// spt_scene_deform_vertices under the scene's lock: its own checks, with the bounds of the face-named vertices taken in the same
// pass, then update_locked - on a large scene with the vertex arrays in place of records, on an LDS-resident one with records
// made here, with the kernels' functions.
spt_status vertices_locked(spt_scene* sc, const spt_scene_update_desc* u, uint32_t n_meshes, const spt_mesh_vertices* meshes) {
    const char* who = "scene_deform_vertices";
    return guarded(who, [&]() -> spt_status {
        const SceneFixed& fx = sc->fixed;
        if (n_meshes == 0u) return update_locked(sc, u, 0u, nullptr, who);
        if (!meshes) fail(SPT_ERR_INVALID_ARG, "scene_deform_vertices: null array");
        if (!fx.own_bvh) fail(SPT_ERR_UNSUPPORTED, "scene_deform_vertices: the scene walks the caller's trees (SPT_REFERENCE_BVH): the library owns none to refit");
        std::vector<uint8_t> named(fx.n_meshes, 0);
        std::vector<VertexEdit> edits(n_meshes);
        for (uint32_t i = 0; i < n_meshes; ++i) {
            const spt_mesh_vertices& e = meshes[i];
            if (e.mesh >= fx.n_meshes) fail(SPT_ERR_INVALID_ARG, "scene_deform_vertices: mesh index out of range");
            if (named[e.mesh]++) fail(SPT_ERR_INVALID_ARG, "scene_deform_vertices: a mesh is named twice");
            if (e.mesh >= sc->topology.size() || !sc->topology[e.mesh]) fail(SPT_ERR_INVALID_ARG, "scene_deform_vertices: the mesh has no registered topology (spt_scene_mesh_topology)");
            const spt_scene::MeshTopology& tp = *sc->topology[e.mesh];
            if (e.n_vertices != tp.n_vertices) fail(SPT_ERR_INVALID_ARG, "scene_deform_vertices: n_vertices differs from the registration's");
            if (!e.positions) fail(SPT_ERR_INVALID_ARG, "scene_deform_vertices: null array");
            // (min / max of finite values do not depend on the order they are taken in, but for the sign of a zero, which no
            // padded box keeps: the box deformed_bounds takes over the records)
            RefitBox raw = refit_empty();
            for (size_t v = 0; v < tp.n_vertices; ++v) {
                const float* p = e.positions + 3 * v;
                bool finite = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
                if (e.normals) finite = finite && std::isfinite(e.normals[3 * v]) && std::isfinite(e.normals[3 * v + 1]) && std::isfinite(e.normals[3 * v + 2]);
                if (!finite) fail(SPT_ERR_INVALID_ARG, "scene_deform_vertices: a value is not finite");
                if (!tp.named[v]) continue;
                for (int k = 0; k < 3; ++k) { raw.lo[k] = refit_min(raw.lo[k], p[k]); raw.hi[k] = refit_max(raw.hi[k], p[k]); }
            }
            edits[i] = VertexEdit{e.mesh, e.positions, e.normals, raw};
        }
        if (fx.n4) return update_locked(sc, u, n_meshes, nullptr, who, edits.data());
        // LDS-resident: the records on the host, by the kernels' schedule - per vertex over the table, then per triangle
        std::vector<std::vector<spt_tri_pos>> pos(n_meshes);
        std::vector<std::vector<spt_tri_attr>> attr(n_meshes);
        std::vector<spt_mesh_deform> recs(n_meshes);
        for (uint32_t i = 0; i < n_meshes; ++i) {
            const spt_scene::MeshTopology& tp = *sc->topology[meshes[i].mesh];
            spt_ma_mesh m{};
            m.n_vertices = tp.n_vertices; m.tri_count = tp.tri_count;
            m.indices = tp.indices.data(); m.face_of_tri = tp.face_of_tri.data();
            m.corner_first = tp.corner_first.data(); m.corners = tp.corners.data();
            m.uv = tp.uv.data(); m.positions = meshes[i].positions; m.normals = meshes[i].normals ? meshes[i].normals : tp.normals.data();
            std::vector<float> tan(3 * (size_t)tp.n_vertices), bit(3 * (size_t)tp.n_vertices);
            for (uint32_t v = 0; v < tp.n_vertices; ++v) spt_ma_vertex_frame(&m, v, &tan[3 * (size_t)v], &bit[3 * (size_t)v]);
            pos[i].resize(tp.tri_count);
            attr[i].resize(tp.tri_count);
            for (uint32_t k = 0; k < tp.tri_count; ++k)
                if (!spt_ma_triangle(&m, tan.data(), bit.data(), k, &pos[i][k], &attr[i][k])) fail(SPT_ERR_INVALID_ARG, "scene_deform_vertices: the registration is inconsistent");
            recs[i] = spt_mesh_deform{meshes[i].mesh, tp.tri_count, pos[i].data(), attr[i].data()};
        }
        const spt_status st = update_locked(sc, u, n_meshes, recs.data(), who);
        if (st != SPT_OK) return st;
        for (uint32_t i = 0; i < n_meshes; ++i)   // the normals now in force
            if (meshes[i].normals) sc->topology[meshes[i].mesh]->normals.assign(meshes[i].normals, meshes[i].normals + 3 * (size_t)meshes[i].n_vertices);
        return SPT_OK;
    });
}

}  // namespace

extern "C" {

spt_status spt_scene_mesh_topology(spt_scene* sc, const spt_mesh_topology* t) {
    if (!sc || !t) { g_error = "scene_mesh_topology: null argument"; return SPT_ERR_INVALID_ARG; }
    if (t->size < sizeof(spt_mesh_topology)) { g_error = "scene_mesh_topology: size is smaller than spt_mesh_topology"; return SPT_ERR_INVALID_ARG; }
    if (sc->fwd) {
        if (!sc->fwd->scene_mesh_topology) { g_error = "scene_mesh_topology: libspt_hip_bez.so does not export spt_scene_mesh_topology"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->scene_mesh_topology(sc->inner, t));
    }
    std::lock_guard<std::mutex> lock(sc->mu);
    return topology_locked(sc, t);
}

spt_status spt_scene_deform_vertices(spt_scene* sc, const spt_scene_update_desc* u, uint32_t n_meshes, const spt_mesh_vertices* meshes) {
    if (!sc || !u) { g_error = "scene_deform_vertices: null argument"; return SPT_ERR_INVALID_ARG; }
    if (u->size < sizeof(spt_scene_update_desc)) { g_error = "scene_deform_vertices: size is smaller than spt_scene_update_desc"; return SPT_ERR_INVALID_ARG; }
    if (sc->fwd) {
        if (!sc->fwd->scene_deform_vertices) { g_error = "scene_deform_vertices: libspt_hip_bez.so does not export spt_scene_deform_vertices"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->scene_deform_vertices(sc->inner, u, n_meshes, meshes));
    }
    std::lock_guard<std::mutex> lock(sc->mu);
    return vertices_locked(sc, u, n_meshes, meshes);
}

spt_status spt_scene_read_triangles(const spt_scene* scene_c, uint32_t first, uint32_t count, spt_tri_pos* tri_pos_out, spt_tri_attr* tri_attr_out) {
    if (!scene_c) { g_error = "scene_read_triangles: null argument"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {
        if (!sc->fwd->scene_read_triangles) { g_error = "scene_read_triangles: libspt_hip_bez.so does not export spt_scene_read_triangles"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->scene_read_triangles(sc->inner, first, count, tri_pos_out, tri_attr_out));
    }
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("scene_read_triangles", [&] {
        if ((uint64_t)first + count > sc->fixed.n_tris) fail(SPT_ERR_INVALID_ARG, "scene_read_triangles: the range leaves the scene's triangles");
        if (count == 0u || (!tri_pos_out && !tri_attr_out)) return SPT_OK;
        HIP_CHECK(hipSetDevice(sc->device));
        HIP_CHECK(hipStreamSynchronize(sc->stream));   // behind the copies and kernels of every update queued so far
        if (tri_pos_out) HIP_CHECK(hipMemcpy(tri_pos_out, sc->tri_pos.as<spt_tri_pos>() + first, (size_t)count * sizeof(spt_tri_pos), hipMemcpyDeviceToHost));
        if (tri_attr_out) HIP_CHECK(hipMemcpy(tri_attr_out, sc->tri_attr.as<spt_tri_attr>() + first, (size_t)count * sizeof(spt_tri_attr), hipMemcpyDeviceToHost));
        return SPT_OK;
    });
}

spt_status spt_scene_update(spt_scene* sc, const spt_scene_update_desc* u) {
    if (!sc || !u) { g_error = "scene_update: null argument"; return SPT_ERR_INVALID_ARG; }
    if (u->size < sizeof(spt_scene_update_desc)) { g_error = "scene_update: size is smaller than spt_scene_update_desc"; return SPT_ERR_INVALID_ARG; }
    if (sc->fwd) {
        if (!sc->fwd->scene_update) { g_error = "scene_update: libspt_hip_bez.so does not export spt_scene_update"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->scene_update(sc->inner, u));
    }
    std::lock_guard<std::mutex> lock(sc->mu);
    return update_locked(sc, u, 0u, nullptr, "scene_update");
}

spt_status spt_scene_deform(spt_scene* sc, const spt_scene_update_desc* u, uint32_t n_meshes, const spt_mesh_deform* meshes) {
    if (!sc || !u) { g_error = "scene_deform: null argument"; return SPT_ERR_INVALID_ARG; }
    if (u->size < sizeof(spt_scene_update_desc)) { g_error = "scene_deform: size is smaller than spt_scene_update_desc"; return SPT_ERR_INVALID_ARG; }
    if (sc->fwd) {
        if (!sc->fwd->scene_deform) { g_error = "scene_deform: libspt_hip_bez.so does not export spt_scene_deform"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->scene_deform(sc->inner, u, n_meshes, meshes));
    }
    std::lock_guard<std::mutex> lock(sc->mu);
    return update_locked(sc, u, n_meshes, meshes, "scene_deform");
}

spt_status spt_scene_origin_candidates(const spt_scene* scene_c, uint64_t* words_out, uint32_t* n_rows_out, double* info_out) {
    if (!scene_c || !n_rows_out) { g_error = "scene_origin_candidates: null argument"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    *n_rows_out = 0u;
    if (sc->fwd) return SPT_OK;   // a scene with Bezier patches never qualifies
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("scene_origin_candidates", [&] {
        if (!sc->origin_ok || std::getenv("SPT_NO_ORIGIN_CANDIDATES") != nullptr) return SPT_OK;
        const spt_oc_info& in = sc->origin_info;
        if (words_out) {   // the device's copy, behind every update queued so far
            HIP_CHECK(hipSetDevice(sc->device));
            HIP_CHECK(hipStreamSynchronize(sc->stream));
            HIP_CHECK(hipMemcpy(words_out, sc->origin_cand.p, (size_t)SPT_OC_WORDS * in.n_rows * sizeof(uint64_t), hipMemcpyDeviceToHost));
        }
        if (info_out) {
            const double out[8] = {in.center[0], in.center[1], in.center[2], in.radius, in.reach, in.delta, (double)in.tight, (double)sc->origin_build_ns};
            std::memcpy(info_out, out, sizeof out);
        }
        *n_rows_out = in.n_rows;
        return SPT_OK;
    });
}

// What spt_render_camera and spt_film_create_camera check of a non-perspective model and its plan before anything else happens; SPT_OK:
// the call may go on
static spt_status check_camera_model(const spt_camera_model* model, const spt_render_params* params, const char* who) {
    if (const char* why = spt_cm_check(model)) { g_error = std::string(who) + ": " + why; return SPT_ERR_INVALID_ARG; }
    if (params && (params->flags & SPT_RENDER_COUNT_VISITS)) { g_error = std::string(who) + ": a camera model does not count visits (SPT_RENDER_COUNT_VISITS)"; return SPT_ERR_UNSUPPORTED; }
    if (params && (params->flags & SPT_RENDER_AOV_ALBEDO)) { g_error = std::string(who) + ": SPT_RENDER_AOV_ALBEDO is not served for a camera model (the albedo kernels read the pinhole's compact records)"; return SPT_ERR_UNSUPPORTED; }
    return SPT_OK;
}

static spt_status render_impl(const spt_scene* scene_c, const spt_camera* cam, const spt_camera_model* model, const spt_render_params* params,
                              float* rgb_mean_out, spt_render_stats* stats);

spt_status spt_render(const spt_scene* scene_c, const spt_camera* cam, const spt_render_params* params,
                      float* rgb_mean_out, spt_render_stats* stats) {
    return render_impl(scene_c, cam, nullptr, params, rgb_mean_out, stats);
}

spt_status spt_render_camera(const spt_scene* scene_c, const spt_camera_model* model, const spt_render_params* params, float* rgb_mean_out,
                             spt_render_stats* stats) {
    if (!scene_c || !model || !params || !rgb_mean_out) { g_error = "render_camera: null argument"; return SPT_ERR_INVALID_ARG; }
    if (model->size >= sizeof(spt_camera_model) && model->type == SPT_CAMERA_PERSPECTIVE) return spt_render(scene_c, &model->base, params, rgb_mean_out, stats);
    const spt_status st = check_camera_model(model, params, "render_camera");
    if (st != SPT_OK) return st;
    return render_impl(scene_c, &model->base, model, params, rgb_mean_out, stats);
}

// model: a checked non-perspective camera model with cam == &model->base, or null
static spt_status render_impl(const spt_scene* scene_c, const spt_camera* cam, const spt_camera_model* model, const spt_render_params* params,
                              float* rgb_mean_out, spt_render_stats* stats) {
    if (!scene_c || !cam || !params || !rgb_mean_out) { g_error = "render: null argument"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {
        if (model == nullptr) return forwarded(sc->fwd, sc->fwd->render(sc->inner, cam, params, rgb_mean_out, stats));
        if (!sc->fwd->render_camera) { g_error = "render_camera: libspt_hip_bez.so does not export spt_render_camera"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->render_camera(sc->inner, model, params, rgb_mean_out, stats));
    }
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("render", [&] {
        const spt_render_params& p = *params;
        check_plan(p, "render");
        const uint32_t shard_count = p.shard_count ? p.shard_count : 1u, strip_rows = p.strip_rows ? p.strip_rows : 1u;
        const uint32_t own_rows = shard_row_count(p);
        const uint64_t own_pix64 = (uint64_t)own_rows * p.width;
        const bool async_out = (p.flags & SPT_RENDER_ASYNC) != 0;
        if (async_out && (stats || (p.flags & (SPT_RENDER_PROFILE | SPT_RENDER_COUNT_VISITS))))
            fail(SPT_ERR_INVALID_ARG, "render: SPT_RENDER_ASYNC returns no stats (stats must be NULL, no PROFILE / COUNT_VISITS)");
        // `stats` belongs to a caller that may have been compiled against an older (shorter) spt_render_stats: fill a
        // local copy and hand back only the bytes the caller says it has (spt_render_params::stats_size, ABI v9)
        spt_render_stats* const stats_out = stats;
        spt_render_stats stats_local;
        std::memset(&stats_local, 0, sizeof stats_local);
        size_t stats_bytes = 0;
        if (stats_out) {
            if (p.stats_size < 8u) fail(SPT_ERR_INVALID_ARG, "render: stats given but params.stats_size is not set (caller built against ABI < 9?)");
            stats_bytes = std::min<size_t>(p.stats_size, sizeof stats_local);
            std::memset(stats_out, 0, stats_bytes);
            stats = &stats_local;
        }
        struct StatsCopy {   // copies on every exit path that got this far, error paths included
            spt_render_stats* dst; const spt_render_stats* src; size_t n;
            ~StatsCopy() { if (dst) std::memcpy(dst, src, n); }
        } stats_copy{stats_out, &stats_local, stats_bytes};
        if (own_pix64 == 0) return SPT_OK;
        if (own_pix64 > 0x7fffffffull) fail(SPT_ERR_UNSUPPORTED, "render: shard larger than 2^31 pixels");
        const uint32_t own_pix = (uint32_t)own_pix64;
        const float radius = plan_radius(p, "render");
        const int32_t R = (int32_t)std::ceil(radius - 0.5f);
        HIP_CHECK(hipSetDevice(sc->device));
        grow(sc, sc->out, (size_t)own_pix * 3 * sizeof(float));
        const size_t strip_bytes = (size_t)strip_rows * p.width * 3 * sizeof(float);
        if (p.out_strip_stride != 0 && p.out_strip_stride < strip_bytes) fail(SPT_ERR_INVALID_ARG, "render: out_strip_stride smaller than a strip");

        RenderRun run;
        run.sc = sc;
        run.cam = cam;
        run.model = model;
        run.params = &p;
        run.stats = stats;
        run_setup(run);
        // an asynchronous frame without a wide box filter takes the overlapped schedule (trace_window); every other render
        // starts behind whatever such a frame left on the film stream
        run.film_overlap = async_out && R <= 0 && run.film_stream;
        run.pipe_plan = R <= 0 && run.film_stream && run.pass_pipeline && run.fused && !run.albedo;
        if (!run.film_overlap) film_join(sc);
        hipEvent_t ev_total0 = run.get_event(), ev_total1 = run.get_event();
        HIP_CHECK(hipEventRecord(ev_total0, run.st));
        run_spans(run);
        // radius 0.5 into pinned memory on the overlapped schedule: the finish kernel stores the image into the caller's buffer itself
        // (k_finish_host).  Overlapped frames only: the kernel is slow by design (few workgroups, film_kernels.h) and belongs on the
        // film stream beside the next frame, not on the critical path of a synchronous or single-stream render
        OutLayout direct_lay{};
        float* const direct_dst = radius == 0.5f && run.direct_out && run.film_overlap ? direct_destination(p, own_rows, strip_rows, rgb_mean_out, &direct_lay) : nullptr;
        const SampleTarget whole{0u, p.spp, nullptr, nullptr, true};   // every sample of the plan, into the scene's film from zero
        if (R <= 0) {
            const RenderCtx rc = trace_window(run, 0, own_rows, p.shard_index, shard_count, strip_rows, false, whole);
            run.begin(SPT_K_RESOLVE);
            const dim3 grid((own_pix + kBlock - 1) / kBlock);
            // overlapped (trace_window may have fallen back): behind the last resolve and the previous frame's copy-out by the
            // film stream's order.  Else the previous frame's copy-out, which reads `out`, is waited for
            const hipStream_t st_fin = run.film_overlap ? sc->stream_film : run.st;
            if (!run.film_overlap && sc->copy_pending) HIP_CHECK(hipStreamWaitEvent(run.st, sc->ev_copy_done, 0));
            if (radius == 0.5f && direct_dst) {
                const uint64_t blocks = (out_layout_items(direct_lay) + kBlock - 1) / kBlock;
                hipLaunchKernelGGL(k_finish_host, dim3((uint32_t)std::min<uint64_t>(blocks, run.direct_grid)), dim3(kBlock), 0, st_fin, rc, direct_lay, direct_dst);
            } else if (radius == 0.5f) hipLaunchKernelGGL(k_finish, dim3((own_pix * 3 + kBlock - 1) / kBlock), dim3(kBlock), 0, st_fin, rc, sc->out.as<float>());
            else hipLaunchKernelGGL(k_finish_box, grid, dim3(kBlock), 0, st_fin, rc, sc->out.as<float>(), radius, R, 0u, p.spp);
            run.end();
        } else {
            // Film::filter_pixel (film.rs:71-92) reads the samples of (2R+1)^2 pixels: each run of consecutive rows of
            // this shard is rendered as bands of whole rows with R rows of halo, all samples kept, then filtered.
            // The halo rows are traced again by the neighbouring band / rank: samples are a pure function of
            // (seed, pixel, sample), so every copy of a row is the same bits.
            std::vector<uint32_t> own;
            for (uint32_t j = 0; j < p.height; ++j)
                if ((j / strip_rows) % shard_count == p.shard_index) own.push_back(j);
            const uint64_t per_row = (uint64_t)p.width * p.spp * 3 * sizeof(float);
            const uint64_t fit = std::max<uint64_t>(1, run.box_band_bytes / per_row);
            const uint32_t run_max = (uint32_t)std::min<uint64_t>(p.height, fit > 2ull * (uint64_t)R ? fit - 2ull * (uint64_t)R : 1ull);
            for (size_t k = 0; k < own.size();) {
                size_t e = k + 1;
                while (e < own.size() && own[e] == own[e - 1] + 1u && e - k < run_max) ++e;
                const uint32_t j0 = own[k], j1 = own[e - 1] + 1u;
                const uint32_t b0 = j0 >= (uint32_t)R ? j0 - (uint32_t)R : 0u, b1 = (uint32_t)std::min<uint64_t>(p.height, (uint64_t)j1 + (uint64_t)R);
                const RenderCtx rc = trace_window(run, b0, b1 - b0, 0u, 1u, 1u, true, whole);
                run.begin(SPT_K_RESOLVE);
                BoxJob job{sc->rad[0].as<float>(), b0, b1 - b0, j0, j1 - j0, sc->out.as<float>() + k * (size_t)p.width * 3, R, radius};
                if (sc->copy_pending) HIP_CHECK(hipStreamWaitEvent(run.st, sc->ev_copy_done, 0));
                hipLaunchKernelGGL(k_filter_box, dim3(((j1 - j0) * p.width + kBlock - 1) / kBlock), dim3(kBlock), 0, run.st, rc, job);
                run.end();
                k = e;
            }
        }
        HIP_CHECK(hipGetLastError());
        hipStream_t st_out = run.st;
        if (async_out) {   // the copy-out leaves the compute stream: the next render's kernels run beside it
            if (!run.film_overlap) {   // (overlapped: the copy follows the finish kernel on the film stream)
                HIP_CHECK(hipEventRecord(sc->ev_out_ready, run.st));
                HIP_CHECK(hipStreamWaitEvent(sc->stream_film, sc->ev_out_ready, 0));
            }
            st_out = sc->stream_film;
        }
        if (direct_dst) {
            ++sc->frames_direct;   // the image is where it belongs: the events below make it visible to the host
        } else {
            const size_t row_bytes = (size_t)p.width * 3 * sizeof(float);
            const bool packed = p.out_strip_stride == 0 || p.out_strip_stride == strip_bytes;
            // strided copy-out: the shard's strips land strip by strip in a larger (full-image) film
            const size_t full = own_rows / strip_rows, rest_rows = own_rows - full * strip_rows;
            hipError_t e = hipSuccess;
            if (packed) e = hipMemcpyAsync(rgb_mean_out, sc->out.p, (size_t)own_pix * 3 * sizeof(float), hipMemcpyDeviceToHost, st_out);
            else {
                if (full) e = hipMemcpy2DAsync(rgb_mean_out, p.out_strip_stride, sc->out.p, strip_bytes, strip_bytes, full, hipMemcpyDeviceToHost, st_out);
                if (e == hipSuccess && rest_rows)
                    e = hipMemcpyAsync((char*)rgb_mean_out + full * p.out_strip_stride, (const char*)sc->out.p + full * strip_bytes, rest_rows * row_bytes,
                                       hipMemcpyDeviceToHost, st_out);
            }
            if (e == hipErrorInvalidValue) {
                // the runtime refuses a destination that is page-locked only in part (a film that straddles the end of a pinned
                // region): through a pageable buffer of the library's own, synchronously - the film is complete when this returns
                (void)hipGetLastError();
                std::vector<float> staged((size_t)own_pix * 3);
                HIP_CHECK(hipStreamSynchronize(st_out));
                HIP_CHECK(hipMemcpy(staged.data(), sc->out.p, staged.size() * sizeof(float), hipMemcpyDeviceToHost));
                const size_t stride = packed ? strip_bytes : (size_t)p.out_strip_stride;
                for (uint32_t r = 0; r < own_rows; ++r)
                    std::memcpy((char*)rgb_mean_out + (r / strip_rows) * stride + (r % strip_rows) * row_bytes, staged.data() + (size_t)r * p.width * 3, row_bytes);
            } else HIP_CHECK(e);
        }
        if (async_out) {
            HIP_CHECK(hipEventRecord(sc->ev_copy_done, sc->stream_film));
            sc->copy_pending = true;
            return SPT_OK;
        }
        unsigned long long h_visits[12] = {};
        if (run.count) HIP_CHECK(hipMemcpyAsync(h_visits, sc->visits.p, sizeof h_visits, hipMemcpyDeviceToHost, run.st));
        HIP_CHECK(hipEventRecord(ev_total1, run.st));
        HIP_CHECK(hipStreamSynchronize(run.st));
        sc->copy_pending = sc->film_inflight = false;   // (the finish kernels of this render waited for any copy-out still in flight, film_join for the film stream)
        if (stats) {
            for (int c = 0; c < 3; ++c)
                for (int k = 0; k < 3; ++k) stats->class_visits[c][k] = h_visits[3 * c + k];
            stats->node_visits = h_visits[0] + h_visits[3] + h_visits[6];
            stats->tri_tests = h_visits[1] + h_visits[4] + h_visits[7];
            stats->instance_visits = h_visits[2] + h_visits[5] + h_visits[8];
            stats->node_bytes = stats->node_visits * 64ull;   // wide 2-ary and compressed 4-ary nodes are both 64-byte records
            stats->samples = run.samples_traced;
            stats->segments_closest = run.seg_closest;
            stats->segments_shadow = run.seg_shadow;
            stats->primary_hits = run.primary_hits;
            stats->path_vertices = run.path_vertices;
            stats->shadow_first = run.shadow_first;
            stats->vertices_second = run.vertices_second;
            stats->live_samples = run.live_samples;
            float ms = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&ms, ev_total0, ev_total1));
            stats->gpu_ms = ms;
            for (auto& sp : run.spans) {
                float k = 0.0f;
                HIP_CHECK(hipEventElapsedTime(&k, sc->events[sp.e0], sc->events[sp.e0 + 1]));
                stats->kernel_ms[sp.cls] += k;
                stats->kernel_launches[sp.cls] += 1;
                if (run.debug_spans) std::fprintf(stderr, "[spt] span class %d: %.3f ms\n", sp.cls, k);
            }
        }
        return SPT_OK;
    });
}

spt_status spt_render_wait(const spt_scene* scene_c) {
    if (!scene_c) { g_error = "render_wait: null argument"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) return forwarded(sc->fwd, sc->fwd->render_wait(sc->inner));
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("render_wait", [&] {
        HIP_CHECK(hipSetDevice(sc->device));
        HIP_CHECK(hipStreamSynchronize(sc->stream));
        HIP_CHECK(hipStreamSynchronize(sc->stream2));
        HIP_CHECK(hipStreamSynchronize(sc->stream_film));
        sc->copy_pending = sc->film_pending = sc->film_inflight = sc->shade_pending = false;
        sc->film_recorded[0] = sc->film_recorded[1] = false;
        sc->tail_set = -1;
        return SPT_OK;
    });
}

static spt_status film_create_impl(const spt_scene* scene_c, const spt_camera* cam, const spt_camera_model* model, const spt_render_params* params,
                                   uint32_t first_sample, uint32_t film_flags, spt_film** out);

spt_status spt_film_create(const spt_scene* scene_c, const spt_camera* cam, const spt_render_params* params, uint32_t first_sample,
                           uint32_t film_flags, spt_film** out) {
    return film_create_impl(scene_c, cam, nullptr, params, first_sample, film_flags, out);
}

spt_status spt_film_create_camera(const spt_scene* scene_c, const spt_camera_model* model, const spt_render_params* params, uint32_t first_sample,
                                  uint32_t film_flags, spt_film** out) {
    if (!scene_c || !model || !params || !out) { g_error = "film_create_camera: null argument"; return SPT_ERR_INVALID_ARG; }
    if (model->size >= sizeof(spt_camera_model) && model->type == SPT_CAMERA_PERSPECTIVE) return spt_film_create(scene_c, &model->base, params, first_sample, film_flags, out);
    *out = nullptr;
    const spt_status st = check_camera_model(model, params, "film_create_camera");
    if (st != SPT_OK) return st;
    return film_create_impl(scene_c, &model->base, model, params, first_sample, film_flags, out);
}

// model: as render_impl's
static spt_status film_create_impl(const spt_scene* scene_c, const spt_camera* cam, const spt_camera_model* model, const spt_render_params* params,
                                   uint32_t first_sample, uint32_t film_flags, spt_film** out) {
    if (!scene_c || !cam || !params || !out) { g_error = "film_create: null argument"; return SPT_ERR_INVALID_ARG; }
    *out = nullptr;
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {
        spt_film* inner = nullptr;
        if (model != nullptr && !sc->fwd->film_create_camera) { g_error = "film_create_camera: libspt_hip_bez.so does not export spt_film_create_camera"; return SPT_ERR_UNSUPPORTED; }
        const spt_status st = forwarded(sc->fwd, model != nullptr ? sc->fwd->film_create_camera(sc->inner, model, params, first_sample, film_flags, &inner)
                                                                  : sc->fwd->film_create(sc->inner, cam, params, first_sample, film_flags, &inner));
        if (st != SPT_OK) return st;
        spt_film* f = new (std::nothrow) spt_film;
        if (!f) { sc->fwd->film_destroy(inner); g_error = "film_create: out of host memory"; return SPT_ERR_OUT_OF_MEMORY; }
        f->fwd = sc->fwd;
        f->inner = inner;
        *out = f;
        return SPT_OK;
    }
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("film_create", [&] {
        const spt_render_params& p = *params;
        check_plan(p, "film_create");
        if (film_flags & ~(uint32_t)(SPT_FILM_MOMENTS | SPT_FILM_KEEP_SAMPLES)) fail(SPT_ERR_INVALID_ARG, "film_create: unknown film flags");
        const bool keep = (film_flags & SPT_FILM_KEEP_SAMPLES) != 0;
        if (keep && (film_flags & SPT_FILM_MOMENTS))
            fail(SPT_ERR_INVALID_ARG, "film_create: SPT_FILM_KEEP_SAMPLES and SPT_FILM_MOMENTS exclude each other (the moments assume every sample of a pixel weighs 1)");
        if (first_sample > p.spp) fail(SPT_ERR_INVALID_ARG, "film_create: first_sample past the plan's spp");
        const float radius = plan_radius(p, "film_create");
        const int32_t R = (int32_t)std::ceil(radius - 0.5f);
        // Film::filter_pixel of a wider box adds the samples of the neighbouring pixels into ONE running sum, pixel after pixel:
        // the sum after n samples is not a prefix of the sum after n + k, so it cannot be extended bit-exactly.  (A film that keeps
        // its samples can: SPT_FILM_KEEP_SAMPLES)
        if (R >= 1 && !keep) fail(SPT_ERR_UNSUPPORTED, "film_create: a box filter reaching neighbouring pixels (ceil(radius - 0.5) >= 1) cannot be rendered in increments");
        const uint64_t own_pix64 = (uint64_t)shard_row_count(p) * p.width;
        if (own_pix64 > 0x7fffffffull) fail(SPT_ERR_UNSUPPORTED, "film_create: shard larger than 2^31 pixels");
        HIP_CHECK(hipSetDevice(sc->device));
        auto f = std::make_unique<spt_film>();
        f->sc = sc;
        f->cam = *cam;
        if (model != nullptr) { f->model = *model; f->model.size = (uint32_t)sizeof(spt_camera_model); }
        f->plan = p;
        f->first = first_sample;
        f->flags = film_flags;
        f->rows = shard_row_count(p);
        f->radius = radius;
        f->R = R;
        if (keep) {
            make_kept_runs(f.get());
            *out = f.release();
            ++sc->live_films;
            return SPT_OK;
        }
        const size_t bytes = (size_t)own_pix64 * 3 * sizeof(float);
        f->sum.alloc(bytes);
        HIP_CHECK(hipMemsetAsync(f->sum.p, 0, f->sum.bytes, sc->stream));
        if (film_flags & SPT_FILM_MOMENTS) {
            f->sq.alloc(bytes);
            HIP_CHECK(hipMemsetAsync(f->sq.p, 0, f->sq.bytes, sc->stream));
        }
        HIP_CHECK(hipStreamSynchronize(sc->stream));
        *out = f.release();
        ++sc->live_films;
        return SPT_OK;
    });
}

spt_status spt_film_render(spt_film* f, uint32_t n_samples) {
    if (!f) { g_error = "film_render: null argument"; return SPT_ERR_INVALID_ARG; }
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_render(f->inner, n_samples));
    if (n_samples == 0) return SPT_OK;
    spt_scene* sc = f->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("film_render", [&] {
        const spt_render_params& p = f->plan;
        // every check comes before the first change: a refused call leaves the film as it was
        if (p.flags & (SPT_RENDER_ASYNC | SPT_RENDER_PROFILE | SPT_RENDER_COUNT_VISITS))
            fail(SPT_ERR_INVALID_ARG, "film_render: the plan asks for SPT_RENDER_ASYNC / PROFILE / COUNT_VISITS (increments are synchronous and return no stats)");
        const uint32_t shard_count = p.shard_count ? p.shard_count : 1u, strip_rows = p.strip_rows ? p.strip_rows : 1u;
        const size_t strip_bytes = (size_t)strip_rows * p.width * 3 * sizeof(float);
        if (p.out_strip_stride != 0 && p.out_strip_stride != strip_bytes) fail(SPT_ERR_INVALID_ARG, "film_render: the plan's out_strip_stride is not packed (films read out packed rows)");
        if ((uint64_t)f->first + f->done + n_samples > p.spp)
            fail(SPT_ERR_INVALID_ARG, "film_render: " + std::to_string(n_samples) + " more samples would pass the plan's spp (" + std::to_string(p.spp) + ", " +
                                          std::to_string(f->first + f->done) + " covered)");
        // (an adaptive film without active pixels traces nothing: `done` still advances, every pixel keeps its n_p)
        if (f->rows != 0 && !(f->adaptive && f->active == 0)) {
            HIP_CHECK(hipSetDevice(sc->device));
            film_join(sc);
            RenderRun run;
            run.sc = sc;
            run.cam = &f->cam;
            run.model = f->model.type != SPT_CAMERA_PERSPECTIVE ? &f->model : nullptr;
            run.params = &p;
            run_setup(run);
            run_spans(run);
            if (f->flags & SPT_FILM_KEEP_SAMPLES) {
                kept_render(f, run, n_samples);
                f->done += n_samples;
                return SPT_OK;
            }
            SampleTarget inc{f->first + f->done, n_samples, f->sum.as<float>(), (f->flags & SPT_FILM_MOMENTS) ? f->sq.as<float>() : nullptr, false};
            if (f->adaptive) {
                inc.mask = FilmMask{f->mask.as<uint8_t>(), f->tile_active.as<uint32_t>()};
                inc.mask_tiles = f->active_tiles;
            }
            if (f->n_buckets != 0u) {
                inc.buckets = f->buckets.as<float>();
                inc.n_buckets = f->n_buckets;
                inc.bucket_plane = (size_t)f->rows * p.width * 3;
            }
            (void)trace_window(run, 0, f->rows, p.shard_index, shard_count, strip_rows, false, inc);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(run.st));
        }
        f->done += n_samples;
        return SPT_OK;
    });
}

spt_status spt_film_samples(const spt_film* f, uint32_t* done) {
    if (!f || !done) { g_error = "film_samples: null argument"; return SPT_ERR_INVALID_ARG; }
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_samples(f->inner, done));
    *done = f->done;
    return SPT_OK;
}

// Where a film read-out goes: the floats as they are (f32), or - spt_film_read_rgb8 - their bytes (u8).  Exactly one is set.
struct FilmReadOut {
    float* f32;
    uint8_t* u8;
};

// The end of every read-out: n_floats floats at `src` on the device (the staging buffer f->out for everything but the raw sums)
// go to the host as they are, or through k_pack_rgb8 and the film's byte buffer.  Synchronous.
// (`out8`: the byte buffer of whoever owns `src` - a film's, or the scene's for spt_denoise_image.)
static void deliver(DeviceBuffer& out8, const void* src, size_t n_floats, const FilmReadOut& to, hipStream_t st) {
    if (to.u8) {
        if (n_floats > 0xfffffffcull) fail(SPT_ERR_UNSUPPORTED, "film_read_rgb8: shard larger than 2^32 - 4 bytes");
        out8.ensure(n_floats);
        launch_pack_rgb8((uint32_t)n_floats, static_cast<const float*>(src), out8.as<uint8_t>(), st);
        HIP_CHECK(hipMemcpyAsync(to.u8, out8.p, n_floats, hipMemcpyDeviceToHost, st));
    } else {
        HIP_CHECK(hipMemcpyAsync(to.f32, src, n_floats * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
}
static void film_deliver(spt_film* f, const void* src, size_t n_floats, const FilmReadOut& to, hipStream_t st) { deliver(f->out8, src, n_floats, to, st); }

// spt_film_read behind its argument checks (the scene's lock is held)
static spt_status film_read_locked(spt_film* f, uint32_t what, const FilmReadOut& to) {
    spt_scene* sc = f->sc;
    const spt_render_params& p = f->plan;
    if (what > SPT_FILM_VAR_OF_MEAN) fail(SPT_ERR_INVALID_ARG, "film_read: unknown SPT_FILM_* value");
    const bool moments = (f->flags & SPT_FILM_MOMENTS) != 0;
    if ((what == SPT_FILM_SUM_SQ || what == SPT_FILM_VAR_OF_MEAN) && !moments)
        fail(SPT_ERR_INVALID_ARG, "film_read: SUM_SQ / VAR_OF_MEAN need a film created with SPT_FILM_MOMENTS");
    if (what == SPT_FILM_VAR_OF_MEAN && f->radius != 0.5f)
        fail(SPT_ERR_UNSUPPORTED, "film_read: VAR_OF_MEAN needs the box radius 0.5 (every sample of the pixel weighs 1)");
    if ((what == SPT_FILM_MEAN || what == SPT_FILM_VAR_OF_MEAN) && f->done == 0) fail(SPT_ERR_INVALID_ARG, "film_read: the film covers no samples yet");
    if (f->rows == 0) return SPT_OK;
    const uint32_t n_pix = f->rows * p.width;
    const size_t bytes = (size_t)n_pix * 3 * sizeof(float);
    HIP_CHECK(hipSetDevice(sc->device));
    film_join(sc);
    const hipStream_t st = sc->stream;
    if (f->flags & SPT_FILM_KEEP_SAMPLES) {   // (SUM_SQ / VAR_OF_MEAN were refused above: such a film has no moments)
        // Film::filter_pixel over the kept samples, run by run: SUM is the colour, MEAN the colour * (1 / weight_sum)
        f->out.ensure(bytes);
        HIP_CHECK(hipEventRecord(sc->ev_keep[0], st));
        for (const auto& r : f->runs) {
            const RenderCtx rc = plan_ctx(p, f->cam, r.b0, r.b1 - r.b0, 0u, 1u, 1u);
            const KeptJob job = kept_job(f, r, f->out.as<float>() + r.out_row * (size_t)p.width * 3, what == SPT_FILM_MEAN);
            const dim3 grid(((r.j1 - r.j0) * p.width + kBlock - 1) / kBlock);
            if (f->filter_type != SPT_FILTER_BOX) {
                launch_filter_weighted(f, grid, st, rc, job);
                continue;
            }
            // samples requested together per lane: 8 up to R = 1, 1 from R = 2 on (measured, see k_film_filter_box)
            hipLaunchKernelGGL(f->R >= 2 ? k_film_filter_box<1u> : k_film_filter_box<8u>, grid, dim3(kBlock), 0, st, rc, job);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(sc->ev_keep[1], st));
        film_deliver(f, f->out.p, (size_t)n_pix * 3, to, st);
        sc->keep_read_ns = keep_elapsed_ns(sc);
        return SPT_OK;
    }
    const void* src = f->sum.p;
    if (what == SPT_FILM_SUM_SQ) src = f->sq.p;
    if (what == SPT_FILM_MEAN || what == SPT_FILM_VAR_OF_MEAN) {
        f->out.ensure(bytes);
        if (what == SPT_FILM_MEAN && f->radius != 0.5f) {
            // k_finish_box over the covered samples: the context it reads is the plan's sampler and shard
            RenderCtx rc = plan_ctx(p, f->cam, 0, f->rows, p.shard_index, p.shard_count ? p.shard_count : 1u, p.strip_rows ? p.strip_rows : 1u);
            rc.film = f->sum.as<float>();
            hipLaunchKernelGGL(k_finish_box, dim3((n_pix + kBlock - 1) / kBlock), dim3(kBlock), 0, st, rc, f->out.as<float>(), f->radius, f->R, f->first, f->done);
        } else if (f->adaptive) {   // radius 0.5 (spt_film_adapt refuses others): per-pixel sample counts
            hipLaunchKernelGGL(k_film_read_counts, dim3((n_pix * 3 + kBlock - 1) / kBlock), dim3(kBlock), 0, st, what, n_pix * 3u, f->sum.as<float>(),
                               f->sq.as<float>(), f->mask.as<uint8_t>(), f->counts.as<uint32_t>(), f->done, f->inv.as<float>(), f->out.as<float>());
        } else {
            const float inv_n = 1.0f / (float)f->done, inv_n1 = f->done > 1u ? 1.0f / (float)(f->done - 1u) : 0.0f;
            hipLaunchKernelGGL(k_film_read, dim3((n_pix * 3 + kBlock - 1) / kBlock), dim3(kBlock), 0, st, what, n_pix * 3u, f->sum.as<float>(),
                               moments ? f->sq.as<float>() : nullptr, f->done, inv_n, inv_n1, f->out.as<float>());
        }
        HIP_CHECK(hipGetLastError());
        src = f->out.p;
    }
    film_deliver(f, src, (size_t)n_pix * 3, to, st);
    return SPT_OK;
}

spt_status spt_film_read(spt_film* f, uint32_t what, float* out) {
    if (!f || !out) { g_error = "film_read: null argument"; return SPT_ERR_INVALID_ARG; }
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_read(f->inner, what, out));
    std::lock_guard<std::mutex> lock(f->sc->mu);
    return guarded("film_read", [&] { return film_read_locked(f, what, FilmReadOut{out, nullptr}); });
}

spt_status spt_film_adapt(spt_film* f, float rel_error, float abs_floor, uint32_t min_samples, uint32_t* active_out) {
    if (!f) { g_error = "film_adapt: null argument"; return SPT_ERR_INVALID_ARG; }
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_adapt(f->inner, rel_error, abs_floor, min_samples, active_out));
    spt_scene* sc = f->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("film_adapt", [&] {
        const spt_render_params& p = f->plan;
        // every check comes before the first change: a refused call leaves the film as it was
        if (!(f->flags & SPT_FILM_MOMENTS)) fail(SPT_ERR_INVALID_ARG, "film_adapt: the film was created without SPT_FILM_MOMENTS (the criterion needs the sums of squares)");
        if (f->radius != 0.5f) fail(SPT_ERR_UNSUPPORTED, "film_adapt: needs the box radius 0.5 (every sample of the pixel weighs 1)");
        if (!std::isfinite(rel_error) || !std::isfinite(abs_floor) || rel_error < 0.0f || abs_floor < 0.0f)
            fail(SPT_ERR_INVALID_ARG, "film_adapt: rel_error and abs_floor must be finite and >= 0");
        const uint32_t n_pix = f->rows * p.width;
        const uint32_t need = std::max(min_samples, 2u);
        if (f->done < need || n_pix == 0 || (f->adaptive && f->active == 0)) {   // nothing to retire: the active set as it stands
            if (active_out) *active_out = f->adaptive ? f->active : n_pix;
            return SPT_OK;
        }
        HIP_CHECK(hipSetDevice(sc->device));
        film_join(sc);
        const hipStream_t st = sc->stream;
        const uint32_t tiles_x = (p.width + kTile - 1) / kTile, n_tiles = tiles_x * ((f->rows + kTile - 1) / kTile);
        if (!f->adaptive) {   // every pixel active, every tile busy; the reciprocal table of the plan's sample counts
            f->mask.alloc(n_pix);
            f->counts.alloc((size_t)n_pix * sizeof(uint32_t));
            f->tile_active.alloc((size_t)n_tiles * sizeof(uint32_t));
            f->totals.alloc(2 * sizeof(uint32_t));
            f->inv.alloc(((size_t)p.spp + 1) * sizeof(float));
            std::vector<float> inv((size_t)p.spp + 1, 0.0f);
            for (uint32_t k = 1; k <= p.spp; ++k) inv[k] = 1.0f / (float)k;
            HIP_CHECK(hipMemsetAsync(f->mask.p, 1, n_pix, st));
            HIP_CHECK(hipMemsetAsync(f->counts.p, 0, f->counts.bytes, st));
            HIP_CHECK(hipMemcpyAsync(f->inv.p, inv.data(), f->inv.bytes, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));   // `inv` is pageable
            f->adaptive = true;
            f->active = n_pix;
            f->active_tiles = n_tiles;
        }
        uint32_t totals[2] = {0u, 0u};
        HIP_CHECK(hipMemsetAsync(f->totals.p, 0, 2 * sizeof(uint32_t), st));
        const float inv_n = 1.0f / (float)f->done, inv_n1 = 1.0f / (float)(f->done - 1u);
        hipLaunchKernelGGL(k_film_adapt, dim3(n_tiles), dim3(kBlock), 0, st, p.width, f->rows, tiles_x, f->sum.as<float>(), f->sq.as<float>(),
                           f->mask.as<uint8_t>(), f->counts.as<uint32_t>(), f->tile_active.as<uint32_t>(), f->totals.as<uint32_t>(), f->done, inv_n,
                           inv_n1, rel_error, abs_floor);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(totals, f->totals.p, sizeof totals, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        f->active = totals[0];
        f->active_tiles = totals[1];
        if (active_out) *active_out = f->active;
        return SPT_OK;
    });
}

spt_status spt_film_read_counts(spt_film* f, uint32_t* out) {
    if (!f || !out) { g_error = "film_read_counts: null argument"; return SPT_ERR_INVALID_ARG; }
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_read_counts(f->inner, out));
    spt_scene* sc = f->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("film_read_counts", [&] {
        const uint32_t n_pix = f->rows * f->plan.width;
        if (!f->adaptive) {
            std::fill(out, out + n_pix, f->done);
            return SPT_OK;
        }
        std::vector<uint8_t> mask(n_pix);
        HIP_CHECK(hipSetDevice(sc->device));
        film_join(sc);
        HIP_CHECK(hipMemcpyAsync(mask.data(), f->mask.p, n_pix, hipMemcpyDeviceToHost, sc->stream));
        HIP_CHECK(hipMemcpyAsync(out, f->counts.p, (size_t)n_pix * sizeof(uint32_t), hipMemcpyDeviceToHost, sc->stream));
        HIP_CHECK(hipStreamSynchronize(sc->stream));
        for (uint32_t i = 0; i < n_pix; ++i)
            if (mask[i]) out[i] = f->done;
        return SPT_OK;
    });
}

// What k_denoise_pack reads of a film that covers at least 2 samples.
static DenoiseFilm denoise_input(const spt_film* f) {
    DenoiseFilm in{};
    in.sum = f->sum.as<float>();
    in.sum_sq = f->sq.as<float>();
    in.done = f->done;
    in.inv_n = 1.0f / (float)f->done;
    in.inv_n1 = 1.0f / (float)(f->done - 1u);
    if (f->adaptive) {
        in.mask = f->mask.as<uint8_t>();
        in.counts = f->counts.as<uint32_t>();
        in.inv = f->inv.as<float>();
    }
    return in;
}

// A film and its guide have to live in the same library (both handles are passed through, or neither).
static bool denoise_libraries_differ(const spt_film* f, const spt_film* guide) {
    if ((f->fwd != nullptr) == (guide ? guide->fwd != nullptr : f->fwd != nullptr)) return false;
    g_error = "film_denoise: the film and the guide are served by different libraries (one scene has Bezier patches)";
    return true;
}

// The albedo film of a spt_film_denoise_job and what the job says about it (null film: spt_film_denoise)
struct DenoiseAlbedoJob {
    spt_film* film = nullptr;
    float k_albedo = 1.0f, eps_albedo = 1e-2f, eps_demod = 1e-2f;
    bool demodulate = false;
};

// The params, k_* and eps_* checks of spt_film_denoise_job (and spt_denoise_image); the parameters with the defaults filled in.
static spt_denoise_params denoise_params_checked(const spt_denoise_params* params, const DenoiseAlbedoJob& aj) {
    for (const float v : {aj.k_albedo, aj.eps_albedo, aj.eps_demod})   // (with or without an albedo film, as k_guide without a guide)
        if (!std::isfinite(v) || !(v > 0.0f)) fail(SPT_ERR_INVALID_ARG, "film_denoise_job: k_albedo, eps_albedo and eps_demod must be finite and > 0");
    spt_denoise_params dp{(uint32_t)sizeof(spt_denoise_params), 5u, 2.0f, 1.0f, 1e-8f, 1e-2f};
    if (params) {
        if (params->size < sizeof(spt_denoise_params)) fail(SPT_ERR_INVALID_ARG, "film_denoise: params->size is smaller than spt_denoise_params");
        dp = *params;
    }
    if (dp.iterations < 1u || dp.iterations > 8u) fail(SPT_ERR_INVALID_ARG, "film_denoise: iterations must be 1 .. 8");
    for (const float v : {dp.k_color, dp.k_guide, dp.eps_color, dp.eps_guide})
        if (!std::isfinite(v) || !(v > 0.0f)) fail(SPT_ERR_INVALID_ARG, "film_denoise: k_color, k_guide, eps_color and eps_guide must be finite and > 0");
    return dp;
}

// The iterations of the filter over packed records: color[0] holds c_0 / lv_0, gbuf / abuf the guide's and the albedo's records
// (null: no such term); the last iteration writes width * rows * 3 f32 to rgb_out.
static void denoise_iterate(hipStream_t st, uint32_t width, uint32_t rows, const spt_denoise_params& dp, const DenoiseAlbedo& ab,
                            float4* const color[2], const float4* gbuf, const float4* abuf, float* rgb_out) {
    const bool guide = gbuf != nullptr, albedo = abuf != nullptr;
    const dim3 block(kBlock);
    DenoiseArgs a{};
    a.width = width;
    a.rows = rows;
    a.tiles_x = (width + kTile - 1) / kTile;
    a.kc2 = dp.k_color * dp.k_color;
    a.kg2 = dp.k_guide * dp.k_guide;
    a.eps_c = dp.eps_color;
    a.eps_g = dp.eps_guide;
    const dim3 grid(a.tiles_x * ((rows + kTile - 1) / kTile));
    for (uint32_t k = 0; k < dp.iterations; ++k) {
        a.step = (int32_t)(1u << k);
        const float4* src = color[k & 1u];
        float4* dst = color[(k + 1u) & 1u];
        const bool last = k + 1u == dp.iterations;
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, st, a, src, gbuf, dst, rgb_out); };
        auto launch_albedo = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, st, a, ab, src, gbuf, abuf, dst, rgb_out); };
        if (albedo && guide && last) launch_albedo(k_denoise_atrous_albedo<true, true>);
        else if (albedo && guide) launch_albedo(k_denoise_atrous_albedo<true, false>);
        else if (albedo && last) launch_albedo(k_denoise_atrous_albedo<false, true>);
        else if (albedo) launch_albedo(k_denoise_atrous_albedo<false, false>);
        else if (guide && last) launch(k_denoise_atrous<true, true>);
        else if (guide) launch(k_denoise_atrous<true, false>);
        else if (last) launch(k_denoise_atrous<false, true>);
        else launch(k_denoise_atrous<false, false>);
        HIP_CHECK(hipGetLastError());
    }
}

// spt_film_denoise and spt_film_denoise_job behind their argument checks (the scene's lock is held)
static spt_status film_denoise_locked(spt_film* f, spt_film* guide, const spt_denoise_params* params, const FilmReadOut& to,
                                      const DenoiseAlbedoJob& aj = DenoiseAlbedoJob{}) {
    spt_scene* sc = f->sc;
    const spt_render_params& p = f->plan;
    spt_film* const albedo = aj.film;
    // every check comes before the first launch: a refused call leaves the workspace as it was, and it reads the films only
    auto check_film = [](const spt_film* x, const char* who) {
        if (!(x->flags & SPT_FILM_MOMENTS))
            fail(SPT_ERR_INVALID_ARG, std::string("film_denoise: the ") + who + " was created without SPT_FILM_MOMENTS (the weights need the variance of the mean)");
        if (x->done < 2) fail(SPT_ERR_INVALID_ARG, std::string("film_denoise: the ") + who + " covers fewer than 2 samples (no variance yet)");
    };
    check_film(f, "film");
    if (guide) {
        if (guide == f) fail(SPT_ERR_INVALID_ARG, "film_denoise: the guide is the film itself");
        if (guide->sc != sc) fail(SPT_ERR_INVALID_ARG, "film_denoise: the guide belongs to another scene object");
        check_film(guide, "guide");
        const spt_render_params& g = guide->plan;
        if (g.width != p.width || g.height != p.height) fail(SPT_ERR_INVALID_ARG, "film_denoise: the guide has another width or height");
        if (g.shard_index != p.shard_index || (g.shard_count ? g.shard_count : 1u) != (p.shard_count ? p.shard_count : 1u) ||
            (g.strip_rows ? g.strip_rows : 1u) != (p.strip_rows ? p.strip_rows : 1u) || guide->rows != f->rows)
            fail(SPT_ERR_INVALID_ARG, "film_denoise: the guide has another shard layout");
    }
    if (albedo) {   // checked exactly as the guide is
        if (albedo == f) fail(SPT_ERR_INVALID_ARG, "film_denoise_job: the albedo film is the film itself");
        if (albedo == guide) fail(SPT_ERR_INVALID_ARG, "film_denoise_job: the albedo film is the guide");
        if (albedo->sc != sc) fail(SPT_ERR_INVALID_ARG, "film_denoise_job: the albedo film belongs to another scene object");
        check_film(albedo, "albedo film");
        const spt_render_params& g = albedo->plan;
        if (g.width != p.width || g.height != p.height) fail(SPT_ERR_INVALID_ARG, "film_denoise_job: the albedo film has another width or height");
        if (g.shard_index != p.shard_index || (g.shard_count ? g.shard_count : 1u) != (p.shard_count ? p.shard_count : 1u) ||
            (g.strip_rows ? g.strip_rows : 1u) != (p.strip_rows ? p.strip_rows : 1u) || albedo->rows != f->rows)
            fail(SPT_ERR_INVALID_ARG, "film_denoise_job: the albedo film has another shard layout");
    }
    const spt_denoise_params dp = denoise_params_checked(params, aj);
    if (f->radius != 0.5f || (guide && guide->radius != 0.5f) || (albedo && albedo->radius != 0.5f))
        fail(SPT_ERR_UNSUPPORTED, "film_denoise: needs the box radius 0.5 on both films (every sample of the pixel weighs 1)");
    if (p.shard_count > 1u) fail(SPT_ERR_UNSUPPORTED, "film_denoise: the plan has shard_count > 1 (a shard's packed rows are not neighbours in the image)");
    if (f->rows == 0 || p.width == 0) return SPT_OK;
    const uint32_t n_pix = f->rows * p.width;
    HIP_CHECK(hipSetDevice(sc->device));
    film_join(sc);
    const hipStream_t st = sc->stream;
    const size_t rec_bytes = (size_t)n_pix * sizeof(float4), out_bytes = (size_t)n_pix * 3 * sizeof(float);
    f->dn_color[0].ensure(rec_bytes);
    if (dp.iterations > 1u) f->dn_color[1].ensure(rec_bytes);
    if (guide) f->dn_guide.ensure(rec_bytes);
    if (albedo) f->dn_albedo.ensure(rec_bytes);
    f->out.ensure(out_bytes);
    float4* color[2] = {f->dn_color[0].as<float4>(), dp.iterations > 1u ? f->dn_color[1].as<float4>() : nullptr};
    float4* const gbuf = guide ? f->dn_guide.as<float4>() : nullptr;
    float4* const abuf = albedo ? f->dn_albedo.as<float4>() : nullptr;
    const DenoiseAlbedo ab{aj.k_albedo * aj.k_albedo, aj.eps_albedo, aj.eps_demod, aj.demodulate ? 1u : 0u};
    const dim3 pack_grid((n_pix + kBlock - 1) / kBlock), block(kBlock);
    if (albedo) {
        const DenoiseFilm gin = guide ? denoise_input(guide) : DenoiseFilm{};
        auto pack = [&](auto kernel) { hipLaunchKernelGGL(kernel, pack_grid, block, 0, st, n_pix, denoise_input(f), gin, denoise_input(albedo), ab, color[0], gbuf, abuf); };
        if (guide) pack(k_denoise_pack_albedo<true>);
        else pack(k_denoise_pack_albedo<false>);
    } else if (guide) hipLaunchKernelGGL(k_denoise_pack<true>, pack_grid, block, 0, st, n_pix, denoise_input(f), denoise_input(guide), color[0], gbuf);
    else hipLaunchKernelGGL(k_denoise_pack<false>, pack_grid, block, 0, st, n_pix, denoise_input(f), DenoiseFilm{}, color[0], gbuf);
    HIP_CHECK(hipGetLastError());
    denoise_iterate(st, p.width, f->rows, dp, ab, color, gbuf, abuf, f->out.as<float>());
    film_deliver(f, f->out.p, (size_t)n_pix * 3, to, st);
    return SPT_OK;
}

spt_status spt_film_denoise(spt_film* f, spt_film* guide, const spt_denoise_params* params, float* out) {
    if (!f || !out) { g_error = "film_denoise: null argument"; return SPT_ERR_INVALID_ARG; }
    if (denoise_libraries_differ(f, guide)) return SPT_ERR_INVALID_ARG;
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_denoise(f->inner, guide ? guide->inner : nullptr, params, out));
    std::lock_guard<std::mutex> lock(f->sc->mu);
    return guarded("film_denoise", [&] { return film_denoise_locked(f, guide, params, FilmReadOut{out, nullptr}); });
}

spt_status spt_film_denoise_job(spt_film* f, const spt_denoise_job* job, void* out) {
    if (!f || !job || !out) { g_error = "film_denoise_job: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < offsetof(spt_denoise_job, k_albedo)) { g_error = "film_denoise_job: job->size ends before k_albedo"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)(SPT_DENOISE_DEMODULATE | SPT_DENOISE_OUT_RGB8)) { g_error = "film_denoise_job: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if ((job->flags & SPT_DENOISE_DEMODULATE) && !job->albedo) { g_error = "film_denoise_job: SPT_DENOISE_DEMODULATE needs an albedo film"; return SPT_ERR_INVALID_ARG; }
    if (denoise_libraries_differ(f, job->guide) || denoise_libraries_differ(f, job->albedo)) return SPT_ERR_INVALID_ARG;
    if (f->fwd) {   // the same job with the inner handles
        spt_denoise_job inner{};
        std::memcpy(&inner, job, std::min<size_t>(job->size, sizeof inner));
        inner.size = (uint32_t)std::min<size_t>(job->size, sizeof inner);
        inner.guide = job->guide ? job->guide->inner : nullptr;
        inner.albedo = job->albedo ? job->albedo->inner : nullptr;
        return forwarded(f->fwd, f->fwd->film_denoise_job(f->inner, &inner, out));
    }
    DenoiseAlbedoJob aj;
    aj.film = job->albedo;
    aj.demodulate = (job->flags & SPT_DENOISE_DEMODULATE) != 0;
    // (the struct only grows at its tail: a float the caller's struct ends before keeps its default)
    if (job->size >= offsetof(spt_denoise_job, k_albedo) + sizeof(float)) aj.k_albedo = job->k_albedo;
    if (job->size >= offsetof(spt_denoise_job, eps_albedo) + sizeof(float)) aj.eps_albedo = job->eps_albedo;
    if (job->size >= offsetof(spt_denoise_job, eps_demod) + sizeof(float)) aj.eps_demod = job->eps_demod;
    const bool rgb8 = (job->flags & SPT_DENOISE_OUT_RGB8) != 0;
    const FilmReadOut to{rgb8 ? nullptr : static_cast<float*>(out), rgb8 ? static_cast<uint8_t*>(out) : nullptr};
    std::lock_guard<std::mutex> lock(f->sc->mu);
    return guarded("film_denoise_job", [&] { return film_denoise_locked(f, job->guide, job->params, to, aj); });
}

// The filter of spt_film_denoise_job on caller-provided images: the arrays go up through the scene's page-locked staging buffer,
// k_denoise_pack_image makes the records, and the a-trous kernels, k_pack_rgb8 and the copy-out are those of the film calls.
spt_status spt_denoise_image(const spt_scene* scene_c, const spt_image_denoise_job* job, void* out) {
    if (!scene_c || !job || !out) { g_error = "denoise_image: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < offsetof(spt_image_denoise_job, k_albedo)) { g_error = "denoise_image: job->size ends before k_albedo"; return SPT_ERR_INVALID_ARG; }
    if (!job->mean || !job->var) { g_error = "denoise_image: null mean or var array"; return SPT_ERR_INVALID_ARG; }
    if ((job->guide_mean != nullptr) != (job->guide_var != nullptr)) { g_error = "denoise_image: guide_mean and guide_var go together (both or neither)"; return SPT_ERR_INVALID_ARG; }
    if ((job->albedo_mean != nullptr) != (job->albedo_var != nullptr)) { g_error = "denoise_image: albedo_mean and albedo_var go together (both or neither)"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)(SPT_DENOISE_DEMODULATE | SPT_DENOISE_OUT_RGB8)) { g_error = "denoise_image: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if ((job->flags & SPT_DENOISE_DEMODULATE) && !job->albedo_mean) { g_error = "denoise_image: SPT_DENOISE_DEMODULATE needs the albedo arrays"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) return forwarded(sc->fwd, sc->fwd->denoise_image(sc->inner, job, out));
    DenoiseAlbedoJob aj;
    aj.demodulate = (job->flags & SPT_DENOISE_DEMODULATE) != 0;
    // (the struct only grows at its tail: a float the caller's struct ends before keeps its default)
    if (job->size >= offsetof(spt_image_denoise_job, k_albedo) + sizeof(float)) aj.k_albedo = job->k_albedo;
    if (job->size >= offsetof(spt_image_denoise_job, eps_albedo) + sizeof(float)) aj.eps_albedo = job->eps_albedo;
    if (job->size >= offsetof(spt_image_denoise_job, eps_demod) + sizeof(float)) aj.eps_demod = job->eps_demod;
    const bool rgb8 = (job->flags & SPT_DENOISE_OUT_RGB8) != 0;
    const FilmReadOut to{rgb8 ? nullptr : static_cast<float*>(out), rgb8 ? static_cast<uint8_t*>(out) : nullptr};
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("denoise_image", [&] {
        // every check comes before the first allocation, copy or launch: a refused call leaves the workspace as it was
        const spt_denoise_params dp = denoise_params_checked(job->params, aj);
        const uint64_t n_pix64 = (uint64_t)job->width * job->rows;
        if (n_pix64 * 3u > 0xfffffffcull) fail(SPT_ERR_UNSUPPORTED, "denoise_image: image larger than 2^32 - 4 floats");
        if (n_pix64 == 0) return SPT_OK;
        const uint32_t n_pix = (uint32_t)n_pix64;
        const bool guide = job->guide_mean != nullptr, albedo = job->albedo_mean != nullptr;
        const float* const src[6] = {job->mean, job->var, job->guide_mean, job->guide_var, job->albedo_mean, job->albedo_var};
        const size_t img_bytes = (size_t)n_pix * 3 * sizeof(float), rec_bytes = (size_t)n_pix * sizeof(float4);
        HIP_CHECK(hipSetDevice(sc->device));
        film_join(sc);
        const hipStream_t st = sc->stream;
        sc->img_stage.ensure(img_bytes * (2u + (guide ? 2u : 0u) + (albedo ? 2u : 0u)));
        for (int k = 0; k < 6; ++k)
            if (src[k]) sc->img_in[k].ensure(img_bytes);
        sc->img_color[0].ensure(rec_bytes);
        if (dp.iterations > 1u) sc->img_color[1].ensure(rec_bytes);
        if (guide) sc->img_guide.ensure(rec_bytes);
        if (albedo) sc->img_albedo.ensure(rec_bytes);
        sc->img_out.ensure(img_bytes);
        // Each array has a slot of its own in the staging buffer: the host copies array k + 1 into its slot while the DMA of
        // array k is in flight, and nothing waits before the end of the call (which is why no slot is reused within it)
        char* slot = static_cast<char*>(sc->img_stage.p);
        for (int k = 0; k < 6; ++k) {
            if (!src[k]) continue;
            std::memcpy(slot, src[k], img_bytes);
            HIP_CHECK(hipMemcpyAsync(sc->img_in[k].p, slot, img_bytes, hipMemcpyHostToDevice, st));
            slot += img_bytes;
        }
        DenoiseImage in{};
        in.mean = sc->img_in[0].as<float>();
        in.var = sc->img_in[1].as<float>();
        if (guide) { in.guide_mean = sc->img_in[2].as<float>(); in.guide_var = sc->img_in[3].as<float>(); }
        if (albedo) { in.albedo_mean = sc->img_in[4].as<float>(); in.albedo_var = sc->img_in[5].as<float>(); }
        float4* color[2] = {sc->img_color[0].as<float4>(), dp.iterations > 1u ? sc->img_color[1].as<float4>() : nullptr};
        float4* const gbuf = guide ? sc->img_guide.as<float4>() : nullptr;
        float4* const abuf = albedo ? sc->img_albedo.as<float4>() : nullptr;
        const DenoiseAlbedo ab{aj.k_albedo * aj.k_albedo, aj.eps_albedo, aj.eps_demod, aj.demodulate ? 1u : 0u};
        const dim3 pack_grid((n_pix + kBlock - 1) / kBlock), block(kBlock);
        auto pack = [&](auto kernel) { hipLaunchKernelGGL(kernel, pack_grid, block, 0, st, n_pix, in, ab, color[0], gbuf, abuf); };
        if (guide && albedo) pack(k_denoise_pack_image<true, true>);
        else if (albedo) pack(k_denoise_pack_image<false, true>);
        else if (guide) pack(k_denoise_pack_image<true, false>);
        else pack(k_denoise_pack_image<false, false>);
        HIP_CHECK(hipGetLastError());
        denoise_iterate(st, job->width, job->rows, dp, ab, color, gbuf, abuf, sc->img_out.as<float>());
        deliver(sc->img_out8, sc->img_out.p, (size_t)n_pix * 3, to, st);
        return SPT_OK;
    });
}

spt_status spt_render_flags_supported(uint32_t* mask) {
    if (!mask) { g_error = "render_flags_supported: null argument"; return SPT_ERR_INVALID_ARG; }
    *mask = SPT_RENDER_PROFILE | SPT_RENDER_BOX_RADIUS | SPT_RENDER_COUNT_VISITS | SPT_RENDER_ASYNC | SPT_RENDER_DEBUG_NORMAL | SPT_RENDER_AOV_ALBEDO;
    return SPT_OK;
}

spt_status spt_film_buckets(spt_film* f, uint32_t n_buckets) {
    if (!f) { g_error = "film_buckets: null argument"; return SPT_ERR_INVALID_ARG; }
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_buckets(f->inner, n_buckets));
    spt_scene* sc = f->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("film_buckets", [&] {
        const spt_render_params& p = f->plan;
        // every check comes before the first change: a refused call leaves the film as it was
        if (f->flags & SPT_FILM_KEEP_SAMPLES) fail(SPT_ERR_INVALID_ARG, "film_buckets: a film that keeps its samples (SPT_FILM_KEEP_SAMPLES) has no bucket sums");
        if (n_buckets < 3u || n_buckets > kMaxBuckets || (n_buckets & 1u) == 0u)
            fail(SPT_ERR_INVALID_ARG, "film_buckets: n_buckets must be odd and 3 .. 15 (got " + std::to_string(n_buckets) + ")");
        if (f->n_buckets != 0u) fail(SPT_ERR_INVALID_ARG, "film_buckets: the film already has buckets");
        if (f->done != 0u) fail(SPT_ERR_INVALID_ARG, "film_buckets: the film already covers samples (buckets start with the film)");
        if (f->radius != 0.5f) fail(SPT_ERR_UNSUPPORTED, "film_buckets: needs the box radius 0.5 (every sample of the pixel weighs 1)");
        HIP_CHECK(hipSetDevice(sc->device));
        film_join(sc);
        const hipStream_t st = sc->stream;
        const size_t bytes = (size_t)n_buckets * f->rows * p.width * 3 * sizeof(float);
        DeviceBuffer buckets, inv_dev;   // the film gets them once everything has worked
        std::vector<float> inv((size_t)p.spp + 1, 0.0f);
        for (uint32_t k = 1; k <= p.spp; ++k) inv[k] = 1.0f / (float)k;
        if (bytes != 0) {
            buckets.alloc(bytes);
            HIP_CHECK(hipMemsetAsync(buckets.p, 0, bytes, st));
        }
        inv_dev.alloc(inv.size() * sizeof(float));
        HIP_CHECK(hipMemcpyAsync(inv_dev.p, inv.data(), inv.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));   // `inv` is pageable
        f->buckets.swap(buckets);
        f->b_inv.swap(inv_dev);
        f->n_buckets = n_buckets;
        return SPT_OK;
    });
}

spt_status spt_film_read_buckets(spt_film* f, float* out) {
    if (!f || !out) { g_error = "film_read_buckets: null argument"; return SPT_ERR_INVALID_ARG; }
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_read_buckets(f->inner, out));
    spt_scene* sc = f->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("film_read_buckets", [&] {
        if (f->n_buckets == 0u) fail(SPT_ERR_INVALID_ARG, "film_read_buckets: the film has no buckets (spt_film_buckets)");
        const size_t bytes = (size_t)f->n_buckets * f->rows * f->plan.width * 3 * sizeof(float);
        if (bytes == 0) return SPT_OK;
        HIP_CHECK(hipSetDevice(sc->device));
        film_join(sc);
        HIP_CHECK(hipMemcpyAsync(out, f->buckets.p, bytes, hipMemcpyDeviceToHost, sc->stream));
        HIP_CHECK(hipStreamSynchronize(sc->stream));
        return SPT_OK;
    });
}

// spt_film_read_robust behind its argument checks (the scene's lock is held)
static spt_status film_read_robust_locked(spt_film* f, uint32_t estimator, const FilmReadOut& to) {
    spt_scene* sc = f->sc;
    const spt_render_params& p = f->plan;
    if (f->n_buckets == 0u) fail(SPT_ERR_INVALID_ARG, "film_read_robust: the film has no buckets (spt_film_buckets)");
    if (estimator > SPT_ROBUST_GMON) fail(SPT_ERR_INVALID_ARG, "film_read_robust: unknown SPT_ROBUST_* value");
    if (f->done == 0) fail(SPT_ERR_INVALID_ARG, "film_read_robust: the film covers no samples yet");
    if (f->rows == 0 || p.width == 0) return SPT_OK;
    const uint32_t n_pix = f->rows * p.width, K = f->n_buckets;
    const size_t bytes = (size_t)n_pix * 3 * sizeof(float);
    HIP_CHECK(hipSetDevice(sc->device));
    film_join(sc);
    const hipStream_t st = sc->stream;
    f->out.ensure(bytes);
    const float kf = (float)K, gk = (float)(K + 1u) / (float)K, hf = (float)((K - 1u) / 2u);
    const dim3 grid((n_pix * 3 + kBlock - 1) / kBlock), block(kBlock);
    if (f->adaptive)
        hipLaunchKernelGGL(k_film_read_robust<true>, grid, block, 0, st, estimator, n_pix * 3u, K, f->sum.as<float>(), f->buckets.as<float>(),
                           (size_t)n_pix * 3, f->first, f->done, f->mask.as<uint8_t>(), f->counts.as<uint32_t>(), f->b_inv.as<float>(), kf, gk, hf,
                           f->out.as<float>());
    else
        hipLaunchKernelGGL(k_film_read_robust<false>, grid, block, 0, st, estimator, n_pix * 3u, K, f->sum.as<float>(), f->buckets.as<float>(),
                           (size_t)n_pix * 3, f->first, f->done, (const uint8_t*)nullptr, (const uint32_t*)nullptr, f->b_inv.as<float>(), kf, gk, hf,
                           f->out.as<float>());
    HIP_CHECK(hipGetLastError());
    film_deliver(f, f->out.p, (size_t)n_pix * 3, to, st);
    return SPT_OK;
}

spt_status spt_film_read_robust(spt_film* f, uint32_t estimator, float* out) {
    if (!f || !out) { g_error = "film_read_robust: null argument"; return SPT_ERR_INVALID_ARG; }
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_read_robust(f->inner, estimator, out));
    std::lock_guard<std::mutex> lock(f->sc->mu);
    return guarded("film_read_robust", [&] { return film_read_robust_locked(f, estimator, FilmReadOut{out, nullptr}); });
}

// The 8-bit read-out: the float image of `source` exactly as the matching call above stages it, then k_pack_rgb8.
spt_status spt_film_read_rgb8(spt_film* f, uint32_t source, spt_film* guide, const spt_denoise_params* dn, uint8_t* out) {
    if (!f || !out) { g_error = "film_read_rgb8: null argument"; return SPT_ERR_INVALID_ARG; }
    if (source > SPT_READ_DENOISED) { g_error = "film_read_rgb8: unknown SPT_READ_* value"; return SPT_ERR_INVALID_ARG; }
    const bool denoised = source == SPT_READ_DENOISED;
    if (denoised && denoise_libraries_differ(f, guide)) return SPT_ERR_INVALID_ARG;
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_read_rgb8(f->inner, source, denoised && guide ? guide->inner : nullptr, dn, out));
    std::lock_guard<std::mutex> lock(f->sc->mu);
    return guarded("film_read_rgb8", [&] {
        const FilmReadOut to{nullptr, out};
        if (denoised) return film_denoise_locked(f, guide, dn, to);
        if (source == SPT_READ_MEAN) return film_read_locked(f, SPT_FILM_MEAN, to);
        return film_read_robust_locked(f, source == SPT_READ_ROBUST_MON ? SPT_ROBUST_MON : SPT_ROBUST_GMON, to);
    });
}

spt_status spt_film_filter(spt_film* f, const spt_filter_desc* desc) {
    if (!f || !desc) { g_error = "film_filter: null argument"; return SPT_ERR_INVALID_ARG; }
    if (f->fwd) {
        if (!f->fwd->film_filter) { g_error = "film_filter: libspt_hip_bez.so does not export spt_film_filter"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(f->fwd, f->fwd->film_filter(f->inner, desc));
    }
    std::lock_guard<std::mutex> lock(f->sc->mu);
    return guarded("film_filter", [&] {
        // every check comes before the first change: a refused call leaves the film and its filter as they were
        if (desc->size < sizeof(spt_filter_desc)) fail(SPT_ERR_INVALID_ARG, "film_filter: desc->size is below sizeof(spt_filter_desc)");
        if (desc->type > SPT_FILTER_MITCHELL) fail(SPT_ERR_INVALID_ARG, "film_filter: unknown SPT_FILTER_* value");
        if (!(f->flags & SPT_FILM_KEEP_SAMPLES)) fail(SPT_ERR_INVALID_ARG, "film_filter: the film was created without SPT_FILM_KEEP_SAMPLES");
        if (desc->type == SPT_FILTER_BOX) {
            f->filter_type = SPT_FILTER_BOX;
            return SPT_OK;
        }
        const float r = desc->radius;
        if (!std::isfinite(r) || r <= 0.0f) fail(SPT_ERR_INVALID_ARG, "film_filter: the radius must be finite and > 0");
        const float rf = std::max(std::ceil(r - 0.5f), 0.0f);
        const int32_t halo = std::max(f->R, 0);
        if (rf > (float)halo)
            fail(SPT_ERR_INVALID_ARG, "film_filter: radius " + std::to_string(r) + " reads " + std::to_string((double)rf) + " neighbouring rows, the film stores " +
                                          std::to_string(halo) + " (create it with the plan's filter_radius " + std::to_string(r) + " or more)");
        FilterCoef fc{};
        if (desc->type == SPT_FILTER_GAUSSIAN) {
            const float alpha = desc->p0;
            if (!std::isfinite(alpha) || alpha <= 0.0f) fail(SPT_ERR_INVALID_ARG, "film_filter: the Gaussian's alpha must be finite and > 0");
            fc.a[0] = alpha;
            fc.a[1] = spt_exp(-(alpha * (r * r)));
        } else if (desc->type == SPT_FILTER_MITCHELL) {
            if (!std::isfinite(desc->p0) || !std::isfinite(desc->p1)) fail(SPT_ERR_INVALID_ARG, "film_filter: Mitchell's B and C must be finite");
            const double B = (double)desc->p0, C = (double)desc->p1;
            fc.a[0] = (float)((-B - 6 * C) / 6);
            fc.a[1] = (float)((6 * B + 30 * C) / 6);
            fc.a[2] = (float)((-12 * B - 48 * C) / 6);
            fc.a[3] = (float)((8 * B + 24 * C) / 6);
            fc.a[4] = (float)((12 - 9 * B - 6 * C) / 6);
            fc.a[5] = (float)((-18 + 12 * B + 6 * C) / 6);
            fc.a[6] = (float)((6 - 2 * B) / 6);
        }
        f->filter_type = desc->type;
        f->filter_radius = r;
        f->filter_R = (int32_t)rf;
        f->filter_coef = fc;
        return SPT_OK;
    });
}

spt_status spt_film_read_samples(spt_film* f, uint32_t first, uint32_t count, float* out) {
    if (!f || !out) { g_error = "film_read_samples: null argument"; return SPT_ERR_INVALID_ARG; }
    if (f->fwd) return forwarded(f->fwd, f->fwd->film_read_samples(f->inner, first, count, out));
    spt_scene* sc = f->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("film_read_samples", [&] {
        const spt_render_params& p = f->plan;
        if (!(f->flags & SPT_FILM_KEEP_SAMPLES)) fail(SPT_ERR_INVALID_ARG, "film_read_samples: the film was created without SPT_FILM_KEEP_SAMPLES");
        if (first < f->first || (uint64_t)first + count > (uint64_t)f->first + f->done)
            fail(SPT_ERR_INVALID_ARG, "film_read_samples: samples [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                          ") are not all covered (the film covers [" + std::to_string(f->first) + ", " + std::to_string(f->first + f->done) + "))");
        if (count == 0 || f->rows == 0) return SPT_OK;
        HIP_CHECK(hipSetDevice(sc->device));
        film_join(sc);
        const hipStream_t st = sc->stream;
        // staged through the film's read-out buffer, up to 256 MB (and the grid's 65535 planes) at a time
        const size_t plane = (size_t)f->rows * p.width * 3;
        const uint32_t batch = (uint32_t)std::max<size_t>(1, std::min<size_t>(65535, (256u << 20) / (plane * sizeof(float))));
        f->out.ensure(plane * sizeof(float) * std::min(batch, count));
        for (uint32_t k0 = 0; k0 < count; k0 += batch) {
            const uint32_t n = std::min(batch, count - k0);
            for (const auto& r : f->runs) {
                const KeptJob job = kept_job(f, r, f->out.as<float>() + r.out_row * (size_t)p.width * 3, false);
                const size_t floats = (size_t)(r.j1 - r.j0) * p.width * 3;
                hipLaunchKernelGGL(k_film_read_kept, dim3((uint32_t)((floats + kBlock - 1) / kBlock), n), dim3(kBlock), 0, st, job, p.width, first + k0, plane);
            }
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(out + (size_t)k0 * plane, f->out.p, (size_t)n * plane * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        return SPT_OK;
    });
}

void spt_film_destroy(spt_film* f) {
    if (!f) return;
    if (f->fwd) {
        f->fwd->film_destroy(f->inner);
        delete f;
        return;
    }
    std::lock_guard<std::mutex> lock(f->sc->mu);
    (void)hipSetDevice(f->sc->device);
    (void)hipStreamSynchronize(f->sc->stream);   // (every film call is synchronous; nothing of this film is queued)
    if (f->sc->live_films) --f->sc->live_films;
    delete f;
}

static spt_status trace_common(const spt_scene* scene_c, uint32_t n, const spt_ray* rays, void* out, size_t out_elem, bool closest) {
    if (!scene_c || (n && (!rays || !out))) { g_error = "trace: null argument"; return SPT_ERR_INVALID_ARG; }
    if (n == 0) return SPT_OK;
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd)
        return forwarded(sc->fwd, closest ? sc->fwd->trace_closest(sc->inner, n, rays, static_cast<spt_hit*>(out))
                                          : sc->fwd->trace_any(sc->inner, n, rays, static_cast<uint8_t*>(out)));
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("trace", [&] {
        HIP_CHECK(hipSetDevice(sc->device));
        film_join(sc);
        sc->trace_in.ensure((size_t)n * sizeof(spt_ray));
        sc->trace_out.ensure((size_t)n * out_elem);
        hipStream_t st = sc->stream;
        HIP_CHECK(hipMemcpyAsync(sc->trace_in.p, rays, (size_t)n * sizeof(spt_ray), hipMemcpyHostToDevice, st));
        // the streaming walker, or the walker over the LDS-resident / memory geometry
        const bool stream = sc->swalk && !sc->lds_geo;
        auto launch = [&](auto kernel, auto* results) {
            hipLaunchKernelGGL(kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), sc->lds_bytes, st, sc->d, n, sc->trace_in.as<spt_ray>(), results);
        };
        if (closest) launch(stream ? k_trace_closest_stream : sc->lds_geo ? k_trace_closest<true> : k_trace_closest<false>, sc->trace_out.as<spt_hit>());
        else launch(stream ? k_trace_any_stream : sc->lds_geo ? k_trace_any<true> : k_trace_any<false>, sc->trace_out.as<uint8_t>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out, sc->trace_out.p, (size_t)n * out_elem, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return SPT_OK;
    });
}

// ---- jobs of n items x S samples without a camera: spt_radiance (rays x repetitions), spt_bake (points), spt_probe (probes) ----
// An entry checks its arguments, begins an ItemRun, cuts the job into passes of P items x chunks of R samples, and per pass stages its
// item records, fills its kernels' job struct and runs the chunks with its intake and finish kernels.

// `p` is device memory on the scene's device, aligned to `align` bytes (a power of two); below: to 16 bytes where `align16` (records
// loaded as float4), else to 4
static void check_device_pointer_aligned(const spt_scene* sc, const char* who, const char* flag, const void* p, const char* what, uint32_t align) {
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof at);
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != sc->device)
        fail(SPT_ERR_INVALID_ARG, std::string(who) + ": " + flag + " and `" + what + "` is not device memory on the scene's device");
    if ((reinterpret_cast<uintptr_t>(p) & (uintptr_t)(align - 1u)) != 0)
        fail(SPT_ERR_INVALID_ARG, std::string(who) + ": device pointer `" + what + "` is not " + std::to_string(align) + "-byte aligned");
}
static void check_device_pointer(const spt_scene* sc, const char* who, const char* flag, const void* p, const char* what, bool align16) {
    check_device_pointer_aligned(sc, who, flag, p, what, align16 ? 16u : 4u);
}

extern "C++" {   // (member templates cannot have C linkage; it stands here, inside the file's extern "C" block, behind deliver and FilmReadOut)
struct ItemRun {
    spt_scene* const sc;
    const char* const who;         // the entry, for the refusals
    spt_render_params plan{};      // what run_setup and bounce read of a plan
    const spt_camera no_camera{};
    RenderRun run;                 // (points at the two above)
    RenderCtx rc{};
    hipStream_t st = nullptr;
    uint32_t P = 0, R = 0;         // items per pass, samples per chunk
    uint32_t k_end = 0;            // the samples that are traced: S, or 0 where nothing asks for a first segment's path
    size_t counts_words = 0;
    size_t in_cap = 0;             // host lists: the bytes of a staging slot that hold the item records of a full pass

    // Joins the films and makes the kernel choices of the call (the scene's lock is held and its device selected)
    ItemRun(spt_scene* sc_, const char* who_, uint32_t max_depth, uint64_t seed, uint32_t S) : sc(sc_), who(who_) {
        film_join(sc);
        plan.max_depth = max_depth;
        run.sc = sc;
        run.cam = &no_camera;
        run.params = &plan;
        run.rays = true;
        run_setup(run);
        st = run.st;
        rc.max_depth = max_depth;
        rc.seed = seed;
        rc.spp = S;
        rc.dyn_refill_below = run.dyn_refill_below;
        rc.dyn_steps = run.dyn_steps;
        rc.stream_rounds = run.stream_rounds;
        rc.stream_refill_below = run.stream_refill_below;
        rc.visits = sc->visits.as<unsigned long long>();
    }
    ItemRun(const ItemRun&) = delete;

    // Passes of P items x chunks of R samples, around 2^22 paths each (`per_pass`: the caller's P, the job field `per_pass_name`; 0:
    // ours).  Workgroup g of an intake launch appends to queue shard g % kShards only, so a shard's capacity comes in steps of
    // kShards * kBlock items - the default P is a multiple of that - times R (first_segment.h).  Grows the queues, the counters and
    // the radiance slots of such a pass and binds them into rc, as grow_workspace does for a window of pixels.
    void cut(uint64_t n_items, uint32_t S, uint32_t per_pass, const char* per_pass_name, uint32_t k_end_) {
        constexpr uint64_t kStep = (uint64_t)kShards * kBlock, kTargetPaths = 1ull << 22;
        const uint64_t P64 = std::min<uint64_t>(per_pass ? per_pass : std::max(kStep, kTargetPaths / S / kStep * kStep), n_items);
        const uint64_t P_up = (P64 + kStep - 1) / kStep * kStep;
        P = (uint32_t)P64;
        R = (uint32_t)std::min<uint64_t>(S, std::max<uint64_t>(1, 2 * kTargetPaths / P_up));
        if (P_up * R > 0x7fffffffull) fail(SPT_ERR_UNSUPPORTED, std::string(who) + ": pass too large (lower " + per_pass_name + ")");
        k_end = k_end_;
        const uint32_t reps = k_end ? R : 1u;
        counts_words = grow_queues(sc, (size_t)(P_up * reps), (uint32_t)(P_up / kShards * reps), rc.max_depth, run.fused, run.class_queues, false, rc);
        grow(sc, sc->rad[0], (size_t)P * reps * 3 * sizeof(float));
        rc.rad = sc->rad[0].as<float>();
    }

    // Host lists: the two pinned staging slots of in_bytes + aux_bytes with their events, the device copies of a pass' records, and
    // `out_bytes` of results for the whole job (sc->ray_rgb), which it returns
    float* stage_buffers(size_t in_bytes, size_t aux_bytes, size_t out_bytes) {
        in_cap = in_bytes;
        for (int k = 0; k < 2; ++k) {
            sc->ray_stage[k].ensure(in_bytes + aux_bytes);
            if (!sc->ev_ray[k]) HIP_CHECK(hipEventCreateWithFlags(&sc->ev_ray[k], hipEventDisableTiming));
        }
        sc->ray_in.ensure(in_bytes);
        if (aux_bytes) sc->ray_aux_in.ensure(aux_bytes);
        sc->ray_rgb.ensure(out_bytes);
        return sc->ray_rgb.as<float>();
    }

    // Host lists: once the slot's previous copy (two passes ago) has left it, `fill(records, aux)` fills it beside the pass in flight;
    // then its in_bytes go to sc->ray_in and its aux_bytes, which lie behind the records of a full pass, to sc->ray_aux_in
    template <class Fill>
    void stage(uint64_t pass, size_t in_bytes, size_t aux_bytes, Fill fill) {
        char* const slot = static_cast<char*>(sc->ray_stage[pass & 1u].p);
        if (pass >= 2) HIP_CHECK(hipEventSynchronize(sc->ev_ray[pass & 1u]));
        fill(slot, slot + in_cap);
        HIP_CHECK(hipMemcpyAsync(sc->ray_in.p, slot, in_bytes, hipMemcpyHostToDevice, st));
        if (aux_bytes) HIP_CHECK(hipMemcpyAsync(sc->ray_aux_in.p, slot + in_cap, aux_bytes, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipEventRecord(sc->ev_ray[pass & 1u], st));
    }

    // Host lists of spt_path_ray (spt_radiance, spt_gbuffer): stage() of the n rays from r0 on, checked while they are copied, with
    // their auxiliary rays (`aux`, or null) behind them
    void stage_rays(uint64_t pass, uint64_t r0, uint32_t n, const spt_path_ray* rays, const spt_ray_aux* aux) {
        stage(pass, (size_t)n * sizeof(spt_path_ray), aux ? (size_t)n * sizeof(spt_ray_aux) : 0, [&](char* records, char* aux_records) {
            spt_path_ray* const dst = reinterpret_cast<spt_path_ray*>(records);
            const spt_path_ray* const src = rays + r0;
            for (uint32_t i = 0; i < n; ++i) {
                const spt_path_ray& r = src[i];
                const bool finite = std::isfinite(r.o[0]) && std::isfinite(r.o[1]) && std::isfinite(r.o[2]) && std::isfinite(r.d[0]) &&
                                    std::isfinite(r.d[1]) && std::isfinite(r.d[2]) && std::isfinite(r.t_min);
                if (!finite || (r.d[0] == 0.0f && r.d[1] == 0.0f && r.d[2] == 0.0f)) {
                    HIP_CHECK(hipStreamSynchronize(st));   // the earlier passes wrote the library's own buffers only
                    fail(SPT_ERR_INVALID_ARG, std::string(who) + ": ray " + std::to_string(r0 + i) + (finite ? " has an all-zero direction" : " has a non-finite o, d or t_min"));
                }
                dst[i] = r;
            }
            if (aux) std::memcpy(aux_records, aux + r0, (size_t)n * sizeof(spt_ray_aux));
        });
    }

    // one of an entry's three intake kernels over the n items of the pass, behind the zeroing of the queue counters
    template <class Job>
    void launch_intake(void (*lds)(DScene, RenderCtx, Job), void (*mem)(DScene, RenderCtx, Job), void (*streaming)(DScene, RenderCtx, Job), const Job& job) {
        const bool stream = sc->swalk && !sc->lds_geo;   // the walkers of spt_trace_closest / spt_trace_any
        HIP_CHECK(hipMemsetAsync(rc.counts, 0, counts_words * sizeof(uint32_t), st));
        hipLaunchKernelGGL(stream ? streaming : sc->lds_geo ? lds : mem, dim3((job.n + kBlock - 1) / kBlock), dim3(kBlock), sc->lds_bytes, st, sc->d, rc, job);
        HIP_CHECK(hipGetLastError());
    }

    // The chunks of a pass of n items: per chunk it writes the job's `k_first` and `reps`, then `intake(first)` (the entry's
    // launch_intake), the bounces, `finish(first, last)`.  With k_end == 0 (`while curr_depth < self.max_depth`, pt.rs:48, never
    // runs: every path is 0) there is one chunk of no samples
    template <class Intake, class Finish>
    void chunks(uint32_t n, uint32_t& k_first, uint32_t& reps, const float4* ray_aux, Intake intake, Finish finish) {
        run.ray_aux = ray_aux;
        run.ray_aux_wrap = n;
        rc.n_pixels = n;
        for (uint64_t k0 = 0; k0 == 0u || k0 < k_end; k0 += R) {
            k_first = (uint32_t)k0;
            reps = (uint32_t)std::min<uint64_t>(R, k_end - std::min<uint64_t>(k0, k_end));
            rc.pass_first = k_first;
            rc.pass_samples = reps;
            rc.rad_plane = (size_t)std::max(reps, 1u) * n;
            intake(k0 == 0u);
            for (uint32_t b = 0; b < (reps ? rc.max_depth : 0u); ++b)
                if (bounce(run, rc, b, st)) break;
            finish(k0 == 0u ? 1u : 0u, k0 + R >= k_end ? 1u : 0u);
            HIP_CHECK(hipGetLastError());
        }
    }

    // the results are where the caller asked: host lists through the device-to-host path of the film read-outs
    void deliver_out(bool dev, float* out, size_t n_floats) {
        if (!dev) deliver(sc->img_out8, sc->ray_rgb.p, n_floats, FilmReadOut{out, nullptr}, st);
        else HIP_CHECK(hipStreamSynchronize(st));
    }
};
}

// ---- radiance along caller rays (spt_radiance) ----
spt_status spt_radiance(const spt_scene* scene_c, const spt_radiance_job* job) {
    if (!scene_c || !job) { g_error = "radiance: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < sizeof(spt_radiance_job)) { g_error = "radiance: job->size is below sizeof(spt_radiance_job)"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)SPT_RADIANCE_DEVICE_POINTERS) { g_error = "radiance: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if (job->repeats == 0) { g_error = "radiance: repeats must be >= 1"; return SPT_ERR_INVALID_ARG; }
    if (job->n_rays != 0 && (!job->rays || !job->rgb_out)) { g_error = "radiance: null rays or rgb_out"; return SPT_ERR_INVALID_ARG; }
    if (job->max_depth > 255) { g_error = "radiance: max_depth > 255"; return SPT_ERR_UNSUPPORTED; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) return forwarded(sc->fwd, sc->fwd->radiance(sc->inner, job));
    if (job->n_rays == 0) return SPT_OK;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("radiance", [&] {
        const uint64_t n_rays = job->n_rays;
        const uint32_t S = job->repeats;
        const bool dev = (job->flags & SPT_RADIANCE_DEVICE_POINTERS) != 0;
        const bool want_hits = job->hits_out != nullptr;
        if (n_rays > (1ull << 40)) fail(SPT_ERR_UNSUPPORTED, "radiance: more than 2^40 rays");
        HIP_CHECK(hipSetDevice(sc->device));
        if (dev) {   // every check comes before the first allocation, copy or launch
            const auto check = [&](const void* p, const char* what, bool align16) { check_device_pointer(sc, "radiance", "SPT_RADIANCE_DEVICE_POINTERS", p, what, align16); };
            check(job->rays, "rays", true);
            if (job->aux) check(job->aux, "aux", true);
            check(job->rgb_out, "rgb_out", false);
            if (want_hits) check(job->hits_out, "hits_out", false);
        }
        ItemRun ir(sc, "radiance", job->max_depth, job->seed, S);
        // auxiliary rays are read by the textured shade levels only
        const bool use_aux = job->aux != nullptr && sc->textured && !sc->simple && !ir.run.fused && job->max_depth > 0;
        // max_depth 0: no path runs; the intake still reports the hits
        ir.cut(n_rays, S, job->rays_per_pass, "rays_per_pass", job->max_depth ? S : 0u);
        const uint32_t P = ir.P;
        float* rgb_dev = job->rgb_out;
        spt_hit* hits_dev = job->hits_out;
        if (!dev) {
            rgb_dev = ir.stage_buffers((size_t)P * sizeof(spt_path_ray), use_aux ? (size_t)P * sizeof(spt_ray_aux) : 0, (size_t)n_rays * 3 * sizeof(float));
            if (want_hits) sc->ray_hits.ensure((size_t)n_rays * sizeof(spt_hit));
            hits_dev = want_hits ? sc->ray_hits.as<spt_hit>() : nullptr;
        }
        const float inv = 1.0f / (float)S;
        uint64_t pass = 0;
        for (uint64_t r0 = 0; r0 < n_rays; r0 += P, ++pass) {
            RayJob rj{};
            rj.seed = job->seed;
            rj.n = (uint32_t)std::min<uint64_t>(P, n_rays - r0);
            rj.rng_skip = job->rng_skip;
            rj.rgb_out = rgb_dev + 3 * r0;
            rj.rays = reinterpret_cast<const float4*>(job->rays + r0);
            const float4* aux_dev = use_aux ? reinterpret_cast<const float4*>(job->aux + r0) : nullptr;
            if (!dev) {   // the host checks the rays while it copies them
                ir.stage_rays(pass, r0, rj.n, job->rays, use_aux ? job->aux : nullptr);
                rj.rays = sc->ray_in.as<float4>();
                if (use_aux) aux_dev = sc->ray_aux_in.as<float4>();
            }
            // (chunks() writes rj.k_first and rj.reps before each call of the two lambdas, which launch with rj as it then stands)
            ir.chunks(rj.n, rj.k_first, rj.reps, aux_dev,
                      [&](bool first) {
                          rj.hits_out = (first && hits_dev) ? hits_dev + r0 : nullptr;
                          if (rj.reps != 0u || rj.hits_out != nullptr) ir.launch_intake(k_ray_intake<true>, k_ray_intake<false>, k_ray_intake_stream, rj);
                      },
                      [&](uint32_t first, uint32_t last) {
                          hipLaunchKernelGGL(k_ray_finish, dim3((rj.n + kBlock - 1) / kBlock), dim3(kBlock), 0, ir.st, ir.rc, rj, first, last, inv);
                      });
        }
        if (!dev && want_hits) HIP_CHECK(hipMemcpyAsync(job->hits_out, sc->ray_hits.p, (size_t)n_rays * sizeof(spt_hit), hipMemcpyDeviceToHost, ir.st));
        ir.deliver_out(dev, job->rgb_out, (size_t)n_rays * 3);
        return SPT_OK;
    });
}

// ---- first-hit surface records along caller rays (spt_gbuffer): spt_radiance's intake for the hits, then k_gbuffer (gbuffer_kernels.h) ----
spt_status spt_gbuffer(const spt_scene* scene_c, const spt_gbuffer_job* job) {
    if (!scene_c || !job) { g_error = "gbuffer: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < sizeof(spt_gbuffer_job)) { g_error = "gbuffer: job->size is below sizeof(spt_gbuffer_job)"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)SPT_GBUFFER_DEVICE_POINTERS) { g_error = "gbuffer: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if (job->n_rays != 0 && (!job->rays || !job->out)) { g_error = "gbuffer: null rays or out"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {
        if (!sc->fwd->gbuffer) { g_error = "gbuffer: libspt_hip_bez.so does not export spt_gbuffer"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->gbuffer(sc->inner, job));
    }
    if (job->n_rays == 0) return SPT_OK;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("gbuffer", [&] {
        const uint64_t n_rays = job->n_rays;
        const bool dev = (job->flags & SPT_GBUFFER_DEVICE_POINTERS) != 0;
        if (n_rays > (1ull << 40)) fail(SPT_ERR_UNSUPPORTED, "gbuffer: more than 2^40 rays");
        HIP_CHECK(hipSetDevice(sc->device));
        if (dev) {   // every check comes before the first allocation, copy or launch
            const auto check = [&](const void* p, const char* what) { check_device_pointer(sc, "gbuffer", "SPT_GBUFFER_DEVICE_POINTERS", p, what, true); };
            check(job->rays, "rays");
            if (job->aux) check(job->aux, "aux");
            check(job->out, "out");
        }
        ItemRun ir(sc, "gbuffer", 0u, 0u, 1u);   // max_depth 0: no path runs, nothing is random; the intake reports the hits
        const bool use_aux = job->aux != nullptr && sc->textured;   // auxiliary rays are read by the textured instances only
        ir.cut(n_rays, 1u, job->rays_per_pass, "rays_per_pass", 0u);
        const uint32_t P = ir.P;
        sc->ray_hits.ensure((size_t)P * sizeof(spt_hit));   // the hits of a pass, between the two kernels
        float4* out_dev = reinterpret_cast<float4*>(job->out);
        if (!dev)
            out_dev = reinterpret_cast<float4*>(
                ir.stage_buffers((size_t)P * sizeof(spt_path_ray), use_aux ? (size_t)P * sizeof(spt_ray_aux) : 0, (size_t)n_rays * sizeof(spt_gbuffer_rec)));
        // the instance, as bounce() chooses k_shade_albedo's
        const bool pndf = sc->textured && sc->subsurface && sc->has_pndf;
        void (*const fn)(DScene, GBufferJob) = pndf ? k_gbuffer<true, true> : sc->textured ? k_gbuffer<true, false> : k_gbuffer<false, false>;
        uint64_t pass = 0;
        for (uint64_t r0 = 0; r0 < n_rays; r0 += P, ++pass) {
            RayJob rj{};
            rj.n = (uint32_t)std::min<uint64_t>(P, n_rays - r0);
            rj.rays = reinterpret_cast<const float4*>(job->rays + r0);
            rj.hits_out = sc->ray_hits.as<spt_hit>();
            const float4* aux_dev = use_aux ? reinterpret_cast<const float4*>(job->aux + r0) : nullptr;
            if (!dev) {   // the host checks the rays while it copies them
                ir.stage_rays(pass, r0, rj.n, job->rays, use_aux ? job->aux : nullptr);
                rj.rays = sc->ray_in.as<float4>();
                if (use_aux) aux_dev = sc->ray_aux_in.as<float4>();
            }
            const GBufferJob gj{rj.rays, rj.hits_out, aux_dev, out_dev + 4u * r0, rj.n};
            // (one chunk of no samples: chunks() leaves rj.reps == 0, so the intake files no path and writes the hits only)
            ir.chunks(rj.n, rj.k_first, rj.reps, nullptr,
                      [&](bool) { ir.launch_intake(k_ray_intake<true>, k_ray_intake<false>, k_ray_intake_stream, rj); },
                      [&](uint32_t, uint32_t) { hipLaunchKernelGGL(fn, dim3((gj.n + kBlock - 1) / kBlock), dim3(kBlock), 0, ir.st, sc->d, gj); });
        }
        ir.deliver_out(dev, reinterpret_cast<float*>(job->out), (size_t)n_rays * (sizeof(spt_gbuffer_rec) / sizeof(float)));
        return SPT_OK;
    });
}

// ---- camera rays and first-hit images made on the device (spt_camera_rays, spt_camera_gbuffer): camera_device_kernels.h ----
// What spt_host_camera_rays refuses of a model, a plan and a range of its samples, and the sizes the kernels' 32-bit indices bound;
// returns the job's rays
static uint64_t check_camera_plan(const char* who, const spt_camera_model* model, const spt_render_params* plan, uint32_t first, uint32_t count) {
    const std::string w(who);
    if (!plan) fail(SPT_ERR_INVALID_ARG, w + ": null plan");
    if (const char* why = spt_cm_check(model)) fail(SPT_ERR_INVALID_ARG, w + ": " + why);
    const spt_render_params& p = *plan;
    if (p.width == 0 || p.height == 0 || p.spp == 0 || p.sampler > SPT_SAMPLER_RECURRENCE || (uint64_t)first + count > p.spp)
        fail(SPT_ERR_INVALID_ARG, w + ": bad plan (width, height, spp > 0, a known sampler) or samples past the plan's spp");
    if (p.sampler == SPT_SAMPLER_JITTERED && (p.division_x == 0 || p.division_y == 0)) fail(SPT_ERR_INVALID_ARG, w + ": jittered sampler without divisions");
    const uint64_t n_pix = (uint64_t)p.width * p.height;
    if (n_pix > (1ull << 31)) fail(SPT_ERR_UNSUPPORTED, w + ": more than 2^31 pixels");
    if (n_pix * count > (1ull << 40)) fail(SPT_ERR_UNSUPPORTED, w + ": more than 2^40 rays");
    return n_pix * count;
}

// k_camera_rays over the n rays of the job from ray r0 on, into `rays` and `aux` (or null)
static void launch_camera_rays(const RenderCtx& rc, const spt_camera_model& model, uint32_t first, uint64_t r0, uint32_t n, float4* rays, float4* aux,
                               hipStream_t st) {
    CamRaysJob cj{};
    cj.model = model;
    cj.plan = spt_cm_plan_make(&model, rc.width, rc.height);
    cj.rays = rays;
    cj.aux = aux;
    cj.n = n;
    cj.p0 = (uint32_t)(r0 % rc.n_pixels);
    cj.s0 = first + (uint32_t)(r0 / rc.n_pixels);
    hipLaunchKernelGGL(k_camera_rays, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, rc, cj);
    HIP_CHECK(hipGetLastError());
}

spt_status spt_camera_rays(const spt_scene* scene_c, const spt_camera_rays_job* job) {
    if (!scene_c || !job) { g_error = "camera_rays: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < sizeof(spt_camera_rays_job)) { g_error = "camera_rays: job->size is below sizeof(spt_camera_rays_job)"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)SPT_CAMERA_RAYS_DEVICE_POINTERS) { g_error = "camera_rays: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if (job->count != 0 && !job->rays) { g_error = "camera_rays: null rays"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {
        if (!sc->fwd->camera_rays) { g_error = "camera_rays: libspt_hip_bez.so does not export spt_camera_rays"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->camera_rays(sc->inner, job));
    }
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("camera_rays", [&] {
        const uint64_t n_rays = check_camera_plan("camera_rays", job->model, job->plan, job->first, job->count);
        if (n_rays == 0) return SPT_OK;
        const bool dev = (job->flags & SPT_CAMERA_RAYS_DEVICE_POINTERS) != 0;
        HIP_CHECK(hipSetDevice(sc->device));
        if (dev) {   // every check comes before the first allocation, copy or launch
            check_device_pointer(sc, "camera_rays", "SPT_CAMERA_RAYS_DEVICE_POINTERS", job->rays, "rays", true);
            if (job->aux) check_device_pointer(sc, "camera_rays", "SPT_CAMERA_RAYS_DEVICE_POINTERS", job->aux, "aux", true);
        }
        film_join(sc);
        const hipStream_t st = sc->stream;
        const spt_render_params& p = *job->plan;
        const RenderCtx rc = plan_ctx(p, job->model->base, 0u, p.height, 0u, 1u, 1u);
        // passes of around 2^22 rays; below 2^30, so that a pass' pixel indices stay below 2^32 (camera_device_kernels.h)
        const uint32_t P = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(job->rays_per_pass ? job->rays_per_pass : 1u << 22, 1u << 30), n_rays);
        if (!dev) {
            sc->ray_in.ensure((size_t)P * sizeof(spt_path_ray));
            if (job->aux) sc->ray_aux_in.ensure((size_t)P * sizeof(spt_ray_aux));
        }
        for (uint64_t r0 = 0; r0 < n_rays; r0 += P) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(P, n_rays - r0);
            float4* const rays_dev = dev ? reinterpret_cast<float4*>(job->rays + r0) : sc->ray_in.as<float4>();
            float4* const aux_dev = !job->aux ? nullptr : dev ? reinterpret_cast<float4*>(job->aux + r0) : sc->ray_aux_in.as<float4>();
            launch_camera_rays(rc, *job->model, job->first, r0, n, rays_dev, aux_dev, st);
            if (!dev) {
                HIP_CHECK(hipMemcpyAsync(job->rays + r0, rays_dev, (size_t)n * sizeof(spt_path_ray), hipMemcpyDeviceToHost, st));
                if (job->aux) HIP_CHECK(hipMemcpyAsync(job->aux + r0, aux_dev, (size_t)n * sizeof(spt_ray_aux), hipMemcpyDeviceToHost, st));
            }
        }
        HIP_CHECK(hipStreamSynchronize(st));
        return SPT_OK;
    });
}

// The staged form: per pass k_camera_rays into the workspace, spt_gbuffer's intake for the hits, k_gbuffer_image into the per-pixel
// sums; k_gbuffer_image_finish behind the last pass
spt_status spt_camera_gbuffer(const spt_scene* scene_c, const spt_camera_gbuffer_job* job) {
    if (!scene_c || !job) { g_error = "camera_gbuffer: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < sizeof(spt_camera_gbuffer_job)) { g_error = "camera_gbuffer: job->size is below sizeof(spt_camera_gbuffer_job)"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)SPT_CAMERA_GBUFFER_DEVICE_POINTERS) { g_error = "camera_gbuffer: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if (!job->albedo && !job->normal && !job->depth && !job->coverage) { g_error = "camera_gbuffer: no image is asked for"; return SPT_ERR_INVALID_ARG; }
    if (job->count == 0) { g_error = "camera_gbuffer: count must be >= 1"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {
        if (!sc->fwd->camera_gbuffer) { g_error = "camera_gbuffer: libspt_hip_bez.so does not export spt_camera_gbuffer"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->camera_gbuffer(sc->inner, job));
    }
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("camera_gbuffer", [&] {
        const uint64_t n_rays = check_camera_plan("camera_gbuffer", job->model, job->plan, job->first, job->count);
        const bool dev = (job->flags & SPT_CAMERA_GBUFFER_DEVICE_POINTERS) != 0;
        HIP_CHECK(hipSetDevice(sc->device));
        if (dev) {   // every check comes before the first allocation, copy or launch
            const auto check = [&](const void* ptr, const char* what) {
                if (ptr) check_device_pointer(sc, "camera_gbuffer", "SPT_CAMERA_GBUFFER_DEVICE_POINTERS", ptr, what, false);
            };
            check(job->albedo, "albedo");
            check(job->normal, "normal");
            check(job->depth, "depth");
            check(job->coverage, "coverage");
        }
        const spt_render_params& p = *job->plan;
        const uint32_t n_pix = p.width * p.height;
        ItemRun ir(sc, "camera_gbuffer", 0u, 0u, 1u);   // max_depth 0: no path runs, nothing is random; the intake reports the hits
        const RenderCtx cam_rc = plan_ctx(p, job->model->base, 0u, p.height, 0u, 1u, 1u);
        ir.cut(n_rays, 1u, job->rays_per_pass, "rays_per_pass", 0u);   // (P < 2^31, as camera_device_kernels.h wants it)
        const uint32_t P = ir.P;
        const bool use_aux = sc->textured;   // auxiliary rays are read by the textured instances only
        sc->ray_in.ensure((size_t)P * sizeof(spt_path_ray));
        if (use_aux) sc->ray_aux_in.ensure((size_t)P * sizeof(spt_ray_aux));
        sc->ray_hits.ensure((size_t)P * sizeof(spt_hit));
        // the sums, 8 words per pixel, and behind them - host pointers - the four images, 8 floats per pixel together
        const size_t sums_bytes = (size_t)n_pix * 2 * sizeof(float4);
        sc->ray_rgb.ensure(sums_bytes + (dev ? 0 : (size_t)n_pix * 8 * sizeof(float)));
        float4* const sums = sc->ray_rgb.as<float4>();
        HIP_CHECK(hipMemsetAsync(sums, 0, sums_bytes, ir.st));
        float4* const rays_dev = sc->ray_in.as<float4>();
        float4* const aux_dev = use_aux ? sc->ray_aux_in.as<float4>() : nullptr;
        // the instance, as spt_gbuffer chooses k_gbuffer's
        const bool pndf = sc->textured && sc->subsurface && sc->has_pndf;
        void (*const fn)(DScene, GBufferImageJob) = pndf ? k_gbuffer_image<true, true> : sc->textured ? k_gbuffer_image<true, false> : k_gbuffer_image<false, false>;
        for (uint64_t r0 = 0; r0 < n_rays; r0 += P) {
            RayJob rj{};
            rj.n = (uint32_t)std::min<uint64_t>(P, n_rays - r0);
            rj.rays = rays_dev;
            rj.hits_out = sc->ray_hits.as<spt_hit>();
            launch_camera_rays(cam_rc, *job->model, job->first, r0, rj.n, rays_dev, aux_dev, ir.st);
            const GBufferImageJob gj{rays_dev, rj.hits_out, aux_dev, sums, rj.n, (uint32_t)(r0 % n_pix), n_pix};
            const uint32_t lanes = std::min(gj.n, n_pix);
            // (one chunk of no samples: chunks() leaves rj.reps == 0, so the intake files no path and writes the hits only)
            ir.chunks(rj.n, rj.k_first, rj.reps, nullptr,
                      [&](bool) { ir.launch_intake(k_ray_intake<true>, k_ray_intake<false>, k_ray_intake_stream, rj); },
                      [&](uint32_t, uint32_t) { hipLaunchKernelGGL(fn, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, ir.st, sc->d, gj); });
        }
        GBufferImageOut go{};
        go.sums = sums;
        go.n_pixels = n_pix;
        go.count = (float)job->count;
        go.inv = 1.0f / (float)job->count;
        float* const images = reinterpret_cast<float*>(sc->ray_rgb.as<char>() + sums_bytes);
        go.albedo = !job->albedo ? nullptr : dev ? job->albedo : images;
        go.normal = !job->normal ? nullptr : dev ? job->normal : images + 3 * (size_t)n_pix;
        go.depth = !job->depth ? nullptr : dev ? job->depth : images + 6 * (size_t)n_pix;
        go.coverage = !job->coverage ? nullptr : dev ? job->coverage : images + 7 * (size_t)n_pix;
        hipLaunchKernelGGL(k_gbuffer_image_finish, dim3((n_pix + kBlock - 1) / kBlock), dim3(kBlock), 0, ir.st, go);
        HIP_CHECK(hipGetLastError());
        if (!dev) {
            const auto copy_out = [&](float* to, const float* from, size_t floats) {
                if (to) HIP_CHECK(hipMemcpyAsync(to, from, floats * sizeof(float), hipMemcpyDeviceToHost, ir.st));
            };
            copy_out(job->albedo, go.albedo, 3 * (size_t)n_pix);
            copy_out(job->normal, go.normal, 3 * (size_t)n_pix);
            copy_out(job->depth, go.depth, n_pix);
            copy_out(job->coverage, go.coverage, n_pix);
        }
        HIP_CHECK(hipStreamSynchronize(ir.st));
        return SPT_OK;
    });
}

// A host list of spt_bake's points (spt_bake, spt_ao) is checked as a whole, so that a refusal has written nothing at all.
// SURFACE points are checked against the scene's CURRENT tables: the instance records as the device holds them behind the
// updates queued so far (read back as spt_trace_* read their results back), the meshes' ranges from the creation
static void check_host_points(spt_scene* sc, const char* who, bool world, const void* points, uint64_t n_points) {
    const SceneFixed& fx = sc->fixed;
    std::vector<spt_instance> inst_tab(world ? 0 : fx.n_instances);
    std::vector<spt_mesh> mesh_tab(fx.n_meshes);
    for (uint32_t m = 0; m < fx.n_meshes; ++m) mesh_tab[m] = spt_mesh{0u, 0u, fx.mesh_first[m], fx.mesh_tris[m]};
    if (!inst_tab.empty()) {
        film_join(sc);
        HIP_CHECK(hipMemcpyAsync(inst_tab.data(), sc->instances.p, inst_tab.size() * sizeof(spt_instance), hipMemcpyDeviceToHost, sc->stream));
        HIP_CHECK(hipStreamSynchronize(sc->stream));
    }
    const uint32_t n_inst = (uint32_t)inst_tab.size(), n_mesh = fx.n_meshes;
    const uint32_t* const inst_words = inst_tab.empty() ? nullptr : &inst_tab[0].prim_type;
    for (uint64_t i = 0; i < n_points; ++i) {
        const bool ok = world ? spt_bake_world_ok(static_cast<const spt_bake_world_point*>(points) + i)
                              : spt_bake_point_ok(static_cast<const spt_bake_point*>(points) + i, n_inst, inst_words, (uint32_t)(sizeof(spt_instance) / sizeof(uint32_t)), n_mesh, mesh_tab.data());
        if (!ok)
            fail(SPT_ERR_INVALID_ARG, std::string(who) + ": point " + std::to_string(i) +
                                          (world ? " has a non-finite p or n or an all-zero n"
                                                 : " does not name a triangle of a mesh instance (instance, prim) or has a non-finite v or w"));
    }
}

// ---- irradiance at surface points (spt_bake): the rays are made by the intake kernel (bake_kernels.h) ----
spt_status spt_bake(const spt_scene* scene_c, const spt_bake_job* job) {
    if (!scene_c || !job) { g_error = "bake: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < sizeof(spt_bake_job)) { g_error = "bake: job->size is below sizeof(spt_bake_job)"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)(SPT_BAKE_DEVICE_POINTERS | SPT_BAKE_FLIP)) { g_error = "bake: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if (job->kind > SPT_BAKE_POINTS_WORLD) { g_error = "bake: unknown kind of points"; return SPT_ERR_INVALID_ARG; }
    if (job->samples == 0) { g_error = "bake: samples must be >= 1"; return SPT_ERR_INVALID_ARG; }
    if (job->n_points != 0 && (!job->points || !job->rgb_out)) { g_error = "bake: null points or rgb_out"; return SPT_ERR_INVALID_ARG; }
    if (job->max_depth > 255) { g_error = "bake: max_depth > 255"; return SPT_ERR_UNSUPPORTED; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {
        if (!sc->fwd->bake) { g_error = "bake: libspt_hip_bez.so does not export spt_bake"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->bake(sc->inner, job));
    }
    if (job->n_points == 0) return SPT_OK;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("bake", [&] {
        const uint64_t n_points = job->n_points;
        const uint32_t S = job->samples;
        const bool dev = (job->flags & SPT_BAKE_DEVICE_POINTERS) != 0;
        const bool world = job->kind == SPT_BAKE_POINTS_WORLD;
        const size_t rec_bytes = world ? sizeof(spt_bake_world_point) : sizeof(spt_bake_point);
        if (n_points > (1ull << 40)) fail(SPT_ERR_UNSUPPORTED, "bake: more than 2^40 points");
        HIP_CHECK(hipSetDevice(sc->device));
        if (dev) {   // every check comes before the first allocation, copy or launch
            check_device_pointer(sc, "bake", "SPT_BAKE_DEVICE_POINTERS", job->points, "points", true);
            check_device_pointer(sc, "bake", "SPT_BAKE_DEVICE_POINTERS", job->rgb_out, "rgb_out", false);
        } else {     // ... and a host list is checked as a whole (check_host_points)
            check_host_points(sc, "bake", world, job->points, n_points);
        }
        ItemRun ir(sc, "bake", job->max_depth, job->seed, S);
        // max_depth 0: no path runs and out = D; the intake still sums the delta lights
        ir.cut(n_points, S, job->points_per_pass, "points_per_pass", job->max_depth ? S : 0u);
        const uint32_t P = ir.P;
        sc->ray_hits.ensure((size_t)P * 4 * sizeof(float));   // D and validity per point of a pass, 4 planes (bake_kernels.h): spt_radiance's hit buffer, idle here
        float* rgb_dev = job->rgb_out;
        if (!dev) rgb_dev = ir.stage_buffers((size_t)P * rec_bytes, 0, (size_t)n_points * 3 * sizeof(float));
        const float inv = 1.0f / (float)S;
        uint64_t pass = 0;
        for (uint64_t r0 = 0; r0 < n_points; r0 += P, ++pass) {
            BakeJob bj{};
            bj.seed = job->seed;
            bj.n = (uint32_t)std::min<uint64_t>(P, n_points - r0);
            bj.rgb_out = rgb_dev + 3 * r0;
            bj.d_planes = sc->ray_hits.as<float>();
            bj.stream_a = job->first_point + (uint32_t)r0;   // (u32 wrap)
            bj.stream_b = job->first_sample;
            bj.kind = job->kind;
            bj.flip = (job->flags & SPT_BAKE_FLIP) ? 1u : 0u;
            const char* const src = static_cast<const char*>(job->points) + r0 * rec_bytes;
            bj.points = reinterpret_cast<const float4*>(src);
            if (!dev) {
                ir.stage(pass, (size_t)bj.n * rec_bytes, 0, [&](char* records, char*) { std::memcpy(records, src, (size_t)bj.n * rec_bytes); });
                bj.points = sc->ray_in.as<float4>();
            }
            // (chunks() writes bj.k_first and bj.reps before each call of the two lambdas, which launch with bj as it then stands)
            ir.chunks(bj.n, bj.k_first, bj.reps, nullptr, [&](bool) { ir.launch_intake(k_bake_intake<true>, k_bake_intake<false>, k_bake_intake_stream, bj); },
                      [&](uint32_t first, uint32_t last) {
                          hipLaunchKernelGGL(k_bake_finish, dim3((bj.n + kBlock - 1) / kBlock), dim3(kBlock), 0, ir.st, ir.rc, bj, first, last, inv);
                      });
        }
        ir.deliver_out(dev, job->rgb_out, (size_t)n_points * 3);
        return SPT_OK;
    });
}

// ---- visibility along caller rays and at surface points (spt_occluded, spt_ao): any-hit walks, visibility_kernels.h ----
// Both use an ItemRun for the join with the films, the stream, the staging slots and the delivery, and never cut(): no queue, counter or
// radiance slot of the render workspace is sized or touched.

// one of an entry's three kernels, chosen as spt_trace_any chooses its walker
extern "C++" {   // (a template, inside the file's extern "C" block: as ItemRun)
template <class Job>
static void launch_visibility(spt_scene* sc, hipStream_t st, void (*lds)(DScene, Job), void (*mem)(DScene, Job), void (*streaming)(DScene, Job), const Job& job) {
    const bool stream = sc->swalk && !sc->lds_geo;
    hipLaunchKernelGGL(stream ? streaming : sc->lds_geo ? lds : mem, dim3((job.n + kBlock - 1) / kBlock), dim3(kBlock), sc->lds_bytes, st, sc->d, job);
    HIP_CHECK(hipGetLastError());
}
}

spt_status spt_occluded(const spt_scene* scene_c, const spt_occluded_job* job) {
    if (!scene_c || !job) { g_error = "occluded: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < sizeof(spt_occluded_job)) { g_error = "occluded: job->size is below sizeof(spt_occluded_job)"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)(SPT_OCCLUDED_DEVICE_POINTERS | SPT_OCCLUDED_PACKED)) { g_error = "occluded: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if (job->n_rays != 0 && (!job->rays || !job->out)) { g_error = "occluded: null rays or out"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {
        if (!sc->fwd->occluded) { g_error = "occluded: libspt_hip_bez.so does not export spt_occluded"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->occluded(sc->inner, job));
    }
    if (job->n_rays == 0) return SPT_OK;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("occluded", [&] {
        const uint64_t n_rays = job->n_rays;
        const bool dev = (job->flags & SPT_OCCLUDED_DEVICE_POINTERS) != 0;
        const bool packed = (job->flags & SPT_OCCLUDED_PACKED) != 0;
        if (n_rays > (1ull << 40)) fail(SPT_ERR_UNSUPPORTED, "occluded: more than 2^40 rays");
        HIP_CHECK(hipSetDevice(sc->device));
        if (dev) {   // every check comes before the first allocation, copy or launch
            check_device_pointer_aligned(sc, "occluded", "SPT_OCCLUDED_DEVICE_POINTERS", job->rays, "rays", 16u);
            check_device_pointer_aligned(sc, "occluded", "SPT_OCCLUDED_DEVICE_POINTERS", job->out, "out", packed ? 8u : 1u);
        }
        ItemRun ir(sc, "occluded", 0u, 0u, 1u);
        // Passes of 2^20 rays by default where they are staged (the host fills one slot beside the copy and the walk of the other), of 2^30
        // behind device pointers: every launch ends in a tail of its longest walks, and nothing is gained by cutting (16 launches of 2^20
        // rays took 11.4 ms on the million-triangle grid where one launch takes 6.1, profiles/visibility_cost.json).  A PACKED pass begins
        // at a word of its own
        uint64_t P64 = std::min<uint64_t>(job->rays_per_pass ? job->rays_per_pass : dev ? (1u << 30) : (1u << 20), n_rays);
        if (packed) P64 = (P64 + 63u) / 64u * 64u;
        const uint32_t P = (uint32_t)P64;
        const size_t out_bytes = packed ? (size_t)((n_rays + 63u) / 64u) * sizeof(uint64_t) : (size_t)n_rays;
        char* out_dev = static_cast<char*>(job->out);
        if (!dev) out_dev = reinterpret_cast<char*>(ir.stage_buffers((size_t)P * sizeof(spt_ray), 0, out_bytes));
        uint64_t pass = 0;
        for (uint64_t r0 = 0; r0 < n_rays; r0 += P, ++pass) {
            OccludedJob oj{};
            oj.n = (uint32_t)std::min<uint64_t>(P, n_rays - r0);
            oj.packed = packed ? 1u : 0u;
            oj.rays = reinterpret_cast<const float4*>(job->rays + r0);
            oj.out = out_dev + (packed ? r0 / 64u * sizeof(uint64_t) : r0);
            if (!dev) {   // the host checks the rays while it copies them
                ir.stage(pass, (size_t)oj.n * sizeof(spt_ray), 0, [&](char* records, char*) {
                    spt_ray* const dst = reinterpret_cast<spt_ray*>(records);
                    const spt_ray* const src = job->rays + r0;
                    for (uint32_t i = 0; i < oj.n; ++i) {
                        const spt_ray& r = src[i];
                        const bool finite = std::isfinite(r.o[0]) && std::isfinite(r.o[1]) && std::isfinite(r.o[2]) && std::isfinite(r.d[0]) &&
                                            std::isfinite(r.d[1]) && std::isfinite(r.d[2]) && std::isfinite(r.t_min);
                        const bool zero = r.d[0] == 0.0f && r.d[1] == 0.0f && r.d[2] == 0.0f;
                        if (!finite || zero || std::isnan(r.t_max)) {
                            HIP_CHECK(hipStreamSynchronize(ir.st));   // the earlier passes wrote the library's own buffers only
                            fail(SPT_ERR_INVALID_ARG, "occluded: ray " + std::to_string(r0 + i) +
                                                          (!finite ? " has a non-finite o, d or t_min" : zero ? " has an all-zero direction" : " has a NaN t_max"));
                        }
                        dst[i] = r;
                    }
                });
                oj.rays = sc->ray_in.as<float4>();
            }
            launch_visibility(sc, ir.st, k_occluded<true>, k_occluded<false>, k_occluded_stream, oj);
        }
        if (!dev) HIP_CHECK(hipMemcpyAsync(job->out, sc->ray_rgb.p, out_bytes, hipMemcpyDeviceToHost, ir.st));
        HIP_CHECK(hipStreamSynchronize(ir.st));
        return SPT_OK;
    });
}

// ---- all hits along caller rays (spt_hits): the K nearest crossings and the crossing counts, hits_kernels.h ----
// As spt_occluded: an ItemRun without cut(), the two staging slots, one lane per ray.  The results of a host call stay in
// sc->ray_rgb, [records | counts], until the last pass is done, so a ray refused in a later pass leaves the caller's memory as it was.
spt_status spt_hits(const spt_scene* scene_c, const spt_hits_job* job) {
    if (!scene_c || !job) { g_error = "hits: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < sizeof(spt_hits_job)) { g_error = "hits: job->size is below sizeof(spt_hits_job)"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)(SPT_HITS_DEVICE_POINTERS | SPT_HITS_COUNT_ALL)) { g_error = "hits: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if (job->max_hits > 64u) { g_error = "hits: max_hits must be in 0 .. 64"; return SPT_ERR_INVALID_ARG; }
    if (job->max_hits == 0u && !(job->flags & SPT_HITS_COUNT_ALL)) { g_error = "hits: max_hits == 0 needs SPT_HITS_COUNT_ALL"; return SPT_ERR_INVALID_ARG; }
    if (job->n_rays != 0 && (!job->rays || !job->counts)) { g_error = "hits: null rays or counts"; return SPT_ERR_INVALID_ARG; }
    if (job->n_rays != 0 && job->max_hits != 0u && !job->hits) { g_error = "hits: null hits with max_hits > 0"; return SPT_ERR_INVALID_ARG; }
#if SPT_WITH_BEZIER
    // (this library serves the scenes with patch instances, and compiles no k_hits)
    g_error = "hits: scenes with Bezier patches are not supported: the patch test yields one root by construction";
    return SPT_ERR_UNSUPPORTED;
#else
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {   // not forwarded: there is nothing libspt_hip_bez.so could answer
        g_error = "hits: the scene has Bezier-patch instances (Catmull-Clark surfaces included), which are not supported: the patch test yields one root by construction, "
                  "so the crossings behind it are not defined";
        return SPT_ERR_UNSUPPORTED;
    }
    if (job->n_rays == 0) return SPT_OK;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("hits", [&] {
        const uint64_t n_rays = job->n_rays;
        const uint32_t K = job->max_hits;
        const bool dev = (job->flags & SPT_HITS_DEVICE_POINTERS) != 0;
        const bool all = (job->flags & SPT_HITS_COUNT_ALL) != 0;
        if (n_rays > (1ull << 40)) fail(SPT_ERR_UNSUPPORTED, "hits: more than 2^40 rays");
        HIP_CHECK(hipSetDevice(sc->device));
        if (dev) {   // every check comes before the first allocation, copy or launch
            check_device_pointer_aligned(sc, "hits", "SPT_HITS_DEVICE_POINTERS", job->rays, "rays", 16u);
            if (K) check_device_pointer_aligned(sc, "hits", "SPT_HITS_DEVICE_POINTERS", job->hits, "hits", 16u);
            check_device_pointer_aligned(sc, "hits", "SPT_HITS_DEVICE_POINTERS", job->counts, "counts", 8u);
        }
        ItemRun ir(sc, "hits", 0u, 0u, 1u);
        // Passes as spt_occluded cuts them: 2^30 rays behind device pointers (a lane's index and its max_hits records stay below
        // 2^32 and are addressed in 64 bits), and where the rays are staged as many as write the 32 MiB of a default slot, 2^20 at most
        const size_t per_ray = (size_t)K * sizeof(spt_hit_rec) + sizeof(spt_hit_count);
        const uint64_t staged = std::max<uint64_t>(1u, std::min<uint64_t>(1u << 20, ((size_t)32 << 20) / per_ray));
        const uint32_t P = (uint32_t)std::min<uint64_t>(job->rays_per_pass ? job->rays_per_pass : dev ? (1u << 30) : staged, n_rays);
        const size_t hits_bytes = (size_t)n_rays * K * sizeof(spt_hit_rec), counts_bytes = (size_t)n_rays * sizeof(spt_hit_count);
        spt_hit_rec* hits_dev = job->hits;
        spt_hit_count* counts_dev = job->counts;
        if (!dev) {
            char* const out = reinterpret_cast<char*>(ir.stage_buffers((size_t)P * sizeof(spt_ray), 0, hits_bytes + counts_bytes));
            hits_dev = reinterpret_cast<spt_hit_rec*>(out);
            counts_dev = reinterpret_cast<spt_hit_count*>(out + hits_bytes);   // (a multiple of 32 bytes behind an aligned allocation)
        }
        uint64_t pass = 0;
        for (uint64_t r0 = 0; r0 < n_rays; r0 += P, ++pass) {
            HitsJob hj{};
            hj.n = (uint32_t)std::min<uint64_t>(P, n_rays - r0);
            hj.max_hits = K;
            hj.rays = reinterpret_cast<const float4*>(job->rays + r0);
            hj.hits = reinterpret_cast<float4*>(hits_dev + (K ? r0 * K : 0u));
            hj.counts = reinterpret_cast<uint2*>(counts_dev + r0);
            if (!dev) {   // the host checks the rays while it copies them
                ir.stage(pass, (size_t)hj.n * sizeof(spt_ray), 0, [&](char* records, char*) {
                    spt_ray* const dst = reinterpret_cast<spt_ray*>(records);
                    const spt_ray* const src = job->rays + r0;
                    for (uint32_t i = 0; i < hj.n; ++i) {
                        const spt_ray& r = src[i];
                        const bool finite = std::isfinite(r.o[0]) && std::isfinite(r.o[1]) && std::isfinite(r.o[2]) && std::isfinite(r.d[0]) &&
                                            std::isfinite(r.d[1]) && std::isfinite(r.d[2]) && std::isfinite(r.t_min);
                        const bool zero = r.d[0] == 0.0f && r.d[1] == 0.0f && r.d[2] == 0.0f;
                        if (!finite || zero || std::isnan(r.t_max)) {
                            HIP_CHECK(hipStreamSynchronize(ir.st));   // the earlier passes wrote the library's own buffers only
                            fail(SPT_ERR_INVALID_ARG, "hits: ray " + std::to_string(r0 + i) +
                                                          (!finite ? " has a non-finite o, d or t_min" : zero ? " has an all-zero direction" : " has a NaN t_max"));
                        }
                        dst[i] = r;
                    }
                });
                hj.rays = sc->ray_in.as<float4>();
            }
            void (*const kernel)(DScene, HitsJob) = sc->lds_geo ? (all ? k_hits<true, true> : k_hits<true, false>) : (all ? k_hits<false, true> : k_hits<false, false>);
            hipLaunchKernelGGL(kernel, dim3((hj.n + kBlock - 1) / kBlock), dim3(kBlock), sc->lds_bytes, ir.st, sc->d, hj);
            HIP_CHECK(hipGetLastError());
        }
        if (!dev) {
            if (K) HIP_CHECK(hipMemcpyAsync(job->hits, hits_dev, hits_bytes, hipMemcpyDeviceToHost, ir.st));
            HIP_CHECK(hipMemcpyAsync(job->counts, counts_dev, counts_bytes, hipMemcpyDeviceToHost, ir.st));
        }
        HIP_CHECK(hipStreamSynchronize(ir.st));
        return SPT_OK;
    });
#endif
}

spt_status spt_ao(const spt_scene* scene_c, const spt_ao_job* job) {
    if (!scene_c || !job) { g_error = "ao: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < sizeof(spt_ao_job)) { g_error = "ao: job->size is below sizeof(spt_ao_job)"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)(SPT_AO_DEVICE_POINTERS | SPT_AO_FLIP)) { g_error = "ao: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if (job->kind > SPT_BAKE_POINTS_WORLD) { g_error = "ao: unknown kind of points"; return SPT_ERR_INVALID_ARG; }
    if (job->samples == 0 || job->samples > (1u << 24)) { g_error = "ao: samples must be in 1 .. 2^24"; return SPT_ERR_INVALID_ARG; }
    if (!(job->max_distance > 0.0f)) { g_error = "ao: max_distance must be > 0 (+inf: no limit)"; return SPT_ERR_INVALID_ARG; }
    if (job->n_points != 0 && (!job->points || !job->out)) { g_error = "ao: null points or out"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {
        if (!sc->fwd->ao) { g_error = "ao: libspt_hip_bez.so does not export spt_ao"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->ao(sc->inner, job));
    }
    if (job->n_points == 0) return SPT_OK;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("ao", [&] {
        const uint64_t n_points = job->n_points;
        const uint32_t S = job->samples;
        const bool dev = (job->flags & SPT_AO_DEVICE_POINTERS) != 0;
        const bool world = job->kind == SPT_BAKE_POINTS_WORLD;
        const size_t rec_bytes = world ? sizeof(spt_bake_world_point) : sizeof(spt_bake_point);
        if (n_points > (1ull << 40)) fail(SPT_ERR_UNSUPPORTED, "ao: more than 2^40 points");
        HIP_CHECK(hipSetDevice(sc->device));
        if (dev) {   // every check comes before the first allocation, copy or launch
            check_device_pointer(sc, "ao", "SPT_AO_DEVICE_POINTERS", job->points, "points", true);
            check_device_pointer(sc, "ao", "SPT_AO_DEVICE_POINTERS", job->out, "out", true);
        } else {     // ... and a host list is checked as a whole (check_host_points)
            check_host_points(sc, "ao", world, job->points, n_points);
        }
        ItemRun ir(sc, "ao", 0u, job->seed, S);
        // Passes of 2^20 points by default, and launches of at most R samples: around 2^24 rays each, 16 .. 512 samples.  The chunks
        // behind the first carry sum and count through the out record (k_ao).
        const uint32_t P = (uint32_t)std::min<uint64_t>(job->points_per_pass ? job->points_per_pass : (1u << 20), n_points);
        const uint32_t R = std::min(S, std::max(16u, std::min(512u, (1u << 24) / P)));
        float4* out_dev = reinterpret_cast<float4*>(job->out);
        if (!dev) out_dev = reinterpret_cast<float4*>(ir.stage_buffers((size_t)P * rec_bytes, 0, (size_t)n_points * sizeof(spt_ao_rec)));
        uint64_t pass = 0;
        for (uint64_t r0 = 0; r0 < n_points; r0 += P, ++pass) {
            AoJob aj{};
            aj.seed = job->seed;
            aj.t_max = std::isfinite(job->max_distance) ? job->max_distance : SPT_F32_MAX;
            aj.inv = 1.0f / (float)S;
            aj.n = (uint32_t)std::min<uint64_t>(P, n_points - r0);
            aj.out = out_dev + 2u * r0;
            aj.stream_a = job->first_point + (uint32_t)r0;   // (u32 wrap)
            aj.stream_b = job->first_sample;
            aj.kind = job->kind;
            aj.flip = (job->flags & SPT_AO_FLIP) ? 1u : 0u;
            const char* const src = static_cast<const char*>(job->points) + r0 * rec_bytes;
            aj.points = reinterpret_cast<const float4*>(src);
            if (!dev) {
                ir.stage(pass, (size_t)aj.n * rec_bytes, 0, [&](char* records, char*) { std::memcpy(records, src, (size_t)aj.n * rec_bytes); });
                aj.points = sc->ray_in.as<float4>();
            }
            for (uint32_t k0 = 0; k0 < S; k0 += R) {
                aj.k_first = k0;
                aj.reps = std::min(R, S - k0);
                aj.last = k0 + aj.reps == S ? 1u : 0u;
                launch_visibility(sc, ir.st, k_ao<true>, k_ao<false>, k_ao_stream, aj);
            }
        }
        ir.deliver_out(dev, reinterpret_cast<float*>(job->out), (size_t)n_points * (sizeof(spt_ao_rec) / sizeof(float)));
        return SPT_OK;
    });
}

// ---- spherical-harmonic light probes (spt_probe): uniform sphere rays and a projection behind the bounces (probe_kernels.h) ----
spt_status spt_probe(const spt_scene* scene_c, const spt_probe_job* job) {
    if (!scene_c || !job) { g_error = "probe: null argument"; return SPT_ERR_INVALID_ARG; }
    if (job->size < sizeof(spt_probe_job)) { g_error = "probe: job->size is below sizeof(spt_probe_job)"; return SPT_ERR_INVALID_ARG; }
    if (job->flags & ~(uint32_t)SPT_PROBE_DEVICE_POINTERS) { g_error = "probe: unknown flags"; return SPT_ERR_INVALID_ARG; }
    if (job->samples == 0) { g_error = "probe: samples must be >= 1"; return SPT_ERR_INVALID_ARG; }
    if (job->n_points != 0 && (!job->points || !job->sh_out)) { g_error = "probe: null points or sh_out"; return SPT_ERR_INVALID_ARG; }
    if (job->max_depth > 255) { g_error = "probe: max_depth > 255"; return SPT_ERR_UNSUPPORTED; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) {
        if (!sc->fwd->probe) { g_error = "probe: libspt_hip_bez.so does not export spt_probe"; return SPT_ERR_UNSUPPORTED; }
        return forwarded(sc->fwd, sc->fwd->probe(sc->inner, job));
    }
    if (job->n_points == 0) return SPT_OK;
    std::lock_guard<std::mutex> lock(sc->mu);
    return guarded("probe", [&] {
        const uint64_t n_points = job->n_points;
        const uint32_t S = job->samples;
        const bool dev = (job->flags & SPT_PROBE_DEVICE_POINTERS) != 0;
        const bool want_aux = job->aux_out != nullptr;
        if (n_points > (1ull << 36)) fail(SPT_ERR_UNSUPPORTED, "probe: more than 2^36 probes");
        HIP_CHECK(hipSetDevice(sc->device));
        if (dev) {   // every check comes before the first allocation, copy or launch
            check_device_pointer(sc, "probe", "SPT_PROBE_DEVICE_POINTERS", job->points, "points", true);
            check_device_pointer(sc, "probe", "SPT_PROBE_DEVICE_POINTERS", job->sh_out, "sh_out", false);
            if (want_aux) check_device_pointer(sc, "probe", "SPT_PROBE_DEVICE_POINTERS", job->aux_out, "aux_out", false);
        } else {     // ... and a host list is checked as a whole, so that a refusal has written nothing at all
            for (uint64_t i = 0; i < n_points; ++i)
                if (!spt_probe_ok(job->points + i)) fail(SPT_ERR_INVALID_ARG, "probe: point " + std::to_string(i) + " has a non-finite p");
        }
        ItemRun ir(sc, "probe", job->max_depth, job->seed, S);
        // max_depth 0: no path runs and sh = D; the first segments are still traced when the visibility record is asked for
        ir.cut(n_points, S, job->points_per_pass, "points_per_pass", (job->max_depth || want_aux) ? S : 0u);
        const uint32_t P = ir.P;
        // D, validity and the visibility carry per probe of a pass (kProbePlanes planes of P words), then the first segments of a chunk
        // (R * P words), probe_kernels.h: spt_radiance's hit buffer, idle here
        const size_t seg_cap = (size_t)P * std::max(ir.R, 1u);
        sc->ray_hits.ensure(((size_t)P * kProbePlanes + seg_cap) * sizeof(float));
        float* sh_dev = job->sh_out;
        float* aux_dev = job->aux_out;
        if (!dev) {   // sh for every probe, then aux for every probe
            sh_dev = ir.stage_buffers((size_t)P * sizeof(spt_probe_point), 0, (size_t)n_points * (SPT_PROBE_SH_WORDS + (want_aux ? SPT_PROBE_AUX_WORDS : 0u)) * sizeof(float));
            aux_dev = want_aux ? sh_dev + (size_t)n_points * SPT_PROBE_SH_WORDS : nullptr;
        }
        const float inv = 1.0f / (float)S;
        const float w = spt_probe_weight(S);
        uint64_t pass = 0;
        for (uint64_t r0 = 0; r0 < n_points; r0 += P, ++pass) {
            ProbeJob pj{};
            pj.seed = job->seed;
            pj.n = (uint32_t)std::min<uint64_t>(P, n_points - r0);
            pj.sh_out = sh_dev + SPT_PROBE_SH_WORDS * r0;
            pj.aux_out = aux_dev ? aux_dev + SPT_PROBE_AUX_WORDS * r0 : nullptr;
            pj.planes = sc->ray_hits.as<float>();
            pj.seg = reinterpret_cast<uint32_t*>(sc->ray_hits.as<float>() + (size_t)P * kProbePlanes);
            pj.plane_cap = P;
            pj.seg_cap = (uint32_t)seg_cap;
            pj.stream_a = job->first_point + (uint32_t)r0;   // (u32 wrap)
            pj.stream_b = job->first_sample;
            pj.paths = job->max_depth ? 1u : 0u;
            const spt_probe_point* const src = job->points + r0;
            pj.points = reinterpret_cast<const float4*>(src);
            if (!dev) {
                ir.stage(pass, (size_t)pj.n * sizeof(spt_probe_point), 0, [&](char* records, char*) { std::memcpy(records, src, (size_t)pj.n * sizeof(spt_probe_point)); });
                pj.points = sc->ray_in.as<float4>();
            }
            // (chunks() writes pj.k_first and pj.reps before each call of the two lambdas, which launch with pj as it then stands)
            ir.chunks(pj.n, pj.k_first, pj.reps, nullptr, [&](bool) { ir.launch_intake(k_probe_intake<true>, k_probe_intake<false>, k_probe_intake_stream, pj); },
                      [&](uint32_t first, uint32_t last) {   // a lane per (coefficient, probe)
                          const dim3 grid((uint32_t)(((uint64_t)pj.n * SPT_PROBE_COEFFS + kBlock - 1) / kBlock));
                          hipLaunchKernelGGL(k_probe_finish, grid, dim3(kBlock), 0, ir.st, ir.rc, pj, first, last, w, inv);
                      });
        }
        if (!dev && want_aux) HIP_CHECK(hipMemcpyAsync(job->aux_out, aux_dev, (size_t)n_points * SPT_PROBE_AUX_WORDS * sizeof(float), hipMemcpyDeviceToHost, ir.st));
        ir.deliver_out(dev, job->sh_out, (size_t)n_points * SPT_PROBE_SH_WORDS);
        return SPT_OK;
    });
}

spt_status spt_alloc_pinned(uint64_t bytes, void** out) {
    if (!out || bytes == 0) { g_error = "alloc_pinned: bad argument"; return SPT_ERR_INVALID_ARG; }
    *out = nullptr;
    if (usable_device_count() <= 0) { g_error = "no HIP device is visible: libspt_hip has no CPU fallback"; return SPT_ERR_NO_DEVICE; }
    hipError_t e = hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault);
    if (e != hipSuccess) { g_error = std::string("hipHostMalloc: ") + hipGetErrorString(e); return SPT_ERR_OUT_OF_MEMORY; }
    return SPT_OK;
}
spt_status spt_pin_host(void* p, uint64_t bytes) {
    if (!p || !bytes) { g_error = "pin_host: null argument"; return SPT_ERR_INVALID_ARG; }
    if (usable_device_count() == 0) { g_error = "no HIP device is visible: libspt_hip has no CPU fallback"; return SPT_ERR_NO_DEVICE; }
    if (hipHostRegister(p, (size_t)bytes, hipHostRegisterPortable) != hipSuccess) {
        (void)hipGetLastError();
        g_error = "pin_host: hipHostRegister failed";
        return SPT_ERR_OUT_OF_MEMORY;
    }
    return SPT_OK;
}
void spt_unpin_host(void* p) {
    if (p) (void)hipHostUnregister(p);
}

void spt_free_pinned(void* p) {
    if (p) (void)hipHostFree(p);
}

spt_status spt_debug_detmath(int32_t device, uint32_t fn, uint32_t n, const float* a, const float* b, float* out) {
    if (n && (!a || !b || !out)) { g_error = "debug_detmath: null argument"; return SPT_ERR_INVALID_ARG; }
    if (n == 0) return SPT_OK;
    return guarded("debug_detmath", [&] {
        int nd = usable_device_count();
        if (nd <= 0) fail(SPT_ERR_NO_DEVICE, "no HIP device is visible: libspt_hip has no CPU fallback");
        if (device < 0 || device >= nd) fail(SPT_ERR_NO_DEVICE, "device index out of range");
        HIP_CHECK(hipSetDevice(device));
        DeviceBuffer da, db, dout;
        da.upload(a, n);
        db.upload(b, n);
        dout.alloc((size_t)n * sizeof(float));
        hipLaunchKernelGGL(k_detmath, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, fn, n, da.as<float>(), db.as<float>(), dout.as<float>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out, dout.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        return SPT_OK;
    });
}

spt_status spt_debug_pack_rgb8(int32_t device, uint32_t n, const float* in, uint8_t* out) {
    if (n && (!in || !out)) { g_error = "debug_pack_rgb8: null argument"; return SPT_ERR_INVALID_ARG; }
    if (n == 0) return SPT_OK;
    return guarded("debug_pack_rgb8", [&] {
        if (n > 0xfffffffcu) fail(SPT_ERR_UNSUPPORTED, "debug_pack_rgb8: more than 2^32 - 4 floats");
        int nd = usable_device_count();
        if (nd <= 0) fail(SPT_ERR_NO_DEVICE, "no HIP device is visible: libspt_hip has no CPU fallback");
        if (device < 0 || device >= nd) fail(SPT_ERR_NO_DEVICE, "device index out of range");
        HIP_CHECK(hipSetDevice(device));
        DeviceBuffer din, dout;
        din.upload(in, n);
        dout.alloc(n);
        launch_pack_rgb8(n, din.as<float>(), dout.as<uint8_t>(), 0);
        HIP_CHECK(hipMemcpy(out, dout.p, n, hipMemcpyDeviceToHost));
        return SPT_OK;
    });
}

spt_status spt_debug_render_info(const spt_scene* scene_c, uint32_t what, uint64_t* out) {
    if (!scene_c || !out || what > 8u) { g_error = "debug_render_info: null argument or unknown counter"; return SPT_ERR_INVALID_ARG; }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc->fwd) return forwarded(sc->fwd, sc->fwd->debug_render_info(sc->inner, what, out));
    std::lock_guard<std::mutex> lock(sc->mu);
    if (what == 6u) {   // waits for the last deformation's copies and kernels
        return guarded("debug_render_info", [&] {
            *out = 0;
            if (!sc->deform_timed) return SPT_OK;
            HIP_CHECK(hipSetDevice(sc->device));
            HIP_CHECK(hipEventSynchronize(sc->ev_deform[1]));
            float ms = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&ms, sc->ev_deform[0], sc->ev_deform[1]));
            *out = (uint64_t)((double)ms * 1e6);
            return SPT_OK;
        });
    }
    *out = what == 8u ? sc->passes_cam : what == 7u ? sc->passes_pipe : what == 0u ? sc->passes_film : what == 1u ? sc->passes_single : what == 2u ? sc->keep_read_ns : what == 3u ? sc->frames_direct : what == 4u ? sc->updates : sc->update_bytes;
    return SPT_OK;
}

spt_status spt_debug_bxdf(const spt_scene* scene_c, int32_t device, const spt_material* mt, uint32_t op, uint32_t n, const float* wo,
                          const float* wi_in, const uint64_t* rng_state, float* wi_out, float* f_out, float* pdf_out, int32_t* dir_out) {
    if (!mt || op > 1u || (n && (!wo || !f_out || !pdf_out || (op == 0u ? (!rng_state || !wi_out || !dir_out) : !wi_in)))) {
        g_error = "debug_bxdf: null argument or unknown op";
        return SPT_ERR_INVALID_ARG;
    }
    spt_scene* sc = const_cast<spt_scene*>(scene_c);
    if (sc && sc->fwd)   // a patch scene lives in the other code object
        return forwarded(sc->fwd, sc->fwd->debug_bxdf(sc->inner, device, mt, op, n, wo, wi_in, rng_state, wi_out, f_out, pdf_out, dir_out));
    if (n == 0) return SPT_OK;
    return guarded("debug_bxdf", [&] {
        if (mt->bxdf > SPT_BXDF_PNDF_PLASTIC) fail(SPT_ERR_INVALID_ARG, "debug_bxdf: unknown bxdf");
        if (mt->recipe != 0u) fail(SPT_ERR_INVALID_ARG, "debug_bxdf: the record must be a constant Bxdf (recipe 0)");
        const bool pndf = mt->bxdf == SPT_BXDF_PNDF_CONDUCTOR || mt->bxdf == SPT_BXDF_PNDF_PLASTIC;
        if (pndf && !sc) fail(SPT_ERR_INVALID_ARG, "debug_bxdf: a position-normal-distribution lobe needs the scene that holds its tables");
        if (pndf && (sc->pndfs.bytes == 0 || (size_t)spt_f2u(mt->c1[2]) >= sc->pndfs.bytes / sizeof(spt_pndf))) fail(SPT_ERR_INVALID_ARG, "debug_bxdf: P-NDF index (c1[2]) out of range");
        // the exit point of a Subsurface substrate is a traced probe ray (substrate.rs:231-350): only whole films cover it
        if (mt->substrate == SPT_SUBSTRATE_SUBSURFACE && (mt->bxdf == SPT_BXDF_MICROFACET_PLASTIC || mt->bxdf == SPT_BXDF_SPECULAR_PLASTIC || mt->bxdf == SPT_BXDF_PNDF_PLASTIC))
            fail(SPT_ERR_UNSUPPORTED, "debug_bxdf: the Subsurface substrate samples through a probe ray and has no stand-alone seam");
        if (sc) device = sc->device;
        int nd = usable_device_count();
        if (nd <= 0) fail(SPT_ERR_NO_DEVICE, "no HIP device is visible: libspt_hip has no CPU fallback");
        if (device < 0 || device >= nd) fail(SPT_ERR_NO_DEVICE, "device index out of range");
        HIP_CHECK(hipSetDevice(device));
        DMat m;
        m.bxdf = mt->bxdf;
        m.c0 = f3{mt->c0[0], mt->c0[1], mt->c0[2]};
        m.c1 = f3{mt->c1[0], mt->c1[1], mt->c1[2]};
        m.c2 = f3{mt->c2[0], mt->c2[1], mt->c2[2]};
        m.ax = mt->ax; m.ay = mt->ay; m.ior = mt->ior;
        m.fresnel = mt->fresnel; m.substrate = mt->substrate;
        DeviceBuffer dwo, dwi, drng, dwio, df, dpdf, ddir;
        dwo.upload(wo, (size_t)n * 3);
        if (op == 0u) { drng.upload(rng_state, n); dwio.alloc((size_t)n * 3 * sizeof(float)); ddir.alloc((size_t)n * sizeof(int32_t)); }
        else dwi.upload(wi_in, (size_t)n * 3);
        df.alloc((size_t)n * 3 * sizeof(float));
        dpdf.alloc((size_t)n * sizeof(float));
        const dim3 grid((n + kBlock - 1) / kBlock);
        const auto kernel = pndf ? k_debug_bxdf<true> : k_debug_bxdf<false>;
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, 0, pndf ? sc->d : DScene{}, m, op, n, dwo.as<float>(), dwi.as<float>(), drng.as<uint64_t>(),
                           dwio.as<float>(), df.as<float>(), dpdf.as<float>(), ddir.as<int32_t>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(f_out, df.p, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(pdf_out, dpdf.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        if (op == 0u) {
            HIP_CHECK(hipMemcpy(wi_out, dwio.p, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(dir_out, ddir.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        return SPT_OK;
    });
}

spt_status spt_trace_closest(const spt_scene* scene, uint32_t n, const spt_ray* rays, spt_hit* hits) {
    return trace_common(scene, n, rays, hits, sizeof(spt_hit), true);
}
spt_status spt_trace_any(const spt_scene* scene, uint32_t n, const spt_ray* rays, uint8_t* occluded) {
    return trace_common(scene, n, rays, occluded, 1, false);
}

}  // extern "C"

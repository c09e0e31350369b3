// spt — command-line driver with the reference's flags (reference src/main.rs:26-66):
//   spt -s scene.json -r renderer.json [-w 512] [-h 512] -o out.png [-c camera]
// plus --seed, --spp, --device D | --gpus N (one image over N devices: one worker thread and one scene replica per device,
// interleaved row strips, one film - spt_host_multi_*, the counterpart of the thread fan-out of pt.rs:243-287),
// --strip-rows R, --debug-normal and --bezier-ni (the reference's two cargo features, Cargo.toml:34-36: pt.rs:113-118, bezier.rs:58-103),
// and progressive rendering on one device through a film object (spt_film_*): --preview-every K rewrites the image after every
// K samples, --time-limit SEC stops after the increment during which SEC seconds have passed, --variance-out PATH.exr writes the
// per-pixel variance of the mean, --adaptive REL [--adaptive-floor A] [--adaptive-min-samples N] retires converged pixels after
// every increment (spt_film_adapt) and stops once none is active, --samples-out PATH.exr writes each pixel's sample count,
// --denoise [--denoise-iterations K] [--guide-samples N] [--noisy-out PATH] renders N samples of a first-hit normal film first and
// writes every preview and the final image through the edge-aware filter (spt_film_denoise), the plain mean to PATH;
// --guide normal|albedo|both picks the guide films (albedo: the same plan with SPT_RENDER_AOV_ALBEDO, spt_film_denoise_job),
// --demodulate filters colour / albedo and multiplies the albedo back, --albedo-out PATH writes the albedo film's mean,
// --robust K [--robust-estimator mon|gmon] [--mean-out PATH] keeps K bucket sums per pixel (spt_film_buckets) and writes every preview
// and the final image from their median (mon) or Gini-adaptive trimmed mean (gmon, the default), the plain mean to PATH.  It loads the scene
// with libspt_host, renders with libspt_hip (HIP kernels only) and writes the image; like the reference it reports the
// time spent inside `render`.  The images of a film (previews, the final image, --noisy-out, --mean-out) leave the device as the
// 8-bit image the reference saves (spt_film_read_rgb8: a quarter of the float film's bytes); the EXR outputs stay float.
// --film-devices d0,d1,.. (an index may repeat) runs the same progressive loop over a multi film on those devices (one shard film per
// device, spt_host_multi_film_*; the denoiser runs once on the gathered image, spt_denoise_image) and writes the same bytes.
// --gbuffer-out STEM [--gbuffer-samples N] writes the first-hit images of the camera, or of the camera model of the same command line,
// as float EXR files STEM_albedo.exr, STEM_normal.exr and STEM_depth.exr (R depth, G coverage): one spt_camera_gbuffer call, N plan
// samples averaged, on one device; -o may then be left out.  --gbuffer-host-rays takes the route that call replaces, spt_gbuffer over
// spt_host_camera_rays with the sums made here (the same bytes), which also serves when the device library refuses the call as unsupported.
// A renderer whose box filter reaches neighbouring pixels (ceil(radius - 0.5) >= 1) gets a film that keeps its samples
// (SPT_FILM_KEEP_SAMPLES): --preview-every, --time-limit and --film-devices work with it, the options that need moments or buckets exit with code 2.
// A renderer with a weighted filter ("tent", "gaussian", "mitchell") always renders through such a film plus spt_film_filter, the plain
// run included; --preview-every and --time-limit work with it, the options above and --film-devices exit with code 2.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../../include/spt_host.h"

static void usage() {
    std::fprintf(stderr,
                 "usage: spt -s <scene.json> -r <renderer.json> -o <out.png> [-w 512] [-h 512] [-c camera]\n"
                 "           [--seed N] [--spp N] [--device D | --gpus N | --devices a,b,..] [--strip-rows R] [--debug-normal] [--bezier-ni]\n"
                 "           [--preview-every K] [--time-limit SEC] [--variance-out var.exr]\n"
                 "           [--adaptive REL [--adaptive-floor A] [--adaptive-min-samples N]] [--samples-out counts.exr]\n"
                 "           [--denoise [--denoise-iterations K] [--guide-samples N] [--noisy-out noisy.png]\n"
                 "            [--guide normal|albedo|both] [--demodulate] [--albedo-out albedo.png]]\n"
                 "           [--robust K [--robust-estimator mon|gmon] [--mean-out mean.png]]   (K odd, 3 .. 15)\n"
                 "           [--film-devices a,b,..]   (the progressive options above over several devices)\n"
                 "           [--lens-radius R --focus-distance D | --orthographic H | --panorama]   (a camera model in the scene camera's place)\n"
                 "           [--bake-lightmap INSTANCE --bake-size WxH [--bake-samples N]]   (a float RGB EXR lightmap of a mesh instance: E / pi per texel)\n"
                 "           [--bake-ao INSTANCE --bake-size WxH [--ao-samples N] [--ao-distance D] [--bent-out bent.exr]]   (a float EXR of the cosine-weighted openness per texel; the bent normals)\n"
                 "           [--bake-probes points.txt [--probe-samples N]]   (SH light probes at the `x y z` of each line: 27 coefficients + 4 visibility numbers per line of -o)\n"
                 "           [--gbuffer-out STEM [--gbuffer-samples N] [--gbuffer-host-rays]]   (first-hit images STEM_albedo.exr, STEM_normal.exr, STEM_depth.exr; -o may be left out)\n"
                 "           [--animate frames.json]   (one plain image <out>_NNNN per frame: {\"frames\": [{\"<instance>\": {<transform>}, ..}, ..]})\n");
}

// "0,1,2" -> indices; false for an empty list, an empty item or anything but decimal digits
static bool parse_device_list(const std::string& list, std::vector<int32_t>* out) {
    out->clear();
    if (list.empty()) return false;
    for (size_t pos = 0; pos <= list.size();) {
        const size_t comma = std::min(list.find(',', pos), list.size());
        const std::string item = list.substr(pos, comma - pos);
        if (item.empty() || item.size() > 6 || item.find_first_not_of("0123456789") != std::string::npos) return false;
        out->push_back(std::atoi(item.c_str()));
        pos = comma + 1;
    }
    return !out->empty();
}

// What the progressive loop needs to know: the command line's options, the plan and where the images go.
struct ProgressiveJob {
    spt_host_scene* hs;
    spt_camera cam;
    spt_render_params params;
    std::vector<int32_t> devices;
    uint32_t strip_rows, preview_every;
    double time_limit;
    bool adaptive_on;
    double adaptive, adaptive_floor;
    uint32_t adaptive_min;
    bool denoise, guide_normal, guide_albedo, demodulate;
    uint32_t denoise_iterations, guide_samples;
    bool robust;
    uint32_t robust_k, estimator;
    std::string out_path, noisy_out, albedo_out, mean_out, variance_out, samples_out;
    uint32_t keep_flag;   // SPT_FILM_KEEP_SAMPLES for a box filter that reaches neighbouring pixels, else 0
};

// The progressive loop of main() over a multi film (--film-devices): the same increments, the same decisions and the same
// read-outs in the same order, every spt_film_* call replaced by its spt_host_multi_film_* counterpart.  Returns the exit code.
static int progressive_on_devices(const ProgressiveJob& o) {
    const uint32_t width = o.params.width, height = o.params.height;
    const spt_render_params& params = o.params;
    const spt_device_api api = {spt_scene_create, spt_scene_destroy, spt_render, spt_last_error, spt_pin_host, spt_unpin_host};
    spt_device_film_api fapi;
    std::memset(&fapi, 0, sizeof fapi);
    fapi.size = (uint32_t)sizeof fapi;
    fapi.film_create = spt_film_create;
    fapi.film_destroy = spt_film_destroy;
    fapi.film_render = spt_film_render;
    fapi.film_samples = spt_film_samples;
    fapi.film_read = spt_film_read;
    fapi.film_read_counts = spt_film_read_counts;
    fapi.film_adapt = spt_film_adapt;
    fapi.film_buckets = spt_film_buckets;
    fapi.film_read_robust = spt_film_read_robust;
    fapi.film_read_rgb8 = spt_film_read_rgb8;
    fapi.denoise_image = spt_denoise_image;
    fapi.last_error = spt_last_error;
    spt_host_multi* multi = nullptr;
    spt_host_multi_film *pf = nullptr, *guide = nullptr, *albedo = nullptr;
    auto finish = [&](int code) {
        if (albedo) spt_host_multi_film_destroy(albedo);
        if (guide) spt_host_multi_film_destroy(guide);
        if (pf) spt_host_multi_film_destroy(pf);
        if (multi) spt_host_multi_destroy(multi);
        spt_host_scene_free(o.hs);
        return code;
    };
    auto fail = [&](const char* why = nullptr) {
        std::fprintf(stderr, "Error: %s\n", why ? why : spt_host_last_error());
        return finish(1);
    };
    if (spt_host_multi_create(spt_host_scene_desc(o.hs), &api, (uint32_t)o.devices.size(), o.devices.data(), &multi) != SPT_OK) return fail();
    std::fprintf(stderr, "Scene JSON is loaded successfully. Rendering a film on %zu device(s)...\n", o.devices.size());
    const auto t0 = std::chrono::steady_clock::now();
    const bool moments = !o.variance_out.empty() || o.adaptive_on || o.denoise;
    if (spt_host_multi_film_create(multi, &fapi, &o.cam, &params, o.strip_rows, 0, (moments ? (uint32_t)SPT_FILM_MOMENTS : 0u) | o.keep_flag, o.robust ? o.robust_k : 0u, &pf) != SPT_OK)
        return fail();
    const spt_denoise_params dn = {(uint32_t)sizeof(spt_denoise_params), o.denoise_iterations, 2.0f, 1.0f, 1e-8f, 1e-2f};
    const uint32_t n_guide = std::max(2u, std::min(params.spp, o.guide_samples));
    if (o.denoise && o.guide_normal) {
        spt_render_params gp = params;
        gp.flags |= SPT_RENDER_DEBUG_NORMAL;
        if (spt_host_multi_film_create(multi, &fapi, &o.cam, &gp, o.strip_rows, 0, (uint32_t)SPT_FILM_MOMENTS, 0, &guide) != SPT_OK) return fail();
        if (spt_host_multi_film_render(guide, n_guide) != SPT_OK) return fail();
    }
    if (o.denoise && o.guide_albedo) {
        uint32_t honoured = 0;
        if (spt_render_flags_supported(&honoured) != SPT_OK) return fail(spt_last_error());
        if (!(honoured & SPT_RENDER_AOV_ALBEDO)) return fail("this libspt_hip.so renders no albedo films");
        spt_render_params ap = params;
        ap.flags = (ap.flags & ~(uint32_t)SPT_RENDER_DEBUG_NORMAL) | SPT_RENDER_AOV_ALBEDO;
        if (spt_host_multi_film_create(multi, &fapi, &o.cam, &ap, o.strip_rows, 0, (uint32_t)SPT_FILM_MOMENTS, 0, &albedo) != SPT_OK) return fail();
        if (spt_host_multi_film_render(albedo, n_guide) != SPT_OK) return fail();
    }
    spt_host_multi_film_denoise_job job;
    std::memset(&job, 0, sizeof job);
    job.size = (uint32_t)sizeof job;
    job.flags = SPT_DENOISE_OUT_RGB8 | (o.demodulate ? (uint32_t)SPT_DENOISE_DEMODULATE : 0u);
    job.guide = guide;
    job.albedo = albedo;
    job.params = &dn;
    job.k_albedo = 1.0f; job.eps_albedo = 1e-2f; job.eps_demod = 1e-2f;
    std::vector<uint8_t> film8((size_t)width * height * 3);
    auto write_image8 = [&](const std::string& path) {
        if (spt_host_write_image(path.c_str(), film8.data(), width, height) != SPT_OK)
            std::printf("Failed to save image, err: %s\n", spt_host_last_error());  // printed and ignored, like pt.rs:292-294
    };
    uint32_t done = 0;
    auto read_image = [&]() {
        if (o.robust) return spt_host_multi_film_read_rgb8(pf, o.estimator == (uint32_t)SPT_ROBUST_MON ? SPT_READ_ROBUST_MON : SPT_READ_ROBUST_GMON, film8.data());
        if (o.denoise && done >= 2) return spt_host_multi_film_denoise(pf, &job, film8.data());
        return spt_host_multi_film_read_rgb8(pf, SPT_READ_MEAN, film8.data());
    };
    const uint32_t inc = o.preview_every ? o.preview_every : ((o.time_limit > 0.0 || o.adaptive_on) ? std::max(1u, params.spp / 16u) : params.spp);
    uint32_t active = width * height;
    while (done < params.spp) {
        const uint32_t n = std::min(inc, params.spp - done);
        if (spt_host_multi_film_render(pf, n) != SPT_OK) return fail();
        done += n;
        if (o.adaptive_on && spt_host_multi_film_adapt(pf, (float)o.adaptive, (float)o.adaptive_floor, o.adaptive_min, &active) != SPT_OK) return fail();
        const bool out_of_time = o.time_limit > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= o.time_limit;
        if (done == params.spp || out_of_time || active == 0) break;
        if (o.preview_every) {
            if (read_image() != SPT_OK) return fail();
            write_image8(o.out_path);
        }
    }
    if (!o.noisy_out.empty()) {
        if (spt_host_multi_film_read_rgb8(pf, SPT_READ_MEAN, film8.data()) != SPT_OK) return fail();
        write_image8(o.noisy_out);
    }
    if (!o.albedo_out.empty()) {
        if (spt_host_multi_film_read_rgb8(albedo, SPT_READ_MEAN, film8.data()) != SPT_OK) return fail();
        write_image8(o.albedo_out);
    }
    if (!o.mean_out.empty()) {
        if (spt_host_multi_film_read_rgb8(pf, SPT_READ_MEAN, film8.data()) != SPT_OK) return fail();
        write_image8(o.mean_out);
    }
    if (read_image() != SPT_OK) return fail();
    if (o.adaptive_on) {
        std::fprintf(stderr, "Rendered %u of %u samples per pixel, %u of %u pixels active\n", done, params.spp, active, width * height);
    } else if (o.time_limit > 0.0) {
        std::fprintf(stderr, "Rendered %u of %u samples per pixel\n", done, params.spp);
    }
    if (o.time_limit > 0.0 && done < params.spp && params.sampler == SPT_SAMPLER_JITTERED)
        std::fprintf(stderr, "Warning: the jittered sampler's %ux%u grid is walked row by row: these %u samples cover only its first rows\n",
                     params.division_x, params.division_y, done);
    if (!o.variance_out.empty()) {
        std::vector<float> var((size_t)width * height * 3);
        if (spt_host_multi_film_read(pf, SPT_FILM_VAR_OF_MEAN, var.data()) != SPT_OK) return fail();
        if (spt_host_write_exr(o.variance_out.c_str(), var.data(), width, height) != SPT_OK) return fail();
    }
    if (!o.samples_out.empty()) {   // the samples each pixel covers, as f32 in all three channels
        std::vector<uint32_t> counts((size_t)width * height);
        if (spt_host_multi_film_read_counts(pf, counts.data()) != SPT_OK) return fail();
        std::vector<float> rgb((size_t)width * height * 3);
        for (size_t k = 0; k < counts.size(); ++k) rgb[3 * k] = rgb[3 * k + 1] = rgb[3 * k + 2] = (float)counts[k];
        if (spt_host_write_exr(o.samples_out.c_str(), rgb.data(), width, height) != SPT_OK) return fail();
    }
    write_image8(o.out_path);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "Finished, time used: %.3fs (%.1f Msamples/s, %u samples per pixel)\n", sec, (double)width * height * done / (sec * 1e6), done);
    return finish(0);
}

int main(int argc, char** argv) {
    std::string scene_path, renderer_path, out_path, camera;
    uint32_t width = 512, height = 512, spp_override = 0;
    uint64_t seed = 1;
    int device = 0, gpus = 0;
    uint32_t strip_rows = 0;
    bool debug_normal = false, bezier_ni = false;
    uint32_t preview_every = 0;
    double time_limit = 0.0;
    std::string variance_out, samples_out;
    double adaptive = -1.0, adaptive_floor = 0.0;   // adaptive < 0: off
    uint32_t adaptive_min = 16;
    bool denoise = false;
    uint32_t denoise_iterations = 5, guide_samples = 16;
    std::string noisy_out, guide_mode = "normal", albedo_out;
    bool demodulate = false;
    bool robust = false;
    int robust_k = 0;
    std::string robust_estimator, mean_out;
    std::string animate_path;
    // camera models (spt_render_camera / spt_film_create_camera): a thin lens, an orthographic view or an equirectangular panorama
    double lens_radius = 0.0, focus_distance = 0.0, view_height = 0.0;
    bool lens_given = false, focus_given = false, ortho_given = false, panorama = false;
    // --bake-lightmap INSTANCE --bake-size WxH [--bake-samples N]: spt_bake over the texels of the instance's lightmap
    std::string bake_instance, bake_size;
    uint32_t bake_samples = 16;
    // --bake-ao INSTANCE --bake-size WxH [--ao-samples N] [--ao-distance D] [--bent-out bent.exr]: spt_ao over the same texels
    std::string ao_instance, bent_out;
    uint32_t ao_samples = 16;
    double ao_distance = std::numeric_limits<double>::infinity();
    bool ao_option_given = false;
    // --bake-probes points.txt [--probe-samples N]: spt_probe at the points of the file
    std::string probe_path;
    uint32_t probe_samples = 64;
    // --gbuffer-out STEM [--gbuffer-samples N]: spt_gbuffer over the camera's rays
    std::string gbuffer_out;
    uint32_t gbuffer_samples = 1;
    bool gbuffer_samples_given = false, gbuffer_host_rays = false;
    std::vector<int32_t> device_list;
    std::vector<int32_t> film_devices;
    bool film_devices_given = false, film_devices_ok = true;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) { usage(); std::exit(2); }
            return argv[++i];
        };
        if (a == "-s" || a == "--scene") scene_path = next();
        else if (a == "-r" || a == "--renderer") renderer_path = next();
        else if (a == "-o" || a == "--output") out_path = next();
        else if (a == "-w" || a == "--width") width = (uint32_t)std::atoi(next());
        else if (a == "-h" || a == "--height") height = (uint32_t)std::atoi(next());
        else if (a == "-c" || a == "--camera") camera = next();
        else if (a == "--seed") seed = std::strtoull(next(), nullptr, 10);
        else if (a == "--device") device = std::atoi(next());
        else if (a == "--spp") spp_override = (uint32_t)std::atoi(next());
        else if (a == "--gpus") gpus = std::atoi(next());
        else if (a == "--devices") {      // explicit device list "0,1,2" (an index may repeat: e.g. 0,0 rehearses two workers on one GPU)
            std::string list = next();
            for (size_t pos = 0; pos <= list.size();) {
                const size_t comma = std::min(list.find(',', pos), list.size());
                if (comma > pos) device_list.push_back(std::atoi(list.substr(pos, comma - pos).c_str()));
                pos = comma + 1;
            }
            gpus = (int)device_list.size();
        }
        else if (a == "--strip-rows") strip_rows = (uint32_t)std::atoi(next());
        else if (a == "--debug-normal") debug_normal = true;
        else if (a == "--bezier-ni") bezier_ni = true;
        else if (a == "--preview-every") preview_every = (uint32_t)std::atoi(next());
        else if (a == "--time-limit") time_limit = std::atof(next());
        else if (a == "--variance-out") variance_out = next();
        else if (a == "--adaptive") adaptive = std::atof(next());
        else if (a == "--adaptive-floor") adaptive_floor = std::atof(next());
        else if (a == "--adaptive-min-samples") adaptive_min = (uint32_t)std::atoi(next());
        else if (a == "--samples-out") samples_out = next();
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-iterations") { denoise_iterations = (uint32_t)std::atoi(next()); denoise = true; }
        else if (a == "--guide-samples") { guide_samples = (uint32_t)std::atoi(next()); denoise = true; }
        else if (a == "--noisy-out") { noisy_out = next(); denoise = true; }
        else if (a == "--guide") { guide_mode = next(); denoise = true; }
        else if (a == "--demodulate") { demodulate = true; denoise = true; }
        else if (a == "--albedo-out") { albedo_out = next(); denoise = true; }
        else if (a == "--robust") { robust_k = std::atoi(next()); robust = true; }
        else if (a == "--robust-estimator") robust_estimator = next();
        else if (a == "--mean-out") mean_out = next();
        else if (a == "--animate") animate_path = next();
        else if (a == "--lens-radius") { lens_radius = std::atof(next()); lens_given = true; }
        else if (a == "--focus-distance") { focus_distance = std::atof(next()); focus_given = true; }
        else if (a == "--orthographic") { view_height = std::atof(next()); ortho_given = true; }
        else if (a == "--panorama") panorama = true;
        else if (a == "--bake-lightmap") bake_instance = next();
        else if (a == "--bake-size") bake_size = next();
        else if (a == "--bake-samples") bake_samples = (uint32_t)std::atoi(next());
        else if (a == "--bake-ao") ao_instance = next();
        else if (a == "--ao-samples") { ao_samples = (uint32_t)std::atoi(next()); ao_option_given = true; }
        else if (a == "--ao-distance") { ao_distance = std::atof(next()); ao_option_given = true; }
        else if (a == "--bent-out") { bent_out = next(); ao_option_given = true; }
        else if (a == "--bake-probes") probe_path = next();
        else if (a == "--probe-samples") probe_samples = (uint32_t)std::atoi(next());
        else if (a == "--gbuffer-out") gbuffer_out = next();
        else if (a == "--gbuffer-host-rays") { gbuffer_host_rays = true; gbuffer_samples_given = true; }
        else if (a == "--gbuffer-samples") { gbuffer_samples = (uint32_t)std::atoi(next()); gbuffer_samples_given = true; }
        else if (a == "--film-devices") { film_devices_given = true; film_devices_ok = parse_device_list(next(), &film_devices); }
        else { usage(); return 2; }
    }
    if (scene_path.empty() || renderer_path.empty() || (out_path.empty() && gbuffer_out.empty())) { usage(); return 2; }
    const bool adaptive_on = adaptive >= 0.0;
    if (!robust && (!robust_estimator.empty() || !mean_out.empty())) {
        std::fprintf(stderr, "Error: --robust-estimator and --mean-out need --robust K\n");
        return 2;
    }
    if (robust && (robust_k < 3 || robust_k > 15 || robust_k % 2 == 0)) {
        std::fprintf(stderr, "Error: --robust %d: the bucket count must be odd and 3 .. 15\n", robust_k);
        return 2;
    }
    if (robust && !robust_estimator.empty() && robust_estimator != "mon" && robust_estimator != "gmon") {
        std::fprintf(stderr, "Error: --robust-estimator %s: mon or gmon\n", robust_estimator.c_str());
        return 2;
    }
    if (robust && denoise) {
        std::fprintf(stderr, "Error: --robust and --denoise exclude each other (the denoiser filters the plain mean)\n");
        return 2;
    }
    if (guide_mode != "normal" && guide_mode != "albedo" && guide_mode != "both") {
        std::fprintf(stderr, "Error: --guide %s: normal, albedo or both\n", guide_mode.c_str());
        return 2;
    }
    const bool guide_normal = guide_mode != "albedo", guide_albedo = guide_mode != "normal";
    if ((demodulate || !albedo_out.empty()) && !guide_albedo) {
        std::fprintf(stderr, "Error: --demodulate and --albedo-out need the albedo film (--guide albedo or --guide both)\n");
        return 2;
    }
    const bool thin_lens = lens_given || focus_given;
    const bool camera_model = thin_lens || ortho_given || panorama;
    if ((thin_lens ? 1 : 0) + (ortho_given ? 1 : 0) + (panorama ? 1 : 0) > 1) {
        std::fprintf(stderr, "Error: --lens-radius / --focus-distance, --orthographic and --panorama exclude each other (one camera model)\n");
        return 2;
    }
    if (thin_lens && !(lens_given && focus_given)) {
        std::fprintf(stderr, "Error: a thin lens needs both --lens-radius R and --focus-distance D\n");
        return 2;
    }
    if (camera_model && (gpus > 1 || (film_devices_given && film_devices.size() > 1) || !animate_path.empty() || (denoise && guide_albedo))) {
        std::fprintf(stderr, "Error: a camera model (--lens-radius, --orthographic, --panorama) renders on one device: not with several --gpus / --devices / "
                             "--film-devices, --animate or --guide albedo|both\n");
        return 2;
    }
    bool progressive = preview_every > 0 || time_limit > 0.0 || !variance_out.empty() || adaptive_on || !samples_out.empty() || denoise || robust;
    uint32_t bake_w = 0, bake_h = 0;
    if (ao_option_given && ao_instance.empty()) {
        std::fprintf(stderr, "Error: --ao-samples, --ao-distance and --bent-out need --bake-ao INSTANCE\n");
        return 2;
    }
    if (!ao_instance.empty()) {
        unsigned bw = 0, bh = 0;
        char tail = 0;
        if (std::sscanf(bake_size.c_str(), "%ux%u%c", &bw, &bh, &tail) != 2 || bw == 0 || bh == 0 || ao_samples == 0 || ao_samples > (1u << 24) || !(ao_distance > 0.0)) {
            std::fprintf(stderr, "Error: --bake-ao INSTANCE needs --bake-size WxH (and --ao-samples N in 1 .. 2^24, --ao-distance D > 0)\n");
            return 2;
        }
        if (progressive || camera_model || !animate_path.empty() || gpus > 0 || film_devices_given || debug_normal || !bake_instance.empty() || !probe_path.empty() ||
            !gbuffer_out.empty()) {
            std::fprintf(stderr, "Error: --bake-ao bakes on one device (--device D): not with a film option (--preview-every, --time-limit, --variance-out, "
                                 "--adaptive, --samples-out, --denoise, --robust, --film-devices), a camera model, --animate, --debug-normal, --bake-lightmap, "
                                 "--bake-probes, --gbuffer-out or --gpus / --devices\n");
            return 2;
        }
        bake_w = bw;
        bake_h = bh;
    }
    if (gbuffer_samples_given && gbuffer_out.empty()) {
        std::fprintf(stderr, "Error: --gbuffer-samples and --gbuffer-host-rays need --gbuffer-out STEM\n");
        return 2;
    }
    if (!gbuffer_out.empty()) {
        if (gbuffer_samples == 0) {
            std::fprintf(stderr, "Error: --gbuffer-samples N needs N >= 1\n");
            return 2;
        }
        if (gpus > 1 || (film_devices_given && film_devices.size() > 1)) {
            std::fprintf(stderr, "Error: --gbuffer-out runs on one device: not with several --gpus / --devices / --film-devices\n");
            return 2;
        }
        if (!animate_path.empty() || !bake_instance.empty() || !bake_size.empty() || !probe_path.empty()) {
            std::fprintf(stderr, "Error: --gbuffer-out writes the first-hit images of one camera: not with --animate, --bake-lightmap or --bake-probes\n");
            return 2;
        }
    }
    const uint32_t estimator = robust_estimator == "mon" ? (uint32_t)SPT_ROBUST_MON : (uint32_t)SPT_ROBUST_GMON;
    if (ao_instance.empty() && (!bake_instance.empty() || !bake_size.empty())) {
        unsigned bw = 0, bh = 0;
        char tail = 0;
        if (bake_instance.empty() || std::sscanf(bake_size.c_str(), "%ux%u%c", &bw, &bh, &tail) != 2 || bw == 0 || bh == 0 || bake_samples == 0) {
            std::fprintf(stderr, "Error: a lightmap needs --bake-lightmap INSTANCE and --bake-size WxH (and --bake-samples N >= 1)\n");
            return 2;
        }
        if (progressive || camera_model || !animate_path.empty() || gpus > 0 || film_devices_given || debug_normal) {
            std::fprintf(stderr, "Error: --bake-lightmap bakes on one device (--device D): not with a film option (--preview-every, --time-limit, --variance-out, "
                                 "--adaptive, --samples-out, --denoise, --robust, --film-devices), a camera model, --animate, --debug-normal or --gpus / --devices\n");
            return 2;
        }
        bake_w = bw;
        bake_h = bh;
    }
    std::vector<spt_probe_point> probe_points;
    if (!probe_path.empty()) {
        if (probe_samples == 0) {
            std::fprintf(stderr, "Error: --probe-samples N needs N >= 1\n");
            return 2;
        }
        if (progressive || camera_model || !animate_path.empty() || gpus > 0 || film_devices_given || debug_normal || !bake_instance.empty()) {
            std::fprintf(stderr, "Error: --bake-probes runs on one device (--device D): not with a film option (--preview-every, --time-limit, --variance-out, "
                                 "--adaptive, --samples-out, --denoise, --robust, --film-devices), a camera model, --animate, --debug-normal, --bake-lightmap or "
                                 "--gpus / --devices\n");
            return 2;
        }
        // one `x y z` per line; blank lines are skipped, anything else is malformed
        std::FILE* pf = std::fopen(probe_path.c_str(), "r");
        if (!pf) {
            std::fprintf(stderr, "Error: cannot open %s\n", probe_path.c_str());
            return 2;
        }
        char line[512];
        size_t line_no = 0;
        bool good = true;
        while (good && std::fgets(line, sizeof line, pf)) {
            ++line_no;
            if (line[std::strspn(line, " \t\r\n")] == 0) continue;
            float x = 0.0f, y = 0.0f, z = 0.0f;
            char tail = 0;
            spt_probe_point pt{};
            if (std::sscanf(line, "%f %f %f %c", &x, &y, &z, &tail) != 3 || !std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) good = false;
            pt.p[0] = x; pt.p[1] = y; pt.p[2] = z;
            probe_points.push_back(pt);
        }
        std::fclose(pf);
        if (!good) {
            std::fprintf(stderr, "Error: %s line %zu: three finite numbers `x y z` are expected\n", probe_path.c_str(), line_no);
            return 2;
        }
    }
    if (film_devices_given && !film_devices_ok) {
        std::fprintf(stderr, "Error: --film-devices takes a list of device indices such as 0,1,2 (an index may repeat)\n");
        return 2;
    }
    if (film_devices_given && gpus > 0) {
        std::fprintf(stderr, "Error: --film-devices and --gpus / --devices exclude each other (--gpus renders one image in one call, --film-devices a film in increments)\n");
        return 2;
    }
    if (!animate_path.empty() && (gpus > 1 || film_devices_given || progressive)) {
        std::fprintf(stderr, "Error: --animate renders plain frames on one device: not with several --gpus / --devices, --film-devices, --preview-every, --time-limit, "
                             "--variance-out, --adaptive, --samples-out, --denoise or --robust\n");
        return 2;
    }
    if (progressive && gpus > 1) {
        std::fprintf(stderr, "Error: --preview-every, --time-limit, --variance-out, --adaptive, --samples-out, --denoise and --robust render on one device (a film object), "
                             "not on the %d of --gpus / --devices\n", gpus);
        return 2;
    }
    if (progressive && gpus == 1) {   // one device named through --gpus 1 / --devices d: the film lives there
        device = device_list.empty() ? 0 : device_list[0];
        gpus = 0;
    }

    // this binary and the library it found at run time must agree on the struct layouts of include/spt_abi.h
    if (spt_abi_version() != SPT_ABI_VERSION) {
        std::fprintf(stderr, "Error: libspt_hip.so exports ABI version %u, this program was built against %u\n", spt_abi_version(), (unsigned)SPT_ABI_VERSION);
        return 1;
    }
    std::fprintf(stderr, "Loading from JSON and building aggregate...\n");
    spt_host_scene* hs = nullptr;
    if (spt_host_load_scene(scene_path.c_str(), &hs) != SPT_OK) {
        std::fprintf(stderr, "Error: %s\n", spt_host_last_error());
        return 1;
    }
    if (bezier_ni) spt_host_scene_set_bezier_newton(hs, 1);   // `cargo build --features bezier_ni`
    spt_render_params params;
    std::memset(&params, 0, sizeof params);
    spt_filter_desc filter;
    if (spt_host_load_renderer_filter(renderer_path.c_str(), &params, &filter) != SPT_OK) {
        std::fprintf(stderr, "Error: %s\n", spt_host_last_error());
        return 1;
    }
    if (spp_override && params.sampler != SPT_SAMPLER_JITTERED) params.spp = spp_override;
    // A weighted filter (tent, gaussian, mitchell) is a read-out of kept samples: the run always goes through one sample-keeping film
    // plus spt_film_filter, the plain run included (in increments of spp / 16).  What assumes that every sample of a pixel
    // weighs 1, and films over several devices, cannot serve it
    const bool weighted = filter.type != SPT_FILTER_BOX;
    if (weighted && !animate_path.empty()) {
        std::fprintf(stderr, "Error: --animate needs the box filter; the renderer's filter is weighted (a read-out of one film)\n");
        spt_host_scene_free(hs);
        return 2;
    }
    // --animate FILE: the frames are read and checked against the scene before any device is touched
    spt_host_animation* animation = nullptr;
    struct AnimationOwner {   // freed on every way out of main
        spt_host_animation*& a;
        ~AnimationOwner() { spt_host_animation_free(a); }
    } animation_owner{animation};
    if (!animate_path.empty()) {
        if (spt_host_animation_load(animate_path.c_str(), hs, &animation) != SPT_OK) {
            std::fprintf(stderr, "Error: %s\n", spt_host_last_error());
            spt_host_scene_free(hs);
            return 2;
        }
        if (gpus == 1) {
            device = device_list.empty() ? 0 : device_list[0];
            gpus = 0;
        }
    }
    if (weighted) {
        if (!variance_out.empty() || adaptive_on || !samples_out.empty() || denoise || robust || film_devices_given || gpus > 1) {
            std::fprintf(stderr, "Error: --variance-out, --adaptive, --samples-out, --denoise, --robust, --film-devices and several --gpus / --devices need the box "
                                 "filter; the renderer's filter is weighted (--preview-every and --time-limit work with it)\n");
            spt_host_scene_free(hs);
            return 2;
        }
        if (gpus == 1) {
            device = device_list.empty() ? 0 : device_list[0];
            gpus = 0;
        }
        progressive = true;
    }
    // (after the renderer file is read: under a weighted filter the refusal above is the one that applies)
    if (film_devices_given && !progressive) {
        std::fprintf(stderr, "Error: --film-devices needs a progressive option (--preview-every, --time-limit, --variance-out, --adaptive, --samples-out, --denoise or --robust); "
                             "--gpus / --devices render a plain image on several devices\n");
        spt_host_scene_free(hs);
        return 2;
    }
    // a camera model on one device named through --film-devices d or --gpus 1 / --devices d: the film, or the plain image, lives there
    // (behind every refusal above, which holds for these runs as for any other)
    if (camera_model && film_devices_given) {
        device = film_devices[0];
        film_devices_given = false;
    }
    if (camera_model && gpus == 1) {
        device = device_list.empty() ? 0 : device_list[0];
        gpus = 0;
    }
    // A box filter that reaches neighbouring pixels (ceil(radius - 0.5) >= 1): its film keeps the samples (SPT_FILM_KEEP_SAMPLES),
    // which previews, time limits and several devices can use.  What needs moments or buckets cannot: the library would refuse
    // (spt_film_create with SPT_FILM_MOMENTS, spt_film_buckets), so the run ends here, before any sample is traced
    const bool wide_box = progressive && (params.flags & SPT_RENDER_BOX_RADIUS) && std::ceil(params.filter_radius - 0.5f) >= 1.0f;
    if (wide_box && (!variance_out.empty() || adaptive_on || !samples_out.empty() || denoise || robust)) {
        std::fprintf(stderr, "Error: --variance-out, --adaptive, --samples-out, --denoise and --robust need a box filter within one pixel; the renderer's radius %g "
                             "reaches neighbouring pixels (--preview-every, --time-limit and --film-devices work with it)\n", (double)params.filter_radius);
        spt_host_scene_free(hs);
        return 2;
    }
    if (!probe_path.empty()) {   // the probes: max_depth from the renderer file, the seed of --seed
        auto probe_fail = [&](const char* what) {
            std::fprintf(stderr, "Error: %s\n", what);
            spt_host_scene_free(hs);
            return 1;
        };
        std::vector<float> sh(probe_points.size() * 27), vis(probe_points.size() * 4);
        const auto t_probe = std::chrono::steady_clock::now();
        if (!probe_points.empty()) {
            spt_scene* scene = nullptr;
            if (spt_scene_create(spt_host_scene_desc(hs), device, &scene) != SPT_OK) return probe_fail(spt_last_error());
            spt_probe_job job;
            std::memset(&job, 0, sizeof job);
            job.size = (uint32_t)sizeof job;
            job.n_points = probe_points.size();
            job.points = probe_points.data();
            job.sh_out = sh.data();
            job.aux_out = vis.data();
            job.samples = probe_samples;
            job.max_depth = params.max_depth;
            job.seed = seed;
            const spt_status e = spt_probe(scene, &job);
            const std::string why = e == SPT_OK ? "" : spt_last_error();
            spt_scene_destroy(scene);
            if (e != SPT_OK) return probe_fail(why.c_str());
        }
        std::FILE* of = std::fopen(out_path.c_str(), "w");
        if (!of) return probe_fail("cannot write the output file");
        for (size_t i = 0; i < probe_points.size(); ++i) {   // %.9g round-trips f32
            for (int q = 0; q < 27; ++q) std::fprintf(of, "%.9g ", (double)sh[27 * i + q]);
            std::fprintf(of, "%.9g %.9g %.9g %.9g\n", (double)vis[4 * i], (double)vis[4 * i + 1], (double)vis[4 * i + 2], (double)vis[4 * i + 3]);
        }
        if (std::fclose(of) != 0) return probe_fail("cannot write the output file");
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_probe).count();
        std::fprintf(stderr, "Finished, time used: %.3fs (%zu probes, %u samples each)\n", sec, probe_points.size(), probe_samples);
        spt_host_scene_free(hs);
        return 0;
    }
    if (!ao_instance.empty()) {   // the openness map (and the bent normals): the texels of --bake-lightmap, the seed of --seed; uncovered texels are 0
        auto ao_fail = [&](const char* what) {
            std::fprintf(stderr, "Error: %s\n", what);
            spt_host_scene_free(hs);
            return 1;
        };
        uint64_t n_points = 0;
        if (spt_host_lightmap_points(hs, ao_instance.c_str(), bake_w, bake_h, nullptr, nullptr, 0, &n_points) != SPT_OK) return ao_fail(spt_host_last_error());
        std::vector<spt_bake_point> points(n_points);
        std::vector<uint32_t> texels(n_points);
        if (n_points && spt_host_lightmap_points(hs, ao_instance.c_str(), bake_w, bake_h, points.data(), texels.data(), n_points, &n_points) != SPT_OK)
            return ao_fail(spt_host_last_error());
        std::vector<float> open_map((size_t)bake_w * bake_h * 3, 0.0f), bent_map(bent_out.empty() ? 0 : (size_t)bake_w * bake_h * 3, 0.0f);
        std::vector<spt_ao_rec> recs(points.size());
        const auto t_ao = std::chrono::steady_clock::now();
        if (!points.empty()) {
            spt_scene* scene = nullptr;
            if (spt_scene_create(spt_host_scene_desc(hs), device, &scene) != SPT_OK) return ao_fail(spt_last_error());
            spt_ao_job job;
            std::memset(&job, 0, sizeof job);
            job.size = (uint32_t)sizeof job;
            job.kind = SPT_BAKE_POINTS_SURFACE;
            job.n_points = points.size();
            job.points = points.data();
            job.out = recs.data();
            job.samples = ao_samples;
            job.max_distance = (float)ao_distance;
            job.seed = seed;
            const spt_status e = spt_ao(scene, &job);
            const std::string why = e == SPT_OK ? "" : spt_last_error();
            spt_scene_destroy(scene);
            if (e != SPT_OK) return ao_fail(why.c_str());
        }
        for (size_t k = 0; k < points.size(); ++k)
            for (int c = 0; c < 3; ++c) {
                open_map[3 * (size_t)texels[k] + c] = recs[k].open;
                if (!bent_map.empty()) bent_map[3 * (size_t)texels[k] + c] = recs[k].bent[c];
            }
        if (spt_host_write_exr(out_path.c_str(), open_map.data(), bake_w, bake_h) != SPT_OK) return ao_fail(spt_host_last_error());
        if (!bent_out.empty() && spt_host_write_exr(bent_out.c_str(), bent_map.data(), bake_w, bake_h) != SPT_OK) return ao_fail(spt_host_last_error());
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_ao).count();
        std::fprintf(stderr, "Finished, time used: %.3fs (%zu of %zu texels covered, %u samples each)\n", sec, points.size(), (size_t)bake_w * bake_h, ao_samples);
        spt_host_scene_free(hs);
        return 0;
    }
    if (!bake_instance.empty()) {   // the lightmap: max_depth from the renderer file, the seed of --seed; uncovered texels are 0
        auto bake_fail = [&](const char* what) {
            std::fprintf(stderr, "Error: %s\n", what);
            spt_host_scene_free(hs);
            return 1;
        };
        uint64_t n_points = 0;
        if (spt_host_lightmap_points(hs, bake_instance.c_str(), bake_w, bake_h, nullptr, nullptr, 0, &n_points) != SPT_OK) return bake_fail(spt_host_last_error());
        std::vector<spt_bake_point> points(n_points);
        std::vector<uint32_t> texels(n_points);
        if (n_points && spt_host_lightmap_points(hs, bake_instance.c_str(), bake_w, bake_h, points.data(), texels.data(), n_points, &n_points) != SPT_OK)
            return bake_fail(spt_host_last_error());
        std::vector<float> map((size_t)bake_w * bake_h * 3, 0.0f), rgb(points.size() * 3);
        const auto t_bake = std::chrono::steady_clock::now();
        if (!points.empty()) {
            spt_scene* scene = nullptr;
            if (spt_scene_create(spt_host_scene_desc(hs), device, &scene) != SPT_OK) return bake_fail(spt_last_error());
            spt_bake_job job;
            std::memset(&job, 0, sizeof job);
            job.size = (uint32_t)sizeof job;
            job.kind = SPT_BAKE_POINTS_SURFACE;
            job.n_points = points.size();
            job.points = points.data();
            job.rgb_out = rgb.data();
            job.samples = bake_samples;
            job.max_depth = params.max_depth;
            job.seed = seed;
            const spt_status e = spt_bake(scene, &job);
            const std::string why = e == SPT_OK ? "" : spt_last_error();
            spt_scene_destroy(scene);
            if (e != SPT_OK) return bake_fail(why.c_str());
        }
        for (size_t k = 0; k < points.size(); ++k)
            for (int c = 0; c < 3; ++c) map[3 * (size_t)texels[k] + c] = rgb[3 * k + c];
        if (spt_host_write_exr(out_path.c_str(), map.data(), bake_w, bake_h) != SPT_OK) return bake_fail(spt_host_last_error());
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_bake).count();
        std::fprintf(stderr, "Finished, time used: %.3fs (%zu of %zu texels covered, %u samples each)\n", sec, points.size(), (size_t)bake_w * bake_h, bake_samples);
        spt_host_scene_free(hs);
        return 0;
    }
    const uint32_t keep_flag = (wide_box || weighted) ? (uint32_t)SPT_FILM_KEEP_SAMPLES : 0u;
    spt_camera cam;
    if (spt_host_scene_camera(hs, camera.empty() ? nullptr : camera.c_str(), &cam) != SPT_OK) {
        std::fprintf(stderr, "Error: %s\n", spt_host_last_error());
        return 1;
    }
    spt_camera_model model;
    std::memset(&model, 0, sizeof model);
    model.size = (uint32_t)sizeof model;
    model.type = thin_lens ? SPT_CAMERA_THIN_LENS : ortho_given ? SPT_CAMERA_ORTHOGRAPHIC : panorama ? SPT_CAMERA_PANORAMA : SPT_CAMERA_PERSPECTIVE;
    model.base = cam;
    model.lens_radius = (float)lens_radius;
    model.focus_distance = (float)focus_distance;
    model.view_height = (float)view_height;
    // the plain run and every film of it take the model when one is given (SPT_CAMERA_PERSPECTIVE: the calls they replace)
    auto render_call = [&](const spt_scene* scene, const spt_render_params* rp, float* out, spt_render_stats* stats) {
        return camera_model ? spt_render_camera(scene, &model, rp, out, stats) : spt_render(scene, &cam, rp, out, stats);
    };
    auto film_create_call = [&](const spt_scene* scene, const spt_render_params* rp, uint32_t first, uint32_t flags, spt_film** out) {
        return camera_model ? spt_film_create_camera(scene, &model, rp, first, flags, out) : spt_film_create(scene, &cam, rp, first, flags, out);
    };
    params.width = width;
    params.height = height;
    params.seed = seed;
    params.shard_index = 0;
    params.shard_count = 1;
    params.strip_rows = 16;
    if (debug_normal) params.flags |= SPT_RENDER_DEBUG_NORMAL;
    if (!gbuffer_out.empty()) {
        // The first-hit images, from a device scene of their own ahead of the render, which then runs as it would without them:
        // spt_camera_gbuffer over the plan samples 0 .. N - 1.  The route it replaces gives the same words: per plan sample k the
        // model's rays (spt_host_camera_rays, with their auxiliary rays) go through spt_gbuffer; albedo and normal are the sums in
        // sample order (a miss adds 0) times 1 / N, depth the sum of t over the hit samples divided by their count (0 without one),
        // coverage hits / N
        auto gbuffer_fail = [&](const char* what) {
            std::fprintf(stderr, "Error: %s\n", what);
            spt_host_scene_free(hs);
            return 1;
        };
        const int32_t gdevice = (film_devices_given && !film_devices.empty()) ? film_devices[0] : (gpus == 1 && !device_list.empty()) ? device_list[0] : gpus == 1 ? 0 : device;
        const size_t n_pix = (size_t)width * height;
        std::vector<float> albedo(n_pix * 3, 0.0f), normal(n_pix * 3, 0.0f), depth(n_pix * 3, 0.0f), t_sum(n_pix, 0.0f), hits(n_pix, 0.0f);
        spt_scene* scene = nullptr;
        if (spt_scene_create(spt_host_scene_desc(hs), gdevice, &scene) != SPT_OK) return gbuffer_fail(spt_last_error());
        bool on_device = false;
        if (!gbuffer_host_rays) {
            spt_camera_gbuffer_job job;
            std::memset(&job, 0, sizeof job);
            job.size = (uint32_t)sizeof job;
            job.model = &model;
            job.plan = &params;
            job.count = gbuffer_samples;
            job.albedo = albedo.data();
            job.normal = normal.data();
            job.depth = t_sum.data();
            job.coverage = hits.data();
            const spt_status st = spt_camera_gbuffer(scene, &job);
            if (st != SPT_OK && st != SPT_ERR_UNSUPPORTED) {
                const std::string why = spt_last_error();
                spt_scene_destroy(scene);
                return gbuffer_fail(why.c_str());
            }
            on_device = st == SPT_OK;
            for (size_t i = 0; on_device && i < n_pix; ++i) {
                depth[3 * i] = t_sum[i];
                depth[3 * i + 1] = hits[i];
            }
        }
        std::vector<spt_path_ray> rays(on_device ? 0 : n_pix);
        std::vector<spt_ray_aux> aux(on_device ? 0 : n_pix);
        std::vector<spt_gbuffer_rec> rec(on_device ? 0 : n_pix);
        for (uint32_t k = 0; !on_device && k < gbuffer_samples; ++k) {
            if (spt_host_camera_rays(&model, &params, k, 1, rays.data(), aux.data()) != SPT_OK) {
                spt_scene_destroy(scene);
                return gbuffer_fail(spt_host_last_error());
            }
            spt_gbuffer_job job;
            std::memset(&job, 0, sizeof job);
            job.size = (uint32_t)sizeof job;
            job.n_rays = n_pix;
            job.rays = rays.data();
            job.aux = aux.data();
            job.out = rec.data();
            if (spt_gbuffer(scene, &job) != SPT_OK) {
                const std::string why = spt_last_error();
                spt_scene_destroy(scene);
                return gbuffer_fail(why.c_str());
            }
            for (size_t i = 0; i < n_pix; ++i) {
                const spt_gbuffer_rec& r = rec[i];
                for (int c = 0; c < 3; ++c) {
                    albedo[3 * i + c] += r.albedo[c];
                    normal[3 * i + c] += r.n[c];
                }
                if (r.instance >= 0) {
                    t_sum[i] += r.t;
                    hits[i] += 1.0f;
                }
            }
        }
        spt_scene_destroy(scene);
        const float inv = 1.0f / (float)gbuffer_samples;
        for (size_t i = 0; !on_device && i < n_pix; ++i) {
            for (int c = 0; c < 3; ++c) {
                albedo[3 * i + c] *= inv;
                normal[3 * i + c] *= inv;
            }
            depth[3 * i] = hits[i] > 0.0f ? t_sum[i] / hits[i] : 0.0f;
            depth[3 * i + 1] = hits[i] / (float)gbuffer_samples;
        }
        if (spt_host_write_exr((gbuffer_out + "_albedo.exr").c_str(), albedo.data(), width, height) != SPT_OK ||
            spt_host_write_exr((gbuffer_out + "_normal.exr").c_str(), normal.data(), width, height) != SPT_OK ||
            spt_host_write_exr((gbuffer_out + "_depth.exr").c_str(), depth.data(), width, height) != SPT_OK)
            return gbuffer_fail(spt_host_last_error());
        if (out_path.empty()) {
            spt_host_scene_free(hs);
            return 0;
        }
    }
    if (film_devices_given) {   // the progressive loop over a multi film: a second implementation of the loop below
        ProgressiveJob o;
        o.hs = hs; o.cam = cam; o.params = params; o.devices = film_devices;
        o.strip_rows = strip_rows; o.preview_every = preview_every; o.time_limit = time_limit;
        o.adaptive_on = adaptive_on; o.adaptive = adaptive; o.adaptive_floor = adaptive_floor; o.adaptive_min = adaptive_min;
        o.denoise = denoise; o.guide_normal = guide_normal; o.guide_albedo = guide_albedo; o.demodulate = demodulate;
        o.denoise_iterations = denoise_iterations; o.guide_samples = guide_samples;
        o.robust = robust; o.robust_k = (uint32_t)robust_k; o.estimator = estimator;
        o.out_path = out_path; o.noisy_out = noisy_out; o.albedo_out = albedo_out; o.mean_out = mean_out;
        o.variance_out = variance_out; o.samples_out = samples_out;
        o.keep_flag = keep_flag;
        return progressive_on_devices(o);
    }
    std::vector<float> film((size_t)width * height * 3);
    std::vector<spt_render_stats> st((size_t)std::max(gpus, 1));
    std::memset(st.data(), 0, st.size() * sizeof(spt_render_stats));
    params.stats_size = (uint32_t)sizeof(spt_render_stats);   // the library writes no more than this (ABI v9)
    std::chrono::steady_clock::time_point t0;
    spt_scene* ds = nullptr;
    spt_host_multi* multi = nullptr;
    if (gpus > 0) {
        // --gpus N: devices 0 .. N-1, one replica and one worker thread each, one film
        int32_t have = 0;
        if (device_list.empty() && (spt_device_count(&have) != SPT_OK || have < gpus)) {
            std::fprintf(stderr, "Error: --gpus %d but %d usable gfx950 device(s) are visible\n", gpus, have);
            return 1;
        }
        std::vector<int32_t> devs = device_list;
        if (devs.empty())
            for (int k = 0; k < gpus; ++k) devs.push_back(k);
        const spt_device_api api = {spt_scene_create, spt_scene_destroy, spt_render, spt_last_error, spt_pin_host, spt_unpin_host};
        if (spt_host_multi_create(spt_host_scene_desc(hs), &api, (uint32_t)gpus, devs.data(), &multi) != SPT_OK) {
            std::fprintf(stderr, "Error: %s\n", spt_host_last_error());
            return 1;
        }
        std::fprintf(stderr, "Scene JSON is loaded successfully. Rendering on %d device(s)...\n", gpus);
        t0 = std::chrono::steady_clock::now();
        if (spt_host_multi_render(multi, &cam, &params, strip_rows, film.data(), st.data()) != SPT_OK) {
            std::fprintf(stderr, "Error: %s\n", spt_host_last_error());
            return 1;
        }
    } else {
        if (spt_scene_create(spt_host_scene_desc(hs), device, &ds) != SPT_OK) {
            std::fprintf(stderr, "Error: %s\n", spt_last_error());
            return 1;
        }
        std::fprintf(stderr, "Scene JSON is loaded successfully. Rendering...\n");
        t0 = std::chrono::steady_clock::now();
        if (animation) {
            // one device scene for all frames: every frame moves its instances (spt_host_scene_set_transforms through the
            // animation), hands the new arrays to spt_scene_update and renders the plain run into <out stem>_%04d<ext>
            const size_t slash = out_path.find_last_of('/'), dot = out_path.find_last_of('.');
            const bool has_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
            const std::string stem = has_ext ? out_path.substr(0, dot) : out_path, ext = has_ext ? out_path.substr(dot) : std::string();
            auto anim_fail = [&](const char* msg) {
                std::fprintf(stderr, "Error: %s\n", msg);
                spt_scene_destroy(ds);
                spt_host_scene_free(hs);
                return 1;
            };
            const uint32_t n_frames = spt_host_animation_frames(animation);
            for (uint32_t f = 0; f < n_frames; ++f) {
                if (spt_host_animation_apply(animation, f, hs) != SPT_OK) return anim_fail(spt_host_last_error());
                const spt_scene_desc* dsc = spt_host_scene_desc(hs);
                spt_scene_update_desc up;
                std::memset(&up, 0, sizeof up);
                up.size = (uint32_t)sizeof up;
                up.n_tlas_nodes = dsc->n_tlas_nodes; up.tlas_nodes = dsc->tlas_nodes;
                up.n_instances = dsc->n_instances; up.instances = dsc->instances;
                up.n_lights = dsc->n_lights; up.lights = dsc->lights;
                up.light_alias = dsc->light_alias;
                if (spt_scene_update(ds, &up) != SPT_OK) return anim_fail(spt_last_error());
                if (spt_render(ds, &cam, &params, film.data(), st.data()) != SPT_OK) return anim_fail(spt_last_error());
                char num[16];
                std::snprintf(num, sizeof num, "_%04u", f);
                std::vector<uint8_t> rgb8(film.size());
                spt_host_film_to_rgb8(film.data(), (uint64_t)width * height, rgb8.data());
                if (spt_host_write_image((stem + num + ext).c_str(), rgb8.data(), width, height) != SPT_OK)
                    std::printf("Failed to save image, err: %s\n", spt_host_last_error());  // printed and ignored, like pt.rs:292-294
            }
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            std::fprintf(stderr, "Finished, time used: %.3fs (%u frames)\n", sec, n_frames);
            spt_scene_destroy(ds);
            spt_host_scene_free(hs);
            return 0;
        }
        if (!progressive && render_call(ds, &params, film.data(), st.data()) != SPT_OK) {
            std::fprintf(stderr, "Error: %s\n", spt_last_error());
            return 1;
        }
    }
    auto write_image = [&](const std::string& path, const std::vector<float>& img) {
        std::vector<uint8_t> rgb8(img.size());
        spt_host_film_to_rgb8(img.data(), (uint64_t)width * height, rgb8.data());
        if (spt_host_write_image(path.c_str(), rgb8.data(), width, height) != SPT_OK)
            std::printf("Failed to save image, err: %s\n", spt_host_last_error());  // printed and ignored, like pt.rs:292-294
    };
    // a film's image comes from the device in 8 bits (spt_film_read_rgb8); a plain render's film is converted here
    std::vector<uint8_t> film8;
    auto write_image8 = [&](const std::string& path) {
        if (spt_host_write_image(path.c_str(), film8.data(), width, height) != SPT_OK)
            std::printf("Failed to save image, err: %s\n", spt_host_last_error());  // printed and ignored, like pt.rs:292-294
    };
    auto write_film = [&]() {
        if (progressive) write_image8(out_path);
        else write_image(out_path, film);
    };
    uint32_t done = 0;
    if (progressive) {
        // the film takes the plan's samples in increments; the mean after all of them has the bits of one spt_render
        spt_film* pf = nullptr;
        spt_film* guide = nullptr;   // --denoise: the same plan with SPT_RENDER_DEBUG_NORMAL, a first-hit normal film
        spt_film* albedo = nullptr;  // --guide albedo | both: the same plan with SPT_RENDER_AOV_ALBEDO, a first-hit albedo film
        auto film_fail = [&](const char* why = nullptr) {
            std::fprintf(stderr, "Error: %s\n", why ? why : spt_last_error());
            if (albedo) spt_film_destroy(albedo);
            if (guide) spt_film_destroy(guide);
            if (pf) spt_film_destroy(pf);
            spt_scene_destroy(ds);
            spt_host_scene_free(hs);
            return 1;
        };
        const bool moments = !variance_out.empty() || adaptive_on || denoise;
        if (film_create_call(ds, &params, 0, (moments ? (uint32_t)SPT_FILM_MOMENTS : 0u) | keep_flag, &pf) != SPT_OK) return film_fail();
        if (weighted && spt_film_filter(pf, &filter) != SPT_OK) return film_fail();
        if (robust && spt_film_buckets(pf, (uint32_t)robust_k) != SPT_OK) return film_fail();
        const spt_denoise_params dn = {(uint32_t)sizeof(spt_denoise_params), denoise_iterations, 2.0f, 1.0f, 1e-8f, 1e-2f};
        if (denoise && guide_normal) {   // the guide's samples come first: every preview is filtered with the whole guide
            spt_render_params gp = params;
            gp.flags |= SPT_RENDER_DEBUG_NORMAL;
            if (film_create_call(ds, &gp, 0, (uint32_t)SPT_FILM_MOMENTS, &guide) != SPT_OK) return film_fail();
            if (spt_film_render(guide, std::max(2u, std::min(params.spp, guide_samples))) != SPT_OK) return film_fail();
        }
        if (denoise && guide_albedo) {
            uint32_t honoured = 0;
            if (spt_render_flags_supported(&honoured) != SPT_OK) return film_fail();
            if (!(honoured & SPT_RENDER_AOV_ALBEDO)) return film_fail("this libspt_hip.so renders no albedo films");
            spt_render_params ap = params;
            ap.flags = (ap.flags & ~(uint32_t)SPT_RENDER_DEBUG_NORMAL) | SPT_RENDER_AOV_ALBEDO;
            if (spt_film_create(ds, &cam, &ap, 0, (uint32_t)SPT_FILM_MOMENTS, &albedo) != SPT_OK) return film_fail();
            if (spt_film_render(albedo, std::max(2u, std::min(params.spp, guide_samples))) != SPT_OK) return film_fail();
        }
        spt_denoise_job job;
        std::memset(&job, 0, sizeof job);
        job.size = (uint32_t)sizeof job;
        job.flags = SPT_DENOISE_OUT_RGB8 | (demodulate ? (uint32_t)SPT_DENOISE_DEMODULATE : 0u);
        job.guide = guide;
        job.albedo = albedo;
        job.params = &dn;
        job.k_albedo = 1.0f; job.eps_albedo = 1e-2f; job.eps_demod = 1e-2f;
        // the image of a preview and of the end: the film's mean, the filtered mean (after one sample there is no variance yet)
        // or the robust read-out of the buckets
        film8.resize(film.size());
        auto read_image = [&]() {
            if (robust) return spt_film_read_rgb8(pf, estimator == (uint32_t)SPT_ROBUST_MON ? SPT_READ_ROBUST_MON : SPT_READ_ROBUST_GMON, nullptr, nullptr, film8.data());
            if (denoise && done >= 2 && albedo) return spt_film_denoise_job(pf, &job, film8.data());
            return denoise && done >= 2 ? spt_film_read_rgb8(pf, SPT_READ_DENOISED, guide, &dn, film8.data())
                                        : spt_film_read_rgb8(pf, SPT_READ_MEAN, nullptr, nullptr, film8.data());
        };
        // (a weighted filter's plain run takes its one film in sixteenths too: the read-out does not depend on the increments)
        const uint32_t inc = preview_every ? preview_every : ((time_limit > 0.0 || adaptive_on || weighted) ? std::max(1u, params.spp / 16u) : params.spp);
        uint32_t active = width * height;
        while (done < params.spp) {
            const uint32_t n = std::min(inc, params.spp - done);
            if (spt_film_render(pf, n) != SPT_OK) return film_fail();
            done += n;
            // adaptive: retire the converged pixels after every increment; the render ends once none is left
            if (adaptive_on && spt_film_adapt(pf, (float)adaptive, (float)adaptive_floor, adaptive_min, &active) != SPT_OK) return film_fail();
            const bool out_of_time = time_limit > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= time_limit;
            if (done == params.spp || out_of_time || active == 0) break;
            if (preview_every) {
                if (read_image() != SPT_OK) return film_fail();
                write_film();
            }
        }
        if (!noisy_out.empty()) {
            if (spt_film_read_rgb8(pf, SPT_READ_MEAN, nullptr, nullptr, film8.data()) != SPT_OK) return film_fail();
            write_image8(noisy_out);
        }
        if (!albedo_out.empty()) {
            if (spt_film_read_rgb8(albedo, SPT_READ_MEAN, nullptr, nullptr, film8.data()) != SPT_OK) return film_fail();
            write_image8(albedo_out);
        }
        if (!mean_out.empty()) {
            if (spt_film_read_rgb8(pf, SPT_READ_MEAN, nullptr, nullptr, film8.data()) != SPT_OK) return film_fail();
            write_image8(mean_out);
        }
        if (read_image() != SPT_OK) return film_fail();
        if (adaptive_on) {
            std::fprintf(stderr, "Rendered %u of %u samples per pixel, %u of %u pixels active\n", done, params.spp, active, width * height);
        } else if (time_limit > 0.0) {
            std::fprintf(stderr, "Rendered %u of %u samples per pixel\n", done, params.spp);
        }
        if (time_limit > 0.0) {
            if (done < params.spp && params.sampler == SPT_SAMPLER_JITTERED)
                std::fprintf(stderr, "Warning: the jittered sampler's %ux%u grid is walked row by row: these %u samples cover only its first rows\n",
                             params.division_x, params.division_y, done);
        }
        if (!variance_out.empty()) {
            std::vector<float> var(film.size());
            if (spt_film_read(pf, SPT_FILM_VAR_OF_MEAN, var.data()) != SPT_OK) return film_fail();
            if (spt_host_write_exr(variance_out.c_str(), var.data(), width, height) != SPT_OK) {
                std::fprintf(stderr, "Error: %s\n", spt_host_last_error());
                if (albedo) spt_film_destroy(albedo);
                if (guide) spt_film_destroy(guide);
                spt_film_destroy(pf);
                spt_scene_destroy(ds);
                spt_host_scene_free(hs);
                return 1;
            }
        }
        if (!samples_out.empty()) {   // the samples each pixel covers, as f32 in all three channels
            std::vector<uint32_t> counts((size_t)width * height);
            if (spt_film_read_counts(pf, counts.data()) != SPT_OK) return film_fail();
            std::vector<float> rgb(film.size());
            for (size_t k = 0; k < counts.size(); ++k) rgb[3 * k] = rgb[3 * k + 1] = rgb[3 * k + 2] = (float)counts[k];
            if (spt_host_write_exr(samples_out.c_str(), rgb.data(), width, height) != SPT_OK) {
                std::fprintf(stderr, "Error: %s\n", spt_host_last_error());
                if (albedo) spt_film_destroy(albedo);
                if (guide) spt_film_destroy(guide);
                spt_film_destroy(pf);
                spt_scene_destroy(ds);
                spt_host_scene_free(hs);
                return 1;
            }
        }
        if (albedo) spt_film_destroy(albedo);
        if (guide) spt_film_destroy(guide);
        spt_film_destroy(pf);
    }
    write_film();
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (progressive) {   // (a film returns no kernel times: the host clock of the whole loop)
        std::fprintf(stderr, "Finished, time used: %.3fs (%.1f Msamples/s, %u samples per pixel)\n", sec,
                     (double)width * height * done / (sec * 1e6), done);
        spt_scene_destroy(ds);
        spt_host_scene_free(hs);
        return 0;
    }
    uint64_t samples = 0;
    double gpu_ms = 0.0;      // the slowest device's time on its stream
    for (const spt_render_stats& d : st) { samples += d.samples; gpu_ms = std::max(gpu_ms, d.gpu_ms); }
    std::fprintf(stderr, "Finished, time used: %.3fs (%.1f Msamples/s on the GPU%s, %.3f ms)\n", sec, (double)samples / (gpu_ms * 1e3),
                 gpus > 1 ? "s" : "", gpu_ms);
    if (multi) spt_host_multi_destroy(multi);
    if (ds) spt_scene_destroy(ds);
    spt_host_scene_free(hs);
    return 0;
}

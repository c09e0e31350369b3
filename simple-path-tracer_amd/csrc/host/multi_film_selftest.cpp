// Stand-alone self-test of the film fan-out of multi.cpp (spt_host_multi_film_*), built with -fsanitize=thread and with
// -fsanitize=address,undefined (Makefile: `make selftest`) and run by tests/test_multi_film_selftest.py.  The device and film
// tables are stand-ins whose films are closed-form functions of (pixel, sample), so every read-out of the full image is known
// without a device; what runs is the library's own threading, scatter, gather and error handling, over 1 - 5 workers.
// It links multi.cpp alone: the two functions multi.cpp takes from host_abi.cpp are defined here.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/spt_host.h"

namespace spt_host {
static std::mutex g_mu;
static std::string g_error;
void set_error(const std::string& m) {
    std::lock_guard<std::mutex> lock(g_mu);
    g_error = m;
}
}  // namespace spt_host
extern "C" const char* spt_host_last_error(void) { return spt_host::g_error.c_str(); }   // (read by the calling thread only, between calls)

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond);  \
            ++g_failures;                                                                  \
        }                                                                                  \
    } while (0)

// ---- the stand-in device ---------------------------------------------------------------------------------------------------------
struct StubScene { int32_t device; };
struct StubFilm {
    spt_render_params p;
    uint32_t first, flags, done, buckets;
    std::vector<uint32_t> rows;         // image rows of the shard, increasing
    std::vector<uint32_t> retired_at;   // per pixel of the shard: 0 = active
};

std::atomic<int> g_scenes{0}, g_films{0}, g_creates{0}, g_destroys{0};
std::atomic<int> g_fail_render_shard{-1}, g_fail_create_shard{-1};
thread_local std::string t_error;

float sample_value(uint32_t pixel, uint32_t s, uint32_t c) { return (float)((pixel * 31u + s * 7u + c * 3u) % 17u) * 0.25f; }
bool retires(uint32_t pixel) { return pixel % 3u == 0u; }
uint32_t pixel_count(const StubFilm* f, size_t i) { return f->retired_at[i] ? f->retired_at[i] : f->done; }
// S of pixel `pixel`, channel c, over the samples [first, first + n)
float sum_value(uint32_t pixel, uint32_t first, uint32_t n, uint32_t c) {
    float s = 0.0f;
    for (uint32_t k = 0; k < n; ++k) s += sample_value(pixel, first + k, c);
    return s;
}

spt_status scene_create(const spt_scene_desc*, int32_t device, spt_scene** out) {
    *out = reinterpret_cast<spt_scene*>(new StubScene{device});
    ++g_scenes;
    return SPT_OK;
}
void scene_destroy(spt_scene* s) {
    delete reinterpret_cast<StubScene*>(s);
    --g_scenes;
}
spt_status render(const spt_scene*, const spt_camera*, const spt_render_params*, float*, spt_render_stats*) { return SPT_OK; }
const char* last_error(void) { return t_error.c_str(); }

spt_status film_create(const spt_scene* scene, const spt_camera* cam, const spt_render_params* p, uint32_t first, uint32_t flags, spt_film** out) {
    if (!scene || !cam || !p || !out) return SPT_ERR_INVALID_ARG;
    if ((int)p->shard_index == g_fail_create_shard.load()) { t_error = "stub: induced create failure"; return SPT_ERR_HIP; }
    StubFilm* f = new StubFilm{*p, first, flags, 0u, 0u, {}, {}};
    for (uint32_t j = 0; j < p->height; ++j)
        if ((j / p->strip_rows) % p->shard_count == p->shard_index) f->rows.push_back(j);
    f->retired_at.assign(f->rows.size() * p->width, 0u);
    *out = reinterpret_cast<spt_film*>(f);
    ++g_films;
    ++g_creates;
    return SPT_OK;
}
void film_destroy(spt_film* h) {
    delete reinterpret_cast<StubFilm*>(h);
    --g_films;
    ++g_destroys;
}
spt_status film_render(spt_film* h, uint32_t n) {
    StubFilm* f = reinterpret_cast<StubFilm*>(h);
    if ((int)f->p.shard_index == g_fail_render_shard.load()) { t_error = "stub: induced render failure"; return SPT_ERR_HIP; }
    if (f->first + f->done + n > f->p.spp) { t_error = "stub: past the plan's spp"; return SPT_ERR_INVALID_ARG; }
    f->done += n;
    return SPT_OK;
}
spt_status film_samples(const spt_film* h, uint32_t* done) {
    *done = reinterpret_cast<const StubFilm*>(h)->done;
    return SPT_OK;
}
template <class Fn>
void for_pixels(const StubFilm* f, Fn fn) {   // fn(index in the shard, pixel of the image)
    size_t i = 0;
    for (uint32_t j : f->rows)
        for (uint32_t x = 0; x < f->p.width; ++x, ++i) fn(i, j * f->p.width + x);
}
spt_status film_read(spt_film* h, uint32_t what, float* out) {
    StubFilm* f = reinterpret_cast<StubFilm*>(h);
    if (what > SPT_FILM_VAR_OF_MEAN) { t_error = "stub: unknown read-out"; return SPT_ERR_INVALID_ARG; }
    if (what >= SPT_FILM_SUM_SQ && !(f->flags & SPT_FILM_MOMENTS)) { t_error = "stub: no moments"; return SPT_ERR_INVALID_ARG; }
    for_pixels(f, [&](size_t i, uint32_t pixel) {
        const uint32_t n = pixel_count(f, i);
        for (uint32_t c = 0; c < 3; ++c) {
            const float s = sum_value(pixel, f->first, n, c);
            out[3 * i + c] = what == SPT_FILM_MEAN ? s / (float)n : (what == SPT_FILM_SUM ? s : (what == SPT_FILM_SUM_SQ ? s * s : 1.0f / (float)(n + pixel)));
        }
    });
    return SPT_OK;
}
spt_status film_read_counts(spt_film* h, uint32_t* out) {
    StubFilm* f = reinterpret_cast<StubFilm*>(h);
    for_pixels(f, [&](size_t i, uint32_t) { out[i] = pixel_count(f, i); });
    return SPT_OK;
}
spt_status film_adapt(spt_film* h, float, float, uint32_t min_samples, uint32_t* active) {
    StubFilm* f = reinterpret_cast<StubFilm*>(h);
    uint32_t left = 0;
    for_pixels(f, [&](size_t i, uint32_t pixel) {
        if (f->done >= min_samples && !f->retired_at[i] && retires(pixel)) f->retired_at[i] = f->done;
        left += f->retired_at[i] ? 0u : 1u;
    });
    if (active) *active = left;
    return SPT_OK;
}
spt_status film_buckets(spt_film* h, uint32_t k) {
    if (k % 2u == 0u) { t_error = "stub: even bucket count"; return SPT_ERR_INVALID_ARG; }
    reinterpret_cast<StubFilm*>(h)->buckets = k;
    return SPT_OK;
}
spt_status film_read_robust(spt_film* h, uint32_t estimator, float* out) {
    StubFilm* f = reinterpret_cast<StubFilm*>(h);
    if (!f->buckets) { t_error = "stub: no buckets"; return SPT_ERR_INVALID_ARG; }
    for_pixels(f, [&](size_t i, uint32_t pixel) {
        for (uint32_t c = 0; c < 3; ++c) out[3 * i + c] = (float)(pixel * 3u + c) + 0.5f * (float)estimator + (float)f->buckets;
    });
    return SPT_OK;
}
spt_status film_read_rgb8(spt_film* h, uint32_t source, spt_film* guide, const spt_denoise_params* dn, uint8_t* out) {
    StubFilm* f = reinterpret_cast<StubFilm*>(h);
    if (guide || dn) return SPT_ERR_INVALID_ARG;
    for_pixels(f, [&](size_t i, uint32_t pixel) {
        for (uint32_t c = 0; c < 3; ++c) out[3 * i + c] = (uint8_t)((pixel * 3u + c + 11u * source + f->done) & 255u);
    });
    return SPT_OK;
}
std::atomic<int> g_denoise_device{-99};
spt_status denoise_image(const spt_scene* scene, const spt_image_denoise_job* job, void* out) {
    g_denoise_device = reinterpret_cast<const StubScene*>(scene)->device;
    const size_t n = (size_t)job->width * job->rows * 3;
    for (size_t i = 0; i < n; ++i) {
        float v = job->mean[i] + 2.0f * job->var[i];
        if (job->guide_mean) v += 4.0f * job->guide_mean[i] + 8.0f * job->guide_var[i];
        if (job->albedo_mean) v += 16.0f * job->albedo_mean[i] + 32.0f * job->albedo_var[i];
        if (job->flags & SPT_DENOISE_OUT_RGB8) static_cast<uint8_t*>(out)[i] = (uint8_t)((uint32_t)v & 255u);
        else static_cast<float*>(out)[i] = v;
    }
    return SPT_OK;
}

// ---- the expected full images ----------------------------------------------------------------------------------------------------
struct Expect {
    uint32_t w, h, first, done, retired_done;   // retired_done: `done` at the adapt call (0: none)
    uint32_t count(uint32_t pixel) const { return retired_done && retires(pixel) ? retired_done : done; }
    float read(uint32_t what, uint32_t pixel, uint32_t c) const {
        const uint32_t n = count(pixel);
        const float s = sum_value(pixel, first, n, c);
        return what == SPT_FILM_MEAN ? s / (float)n : (what == SPT_FILM_SUM ? s : (what == SPT_FILM_SUM_SQ ? s * s : 1.0f / (float)(n + pixel)));
    }
};

void check_read_outs(spt_host_multi_film* f, const Expect& e, uint32_t buckets) {
    const size_t n_pix = (size_t)e.w * e.h;
    std::vector<float> img(n_pix * 3);
    uint32_t done = 0;
    CHECK(spt_host_multi_film_samples(f, &done) == SPT_OK && done == e.done);
    for (uint32_t what = 0; what <= SPT_FILM_VAR_OF_MEAN; ++what) {
        std::fill(img.begin(), img.end(), -1.0f);
        CHECK(spt_host_multi_film_read(f, what, img.data()) == SPT_OK);
        bool same = true;
        for (uint32_t p = 0; p < n_pix; ++p)
            for (uint32_t c = 0; c < 3; ++c) same = same && img[3 * p + c] == e.read(what, p, c);
        CHECK(same);
    }
    std::vector<uint32_t> counts(n_pix, 0xffffffffu);
    CHECK(spt_host_multi_film_read_counts(f, counts.data()) == SPT_OK);
    for (uint32_t p = 0; p < n_pix; ++p) CHECK(counts[p] == e.count(p));
    for (uint32_t est = 0; est < 2; ++est) {
        CHECK(spt_host_multi_film_read_robust(f, est, img.data()) == SPT_OK);
        bool same = true;
        for (uint32_t i = 0; i < n_pix * 3; ++i) same = same && img[i] == (float)i + 0.5f * (float)est + (float)buckets;
        CHECK(same);
    }
    std::vector<uint8_t> bytes(n_pix * 3);
    for (uint32_t source = 0; source < 3; ++source) {
        CHECK(spt_host_multi_film_read_rgb8(f, source, bytes.data()) == SPT_OK);
        bool same = true;
        for (uint32_t i = 0; i < n_pix * 3; ++i) same = same && bytes[i] == (uint8_t)((i + 11u * source + e.done) & 255u);
        CHECK(same);
    }
    CHECK(spt_host_multi_film_read_rgb8(f, SPT_READ_DENOISED, bytes.data()) == SPT_ERR_INVALID_ARG);
    CHECK(std::strstr(spt_host_last_error(), "spt_host_multi_film_denoise") != nullptr);
}

void run(uint32_t n_workers, uint32_t w, uint32_t h, uint32_t strip_rows) {
    const spt_device_api api = {scene_create, scene_destroy, render, last_error, nullptr, nullptr};
    spt_device_film_api fapi;
    std::memset(&fapi, 0, sizeof fapi);
    fapi.size = (uint32_t)sizeof fapi;
    fapi.film_create = film_create; fapi.film_destroy = film_destroy; fapi.film_render = film_render; fapi.film_samples = film_samples;
    fapi.film_read = film_read; fapi.film_read_counts = film_read_counts; fapi.film_adapt = film_adapt; fapi.film_buckets = film_buckets;
    fapi.film_read_robust = film_read_robust; fapi.film_read_rgb8 = film_read_rgb8; fapi.denoise_image = denoise_image; fapi.last_error = last_error;
    spt_scene_desc desc;
    std::memset(&desc, 0, sizeof desc);
    std::vector<int32_t> devices;
    for (uint32_t k = 0; k < n_workers; ++k) devices.push_back(10 + (int32_t)(k % 3u));   // indices repeat from 4 workers on
    spt_host_multi* m = nullptr;
    CHECK(spt_host_multi_create(&desc, &api, n_workers, devices.data(), &m) == SPT_OK);
    if (!m) return;
    spt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    spt_render_params p;
    std::memset(&p, 0, sizeof p);
    p.width = w; p.height = h; p.spp = 20;
    spt_host_multi_film *f = nullptr, *guide = nullptr, *albedo = nullptr;
    CHECK(spt_host_multi_film_create(m, &fapi, &cam, &p, strip_rows, 3, SPT_FILM_MOMENTS, 5, &f) == SPT_OK);
    CHECK(spt_host_multi_film_create(m, &fapi, &cam, &p, strip_rows, 0, SPT_FILM_MOMENTS, 0, &guide) == SPT_OK);
    CHECK(spt_host_multi_film_create(m, &fapi, &cam, &p, strip_rows, 1, SPT_FILM_MOMENTS, 0, &albedo) == SPT_OK);
    if (!f || !guide || !albedo) return;
    CHECK(g_films.load() == (int)(3 * n_workers));
    Expect e{w, h, 3, 0, 0};
    CHECK(spt_host_multi_film_render(f, 4) == SPT_OK);
    e.done = 4;
    check_read_outs(f, e, 5);
    uint32_t active = 0, want_active = 0;
    for (uint32_t px = 0; px < w * h; ++px) want_active += retires(px) ? 0u : 1u;
    CHECK(spt_host_multi_film_adapt(f, 0.1f, 0.0f, 2, &active) == SPT_OK && active == want_active);
    e.retired_done = 4;
    CHECK(spt_host_multi_film_render(f, 5) == SPT_OK);
    e.done = 9;
    check_read_outs(f, e, 5);
    // a call that every shard refuses leaves the film as it was
    CHECK(spt_host_multi_film_render(f, 100) == SPT_ERR_INVALID_ARG);
    CHECK(std::strstr(spt_host_last_error(), "device 10 (shard 0 of ") != nullptr && std::strstr(spt_host_last_error(), "past the plan") != nullptr);
    check_read_outs(f, e, 5);
    // the denoiser: the gathered arrays are the whole films', the filter runs on replica 0
    CHECK(spt_host_multi_film_render(guide, 2) == SPT_OK && spt_host_multi_film_render(albedo, 3) == SPT_OK);
    const Expect eg{w, h, 0, 2, 0}, ea{w, h, 1, 3, 0};
    spt_host_multi_film_denoise_job job;
    std::memset(&job, 0, sizeof job);
    job.size = (uint32_t)sizeof job;
    job.guide = guide;
    job.albedo = albedo;
    std::vector<float> img((size_t)w * h * 3, -1.0f);
    CHECK(spt_host_multi_film_denoise(f, &job, img.data()) == SPT_OK);
    CHECK(g_denoise_device.load() == 10);
    bool same = true;
    for (uint32_t px = 0; px < w * h; ++px)
        for (uint32_t c = 0; c < 3; ++c) {
            float want = e.read(0, px, c) + 2.0f * e.read(3, px, c);      // (the stand-in's grouping of the sums)
            want += 4.0f * eg.read(0, px, c) + 8.0f * eg.read(3, px, c);
            want += 16.0f * ea.read(0, px, c) + 32.0f * ea.read(3, px, c);
            same = same && img[3 * px + c] == want;
        }
    CHECK(same);
    job.guide = nullptr;
    job.albedo = nullptr;
    job.flags = SPT_DENOISE_OUT_RGB8;
    std::vector<uint8_t> bytes((size_t)w * h * 3);
    CHECK(spt_host_multi_film_denoise(f, &job, bytes.data()) == SPT_OK);
    same = true;
    for (uint32_t px = 0; px < w * h; ++px)
        for (uint32_t c = 0; c < 3; ++c) same = same && bytes[3 * px + c] == (uint8_t)((uint32_t)(e.read(0, px, c) + 2.0f * e.read(3, px, c)) & 255u);
    CHECK(same);
    job.guide = f;
    CHECK(spt_host_multi_film_denoise(f, &job, bytes.data()) == SPT_ERR_INVALID_ARG);
    // the error path: one shard fails (with two or more workers the film is then broken), every later call is refused
    if (n_workers >= 2) {
        g_fail_render_shard = 1;
        CHECK(spt_host_multi_film_render(f, 1) == SPT_ERR_HIP);
        CHECK(std::strstr(spt_host_last_error(), "device 11 (shard 1 of ") != nullptr);
        g_fail_render_shard = -1;
        uint32_t done = 0;
        CHECK(spt_host_multi_film_render(f, 1) == SPT_ERR_INVALID_ARG && std::strstr(spt_host_last_error(), "broken") != nullptr);
        CHECK(std::strstr(spt_host_last_error(), "induced render failure") != nullptr);
        CHECK(spt_host_multi_film_samples(f, &done) == SPT_ERR_INVALID_ARG);
        CHECK(spt_host_multi_film_read(f, 0, img.data()) == SPT_ERR_INVALID_ARG);
        CHECK(spt_host_multi_film_read_counts(f, reinterpret_cast<uint32_t*>(img.data())) == SPT_ERR_INVALID_ARG);
        CHECK(spt_host_multi_film_read_robust(f, 0, img.data()) == SPT_ERR_INVALID_ARG);
        CHECK(spt_host_multi_film_read_rgb8(f, 0, bytes.data()) == SPT_ERR_INVALID_ARG);
        CHECK(spt_host_multi_film_adapt(f, 0.1f, 0.0f, 2, &active) == SPT_ERR_INVALID_ARG);
        job.guide = nullptr;
        CHECK(spt_host_multi_film_denoise(f, &job, bytes.data()) == SPT_ERR_INVALID_ARG);
        // a refused create releases the shards that did come up
        const int before = g_films.load();
        g_fail_create_shard = (int)n_workers - 1;
        spt_host_multi_film* none = reinterpret_cast<spt_host_multi_film*>(&job);
        CHECK(spt_host_multi_film_create(m, &fapi, &cam, &p, strip_rows, 0, 0, 0, &none) == SPT_ERR_HIP);
        CHECK(none == reinterpret_cast<spt_host_multi_film*>(&job) && g_films.load() == before);
        g_fail_create_shard = -1;
    }
    spt_host_multi_film* refused = nullptr;
    CHECK(spt_host_multi_film_create(m, &fapi, &cam, &p, strip_rows, 0, 0, 4, &refused) == SPT_ERR_INVALID_ARG && refused == nullptr);   // the shards refuse 4 buckets
    spt_host_multi_film_destroy(albedo);
    spt_host_multi_film_destroy(guide);
    // the spt_host_multi goes first: it releases the shard films of `f`, which refuses every call and is destroyed afterwards
    CHECK(g_films.load() == (int)n_workers);
    spt_host_multi_destroy(m);
    CHECK(g_films.load() == 0 && g_scenes.load() == 0);
    uint32_t done_after = 0;
    CHECK(spt_host_multi_film_samples(f, &done_after) == SPT_ERR_INVALID_ARG && std::strstr(spt_host_last_error(), "has been destroyed") != nullptr);
    CHECK(spt_host_multi_film_render(f, 1) == SPT_ERR_INVALID_ARG);
    spt_host_multi_film_destroy(f);
}

}  // namespace

int main() {
    const uint32_t shapes[][3] = {{7, 11, 1}, {7, 11, 3}, {5, 9, 0}, {9, 1, 16}, {3, 2, 2}};
    for (uint32_t n = 1; n <= 5; ++n)
        for (const auto& s : shapes) run(n, s[0], s[1], s[2]);
    CHECK(g_creates.load() == g_destroys.load() && g_creates.load() > 0);
    if (g_failures) {
        std::fprintf(stderr, "multi_film_selftest: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("multi_film_selftest ok: %d shard films over 1 - 5 workers\n", g_creates.load());
    return 0;
}

// One call, N devices, one film (include/spt_host.h): the counterpart of the thread fan-out of PathTracer::render
// (reference src/renderer/pt.rs:243-287) with a GPU behind every worker.  The reference cuts the image into contiguous
// row bands, one per thread (src/renderer/util.rs:6-19), and lets every thread write its pixels into the one film through
// UnsafeFilm (src/core/film.rs:101-116).  Here the bands are interleaved strips - a contiguous band would put the whole
// object of a typical scene on two or three of eight devices - and "write into the one film" is a strided device-to-host
// copy per worker; nothing else changes hands, so there is no collective and no ordering between workers to get wrong.
//
// Workers are persistent threads (created with the replicas, parked on a condition variable between frames): a frame of
// the headline workload is ~0.5 ms per device at n = 8, thread creation would be a tenth of that.  A worker's job is a callable
// that receives the worker's index: a frame of spt_host_multi_render, or one call of a multi film (spt_host_multi_film_*, below).
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <functional>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/spt_host.h"

struct spt_host_multi;
namespace spt_host {
void set_error(const std::string& m);
void detach_films(spt_host_multi* m);   // below, with the multi films
}

struct spt_host_multi_film;

struct spt_host_multi {
    spt_device_api api{};
    std::vector<int32_t> devices;
    std::vector<spt_scene*> scenes;
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    uint64_t job_id = 0;          // incremented per job; a worker runs job k once
    uint32_t pending = 0;         // workers still busy with the current job
    bool quit = false;
    std::mutex call_mu;           // one job at a time (held by run_on_workers)
    std::function<void(uint32_t)> job;   // the current job: called once on every worker with the worker's index
    // the current frame of spt_host_multi_render
    const spt_camera* cam = nullptr;
    spt_render_params params{};
    float* film = nullptr;
    spt_render_stats* stats = nullptr;
    std::vector<spt_status> status;
    std::vector<std::string> errors;
    void* pinned = nullptr;       // film currently page-locked through api.pin_host
    uint64_t pinned_bytes = 0;
    std::vector<spt_host_multi_film*> multi_films;   // alive on these replicas: spt_host_multi_destroy releases their shards
};

namespace {

void worker_main(spt_host_multi* m, uint32_t k) {
    uint64_t seen = 0;
    for (;;) {
        {
            std::unique_lock<std::mutex> lock(m->mu);
            m->cv_job.wait(lock, [&] { return m->quit || m->job_id != seen; });
            if (m->quit) return;
            seen = m->job_id;
        }
        m->job(k);   // (set before job_id moved, unchanged until every worker is done)
        {
            std::lock_guard<std::mutex> lock(m->mu);
            if (--m->pending == 0) m->cv_done.notify_all();
        }
    }
}

// Runs fn(k) on worker k, for every k, and returns when all are done.  The caller holds m->call_mu.
void run_on_workers_locked(spt_host_multi* m, std::function<void(uint32_t)> fn) {
    std::unique_lock<std::mutex> lock(m->mu);
    m->job = std::move(fn);
    m->pending = (uint32_t)m->devices.size();
    ++m->job_id;
    m->cv_job.notify_all();
    m->cv_done.wait(lock, [&] { return m->pending == 0; });
    m->job = nullptr;
}

// The same for a caller that shares nothing else of `m` with other callers: one job at a time.
void run_on_workers(spt_host_multi* m, std::function<void(uint32_t)> fn) {
    std::lock_guard<std::mutex> call(m->call_mu);
    run_on_workers_locked(m, std::move(fn));
}

// One worker's share of a frame of spt_host_multi_render
void render_shard(spt_host_multi* m, uint32_t k) {
    const uint32_t n = (uint32_t)m->devices.size();
    spt_render_params p = m->params;
    p.shard_index = k;
    p.shard_count = n;
    const uint64_t row_bytes = (uint64_t)p.width * 3u * sizeof(float);
    p.out_strip_stride = (uint64_t)n * p.strip_rows * row_bytes;      // this worker's strips, in place in the full film
    float* first = m->film + (size_t)k * p.strip_rows * p.width * 3u;
    // a worker whose first strip lies below the image has no rows at all (more devices than strips)
    if ((uint64_t)k * p.strip_rows >= p.height) first = m->film;
    spt_render_stats* st = m->stats ? reinterpret_cast<spt_render_stats*>(reinterpret_cast<char*>(m->stats) + (size_t)k * p.stats_size) : nullptr;
    const spt_status rc = m->api.render(m->scenes[k], m->cam, &p, first, st);
    std::string err;
    if (rc != SPT_OK) {
        const char* e = m->api.last_error ? m->api.last_error() : nullptr;   // thread-local in libspt_hip.so: read it on THIS thread
        err = "device " + std::to_string(m->devices[k]) + " (shard " + std::to_string(k) + " of " + std::to_string(n) + "): " + (e ? e : "render failed");
    }
    m->status[k] = rc;      // (entry k is this worker's; the caller reads it after run_on_workers)
    m->errors[k] = err;
}

// The strip height spt_host_multi_render and spt_host_multi_film_create use for strip_rows == 0
uint32_t default_strip_rows(uint32_t height, uint32_t n) {
    // Even shares: every device should own several strips spread over the whole image.  16 rows (one tile row of the
    // primary kernel) while that still leaves >= 8 strips per device, finer below (measured on the headline image at n = 8:
    // slowest / mean device 1.15 with 16-row strips, 1.05 with 4-row strips, tools/strip_rows_sweep.py)
    uint32_t strip_rows = 16;
    while (strip_rows > 1 && (uint64_t)height < (uint64_t)strip_rows * n * 8u) strip_rows /= 2;
    return strip_rows;
}

void stop_workers(spt_host_multi* m) {
    {
        std::lock_guard<std::mutex> lock(m->mu);
        m->quit = true;
    }
    m->cv_job.notify_all();
    for (auto& t : m->workers)
        if (t.joinable()) t.join();
    m->workers.clear();
}

}  // namespace

extern "C" {

spt_status spt_host_multi_create(const spt_scene_desc* desc, const spt_device_api* api, uint32_t n_devices, const int32_t* devices,
                                 spt_host_multi** out) {
    if (!desc || !api || !devices || !out || n_devices == 0) { spt_host::set_error("multi_create: null argument or no devices"); return SPT_ERR_INVALID_ARG; }
    if (!api->scene_create || !api->scene_destroy || !api->render) { spt_host::set_error("multi_create: the device table lacks scene_create / scene_destroy / render"); return SPT_ERR_INVALID_ARG; }
    if (n_devices > 1024u) { spt_host::set_error("multi_create: more than 1024 devices"); return SPT_ERR_INVALID_ARG; }
    *out = nullptr;
    spt_host_multi* m = new spt_host_multi();
    m->api = *api;
    m->devices.assign(devices, devices + n_devices);
    m->scenes.assign(n_devices, nullptr);
    m->status.assign(n_devices, SPT_OK);
    m->errors.assign(n_devices, std::string());
    // the replicas are uploaded side by side (a scene create is a BVH build + an upload: hundreds of ms for a large scene)
    {
        std::vector<std::thread> th;
        for (uint32_t k = 0; k < n_devices; ++k)
            th.emplace_back([m, desc, k] {
                const spt_status rc = m->api.scene_create(desc, m->devices[k], &m->scenes[k]);
                m->status[k] = rc;
                if (rc != SPT_OK) {
                    const char* e = m->api.last_error ? m->api.last_error() : nullptr;
                    m->errors[k] = "device " + std::to_string(m->devices[k]) + ": " + (e ? e : "scene_create failed");
                }
            });
        for (auto& t : th) t.join();
    }
    for (uint32_t k = 0; k < n_devices; ++k) {
        if (m->status[k] != SPT_OK) {
            const spt_status rc = m->status[k];
            spt_host::set_error("multi_create: " + m->errors[k]);
            for (spt_scene* s : m->scenes)
                if (s) m->api.scene_destroy(s);
            delete m;
            return rc;
        }
    }
    for (uint32_t k = 0; k < n_devices; ++k) m->workers.emplace_back(worker_main, m, k);
    *out = m;
    return SPT_OK;
}

uint32_t spt_host_multi_device_count(const spt_host_multi* m) { return m ? (uint32_t)m->devices.size() : 0u; }

spt_status spt_host_multi_render(spt_host_multi* m, const spt_camera* cam, const spt_render_params* params, uint32_t strip_rows,
                                 float* film, spt_render_stats* stats) {
    if (!m || !cam || !params || !film) { spt_host::set_error("multi_render: null argument"); return SPT_ERR_INVALID_ARG; }
    if (params->width == 0 || params->height == 0) { spt_host::set_error("multi_render: width and height must be > 0"); return SPT_ERR_INVALID_ARG; }
    if (stats && params->stats_size < 8u) { spt_host::set_error("multi_render: stats given but params.stats_size is not set"); return SPT_ERR_INVALID_ARG; }
    if (params->flags & SPT_RENDER_ASYNC) { spt_host::set_error("multi_render: SPT_RENDER_ASYNC is not supported (the call returns a complete film)"); return SPT_ERR_INVALID_ARG; }
    const uint32_t n = (uint32_t)m->devices.size();
    if (strip_rows == 0) strip_rows = default_strip_rows(params->height, n);
    // the frame fields, the registration of the film and the per-worker status are the spt_host_multi's: one frame at a time,
    // also next to a multi film's calls from another thread
    std::lock_guard<std::mutex> call(m->call_mu);
    const uint64_t bytes = (uint64_t)params->width * params->height * 3u * sizeof(float);
    if (m->api.pin_host && m->api.unpin_host && (m->pinned != film || m->pinned_bytes != bytes)) {
        if (m->pinned) m->api.unpin_host(m->pinned);
        m->pinned = nullptr;
        if (m->api.pin_host(film, bytes) == SPT_OK) { m->pinned = film; m->pinned_bytes = bytes; }   // not fatal: the copy-out is slower, not wrong
    }
    m->cam = cam;
    m->params = *params;
    m->params.strip_rows = strip_rows;
    m->film = film;
    m->stats = stats;
    run_on_workers_locked(m, [m](uint32_t k) { render_shard(m, k); });
    for (uint32_t k = 0; k < n; ++k)
        if (m->status[k] != SPT_OK) {
            spt_host::set_error("multi_render: " + m->errors[k]);
            return m->status[k];
        }
    return SPT_OK;
}

void spt_host_multi_destroy(spt_host_multi* m) {
    if (!m) return;
    spt_host::detach_films(m);
    stop_workers(m);
    if (m->pinned && m->api.unpin_host) m->api.unpin_host(m->pinned);
    for (spt_scene* s : m->scenes)
        if (s) m->api.scene_destroy(s);
    delete m;
}

}  // extern "C"

// ---- a progressive film over the replicas (spt_host_multi_film_*, include/spt_host.h) -----------------------------------------
// One shard film per replica, every call the same call on every shard, on the workers.  A read-out is "read the shard's packed
// rows into this worker's buffer, then copy its strips to their rows of the caller's image", both on the worker: no two workers
// own a row, so the scatter needs no lock, and the copies of one shard run beside the device read of another.
struct spt_host_multi_film {
    spt_host_multi* m = nullptr;
    spt_device_film_api api{};
    spt_camera cam{};
    spt_render_params plan{};     // shard_count = n, strip_rows resolved; shard_index is set per worker
    uint32_t n = 0;
    std::vector<spt_film*> films;
    std::vector<uint32_t> rows;   // image rows of shard k
    std::vector<std::vector<unsigned char>> packed;   // per worker: the packed rows of the read-out in flight
    std::vector<float> gathered[6];                   // denoise: m, v, g, u, al, ua of the whole image
    std::vector<spt_status> status;
    std::vector<std::string> errors;
    std::vector<uint32_t> active;
    bool broken = false;
    std::string first_error;
    bool detached = false;        // its spt_host_multi was destroyed first (which released the shard films): only destroy is left
};

namespace {

using MultiFilm = spt_host_multi_film;

uint32_t shard_rows_of(uint32_t height, uint32_t strip_rows, uint32_t k, uint32_t n) {
    uint32_t rows = 0;
    for (uint64_t j0 = (uint64_t)k * strip_rows; j0 < height; j0 += (uint64_t)n * strip_rows) rows += (uint32_t)std::min<uint64_t>(strip_rows, height - j0);
    return rows;
}

// Shard k's packed rows to their rows of the full image; `pixel_bytes` per pixel.
void scatter(const MultiFilm* f, uint32_t k, const unsigned char* shard, size_t pixel_bytes, unsigned char* image) {
    const spt_render_params& p = f->plan;
    const size_t row_bytes = (size_t)p.width * pixel_bytes;
    for (uint64_t j0 = (uint64_t)k * p.strip_rows; j0 < p.height; j0 += (uint64_t)f->n * p.strip_rows) {
        const size_t bytes = (size_t)std::min<uint64_t>(p.strip_rows, p.height - j0) * row_bytes;
        std::memcpy(image + (size_t)j0 * row_bytes, shard, bytes);
        shard += bytes;
    }
}

std::string shard_name(const MultiFilm* f, uint32_t k) {
    return "device " + std::to_string(f->m->devices[k]) + " (shard " + std::to_string(k) + " of " + std::to_string(f->n) + "): ";
}

// Notes what call `rc` of shard k returned (on the worker: the message is thread-local in libspt_hip.so).
void note(MultiFilm* f, uint32_t k, spt_status rc, const char* what) {
    f->status[k] = rc;
    f->errors[k].clear();
    if (rc == SPT_OK) return;
    const char* e = f->api.last_error ? f->api.last_error() : nullptr;
    f->errors[k] = shard_name(f, k) + (e && *e ? e : (std::string(what) + " failed"));
}

// fn(k) -> status on every worker; the first shard's error, if any, becomes the call's.
spt_status on_shards(MultiFilm* f, const char* who, const char* what, const std::function<spt_status(uint32_t)>& fn) {
    run_on_workers(f->m, [&](uint32_t k) { note(f, k, fn(k), what); });
    for (uint32_t k = 0; k < f->n; ++k)
        if (f->status[k] != SPT_OK) {
            spt_host::set_error(std::string(who) + ": " + f->errors[k]);
            return f->status[k];
        }
    return SPT_OK;
}

// The entry of a call: null film, broken film.
bool usable(const MultiFilm* f, const char* who) {
    if (!f) { spt_host::set_error(std::string(who) + ": null argument"); return false; }
    if (f->detached) { spt_host::set_error(std::string(who) + ": the spt_host_multi of this multi film has been destroyed (only spt_host_multi_film_destroy is left)"); return false; }
    if (f->broken) {
        spt_host::set_error(std::string(who) + ": the multi film is broken (a call failed on some of its shards and not on others, they are out of step); the first error was: " + f->first_error);
        return false;
    }
    return true;
}

spt_status unsupported(const char* who, const char* entry) {
    spt_host::set_error(std::string(who) + ": the film table has no " + entry);
    return SPT_ERR_UNSUPPORTED;
}

// A call that changes the shards (render, adapt): all fail -> refused; some fail -> the film is broken.
spt_status on_shards_changing(MultiFilm* f, const char* who, const char* what, const std::function<spt_status(uint32_t)>& fn) {
    const spt_status rc = on_shards(f, who, what, fn);
    if (rc == SPT_OK) return rc;
    uint32_t failed = 0;
    for (uint32_t k = 0; k < f->n; ++k) failed += f->status[k] != SPT_OK ? 1u : 0u;
    if (failed != f->n) {
        f->broken = true;
        for (uint32_t k = 0; k < f->n; ++k)
            if (f->status[k] != SPT_OK) { f->first_error = f->errors[k]; break; }
    }
    return rc;
}

// A read-out of `pixel_bytes` per pixel: read(k, shard film, packed buffer) on every worker, then the worker's scatter.
spt_status read_out(MultiFilm* f, const char* who, size_t pixel_bytes, void* image, const std::function<spt_status(spt_film*, void*)>& read) {
    return on_shards(f, who, "read", [&](uint32_t k) {
        std::vector<unsigned char>& buf = f->packed[k];
        const size_t bytes = (size_t)f->rows[k] * f->plan.width * pixel_bytes;
        if (buf.size() < std::max<size_t>(bytes, 16)) buf.resize(std::max<size_t>(bytes, 16));   // (never null: a shard without rows still checks its arguments)
        const spt_status rc = read(f->films[k], buf.data());
        if (rc == SPT_OK) scatter(f, k, buf.data(), pixel_bytes, static_cast<unsigned char*>(image));
        return rc;
    });
}

void destroy_shards(MultiFilm* f) {
    run_on_workers(f->m, [f](uint32_t k) {
        if (f->films[k]) f->api.film_destroy(f->films[k]);
        f->films[k] = nullptr;
    });
}

}  // namespace

extern "C" {

spt_status spt_host_multi_film_create(spt_host_multi* m, const spt_device_film_api* film_api, const spt_camera* cam,
                                      const spt_render_params* params, uint32_t strip_rows, uint32_t first_sample, uint32_t film_flags,
                                      uint32_t n_buckets, spt_host_multi_film** out) {
    const char* who = "multi_film_create";
    if (!m || !film_api || !cam || !params || !out) { spt_host::set_error("multi_film_create: null argument"); return SPT_ERR_INVALID_ARG; }
    if (film_api->size < offsetof(spt_device_film_api, film_create)) { spt_host::set_error("multi_film_create: film_api->size is not set"); return SPT_ERR_INVALID_ARG; }
    if (params->width == 0 || params->height == 0) { spt_host::set_error("multi_film_create: width and height must be > 0"); return SPT_ERR_INVALID_ARG; }
    if (params->flags & (SPT_RENDER_ASYNC | SPT_RENDER_PROFILE | SPT_RENDER_COUNT_VISITS)) {
        spt_host::set_error("multi_film_create: SPT_RENDER_ASYNC / PROFILE / COUNT_VISITS are not supported (a film's calls are synchronous and return no stats)");
        return SPT_ERR_INVALID_ARG;
    }
    if (params->out_strip_stride != 0) { spt_host::set_error("multi_film_create: out_strip_stride must be 0 (a film's rows are packed)"); return SPT_ERR_INVALID_ARG; }
    MultiFilm* f = new MultiFilm();
    f->m = m;
    std::memcpy(&f->api, film_api, std::min<size_t>(film_api->size, sizeof f->api));   // entries behind `size` stay NULL
    if (!f->api.film_create || !f->api.film_destroy) { delete f; return unsupported(who, "film_create / film_destroy"); }
    if (n_buckets != 0 && !f->api.film_buckets) { delete f; return unsupported(who, "film_buckets"); }
    f->n = (uint32_t)m->devices.size();
    f->cam = *cam;
    f->plan = *params;
    f->plan.shard_count = f->n;
    f->plan.strip_rows = strip_rows ? strip_rows : default_strip_rows(params->height, f->n);
    f->films.assign(f->n, nullptr);
    f->packed.resize(f->n);
    f->status.assign(f->n, SPT_OK);
    f->errors.assign(f->n, std::string());
    f->active.assign(f->n, 0u);
    for (uint32_t k = 0; k < f->n; ++k) f->rows.push_back(shard_rows_of(f->plan.height, f->plan.strip_rows, k, f->n));
    const spt_status rc = on_shards(f, who, "film_create", [&](uint32_t k) {
        spt_render_params p = f->plan;
        p.shard_index = k;
        spt_status st = f->api.film_create(m->scenes[k], &f->cam, &p, first_sample, film_flags, &f->films[k]);
        if (st != SPT_OK) f->films[k] = nullptr;
        if (st == SPT_OK && n_buckets != 0) st = f->api.film_buckets(f->films[k], n_buckets);
        return st;
    });
    if (rc != SPT_OK) {   // (the message is set; film_destroy does not touch it)
        destroy_shards(f);
        delete f;
        return rc;
    }
    m->multi_films.push_back(f);
    *out = f;
    return SPT_OK;
}

spt_status spt_host_multi_film_render(spt_host_multi_film* f, uint32_t n_samples) {
    const char* who = "multi_film_render";
    if (!usable(f, who)) return SPT_ERR_INVALID_ARG;
    if (!f->api.film_render) return unsupported(who, "film_render");
    return on_shards_changing(f, who, "film_render", [&](uint32_t k) { return f->api.film_render(f->films[k], n_samples); });
}

spt_status spt_host_multi_film_adapt(spt_host_multi_film* f, float rel_error, float abs_floor, uint32_t min_samples, uint32_t* active_out) {
    const char* who = "multi_film_adapt";
    if (!usable(f, who)) return SPT_ERR_INVALID_ARG;
    if (!f->api.film_adapt) return unsupported(who, "film_adapt");
    const spt_status rc = on_shards_changing(f, who, "film_adapt", [&](uint32_t k) {
        f->active[k] = 0;
        return f->api.film_adapt(f->films[k], rel_error, abs_floor, min_samples, &f->active[k]);
    });
    if (rc != SPT_OK) return rc;
    if (active_out) {
        uint32_t sum = 0;
        for (uint32_t a : f->active) sum += a;
        *active_out = sum;
    }
    return SPT_OK;
}

spt_status spt_host_multi_film_samples(const spt_host_multi_film* f, uint32_t* done) {
    const char* who = "multi_film_samples";
    if (!usable(f, who)) return SPT_ERR_INVALID_ARG;
    if (!done) { spt_host::set_error("multi_film_samples: null argument"); return SPT_ERR_INVALID_ARG; }
    if (!f->api.film_samples) return unsupported(who, "film_samples");
    // (every shard is at the same plan position; shard 0 always exists.  No device work: the calling thread asks)
    const spt_status rc = f->api.film_samples(f->films[0], done);
    if (rc != SPT_OK) {
        const char* e = f->api.last_error ? f->api.last_error() : nullptr;
        spt_host::set_error(std::string(who) + ": " + shard_name(f, 0) + (e && *e ? e : "film_samples failed"));
    }
    return rc;
}

spt_status spt_host_multi_film_read(spt_host_multi_film* f, uint32_t what, float* image) {
    const char* who = "multi_film_read";
    if (!usable(f, who)) return SPT_ERR_INVALID_ARG;
    if (!image) { spt_host::set_error("multi_film_read: null argument"); return SPT_ERR_INVALID_ARG; }
    if (!f->api.film_read) return unsupported(who, "film_read");
    return read_out(f, who, 3 * sizeof(float), image, [&](spt_film* s, void* buf) { return f->api.film_read(s, what, static_cast<float*>(buf)); });
}

spt_status spt_host_multi_film_read_counts(spt_host_multi_film* f, uint32_t* image) {
    const char* who = "multi_film_read_counts";
    if (!usable(f, who)) return SPT_ERR_INVALID_ARG;
    if (!image) { spt_host::set_error("multi_film_read_counts: null argument"); return SPT_ERR_INVALID_ARG; }
    if (!f->api.film_read_counts) return unsupported(who, "film_read_counts");
    return read_out(f, who, sizeof(uint32_t), image, [&](spt_film* s, void* buf) { return f->api.film_read_counts(s, static_cast<uint32_t*>(buf)); });
}

spt_status spt_host_multi_film_read_robust(spt_host_multi_film* f, uint32_t estimator, float* image) {
    const char* who = "multi_film_read_robust";
    if (!usable(f, who)) return SPT_ERR_INVALID_ARG;
    if (!image) { spt_host::set_error("multi_film_read_robust: null argument"); return SPT_ERR_INVALID_ARG; }
    if (!f->api.film_read_robust) return unsupported(who, "film_read_robust");
    return read_out(f, who, 3 * sizeof(float), image, [&](spt_film* s, void* buf) { return f->api.film_read_robust(s, estimator, static_cast<float*>(buf)); });
}

spt_status spt_host_multi_film_read_rgb8(spt_host_multi_film* f, uint32_t source, uint8_t* image) {
    const char* who = "multi_film_read_rgb8";
    if (!usable(f, who)) return SPT_ERR_INVALID_ARG;
    if (!image) { spt_host::set_error("multi_film_read_rgb8: null argument"); return SPT_ERR_INVALID_ARG; }
    if (source == SPT_READ_DENOISED) {
        spt_host::set_error("multi_film_read_rgb8: SPT_READ_DENOISED is not a per-shard read-out (a shard's rows are not neighbours): use spt_host_multi_film_denoise with SPT_DENOISE_OUT_RGB8");
        return SPT_ERR_INVALID_ARG;
    }
    if (source > SPT_READ_DENOISED) { spt_host::set_error("multi_film_read_rgb8: unknown SPT_READ_* value"); return SPT_ERR_INVALID_ARG; }
    if (!f->api.film_read_rgb8) return unsupported(who, "film_read_rgb8");
    return read_out(f, who, 3, image, [&](spt_film* s, void* buf) { return f->api.film_read_rgb8(s, source, nullptr, nullptr, static_cast<uint8_t*>(buf)); });
}

spt_status spt_host_multi_film_denoise(spt_host_multi_film* f, const spt_host_multi_film_denoise_job* job, void* image) {
    const char* who = "multi_film_denoise";
    if (!usable(f, who)) return SPT_ERR_INVALID_ARG;
    if (!job || !image) { spt_host::set_error("multi_film_denoise: null argument"); return SPT_ERR_INVALID_ARG; }
    if (job->size < offsetof(spt_host_multi_film_denoise_job, k_albedo)) { spt_host::set_error("multi_film_denoise: job->size ends before k_albedo"); return SPT_ERR_INVALID_ARG; }
    if (!f->api.film_read) return unsupported(who, "film_read");
    if (!f->api.denoise_image) return unsupported(who, "denoise_image");
    MultiFilm* const src[3] = {f, job->guide, job->albedo};
    const char* const names[3] = {"film", "guide", "albedo film"};
    for (int i = 1; i < 3; ++i) {
        const MultiFilm* g = src[i];
        if (!g) continue;
        if (g->broken || g->detached) { usable(g, who); return SPT_ERR_INVALID_ARG; }
        std::string why;
        if (g == f) why = "is the film itself";
        else if (i == 2 && g == job->guide) why = "is the guide";
        else if (g->m != f->m) why = "belongs to another spt_host_multi";
        else if (g->plan.width != f->plan.width || g->plan.height != f->plan.height) why = "has another width or height";
        else if (g->plan.strip_rows != f->plan.strip_rows || g->n != f->n) why = "has another strip layout";
        if (!why.empty()) { spt_host::set_error(std::string("multi_film_denoise: the ") + names[i] + " " + why); return SPT_ERR_INVALID_ARG; }
        if (!g->api.film_read) return unsupported(who, "film_read (the guide's or the albedo film's table)");
    }
    if ((job->flags & SPT_DENOISE_DEMODULATE) && !job->albedo) { spt_host::set_error("multi_film_denoise: SPT_DENOISE_DEMODULATE needs an albedo film"); return SPT_ERR_INVALID_ARG; }
    // gather: every worker reads mean and variance of the mean of its shard of each film and scatters them
    const size_t n_floats = (size_t)f->plan.width * f->plan.height * 3;
    for (int i = 0; i < 3; ++i)
        if (src[i])
            for (int q = 0; q < 2; ++q)
                if (f->gathered[2 * i + q].size() < n_floats) f->gathered[2 * i + q].resize(n_floats);
    spt_status rc = on_shards(f, who, "film_read", [&](uint32_t k) {
        std::vector<unsigned char>& buf = f->packed[k];
        const size_t bytes = (size_t)f->rows[k] * f->plan.width * 3 * sizeof(float);
        if (buf.size() < std::max<size_t>(bytes, 16)) buf.resize(std::max<size_t>(bytes, 16));
        for (int i = 0; i < 3; ++i) {
            if (!src[i]) continue;
            for (uint32_t q = 0; q < 2; ++q) {
                // (each film through the table it was created with)
                const spt_status st = src[i]->api.film_read(src[i]->films[k], q == 0 ? (uint32_t)SPT_FILM_MEAN : (uint32_t)SPT_FILM_VAR_OF_MEAN, reinterpret_cast<float*>(buf.data()));
                if (st != SPT_OK) return st;
                scatter(f, k, buf.data(), 3 * sizeof(float), reinterpret_cast<unsigned char*>(f->gathered[2 * i + q].data()));
            }
        }
        return (spt_status)SPT_OK;
    });
    if (rc != SPT_OK) return rc;
    spt_image_denoise_job ij;
    std::memset(&ij, 0, sizeof ij);
    ij.size = (uint32_t)sizeof ij;
    ij.flags = job->flags;
    ij.width = f->plan.width;
    ij.rows = f->plan.height;
    ij.mean = f->gathered[0].data();
    ij.var = f->gathered[1].data();
    if (job->guide) { ij.guide_mean = f->gathered[2].data(); ij.guide_var = f->gathered[3].data(); }
    if (job->albedo) { ij.albedo_mean = f->gathered[4].data(); ij.albedo_var = f->gathered[5].data(); }
    ij.params = job->params;
    ij.k_albedo = 1.0f; ij.eps_albedo = 1e-2f; ij.eps_demod = 1e-2f;
    if (job->size >= offsetof(spt_host_multi_film_denoise_job, k_albedo) + sizeof(float)) ij.k_albedo = job->k_albedo;
    if (job->size >= offsetof(spt_host_multi_film_denoise_job, eps_albedo) + sizeof(float)) ij.eps_albedo = job->eps_albedo;
    if (job->size >= offsetof(spt_host_multi_film_denoise_job, eps_demod) + sizeof(float)) ij.eps_demod = job->eps_demod;
    // one filter over the whole image, on replica 0's scene, run by worker 0 as the shard calls of that replica are (the other
    // workers return at once)
    run_on_workers(f->m, [&](uint32_t k) {
        if (k == 0) note(f, 0, f->api.denoise_image(f->m->scenes[0], &ij, image), "denoise_image");
    });
    if (f->status[0] != SPT_OK) {
        spt_host::set_error(std::string(who) + ": " + f->errors[0]);
        return f->status[0];
    }
    return SPT_OK;
}

void spt_host_multi_film_destroy(spt_host_multi_film* f) {
    if (!f) return;
    if (!f->detached) {
        destroy_shards(f);
        std::vector<spt_host_multi_film*>& alive = f->m->multi_films;
        alive.erase(std::remove(alive.begin(), alive.end(), f), alive.end());
    }
    delete f;
}

}  // extern "C"

// spt_host_multi_destroy with multi films still alive: their shard films go (a film is destroyed before its scene) and the
// multi films stay behind as husks that refuse every call, so that destroying them later - in whatever order a garbage
// collector finds - touches nothing of the spt_host_multi that is gone.
void spt_host::detach_films(spt_host_multi* m) {
    for (spt_host_multi_film* f : m->multi_films) {
        destroy_shards(f);
        f->detached = true;
        f->m = nullptr;
    }
    m->multi_films.clear();
}

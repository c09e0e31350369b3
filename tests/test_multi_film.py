"""A progressive film over the replicas of a MultiDevice (spt_host_multi_film_*, include/spt_host.h).

CPU half: the film entry points are stand-ins (ctypes callbacks) whose films are float32 numpy restatements fed by the CPU oracle's
single samples - the fan-out, the shard plans, the scatter of every read-out, the gather of the denoiser, the error paths and the
"broken" state are the library's own code.  The expected value is the SAME restatement as one whole-image film (shard 0 of 1).
GPU half: libspt_hip.so's functions, two and three workers on the one device, every read-out and the denoised image equal to the
single-device ProgressiveFilm of the same plan bit for bit; and `spt --film-devices 0,0`."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import _albedo_ref as A
import _denoise_job_ref as J
import _robust_ref as R
import _util
from test_multi_device import StubDevices

spt = _util.load_pkg()
INVALID, HIP_ERROR, UNSUPPORTED = 1, 3, 4
W, H, SPP = 24, 20, 24

FILM_CREATE = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(spt.Camera), C.POINTER(spt.RenderParams), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p))
FILM_DESTROY = C.CFUNCTYPE(None, C.c_void_p)
FILM_RENDER = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_uint32)
FILM_SAMPLES = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_uint32))
FILM_READ = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p)
FILM_READ_COUNTS = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p)
FILM_ADAPT = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.POINTER(C.c_uint32))
FILM_BUCKETS = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_uint32)
FILM_READ_RGB8 = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
DENOISE_IMAGE = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(spt.ImageDenoiseJob), C.c_void_p)
LAST_ERROR = C.CFUNCTYPE(C.c_void_p)


class NumpyFilm:
    """One shard film of spt_abi.h in float32 numpy: the rows `rows` of the whole-image samples x[s]."""

    def __init__(self, x, rows, spp, first, moments):
        self.x, self.rows, self.spp, self.first, self.moments = x, rows, spp, first, moments
        shape = (len(rows), x.shape[2], 3)
        self.s, self.q = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        self.done = 0
        self.active = np.ones(shape[:2], bool)
        self.retired_at = np.zeros(shape[:2], np.uint32)
        self.b = None

    def buckets(self, k):
        if k < 3 or k > 15 or k % 2 == 0 or self.done or self.b is not None:
            return INVALID
        self.b = np.zeros((k,) + self.s.shape, np.float32)
        return 0

    def render(self, n):
        if self.first + self.done + n > self.spp:
            return INVALID
        with np.errstate(all="ignore"):
            for i in range(n):
                plan_index = self.first + self.done
                x = self.x[plan_index][self.rows]
                self.s, self.q = _util.film_add_sample(self.s, self.q, x, self.active)
                if self.b is not None:
                    j = plan_index % len(self.b)
                    self.b[j] = np.where(self.active[..., None], self.b[j] + x, self.b[j])
                self.done += 1
        return 0

    def counts(self):
        return np.where(self.active, np.uint32(self.done), self.retired_at).astype(np.uint32)

    def adapt(self, rel, floor, min_samples):
        if not self.moments:
            return INVALID, 0
        if self.done >= max(min_samples, 2) and self.s.size:
            with np.errstate(all="ignore"):
                retire = _util.film_criterion(self.s, self.q, self.done, rel, floor) & self.active
            self.retired_at[retire] = self.done
            self.active &= ~retire
        return 0, int(self.active.sum())

    def read(self, what):
        if what > 3 or (what >= 2 and not self.moments) or (what in (0, 3) and self.done == 0):
            return None
        if what == 1:
            return self.s
        if what == 2:
            return self.q
        with np.errstate(all="ignore"):
            m, v = _util.film_mean_and_variance(self.s, self.q, self.counts())
        return m if what == 0 else v

    def robust(self, estimator):
        if self.b is None or estimator > 1 or self.done == 0:
            return None
        with np.errstate(all="ignore"):
            return R.robust(self.b, self.s, self.first, self.counts(), estimator)

    def rgb8(self, source):
        img = self.read(0) if source == 0 else (self.robust(source - 1) if source in (1, 2) else None)
        if img is None:
            return None
        return spt.film_to_rgb8(np.ascontiguousarray(img)) if img.size else np.zeros(img.shape, np.uint8)


_SAMPLES = {}


def _plan_samples(scene_name, flags, w, h):
    """The whole-image single samples of the test plan (spp SPP, seed 7): beauty, first-hit normal (flags 16) or albedo (32)."""
    key = (scene_name, flags, w, h)
    if key not in _SAMPLES:
        sc = spt.load_scene(os.path.join(_util.SCENES, scene_name))
        kw = dict(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=SPP, seed=7)
        if flags & spt.RENDER_AOV_ALBEDO:
            x = _util.oracle_render_samples(A.StandIn(sc), spt.PathTracer(**dict(kw, max_depth=1)), w, h, 0, SPP)
        else:
            x = _util.oracle_render_samples(sc, spt.PathTracer(debug_normal=bool(flags & spt.RENDER_DEBUG_NORMAL), **kw), w, h, 0, SPP)
        x.setflags(write=False)
        _SAMPLES[key] = x
        sc.close()
    return _SAMPLES[key]


def _tracer():
    return spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=SPP, seed=7)


class StubFilms:
    """Stand-in for the film half of libspt_hip.so: NumpyFilm objects behind integer handles."""

    def __init__(self, scene_name="cfg2_cube.json", fail_render_shard=None, fail_create_shard=None, without=()):
        self.scene_name = scene_name
        self.films, self.next_handle = {}, 5000
        self.created, self.destroyed = 0, 0
        self.threads = {}
        self.lock = threading.Lock()
        self.fail_render_shard, self.fail_create_shard = fail_render_shard, fail_create_shard
        self.denoise_calls = []
        self._err = C.create_string_buffer(b"stub: induced failure")
        self._cb = dict(film_create=FILM_CREATE(self.film_create), film_destroy=FILM_DESTROY(self.film_destroy),
                        film_render=FILM_RENDER(self.film_render), film_samples=FILM_SAMPLES(self.film_samples),
                        film_read=FILM_READ(self.film_read), film_read_counts=FILM_READ_COUNTS(self.film_read_counts),
                        film_adapt=FILM_ADAPT(self.film_adapt), film_buckets=FILM_BUCKETS(self.film_buckets),
                        film_read_robust=FILM_READ(self.film_read_robust), film_read_rgb8=FILM_READ_RGB8(self.film_read_rgb8),
                        denoise_image=DENOISE_IMAGE(self.denoise_image), last_error=LAST_ERROR(lambda: C.addressof(self._err)))
        self.api = spt.DeviceFilmApi(C.sizeof(spt.DeviceFilmApi))
        for name, cb in self._cb.items():
            if name not in without:
                setattr(self.api, name, C.cast(cb, C.c_void_p).value)

    def film_create(self, scene, cam, params, first, flags, out):
        p = params.contents
        if p.shard_index == self.fail_create_shard:
            return HIP_ERROR
        if (p.flags & spt.RENDER_BOX_RADIUS) and np.ceil(p.filter_radius - 0.5) >= 1:
            return UNSUPPORTED
        x = _plan_samples(self.scene_name, p.flags & (spt.RENDER_DEBUG_NORMAL | spt.RENDER_AOV_ALBEDO), p.width, p.height)
        rows = spt.shard_rows(p.height, p.shard_index, p.shard_count, p.strip_rows)
        film = NumpyFilm(x, rows, p.spp, first, bool(flags & spt.FILM_MOMENTS))
        film.shard = (p.shard_index, p.shard_count, p.strip_rows)
        with self.lock:
            self.next_handle += 1
            self.films[self.next_handle] = film
            self.created += 1
            out[0] = self.next_handle
        return 0

    def film_destroy(self, h):
        with self.lock:
            del self.films[h]
            self.destroyed += 1

    def film_render(self, h, n):
        f = self.films[h]
        with self.lock:
            self.threads[f.shard[0]] = threading.get_ident()
        if f.shard[0] == self.fail_render_shard:
            return HIP_ERROR
        return f.render(n)

    def film_samples(self, h, done):
        done[0] = self.films[h].done
        return 0

    @staticmethod
    def _deliver(img, out):
        if img is None or not out:      # (a null pointer is refused even by a shard without rows, as libspt_hip.so does)
            return INVALID
        img = np.ascontiguousarray(img)
        if img.nbytes:
            C.memmove(out, img.ctypes.data, img.nbytes)
        return 0

    def film_read(self, h, what, out):
        return self._deliver(self.films[h].read(what), out)

    def film_read_counts(self, h, out):
        return self._deliver(self.films[h].counts(), out)

    def film_adapt(self, h, rel, floor, min_samples, active):
        rc, n = self.films[h].adapt(rel, floor, min_samples)
        if rc == 0 and active:
            active[0] = n
        return rc

    def film_buckets(self, h, k):
        return self.films[h].buckets(k)

    def film_read_robust(self, h, estimator, out):
        return self._deliver(self.films[h].robust(estimator), out)

    def film_read_rgb8(self, h, source, guide, dn, out):
        assert not guide and not dn
        return self._deliver(self.films[h].rgb8(source), out)

    def denoise_image(self, scene, job, out):
        j = job.contents
        shape = (j.rows, j.width, 3)
        arr = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=shape).copy() if p else None
        got = dict(scene=scene, flags=j.flags, m=arr(j.mean), v=arr(j.var), g=arr(j.guide_mean), u=arr(j.guide_var), al=arr(j.albedo_mean),
                   ua=arr(j.albedo_var), iterations=j.params.contents.iterations, k_albedo=j.k_albedo, thread=threading.get_ident())
        self.denoise_calls.append(got)
        res = J.denoise_job(got["m"], got["v"], got["g"], got["u"], got["al"], got["ua"], demodulate=bool(j.flags & spt.DENOISE_DEMODULATE),
                            iterations=got["iterations"], k_albedo=j.k_albedo, eps_albedo=j.eps_albedo, eps_demod=j.eps_demod)
        return self._deliver(spt.film_to_rgb8(res) if j.flags & spt.DENOISE_OUT_RGB8 else res, out)


@pytest.fixture(scope="module")
def cube():
    _util.ensure_cpu_build()
    sc = spt.load_scene(os.path.join(_util.SCENES, "cfg2_cube.json"))
    yield sc
    sc.close()


def _whole(w=W, h=H, flags=0, first=0, moments=True, buckets=0, scene_name="cfg2_cube.json"):
    """The whole-image film of the plan: one NumpyFilm over every row."""
    f = NumpyFilm(_plan_samples(scene_name, flags, w, h), np.arange(h), SPP, first, moments)
    if buckets:
        assert f.buckets(buckets) == 0
    return f


def _multi(cube, n, stub=None, devices=None):
    stub = stub or StubFilms()
    replicas = StubDevices(cube)
    md = spt.MultiDevice(cube, devices or list(range(n)), api=replicas.api)
    md.replicas = replicas        # (keeps the callbacks alive as long as the MultiDevice)
    return md, stub


def _words(a, b):
    assert _util.same_words(a, b), int((a.view(np.uint32) != b.view(np.uint32)).sum())


def _compare_read_outs(film, want, buckets=True):
    assert film.samples == want.done
    for got, what in ((film.mean(), 0), (film.sum(), 1), (film.sum_sq(), 2), (film.variance_of_mean(), 3)):
        assert got.shape == (want.s.shape[0], want.s.shape[1], 3)
        _words(got, want.read(what))
    assert np.array_equal(film.sample_counts(), want.counts())
    assert np.array_equal(film.read_rgb8("mean"), want.rgb8(0))
    if buckets:
        _words(film.robust_mean("mon"), want.robust(0))
        _words(film.robust_mean("gmon"), want.robust(1))
        assert np.array_equal(film.read_rgb8("mon"), want.rgb8(1)) and np.array_equal(film.read_rgb8("gmon"), want.rgb8(2))


@pytest.mark.parametrize("strip", [1, 4, 16])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_every_layout_reads_out_the_whole_film(cube, n, strip):
    md, stub = _multi(cube, n)
    want = _whole(buckets=5)
    with md.progressive(_tracer(), spt.OutputConfig(W, H), strip_rows=strip, moments=True, buckets=5, film_api=stub.api) as film:
        assert stub.created == n and sorted(f.shard for f in stub.films.values()) == [(k, n, strip) for k in range(n)]
        for inc in (5, 7):
            film.render(inc)
            assert want.render(inc) == 0
            _compare_read_outs(film, want)
        assert len(set(stub.threads.values())) == n            # one persistent worker per shard
    assert stub.destroyed == n and not stub.films
    md.close()


@pytest.mark.parametrize("w,h,strip,n", [(9, 1, 16, 4), (5, 3, 2, 4), (7, 2, 0, 3)])
def test_more_devices_than_strips_and_one_row_images(cube, w, h, strip, n):
    md, stub = _multi(cube, n)
    want = _whole(w, h, buckets=3)
    with md.progressive(_tracer(), spt.OutputConfig(w, h), strip_rows=strip, moments=True, buckets=3, film_api=stub.api) as film:
        assert any(len(f.rows) == 0 for f in stub.films.values()) or strip == 0
        film.render(6)
        want.render(6)
        _compare_read_outs(film, want)
        assert film.adapt(0.05, 0.0, 2) == want.adapt(0.05, 0.0, 2)[1]
    md.close()


def test_adaptive_counts_are_the_single_films(cube):
    md, stub = _multi(cube, 3)
    want = _whole()
    with md.progressive(_tracer(), spt.OutputConfig(W, H), strip_rows=4, moments=True, film_api=stub.api) as film:
        for inc in (5, 7):
            film.render(inc)
            want.render(inc)
            active = film.adapt(0.05, 0.0, 2)
            assert active == want.adapt(0.05, 0.0, 2)[1] == sum(int(f.active.sum()) for f in stub.films.values())
            assert 0 < active < W * H                        # the black background retires, the cube's edges do not
        counts = film.sample_counts()
        assert set(np.unique(counts)) == {5, 12} and np.array_equal(counts, want.counts())
        _compare_read_outs(film, want, buckets=False)
    md.close()


def test_buckets_with_a_first_sample(cube):
    md, stub = _multi(cube, 2)
    want = _whole(first=5, buckets=3, moments=False)
    with md.progressive(_tracer(), spt.OutputConfig(W, H), strip_rows=4, first_sample=5, buckets=3, film_api=stub.api) as film:
        assert all(f.first == 5 and len(f.b) == 3 and not f.moments for f in stub.films.values())
        for inc in (5, 7):
            film.render(inc)
            want.render(inc)
        for est in (0, 1):
            _words(film.robust_mean("mon" if est == 0 else "gmon"), want.robust(est))
            assert np.array_equal(film.read_rgb8("mon" if est == 0 else "gmon"), want.rgb8(est + 1))
        _words(film.mean(), want.read(0))
        with pytest.raises(spt.SptError) as e:                 # a refusal of the shards (no moments), with their status
            film.variance_of_mean()
        assert e.value.status == INVALID and "device 0 (shard 0 of 2)" in str(e.value)
        _words(film.sum(), want.read(1))                       # ... leaves the multi film usable
    md.close()


def test_denoise_gathers_the_whole_films_arrays(cube):
    md, stub = _multi(cube, 3)
    r, cfg = _tracer(), spt.OutputConfig(W, H)
    whole = [_whole(), _whole(flags=spt.RENDER_DEBUG_NORMAL), _whole(flags=spt.RENDER_AOV_ALBEDO)]
    films = [md.progressive(r, cfg, strip_rows=4, moments=True, flags=fl, film_api=stub.api) for fl in (0, spt.RENDER_DEBUG_NORMAL, spt.RENDER_AOV_ALBEDO)]
    for film, want, n in zip(films, whole, (12, 4, 4)):
        film.render(n)
        want.render(n)
    film, guide, albedo = films
    film.adapt(0.05, 0.0, 2)                                    # per-pixel counts enter the gathered variance
    whole[0].adapt(0.05, 0.0, 2)
    (m, v), (g, u), (al, ua) = [(w.read(0), w.read(3)) for w in whole]
    assert (al != 0).any() and not _util.same_words(g, m)
    got = film.denoise_job(guide, albedo, iterations=2)
    call = stub.denoise_calls[-1]
    for name, want in (("m", m), ("v", v), ("g", g), ("u", u), ("al", al), ("ua", ua)):
        _words(call[name], want)
    assert call["iterations"] == 2 and call["flags"] == 0 and call["scene"] in (1001, 1002, 1003)
    _words(got, J.denoise_job(m, v, g, u, al, ua, iterations=2))
    got8 = film.denoise_job(albedo=albedo, demodulate=True, rgb8=True, iterations=1, k_albedo=0.5)
    call = stub.denoise_calls[-1]
    assert call["g"] is None and call["flags"] == 3 and call["k_albedo"] == 0.5
    assert got8.dtype == np.uint8 and np.array_equal(got8, spt.film_to_rgb8(J.denoise_job(m, v, al=al, ua=ua, demodulate=True, iterations=1, k_albedo=0.5)))
    _words(film.denoise_job(iterations=1), J.denoise_job(m, v, iterations=1))
    assert stub.denoise_calls[-1]["g"] is None and stub.denoise_calls[-1]["al"] is None
    with pytest.raises(spt.SptError) as e:
        film.read_rgb8("denoised")
    assert e.value.status == INVALID and "spt_host_multi_film_denoise" in str(e.value)
    md.close()                                                  # closes the three films first
    assert stub.destroyed == 9 and not stub.films


def test_a_failed_shard_breaks_the_film_and_names_its_device(cube):
    stub = StubFilms(fail_render_shard=1)
    md, _ = _multi(cube, 3, stub, devices=[4, 5, 6])
    film = md.progressive(_tracer(), spt.OutputConfig(W, H), strip_rows=4, moments=True, film_api=stub.api)
    with pytest.raises(spt.SptError) as e:
        film.render(5)
    assert e.value.status == HIP_ERROR and "device 5 (shard 1 of 3)" in str(e.value) and "induced" in str(e.value)
    stub.fail_render_shard = None
    for call in (lambda: film.render(1), lambda: film.samples, film.mean, film.sample_counts, lambda: film.adapt(0.1), film.robust_mean,
                 film.read_rgb8, film.denoise_job):
        with pytest.raises(spt.SptError) as e:
            call()
        assert e.value.status == INVALID and "broken" in str(e.value) and "device 5 (shard 1 of 3)" in str(e.value), str(e.value)
    # a healthy film refuses a broken guide
    other = md.progressive(_tracer(), spt.OutputConfig(W, H), strip_rows=4, moments=True, film_api=stub.api)
    other.render(2)
    with pytest.raises(spt.SptError) as e:
        other.denoise_job(guide=film)
    assert "broken" in str(e.value)
    film.close()
    other.close()
    assert stub.created == stub.destroyed == 6
    md.close()


def test_a_call_every_shard_refuses_leaves_the_film_as_it_was(cube):
    md, stub = _multi(cube, 2)
    want = _whole()
    with md.progressive(_tracer(), spt.OutputConfig(W, H), strip_rows=4, moments=True, film_api=stub.api) as film:
        film.render(5)
        want.render(5)
        with pytest.raises(spt.SptError) as e:
            film.render(SPP)                                    # past the plan's spp: every shard refuses
        assert e.value.status == INVALID and "device 0 (shard 0 of 2)" in str(e.value)
        with pytest.raises(spt.SptError) as e:
            film.robust_mean()                                  # no buckets
        assert e.value.status == INVALID
        film.render(7)
        want.render(7)
        _compare_read_outs(film, want, buckets=False)
    md.close()


def test_a_refused_create_leaves_no_film_behind(cube):
    md, stub = _multi(cube, 3)
    cfg = spt.OutputConfig(W, H)
    wide = spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=SPP, seed=7, filter_radius=1.2)
    with pytest.raises(spt.SptError) as e:
        md.progressive(wide, cfg, film_api=stub.api)
    assert e.value.status == UNSUPPORTED and "device 0 (shard 0 of 3)" in str(e.value)
    assert stub.created == stub.destroyed == 0
    for flag in (spt.RENDER_ASYNC, spt.RENDER_PROFILE, spt.RENDER_COUNT_VISITS):
        with pytest.raises(spt.SptError) as e:
            md.progressive(_tracer(), cfg, flags=flag, film_api=stub.api)
        assert e.value.status == INVALID and "ASYNC" in str(e.value)
    assert stub.created == 0
    with pytest.raises(spt.SptError) as e:
        md.progressive(_tracer(), cfg, buckets=4, film_api=stub.api)          # the shards refuse the bucket count
    assert e.value.status == INVALID and stub.created == stub.destroyed == 3 and not stub.films
    stub.fail_create_shard = 2
    with pytest.raises(spt.SptError) as e:
        md.progressive(_tracer(), cfg, film_api=stub.api)
    assert e.value.status == HIP_ERROR and "device 2 (shard 2 of 3)" in str(e.value)
    assert stub.created == stub.destroyed == 5 and not stub.films            # the two shards that did come up are released
    stub.fail_create_shard = None
    with md.progressive(_tracer(), cfg, film_api=stub.api) as film:          # the workers survive
        assert film.render(3).samples == 3
    md.close()


def test_a_guide_of_another_size_layout_or_multi_is_refused(cube):
    md, stub = _multi(cube, 2)
    md2, _ = _multi(cube, 2)
    r = _tracer()
    film = md.progressive(r, spt.OutputConfig(W, H), strip_rows=4, moments=True, film_api=stub.api).render(4)
    cases = ((md.progressive(r, spt.OutputConfig(W, H - 4), strip_rows=4, moments=True, film_api=stub.api), "width or height"),
             (md.progressive(r, spt.OutputConfig(W, H), strip_rows=2, moments=True, film_api=stub.api), "strip layout"),
             (md2.progressive(r, spt.OutputConfig(W, H), strip_rows=4, moments=True, film_api=stub.api), "another spt_host_multi"),
             (film, "the film itself"))
    for other, word in cases:
        if other is not film:
            other.render(4)
        for kw in (dict(guide=other), dict(albedo=other)):
            with pytest.raises(spt.SptError) as e:
                film.denoise_job(**kw)
            assert e.value.status == INVALID and word in str(e.value), str(e.value)
    good = md.progressive(r, spt.OutputConfig(W, H), strip_rows=4, moments=True, flags=spt.RENDER_DEBUG_NORMAL, film_api=stub.api).render(4)
    with pytest.raises(spt.SptError) as e:
        film.denoise_job(guide=good, albedo=good)
    assert "is the guide" in str(e.value)
    with pytest.raises(spt.SptError) as e:
        film.denoise_job(guide=good, demodulate=True)
    assert "albedo" in str(e.value)
    assert not stub.denoise_calls
    assert np.isfinite(film.denoise_job(guide=good, iterations=1)).all() and len(stub.denoise_calls) == 1
    md.close()
    md2.close()


def test_the_devices_may_go_before_their_films(cube):
    """A garbage collector finalises a MultiDevice and its MultiFilms in any order (and clears the weak references first): the
    library releases the shard films with the replicas, the film left behind refuses every call and can still be destroyed."""
    md, stub = _multi(cube, 3)
    film = md.progressive(_tracer(), spt.OutputConfig(W, H), moments=True, film_api=stub.api).render(3)
    handle = film._h
    md._films.clear()                                          # what the collector does to the weak references
    md.close()
    assert stub.created == stub.destroyed == 3 and not stub.films
    for call in (lambda: film.render(1), film.mean, lambda: film.samples):
        with pytest.raises(spt.SptError) as e:
            call()
        assert e.value.status == INVALID and "has been destroyed" in str(e.value)
    assert film._h.value == handle.value
    film.close()
    assert stub.destroyed == 3


def test_a_guide_is_read_through_its_own_table(cube):
    """Two multi films of one MultiDevice may come from two film tables: the gather reads each through the table it was created with."""
    md, stub = _multi(cube, 2)
    other = StubFilms()
    other.next_handle = 9000                                   # its own handles: `stub` knows none of them
    r, cfg = _tracer(), spt.OutputConfig(W, H)
    film = md.progressive(r, cfg, strip_rows=4, moments=True, film_api=stub.api).render(6)
    guide = md.progressive(r, cfg, strip_rows=4, moments=True, flags=spt.RENDER_DEBUG_NORMAL, film_api=other.api).render(4)
    assert set(stub.films).isdisjoint(other.films) and len(other.films) == 2
    want, want_g = _whole(), _whole(flags=spt.RENDER_DEBUG_NORMAL)
    want.render(6)
    want_g.render(4)
    got = film.denoise_job(guide=guide, iterations=1)
    call = stub.denoise_calls[-1]                              # the filter runs through the FILM's table
    _words(call["g"], want_g.read(0))
    _words(call["u"], want_g.read(3))
    _words(got, J.denoise_job(want.read(0), want.read(3), want_g.read(0), want_g.read(3), iterations=1))
    assert not other.denoise_calls
    md.close()


def test_hip_film_table_leaves_missing_entry_points_null(monkeypatch):
    lib = spt.hip_lib()

    class Older:                                               # a library from before spt_denoise_image
        def __getattr__(self, name):
            if name == "spt_denoise_image":
                raise AttributeError(name)
            return getattr(lib, name)
    real = spt.hip_device_film_api()
    assert real.denoise_image and real.film_create and real.size == C.sizeof(spt.DeviceFilmApi)
    monkeypatch.setattr(spt, "hip_lib", lambda: Older())
    older = spt.hip_device_film_api()
    assert older.denoise_image is None and older.film_read == real.film_read


def test_a_table_without_an_entry_is_unsupported(cube):
    stub = StubFilms(without=("film_read_robust", "denoise_image", "film_adapt"))
    md, _ = _multi(cube, 2, stub)
    with md.progressive(_tracer(), spt.OutputConfig(W, H), moments=True, buckets=3, film_api=stub.api) as film:
        film.render(4)
        for call in (film.robust_mean, film.denoise_job, lambda: film.adapt(0.1)):
            with pytest.raises(spt.SptError) as e:
                call()
            assert e.value.status == UNSUPPORTED
        assert film.read_rgb8("gmon").shape == (H, W, 3)       # the shards' own read-out is there
    short = StubFilms()
    short.api.size = spt.DeviceFilmApi.film_adapt.offset        # a caller compiled against a table that ended before film_adapt
    with md.progressive(_tracer(), spt.OutputConfig(W, H), moments=True, film_api=short.api) as film:
        film.render(4)
        assert film.sample_counts().max() == 4
        with pytest.raises(spt.SptError) as e:
            film.adapt(0.1)
        assert e.value.status == UNSUPPORTED
    md.close()


# ---- the GPU half --------------------------------------------------------------------------------------------------------------

GPU_CASES = [("cfg2_cube.json", None, 48, 32, [0, 0], 1, 0), ("cfg2_cube.json", None, 48, 32, [0, 0, 0], 4, 0),
             ("cfg2_cube.json", None, 48, 32, [0, 0, 0], 16, 0), ("t_textured.json", None, 40, 25, [0, 0], 1, 0),
             ("t_textured.json", None, 40, 25, [0, 0], 16, 0), ("t_textured.json", None, 40, 25, [0, 0, 0], 4, 5),
             ("t_textured.json", None, 40, 25, [0, 0, 0], 16, 0)]           # the last: 25 rows are two strips for three workers


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,camera,w,h,devices,strip,first", GPU_CASES)
def test_gpu_multi_film_equals_the_single_device_film(scene_name, camera, w, h, devices, strip, first):
    sc = spt.load_scene(os.path.join(_util.SCENES, scene_name))
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=24, seed=9)
    cfg = spt.OutputConfig(w, h, None, camera)
    md = spt.MultiDevice(sc, devices)
    try:
        kinds = (0, spt.RENDER_DEBUG_NORMAL, spt.RENDER_AOV_ALBEDO)
        single = [r.progressive(sc, cfg, first_sample=first, moments=True, flags=fl, buckets=5 if fl == 0 else 0) for fl in kinds]
        multi = [md.progressive(r, cfg, strip_rows=strip, first_sample=first, moments=True, flags=fl, buckets=5 if fl == 0 else 0) for fl in kinds]
        for s, m in zip(single[1:], multi[1:]):
            s.render(4)
            m.render(4)
        s, m = single[0], multi[0]
        for inc in (5, 7):
            s.render(inc)
            m.render(inc)
            assert m.samples == s.samples
            for name in ("mean", "sum", "sum_sq", "variance_of_mean"):
                _words(getattr(m, name)(), getattr(s, name)())
            for est in ("mon", "gmon"):
                _words(m.robust_mean(est), s.robust_mean(est))
            for src in ("mean", "mon", "gmon"):
                assert np.array_equal(m.read_rgb8(src), s.read_rgb8(src))
            assert m.adapt(0.05, 0.0, 2) == s.adapt(0.05, 0.0, 2)
            assert np.array_equal(m.sample_counts(), s.sample_counts())
        assert len(np.unique(s.sample_counts())) > 1                   # some pixels retired after 5 samples
        _words(m.mean(), s.mean())                                      # at the per-pixel counts
        _words(m.variance_of_mean(), s.variance_of_mean())
        _words(m.denoise_job(guide=multi[1]), s.denoise_job(guide=single[1]))
        _words(m.denoise_job(albedo=multi[2], iterations=2), s.denoise_job(albedo=single[2], iterations=2))
        got = m.denoise_job(guide=multi[1], albedo=multi[2], demodulate=True, rgb8=True)
        assert got.dtype == np.uint8 and np.array_equal(got, s.denoise_job(guide=single[1], albedo=single[2], demodulate=True, rgb8=True))
        _words(m.sum(), s.sum())                                        # the films are read only
    finally:          # in this order, whatever failed: the films of the replicas, the replicas, the scene
        md.close()
        sc.close()


@pytest.mark.gpu
def test_gpu_cli_film_devices_writes_the_same_files(tmp_path):
    exe = os.path.join(_util.PKG_DIR, "lib", "spt")
    base = [exe, "-s", os.path.join(_util.SCENES, "t_textured.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-w", "72", "-h", "50", "--spp", "16",
            "--preview-every", "4", "--adaptive", "0.05", "--adaptive-min-samples", "4", "--denoise", "--guide", "both", "--demodulate"]
    names = ("out.png", "samples.exr", "var.exr", "noisy.png", "albedo.png")
    for sub, extra in (("one", []), ("two", ["--film-devices", "0,0"]), ("three", ["--film-devices", "0,0,0", "--strip-rows", "4"])):
        d = tmp_path / sub
        d.mkdir()
        res = subprocess.run(base + ["-o", str(d / names[0]), "--samples-out", str(d / names[1]), "--variance-out", str(d / names[2]),
                                     "--noisy-out", str(d / names[3]), "--albedo-out", str(d / names[4])] + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        assert "Finished" in res.stderr
    for name in names:
        one = (tmp_path / "one" / name).read_bytes()
        assert len(one) > 100 and one == (tmp_path / "two" / name).read_bytes() == (tmp_path / "three" / name).read_bytes(), name
    assert (tmp_path / "one" / "out.png").read_bytes() != (tmp_path / "one" / "noisy.png").read_bytes()

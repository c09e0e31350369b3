"""spt_denoise_image on the device: the filter of spt_film_denoise_job on caller-provided images.

Fed with what films read out (SPT_FILM_MEAN / SPT_FILM_VAR_OF_MEAN) it has to return the bits of spt_film_denoise_job on those films,
and on any arrays the bits of the float32 restatement (tests/_denoise_job_ref.py).  The hand-made sizes are the smallest at which
the kernels take another path: 5 x 3 lies below the largest step, 16 x 16 is one tile, 33 x 17 has ragged tiles in both directions,
1 x 40 is a sliver one pixel wide."""
import ctypes as C
import os

import numpy as np
import pytest

import _denoise_job_ref as J
import _util

pytestmark = pytest.mark.gpu

INVALID = 1
f32 = np.float32


@pytest.fixture(scope="module")
def spt():
    pkg = _util.load_pkg()
    _util.ensure_cpu_build()
    return pkg


def _words(a, b):
    assert _util.same_words(a, b), int((a.view(np.uint32) != b.view(np.uint32)).sum())


def _films(spt, scene_name, camera, w, h, n, adaptive):
    """A scene with a colour film, a first-hit normal film and an albedo film of one plan, n samples each."""
    sc = spt.load_scene(os.path.join(_util.SCENES, scene_name))
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=16, seed=5)
    cfg = spt.OutputConfig(w, h, None, camera)
    film, guide, albedo = r.progressive(sc, cfg, moments=True), r.guide_film(sc, cfg), r.albedo_film(sc, cfg)
    guide.render(n)
    albedo.render(n)
    if adaptive:       # retire the converged pixels after two samples: the read-outs follow per-pixel counts
        film.render(2)
        assert 0 < film.adapt(0.05, 0.0, 2) < w * h
        film.render(n - 2)
        assert len(np.unique(film.sample_counts())) == 2
    else:
        film.render(n)
    return sc, film, guide, albedo


# (guide, albedo, demodulate, rgb8, iterations)
COMBOS = [(False, False, False, False, 1), (True, False, False, False, 5), (False, True, False, False, 2), (True, True, False, False, 5),
          (True, True, True, False, 2), (False, True, True, True, 1), (True, False, False, True, 5)]


@pytest.mark.parametrize("scene_name,camera,w,h,n,adaptive", [("cfg2_cube.json", None, 48, 32, 4, True), ("t_textured.json", None, 40, 25, 6, False)])
def test_images_from_films_give_the_bits_of_the_film_call(spt, scene_name, camera, w, h, n, adaptive):
    sc, film, guide, albedo = _films(spt, scene_name, camera, w, h, n, adaptive)
    sums = [(f.sum(), f.sum_sq()) for f in (film, guide, albedo)]
    m, v = film.mean(), film.variance_of_mean()
    g, u = guide.mean(), guide.variance_of_mean()
    al, ua = albedo.mean(), albedo.variance_of_mean()
    for use_g, use_a, demod, rgb8, its in COMBOS:
        got = spt.denoise_image(sc, m, v, guide=(g, u) if use_g else None, albedo=(al, ua) if use_a else None, demodulate=demod, rgb8=rgb8, iterations=its)
        want = film.denoise_job(guide if use_g else None, albedo if use_a else None, demodulate=demod, rgb8=rgb8, iterations=its)
        ref = J.denoise_job(m, v, g if use_g else None, u if use_g else None, al if use_a else None, ua if use_a else None, demodulate=demod, iterations=its)
        if rgb8:
            assert got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(got, spt.film_to_rgb8(ref))
        else:
            _words(got, want)
            _words(got, ref)
    assert not _util.same_words(spt.denoise_image(sc, m, v), m)                       # it does filter
    # a DeviceScene names the device as well, and other parameters arrive
    kw = dict(iterations=3, k_color=1.5, k_guide=0.7, eps_color=1e-6, eps_guide=2e-2, k_albedo=0.8, eps_albedo=3e-2, eps_demod=5e-2)
    _words(spt.denoise_image(sc.device_scene(0), m, v, (g, u), (al, ua), demodulate=True, **kw), J.denoise_job(m, v, g, u, al, ua, demodulate=True, **kw))
    for f, (s, q) in zip((film, guide, albedo), sums):                                # the films are untouched
        _words(f.sum(), s)
        _words(f.sum_sq(), q)
    sc.close()


def _hand_made(w, h, seed):
    """Six images with everything the filter has to survive planted in them."""
    rng = np.random.default_rng(seed)
    shape = (h, w, 3)
    # smooth images with an edge, plus noise of about the stated variance: most taps pass the three distance terms
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    wave = lambda fx, fy, ph: 0.5 + 0.3 * np.sin(fx * x + fy * y + ph)[..., None] * np.array([1.0, 0.8, 0.6])
    edge = (x + y > 0.6 * (w + h) / 2)[..., None]
    v = (rng.uniform(0.01, 0.08, shape) ** 2).astype(f32)
    m = (wave(0.21, 0.13, 0.0) + 0.5 * edge + rng.normal(size=shape) * np.sqrt(v)).astype(f32)
    u = rng.uniform(1e-4, 1e-3, shape).astype(f32)
    g = (wave(0.11, 0.17, 1.0) * ~edge + 0.2 * edge + rng.normal(size=shape) * np.sqrt(u)).astype(f32)
    ua = rng.uniform(1e-4, 1e-3, shape).astype(f32)
    al = np.abs(wave(0.19, 0.07, 2.0) * 0.9 + 0.05 + rng.normal(size=shape) * np.sqrt(ua)).astype(f32)
    flat = lambda a: a.reshape(-1, 3)
    n = w * h
    pick = rng.permutation(n)
    bad = dict(inf_var=pick[0:max(1, n // 9)], nan=pick[n // 9 + 1:n // 9 + 1 + max(1, n // 11)])
    flat(v)[bad["inf_var"]] = np.inf                 # one-sample pixels
    flat(m)[bad["nan"], 1] = np.nan                  # a NaN colour
    rest = pick[n // 9 + 1 + max(1, n // 11):]
    flat(m)[rest[0::7], 2] = f32(-0.0)
    flat(al)[rest[1::7], 0] = f32(-0.3)              # a negative albedo: the floor
    flat(al)[rest[2::7]] = f32(1e-3)                 # below eps_demod
    flat(al)[rest[3::11], 1] = np.nan                # a NaN albedo gives the floor too (and no tap passes it)
    flat(u)[rest[4::13], 0] = np.inf
    return (m, v, g, u, al, ua), bad


@pytest.fixture(scope="module")
def cube_scene(spt):
    sc = spt.load_scene(os.path.join(_util.SCENES, "cfg2_cube.json"))
    yield sc
    sc.close()


@pytest.mark.parametrize("w,h", [(5, 3), (16, 16), (33, 17), (1, 40)])
def test_hand_made_arrays_equal_the_restatement(spt, cube_scene, w, h):
    (m, v, g, u, al, ua), bad = _hand_made(w, h, 100 * w + h)
    for use_g, use_a, demod, its in ((True, True, True, 5), (True, True, False, 3), (False, False, False, 5), (True, False, False, 1), (False, True, True, 2)):
        kw = dict(guide=(g, u) if use_g else None, albedo=(al, ua) if use_a else None, demodulate=demod, iterations=its)
        got = spt.denoise_image(cube_scene, m, v, **kw)
        ref = J.denoise_job(m, v, g if use_g else None, u if use_g else None, al if use_a else None, ua if use_a else None, demodulate=demod, iterations=its)
        _words(got, ref)
        assert np.array_equal(spt.denoise_image(cube_scene, m, v, rgb8=True, **kw), spt.film_to_rgb8(ref))
        # non-finite pixels pass through and poison nobody
        flat, fm = got.reshape(-1, 3), m.reshape(-1, 3)
        nan_px = np.zeros(w * h, bool)
        nan_px[bad["nan"]] = True
        # (a pixel whose ALBEDO is NaN is ok(p) by the specification, fails every tap, its own included, and divides 0 by 0)
        lost = np.isnan(al).any(axis=-1).reshape(-1) & use_a
        assert lost.any() or not use_a
        assert np.isfinite(flat[~nan_px & ~lost]).all() and np.isnan(flat[lost]).all()
        assert np.isnan(flat[nan_px, 1]).all() and np.isfinite(flat[nan_px][:, (0, 2)]).all()
        if not demod:
            _words(flat[bad["inf_var"]], fm[bad["inf_var"]])
            _words(flat[nan_px], fm[nan_px])
    assert got.shape == (h, w, 3)


def test_a_bezier_scene_forwards_the_call(spt):
    sc, film, guide, albedo = _films(spt, "t_bezier.json", "main", 24, 16, 4, False)
    m, v, g, u, al, ua = film.mean(), film.variance_of_mean(), guide.mean(), guide.variance_of_mean(), albedo.mean(), albedo.variance_of_mean()
    got = spt.denoise_image(sc, m, v, (g, u), (al, ua), demodulate=True, iterations=3)
    _words(got, film.denoise_job(guide, albedo, demodulate=True, iterations=3))
    _words(got, J.denoise_job(m, v, g, u, al, ua, demodulate=True, iterations=3))
    assert np.array_equal(spt.denoise_image(sc, m, v, rgb8=True), film.denoise_job(rgb8=True))
    # a refusal comes back through the forwarded library with its message
    with pytest.raises(spt.SptError) as e:
        spt.denoise_image(sc, m, v, iterations=9)
    assert e.value.status == INVALID and "iterations" in str(e.value)
    sc.close()


def test_refusals_leave_the_next_good_call_unchanged(spt, cube_scene):
    lib = spt.hip_lib()
    ds = cube_scene.device_scene(0)
    (m, v, g, u, al, ua), _ = _hand_made(20, 18, 7)
    good = spt.denoise_image(cube_scene, m, v, (g, u), (al, ua), demodulate=True)
    P = lambda a: a.ctypes.data
    dp = spt.DenoiseParams(C.sizeof(spt.DenoiseParams), 5, 2.0, 1.0, 1e-8, 1e-2)

    def job(**kw):
        d = dict(size=C.sizeof(spt.ImageDenoiseJob), flags=1, width=20, rows=18, mean=P(m), var=P(v), guide_mean=P(g), guide_var=P(u), albedo_mean=P(al),
                 albedo_var=P(ua), params=C.pointer(dp), k_albedo=1.0, eps_albedo=1e-2, eps_demod=1e-2, pad=0)
        d.update(kw)
        return spt.ImageDenoiseJob(**d)

    def params(**kw):
        d = dict(size=C.sizeof(spt.DenoiseParams), iterations=5, k_color=2.0, k_guide=1.0, eps_color=1e-8, eps_guide=1e-2)
        d.update(kw)
        return C.pointer(spt.DenoiseParams(**d))

    out = np.full((18, 20, 3), 7.0, dtype=f32)
    nan, inf = float("nan"), float("inf")
    refused = [job(mean=None), job(var=None), job(guide_var=None), job(guide_mean=None), job(albedo_var=None), job(albedo_mean=None),
               job(size=spt.ImageDenoiseJob.k_albedo.offset - 4), job(size=0), job(flags=4), job(flags=1 | 8),
               job(flags=1, albedo_mean=None, albedo_var=None),
               job(params=params(size=8)), job(params=params(iterations=0)), job(params=params(iterations=9)), job(params=params(k_color=nan)),
               job(params=params(k_guide=0.0)), job(params=params(eps_color=-1.0)), job(params=params(eps_guide=inf)),
               job(k_albedo=0.0), job(eps_albedo=nan), job(eps_demod=-1e-2)]
    for k, j in enumerate(refused):
        assert lib.spt_denoise_image(ds._h, C.byref(j), P(out)) == INVALID, k
        assert lib.spt_last_error().decode() != "", k
        assert (out == 7.0).all(), k
        if k % 5 == 0:
            _words(spt.denoise_image(cube_scene, m, v, (g, u), (al, ua), demodulate=True), good)
    assert lib.spt_denoise_image(None, C.byref(job()), P(out)) == INVALID and lib.spt_denoise_image(ds._h, None, P(out)) == INVALID
    assert lib.spt_denoise_image(ds._h, C.byref(job()), None) == INVALID
    # an empty image is no error and writes nothing
    for kw in (dict(width=0), dict(rows=0)):
        j = job(**kw)
        assert lib.spt_denoise_image(ds._h, C.byref(j), P(out)) == 0 and (out == 7.0).all()
    # a struct that ends before the three floats takes their defaults
    short = job(size=spt.ImageDenoiseJob.k_albedo.offset, k_albedo=55.0, eps_albedo=55.0, eps_demod=55.0)
    assert lib.spt_denoise_image(ds._h, C.byref(short), P(out)) == 0
    _words(out, good)
    _words(spt.denoise_image(cube_scene, m, v, (g, u), (al, ua), demodulate=True), good)

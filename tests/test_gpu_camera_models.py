"""Camera models on the device (spt_render_camera, spt_film_create_camera, k_primary_cam).

1. The general kernel against the oracle: under SPT_CAMERA_GENERAL=1 the pinhole goes through k_primary_cam and must give the
   oracle's film word for word; a thin lens of radius 0 focused at 2 * hc is the pinhole too (its rays have the pinhole's bits, which
   the test asserts on the CPU first) and must give that film without the switch.
2. Real parameters against the existing integrator: the kept samples of a film of the model equal spt_radiance (unchanged code) over
   the rays of tests/_camera_ref.py, sample by sample, word for word.  test_gpu_radiance.py holds spt_radiance to the oracle on a
   pinhole's rays only, so the tie to the oracle for these rays is test_kept_samples_equal_the_oracles_radiance_over_the_reference_rays
   (oracle_radiance over the same rays) and, for spt_radiance itself, tests/test_gpu_radiance_anywhere.py.
3. Film semantics on films of a model.  4. An independent pin of the orthographic model.  5. Refusals.  6. The command-line program.
Every comparison is word for word with NaN counted equal (_util.same_words)."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import _camera_ref
import _denoise_job_ref
import _filter_ref
import _radiance_ref
import _robust_ref
import _util
import _wide_film_ref

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32
W, H, DEPTH, SEED = 40, 24, 5, 7
SAMPLERS = {"random": spt.SAMPLER_RANDOM, "jittered": spt.SAMPLER_JITTERED, "recurrence": spt.SAMPLER_RECURRENCE}
CAMERAS = {"cfg2_cube.json": None, "t_materials.json": "main", "t_textured.json": None, "t_medium.json": None, "t_bezier.json": "main",
           "cfg1_sphere.json": None}
SWITCH = "SPT_CAMERA_GENERAL"
INVALID, UNSUPPORTED = 1, 4


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)


@functools.lru_cache(maxsize=None)
def _scene(name):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_util.SCENES, name))


def _tracer(sampler="recurrence", spp=8, **kw):
    return spt.PathTracer(max_depth=DEPTH, sampler=SAMPLERS[sampler], spp=spp, division_x=4, division_y=2, seed=SEED, **kw)


def _cfg(name, w=W, h=H):
    return spt.OutputConfig(w, h, None, CAMERAS[name])


def _cam(name):
    return _scene(name).get_camera(CAMERAS[name])


def _same(a, b, what=""):
    assert a.shape == b.shape, what
    bad = ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    assert _util.same_words(a, b), "%s: %d of %d words differ" % (what, int(bad.sum()), bad.size)


def _pinhole_lens(cam):
    """Radius 0, focus 2 * hc: ft == 2.0f, and the power-of-two scale leaves normalize bit-invariant."""
    return spt.CameraModel.thin_lens(cam, 0.0, float(f32(2) * f32(cam.half_cot_half_fov)))


def _models(name):
    """Thin lens (radius 0.15, focused at the world origin's depth, where the scenes stand), an orthographic view of about the pinhole's
    framing there, and a panorama from the camera's eye."""
    cam = _cam(name)
    eye, fwd = np.array(cam.eye[:], dtype=np.float64), np.array(cam.forward[:], dtype=np.float64)
    focus = max(float(np.dot(-eye, fwd)), 1.0)
    return {"thin_lens": spt.CameraModel.thin_lens(cam, 0.15, focus),
            "orthographic": spt.CameraModel.orthographic(cam, focus / float(cam.half_cot_half_fov)),
            "panorama": spt.CameraModel.panorama(cam.eye[:])}


@functools.lru_cache(maxsize=None)
def _oracle(name, sampler, spp):
    film, _ = _util.oracle_render(_scene(name), _tracer(sampler, spp), W, H, camera=CAMERAS[name], flags=_util.device_oracle_flags())
    film.setflags(write=False)
    return film


def _info(sc, what=8):
    return sc.device_scene(0).render_info(what)


# ---- 1. oracle anchor, general kernel ----------------------------------------------------------------------------------------------

def _anchor(sc, name, sampler, spp, spp_pass, monkeypatch):
    want = _oracle(name, sampler, spp)
    assert np.isfinite(want).any() and want[np.isfinite(want)].max() > 0.05
    r, cfg, cam = _tracer(sampler, spp), _cfg(name), sc.get_camera(CAMERAS[name])
    lens = _pinhole_lens(cam)
    # precondition, on the CPU: the lens model's rays for this plan have the pinhole plan's bits (no signed-zero corner case)
    if sampler == "jittered":
        # tests/_wide_film_ref.offsets has no jittered sampler, so the restated specification cannot make this plan's screen points: both sides
        # are the host generator here, code under test.  This case guards against a signed zero only; the specification is checked by the others
        a, b = spt.camera_rays(lens, r, W, H, aux=True), spt.camera_rays(spt.CameraModel.perspective(cam), r, W, H, aux=True)
    else:
        a, b = _camera_ref.plan_rays(spt, lens, r, W, H, 0, spp, aux=True), _radiance_ref.plan_rays(spt, sc, r, W, H, 0, spp, camera=CAMERAS[name], aux=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    before = _info(sc)
    monkeypatch.setenv(SWITCH, "1")
    got = r.render_shard(sc, cfg, samples_per_pass=spp_pass).copy()
    monkeypatch.delenv(SWITCH)
    mid = _info(sc)
    assert mid > before, "SPT_CAMERA_GENERAL=1 did not reach k_primary_cam"
    _same(got, want, "%s under SPT_CAMERA_GENERAL=1" % name)
    _same(r.render_shard(sc, cfg, samples_per_pass=spp_pass, camera_model=lens), want, "%s through the pinhole lens" % name)
    after = _info(sc)
    assert after - mid == (1 if spp_pass == 0 else -(-spp // spp_pass))   # one per pass
    _same(r.render_shard(sc, cfg, samples_per_pass=spp_pass), want, "%s, the pinhole path" % name)
    assert _info(sc) == after   # the pinhole's own kernels do not count


@pytest.mark.parametrize("name,sampler,spp_pass", [
    ("cfg2_cube.json", "recurrence", 0),     # fused
    ("cfg2_cube.json", "random", 0),
    ("cfg2_cube.json", "jittered", 0),
    ("cfg2_cube.json", "recurrence", 3),     # passes of 3, 3, 2
    ("t_materials.json", "recurrence", 0),   # un-fused, class queues, environment
    ("t_materials.json", "random", 3),
    ("t_textured.json", "recurrence", 0),    # auxiliary rays per slot
    ("t_textured.json", "random", 3),
    ("t_medium.json", "recurrence", 0),
])
def test_general_kernel_gives_the_oracles_film(name, sampler, spp_pass, monkeypatch):
    _anchor(_scene(name), name, sampler, 8, spp_pass, monkeypatch)


@pytest.mark.parametrize("no_stream", [False, True], ids=["streaming", "memory"])
@pytest.mark.parametrize("name", ["t_materials.json", "t_textured.json"])
def test_general_kernel_with_the_geometry_in_memory(name, no_stream, monkeypatch):
    monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    if no_stream:
        monkeypatch.setenv("SPT_NO_STREAM", "1")
    sc = spt.load_scene(os.path.join(_util.SCENES, name))   # (a scene of its own: the switches are read at creation)
    try:
        _anchor(sc, name, "recurrence", 8, 3, monkeypatch)
    finally:
        sc.close()


# ---- 2. real parameters equal the existing integrator ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _samples(name, kind, sampler="random", spp=4, w=W, h=H, flags=0):
    """(rays, aux, offsets, radiance): the model's plan from tests/_camera_ref.py and spt_radiance's colour of every sample, (spp, h, w, 3)."""
    sc, r, m = _scene(name), _tracer(sampler, spp), _models(name)[kind]
    rays, aux = _camera_ref.plan_rays(spt, m, r, w, h, 0, spp, aux=True)
    rgb = sc.device_scene(0).radiance(rays.reshape(-1), aux=aux.reshape(-1), max_depth=DEPTH, seed=SEED, rng_skip=_radiance_ref.rng_skip(spt, r))
    rgb = rgb.reshape(spp, h, w, 3)
    rgb.setflags(write=False)
    return rays, aux, rgb


@pytest.mark.parametrize("kind", ["thin_lens", "orthographic", "panorama"])
@pytest.mark.parametrize("name", ["cfg2_cube.json", "t_materials.json", "t_textured.json", "t_bezier.json"])
def test_kept_samples_equal_radiance_over_the_reference_rays(name, kind):
    sc, r = _scene(name), _tracer("random", 4)
    _, _, want = _samples(name, kind)
    assert np.isfinite(want).any() and want[np.isfinite(want)].max() > 0.01 and len(np.unique(want.view(np.uint32))) > 2
    before = _info(sc)
    with r.progressive(sc, _cfg(name), keep_samples=True, camera_model=_models(name)[kind]) as film:
        film.render(1)
        film.render(3)
        _same(film.kept(), want, "%s, %s" % (name, kind))
    assert _info(sc) > before
    # ... and the model matters: the pinhole's samples are other samples
    with r.progressive(sc, _cfg(name), keep_samples=True) as film:
        assert not _util.same_words(film.render(4).kept(), want)


@pytest.mark.parametrize("kind", ["thin_lens", "orthographic", "panorama"])
@pytest.mark.parametrize("name", ["t_materials.json", "t_textured.json"])
def test_kept_samples_equal_the_oracles_radiance_over_the_reference_rays(name, kind):
    """No device call on the expected side: oracle_radiance (trace_ray on caller rays) over the same restated rays and auxiliary rays."""
    sc, r = _scene(name), _tracer("random", 4)
    rays, aux, _ = _samples(name, kind)
    want = _util.oracle_radiance(sc, rays.reshape(-1), aux.reshape(-1), max_depth=DEPTH, seed=SEED, rng_skip=_radiance_ref.rng_skip(spt, r),
                                 flags=_util.device_oracle_flags()).reshape(4, H, W, 3)
    flat = want.reshape(-1, 3)
    lit = np.isfinite(flat).all(axis=-1) & (flat != 0).any(axis=-1)
    assert lit.mean() >= 0.25 and len(np.unique(flat[lit], axis=0)) >= 100
    with r.progressive(sc, _cfg(name), keep_samples=True, camera_model=_models(name)[kind]) as film:
        _same(film.render(4).kept(), want, "%s, %s, against the oracle" % (name, kind))


# ---- 3. film semantics -------------------------------------------------------------------------------------------------------------

def _sum_in_order(xs):
    s = np.zeros(xs.shape[1:], dtype=f32)
    for x in xs:
        s = s + x
    return s


@pytest.mark.parametrize("name,kind", [("t_materials.json", "thin_lens"), ("cfg2_cube.json", "orthographic"), ("t_textured.json", "panorama")])
def test_increments_render_and_shards(name, kind):
    sc, r, m, cfg = _scene(name), _tracer("random", 8), _models(name)[kind], _cfg(name)
    _, _, xs = _samples(name, kind, "random", 8)
    want_sum = _sum_in_order(xs)
    want_mean = (want_sum * (f32(1) / f32(8))).astype(f32)
    with r.progressive(sc, cfg, moments=True, camera_model=m) as film:
        film.render(3)
        _same(film.sum(), _sum_in_order(xs[:3]), "3 samples")
        film.render(5)
        _same(film.sum(), want_sum, "3 + 5")
        _same(film.mean(), want_mean, "mean")
    with r.progressive(sc, cfg, camera_model=m, samples_per_pass=3) as film:
        _same(film.render(8).sum(), want_sum, "one increment, passes of 3")
    whole = r.render_shard(sc, cfg, camera_model=m).copy()
    _same(whole, want_mean, "spt_render_camera")
    _same(r.render_shard(sc, cfg, camera_model=m, profile=True), want_mean, "SPT_RENDER_PROFILE")
    # two shards with strip_rows = 4, interleaved
    both = np.zeros((H, W, 3), dtype=f32)
    for k in range(2):
        r.render_shard(sc, cfg, shard_index=k, shard_count=2, strip_rows=4, camera_model=m, film=both)
    _same(both, whole, "two shards")
    with r.progressive(sc, cfg, shard_index=1, shard_count=2, strip_rows=4, camera_model=m) as film:
        _same(film.render(8).mean(), whole[spt.shard_rows(H, 1, 2, 4)], "a film of shard 1")
    # asynchronous frames
    buf = r.render_shard(sc, cfg, camera_model=m, reuse_output=True)
    for _ in range(3):
        r.render_shard(sc, cfg, camera_model=m, reuse_output=True, wait=False)
    r.wait(sc)
    _same(np.array(buf), whole, "wait=False frames")
    # max_depth 0: every sample is black
    r0 = spt.PathTracer(max_depth=0, sampler=spt.SAMPLER_RANDOM, spp=8, seed=SEED)
    assert not r0.render_shard(sc, cfg, camera_model=m).any()


def test_box_radius_one_and_tent_filter():
    name, kind = "t_materials.json", "thin_lens"
    sc, m, cfg = _scene(name), _models(name)[kind], _cfg(name)
    _, _, xs = _samples(name, kind, "random", 8)
    off = _wide_film_ref.offsets(spt, SEED, W, H, 8, spt.SAMPLER_RANDOM, 0, 8)
    r = _tracer("random", 8, filter_radius=1.0)
    _, _, mean = _wide_film_ref.filter_film(xs, off, 1.0)
    _same(r.render_shard(sc, cfg, camera_model=m), mean, "spt_render_camera, box radius 1 (the band path)")
    with r.progressive(sc, cfg, keep_samples=True, camera_model=m) as film:
        film.render(3)
        film.render(5)
        _same(film.mean(), mean, "sample-keeping film, box radius 1")
        film.set_filter("tent", radius=1.0)
        color, wsum, tent = _filter_ref.filter_film(xs, off, "tent", 1.0)
        assert len(np.unique(wsum)) > 3
        _same(film.sum(), color, "tent sum")
        _same(film.mean(), tent, "tent mean")


def test_adaptive_film_of_a_model():
    name, kind = "t_materials.json", "thin_lens"
    sc, r, m, cfg = _scene(name), _tracer("random", 16), _models(name)[kind], _cfg(name)
    _, _, xs = _samples(name, kind, "random", 16)
    with r.progressive(sc, cfg, moments=True, camera_model=m) as film:
        film.render(8)
        mean, sd = film.mean().astype(np.float64), np.sqrt(film.variance_of_mean().astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            need = np.max(sd / np.abs(mean), axis=-1)
        need = need[np.isfinite(need) & (need > 0)]
        active = film.adapt(float(np.quantile(need, 0.5)), 0.0, 4)
        assert 0 < active < W * H
        before = _info(sc)
        film.render(8)
        assert _info(sc) == before + 1   # the masked kernel ran
        counts = film.sample_counts()
        assert set(np.unique(counts)) == {8, 16}
        # every pixel holds the in-order sum of its first n_p samples: a retired one the bits of a plain film stopped at 8
        want = np.where((counts == 16)[..., None], _sum_in_order(xs), _sum_in_order(xs[:8]))
        _same(film.sum(), want.astype(f32), "adaptive film")


def test_buckets_robust_and_rgb8_of_a_model():
    name, kind = "t_materials.json", "orthographic"
    sc, r, m, cfg = _scene(name), _tracer("random", 16), _models(name)[kind], _cfg(name)
    _, _, xs = _samples(name, kind, "random", 16)
    with r.progressive(sc, cfg, buckets=5, camera_model=m) as film:
        film.render(7)
        film.render(9)
        b = _robust_ref.bucket_sums(xs, 0, 5)
        _same(film.bucket_sums(), b, "bucket sums")
        s = film.sum()
        _same(s, _sum_in_order(xs), "sum")
        for est, which in (("mon", _robust_ref.MON), ("gmon", _robust_ref.GMON)):
            _same(film.robust_mean(est), _robust_ref.robust(b, s, 0, 16, which), est)
        assert np.array_equal(film.read_rgb8("mean"), spt.film_to_rgb8(film.mean()))
        assert np.array_equal(film.read_rgb8("gmon"), spt.film_to_rgb8(film.robust_mean("gmon")))


def test_denoise_with_a_guide_of_the_same_model():
    name, kind = "t_materials.json", "thin_lens"
    sc, r, m, cfg = _scene(name), _tracer("random", 8), _models(name)[kind], _cfg(name)
    with r.progressive(sc, cfg, moments=True, camera_model=m) as film, \
            r.progressive(sc, cfg, moments=True, flags=spt.RENDER_DEBUG_NORMAL, camera_model=m) as guide, \
            r.progressive(sc, cfg, moments=True, flags=spt.RENDER_DEBUG_NORMAL) as pinhole_guide:
        film.render(8)
        guide.render(4)
        pinhole_guide.render(4)
        out = film.denoise(guide)
        # the filter of tests/_denoise_job_ref.py over what the two films read out: a guide of the model is a guide like any other
        _same(out, _denoise_job_ref.denoise_job(film.mean(), film.variance_of_mean(), guide.mean(), guide.variance_of_mean()), "denoise with a guide of the model")
        assert np.isfinite(out).all() and not _util.same_words(out, film.mean())
        assert not _util.same_words(out, film.denoise(pinhole_guide))   # ... and it is the guide the filter used
        assert not _util.same_words(guide.mean(), pinhole_guide.mean())   # the guide saw the scene through the lens
        assert np.array_equal(film.read_rgb8("denoised", guide), spt.film_to_rgb8(out))


# ---- 4. independent pin: an orthographic view of a sphere ---------------------------------------------------------------------------

def test_orthographic_silhouette_of_a_sphere():
    """The fraction of non-black samples of an orthographic DEBUG_NORMAL film of cfg1_sphere is pi R^2 / (view_height^2 * aspect).
    Tolerance: a sample can only be on the wrong side of the count inside a pixel whose square meets the circle's outline, so the
    number of such pixels (float64, below) over the pixel total bounds the error of the fraction.
    Measured on an MI355X: fraction 0.34930 against 0.34907, bound 0.04150 (170 outline pixels); from twice the distance the same
    fraction, with 4917 of 5723 common samples differing in some low bit of the normal (the hit point is rounded at another t), so
    only the fraction is asserted there."""
    name, n, spp, vh = "cfg1_sphere.json", 64, 4, 3.0
    sc = _scene(name)
    desc = json.load(open(os.path.join(_util.SCENES, name)))
    radius = float(desc["primitives"][0]["radius"])
    centre = np.array(desc["instances"][0]["translate"], dtype=np.float64)
    r = _tracer("recurrence", spp)
    cfg = spt.OutputConfig(n, n)

    def fraction_and_film(cam):
        with r.progressive(sc, cfg, keep_samples=True, flags=spt.RENDER_DEBUG_NORMAL, camera_model=spt.CameraModel.orthographic(cam, vh)) as film:
            kept = film.render(spp).kept()
        return float((kept != 0).any(axis=-1).mean()), kept

    cam = sc.get_camera(None)
    eye, fwd, up, right = (np.array(v[:], dtype=np.float64) for v in (cam.eye, cam.forward, cam.up, cam.right))
    cu, cv = float(np.dot(centre - eye, right)), float(np.dot(centre - eye, up))
    # pixel (i, j) covers [x0, x0 + px] x [y0, y0 + px] of the view plane; it meets the outline unless it is wholly inside or outside
    px = vh / n
    x0 = (np.arange(n) * px - vh / 2)[None, :] - cu
    y0 = ((n - 1 - np.arange(n)) * px - vh / 2)[:, None] - cv
    near = np.hypot(np.clip(0.0, x0, x0 + px), np.clip(0.0, y0, y0 + px))
    far = np.hypot(np.maximum(np.abs(x0), np.abs(x0 + px)), np.maximum(np.abs(y0), np.abs(y0 + px)))
    outline = int(((near <= radius) & (far >= radius)).sum())
    want, tol = np.pi * radius * radius / (vh * vh), outline / float(n * n)
    got, kept = fraction_and_film(cam)
    print("orthographic sphere: fraction %.5f, expected %.5f, bound %.5f (%d outline pixels)" % (got, want, tol, outline))
    assert 0.2 < want < 0.5 and tol < 0.1
    assert abs(got - want) <= tol
    # the same view from twice the distance: an orthographic image does not depend on it
    # (eye - centre has a component across the view: keep it, double only the distance along forward)
    along = float(np.dot(centre - eye, fwd))
    assert along > radius
    back = spt.make_camera(tuple(eye - fwd * along), tuple(fwd), (0.0, 1.0, 0.0), 45.0)
    got2, kept2 = fraction_and_film(back)
    both = (kept != 0).any(axis=-1) & (kept2 != 0).any(axis=-1)
    differing = int((kept.view(np.uint32) != kept2.view(np.uint32)).any(axis=-1)[both].sum())
    print("orthographic sphere at twice the distance: fraction %.5f, %d of %d common samples differ in some bit" % (got2, differing, int(both.sum())))
    assert got2 == got


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_nothing_changed():
    name = "t_materials.json"
    sc, r, cfg, cam = _scene(name), _tracer("random", 4), _cfg(name), _cam(name)
    ds = sc.device_scene(0)
    lib = spt.hip_lib()
    good = _models(name)["thin_lens"]
    before = r.render_shard(sc, cfg, camera_model=good).copy()
    info = [_info(sc, k) for k in (0, 1, 7, 8)]
    p = r.params(W, H)
    out = np.full((H, W, 3), 7.0, dtype=f32)
    small = spt.CameraModel.panorama([0, 0, 0])
    small.size -= 4
    bad = [spt.CameraModel.thin_lens(cam, -0.1, 1.0), spt.CameraModel.thin_lens(cam, float("inf"), 1.0), spt.CameraModel.thin_lens(cam, 0.1, 0.0),
           spt.CameraModel.thin_lens(cam, 0.1, float("nan")), spt.CameraModel.orthographic(cam, 0.0), spt.CameraModel.orthographic(cam, -1.0),
           spt.CameraModel.orthographic(cam, float("inf")), spt.CameraModel._make(4, cam), small]

    def both_calls(model, params, want):
        film = C.c_void_p()
        assert lib.spt_render_camera(ds._h, C.byref(model) if model is not None else None, C.byref(params), out.ctypes.data, None) == want
        assert lib.spt_film_create_camera(ds._h, C.byref(model) if model is not None else None, C.byref(params), 0, 0, C.byref(film)) == want
        assert not film.value and (out == 7.0).all()

    both_calls(None, p, INVALID)
    for m in bad:
        both_calls(m, p, INVALID)
    for flag in (spt.RENDER_COUNT_VISITS, spt.RENDER_AOV_ALBEDO):
        for kind in ("thin_lens", "orthographic", "panorama"):
            both_calls(_models(name)[kind], r.params(W, H, flags=flag), UNSUPPORTED)
    assert [_info(sc, k) for k in (0, 1, 7, 8)] == info
    _same(r.render_shard(sc, cfg, camera_model=good), before, "a render after the refusals")
    assert spt.hip_lib().spt_debug_render_info(ds._h, 9, C.byref(C.c_uint64())) == INVALID


def test_perspective_through_the_new_calls_is_the_old_calls():
    for name in ("cfg2_cube.json", "t_textured.json"):
        sc, r, cfg = _scene(name), _tracer("random", 8), _cfg(name)
        m = spt.CameraModel.perspective(_cam(name))
        want = r.render_shard(sc, cfg).copy()
        before = _info(sc)
        _same(r.render_shard(sc, cfg, camera_model=m), want, "spt_render_camera(PERSPECTIVE)")
        with r.progressive(sc, cfg, moments=True) as a, r.progressive(sc, cfg, moments=True, camera_model=m) as b:
            a.render(8)
            b.render(3)
            b.render(5)
            _same(b.sum(), a.sum(), "spt_film_create_camera(PERSPECTIVE)")
            _same(b.sum_sq(), a.sum_sq(), "its squares")
            _same(b.mean(), want, "its mean")
        assert _info(sc) == before   # the pinhole's own kernels


# ---- 6. the command-line program -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("option,film_option", [
    (["--lens-radius", "0.1", "--focus-distance", "4"], ["--preview-every", "2"]),
    (["--orthographic", "3"], ["--film-devices", "0", "--preview-every", "2"]),    # one device named through --film-devices: the film lives there
    (["--panorama"], ["--gpus", "1", "--time-limit", "1000"]),
], ids=["thin_lens", "orthographic", "panorama"])
def test_cli_hands_the_model_to_the_library(option, film_option, tmp_path):
    """`spt` with a camera-model option writes the 8-bit image of render_shard(camera_model=) - the plain run through spt_render_camera,
    a progressive run through spt_film_create_camera - and not the pinhole's."""
    name, w, h, spp, seed = "cfg2_cube.json", 48, 32, 4, 3
    scene, renderer = os.path.join(_util.SCENES, name), os.path.join(_util.SCENES, "pt.json")
    sc, cam = _scene(name), _cam(name)
    model = {"--lens-radius": lambda: spt.CameraModel.thin_lens(cam, 0.1, 4.0), "--orthographic": lambda: spt.CameraModel.orthographic(cam, 3.0),
             "--panorama": lambda: spt.CameraModel.panorama(cam.eye[:])}[option[0]]()
    ren = spt.load_renderer(renderer, seed=seed)
    ren.spp = spp
    cfg = spt.OutputConfig(w, h)
    want = spt.film_to_rgb8(ren.render_shard(sc, cfg, camera_model=model))
    assert not np.array_equal(want, spt.film_to_rgb8(ren.render_shard(sc, cfg))) and want.max() > 20
    base = [os.path.join(spt.LIB_DIR, "spt"), "-s", scene, "-r", renderer, "-w", str(w), "-h", str(h), "--spp", str(spp), "--seed", str(seed)]
    for k, extra in enumerate(([], film_option)):
        out = tmp_path / ("o%d.png" % k)
        res = subprocess.run(base + ["-o", str(out)] + option + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        assert np.array_equal(spt.read_png(str(out))[..., :3], want), " ".join(option + extra)

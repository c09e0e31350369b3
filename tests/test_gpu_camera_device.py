"""spt_camera_rays and spt_camera_gbuffer (DeviceScene.camera_rays, DeviceScene.camera_gbuffer, camera_gbuffer, `spt --gbuffer-out`): a
plan's camera rays made on the device, and the first-hit images of a camera model without the host in the loop.

Every comparison is of words (_util.same_words): no tolerance.  The plan has spp = 4 and the calls take its samples first = 1,
count = 3, so the sample stride and `first` matter.  Shapes: 37 x 19 (703 pixels: no multiple of 64, the width no multiple of 16), 1 x 1,
64 x 4 (whole waves exactly); rays_per_pass = 100 cuts inside rows and inside samples.

1. Rays: spt_camera_rays against spt_host_camera_rays (and, random and recurrence samplers, against tests/_camera_ref.py).
2. The chain: radiance and gbuffer over device-made rays.
3. Images against the oracle-side reference: the specification of include/spt_abi.h in float32 numpy over tests/_gbuffer_ref.py's
   records of tests/_camera_ref.py's rays - no device call on the expected side (the normals: over DeviceScene.gbuffer's records, as
   _gbuffer_ref has no normal for a patch hit).
4. Images against the route the call replaces: the same sums over gbuffer(camera_rays(...)).
5. Refusals.  6. Scene updates.  7. The command-line program.  8. Device pointers, in a process that imported torch first."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _anywhere_ref as ref
import _camera_ref
import _gbuffer_ref as G
import _radiance_ref
import _scene_update_scenes as SU
import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32
INVALID_ARG, UNSUPPORTED = 1, 4
PATTERN = 0xA5C3F00D
SPP, FIRST, COUNT = 4, 1, 3
W, H = 37, 19
SHAPES = [(37, 19), (1, 1), (64, 4)]
SAMPLERS = {"random": spt.SAMPLER_RANDOM, "recurrence": spt.SAMPLER_RECURRENCE, "jittered": spt.SAMPLER_JITTERED}
KINDS = ["thin_lens", "orthographic", "panorama", "perspective"]
CLI = os.path.join(spt.LIB_DIR, "spt")
IMAGES = {"albedo": 3, "normal": 3, "depth": 1, "coverage": 1}


def _tracer(sampler="random"):
    return spt.PathTracer(max_depth=ref.DEPTH, sampler=SAMPLERS[sampler], spp=SPP, division_x=2, division_y=2, seed=ref.SEED)


def _models(name):
    m = dict(ref.camera_models(name))
    m["perspective"] = spt.CameraModel.perspective(ref.scene(name).get_camera(ref.CAMERAS[name]))
    return m


def _ds(name):
    return ref.scene(name).device_scene(0)


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rays_call(ds, model, renderer, w, h, first=FIRST, count=COUNT, aux=True, per_pass=0):
    """spt_camera_rays through ctypes into arrays with four guard records behind them; (rays, aux or None), shaped (count, h, w).
    Without `aux` a second guarded array stands where the call must not write."""
    n = count * h * w
    rays = np.zeros(n + 4, dtype=spt.PATH_RAY_DTYPE)
    ax = np.zeros(n + 4, dtype=spt.RAY_AUX_DTYPE)
    _words(rays)[:] = PATTERN
    _words(ax)[:] = PATTERN
    p = renderer.params(w, h)
    job = spt.CameraRaysJob(size=C.sizeof(spt.CameraRaysJob), model=C.addressof(model), plan=C.addressof(p), first=first, count=count,
                            rays_per_pass=per_pass)
    job.rays, job.aux = rays.ctypes.data, ax.ctypes.data if aux else None
    assert spt.hip_lib().spt_camera_rays(ds._h, C.byref(job)) == 0, spt.hip_lib().spt_last_error()
    assert (_words(rays[n:]) == PATTERN).all(), "rays: written past the last record"
    assert (_words(ax[n if aux else 0:]) == PATTERN).all(), "aux: written past the last record" if aux else "aux: written without being asked for"
    return rays[:n].reshape(count, h, w), (ax[:n].reshape(count, h, w) if aux else None)


def _images_call(ds, model, renderer, w=W, h=H, first=FIRST, count=COUNT, keys=tuple(IMAGES), per_pass=0, status=0):
    """spt_camera_gbuffer through ctypes into images pre-filled with 7.0; the images asked for (`keys`), the others stay NULL."""
    out = {k: np.full((h, w, c) if c == 3 else (h, w), f32(7.0)) for k, c in IMAGES.items()}
    p = renderer.params(w, h)
    job = spt.CameraGBufferJob(size=C.sizeof(spt.CameraGBufferJob), model=C.addressof(model), plan=C.addressof(p), first=first, count=count,
                               rays_per_pass=per_pass)
    for k in keys:
        setattr(job, k, out[k].ctypes.data)
    assert spt.hip_lib().spt_camera_gbuffer(ds._h, C.byref(job)) == status, spt.hip_lib().spt_last_error()
    for k in IMAGES:
        if k not in keys or status != 0:
            assert (out[k] == f32(7.0)).all(), k
    return {k: out[k] for k in keys}


def _spec(albedo, n, t, hit):
    """The specification of spt_camera_gbuffer over the records of the samples, arrays shaped (count, h, w, ...), in float32."""
    count = albedo.shape[0]
    A, N = np.zeros(albedo.shape[1:], dtype=f32), np.zeros(n.shape[1:], dtype=f32)
    T, K = np.zeros(t.shape[1:], dtype=f32), np.zeros(t.shape[1:], dtype=np.uint32)
    for s in range(count):
        A, N = A + albedo[s], N + n[s]
        T = np.where(hit[s], T + t[s], T)
        K = K + hit[s].astype(np.uint32)
    inv = f32(1.0) / f32(count)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        depth = np.where(K > 0, T / K.astype(f32), f32(0.0))
    out = {"albedo": A * inv, "normal": N * inv, "depth": depth.astype(f32), "coverage": K.astype(f32) / f32(count)}
    assert all(v.dtype == f32 for v in out.values())
    return out


def _spec_of_records(rec):
    hit = rec["instance"] >= 0
    assert (_words(rec["albedo"][~hit]) == 0).all() and (_words(rec["n"][~hit]) == 0).all()      # a miss adds +0
    return _spec(rec["albedo"], rec["n"], rec["t"], hit)


def _same_images(got, want, what, keys=tuple(IMAGES)):
    for k in keys:
        assert got[k].dtype == f32 and got[k].shape == want[k].shape, (what, k)
        bad = _words(got[k]) != _words(want[k])
        assert _util.same_words(got[k], want[k]), "%s, %s: %d of %d words differ, first at %r: got %r, expected %r" % (
            what, k, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[k][bad][0], want[k][bad][0])


# ---- 1. rays -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("kind", KINDS)
def test_rays_are_the_host_generators(kind, sampler, shape):
    w, h = shape
    name = "t_textured"
    model, r, ds = _models(name)[kind], _tracer(sampler), _ds(name)
    want, want_aux = spt.camera_rays(model, r, w, h, FIRST, COUNT, aux=True)
    assert (want["stream_b"] == np.arange(FIRST, FIRST + COUNT, dtype=np.uint32)[:, None, None]).all() and (want["t_min"] == f32(0.0001)).all()
    assert (_words(want["pad"]) == 0).all() and all((_words(want_aux[f]) == 0).all() for f in ("pad0", "pad1", "pad2", "pad3"))
    if sampler != "jittered":      # (tests/_wide_film_ref.py has no jittered sampler): the expected side is not the host generator alone
        spec, spec_aux = _camera_ref.plan_rays(spt, model, r, w, h, FIRST, COUNT, aux=True)
        assert spec.tobytes() == want.tobytes() and spec_aux.tobytes() == want_aux.tobytes()
    if kind == "thin_lens":      # the model matters: a lens' rays are not the pinhole's
        assert not np.array_equal(_words(want["o"]), _words(spt.camera_rays(_models(name)["perspective"], r, w, h, FIRST, COUNT)["o"]))
    for per_pass in ([0, 100] if shape == (37, 19) else [0]):
        got, got_aux = _rays_call(ds, model, r, w, h, aux=True, per_pass=per_pass)
        assert got.tobytes() == want.tobytes(), "rays, rays_per_pass %d" % per_pass
        assert got_aux.tobytes() == want_aux.tobytes(), "aux, rays_per_pass %d" % per_pass
        alone, none = _rays_call(ds, model, r, w, h, aux=False, per_pass=per_pass)
        assert none is None and alone.tobytes() == want.tobytes(), "rays without aux, rays_per_pass %d" % per_pass
    # the method: the module's camera_rays, record for record; the whole plan by default
    got, got_aux = ds.camera_rays(model, r, w, h, FIRST, COUNT, aux=True)
    assert got.dtype == spt.PATH_RAY_DTYPE and got.shape == (COUNT, h, w) and got.tobytes() == want.tobytes() and got_aux.tobytes() == want_aux.tobytes()
    assert ds.camera_rays(model, r, w, h).tobytes() == spt.camera_rays(model, r, w, h).tobytes()


def test_no_samples_is_ok_and_writes_nothing():
    ds, r = _ds("cfg2_cube"), _tracer()
    rays, _ = _rays_call(ds, _models("cfg2_cube")["thin_lens"], r, W, H, first=SPP, count=0, aux=False)
    assert rays.shape == (0, H, W)


# ---- 2. the chain ----------------------------------------------------------------------------------------------------------------------

def test_radiance_over_device_rays_gives_the_films_kept_samples():
    name, kind = "t_textured", "thin_lens"
    sc, r, model, ds = ref.scene(name), _tracer(), _models(name)[kind], _ds(name)
    rays, aux = ds.camera_rays(model, r, W, H, FIRST, COUNT, aux=True)
    got = ds.radiance(rays.reshape(-1), aux=aux.reshape(-1), max_depth=ref.DEPTH, seed=ref.SEED, rng_skip=_radiance_ref.rng_skip(spt, r))
    with r.progressive(sc, spt.OutputConfig(W, H, None, ref.CAMERAS[name]), keep_samples=True, camera_model=model) as film:
        kept = film.render(SPP).kept()
    want = kept[FIRST:FIRST + COUNT]
    assert np.isfinite(want).any() and want[np.isfinite(want)].max() > 0.01 and len(np.unique(_words(want))) > 100
    assert _util.same_words(got.reshape(COUNT, H, W, 3), want)
    assert not _util.same_words(got.reshape(COUNT, H, W, 3), kept[:COUNT])      # `first` matters
    host_rays, host_aux = spt.camera_rays(model, r, W, H, FIRST, COUNT, aux=True)
    rec = ds.gbuffer(rays.reshape(-1), aux.reshape(-1))
    assert (rec["instance"] >= 0).mean() > 0.1
    assert np.array_equal(G.words(rec), G.words(ds.gbuffer(host_rays.reshape(-1), host_aux.reshape(-1))))


# ---- 3. images against the oracle-side reference ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference_records(name, kind, flags):
    """tests/_gbuffer_ref.py's records of tests/_camera_ref.py's rays of the samples FIRST .. FIRST + COUNT - 1, (COUNT, H, W); read-only.
    `flags`: the oracle configuration (cache key)."""
    assert flags == _util.device_oracle_flags()
    rays, aux = _camera_ref.plan_rays(spt, _models(name)[kind], _tracer(), W, H, FIRST, COUNT, aux=True)
    rec, _ = G.expected(ref.scene(name), rays.reshape(-1), aux.reshape(-1))
    for a in (rays, aux, rec):
        a.setflags(write=False)
    return rays, aux, rec.reshape(COUNT, H, W)


def _not_trivial(name, rec, what, instances=5):
    """What keeps a comparison of images from passing vacuously, on the expected records: a hit share in [0.05, 0.95], `instances`
    distinct values of the instance word (the -1 of the misses is one of them: cfg2_cube has one instance and shows 2, the panorama
    of t_bezier hits four instances and shows 5) and, on t_textured, 250 distinct albedo triples among the hits."""
    hit = rec["instance"] >= 0
    share, distinct = float(hit.mean()), len(np.unique(rec["instance"]))
    triples = len(np.unique(_words(rec["albedo"][hit]).reshape(-1, 3), axis=0))
    print("%s: hit share %.3f, %d instances, %d albedo triples" % (what, share, distinct, triples))
    assert 0.05 <= share <= 0.95, what
    assert distinct >= instances, what
    if name == "t_textured":
        assert triples >= 250, what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["t_materials", "t_textured"])
def test_images_are_the_specification_over_the_reference_records(name, kind):
    rays, aux, rec = _reference_records(name, kind, _util.device_oracle_flags())
    _not_trivial(name, rec, "%s, %s" % (name, kind))
    want = _spec(rec["albedo"], rec["n"], rec["t"], rec["instance"] >= 0)
    ds = _ds(name)
    got = _images_call(ds, _models(name)[kind], _tracer())
    _same_images(got, want, "%s, %s" % (name, kind), keys=("albedo", "depth", "coverage"))
    assert len(np.unique(want["coverage"])) >= 3 and (want["depth"] > 0).mean() > 0.05
    # the normals: the same sums over the device's own records of the reference rays
    dev = ds.gbuffer(rays.reshape(-1), aux.reshape(-1)).reshape(COUNT, H, W)
    assert np.array_equal(dev["instance"], rec["instance"])
    _same_images(got, _spec_of_records(dev), "%s, %s" % (name, kind), keys=("normal",))
    assert (np.abs(got["normal"]).sum(axis=-1) > 0).mean() > 0.05


# ---- 4. images against the route the call replaces --------------------------------------------------------------------------------------

def _present_route(ds, model, renderer, first, count, w=W, h=H):
    rays, aux = spt.camera_rays(model, renderer, w, h, first, count, aux=True)
    return ds.gbuffer(rays.reshape(-1), aux.reshape(-1)).reshape(count, h, w)


ROUTE_CASES = [("cfg2_cube", k) for k in ("thin_lens", "orthographic", "perspective")] + \
              [(n, k) for n in ("t_materials", "t_textured", "t_bezier") for k in KINDS] + [("t_pndf", "thin_lens")]


@pytest.mark.parametrize("name,kind", ROUTE_CASES, ids=["%s-%s" % c for c in ROUTE_CASES])
def test_images_are_the_sums_over_gbuffer_of_camera_rays(name, kind):
    ds, model, r = _ds(name), _models(name)[kind], _tracer()
    for first, count in ((FIRST, COUNT), (2, 1)):
        rec = _present_route(ds, model, r, first, count)
        if count == COUNT:
            _not_trivial(name, rec, "%s, %s" % (name, kind), instances=2 if name == "cfg2_cube" else 5)
        want = _spec_of_records(rec)
        what = "%s, %s, %d samples" % (name, kind, count)
        _same_images(_images_call(ds, model, r, first=first, count=count), want, what)
        _same_images(_images_call(ds, model, r, first=first, count=count, per_pass=100), want, what + ", rays_per_pass 100")
    # (what is left of the loop: one sample, sample 2) the method and its default first sample
    got = ds.camera_gbuffer(model, r, W, H, samples=1, first=2)
    assert sorted(got) == sorted(IMAGES)
    _same_images(got, want, what + ", the method")
    zero = ds.camera_gbuffer(model, r, W, H, samples=COUNT)
    _same_images(zero, _spec_of_records(_present_route(ds, model, r, 0, COUNT)), "%s, %s, from sample 0" % (name, kind))


@pytest.mark.parametrize("keys", [("albedo",), ("normal",), ("depth",), ("coverage",), ("albedo", "coverage"), ("normal", "depth", "coverage")],
                         ids=lambda k: "+".join(k))
def test_images_that_are_not_asked_for_are_not_written(keys):
    name, kind = "t_textured", "thin_lens"
    ds, model, r = _ds(name), _models(name)[kind], _tracer()
    want = _spec_of_records(_present_route(ds, model, r, FIRST, COUNT))
    _same_images(_images_call(ds, model, r, keys=keys), want, "+".join(keys), keys=keys)
    _same_images(_images_call(ds, model, r, keys=keys, per_pass=100), want, "+".join(keys), keys=keys)


@pytest.mark.parametrize("sampler", ["recurrence", "jittered"])
@pytest.mark.parametrize("shape", SHAPES[1:], ids=["%dx%d" % s for s in SHAPES[1:]])
def test_images_of_other_shapes_and_samplers(shape, sampler):
    w, h = shape
    name, kind = "t_materials", "orthographic"
    ds, model, r = _ds(name), _models(name)[kind], _tracer(sampler)
    want = _spec_of_records(_present_route(ds, model, r, FIRST, COUNT, w, h))
    _same_images(_images_call(ds, model, r, w, h), want, "%d x %d, %s" % (w, h, sampler))
    _same_images(_images_call(ds, model, r, w, h, per_pass=3), want, "%d x %d, %s, rays_per_pass 3" % (w, h, sampler))


def test_the_module_level_call_takes_the_device_route_and_keeps_the_other():
    name, kind = "t_bezier", "panorama"
    sc, model, r = ref.scene(name), _models(name)[kind], _tracer()
    want = _spec_of_records(_present_route(_ds(name), model, r, 0, COUNT))
    _same_images(spt.camera_gbuffer(sc, model, r, W, H, samples=COUNT), want, "camera_gbuffer")
    _same_images(spt.camera_gbuffer(_ds(name), model, r, W, H, samples=COUNT, host_rays=True), want, "camera_gbuffer, host_rays")


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------

def _counters(ds):
    return [ds.render_info(k) for k in (0, 1, 3, 4, 5, 7, 8)]


def test_refusals_write_nothing_and_leave_the_scene_usable():
    name = "cfg2_cube"
    sc, ds, r, lib = ref.scene(name), _ds(name), _tracer(), spt.hip_lib()
    good = _models(name)["thin_lens"]
    cfg = spt.OutputConfig(W, H, None, ref.CAMERAS[name])
    film_before = r.render_shard(sc, cfg).copy()
    images_before = _images_call(ds, good, r)
    rays_before, aux_before = _rays_call(ds, good, r, W, H)
    counters = _counters(ds)
    n = COUNT * H * W
    rays, aux = np.zeros(n, dtype=spt.PATH_RAY_DTYPE), np.zeros(n, dtype=spt.RAY_AUX_DTYPE)
    out = {k: np.zeros((H, W, c) if c == 3 else (H, W), dtype=f32) for k, c in IMAGES.items()}

    def model_with(**kw):
        m = spt.CameraModel.thin_lens(sc.get_camera(None), 0.15, 4.0)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def plan_with(**kw):
        p = r.params(W, H)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(fn, job_cls, job_kw, scene=ds._h, no_job=False, word=None, status=INVALID_ARG, model=good, plan=None):
        for a in list(out.values()) + [rays, aux]:
            _words(a)[:] = _words(np.array([7.0], dtype=f32))[0]
        plan = r.params(W, H) if plan is None else plan
        kw = dict(size=C.sizeof(job_cls), model=C.addressof(model) if model is not None else None,
                  plan=C.addressof(plan) if plan is not False else None, first=FIRST, count=COUNT)
        if job_cls is spt.CameraRaysJob:
            kw.update(rays=rays.ctypes.data, aux=aux.ctypes.data)
        else:
            kw.update({k: a.ctypes.data for k, a in out.items()})
        kw.update(job_kw)
        job = job_cls(**kw)
        assert fn(scene, None if no_job else C.byref(job)) == status, (job_kw, lib.spt_last_error())
        if word is not None:
            assert word in lib.spt_last_error().decode(), lib.spt_last_error()
        for a in list(out.values()) + [rays, aux]:
            assert (a.view(f32) == f32(7.0)).all(), job_kw

    shared = [
        (dict(), dict(scene=None, word="null")),
        (dict(), dict(no_job=True, word="null")),
        (dict(flags=2), dict(word="unknown flags")),
        (dict(flags=0x80000000), dict(word="unknown flags")),
        (dict(), dict(model=None, word="null camera model")),
        (dict(), dict(model=model_with(type=4), word="unknown type")),
        (dict(), dict(model=model_with(size=8), word="size")),
        (dict(), dict(model=model_with(lens_radius=-1.0), word="lens_radius")),
        (dict(), dict(model=model_with(focus_distance=float("nan")), word="focus_distance")),
        (dict(), dict(model=spt.CameraModel.orthographic(sc.get_camera(None), 0.0), word="view_height")),
        (dict(), dict(plan=False, word="null plan")),
        (dict(), dict(plan=plan_with(width=0), word="bad plan")),
        (dict(), dict(plan=plan_with(spp=0), word="bad plan")),
        (dict(), dict(plan=plan_with(sampler=3), word="bad plan")),
        (dict(first=2, count=3), dict(word="past the plan's spp")),
        (dict(first=0xffffffff, count=2), dict(word="past the plan's spp")),
        (dict(), dict(plan=plan_with(sampler=spt.SAMPLER_JITTERED, division_x=0), word="divisions")),
        (dict(flags=1), dict(word="not device memory")),
        (dict(first=0, count=1024), dict(plan=plan_with(width=65536, height=32768, spp=1024), word="2^40", status=UNSUPPORTED)),
        (dict(count=1), dict(plan=plan_with(width=65536, height=32769), word="2^31", status=UNSUPPORTED)),
    ]
    for fn, cls in ((lib.spt_camera_rays, spt.CameraRaysJob), (lib.spt_camera_gbuffer, spt.CameraGBufferJob)):
        refused(fn, cls, dict(size=C.sizeof(cls) - 8), word="size")
        for job_kw, kw in shared:
            refused(fn, cls, job_kw, **kw)
    refused(lib.spt_camera_rays, spt.CameraRaysJob, dict(rays=None), word="null rays")
    refused(lib.spt_camera_gbuffer, spt.CameraGBufferJob, dict(albedo=None, normal=None, depth=None, coverage=None), word="no image")
    refused(lib.spt_camera_gbuffer, spt.CameraGBufferJob, dict(count=0), word="count")
    assert _counters(ds) == counters
    # good calls afterwards give the words they gave before
    _same_images(_images_call(ds, good, r), images_before, "after the refusals")
    again, again_aux = _rays_call(ds, good, r, W, H)
    assert again.tobytes() == rays_before.tobytes() and again_aux.tobytes() == aux_before.tobytes()
    assert _util.same_words(r.render_shard(sc, cfg), film_before)


# ---- 6. scene updates --------------------------------------------------------------------------------------------------------------------

def test_images_follow_moved_instances():
    _util.ensure_cpu_build()
    path = os.path.join(_util.SCENES, "cfg2_cube.json")
    sc, moved = spt.load_scene(path), spt.load_scene(path)
    try:
        with open(path) as f:
            inst = json.load(f)["instances"][0]["name"]
        r, model = _tracer(), spt.CameraModel.thin_lens(sc.get_camera(None), 0.15, 4.0)
        ds = sc.device_scene(0)
        first = ds.camera_gbuffer(model, r, W, H, samples=COUNT, first=FIRST)
        _same_images(first, _spec_of_records(_present_route(ds, model, r, FIRST, COUNT)), "as loaded")
        fwd = SU.fwd_by_name(sc, [inst])[inst]
        fwd[0:9] = (fwd[0:9].reshape(3, 3) * f32(0.5)).reshape(9)[[3, 4, 5, 0, 1, 2, 6, 7, 8]]      # half the size, two columns swapped
        fwd[9] += f32(0.8)
        for s in (sc, moved):
            s.set_transforms({inst: fwd})
        ds.update()
        after = ds.camera_gbuffer(model, r, W, H, samples=COUNT, first=FIRST)
        assert (after["coverage"] > 0).sum() >= 10 and (after["coverage"] == 0).any()
        _same_images(after, moved.device_scene(0).camera_gbuffer(model, r, W, H, samples=COUNT, first=FIRST), "against a fresh scene")
        _same_images(after, _spec_of_records(_present_route(ds, model, r, FIRST, COUNT)), "after the update")
        assert not _util.same_words(after["coverage"], first["coverage"]) and not _util.same_words(after["depth"], first["depth"])
    finally:
        sc.close()
        moved.close()


def test_an_open_film_is_left_alone():
    name = "t_materials"
    sc, model = ref.scene(name), _models(name)["thin_lens"]
    r = _tracer()
    cfg = spt.OutputConfig(W, H, None, ref.CAMERAS[name])
    with r.progressive(sc, cfg, moments=True) as undisturbed:
        undisturbed.render(4)
        s, q = undisturbed.sum().copy(), undisturbed.sum_sq().copy()
    want = _images_call(_ds(name), model, r)
    with r.progressive(sc, cfg, moments=True) as film:
        film.render(2)
        _same_images(_images_call(_ds(name), model, r), want, "beside an open film")
        film.render(2)
        assert _util.same_words(film.sum(), s) and _util.same_words(film.sum_sq(), q)


# ---- 7. the command-line program -----------------------------------------------------------------------------------------------------------

def test_the_cli_writes_the_device_calls_images(tmp_path):
    name, seed, samples = "cfg2_cube", 3, 3
    scene_file, renderer_file = os.path.join(_util.SCENES, name + ".json"), os.path.join(_util.SCENES, "pt.json")
    sc = ref.scene(name)
    model = spt.CameraModel.orthographic(sc.get_camera(None), 3.0)
    ren = spt.load_renderer(renderer_file, seed=seed)
    ren.spp = 4
    want = _ds(name).camera_gbuffer(model, ren, W, H, samples=samples)
    assert 0.05 <= (want["coverage"] > 0).mean() <= 0.95 and (want["depth"] > 0).sum() >= 10
    base = [CLI, "-s", scene_file, "-r", renderer_file, "-w", str(W), "-h", str(H), "--spp", "4", "--seed", str(seed), "--orthographic", "3",
            "--gbuffer-samples", str(samples)]
    device, host = str(tmp_path / "d"), str(tmp_path / "h")
    for stem, extra in ((device, []), (host, ["--gbuffer-host-rays"])):
        res = subprocess.run(base + ["--gbuffer-out", stem] + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
    assert _util.same_words(spt.read_exr(device + "_albedo.exr"), want["albedo"])
    assert _util.same_words(spt.read_exr(device + "_normal.exr"), want["normal"])
    depth = spt.read_exr(device + "_depth.exr")
    assert _util.same_words(depth[..., 0], want["depth"]) and _util.same_words(depth[..., 1], want["coverage"]) and (_words(depth[..., 2]) == 0).all()
    for part in ("_albedo.exr", "_normal.exr", "_depth.exr"):
        assert open(device + part, "rb").read() == open(host + part, "rb").read(), part


# ---- 8. device pointers ------------------------------------------------------------------------------------------------------------------

_CHILD = r"""
import ctypes, os, sys
import torch                                  # before the package: the tensor path must work in a process torch initialised
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import _util
import _anywhere_ref as ref
import _radiance_ref
spt = _util.load_pkg()
W, H, SPP, FIRST, COUNT = 37, 19, 4, 1, 3
SAMPLERS = (spt.SAMPLER_RANDOM, spt.SAMPLER_RECURRENCE, spt.SAMPLER_JITTERED)
name = "t_textured"
sc = ref.scene(name)
ds = sc.device_scene(0)
dev = torch.device("cuda", 0)
models = dict(ref.camera_models(name))
models["perspective"] = spt.CameraModel.perspective(sc.get_camera(ref.CAMERAS[name]))
def tracer(sampler):
    return spt.PathTracer(max_depth=ref.DEPTH, sampler=sampler, spp=SPP, division_x=2, division_y=2, seed=ref.SEED)
def words(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)
# 1. rays into tensors, every model, sampler and shape, with and without aux
for kind, model in models.items():
    for sampler in SAMPLERS:
        for w, h in ((37, 19), (1, 1), (64, 4)):
            r = tracer(sampler)
            want, want_aux = spt.camera_rays(model, r, w, h, FIRST, COUNT, aux=True)
            for per_pass in ((0, 100) if (w, h) == (37, 19) else (0,)):
                got, got_aux = ds.camera_rays(model, r, w, h, FIRST, COUNT, aux=True, on_device=True, rays_per_pass=per_pass)
                assert got.device == dev and got.dtype == torch.float32 and got.shape == (COUNT, h, w, 12) and got_aux.shape == (COUNT, h, w, 16)
                assert words(got).tobytes() == want.tobytes() and words(got_aux).tobytes() == want_aux.tobytes(), (kind, sampler, w, h, per_pass)
            alone = ds.camera_rays(model, r, w, h, FIRST, COUNT, on_device=True)
            assert words(alone).tobytes() == want.tobytes(), (kind, sampler, w, h)
# guard words behind device arrays, and nothing written to aux when it is not asked for
r, model = tracer(spt.SAMPLER_RANDOM), models["thin_lens"]
n = COUNT * H * W
want, want_aux = spt.camera_rays(model, r, W, H, FIRST, COUNT, aux=True)
lib = spt.hip_lib()
p = r.params(W, H)
def rays_job(rays_ptr, aux_ptr, flags=spt.CAMERA_RAYS_DEVICE_POINTERS):
    job = spt.CameraRaysJob(size=ctypes.sizeof(spt.CameraRaysJob), flags=flags, model=ctypes.addressof(model), plan=ctypes.addressof(p), first=FIRST, count=COUNT)
    job.rays, job.aux = rays_ptr, aux_ptr
    return job
big_rays, big_aux = torch.full((n + 2, 12), 7.0, device=dev), torch.full((n + 2, 16), 7.0, device=dev)
assert lib.spt_camera_rays(ds._h, ctypes.byref(rays_job(big_rays[1:].data_ptr(), None))) == 0
torch.cuda.synchronize()
assert words(big_rays[1:n + 1]).tobytes() == want.tobytes() and bool((big_rays[0] == 7.0).all()) and bool((big_rays[n + 1] == 7.0).all())
assert bool((big_aux == 7.0).all()), "aux written without being asked for"
assert lib.spt_camera_rays(ds._h, ctypes.byref(rays_job(big_rays[1:].data_ptr(), big_aux[1:].data_ptr()))) == 0
torch.cuda.synchronize()
assert words(big_aux[1:n + 1]).tobytes() == want_aux.tobytes() and bool((big_aux[0] == 7.0).all()) and bool((big_aux[n + 1] == 7.0).all())
# refusals: misaligned tensors, host memory under the flag; nothing is written
fill_rays, fill_aux = torch.full((n, 12), 7.0, device=dev), torch.full((n, 16), 7.0, device=dev)
host = np.full((n, 16), np.float32(7.0))
def refused(job, word, fn=lib.spt_camera_rays):
    assert fn(ds._h, ctypes.byref(job)) == 1
    assert word in lib.spt_last_error().decode(), lib.spt_last_error()
    torch.cuda.synchronize()
    assert bool((fill_rays == 7.0).all()) and bool((fill_aux == 7.0).all()) and (host == 7.0).all()
refused(rays_job(fill_rays.data_ptr() + 4, None), "16-byte aligned")
refused(rays_job(fill_rays.data_ptr(), fill_aux.data_ptr() + 8), "16-byte aligned")
refused(rays_job(host.ctypes.data, None), "not device memory")
refused(rays_job(fill_rays.data_ptr(), host.ctypes.data), "not device memory")
# 2. the chain on tensors: radiance over device rays gives the film's kept samples, gbuffer the host rays' records
t_rays, t_aux = ds.camera_rays(model, r, W, H, FIRST, COUNT, aux=True, on_device=True)
rgb = ds.radiance(t_rays.reshape(-1, 12), aux=t_aux.reshape(-1, 16), max_depth=ref.DEPTH, seed=ref.SEED, rng_skip=_radiance_ref.rng_skip(spt, r))
with r.progressive(sc, spt.OutputConfig(W, H, None, ref.CAMERAS[name]), keep_samples=True, camera_model=model) as film:
    kept = film.render(SPP).kept()[FIRST:FIRST + COUNT]
assert np.isfinite(kept).any() and len(np.unique(kept.view(np.uint32))) > 100
assert _util.same_words(rgb.cpu().numpy().reshape(COUNT, H, W, 3), kept), "radiance over device rays differs from the film's kept samples"
rec = ds.gbuffer(t_rays.reshape(-1, 12), t_aux.reshape(-1, 16))
host_rec = ds.gbuffer(want.reshape(-1), want_aux.reshape(-1))
assert (host_rec["instance"] >= 0).mean() > 0.1 and np.array_equal(words(rec), host_rec.view(np.uint32).reshape(-1, 16))
t_seg = t_rays.reshape(-1, 12)[:, :8].contiguous()      # (o, t_min, d, .): spt_occluded's record once t_max stands in its last word
t_seg[:, 7] = float(np.finfo(np.float32).max)
occ = ds.occluded(t_seg)
seg = _util.first_segments(want.reshape(-1))
assert 0.05 < (ds.occluded(seg) != 0).mean() < 0.95
assert np.array_equal(occ.cpu().numpy().reshape(-1) != 0, ds.occluded(seg).reshape(-1) != 0)
# 3. images into tensors
host_images = ds.camera_gbuffer(model, r, W, H, samples=COUNT, first=FIRST)
assert 0.05 < (host_images["coverage"] > 0).mean() < 0.95
for per_pass in (0, 100):
    got = ds.camera_gbuffer(model, r, W, H, samples=COUNT, first=FIRST, on_device=True, rays_per_pass=per_pass)
    for k, v in host_images.items():
        assert got[k].device == dev and tuple(got[k].shape) == v.shape and np.array_equal(words(got[k]), v.view(np.uint32)), (k, per_pass)
images = {k: torch.full(v.shape, 7.0, device=dev) for k, v in host_images.items()}
def images_job(**ptrs):
    job = spt.CameraGBufferJob(size=ctypes.sizeof(spt.CameraGBufferJob), flags=spt.CAMERA_GBUFFER_DEVICE_POINTERS, model=ctypes.addressof(model),
                               plan=ctypes.addressof(p), first=FIRST, count=COUNT)
    for k, v in ptrs.items():
        setattr(job, k, v)
    return job
def images_refused(job, word):
    assert lib.spt_camera_gbuffer(ds._h, ctypes.byref(job)) == 1
    assert word in lib.spt_last_error().decode(), lib.spt_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in images.values()) and (host == 7.0).all()
images_refused(images_job(albedo=images["albedo"].data_ptr(), depth=host.ctypes.data), "not device memory")
images_refused(images_job(normal=images["normal"].data_ptr() + 2), "4-byte aligned")
assert lib.spt_camera_gbuffer(ds._h, ctypes.byref(images_job(depth=images["depth"].data_ptr(), coverage=images["coverage"].data_ptr()))) == 0
torch.cuda.synchronize()
assert np.array_equal(words(images["depth"]), host_images["depth"].view(np.uint32)) and np.array_equal(words(images["coverage"]), host_images["coverage"].view(np.uint32))
assert bool((images["albedo"] == 7.0).all()) and bool((images["normal"] == 7.0).all())
print("camera device tensors ok")
"""


def test_device_pointers_in_a_process_that_imported_torch_first():
    res = subprocess.run([sys.executable, "-c", _CHILD, _util.ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "camera device tensors ok" in res.stdout, res.stdout + res.stderr

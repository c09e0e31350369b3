"""spt_radiance (DeviceScene.radiance): the integrator on caller-provided rays, against the oracle.

The reference is tests/_radiance_ref.py: the rays of a camera plan from oracle_camera_ray, their streams (pixel, sample), and the
oracle's colour of every single sample (oracle_render_samples under the device's oracle flags).  Every comparison is
_util.same_words: every word equal, NaNs in the same places, no ray left out.

Plan: 48 x 36 pixels (3 x 3 tiles of 16 x 16, neither side a multiple), samples 0 .. 3 of a 4-spp plan, max_depth 5: 6912 rays, 27
intake workgroups over 27 queue shards."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _radiance_ref
import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32

W, H, SPP, DEPTH, SEED = 48, 36, 4, 5, 11
PATTERN = np.uint32(0x7fc0beef)   # (a NaN no path produces)
SAMPLERS = {"recurrence": spt.SAMPLER_RECURRENCE, "random": spt.SAMPLER_RANDOM}


@functools.lru_cache(maxsize=None)
def _scene(name):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_util.SCENES, name))


def _tracer(sampler="recurrence", seed=SEED, spp=SPP):
    return spt.PathTracer(max_depth=DEPTH, sampler=SAMPLERS[sampler], spp=spp, seed=seed)


@functools.lru_cache(maxsize=None)
def _plan(name, camera=None, sampler="recurrence", aux=False, cam_override=None, spp=SPP):
    """(rays, aux or None, expected (n, 3), rng_skip) of the plan's first 4 samples, flattened in (sample, row, column) order; read-only."""
    sc = _scene(name)
    r = _tracer(sampler, spp=spp)
    cam = camera if cam_override is None else _CAMERAS[cam_override]
    made = _radiance_ref.plan_rays(spt, sc, r, W, H, 0, SPP, camera=cam, aux=aux)
    rays, ax = (made if aux else (made, None))
    want = _radiance_ref.expected(sc, r, W, H, 0, SPP, camera=cam).reshape(-1, 3)
    rays = rays.reshape(-1)
    rays.setflags(write=False)
    want.setflags(write=False)
    if ax is not None:
        ax = ax.reshape(-1)
        ax.setflags(write=False)
    return rays, ax, want, _radiance_ref.rng_skip(spt, r)


def _radiance(name, rays, aux=None, skip=0, **kw):
    return _scene(name).device_scene(0).radiance(rays, aux=aux, max_depth=DEPTH, seed=SEED, rng_skip=skip, **kw)


def _check(got, want, what):
    assert got.shape == want.shape
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    assert _util.same_words(got, want), "%s: %d of %d words differ from the oracle's samples" % (what, int(bad.sum()), bad.size)


# ---- 1. camera equivalence --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,camera,aux", [
    ("cfg2_cube.json", None, False),        # fused pipeline, LDS-resident
    ("t_materials.json", "main", False),    # general pipeline, class queues, environment (misses and later bounces)
    ("t_medium.json", None, False),         # media: in-medium vertices, the re-traced ray after leaving one
    ("t_plastic.json", None, False),
    ("t_subsurface.json", None, True),      # BSSRDF probe inside the shade kernel; its albedo is an image texture, so the oracle's
                                            #   sample needs the first hit's differentials like every textured scene: aux
    ("t_textured.json", None, True),        # differentials of the first hit from the auxiliary rays (k_shade<2, ..., kAux>)
    ("t_pndf.json", "main", True),          # glint footprints from the same differentials
    ("t_bezier.json", "main", True),        # forwarded to the library with the patch primitive (a textured patch: aux)
])
def test_camera_rays_give_the_oracles_samples(name, camera, aux):
    rays, ax, want, skip = _plan(name, camera, "recurrence", aux)
    assert np.isfinite(want).any() and want[np.isfinite(want)].max() > 0.05
    _check(_radiance(name, rays, ax, skip), want, name)


def test_random_sampler_streams_skip_the_pixel_offsets():
    rays, _, want, skip = _plan("t_materials.json", "main", "random")
    assert skip == 2
    _check(_radiance("t_materials.json", rays, None, skip), want, "random sampler")


# ---- 2. per-ray origins and order -------------------------------------------------------------------------------------------------

_CAMERAS = {
    "a": spt.make_camera((0.0, 0.0, 5.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0),
    "b": spt.make_camera((3.0, 2.0, 4.0), (-0.6, -0.4, -0.8), (0.0, 1.0, 0.0), 50.0),
    "c": spt.make_camera((-2.5, 1.0, -4.0), (0.5, -0.2, 0.8), (0.0, 1.0, 0.0), 35.0),
}


def test_three_cameras_permuted_in_one_call():
    name = "t_materials.json"
    plans = [_plan(name, None, "recurrence", False, key) for key in ("a", "b", "c")]
    rays = np.concatenate([p[0] for p in plans])
    want = np.concatenate([p[2] for p in plans])
    assert len({tuple(p[0]["o"][0]) for p in plans}) == 3
    perm = np.random.default_rng(5).permutation(rays.shape[0])
    _check(_radiance(name, rays[perm]), want[perm], "three cameras, permuted")


# ---- 3. repeats -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,camera", [("cfg2_cube.json", None), ("t_materials.json", "main")])
def test_repeats_are_the_in_order_mean(name, camera):
    rays = _plan(name, camera)[0][: W * H].copy()      # sample 0 of every pixel: streams (pixel, 0), (pixel, 1), (pixel, 2)
    singles = []
    for k in range(3):
        one = rays.copy()
        one["stream_b"] += np.uint32(k)
        singles.append(_radiance(name, one))
    want = ((f32(0) + singles[0]) + singles[1] + singles[2]) * (f32(1) / f32(3))
    # (the cube stands in the void under delta lights: its paths gather direct light at the first hit only, whatever they draw; on
    #  t_materials the stream matters, and there the three calls must not agree)
    if name == "t_materials.json":
        assert not _util.same_words(singles[0], singles[1])
    _check(_radiance(name, rays, repeats=3), want.astype(f32), "repeats = 3")


# ---- 4. passes and ragged sizes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,camera", [("cfg2_cube.json", None), ("t_materials.json", "main")])
def test_passes_and_ragged_sizes(name, camera):
    rays, _, want, skip = _plan(name, camera)
    whole = _radiance(name, rays, None, skip)
    _check(whole, want, name)
    assert _util.same_words(_radiance(name, rays, None, skip, rays_per_pass=1000), whole)
    for n in (1, 63, 65, 257):
        first = 3000   # (rays of the middle of the image, where the scene is)
        assert _util.same_words(_radiance(name, rays[first:first + n], None, skip), whole[first:first + n]), n


# ---- 5. hits ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,camera,aux", [("cfg2_cube.json", None, False), ("t_materials.json", "main", False), ("t_bezier.json", "main", True)])
def test_hits_are_trace_closest(name, camera, aux):
    rays, ax, want, skip = _plan(name, camera, "recurrence", aux)
    rgb, hits = _radiance(name, rays, ax, skip, hits=True)
    _check(rgb, want, name)
    seg = np.zeros(rays.shape[0], dtype=spt.RAY_DTYPE)
    seg["o"], seg["t_min"], seg["d"], seg["t_max"] = rays["o"], rays["t_min"], rays["d"], np.finfo(f32).max
    ref = _scene(name).device_scene(0).trace_closest(seg)
    assert (ref["instance"] >= 0).any() and (ref["instance"] < 0).any()
    assert hits.tobytes() == ref.tobytes()


# ---- 6. aux is inert where it must be ---------------------------------------------------------------------------------------------

def test_aux_is_ignored_without_textures():
    rays, _, want, skip = _plan("cfg2_cube.json")
    aux = np.zeros(rays.shape[0], dtype=spt.RAY_AUX_DTYPE)
    aux["rx_d"], aux["ry_d"] = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    _check(_radiance("cfg2_cube.json", rays, aux, skip), want, "cube with aux")


def test_textured_scene_without_aux():
    """No oracle value for the hits (the oracle's camera rays always carry auxiliary rays): the call succeeds, does not depend on
    how it is cut into passes, and a ray that hits nothing - which reads no differentials - has the oracle's sample."""
    rays, ax, want, skip = _plan("t_textured.json", None, "recurrence", True)
    got, hits = _radiance("t_textured.json", rays, None, skip, hits=True)
    miss = hits["instance"] < 0
    assert miss.any() and (~miss).any()
    assert _util.same_words(got[miss], want[miss])
    assert _util.same_words(_radiance("t_textured.json", rays, None, skip, rays_per_pass=700), got)


@pytest.mark.parametrize("name", ["t_textured.json", "t_subsurface.json"])
def test_no_aux_is_the_oracle_without_a_footprint(name):
    """An oracle value for the hits of a call without aux.  The auxiliary rays of a plan are its camera rays moved by 1 / sqrt(spp)
    of a pixel (pt.rs:272-275); under a plan of 2^30 samples per pixel that is 2^-15 of a pixel, far below a texel of any image of
    these scenes (a 48-pixel-wide view of textures of at most 512 texels), where ImageTex's level is clamp(log2(width + 0.001), 0, ..)
    = 0 exactly and its blend weight 0: the level and the weight it has for no differentials at all (image_tex.rs:127-151).  So the
    oracle's samples of that plan are what "textured without differentials" must give, and what the same rays give with aux."""
    rays, ax, want, skip = _plan(name, None, "recurrence", True, None, 1 << 30)
    _check(_radiance(name, rays, ax, skip), want, name + " with the plan's (tiny) auxiliary offsets")
    _check(_radiance(name, rays, None, skip), want, name + " without aux")
    # ... which is not what the differentials of the 4-spp plan give: half a pixel of offset reaches the coarser levels
    if name == "t_subsurface.json":
        rays4, ax4, want4, _ = _plan(name, None, "recurrence", True)
        assert not _util.same_words(_radiance(name, rays4, None, skip), want4)


# the walkers of scenes that do not fit LDS: the streaming intake kernel, and the walker over the geometry in memory
@pytest.mark.parametrize("switches", [{"SPT_NO_LDS_GEO": "1"}, {"SPT_NO_LDS_GEO": "1", "SPT_NO_STREAM": "1"}], ids=["stream", "memory"])
@pytest.mark.parametrize("name,camera,aux", [("t_materials.json", "main", False), ("t_textured.json", None, True)])
def test_large_scene_walkers(monkeypatch, switches, name, camera, aux):
    rays, ax, want, skip = _plan(name, camera, "recurrence", aux)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)      # (read when the device scene is made)
    sc = spt.load_scene(os.path.join(_util.SCENES, name))
    try:
        rgb, hits = sc.device_scene(0).radiance(rays, aux=ax, max_depth=DEPTH, seed=SEED, rng_skip=skip, hits=True)
    finally:
        sc.close()
    _check(rgb, want, name)
    assert hits.tobytes() == _radiance(name, rays, ax, skip, hits=True)[1].tobytes()


# ---- 7. isolation -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,camera", [("cfg2_cube.json", None), ("t_materials.json", "main")])
def test_films_and_async_frames_are_undisturbed(name, camera):
    sc = _scene(name)
    rays, _, want, skip = _plan(name, camera)
    cfg = spt.OutputConfig(W, H, None, camera)
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=8, seed=3)
    with r.progressive(sc, cfg) as plain:
        undisturbed = plain.render(4).render(4).mean().copy()
    with r.progressive(sc, cfg) as film:
        film.render(4)
        _check(_radiance(name, rays, None, skip), want, "between two increments")
        assert _util.same_words(film.render(4).mean(), undisturbed)
    sync = r.render_shard(sc, cfg).copy()
    buf = r.render_shard(sc, cfg, reuse_output=True, wait=False)
    _check(_radiance(name, rays, None, skip), want, "behind an asynchronous frame")
    r.wait(sc)
    assert _util.same_words(np.array(buf), sync)


# ---- 8. device pointers -----------------------------------------------------------------------------------------------------------

_CHILD = r"""
import os, sys
import torch                                  # before the package: the tensor path must work in a process torch initialised
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import _util
spt = _util.load_pkg()
W, H = 48, 36
sc = spt.load_scene(os.path.join(_util.SCENES, "t_textured.json"))
cam = sc.get_camera(None)
off = np.random.default_rng(9).random((2, H, W, 2), dtype=np.float32)
rays, aux = spt.perspective_rays(cam, W, H, off, aux_spp=4)
rays, aux = rays.reshape(-1), aux.reshape(-1)
ds = sc.device_scene(0)
rgb, hits = ds.radiance(rays, aux=aux, max_depth=5, seed=11, hits=True, repeats=2)
dev = torch.device("cuda", 0)
t_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 12).copy()).to(dev)
t_aux = torch.from_numpy(aux.view(np.float32).reshape(-1, 16).copy()).to(dev)
t_rgb, t_hits = ds.radiance(t_rays, aux=t_aux, max_depth=5, seed=11, hits=True, repeats=2)
assert t_rgb.device == dev and t_rgb.shape == (rays.shape[0], 3) and t_hits.shape == (rays.shape[0], 5)
assert _util.same_words(t_rgb.cpu().numpy(), rgb), "tensor radiance differs from the host path"
assert t_hits.cpu().numpy().tobytes() == hits.tobytes(), "tensor hits differ from the host path"
assert np.isfinite(rgb).any() and rgb[np.isfinite(rgb)].max() > 0.05 and (hits["instance"] >= 0).any()
# a host pointer under the device-pointer flag is refused and writes nothing
job = spt.RadianceJob(size=C_SIZE, flags=spt.RADIANCE_DEVICE_POINTERS, n_rays=rays.shape[0], repeats=1, max_depth=5, seed=11)
out = np.full((rays.shape[0], 3), np.float32(7.0))
job.rays, job.rgb_out = rays.ctypes.data, out.ctypes.data
import ctypes
assert spt.hip_lib().spt_radiance(ds._h, ctypes.byref(job)) == 1 and (out == 7.0).all()
job.rays, job.rgb_out = t_rays.data_ptr(), out.ctypes.data
assert spt.hip_lib().spt_radiance(ds._h, ctypes.byref(job)) == 1 and (out == 7.0).all()
again, _ = ds.radiance(t_rays, aux=t_aux, max_depth=5, seed=11, hits=True, repeats=2)
assert _util.same_words(again.cpu().numpy(), rgb)
sc.close()
print("radiance tensors ok")
""".replace("C_SIZE", str(C.sizeof(spt.RadianceJob)))


def test_device_pointers_in_a_process_that_imported_torch_first():
    res = subprocess.run([sys.executable, "-c", _CHILD, _util.ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "radiance tensors ok" in res.stdout, res.stdout + res.stderr


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_leave_the_scene_usable():
    name = "cfg2_cube.json"
    rays, _, want, skip = _plan(name)
    ds = _scene(name).device_scene(0)
    lib = spt.hip_lib()
    n = rays.shape[0]
    out = np.empty((n, 3), dtype=f32)
    hits = np.empty(n, dtype=spt.HIT_DTYPE)

    def job(rays_arr=rays, **kw):
        j = spt.RadianceJob(size=C.sizeof(spt.RadianceJob), n_rays=rays_arr.shape[0], repeats=1, max_depth=DEPTH, seed=SEED)
        j.rays, j.rgb_out, j.hits_out = rays_arr.ctypes.data, out.ctypes.data, hits.ctypes.data
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(j, scene=ds._h, word=None, status=1):
        out.view(np.uint32)[:] = PATTERN
        hits.view(np.uint8)[:] = 0xa5
        assert lib.spt_radiance(scene, C.byref(j) if j is not None else None) == status
        assert (out.view(np.uint32) == PATTERN).all() and (hits.view(np.uint8) == 0xa5).all()
        if word is not None:
            assert word in lib.spt_last_error().decode(), lib.spt_last_error()

    refused(job(), scene=None)
    refused(None)
    refused(job(rays=None))
    refused(job(rgb_out=None))
    refused(job(size=C.sizeof(spt.RadianceJob) - 8), word="size")
    refused(job(flags=2), word="flags")
    refused(job(flags=0x80000000), word="flags")
    refused(job(repeats=0), word="repeats")
    refused(job(max_depth=256), status=4)
    for field, value, index in (("o", np.nan, 0), ("d", np.inf, 4097), ("t_min", -np.inf, n - 1), ("d", 0.0, 2500)):
        bad = rays.copy()
        if field == "t_min":
            bad[field][index] = value
        elif value == 0.0:
            bad[field][index] = 0.0
        else:
            bad[field][index, 1] = value
        if index + 3 < n:
            bad["o"][index + 3, 0] = np.nan   # a later bad ray: the first one is named
        refused(job(bad), word="ray %d " % index)
        refused(job(bad, rays_per_pass=1024), word="ray %d " % index)   # found in a later pass: still nothing written
    refused(job(flags=spt.RADIANCE_DEVICE_POINTERS), word="device")
    # nothing to do is not a refusal, and writes nothing either
    refused(job(n_rays=0), status=0)
    refused(job(n_rays=0, rays=None, rgb_out=None), status=0)
    # a good call after all of them
    rgb, h2 = ds.radiance(rays, max_depth=DEPTH, seed=SEED, rng_skip=skip, hits=True)
    _check(rgb, want, "after the refusals")
    assert (h2["instance"] >= 0).any()


def test_max_depth_zero_is_black_and_still_reports_hits():
    rays = _plan("t_materials.json", "main")[0]
    ds = _scene("t_materials.json").device_scene(0)
    rgb, hits = ds.radiance(rays, max_depth=0, seed=SEED, hits=True)
    assert (rgb.view(np.uint32) == 0).all()
    _, ref = ds.radiance(rays, max_depth=DEPTH, seed=SEED, hits=True)
    assert hits.tobytes() == ref.tobytes()


# ---- 10. the three item entries share their staging and workspace buffers -----------------------------------------------------------

@pytest.mark.parametrize("name,camera", [("cfg2_cube", None), ("t_materials", "main")])
def test_radiance_bake_and_probes_interleaved_with_sizes_that_shrink_and_grow(name, camera):
    """spt_probe, spt_radiance and spt_bake in turn on one device scene, host lists cut into passes of 256 items: the calls share the
    pinned staging slots and their events, the device copies of a pass' records, the result buffer and the hit buffer, which each
    entry sizes and lays out for itself.  Every call must give, word for word, what it gives as the first call on a fresh device scene.
    The reference is the same code on a fresh scene, not the oracle: this finds state that leaks from one entry into the next, not an
    error every call shares (the oracle-anchored tests above and in test_gpu_bake.py / test_gpu_probe.py are there for that).  The calls
    of 700, 900 and 1000 items have three or four passes and wait for a staging slot's event; those of 300, 40 and 17 have one or two."""
    import test_gpu_bake
    import test_gpu_probe
    sc = _scene(name + ".json")
    rays, _, _, skip = _plan(name + ".json", camera)
    points = test_gpu_bake._points(name)
    probes = np.concatenate([test_gpu_probe._grid(sc, seed) for seed in (5, 6, 7)])
    assert rays.shape[0] >= 4000 and points.shape[0] >= 917 and probes.shape[0] >= 740
    kw = dict(max_depth=DEPTH, seed=SEED)
    calls = [
        lambda ds: ds.probes(probes[:700], samples=8, aux=True, points_per_pass=256, **kw),
        lambda ds: ds.radiance(rays[3000:3300], rng_skip=skip, hits=True, repeats=3, rays_per_pass=256, **kw),
        lambda ds: ds.bake(points[:900], samples=4, points_per_pass=256, **kw),
        lambda ds: ds.probes(probes[700:740], samples=8, points_per_pass=256, **kw),
        lambda ds: ds.radiance(rays[3000:4000], rng_skip=skip, hits=True, rays_per_pass=256, **kw),
        lambda ds: ds.bake(points[900:917], samples=4, points_per_pass=256, **kw),
    ]
    sc.close_device_scene(0)
    ds = sc.device_scene(0)
    got = [call(ds) for call in calls]
    for i, call in enumerate(calls):
        sc.close_device_scene(0)
        want = call(sc.device_scene(0))
        for g, w in zip(got[i] if isinstance(got[i], tuple) else (got[i],), want if isinstance(want, tuple) else (want,)):
            if g.dtype == spt.HIT_DTYPE:
                assert g.tobytes() == w.tobytes(), "call %d: hits" % i
            else:
                assert np.isfinite(w).any() and _util.same_words(g, w), "call %d" % i

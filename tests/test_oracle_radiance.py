"""oracle_radiance: spt_radiance's contract (include/spt_abi.h) on the oracle's trace_ray, for rays of any origin.

It is the reference of tests/test_gpu_radiance_anywhere.py and of the oracle anchors of bake, probe and the camera models, so it is
pinned here on the CPU: on the rays a pinhole camera makes it must return oracle_render_samples' words (the entry the device has been
held to so far), and the rest of the contract - repeats, order independence, max_depth 0 - is checked on the same rays.  For rays no
camera makes there is no second oracle entry to compare with; a furnace whose answer is known in closed form stands in."""
import functools
import json
import os

import numpy as np
import pytest

import _radiance_ref
import _util

spt = _util.load_pkg()
f32 = np.float32

W, H, SPP, DEPTH, SEED = 48, 36, 4, 5, 11
COUNT = 2      # samples 0 and 1 of the 4-spp plan: 3456 rays
SAMPLERS = {"recurrence": spt.SAMPLER_RECURRENCE, "random": spt.SAMPLER_RANDOM}
# the scenes of test_gpu_radiance.py::test_camera_rays_give_the_oracles_samples; textured: the first hit reads its differentials
SCENES = [("cfg2_cube.json", None, False), ("t_materials.json", "main", False), ("t_medium.json", None, False), ("t_plastic.json", None, False),
          ("t_subsurface.json", None, True), ("t_textured.json", None, True), ("t_pndf.json", "main", True), ("t_bezier.json", "main", True)]


@functools.lru_cache(maxsize=None)
def _scene(name):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_util.SCENES, name))


@functools.lru_cache(maxsize=None)
def _plan(name, camera, sampler, spp=SPP):
    """(rays, aux, the oracle's samples (n, 3), rng_skip) of the plan's first COUNT samples; read-only."""
    sc = _scene(name)
    r = spt.PathTracer(max_depth=DEPTH, sampler=SAMPLERS[sampler], spp=spp, seed=SEED)
    rays, aux = _radiance_ref.plan_rays(spt, sc, r, W, H, 0, COUNT, camera=camera, aux=True)
    want = _util.oracle_render_samples(sc, r, W, H, 0, COUNT, camera=camera, flags=_util.device_oracle_flags()).reshape(-1, 3)
    rays, aux = rays.reshape(-1), aux.reshape(-1)
    for a in (rays, aux, want):
        a.setflags(write=False)
    return rays, aux, want, _radiance_ref.rng_skip(spt, r)


def _radiance(name, rays, aux=None, skip=0, **kw):
    kw.setdefault("max_depth", DEPTH)
    return _util.oracle_radiance(_scene(name), rays, aux, seed=SEED, rng_skip=skip, flags=_util.device_oracle_flags(), **kw)


@pytest.mark.parametrize("sampler", ["recurrence", "random"])
@pytest.mark.parametrize("name,camera,textured", SCENES)
def test_camera_rays_give_render_samples_words(name, camera, textured, sampler):
    rays, aux, want, skip = _plan(name, camera, sampler)
    assert skip == (2 if sampler == "random" else 0)
    assert np.isfinite(want).any() and want[np.isfinite(want)].max() > 0.05
    assert _util.same_words(_radiance(name, rays, aux, skip), want)
    plain = _radiance(name, rays, None, skip)
    if not textured:
        assert _util.same_words(plain, want)     # nothing reads the differentials
    else:
        # without aux a ray that hits nothing still has the sample's words; the hits are pinned by the next test
        miss = _util.oracle_trace_closest(_scene(name), _util.first_segments(rays), _util.device_oracle_flags())["instance"] < 0
        assert miss.any() and (~miss).any()
        assert _util.same_words(plain[miss], want[miss])
    if sampler == "random" and name == "t_materials.json":
        assert not _util.same_words(_radiance(name, rays, aux, 0), want)     # the skipped draws matter


@pytest.mark.parametrize("name", ["t_textured.json", "t_subsurface.json"])
def test_no_aux_is_render_samples_without_a_footprint(name):
    """Under a plan of 2^30 samples per pixel the auxiliary rays are 2^-15 of a pixel away, where ImageTex's level and blend weight
    are those of no differentials at all (test_gpu_radiance.py::test_no_aux_is_the_oracle_without_a_footprint has the argument): the
    samples of that plan are what the same rays must give without aux."""
    rays, aux, want, skip = _plan(name, None, "recurrence", 1 << 30)
    assert _util.same_words(_radiance(name, rays, aux, skip), want)
    assert _util.same_words(_radiance(name, rays, None, skip), want)
    rays4, aux4, want4, _ = _plan(name, None, "recurrence")
    if name == "t_subsurface.json":
        assert not _util.same_words(_radiance(name, rays4, None, skip), want4)   # ... and the 4-spp plan's footprint is another one


def test_other_oracle_flags_go_through():
    """The flags reach trace_ray: the reference's own configuration (tree walk, division in the slab test) gives its own samples."""
    name, camera = "t_materials.json", "main"
    sc = _scene(name)
    rays, aux, _, _ = _plan(name, camera, "recurrence")
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=SPP, seed=SEED)
    want = _util.oracle_render_samples(sc, r, W, H, 0, COUNT, camera=camera, flags=0).reshape(-1, 3)
    assert _util.same_words(_util.oracle_radiance(sc, rays, aux, max_depth=DEPTH, seed=SEED, flags=0), want)


def test_repeats_are_the_in_order_mean():
    name = "t_materials.json"
    rays = _plan(name, "main", "recurrence")[0][: W * H]
    singles = []
    for k in range(3):
        one = rays.copy()
        one["stream_b"] += np.uint32(k)
        singles.append(_radiance(name, one))
    assert not _util.same_words(singles[0], singles[1])
    want = ((f32(0) + singles[0]) + singles[1] + singles[2]) * (f32(1) / f32(3))
    assert want.dtype == f32
    assert _util.same_words(_radiance(name, rays, repeats=3), want)


def test_a_permuted_batch_gives_permuted_results():
    name = "t_textured.json"
    rays, aux, want, skip = _plan(name, None, "recurrence")
    perm = np.random.default_rng(5).permutation(rays.shape[0])
    assert _util.same_words(_radiance(name, rays[perm], aux[perm], skip), want[perm])
    # ... and a ray alone is the ray in the batch
    for i in (0, 1234, rays.shape[0] - 1):
        assert _util.same_words(_radiance(name, rays[i:i + 1], aux[i:i + 1], skip), want[i:i + 1])


def test_max_depth_zero_is_black():
    rays = _plan("t_materials.json", "main", "recurrence")[0]
    got = _radiance("t_materials.json", rays, max_depth=0)
    assert got.shape == (rays.shape[0], 3) and (got.view(np.uint32) == 0).all()
    assert _util.oracle_radiance(_scene("t_materials.json"), rays[:0], max_depth=DEPTH).shape == (0, 3)


def test_white_furnace_from_interior_points(tmp_path):
    """Rays no camera makes, with a known answer: the closed Lambert box of test_oracle_bxdf.py::test_white_furnace_closed_lambert_box
    (albedo rho, walls emitting Le, nothing else).  Every path vertex sees Le, so a path from ANY interior point in ANY direction
    has the expectation Le * sum_{k<8} rho^k.  2^18 rays from uniform interior points in uniform directions - the path count of that
    test's 32 x 32 x 256 film, the same estimator - within the same 2 %."""
    rho, le, n = 0.5, 1.0, 1 << 18
    (tmp_path / "cube.obj").write_text(open(os.path.join(_util.SCENES, "models", "cube.obj")).read())
    half = np.array([2.0, 1.5, 2.5])
    sc = {"cameras": {"type": "perspective", "name": "c", "eye": [0.1, -0.2, 0.3], "forward": [0.3, 0.1, -1.0], "up": [0.0, 1.0, 0.0], "fov": 70.0},
          "textures": [{"type": "scalar", "name": "a", "value": [rho, rho, rho]}],
          "materials": [{"type": "lambert", "name": "m", "albedo": "a"}], "mediums": [],
          "surfaces": [{"name": "s", "material": "m", "emissive": [le, le, le], "double_sided": True}],
          "primitives": [{"type": "trimesh", "name": "p", "obj_file": "cube.obj"}],
          "instances": [{"name": "i", "primitive": "p", "surface": "s", "scale": half.tolist()}], "lights": []}
    p = tmp_path / "furnace.json"
    p.write_text(json.dumps(sc))
    scene = spt.load_scene(str(p))
    inst = scene.array("instances")
    assert np.allclose(inst["bmin"][0], -half) and np.allclose(inst["bmax"][0], half)    # the box the points are drawn in
    rng = np.random.default_rng(3)
    rays = np.zeros(n, dtype=spt.PATH_RAY_DTYPE)
    rays["o"] = (rng.uniform(-0.95, 0.95, size=(n, 3)) * half).astype(f32)
    d = rng.normal(size=(n, 3))
    rays["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    rays["t_min"] = f32(0.0001)
    rays["stream_a"], rays["stream_b"] = np.arange(n, dtype=np.uint32), 7
    got = _util.oracle_radiance(scene, rays, max_depth=8, seed=2)
    assert np.isfinite(got).all() and len(np.unique(got[:, 0])) > 100
    expect = le * (1 - rho ** 8) / (1 - rho)      # emission seen at depths 0..7
    print("furnace from interior points: mean %.5f, expected %.5f" % (got.mean(), expect))
    assert abs(got.mean() - expect) / expect < 0.02
    scene.close()

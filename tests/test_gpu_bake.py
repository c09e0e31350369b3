"""spt_bake (DeviceScene.bake): irradiance at surface points, the gather rays made on the device.

The reference of every comparison is computed from calls that exist without spt_bake, over tests/_bake_ref.py's restatement of the
specification:  want_i = D_ref + in-order mean over k of ds.radiance(rays_ref[i, k], repeats=1, rng_skip=0), with D_ref summed from
_bake_ref's li, gated by ds.trace_any on _bake_ref's shadow rays.  Every comparison is _util.same_words; no point is left out.
That reference is the device's own integrator: it shows that spt_bake is those calls, not that those calls are right for rays that
start on a surface.  The tie to the oracle is test_a_bake_is_the_oracles_delta_sum_plus_the_mean_of_the_oracles_radiance (the same
formula over oracle_radiance and oracle_trace_any) and, for spt_radiance itself, tests/test_gpu_radiance_anywhere.py.

Points: the mesh hits of a 48 x 36 camera grid (trace_closest) plus random points and the three corners of a triangle on every mesh
instance; 4 samples, max_depth 5."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _bake_ref
import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32

W, H, S, DEPTH, SEED = 48, 36, 4, 5, 11
PATTERN = np.uint32(0x7fc0beef)   # (a NaN no bake produces)
CAMERAS = {"cfg2_cube": None, "t_materials": "main", "t_medium": None, "t_textured": None, "t_bezier": "main"}


@functools.lru_cache(maxsize=None)
def _scene(name):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_util.SCENES, name + ".json"))


def _ds(name):
    return _scene(name).device_scene(0)


def _grid_hits(scene, ds, camera):
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=1, seed=SEED)
    pr = spt.camera_rays(spt.CameraModel.perspective(scene.get_camera(camera)), r, W, H).reshape(-1)
    rays = np.zeros(pr.shape[0], dtype=spt.RAY_DTYPE)
    rays["o"], rays["t_min"], rays["d"], rays["t_max"] = pr["o"], pr["t_min"], pr["d"], np.finfo(f32).max
    return rays, ds.trace_closest(rays)


def _random_points(scene, per_instance, seed):
    rng = np.random.default_rng(seed)
    inst, meshes = scene.array("instances"), scene.array("meshes")
    out = []
    for i, rec in enumerate(inst):
        if rec["prim_type"] != 1:
            continue
        m = meshes[rec["prim_id"]]
        pts = np.zeros(per_instance + 3, dtype=spt.BAKE_POINT_DTYPE)
        pts["instance"] = i
        pts["prim"] = m["tri_first"] + rng.integers(0, m["tri_count"], size=per_instance + 3)
        a, b = rng.random(per_instance), rng.random(per_instance)
        fold = a + b > 1
        pts["v"][:per_instance], pts["w"][:per_instance] = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
        pts["v"][per_instance:], pts["w"][per_instance:] = [0, 1, 0], [0, 0, 1]
        out.append(pts)
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def _points(name):
    """SURFACE points of the scene: the camera grid's mesh hits fed straight back in, then random points; read-only."""
    scene, ds = _scene(name), _ds(name)
    _, hits = _grid_hits(scene, ds, CAMERAS[name])
    inst = scene.array("instances")
    on_mesh = (hits["instance"] >= 0) & (inst["prim_type"][np.maximum(hits["instance"], 0)] == 1)
    grid = np.zeros(int(on_mesh.sum()), dtype=spt.BAKE_POINT_DTYPE)
    for f in ("instance", "prim", "v", "w"):
        grid[f] = hits[f][on_mesh]
    n_mesh = int((inst["prim_type"] == 1).sum())
    pts = np.concatenate([grid, _random_points(scene, max(24, -(-(1500 - len(grid)) // n_mesh)), 7)])   # about 1500 in all
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _reference(name, world=False):
    """(points, ref inputs, want, D, gather sum) from calls that exist without spt_bake; read-only."""
    scene, ds = _scene(name), _ds(name)
    pts = _world_points(name) if world else _points(name)
    ref = _bake_ref.bake_inputs(spt, _bake_ref.tables(scene), pts, S, SEED, world=world)
    want, D, acc = _bake_ref.bake_from_existing_calls(ds, ref, DEPTH, SEED)
    for a in (want, D, acc):
        a.setflags(write=False)
    return pts, ref, want, D, acc


@functools.lru_cache(maxsize=None)
def _world_points(name):
    """WORLD points where the camera grid hits something that is not a mesh (patches, spheres): the hit point, facing the camera."""
    scene, ds = _scene(name), _ds(name)
    rays, hits = _grid_hits(scene, ds, CAMERAS[name])
    inst = scene.array("instances")
    other = (hits["instance"] >= 0) & (inst["prim_type"][np.maximum(hits["instance"], 0)] != 1)
    pts = np.zeros(int(other.sum()), dtype=spt.BAKE_WORLD_DTYPE)
    pts["p"] = rays["o"][other] + rays["d"][other] * hits["t"][other][:, None]
    pts["n"] = -rays["d"][other]
    pts.setflags(write=False)
    return pts


def _check(got, want, what):
    assert got.shape == want.shape
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    assert _util.same_words(got, want), "%s: %d of %d words differ from the reference built from radiance and trace_any" % (what, int(bad.sum()), bad.size)


# ---- 1. parity --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials", "t_medium", "t_textured"])
def test_a_bake_is_the_delta_sum_plus_the_mean_of_radiance(name):
    pts, ref, want, D, acc = _reference(name)
    assert len(pts) >= 1500
    got = _ds(name).bake(pts, samples=S, max_depth=DEPTH, seed=SEED)
    _check(got, want, name)
    lit = np.any(D > 0, axis=-1)
    if name == "cfg2_cube":       # fused, LDS-resident: faces towards and away from the light
        assert lit.any() and (~lit).any()
    if name == "t_materials":     # class queues, environment, three delta lights
        assert len(np.unique(D[lit], axis=0)) > 10
        assert np.mean(np.any(acc != 0, axis=-1)) > 0.5
    if name in ("t_medium", "t_textured"):
        assert np.any(acc != 0)


@pytest.mark.parametrize("name", ["t_materials", "t_medium", "t_textured"])
def test_a_bake_is_the_oracles_delta_sum_plus_the_mean_of_the_oracles_radiance(name):
    """The same restated rays, but no device call on the expected side: _util.OracleScene stands in for the DeviceScene, so D is gated
    by oracle_trace_any and the gather term is oracle_radiance's (trace_ray from points on surfaces, which no camera ray reaches)."""
    pts, ref, _, _, _ = _reference(name)
    want, D, acc = _bake_ref.bake_from_existing_calls(_util.OracleScene(_scene(name)), ref, DEPTH, SEED)
    gathered = np.isfinite(acc).all(axis=-1) & np.any(acc != 0, axis=-1)
    assert gathered.mean() >= (0.05 if name == "t_medium" else 0.25) and len(np.unique(acc[gathered], axis=0)) >= 100
    if name != "t_medium":        # (t_medium has no delta light)
        assert np.any(D > 0) and not np.all(np.any(D > 0, axis=-1))
    got = _ds(name).bake(pts, samples=S, max_depth=DEPTH, seed=SEED)
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    assert _util.same_words(got, want), "%s: %d of %d words differ from the reference built from the oracle" % (name, int(bad.sum()), bad.size)


def test_a_scene_with_patches_is_forwarded():
    name = "t_bezier"
    pts, ref, want, D, acc = _reference(name, world=True)       # WORLD points on the patches (and the sphere)
    assert len(pts) > 100 and np.any(D > 0) and np.any(acc != 0)
    _check(_ds(name).bake(pts, samples=S, max_depth=DEPTH, seed=SEED, world=True), want, "t_bezier, world points")
    mesh_pts, _, mesh_want, _, _ = _reference(name)            # the floor's mesh points
    assert len(mesh_pts) > 20
    _check(_ds(name).bake(mesh_pts, samples=S, max_depth=DEPTH, seed=SEED), mesh_want, "t_bezier, mesh points")


def test_world_points_and_flip():
    name = "t_materials"
    pts, ref, want, D, acc = _reference(name, world=True)      # the spheres of the scene
    assert len(pts) > 100
    ds = _ds(name)
    _check(ds.bake(pts, samples=S, max_depth=DEPTH, seed=SEED, world=True), want, "world points")
    # flip: the reference of the negated normals
    back = pts.copy()
    back["n"] = -back["n"]
    _check(ds.bake(back, samples=S, max_depth=DEPTH, seed=SEED, world=True, flip=True), want, "flipped back")
    surf = _points(name)[:200]
    fref = _bake_ref.bake_inputs(spt, _bake_ref.tables(_scene(name)), surf, S, SEED, flip=True)
    fwant, _, _ = _bake_ref.bake_from_existing_calls(ds, fref, DEPTH, SEED)
    _check(ds.bake(surf, samples=S, max_depth=DEPTH, seed=SEED, flip=True), fwant, "flipped surface points")
    assert not _util.same_words(fwant, _reference(name)[2][:200])


# the walkers of scenes that do not fit LDS: the streaming intake kernel, and the walker over the geometry in memory
@pytest.mark.parametrize("switches", [{"SPT_NO_LDS_GEO": "1"}, {"SPT_NO_LDS_GEO": "1", "SPT_NO_STREAM": "1"}], ids=["stream", "memory"])
def test_large_scene_walkers(monkeypatch, switches):
    name = "t_materials"
    pts, ref, want, D, acc = _reference(name)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)      # (read when the device scene is made)
    sc = spt.load_scene(os.path.join(_util.SCENES, name + ".json"))
    try:
        got = sc.device_scene(0).bake(pts, samples=S, max_depth=DEPTH, seed=SEED)
    finally:
        sc.close()
    _check(got, want, name)


# ---- 2. max_depth 0 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_max_depth_zero_is_the_delta_sum(name):
    pts, ref, want, D, acc = _reference(name)
    _check(_ds(name).bake(pts, samples=S, max_depth=0, seed=SEED), D, name)


# ---- 3. ragged sizes, passes, chunks ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_ragged_sizes_and_passes(name):
    pts, ref, want, D, acc = _reference(name)
    ds = _ds(name)
    first = 200
    for n in (1, 63, 65, 257):
        got = ds.bake(pts[first:first + n], samples=S, max_depth=DEPTH, seed=SEED, first_point=first)
        _check(got, want[first:first + n], "%d points inside the list" % n)
    for per_pass in (1000, 700):
        _check(ds.bake(pts, samples=S, max_depth=DEPTH, seed=SEED, points_per_pass=per_pass), want, "points_per_pass %d" % per_pass)
    # without first_point the same records are other points of the stream
    if name == "t_materials":
        assert not _util.same_words(ds.bake(pts[first:first + 65], samples=S, max_depth=DEPTH, seed=SEED), want[first:first + 65])


@pytest.mark.parametrize("name,count,depth", [("cfg2_cube", 300, DEPTH), ("t_materials", 16, 2)])
def test_samples_across_a_chunk_boundary(name, count, depth):
    """513 samples: the default chunk is 512 samples, so the last one arrives in a chunk of its own and is added onto rgb_out."""
    pts = _points(name)[100:100 + count]
    ds = _ds(name)
    ref = _bake_ref.bake_inputs(spt, _bake_ref.tables(_scene(name)), pts, 513, SEED, first_point=100)
    want, D, acc = _bake_ref.bake_from_existing_calls(ds, ref, depth, SEED)
    _check(ds.bake(pts, samples=513, max_depth=depth, seed=SEED, first_point=100), want, name)
    if name == "t_materials":
        assert np.any(acc != 0)


def test_first_sample_continues_the_streams():
    """Two calls of 2 samples each, first_sample 0 and 2: each is D + the in-order mean of its own two samples of the 4-sample
    reference; their average is the 4-sample result up to the association of the sum (a few ulp of the largest term)."""
    name = "t_materials"
    pts, ref, want, D, acc = _reference(name)
    ds = _ds(name)
    halves = []
    for fs in (0, 2):
        part = dict(ref)
        part["rays"] = np.ascontiguousarray(ref["rays"][:, fs:fs + 2])
        half_want, _, _ = _bake_ref.bake_from_existing_calls(ds, part, DEPTH, SEED)
        got = ds.bake(pts, samples=2, max_depth=DEPTH, seed=SEED, first_sample=fs)
        _check(got, half_want, "first_sample %d" % fs)
        halves.append(got)
    assert not _util.same_words(halves[0], halves[1])
    mean = (halves[0].astype(np.float64) + halves[1]) / 2
    tol = 8 * np.finfo(f32).eps * np.maximum(np.abs(want), np.maximum(np.abs(halves[0]), np.abs(halves[1])))
    assert np.all(np.abs(mean - want) <= tol + 1e-30)


# ---- 4. analytic --------------------------------------------------------------------------------------------------------------------

def test_a_convex_body_in_the_void_gathers_nothing():
    """cfg2 is a cube under one directional light in the void: the gather term is exactly 0, so out == D, and D is strength * cos / pi
    on the faces turned to the light (under ten rounded f32 operations: within 1e-5 relative of float64) and 0 on the others."""
    name = "cfg2_cube"
    pts, ref, want, D, acc = _reference(name)
    assert not acc.any()
    got = _ds(name).bake(pts, samples=S, max_depth=DEPTH, seed=SEED)
    _check(got, D, name)
    light = _scene(name).array("lights")[0]
    assert light["type"] == 0
    to_light = -light["dir"].astype(np.float64)
    cos = ref["nrm"].astype(np.float64) @ to_light
    lit = cos > 1e-6
    assert lit.any() and (cos < -1e-6).any()
    analytic = light["strength"].astype(np.float64)[None, :] * cos[:, None] / np.pi
    assert np.all(np.abs(got[lit] - analytic[lit]) <= 1e-5 * analytic[lit])
    assert not got[cos < -1e-6].any()


# ---- 5. moving scenes ---------------------------------------------------------------------------------------------------------------

def _device_tables(scene, ds):
    """The reference's tables with the triangle records the device holds (read_triangles) and the Scene's current instances."""
    tab = _bake_ref.tables(scene)
    pos, attr = tab["tri_pos"].copy(), tab["tri_attr"].copy()
    for m, mesh in enumerate(tab["meshes"]):
        p, a = ds.read_triangles(m)
        pos[mesh["tri_first"]:mesh["tri_first"] + mesh["tri_count"]] = p
        attr[mesh["tri_first"]:mesh["tri_first"] + mesh["tri_count"]] = a
    tab["tri_pos"], tab["tri_attr"] = pos, attr
    return tab


def test_a_bake_follows_moved_instances_and_deformed_meshes():
    name = "t_materials"
    path = os.path.join(_util.SCENES, name + ".json")
    sc = spt.load_scene(path)
    try:
        ds = sc.device_scene(0)
        before = ds.bake(_random_points(sc, 24, 3), samples=S, max_depth=DEPTH, seed=SEED)
        # 1. an instance moves (the instance order may change with it: the points are named in the new order)
        c, s = np.cos(0.7), np.sin(0.7)
        sc.set_transforms({"red_cube": np.array([[c, 0, s, 1.5], [0, 1.2, 0, 0.9], [-s, 0, c, -0.5]], dtype=f32)})
        ds.update()
        pts = _random_points(sc, 24, 3)
        ref = _bake_ref.bake_inputs(spt, _device_tables(sc, ds), pts, S, SEED)
        want, D, acc = _bake_ref.bake_from_existing_calls(ds, ref, DEPTH, SEED)
        moved = ds.bake(pts, samples=S, max_depth=DEPTH, seed=SEED)
        _check(moved, want, "after set_transforms + update")
        assert not _util.same_words(moved, before)
        # 2. a mesh is deformed from its vertices: the device makes its own records, the host's are not consulted
        rest = sc.mesh_positions("cube")
        bent = rest.copy()
        bent[:, 1] += f32(0.25) * np.sin(f32(2.0) * rest[:, 0])
        sc.set_mesh_vertices("cube", bent)
        ds.update()
        pts = _random_points(sc, 24, 3)      # (the instance order follows the new boxes)
        ref = _bake_ref.bake_inputs(spt, _device_tables(sc, ds), pts, S, SEED)
        want2, _, _ = _bake_ref.bake_from_existing_calls(ds, ref, DEPTH, SEED)
        deformed = ds.bake(pts, samples=S, max_depth=DEPTH, seed=SEED)
        _check(deformed, want2, "after set_mesh_vertices + update")
        assert not _util.same_words(deformed, moved)
        # 3. a freshly created scene in the same state
        fresh = spt.load_scene(path)
        try:
            fresh.set_transforms({"red_cube": np.array([[c, 0, s, 1.5], [0, 1.2, 0, 0.9], [-s, 0, c, -0.5]], dtype=f32)})
            fresh.set_mesh_positions("cube", bent)
            assert np.array_equal(_random_points(fresh, 24, 3), pts)
            _check(fresh.device_scene(0).bake(pts, samples=S, max_depth=DEPTH, seed=SEED), deformed, "a fresh scene")
        finally:
            fresh.close()
    finally:
        sc.close()


# ---- 6. device pointers -------------------------------------------------------------------------------------------------------------

_CHILD = r"""
import os, sys
import torch                                  # before the package: the tensor path must work in a process torch initialised
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import _util
spt = _util.load_pkg()
sc = spt.load_scene(os.path.join(_util.SCENES, "t_materials.json"))
ds = sc.device_scene(0)
rng = np.random.default_rng(4)
inst, meshes = sc.array("instances"), sc.array("meshes")
rows = []
for i, rec in enumerate(inst):
    if rec["prim_type"] != 1:
        continue
    m = meshes[rec["prim_id"]]
    p = np.zeros(150, dtype=spt.BAKE_POINT_DTYPE)
    p["instance"], p["prim"] = i, m["tri_first"] + rng.integers(0, m["tri_count"], size=150)
    a, b = rng.random(150), rng.random(150)
    p["v"], p["w"] = np.where(a + b > 1, 1 - a, a), np.where(a + b > 1, 1 - b, b)
    rows.append(p)
pts = np.concatenate(rows)
host = ds.bake(pts, samples=3, max_depth=5, seed=11, first_point=9)
dev = torch.device("cuda", 0)
t_pts = torch.from_numpy(pts.view(np.float32).reshape(-1, 4).copy()).to(dev)
t_out = ds.bake(t_pts, samples=3, max_depth=5, seed=11, first_point=9)
assert t_out.device == dev and t_out.shape == (pts.shape[0], 3)
assert _util.same_words(t_out.cpu().numpy(), host), "tensor bake differs from the host path"
assert np.isfinite(host).all() and host.max() > 0.01
made = spt.bake_rays(sc, pts, samples=1)
wp = np.zeros(pts.shape[0], dtype=spt.BAKE_WORLD_DTYPE)
wp["p"], wp["n"] = made["pos"], made["nrm"]
t_wp = torch.from_numpy(wp.view(np.float32).reshape(-1, 8).copy()).to(dev)
t_world = ds.bake(t_wp, samples=3, max_depth=5, seed=11, first_point=9, world=True)
assert _util.same_words(t_world.cpu().numpy(), host), "resolved points given as WORLD tensors differ"
# a host pointer under the device-pointer flag is refused and writes nothing
import ctypes
job = spt.BakeJob(size=ctypes.sizeof(spt.BakeJob), flags=spt.BAKE_DEVICE_POINTERS, n_points=pts.shape[0], samples=1, max_depth=5, seed=11)
out = np.full((pts.shape[0], 3), np.float32(7.0))
job.points, job.rgb_out = pts.ctypes.data, out.ctypes.data
assert spt.hip_lib().spt_bake(ds._h, ctypes.byref(job)) == 1 and (out == 7.0).all()
job.points, job.rgb_out = t_pts.data_ptr(), out.ctypes.data
assert spt.hip_lib().spt_bake(ds._h, ctypes.byref(job)) == 1 and (out == 7.0).all()
job.points, job.rgb_out = t_pts.data_ptr() + 4, t_out.data_ptr()
assert spt.hip_lib().spt_bake(ds._h, ctypes.byref(job)) == 1
assert _util.same_words(ds.bake(t_pts, samples=3, max_depth=5, seed=11, first_point=9).cpu().numpy(), host)
sc.close()
print("bake tensors ok")
"""


def test_device_pointers_in_a_process_that_imported_torch_first():
    res = subprocess.run([sys.executable, "-c", _CHILD, _util.ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "bake tensors ok" in res.stdout, res.stdout + res.stderr


# ---- 7. isolation -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_films_and_async_frames_are_undisturbed(name):
    sc = _scene(name)
    pts, ref, want, D, acc = _reference(name)
    cfg = spt.OutputConfig(W, H, None, CAMERAS[name])
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=8, seed=3)
    with r.progressive(sc, cfg) as plain:
        undisturbed = plain.render(4).render(4).mean().copy()
    with r.progressive(sc, cfg) as film:
        film.render(4)
        _check(_ds(name).bake(pts, samples=S, max_depth=DEPTH, seed=SEED), want, "between two increments")
        assert _util.same_words(film.render(4).mean(), undisturbed)
    sync = r.render_shard(sc, cfg).copy()
    buf = r.render_shard(sc, cfg, reuse_output=True, wait=False)
    _check(_ds(name).bake(pts, samples=S, max_depth=DEPTH, seed=SEED), want, "behind an asynchronous frame")
    r.wait(sc)
    assert _util.same_words(np.array(buf), sync)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_leave_the_scene_usable():
    name = "t_materials"
    pts, ref, want, D, acc = _reference(name)
    sc, ds = _scene(name), _ds(name)
    lib = spt.hip_lib()
    n = pts.shape[0]
    out = np.empty((n, 3), dtype=f32)
    inst, meshes = sc.array("instances"), sc.array("meshes")
    sphere = int(np.flatnonzero(inst["prim_type"] == 0)[0])
    cube = int(np.flatnonzero((inst["prim_type"] == 1) & (inst["prim_id"] == 0))[0])

    def job(arr=pts, **kw):
        j = spt.BakeJob(size=C.sizeof(spt.BakeJob), n_points=arr.shape[0], samples=S, max_depth=DEPTH, seed=SEED)
        j.points, j.rgb_out = arr.ctypes.data, out.ctypes.data
        j.keep = arr      # (the job's pointer does not own the array)
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(j, scene=ds._h, word=None, status=1):
        out.view(np.uint32)[:] = PATTERN
        assert lib.spt_bake(scene, C.byref(j) if j is not None else None) == status
        assert (out.view(np.uint32) == PATTERN).all()
        if word is not None:
            assert word in lib.spt_last_error().decode(), lib.spt_last_error()

    def edited(at, **fields):
        bad = pts.copy()
        for k, v in fields.items():
            bad[k][at] = v
        return bad

    refused(job(), scene=None)
    refused(None)
    refused(job(points=None))
    refused(job(rgb_out=None))
    refused(job(flags=4), word="flags")
    refused(job(flags=0x80000000), word="flags")
    refused(job(kind=2), word="kind")
    refused(job(samples=0), word="samples")
    refused(job(size=C.sizeof(spt.BakeJob) - 8), word="size")
    refused(job(max_depth=256), status=4)
    refused(job(edited(5, instance=sphere)), word="point 5 ")
    refused(job(edited(n - 1, instance=cube, prim=meshes[1]["tri_first"])), word="point %d " % (n - 1))
    refused(job(edited(700, instance=cube, prim=meshes[1]["tri_first"]), points_per_pass=256), word="point 700 ")   # a later pass: still nothing written
    refused(job(edited(3, instance=len(inst))), word="point 3 ")
    refused(job(edited(0, v=np.nan)), word="point 0 ")
    wp = _world_points(name).copy()
    wp["n"][7] = 0.0
    refused(job(wp, kind=spt.BAKE_POINTS_WORLD, n_points=min(len(wp), n)), word="point 7 ")
    refused(job(flags=spt.BAKE_DEVICE_POINTERS), word="device")
    # nothing to do is not a refusal, and writes nothing either
    refused(job(n_points=0), status=0)
    refused(job(n_points=0, points=None, rgb_out=None), status=0)
    # a good call after all of them, and a render
    _check(ds.bake(pts, samples=S, max_depth=DEPTH, seed=SEED), want, "after the refusals")
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=2, seed=3)
    assert np.isfinite(r.render_shard(sc, spt.OutputConfig(W, H, None, CAMERAS[name]))).any()


# ---- 9. the CLI ---------------------------------------------------------------------------------------------------------------------

def test_the_cli_writes_the_lightmap_of_lightmap_points_and_bake(tmp_path):
    name = "t_textured"
    sc = _scene(name)
    cli = os.path.join(spt.LIB_DIR, "spt")
    out = tmp_path / "map.exr"
    renderer = os.path.join(_util.SCENES, "pt.json")
    base = [cli, "-s", os.path.join(_util.SCENES, name + ".json"), "-r", renderer, "-o", str(out), "--bake-lightmap", "floor", "--bake-size", "16x16",
            "--bake-samples", "4", "--seed", "5"]
    res = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    pts, texels = sc.lightmap_points("floor", 16, 16)
    assert len(pts) == 256
    depth = spt.load_renderer(renderer).max_depth
    want = np.zeros((16 * 16, 3), dtype=f32)
    want[texels] = _ds(name).bake(pts, samples=4, max_depth=depth, seed=5)
    got = spt.read_exr(str(out))
    assert got.shape == (16, 16, 3) and _util.same_words(np.ascontiguousarray(got, dtype=f32).reshape(-1, 3), want)
    assert want.max() > 0.01
    # a film option alongside it: exit code 2, nothing written
    out.unlink()
    res = subprocess.run(base + ["--preview-every", "2"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and not out.exists(), res.stdout + res.stderr

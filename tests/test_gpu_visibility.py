"""spt_occluded (DeviceScene.occluded) and spt_ao (DeviceScene.ambient_occlusion): any-hit queries along caller segments and ambient
occlusion at bake points, the rays made on the device.

Every expected value comes from calls that exist without them.  occluded is compared with DeviceScene.trace_any byte for byte;
ambient_occlusion with tests/_visibility_ref.py over spt.bake_rays (the gather rays of the bake with the same seed and streams) and
DeviceScene.trace_any.  Every comparison is _util.same_words; no ray or point is left out.  tests/test_visibility_abi.py shows on the
CPU oracle that the expected records are neither all open nor all closed; test_ao_is_the_oracles_any_hit_over_the_gather_rays ties
the device's words to the oracle.

Segments: the gather rays of about 1500 points x 4 samples (tests/test_gpu_bake.py's point recipe) with t_max f32::MAX and 1/16 of the
scene's extent, plus the 48 x 36 camera rays."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _util
import _visibility_ref as ref

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32

W, H, S, SEED = 48, 36, 4, 11
PATTERN8 = np.uint8(0xa5)
PATTERN32 = np.uint32(0x7fc0beef)   # (a NaN no record holds)
CAMERAS = {"cfg2_cube": None, "t_materials": "main", "t_medium": None, "t_textured": None, "t_bezier": "main"}
SCENES5 = ["cfg2_cube", "t_materials", "t_medium", "t_textured", "t_bezier"]


@functools.lru_cache(maxsize=None)
def _scene(name):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_util.SCENES, name + ".json"))


def _ds(name):
    return _scene(name).device_scene(0)


def _camera_segments(scene, camera):
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=1, seed=SEED)
    return _util.first_segments(spt.camera_rays(spt.CameraModel.perspective(scene.get_camera(camera)), r, W, H).reshape(-1))


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
    hits = ds.trace_closest(_camera_segments(scene, CAMERAS[name]))
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
def _world_points(name):
    """WORLD points where the camera grid hits something that is not a mesh (patches, spheres): the hit point, facing the camera."""
    scene, ds = _scene(name), _ds(name)
    rays = _camera_segments(scene, CAMERAS[name])
    hits = ds.trace_closest(rays)
    inst = scene.array("instances")
    other = (hits["instance"] >= 0) & (inst["prim_type"][np.maximum(hits["instance"], 0)] != 1)
    pts = np.zeros(int(other.sum()), dtype=spt.BAKE_WORLD_DTYPE)
    pts["p"] = rays["o"][other] + rays["d"][other] * hits["t"][other][:, None]
    pts["n"] = -rays["d"][other]
    pts.setflags(write=False)
    return pts


def _near(name):
    return float(ref.scene_extent(_scene(name)) / f32(16))


@functools.lru_cache(maxsize=None)
def _made(name, world=False, flip=False):
    """spt.bake_rays of the scene's points: the gather rays of an AO call with (SEED, first_point 0, first_sample 0)."""
    return spt.bake_rays(_scene(name), _world_points(name) if world else _points(name), samples=S, seed=SEED, world=world, flip=flip)


@functools.lru_cache(maxsize=None)
def _segments(name):
    """(segments, trace_any's bytes): read-only."""
    scene = _scene(name)
    rays = _made(name)["rays"].reshape(-1)
    seg = np.concatenate([ref.segments(spt, rays), ref.segments(spt, rays, _near(name)), _camera_segments(scene, CAMERAS[name])])
    want = _ds(name).trace_any(seg)
    seg.setflags(write=False)
    want.setflags(write=False)
    return seg, want


@functools.lru_cache(maxsize=None)
def _ao_want(name, dist=np.inf, world=False, flip=False):
    rec = ref.ao_records(spt, _made(name, world, flip), _ds(name).trace_any, dist)
    rec.setflags(write=False)
    return rec


def _same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), "%s: %d of %d differ from trace_any" % (what, int((got != want).sum()), want.size)


def _check(got, want, what):
    assert got.dtype == spt.AO_DTYPE and got.shape == want.shape, what
    g, w = ref.words(got), ref.words(want)
    assert _util.same_words(g, w), "%s: %d of %d words differ from the reference built from bake_rays and trace_any" % (what, int((g != w).sum()), w.size)


# ---- 1. occluded is trace_any -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES5)
def test_occluded_is_trace_any(name):
    seg, want = _segments(name)
    assert len(seg) >= 2 * 1500 * S + W * H
    ds = _ds(name)
    _same_bytes(ds.occluded(seg), want, name)
    _same_bytes(ds.occluded(seg, packed=True), spt.pack_occluded(want), name + ", packed")
    gather = want[:len(seg) - W * H].reshape(2, -1)
    if name == "cfg2_cube":      # a convex body in the void: nothing occludes its own surface; the camera sees it before the void
        assert gather.mean() < 0.01 and want[-W * H:].any() and not want[-W * H:].all()
    else:
        assert 0.05 < gather[0].mean() < 0.95 and gather[1].mean() < gather[0].mean()


@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_occluded_ragged_counts_and_passes(name):
    seg, want = _segments(name)
    ds = _ds(name)
    first = 200
    for n in (1, 63, 64, 65, 257):
        _same_bytes(ds.occluded(seg[first:first + n]), want[first:first + n], "%d rays inside the list" % n)
        _same_bytes(ds.occluded(seg[first:first + n], packed=True), spt.pack_occluded(want[first:first + n]), "%d rays inside the list, packed" % n)
    for per_pass in (1000, 700):
        _same_bytes(ds.occluded(seg, rays_per_pass=per_pass), want, "rays_per_pass %d" % per_pass)
        _same_bytes(ds.occluded(seg, packed=True, rays_per_pass=per_pass), spt.pack_occluded(want), "rays_per_pass %d, packed" % per_pass)


# ---- 2. ambient occlusion is the reference over bake_rays and trace_any ------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials", "t_medium", "t_textured"])
def test_ao_is_the_any_hit_over_the_gather_rays(name):
    pts, ds = _points(name), _ds(name)
    assert len(pts) >= 1500
    for dist in (np.inf, _near(name)):
        want = _ao_want(name, dist)
        _check(ds.ambient_occlusion(pts, samples=S, max_distance=dist, seed=SEED), want, "%s, max_distance %g" % (name, dist))
    far, near = _ao_want(name), _ao_want(name, _near(name))
    if name == "cfg2_cube":
        assert far["count"].mean() > 0.99 * S
    else:
        assert 0 < far["count"].sum() < near["count"].sum() < S * len(pts)
    if name in ("t_materials", "t_textured"):
        assert (np.bincount(far["count"], minlength=S + 1) > 0).all()


def test_ao_is_the_oracles_any_hit_over_the_gather_rays():
    """No device call on the expected side: _util.OracleScene's trace_any judges the rays."""
    name = "t_materials"
    oracle = _util.OracleScene(_scene(name))
    for dist in (np.inf, _near(name)):
        want = ref.ao_records(spt, _made(name), oracle.trace_any, dist)
        _check(_ds(name).ambient_occlusion(_points(name), samples=S, max_distance=dist, seed=SEED), want, "max_distance %g" % dist)


def test_a_scene_with_patches_is_forwarded():
    name = "t_bezier"
    ds = _ds(name)
    wp = _world_points(name)                   # WORLD points on the patches (and the sphere)
    assert len(wp) > 100
    for dist in (np.inf, _near(name)):
        want = _ao_want(name, dist, world=True)
        _check(ds.ambient_occlusion(wp, samples=S, max_distance=dist, seed=SEED, world=True), want, "t_bezier, world points, max_distance %g" % dist)
    assert 0 < _ao_want(name, world=True)["count"].sum() < S * len(wp)
    _check(ds.ambient_occlusion(_points(name), samples=S, seed=SEED), _ao_want(name), "t_bezier, mesh points")


def test_ao_world_points_and_flip():
    name = "t_materials"
    ds = _ds(name)
    wp = _world_points(name)                   # the spheres of the scene
    assert len(wp) > 100
    want = _ao_want(name, world=True)
    _check(ds.ambient_occlusion(wp, samples=S, seed=SEED, world=True), want, "world points")
    back = wp.copy()
    back["n"] = -back["n"]
    _check(ds.ambient_occlusion(back, samples=S, seed=SEED, world=True, flip=True), want, "flipped back")
    fwant = _ao_want(name, flip=True)
    _check(ds.ambient_occlusion(_points(name), samples=S, seed=SEED, flip=True), fwant, "flipped surface points")
    assert not _util.same_words(ref.words(fwant), ref.words(_ao_want(name)))
    # a convex body seen from inside: every ray ends on it, but for grazing ones from the random points on its edges and corners
    cube = _ds("cfg2_cube").ambient_occlusion(_points("cfg2_cube"), samples=S, seed=SEED, flip=True)
    _check(cube, _ao_want("cfg2_cube", flip=True), "cfg2_cube from inside")
    closed = cube["count"] == 0
    assert closed.mean() > 0.9 and closed[:200].all() and not ref.words(cube)[closed, :7].any()


@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_ao_ragged_counts_and_passes(name):
    pts, ds, want = _points(name), _ds(name), _ao_want(name)
    first = 200
    for n in (1, 63, 65, 257):
        got = ds.ambient_occlusion(pts[first:first + n], samples=S, seed=SEED, first_point=first)
        _check(got, want[first:first + n], "%d points inside the list" % n)
    for per_pass in (1000, 700):
        _check(ds.ambient_occlusion(pts, samples=S, seed=SEED, points_per_pass=per_pass), want, "points_per_pass %d" % per_pass)
    if name == "t_materials":      # without first_point the same records are other points of the stream
        assert not _util.same_words(ref.words(ds.ambient_occlusion(pts[first:first + 65], samples=S, seed=SEED)), ref.words(want[first:first + 65]))


def test_ao_samples_across_a_launch_boundary():
    """513 samples on 16 points: a launch takes at most 512 samples, so the last one is added onto the out record by a launch of its own."""
    name = "t_materials"
    pts, ds = _points(name)[100:116], _ds(name)
    made = spt.bake_rays(_scene(name), pts, samples=513, seed=SEED, first_point=100)
    want = ref.ao_records(spt, made, ds.trace_any, _near(name))
    assert 0 < want["count"].sum() < 513 * 16
    _check(ds.ambient_occlusion(pts, samples=513, max_distance=_near(name), seed=SEED, first_point=100), want, "513 samples")
    # ... and with next to nothing in reach: the launch of the last sample adds its direction onto the sum it was handed
    occ = ref.occlusion(spt, made, ds.trace_any, 1e-3)
    assert (occ[:, 512] == 0).any()
    _check(ds.ambient_occlusion(pts, samples=513, max_distance=1e-3, seed=SEED, first_point=100), ref.ao_records(spt, made, None, occ=occ), "513 open samples")


def test_first_sample_continues_the_streams():
    """Two calls of 2 samples each, first_sample 0 and 2: each is the reference over its own two columns of the 4-sample rays; their
    counts add up to the one call's, and going on from the first half's sum and count gives the one call's sum word for word."""
    name = "t_materials"
    pts, ds, made, whole = _points(name), _ds(name), _made(name), _ao_want(name)
    occ = ref.occlusion(spt, made, ds.trace_any)
    halves = []
    for fs in (0, 2):
        part = {"rays": np.ascontiguousarray(made["rays"][:, fs:fs + 2])}
        want = ref.ao_records(spt, part, None, occ=occ[:, fs:fs + 2])
        got = ds.ambient_occlusion(pts, samples=2, seed=SEED, first_sample=fs)
        _check(got, want, "first_sample %d" % fs)
        halves.append(got)
    assert not _util.same_words(ref.words(halves[0]), ref.words(halves[1]))
    assert np.array_equal(halves[0]["count"] + halves[1]["count"], whole["count"])
    joined = ref.ao_records(spt, {"rays": np.ascontiguousarray(made["rays"][:, 2:])}, None, occ=occ[:, 2:], start=halves[0], finish=False)
    assert _util.same_words(joined["sum"], whole["sum"]) and np.array_equal(joined["count"], whole["count"])


# ---- 3. the walkers of scenes that do not fit LDS ------------------------------------------------------------------------------------

@pytest.mark.parametrize("switches", [{"SPT_NO_LDS_GEO": "1"}, {"SPT_NO_LDS_GEO": "1", "SPT_NO_STREAM": "1"}], ids=["stream", "memory"])
def test_large_scene_walkers(monkeypatch, switches):
    name = "t_materials"
    seg, want = _segments(name)
    pts = _points(name)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)      # (read when the device scene is made)
    sc = spt.load_scene(os.path.join(_util.SCENES, name + ".json"))
    try:
        ds = sc.device_scene(0)
        _same_bytes(ds.trace_any(seg), want, "trace_any itself")
        _same_bytes(ds.occluded(seg), want, name)
        _same_bytes(ds.occluded(seg, packed=True, rays_per_pass=700), spt.pack_occluded(want), name + ", packed")
        for dist in (np.inf, _near(name)):
            _check(ds.ambient_occlusion(pts, samples=S, max_distance=dist, seed=SEED), _ao_want(name, dist), "max_distance %g" % dist)
        _check(ds.ambient_occlusion(pts[100:116], samples=513, seed=SEED, first_point=100),
               ref.ao_records(spt, spt.bake_rays(sc, pts[100:116], samples=513, seed=SEED, first_point=100), ds.trace_any), "513 samples")
    finally:
        sc.close()


# ---- 4. moving scenes ---------------------------------------------------------------------------------------------------------------

def test_both_calls_follow_moved_instances_and_deformed_meshes():
    name = "t_materials"
    path = os.path.join(_util.SCENES, name + ".json")
    seg, still = _segments(name)
    sc = spt.load_scene(path)
    fresh = []
    try:
        ds = sc.device_scene(0)
        c, s = np.cos(0.7), np.sin(0.7)
        xf = {"red_cube": np.array([[c, 0, s, 1.5], [0, 1.2, 0, 0.9], [-s, 0, c, -0.5]], dtype=f32)}
        rest = sc.mesh_positions("cube")
        bent = rest.copy()
        bent[:, 1] += f32(0.25) * np.sin(f32(2.0) * rest[:, 0])

        def fresh_scene(deformed):
            f = spt.load_scene(path)
            fresh.append(f)
            f.set_transforms(xf)
            if deformed:
                f.set_mesh_positions("cube", bent)
            return f, f.device_scene(0)

        before = ds.ambient_occlusion(_random_points(sc, 24, 3), samples=S, seed=SEED)
        sc.set_transforms(xf)
        ds.update()
        last_occ, last_ao = still, before
        for step in ("set_transforms", "set_mesh_vertices"):
            if step == "set_mesh_vertices":
                sc.set_mesh_vertices("cube", bent)
                ds.update()
            f, fds = fresh_scene(step == "set_mesh_vertices")
            pts = _random_points(f, 24, 3)      # (the instance order follows the new boxes)
            assert np.array_equal(_random_points(sc, 24, 3), pts)
            occ = ds.occluded(seg)
            _same_bytes(occ, fds.trace_any(seg), "after %s + update: a fresh scene's trace_any" % step)
            _same_bytes(occ, fds.occluded(seg), "after %s + update: a fresh scene's occluded" % step)
            _same_bytes(ds.occluded(seg, packed=True), spt.pack_occluded(occ), "after %s + update, packed" % step)
            ao = ds.ambient_occlusion(pts, samples=S, seed=SEED)
            _check(ao, ref.ao_records(spt, spt.bake_rays(f, pts, samples=S, seed=SEED), fds.trace_any), "after %s + update: a fresh scene's reference" % step)
            _check(ao, fds.ambient_occlusion(pts, samples=S, seed=SEED), "after %s + update: a fresh scene's records" % step)
            assert not np.array_equal(occ, last_occ) and not _util.same_words(ref.words(ao), ref.words(last_ao))
            last_occ, last_ao = occ, ao
    finally:
        for f in fresh:
            f.close()
        sc.close()


# ---- 5. device pointers -------------------------------------------------------------------------------------------------------------

_CHILD = r"""
import ctypes, os, sys
import torch                                  # before the package: the tensor path must work in a process torch initialised
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import _util
import _visibility_ref as ref
spt = _util.load_pkg()
sc = spt.load_scene(os.path.join(_util.SCENES, "t_materials.json"))
ds = sc.device_scene(0)
dev = torch.device("cuda", 0)
lib = spt.hip_lib()
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
made = spt.bake_rays(sc, pts, samples=3, seed=11, first_point=9)

# occluded: the same words as the host call, which is trace_any
seg = np.concatenate([ref.segments(spt, made["rays"].reshape(-1)), ref.segments(spt, made["rays"].reshape(-1), 0.9)])
host = ds.occluded(seg)
assert np.array_equal(host, ds.trace_any(seg)) and 0.05 < host.mean() < 0.95
t_seg = torch.from_numpy(seg.view(np.float32).reshape(-1, 8).copy()).to(dev)
t_occ = ds.occluded(t_seg)
assert t_occ.device == dev and t_occ.dtype == torch.uint8 and t_occ.shape == (seg.shape[0],)
assert np.array_equal(t_occ.cpu().numpy(), host), "tensor occluded differs from the host path"
for n in (1, 63, 64, 65, 257, seg.shape[0]):
    t_pk = ds.occluded(t_seg[:n].contiguous(), packed=True, rays_per_pass=700)
    assert t_pk.dtype == torch.int64 and t_pk.shape == ((n + 63) // 64,)
    assert np.array_equal(t_pk.cpu().numpy().view(np.uint64), spt.pack_occluded(host[:n])), "packed tensor, %d rays" % n

# ambient occlusion: the same words as the host call, which is the reference
want = ref.ao_records(spt, made, ds.trace_any, 0.9)
host_ao = ds.ambient_occlusion(pts, samples=3, max_distance=0.9, seed=11, first_point=9)
assert _util.same_words(ref.words(host_ao), ref.words(want))
t_pts = torch.from_numpy(pts.view(np.float32).reshape(-1, 4).copy()).to(dev)
t_ao = ds.ambient_occlusion(t_pts, samples=3, max_distance=0.9, seed=11, first_point=9)
assert t_ao.device == dev and t_ao.shape == (pts.shape[0], 8)
assert _util.same_words(t_ao.cpu().numpy().view(np.uint32), ref.words(want)), "tensor ambient_occlusion differs from the host path"
assert np.array_equal(t_ao.view(torch.int32)[:, 7].cpu().numpy().view(np.uint32), want["count"])
wp = np.zeros(pts.shape[0], dtype=spt.BAKE_WORLD_DTYPE)
wp["p"], wp["n"] = made["pos"], made["nrm"]
t_wp = torch.from_numpy(wp.view(np.float32).reshape(-1, 8).copy()).to(dev)
t_world = ds.ambient_occlusion(t_wp, samples=3, max_distance=0.9, seed=11, first_point=9, world=True)
assert _util.same_words(t_world.cpu().numpy().view(np.uint32), ref.words(want)), "resolved points given as WORLD tensors differ"

# invalid points behind device pointers: the NaN record, and the neighbours as they were
bad = pts.copy()
sphere = int(np.flatnonzero(inst["prim_type"] == 0)[0])
bad["instance"][5] = sphere
bad["instance"][64] = len(inst)
bad["prim"][200] = 0xffffffff
bad["v"][333] = np.nan
bad["w"][len(pts) - 1] = np.inf
at = np.array([5, 64, 200, 333, len(pts) - 1])
expect = ref.words(want).copy()
expect[at, :7] = 0x7fc00000
expect[at, 7] = 0xffffffff
for per_pass in (0, 256):
    t_bad = ds.ambient_occlusion(torch.from_numpy(bad.view(np.float32).reshape(-1, 4).copy()).to(dev), samples=3, max_distance=0.9, seed=11, first_point=9,
                                 points_per_pass=per_pass)
    assert np.array_equal(t_bad.cpu().numpy().view(np.uint32), expect), "invalid points"
bad_w = wp.copy()
bad_w["n"][7] = 0.0
bad_w["p"][70, 1] = np.nan
expect = ref.words(want).copy()
expect[[7, 70], :7] = 0x7fc00000
expect[[7, 70], 7] = 0xffffffff
t_bad = ds.ambient_occlusion(torch.from_numpy(bad_w.view(np.float32).reshape(-1, 8).copy()).to(dev), samples=3, max_distance=0.9, seed=11, first_point=9, world=True)
assert np.array_equal(t_bad.cpu().numpy().view(np.uint32), expect), "invalid world points"

# bad device pointers are refused and write nothing
job = spt.OccludedJob(size=ctypes.sizeof(spt.OccludedJob), flags=spt.OCCLUDED_DEVICE_POINTERS, n_rays=seg.shape[0])
out = np.full(seg.shape[0], 7, dtype=np.uint8)
job.rays, job.out = seg.ctypes.data, out.ctypes.data
assert lib.spt_occluded(ds._h, ctypes.byref(job)) == 1 and (out == 7).all()
job.rays, job.out = t_seg.data_ptr(), out.ctypes.data
assert lib.spt_occluded(ds._h, ctypes.byref(job)) == 1 and (out == 7).all()
t_occ.fill_(9)
job.rays, job.out = t_seg.data_ptr() + 4, t_occ.data_ptr()
assert lib.spt_occluded(ds._h, ctypes.byref(job)) == 1 and b"aligned" in lib.spt_last_error()
t_words = torch.full(((seg.shape[0] + 63) // 64 + 1,), 9, dtype=torch.int64, device=dev)
job.flags |= spt.OCCLUDED_PACKED
job.rays, job.out = t_seg.data_ptr(), t_words.data_ptr() + 4
assert lib.spt_occluded(ds._h, ctypes.byref(job)) == 1 and b"aligned" in lib.spt_last_error()
assert (t_occ == 9).all() and (t_words == 9).all()
job.flags = spt.OCCLUDED_DEVICE_POINTERS
job.out = t_occ.data_ptr() + 1          # bytes need no alignment
job.n_rays = seg.shape[0] - 1
torch.cuda.synchronize()
assert lib.spt_occluded(ds._h, ctypes.byref(job)) == 0
torch.cuda.synchronize()
assert np.array_equal(t_occ[1:].cpu().numpy(), host[:-1]) and int(t_occ[0]) == 9
aj = spt.AoJob(size=ctypes.sizeof(spt.AoJob), flags=spt.AO_DEVICE_POINTERS, n_points=pts.shape[0], samples=3, max_distance=0.9, seed=11, first_point=9)
rec = np.full((pts.shape[0], 8), np.float32(7.0))
aj.points, aj.out = pts.ctypes.data, rec.ctypes.data
assert lib.spt_ao(ds._h, ctypes.byref(aj)) == 1 and (rec == 7.0).all()
aj.points, aj.out = t_pts.data_ptr(), rec.ctypes.data
assert lib.spt_ao(ds._h, ctypes.byref(aj)) == 1 and (rec == 7.0).all()
t_ao.fill_(9.0)
aj.points, aj.out = t_pts.data_ptr() + 4, t_ao.data_ptr()
assert lib.spt_ao(ds._h, ctypes.byref(aj)) == 1
aj.points, aj.out = t_pts.data_ptr(), t_ao.data_ptr() + 8
assert lib.spt_ao(ds._h, ctypes.byref(aj)) == 1
assert (t_ao == 9.0).all()
assert _util.same_words(ds.ambient_occlusion(t_pts, samples=3, max_distance=0.9, seed=11, first_point=9).cpu().numpy().view(np.uint32), ref.words(want))
assert np.array_equal(ds.occluded(t_seg).cpu().numpy(), host)
sc.close()
print("visibility tensors ok")
"""


def test_device_pointers_in_a_process_that_imported_torch_first():
    res = subprocess.run([sys.executable, "-c", _CHILD, _util.ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "visibility tensors ok" in res.stdout, res.stdout + res.stderr


# ---- 6. isolation -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_films_and_async_frames_are_undisturbed(name):
    sc, ds = _scene(name), _ds(name)
    seg, occ_want = _segments(name)
    pts, ao_want = _points(name), _ao_want(name)
    cfg = spt.OutputConfig(W, H, None, CAMERAS[name])
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=8, seed=3)
    with r.progressive(sc, cfg) as plain:
        undisturbed = plain.render(4).render(4).mean().copy()
    sync = r.render_shard(sc, cfg).copy()
    calls = {"occluded": lambda what: _same_bytes(ds.occluded(seg), occ_want, what),
             "ambient_occlusion": lambda what: _check(ds.ambient_occlusion(pts, samples=S, seed=SEED), ao_want, what)}
    for call, check in calls.items():
        with r.progressive(sc, cfg) as film:
            film.render(4)
            check(call + " between two increments")
            assert _util.same_words(film.render(4).mean(), undisturbed)
        buf = r.render_shard(sc, cfg, reuse_output=True, wait=False)
        check(call + " behind an asynchronous frame")
        r.wait(sc)
        assert _util.same_words(np.array(buf), sync)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

def test_occluded_refusals_write_nothing_and_leave_the_scene_usable():
    name = "t_materials"
    seg, want = _segments(name)
    sc, ds = _scene(name), _ds(name)
    lib = spt.hip_lib()
    n = seg.shape[0]
    out = np.empty(n, dtype=np.uint8)

    def job(arr=seg, **kw):
        j = spt.OccludedJob(size=C.sizeof(spt.OccludedJob), n_rays=arr.shape[0])
        j.rays, j.out = arr.ctypes.data, out.ctypes.data
        j.keep = arr      # (the job's pointer does not own the array)
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(j, scene=ds._h, word=None, status=1):
        out[:] = PATTERN8
        assert lib.spt_occluded(scene, C.byref(j) if j is not None else None) == status
        assert (out == PATTERN8).all()
        if word is not None:
            assert word in lib.spt_last_error().decode(), lib.spt_last_error()

    def edited(at, field, value, axis=None):
        bad = seg.copy()
        if axis is None:
            bad[field][at] = value
        else:
            bad[field][at, axis] = value
        return bad

    refused(job(), scene=None)
    refused(None)
    refused(job(rays=None))
    refused(job(out=None))
    refused(job(flags=4), word="flags")
    refused(job(flags=0x80000000), word="flags")
    refused(job(size=C.sizeof(spt.OccludedJob) - 8), word="size")
    refused(job(n_rays=(1 << 40) + 1), status=4)
    refused(job(edited(5, "o", np.nan, 1)), word="ray 5 ")
    refused(job(edited(6, "d", np.inf, 2)), word="ray 6 ")
    refused(job(edited(7, "t_min", np.nan)), word="ray 7 ")
    refused(job(edited(8, "d", 0.0)), word="ray 8 ")
    refused(job(edited(9, "t_max", np.nan)), word="ray 9 ")
    refused(job(edited(n - 1, "t_max", np.nan)), word="ray %d " % (n - 1))
    refused(job(edited(1700, "t_max", np.nan), rays_per_pass=512), word="ray 1700 ")      # a later pass: still nothing written
    refused(job(edited(1700, "o", np.inf, 0), rays_per_pass=500, flags=spt.OCCLUDED_PACKED), word="ray 1700 ")
    refused(job(flags=spt.OCCLUDED_DEVICE_POINTERS), word="device")
    # t_max may be infinite or negative (nothing lies on such a segment): what trace_any says
    odd = edited(9, "t_max", np.inf)
    odd["t_max"][10] = -1.0
    _same_bytes(ds.occluded(odd), ds.trace_any(odd), "infinite and negative t_max")
    # nothing to do is not a refusal, and writes nothing either
    refused(job(n_rays=0), status=0)
    refused(job(n_rays=0, rays=None, out=None), status=0)
    # a good call after all of them, and a render
    _same_bytes(ds.occluded(seg), want, "after the refusals")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=2, seed=3)
    assert np.isfinite(r.render_shard(sc, spt.OutputConfig(W, H, None, CAMERAS[name]))).any()


def test_ao_refusals_write_nothing_and_leave_the_scene_usable():
    name = "t_materials"
    pts, want = _points(name), _ao_want(name)
    sc, ds = _scene(name), _ds(name)
    lib = spt.hip_lib()
    n = pts.shape[0]
    out = np.empty((n, 8), dtype=np.uint32)
    inst, meshes = sc.array("instances"), sc.array("meshes")
    sphere = int(np.flatnonzero(inst["prim_type"] == 0)[0])
    cube = int(np.flatnonzero((inst["prim_type"] == 1) & (inst["prim_id"] == 0))[0])

    def job(arr=pts, **kw):
        j = spt.AoJob(size=C.sizeof(spt.AoJob), n_points=arr.shape[0], samples=S, max_distance=np.inf, seed=SEED)
        j.points, j.out = arr.ctypes.data, out.ctypes.data
        j.keep = arr      # (the job's pointer does not own the array)
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(j, scene=ds._h, word=None, status=1):
        out[:] = PATTERN32
        assert lib.spt_ao(scene, C.byref(j) if j is not None else None) == status
        assert (out == PATTERN32).all()
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
    refused(job(out=None))
    refused(job(flags=4), word="flags")
    refused(job(flags=0x80000000), word="flags")
    refused(job(kind=2), word="kind")
    refused(job(samples=0), word="samples")
    refused(job(samples=(1 << 24) + 1), word="samples")
    refused(job(max_distance=0.0), word="max_distance")
    refused(job(max_distance=-1.0), word="max_distance")
    refused(job(max_distance=-np.inf), word="max_distance")
    refused(job(max_distance=np.nan), word="max_distance")
    refused(job(size=C.sizeof(spt.AoJob) - 8), word="size")
    refused(job(n_points=(1 << 40) + 1), status=4)
    refused(job(edited(5, instance=sphere)), word="point 5 ")
    refused(job(edited(n - 1, instance=cube, prim=meshes[1]["tri_first"])), word="point %d " % (n - 1))
    refused(job(edited(700, instance=cube, prim=meshes[1]["tri_first"]), points_per_pass=256), word="point 700 ")   # a later pass: still nothing written
    refused(job(edited(3, instance=len(inst))), word="point 3 ")
    refused(job(edited(0, v=np.nan)), word="point 0 ")
    wp = _world_points(name).copy()
    wp["n"][7] = 0.0
    refused(job(wp, kind=spt.BAKE_POINTS_WORLD, n_points=min(len(wp), n)), word="point 7 ")
    refused(job(flags=spt.AO_DEVICE_POINTERS), word="device")
    # nothing to do is not a refusal, and writes nothing either
    refused(job(n_points=0), status=0)
    refused(job(n_points=0, points=None, out=None), status=0)
    # a good call after all of them, and a render
    _check(ds.ambient_occlusion(pts, samples=S, seed=SEED), want, "after the refusals")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=2, seed=3)
    assert np.isfinite(r.render_shard(sc, spt.OutputConfig(W, H, None, CAMERAS[name]))).any()


# ---- 8. the CLI ---------------------------------------------------------------------------------------------------------------------

def test_the_cli_writes_the_maps_of_lightmap_points_and_ambient_occlusion(tmp_path):
    name = "t_textured"
    sc = _scene(name)
    cli = os.path.join(spt.LIB_DIR, "spt")
    ao, bent = tmp_path / "ao.exr", tmp_path / "bent.exr"
    dist = _near(name)
    base = [cli, "-s", os.path.join(_util.SCENES, name + ".json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(ao), "--bake-ao", "floor",
            "--bake-size", "16x16", "--ao-samples", "4", "--ao-distance", repr(dist), "--bent-out", str(bent), "--seed", "5"]
    res = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    pts, texels = sc.lightmap_points("floor", 16, 16)
    assert len(pts) == 256
    rec = _ds(name).ambient_occlusion(pts, samples=4, max_distance=dist, seed=5)
    want_open, want_bent = np.zeros((16 * 16, 3), dtype=f32), np.zeros((16 * 16, 3), dtype=f32)
    want_open[texels] = rec["open"][:, None]
    want_bent[texels] = rec["bent"]
    got = spt.read_exr(str(ao))
    assert got.shape == (16, 16, 3) and _util.same_words(np.ascontiguousarray(got, dtype=f32).reshape(-1, 3), want_open)
    got = spt.read_exr(str(bent))
    assert got.shape == (16, 16, 3) and _util.same_words(np.ascontiguousarray(got, dtype=f32).reshape(-1, 3), want_bent)
    assert 0 < rec["count"].sum() < 4 * 256
    # without --bent-out and --ao-distance: the openness alone, to the horizon
    ao.unlink()
    bent.unlink()
    res = subprocess.run(base[:11] + ["--ao-samples", "4", "--seed", "5"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not bent.exists(), res.stdout + res.stderr
    want_open[texels] = _ds(name).ambient_occlusion(pts, samples=4, seed=5)["open"][:, None]
    assert _util.same_words(np.ascontiguousarray(spt.read_exr(str(ao)), dtype=f32).reshape(-1, 3), want_open)

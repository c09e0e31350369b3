"""spt_hits (DeviceScene.all_hits, DeviceScene.enclosed): the K nearest crossings of caller segments and the crossing counts.

Every expected value comes from tests/_hits_ref.py, the float32 numpy restatement of the definition that tests/test_hits_abi.py
anchors to the CPU oracle and shows to be not trivial; where a call exists for the same answer it is asked too: record 0 is
trace_closest's hit, and total > 0 is trace_any's / occluded's byte on the scene without spheres.  Every comparison is of words; no
ray is left out.

Rays (tests/_hits_ref.batches): the 48 x 36 camera grid, _util.random_rays, segments through the whole bounds from outside aimed at
the instances, rays through shared triangle edges (equal t, ordered by prim); each of them also cut at t_max = extent / 16, moved to
a window of that length around the first surface, and with t_min moved past the first crossing."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _hits_ref as ref
import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32

W, H = 48, 36
PATTERN32 = np.uint32(0x7fc0beef)   # (a NaN no record holds)
CAMERAS = {"cfg2_cube": None, "t_materials": "main", "t_textured": None, "t_medium": None}
KS = (1, 2, 4, 7)


@functools.lru_cache(maxsize=None)
def _scene(name):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_util.SCENES, name + ".json"))


def _ds(name):
    return _scene(name).device_scene(0)


@functools.lru_cache(maxsize=None)
def _rays(name):
    """(rays, crossings): every batch of the scene in one array, and the reference's crossings of it; read-only."""
    rays = np.concatenate(list(ref.batches(spt, _scene(name), CAMERAS[name]).values()))
    rays.setflags(write=False)
    return rays, ref.crossings(_scene(name), rays)


@functools.lru_cache(maxsize=None)
def _want(name, K, count_all=False):
    rec, counts = ref.records(spt, _rays(name)[1], K, count_all)
    rec.setflags(write=False)
    counts.setflags(write=False)
    return rec, counts


def _check(got, want, what):
    (rec, counts), (wrec, wcounts) = got, want
    assert rec.dtype == spt.HIT_REC_DTYPE and rec.shape == wrec.shape and counts.dtype == spt.HIT_COUNT_DTYPE and counts.shape == wcounts.shape, what
    g, w = ref.words(rec), ref.words(wrec)
    bad = np.flatnonzero((g != w).any(axis=(1, 2))) if g.size else np.zeros(0, dtype=int)
    assert len(bad) == 0, "%s: the records of %d of %d rays differ from the reference, first ray %d:\n%s\n%s" % (
        what, len(bad), len(g), bad[0], rec[bad[0]], wrec[bad[0]])
    assert np.array_equal(counts, wcounts), "%s: %d of %d counts differ from the reference" % (what, int((counts != wcounts).sum()), len(wcounts))


def _hit_words(rec):
    """(t, instance, prim, v, w) of HIT_REC_DTYPE or HIT_DTYPE records as (n, 5) uint32."""
    out = np.zeros(rec.shape, dtype=spt.HIT_DTYPE)
    for f in ("t", "instance", "prim", "v", "w"):
        out[f] = rec[f]
    return out.view(np.uint32).reshape(-1, 5)


# ---- 1. the records and the counts -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CAMERAS))
def test_the_k_nearest_crossings_and_the_counts(name):
    ds = _ds(name)
    rays, _ = _rays(name)
    for K in KS:
        nearest = ds.all_hits(rays, max_hits=K)
        _check(nearest, _want(name, K), "%s, max_hits %d" % (name, K))
        every = ds.all_hits(rays, max_hits=K, count_all=True)
        _check(every, _want(name, K, True), "%s, max_hits %d, count_all" % (name, K))
        assert np.array_equal(ref.words(nearest[0]), ref.words(every[0])), "max_hits %d: the records of the two modes differ" % K
    rec, counts = ds.all_hits(rays, max_hits=0, count_all=True)
    assert rec.shape == (len(rays), 0)
    assert np.array_equal(counts, _want(name, 0, True)[1])
    # what the expected values hold: lists that are cut at K, lists that end before it, and both facings
    full = _want(name, 7, True)[1]["total"]
    assert (full > 2).any() and (name == "cfg2_cube" or (full > 7).any()) and ((full > 0) & (full < 4)).any() and (_want(name, 4)[1]["back"] > 0).any()


@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_ragged_counts_and_passes(name):
    ds = _ds(name)
    rays, _ = _rays(name)
    rec, counts = _want(name, 4)
    all_counts = _want(name, 4, True)[1]
    for n in (1, 63, 64, 65, 257):
        _check(ds.all_hits(rays[:n], max_hits=4), (rec[:n], counts[:n]), "%d rays" % n)
        _check(ds.all_hits(rays[-n:], max_hits=4, count_all=True), (rec[-n:], all_counts[-n:]), "the last %d rays" % n)
    for per_pass in (1000, 700):
        _check(ds.all_hits(rays, max_hits=4, rays_per_pass=per_pass), (rec, counts), "passes of %d" % per_pass)
        _check(ds.all_hits(rays, max_hits=4, count_all=True, rays_per_pass=per_pass), (rec, all_counts), "passes of %d, count_all" % per_pass)
    got = ds.all_hits(rays[:0], max_hits=4)
    assert got[0].shape == (0, 4) and got[1].shape == (0,)
    # the largest list: 64 records per ray
    _check(ds.all_hits(rays[:300], max_hits=64), tuple(a[:300] for a in _want(name, 64)), "max_hits 64")


# ---- 2. the calls that answer the same question ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CAMERAS))
def test_record_0_is_trace_closest(name):
    ds = _ds(name)
    rays, _ = _rays(name)
    rec, counts = ds.all_hits(rays, max_hits=1)
    hits = ds.trace_closest(rays)
    assert (hits["instance"] >= 0).mean() > 0.3
    assert np.array_equal(_hit_words(rec[:, 0]), _hit_words(hits)), "%d rays differ" % int((_hit_words(rec[:, 0]) != _hit_words(hits)).any(axis=1).sum())
    assert np.array_equal(counts["total"], (hits["instance"] >= 0).astype(np.uint32))


def test_total_is_occluded_on_the_scene_without_spheres():
    name = "cfg2_cube"
    ds = _ds(name)
    rays, _ = _rays(name)
    _, counts = ds.all_hits(rays, max_hits=0, count_all=True)
    occ = ds.occluded(rays)
    assert 0.2 < occ.mean() < 0.8
    assert np.array_equal((counts["total"] > 0).astype(np.uint8), occ) and np.array_equal(occ, ds.trace_any(rays))
    _, counts = ds.all_hits(rays, max_hits=3, count_all=True)
    assert np.array_equal((counts["total"] > 0).astype(np.uint8), occ)


def test_a_segment_inside_a_sphere_crosses_nothing_though_it_is_occluded():
    name = "t_materials"
    sc, ds = _scene(name), _ds(name)
    inst, sph = sc.array("instances"), sc.array("spheres")
    i = int(np.flatnonzero(inst["prim_type"] == ref.PRIM_SPHERE)[0])
    centre = (inst["bmin"][i] + inst["bmax"][i]) / 2
    radius = float((inst["bmax"][i] - inst["bmin"][i]).min() / 2)
    assert len(sph) > 0 and radius > 0
    rays = np.zeros(1, dtype=spt.RAY_DTYPE)
    rays["o"], rays["d"], rays["t_min"], rays["t_max"] = centre, (0, 1, 0), 0.0, radius * 0.5
    rec, counts = ds.all_hits(rays, max_hits=2, count_all=True)
    assert counts["total"][0] == 0 and rec["instance"][0].tolist() == [-1, -1] and ds.trace_any(rays)[0] == 1
    _check((rec, counts), ref.records(spt, ref.crossings(sc, rays), 2, True), "inside a sphere")


# ---- 3. the walkers of scenes that do not fit LDS --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CAMERAS))
def test_four_wide_nodes_from_memory(monkeypatch, name):
    rays, _ = _rays(name)
    monkeypatch.setenv("SPT_NO_LDS_GEO", "1")      # (read when the device scene is made)
    sc = spt.load_scene(os.path.join(_util.SCENES, name + ".json"))
    try:
        ds = sc.device_scene(0)
        for K in (1, 4, 7):
            _check(ds.all_hits(rays, max_hits=K), _want(name, K), "%s from memory, max_hits %d" % (name, K))
        _check(ds.all_hits(rays, max_hits=4, count_all=True, rays_per_pass=700), _want(name, 4, True), "%s from memory, count_all" % name)
        assert np.array_equal(ds.all_hits(rays, max_hits=0, count_all=True)[1], _want(name, 0, True)[1])
    finally:
        sc.close()


# ---- 4. moving scenes ------------------------------------------------------------------------------------------------------------------

def test_the_call_follows_moved_instances_and_deformed_meshes():
    name = "t_materials"
    path = os.path.join(_util.SCENES, name + ".json")
    rays, _ = _rays(name)
    sc = spt.load_scene(path)
    fresh = []
    try:
        ds = sc.device_scene(0)
        c, s = np.cos(0.7), np.sin(0.7)
        xf = {"red_cube": np.array([[c, 0, s, 1.5], [0, 1.2, 0, 0.9], [-s, 0, c, -0.5]], dtype=f32)}
        rest = sc.mesh_positions("cube")
        bent = rest.copy()
        bent[:, 1] += f32(0.25) * np.sin(f32(2.0) * rest[:, 0])
        last = ds.all_hits(rays, max_hits=4, count_all=True)
        _check(last, _want(name, 4, True), "before the edits")
        sc.set_transforms(xf)
        ds.update()
        for step in ("set_transforms", "set_mesh_vertices"):
            if step == "set_mesh_vertices":
                sc.set_mesh_vertices("cube", bent)
                ds.update()
            f = spt.load_scene(path)
            fresh.append(f)
            f.set_transforms(xf)
            if step == "set_mesh_vertices":
                f.set_mesh_positions("cube", bent)
            got = ds.all_hits(rays, max_hits=4, count_all=True)
            _check(got, f.device_scene(0).all_hits(rays, max_hits=4, count_all=True), "after %s + update: a fresh scene's records" % step)
            if step == "set_transforms":      # (the reference reads the descriptor's triangles, which the loader derives for a fresh scene)
                _check(got, ref.records(spt, ref.crossings(f, rays), 4, True), "after %s + update: the reference on a fresh scene" % step)
            assert not np.array_equal(ref.words(got[0]), ref.words(last[0]))
            last = got
    finally:
        for f in fresh:
            f.close()
        sc.close()


# ---- 5. isolation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_films_and_async_frames_are_undisturbed(name):
    sc, ds = _scene(name), _ds(name)
    rays, _ = _rays(name)
    cfg = spt.OutputConfig(W, H, None, CAMERAS[name])
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=8, seed=3)
    with r.progressive(sc, cfg) as plain:
        undisturbed = plain.render(4).render(4).mean().copy()
    sync = r.render_shard(sc, cfg).copy()
    with r.progressive(sc, cfg) as film:
        film.render(4)
        _check(ds.all_hits(rays, max_hits=4, count_all=True), _want(name, 4, True), "between two increments")
        assert _util.same_words(film.render(4).mean(), undisturbed)
    buf = r.render_shard(sc, cfg, reuse_output=True, wait=False)
    _check(ds.all_hits(rays, max_hits=4), _want(name, 4), "behind an asynchronous frame")
    r.wait(sc)
    assert _util.same_words(np.array(buf), sync)


# ---- 6. device pointers ----------------------------------------------------------------------------------------------------------------

_CHILD = r"""
import ctypes, os, sys
import torch                                  # before the package: the tensor path must work in a process torch initialised
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import _util
import _hits_ref as ref
spt = _util.load_pkg()
sc = spt.load_scene(os.path.join(_util.SCENES, "t_materials.json"))
ds = sc.device_scene(0)
dev = torch.device("cuda", 0)
lib = spt.hip_lib()
rays = np.concatenate(list(ref.batches(spt, sc, "main", variants=False).values()))
cr = ref.crossings(sc, rays)
n = rays.shape[0]
t_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to(dev)
for K, every in ((4, False), (4, True), (1, False), (0, True)):
    wrec, wcounts = ref.records(spt, cr, K, every)
    t_rec, t_counts = ds.all_hits(t_rays, max_hits=K, count_all=every)
    assert t_rec.device == dev and t_rec.dtype == torch.float32 and t_rec.shape == (n, K, 8)
    assert t_counts.device == dev and t_counts.dtype == torch.int32 and t_counts.shape == (n, 2)
    assert np.array_equal(t_rec.cpu().numpy().view(np.uint32), ref.words(wrec)), "tensor records, max_hits %d" % K
    assert np.array_equal(t_counts.cpu().numpy().view(np.uint32), wcounts.view(np.uint32).reshape(-1, 2)), "tensor counts, max_hits %d" % K
    hrec, hcounts = ds.all_hits(rays, max_hits=K, count_all=every)
    assert np.array_equal(ref.words(hrec), ref.words(wrec)) and np.array_equal(hcounts, wcounts)
wrec, wcounts = ref.records(spt, cr, 3)
for m in (1, 63, 64, 65, 257):
    t_rec, t_counts = ds.all_hits(t_rays[:m].contiguous(), max_hits=3, rays_per_pass=100)
    assert np.array_equal(t_rec.cpu().numpy().view(np.uint32), ref.words(wrec[:m])), "%d rays" % m
    assert np.array_equal(t_counts.cpu().numpy().view(np.uint32), wcounts[:m].view(np.uint32).reshape(-1, 2))
assert (wcounts["total"] == 3).mean() > 0.2 and (wcounts["back"] > 0).mean() > 0.2

# bad device pointers are refused and write nothing
t_rec = torch.full((n, 3, 8), 9.0, dtype=torch.float32, device=dev)
t_counts = torch.full((n + 1, 2), 9, dtype=torch.int32, device=dev)
host_rec = np.full((n, 3, 8), np.float32(7.0))
host_counts = np.full((n, 2), 7, dtype=np.uint32)
def job(rays_p, hits_p, counts_p, K=3):
    j = spt.HitsJob(size=ctypes.sizeof(spt.HitsJob), flags=spt.HITS_DEVICE_POINTERS, n_rays=n, max_hits=K)
    j.rays, j.hits, j.counts = rays_p, hits_p, counts_p
    return j
for j, word in ((job(rays.ctypes.data, t_rec.data_ptr(), t_counts.data_ptr()), b"rays"),
                (job(t_rays.data_ptr(), host_rec.ctypes.data, t_counts.data_ptr()), b"hits"),
                (job(t_rays.data_ptr(), t_rec.data_ptr(), host_counts.ctypes.data), b"counts"),
                (job(t_rays.data_ptr() + 4, t_rec.data_ptr(), t_counts.data_ptr()), b"aligned"),
                (job(t_rays.data_ptr(), t_rec.data_ptr() + 8, t_counts.data_ptr()), b"aligned"),
                (job(t_rays.data_ptr(), t_rec.data_ptr(), t_counts.data_ptr() + 4), b"aligned")):
    assert lib.spt_hits(ds._h, ctypes.byref(j)) == 1 and word in lib.spt_last_error(), lib.spt_last_error()
torch.cuda.synchronize()
assert (t_rec == 9.0).all() and (t_counts == 9).all() and (host_rec == 7.0).all() and (host_counts == 7).all()
# counts need 8 bytes only; max_hits == 0 reads no `hits`
j = job(t_rays.data_ptr(), None, t_counts.data_ptr() + 8, K=0)
j.flags |= spt.HITS_COUNT_ALL
assert lib.spt_hits(ds._h, ctypes.byref(j)) == 0
torch.cuda.synchronize()
assert np.array_equal(t_counts[1:].cpu().numpy().view(np.uint32), ref.records(spt, cr, 0, True)[1].view(np.uint32).reshape(-1, 2)) and (t_counts[0] == 9).all()
sc.close()
print("hits tensors ok")
"""


def test_device_pointers_in_a_process_that_imported_torch_first():
    res = subprocess.run([sys.executable, "-c", _CHILD, _util.ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "hits tensors ok" in res.stdout, res.stdout + res.stderr


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_leave_the_scene_usable():
    name = "t_materials"
    rays, _ = _rays(name)
    rays = rays[:2000]
    sc, ds = _scene(name), _ds(name)
    lib = spt.hip_lib()
    n, K = rays.shape[0], 3
    hits = np.empty((n, K, 8), dtype=np.uint32)
    counts = np.empty((n, 2), dtype=np.uint32)

    def job(arr=rays, **kw):
        j = spt.HitsJob(size=C.sizeof(spt.HitsJob), n_rays=arr.shape[0], max_hits=K)
        j.rays, j.hits, j.counts = arr.ctypes.data, hits.ctypes.data, counts.ctypes.data
        j.keep = arr      # (the job's pointer does not own the array)
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(j, scene=ds._h, word=None, status=1):
        hits[:] = PATTERN32
        counts[:] = PATTERN32
        assert lib.spt_hits(scene, C.byref(j) if j is not None else None) == status
        assert (hits == PATTERN32).all() and (counts == PATTERN32).all()
        if word is not None:
            assert word in lib.spt_last_error().decode(), lib.spt_last_error()

    def edited(at, field, value, axis=None):
        bad = rays.copy()
        if axis is None:
            bad[field][at] = value
        else:
            bad[field][at, axis] = value
        return bad

    refused(job(), scene=None)
    refused(None)
    refused(job(rays=None))
    refused(job(counts=None))
    refused(job(hits=None), word="hits")
    refused(job(flags=4), word="flags")
    refused(job(flags=0x80000000), word="flags")
    refused(job(size=C.sizeof(spt.HitsJob) - 8), word="size")
    refused(job(max_hits=65), word="max_hits")
    refused(job(max_hits=0), word="max_hits")
    refused(job(max_hits=0xffffffff, flags=spt.HITS_COUNT_ALL), word="max_hits")
    refused(job(n_rays=(1 << 40) + 1), status=4)
    refused(job(edited(5, "o", np.nan, 1)), word="ray 5 ")
    refused(job(edited(6, "d", np.inf, 2)), word="ray 6 ")
    refused(job(edited(7, "t_min", np.nan)), word="ray 7 ")
    refused(job(edited(8, "d", 0.0)), word="ray 8 ")
    refused(job(edited(9, "t_max", np.nan)), word="ray 9 ")
    refused(job(edited(n - 1, "t_max", np.nan)), word="ray %d " % (n - 1))
    refused(job(edited(1700, "t_max", np.nan), rays_per_pass=512), word="ray 1700 ")      # a later pass: still nothing written
    refused(job(edited(1700, "o", np.inf, 0), rays_per_pass=500, flags=spt.HITS_COUNT_ALL), word="ray 1700 ")
    refused(job(flags=spt.HITS_DEVICE_POINTERS), word="device")
    # a scene with Bezier patches: unsupported, and the message says why
    bez = _scene("t_bezier")
    refused(job(), scene=bez.device_scene(0)._h, status=4, word="one root")
    assert "Bezier" in lib.spt_last_error().decode()
    with pytest.raises(spt.SptError, match="Bezier"):
        bez.device_scene(0).all_hits(rays, max_hits=2)
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=2, seed=3)
    assert np.isfinite(r.render_shard(bez, spt.OutputConfig(W, H, None, "main"))).any()
    # t_max may be infinite or negative (nothing lies on such a segment)
    odd = edited(9, "t_max", np.inf)
    odd["t_max"][10] = -1.0
    got = ds.all_hits(odd, max_hits=K, count_all=True)
    _check(got, ref.records(spt, ref.crossings(sc, odd), K, True), "infinite and negative t_max")
    assert got[1]["total"][10] == 0
    # nothing to do is not a refusal, and writes nothing either
    refused(job(n_rays=0), status=0)
    refused(job(n_rays=0, rays=None, hits=None, counts=None), status=0)
    # a good call after all of them, and a render
    _check(ds.all_hits(rays, max_hits=K), tuple(a[:n] for a in _want(name, K)), "after the refusals")
    assert np.isfinite(r.render_shard(sc, spt.OutputConfig(W, H, None, CAMERAS[name]))).any()


# ---- 8. enclosed -----------------------------------------------------------------------------------------------------------------------

def _enclosed_points(sc):
    """(inside, outside): the centre of every mesh instance's and every sphere's box, and points above, beside and below the scene."""
    inst = sc.array("instances")
    lo, hi = ref.scene_box(sc)
    size = inst["bmax"] - inst["bmin"]
    solid = size.min(axis=1) > 0.05 * size.max(axis=1)      # (a floor is a sheet, not a body)
    inside = ((inst["bmin"] + inst["bmax"]) / 2)[solid]
    outside = np.array([hi + 1.0, lo - 1.0, [(lo[0] + hi[0]) / 2, hi[1] + 0.5, (lo[2] + hi[2]) / 2], [hi[0] + 0.5, (lo[1] + hi[1]) / 2, hi[2] + 0.25]])
    return inside.astype(f32), outside.astype(f32)


def test_enclosed_counts_the_crossings_that_leave():
    sc, ds = _scene("cfg2_cube"), _ds("cfg2_cube")
    assert ds.enclosed(np.zeros((1, 3), dtype=f32)).tolist() == [True]      # the cube's centre
    inside, outside = _enclosed_points(sc)
    assert ds.enclosed(inside).all() and not ds.enclosed(outside).any()
    for d in ((0, 0, 1), (0, -1, 0), (0.3, 0.5, -0.8)):
        assert ds.enclosed(inside, direction=d).all() and not ds.enclosed(outside, direction=d).any()
    # inside a sphere of t_materials, and outside everything
    sm, dm = _scene("t_materials"), _ds("t_materials")
    inst = sm.array("instances")
    spheres = np.flatnonzero(inst["prim_type"] == ref.PRIM_SPHERE)
    centres = ((inst["bmin"] + inst["bmax"]) / 2)[spheres].astype(f32)
    up = (0.0, 1.0, 0.0)      # (upwards: away from the floor)
    assert dm.enclosed(centres, direction=up).all()
    _, outside = _enclosed_points(sm)
    assert not dm.enclosed(outside[:1], direction=up).any()
    above =centres + np.array([0, 1, 0], dtype=f32) * (inst["bmax"][spheres, 1] - inst["bmin"][spheres, 1])[:, None]
    assert not dm.enclosed(above, direction=up).any()


def test_enclosed_follows_a_moved_cube():
    path = os.path.join(_util.SCENES, "cfg2_cube.json")
    sc = spt.load_scene(path)
    try:
        ds = sc.device_scene(0)
        centre = np.zeros((1, 3), dtype=f32)
        moved = np.array([[3.0, 0.5, -2.0]], dtype=f32)
        assert ds.enclosed(centre).tolist() == [True] and ds.enclosed(moved).tolist() == [False]
        fwd = sc.array("instances")["fwd"][0].copy()      # the columns of the 3 x 3, then the translation
        fwd[9:12] += moved[0]
        sc.set_transforms({"cube": fwd})
        ds.update()
        assert ds.enclosed(centre).tolist() == [False] and ds.enclosed(moved).tolist() == [True]
    finally:
        sc.close()

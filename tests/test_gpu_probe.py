"""spt_probe (DeviceScene.probes): spherical-harmonic light probes, the gather rays made and projected on the device.

The reference of every comparison is computed from calls that exist without spt_probe, over tests/_probe_ref.py's restatement of the
specification:  want = D_ref + (in-order sum over k of ds.radiance(rays_ref[:, k]) * Y_ref[:, k]) * w, with D_ref summed from
_probe_ref's li * Y(dir), gated by ds.trace_any on _probe_ref's shadow rays; the visibility record from the hits of ds.radiance(...,
hits=True) and _bake_ref.resolve.  Every comparison is _util.same_words; no probe is left out.
That reference is the device's own integrator: it shows that spt_probe is those calls, not that those calls are right for rays that
start at a free point.  The tie to the oracle is test_probes_are_the_oracles_delta_sum_plus_the_oracles_projected_radiance (the same
formulas over oracle_radiance, oracle_trace_closest and oracle_trace_any) and, for spt_radiance itself,
tests/test_gpu_radiance_anywhere.py.

Probes: about 300 on a jittered grid over the scene's bounds grown by 10 %; 8 samples, max_depth 5."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _bake_ref
import _probe_ref
import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32

S, DEPTH, SEED = 8, 5, 11
W, H = 48, 36
F32_MAX = np.finfo(f32).max
PATTERN = np.uint32(0x7fc0beef)   # (a NaN no probe produces)
CAMERAS = {"cfg2_cube": None, "t_materials": "main", "t_medium": None, "t_textured": None, "t_bezier": "main"}


@functools.lru_cache(maxsize=None)
def _scene(name):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_util.SCENES, name + ".json"))


def _ds(name):
    return _scene(name).device_scene(0)


def _grid(scene, seed=5):
    """A jittered 7 x 6 x 7 grid (294 probes) over the bounds of the scene's instances grown by 10 %, (n, 3) f32."""
    inst = scene.array("instances")
    lo, hi = np.clip(inst["bmin"].min(axis=0), -20, 20).astype(np.float64), np.clip(inst["bmax"].max(axis=0), -20, 20).astype(np.float64)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.5) * 1.1
    n = (7, 6, 7)
    cells = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), axis=-1).reshape(-1, 3)
    jitter = np.random.default_rng(seed).random(cells.shape)
    p = (mid - half) + (cells + jitter) / np.array(n) * (2 * half)
    return p.astype(f32)


@functools.lru_cache(maxsize=None)
def _points(name):
    p = _grid(_scene(name))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(points, ref inputs, want, D, gather sum, aux) from calls that exist without spt_probe; read-only."""
    scene, ds = _scene(name), _ds(name)
    p = _points(name)
    ref = _probe_ref.probe_inputs(spt, scene.array("lights"), p, S, SEED)
    want, D, acc, aux = _probe_ref.probes_from_existing_calls(ds, ref, DEPTH, SEED, tab=_bake_ref.tables(scene))
    for a in (want, D, acc, aux):
        a.setflags(write=False)
    return p, ref, want, D, acc, aux


def _check(got, want, what):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    assert _util.same_words(got, want), "%s: %d of %d words differ from the reference built from radiance and trace_any" % (what, int(bad.sum()), bad.size)


# ---- 1. parity --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials", "t_textured", "t_medium", "t_bezier"])
def test_probes_are_the_delta_sum_plus_the_projected_radiance(name):
    p, ref, want, D, acc, aux = _reference(name)
    assert len(p) == 294
    sh, vis = _ds(name).probes(p, samples=S, max_depth=DEPTH, seed=SEED, aux=True)
    _check(sh, want, name)
    _check(vis, aux, name + ", visibility record")
    _check(_ds(name).probes(p, samples=S, max_depth=DEPTH, seed=SEED), want, name + ", without the record")
    assert np.any(aux[:, 0] > 0) and np.any(aux[:, 0] < 1)
    if name == "cfg2_cube":       # fused, flat LDS: probes inside the cube see only back faces, the light reaches the others
        assert np.any(aux[:, 1] == 1) and np.any(D != 0)
    if name == "t_materials":     # class queues, environment, three delta lights
        assert np.any(acc != 0) and np.any(D != 0)
        assert np.mean(np.any(acc.reshape(len(p), -1) != 0, axis=-1)) > 0.5
    if name in ("t_medium", "t_textured", "t_bezier"):
        assert np.any(acc != 0)


@pytest.mark.parametrize("name", ["t_materials", "t_medium", "t_textured"])
def test_probes_are_the_oracles_delta_sum_plus_the_oracles_projected_radiance(name):
    """The same restated rays, but no device call on the expected side: _util.OracleScene stands in for the DeviceScene, so D is gated
    by oracle_trace_any, the projected term is oracle_radiance's (trace_ray from free points, which no camera ray reaches) and the
    visibility record comes from oracle_trace_closest's hits."""
    p, ref, _, _, _, _ = _reference(name)
    want, D, acc, aux = _probe_ref.probes_from_existing_calls(_util.OracleScene(_scene(name)), ref, DEPTH, SEED, tab=_bake_ref.tables(_scene(name)))
    lit = np.any(acc.reshape(len(p), -1) != 0, axis=-1)
    assert np.isfinite(acc).all() and lit.mean() >= (0.05 if name == "t_medium" else 0.25) and len(np.unique(acc[lit].reshape(-1, 27), axis=0)) >= 100
    assert np.any(aux[:, 0] > 0) and np.any(aux[:, 0] < 1) and np.any(aux[:, 1] > 0)
    if name != "t_medium":        # (t_medium has no delta light)
        assert np.any(D != 0)
    sh, vis = _ds(name).probes(p, samples=S, max_depth=DEPTH, seed=SEED, aux=True)
    for got, exp, what in ((sh, want, "coefficients"), (vis, aux, "visibility record")):
        bad = ~((got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp)))
        assert _util.same_words(got, exp), "%s, %s: %d of %d words differ from the reference built from the oracle" % (name, what, int(bad.sum()), bad.size)


# the walkers of scenes that do not fit LDS: the streaming intake kernel, and the walker over the geometry in memory
@pytest.mark.parametrize("switches", [{"SPT_NO_LDS_GEO": "1"}, {"SPT_NO_LDS_GEO": "1", "SPT_NO_STREAM": "1"}], ids=["stream", "memory"])
def test_large_scene_walkers(monkeypatch, switches):
    name = "t_materials"
    p, ref, want, D, acc, aux = _reference(name)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)      # (read when the device scene is made)
    sc = spt.load_scene(os.path.join(_util.SCENES, name + ".json"))
    try:
        sh, vis = sc.device_scene(0).probes(p, samples=S, max_depth=DEPTH, seed=SEED, aux=True)
    finally:
        sc.close()
    _check(sh, want, name)
    _check(vis, aux, name + ", visibility record")


# ---- 2. delta lights, max_depth 0 -----------------------------------------------------------------------------------------------------

def test_max_depth_zero_is_the_delta_sum():
    """t_materials has a directional, a point and a spot light: max_depth 0 gives exactly D, and the visibility record is unchanged."""
    name = "t_materials"
    p, ref, want, D, acc, aux = _reference(name)
    types = _scene(name).array("lights")["type"]
    assert set(types.tolist()) >= {0, 1, 2}
    for kind in (0, 1, 2):
        assert np.any(ref["delta_li"][:, types == kind] != 0)
    assert np.any(D != 0) and not _util.same_words(D, want)
    _check(_ds(name).probes(p, samples=S, max_depth=0, seed=SEED), D, name)
    sh, vis = _ds(name).probes(p, samples=S, max_depth=0, seed=SEED, aux=True)
    _check(sh, D, name + ", with the record")
    _check(vis, aux, name + ", visibility record at max_depth 0")


# ---- 3. ragged sizes, passes, chunks ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_ragged_sizes_and_passes(name):
    p, ref, want, D, acc, aux = _reference(name)
    ds = _ds(name)
    first = 20
    for n in (1, 63, 65, 257):
        sh, vis = ds.probes(p[first:first + n], samples=S, max_depth=DEPTH, seed=SEED, first_point=first, aux=True)
        _check(sh, want[first:first + n], "%d probes inside the list" % n)
        _check(vis, aux[first:first + n], "%d probes inside the list, visibility record" % n)
    for per_pass in (64, 100):
        sh, vis = ds.probes(p, samples=S, max_depth=DEPTH, seed=SEED, points_per_pass=per_pass, aux=True)
        _check(sh, want, "points_per_pass %d" % per_pass)
        _check(vis, aux, "points_per_pass %d, visibility record" % per_pass)
    # without first_point the same records are other probes of the stream
    if name == "t_materials":
        assert not _util.same_words(ds.probes(p[first:first + 65], samples=S, max_depth=DEPTH, seed=SEED), want[first:first + 65])


@pytest.mark.parametrize("samples", [1, 5])
def test_sample_counts(samples):
    name = "t_materials"
    p = _points(name)[:100]
    ds = _ds(name)
    ref = _probe_ref.probe_inputs(spt, _scene(name).array("lights"), p, samples, SEED)
    want, D, acc, aux = _probe_ref.probes_from_existing_calls(ds, ref, DEPTH, SEED, tab=_bake_ref.tables(_scene(name)))
    sh, vis = ds.probes(p, samples=samples, max_depth=DEPTH, seed=SEED, aux=True)
    _check(sh, want, "%d samples" % samples)
    _check(vis, aux, "%d samples, visibility record" % samples)


@pytest.mark.parametrize("name,count,depth", [("cfg2_cube", 40, DEPTH), ("t_materials", 16, 2)])
def test_samples_across_a_chunk_boundary(name, count, depth):
    """513 samples: the pass loop cuts min(S, 2 * 2^22 / (probes rounded up to 64 * 256)) = 512 samples per chunk, so the last one
    arrives in a chunk of its own: the sums continue from sh_out, the counts of the record from their integer planes."""
    p = _points(name)[100:100 + count]
    ds = _ds(name)
    ref = _probe_ref.probe_inputs(spt, _scene(name).array("lights"), p, 513, SEED, first_point=100)
    want, D, acc, aux = _probe_ref.probes_from_existing_calls(ds, ref, depth, SEED, tab=_bake_ref.tables(_scene(name)))
    sh, vis = ds.probes(p, samples=513, max_depth=depth, seed=SEED, first_point=100, aux=True)
    _check(sh, want, name)
    _check(vis, aux, name + ", visibility record")
    assert np.any(acc != 0) or name == "cfg2_cube"
    assert np.any((aux[:, 0] > 0) & (aux[:, 0] < 1))


def test_first_sample_continues_the_streams():
    """Two calls of 4 samples each, first_sample 0 and 4.  Each is D + (the in-order sum of its own four terms) * w4.  A caller who
    carries the sum gets the 8-sample words: the second call's terms are added in k order onto the first call's sum."""
    name = "t_materials"
    p, ref, want, D, acc, aux = _reference(name)
    ds = _ds(name)
    halves = []
    for fs in (0, 4):
        part = dict(ref)
        part["rays"] = np.ascontiguousarray(ref["rays"][:, fs:fs + 4])
        part["weights"] = np.ascontiguousarray(ref["weights"][:, fs:fs + 4])
        half_want, _, half_acc, _ = _probe_ref.probes_from_existing_calls(ds, part, DEPTH, SEED)
        got = ds.probes(p, samples=4, max_depth=DEPTH, seed=SEED, first_sample=fs)
        _check(got, half_want, "first_sample %d" % fs)
        halves.append(got)
    assert not _util.same_words(halves[0], halves[1])
    # the carried sum: the terms of the second call, one by one, onto the first call's sum
    carried, mag = np.zeros_like(acc), np.zeros(acc.shape, dtype=np.float64)
    for k in range(8):
        x = ds.radiance(np.ascontiguousarray(ref["rays"][:, k]), repeats=1, max_depth=DEPTH, seed=SEED, rng_skip=0)
        term = x[:, None, :] * ref["weights"][:, k][:, :, None]
        carried = carried + term
        mag += np.abs(term)
    _check(D + carried * _probe_ref.weight(8), want, "the carried sum")
    # the two calls average to the 8-sample result up to the association of the sums: under 8 roundings of partial sums bounded by
    # the sum of the terms' magnitudes, two of the weight and three of the addition of D on each side
    mean = (halves[0].astype(np.float64) + halves[1]) / 2
    tol = 16 * np.finfo(f32).eps * (mag * float(_probe_ref.weight(8)) + np.abs(D))
    assert np.all(np.abs(mean - want) <= tol + 1e-30)


def test_first_point_wraps():
    name = "t_materials"
    p = _points(name)[:40]
    ds = _ds(name)
    ref = _probe_ref.probe_inputs(spt, _scene(name).array("lights"), p, S, SEED, first_point=0xFFFFFFF0, first_sample=3)
    want, _, _, aux = _probe_ref.probes_from_existing_calls(ds, ref, DEPTH, SEED, tab=_bake_ref.tables(_scene(name)))
    sh, vis = ds.probes(p, samples=S, max_depth=DEPTH, seed=SEED, first_point=0xFFFFFFF0, first_sample=3, aux=True)
    _check(sh, want, "first_point wrap")
    _check(vis, aux, "first_point wrap, visibility record")


# ---- 4. pins that need no reference ---------------------------------------------------------------------------------------------------

def test_a_probe_inside_the_closed_cube_sees_only_back_faces():
    sh, vis = _ds("cfg2_cube").probes(np.zeros((1, 3), dtype=f32), samples=64, max_depth=DEPTH, seed=SEED, aux=True)
    assert vis[0, 0] == 1.0 and vis[0, 1] == 1.0
    assert 0.9 < vis[0, 3] <= vis[0, 2] < 1.8          # the cube's faces (half edge 1) are between 1 and sqrt(3) away
    assert not sh.any()                                 # no light gets in: the directional light is occluded too


def test_a_probe_in_the_void_of_an_unlit_scene_is_black():
    """t_medium has no delta light and no environment; its one emitter is a quad, which a probe this far away does not see."""
    scene = _scene("t_medium")
    assert not np.any(scene.array("lights")["type"] <= 2)
    far = np.array([[0.0, -1.0e4, 0.0]], dtype=f32)    # below the floor: the scene subtends under 1e-7 of the sphere
    sh, vis = _ds("t_medium").probes(far, samples=64, max_depth=DEPTH, seed=SEED, aux=True)
    assert not sh.any()
    assert vis[0, 0] == 0.0 and vis[0, 1] == 0.0 and vis[0, 2] == 0.0 and vis[0, 3] == F32_MAX


def test_sh_irradiance_of_a_probe_above_the_scene_is_positive_upwards():
    """Far above t_materials the environment and the directional light fill the upper hemisphere: the irradiance sh_irradiance
    reconstructs on a plane facing up is finite and positive in every channel."""
    sh = _ds("t_materials").probes(np.array([[0.0, 50.0, 0.0]], dtype=f32), samples=256, max_depth=DEPTH, seed=SEED)
    E = spt.sh_irradiance(sh[0], np.array([0.0, 1.0, 0.0]))
    assert np.all(np.isfinite(E)) and np.all(E > 0)


# ---- 5. moving scenes ---------------------------------------------------------------------------------------------------------------

def test_probes_follow_moved_instances():
    name = "t_materials"
    path = os.path.join(_util.SCENES, name + ".json")
    p, ref, want, D, acc, aux = _reference(name)
    c, s = np.cos(0.7), np.sin(0.7)
    xf = {"red_cube": np.array([[c, 0, s, 1.5], [0, 1.2, 0, 0.9], [-s, 0, c, -0.5]], dtype=f32)}
    sc = spt.load_scene(path)
    try:
        ds = sc.device_scene(0)
        _check(ds.probes(p, samples=S, max_depth=DEPTH, seed=SEED), want, "before the move")
        sc.set_transforms(xf)
        ds.update()
        moved, moved_vis = ds.probes(p, samples=S, max_depth=DEPTH, seed=SEED, aux=True)
        assert not _util.same_words(moved, want)
        mref = _probe_ref.probe_inputs(spt, sc.array("lights"), p, S, SEED)
        mwant, _, _, maux = _probe_ref.probes_from_existing_calls(ds, mref, DEPTH, SEED, tab=_bake_ref.tables(sc))
        _check(moved, mwant, "after set_transforms + update")
        _check(moved_vis, maux, "after set_transforms + update, visibility record")
        fresh = spt.load_scene(path)
        try:
            fresh.set_transforms(xf)
            fsh, fvis = fresh.device_scene(0).probes(p, samples=S, max_depth=DEPTH, seed=SEED, aux=True)
            _check(fsh, moved, "a fresh scene")
            _check(fvis, moved_vis, "a fresh scene, visibility record")
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
p = np.random.default_rng(4).uniform(-3, 3, size=(300, 3)).astype(np.float32)
p[:, 1] += 2.0
host, host_vis = ds.probes(p, samples=3, max_depth=5, seed=11, first_point=9, aux=True)
assert np.isfinite(host).all() and np.abs(host).max() > 0.01
dev = torch.device("cuda", 0)
for width in (3, 4):
    rec = np.zeros((300, width), dtype=np.float32)
    rec[:, :3] = p
    t_sh, t_vis = ds.probes(torch.from_numpy(rec).to(dev), samples=3, max_depth=5, seed=11, first_point=9, aux=True)
    assert t_sh.device == dev and t_sh.shape == (300, 9, 3) and t_vis.shape == (300, 4)
    assert _util.same_words(t_sh.cpu().numpy(), host), "tensor probes differ from the host path"
    assert _util.same_words(t_vis.cpu().numpy(), host_vis), "tensor visibility records differ from the host path"
# an invalid record among device points: NaN words there, untouched neighbours
rec = np.zeros((300, 4), dtype=np.float32)
rec[:, :3] = p
rec[7, 1], rec[64, 0], rec[299, 2] = np.nan, np.inf, -np.inf
t_sh, t_vis = ds.probes(torch.from_numpy(rec).to(dev), samples=3, max_depth=5, seed=11, first_point=9, aux=True)
sh, vis = t_sh.cpu().numpy(), t_vis.cpu().numpy()
bad = np.zeros(300, dtype=bool)
bad[[7, 64, 299]] = True
assert (sh[bad].view(np.uint32) == 0x7fc00000).all() and (vis[bad].view(np.uint32) == 0x7fc00000).all()
assert _util.same_words(sh[~bad], host[~bad]) and _util.same_words(vis[~bad], host_vis[~bad])
# a host pointer under the device-pointer flag is refused and writes nothing
import ctypes
recs = np.zeros(300, dtype=spt.PROBE_DTYPE)
recs["p"] = p
job = spt.ProbeJob(size=ctypes.sizeof(spt.ProbeJob), flags=spt.PROBE_DEVICE_POINTERS, n_points=300, samples=1, max_depth=5, seed=11)
out = np.full((300, 27), np.float32(7.0))
t_pts = torch.from_numpy(rec).to(dev)
job.points, job.sh_out = recs.ctypes.data, out.ctypes.data
assert spt.hip_lib().spt_probe(ds._h, ctypes.byref(job)) == 1 and (out == 7.0).all()
job.points, job.sh_out = t_pts.data_ptr(), out.ctypes.data
assert spt.hip_lib().spt_probe(ds._h, ctypes.byref(job)) == 1 and (out == 7.0).all()
job.points, job.sh_out = t_pts.data_ptr() + 4, t_sh.data_ptr()
assert spt.hip_lib().spt_probe(ds._h, ctypes.byref(job)) == 1
job.points, job.sh_out, job.aux_out = t_pts.data_ptr(), t_sh.data_ptr(), out.ctypes.data
assert spt.hip_lib().spt_probe(ds._h, ctypes.byref(job)) == 1 and (out == 7.0).all()
assert _util.same_words(ds.probes(torch.from_numpy(np.ascontiguousarray(p)).to(dev), samples=3, max_depth=5, seed=11, first_point=9).cpu().numpy(), host)
sc.close()
print("probe tensors ok")
"""


def test_device_pointers_in_a_process_that_imported_torch_first():
    res = subprocess.run([sys.executable, "-c", _CHILD, _util.ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "probe tensors ok" in res.stdout, res.stdout + res.stderr


# ---- 7. isolation -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_films_and_async_frames_are_undisturbed(name):
    sc = _scene(name)
    p, ref, want, D, acc, aux = _reference(name)
    cfg = spt.OutputConfig(W, H, None, CAMERAS[name])
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=8, seed=3)
    with r.progressive(sc, cfg) as plain:
        undisturbed = plain.render(4).render(4).mean().copy()
    with r.progressive(sc, cfg) as film:
        film.render(4)
        _check(_ds(name).probes(p, samples=S, max_depth=DEPTH, seed=SEED), want, "between two increments")
        assert _util.same_words(film.render(4).mean(), undisturbed)
    sync = r.render_shard(sc, cfg).copy()
    buf = r.render_shard(sc, cfg, reuse_output=True, wait=False)
    sh, vis = _ds(name).probes(p, samples=S, max_depth=DEPTH, seed=SEED, aux=True)
    _check(sh, want, "behind an asynchronous frame")
    _check(vis, aux, "behind an asynchronous frame, visibility record")
    r.wait(sc)
    assert _util.same_words(np.array(buf), sync)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_leave_the_scene_usable():
    name = "t_materials"
    p, ref, want, D, acc, aux = _reference(name)
    sc, ds = _scene(name), _ds(name)
    lib = spt.hip_lib()
    n = p.shape[0]
    recs = np.zeros(n, dtype=spt.PROBE_DTYPE)
    recs["p"] = p
    out = np.empty((n, 27), dtype=f32)
    vis = np.empty((n, 4), dtype=f32)

    def job(arr=recs, **kw):
        j = spt.ProbeJob(size=C.sizeof(spt.ProbeJob), n_points=arr.shape[0], samples=S, max_depth=DEPTH, seed=SEED)
        j.points, j.sh_out, j.aux_out = arr.ctypes.data, out.ctypes.data, vis.ctypes.data
        j.keep = arr      # (the job's pointer does not own the array)
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(j, scene=ds._h, word=None, status=1):
        out.view(np.uint32)[:] = PATTERN
        vis.view(np.uint32)[:] = PATTERN
        assert lib.spt_probe(scene, C.byref(j) if j is not None else None) == status
        assert (out.view(np.uint32) == PATTERN).all() and (vis.view(np.uint32) == PATTERN).all()
        if word is not None:
            assert word in lib.spt_last_error().decode(), lib.spt_last_error()

    def edited(at, value):
        bad = recs.copy()
        bad["p"][at] = value
        return bad

    refused(job(), scene=None)
    refused(None)
    refused(job(points=None))
    refused(job(sh_out=None))
    refused(job(flags=2), word="flags")
    refused(job(flags=0x80000000), word="flags")
    refused(job(samples=0), word="samples")
    refused(job(size=C.sizeof(spt.ProbeJob) - 8), word="size")
    refused(job(max_depth=256), status=4)
    refused(job(edited(5, [0, np.nan, 0])), word="point 5 ")
    refused(job(edited(n - 1, [np.inf, 0, 0])), word="point %d " % (n - 1))
    refused(job(edited(200, [0, 0, -np.inf]), points_per_pass=64), word="point 200 ")   # a later pass: still nothing written
    refused(job(flags=spt.PROBE_DEVICE_POINTERS), word="device")
    # nothing to do is not a refusal, and writes nothing either
    refused(job(n_points=0), status=0)
    refused(job(n_points=0, points=None, sh_out=None, aux_out=None), status=0)
    # a good call after all of them, and a render
    sh, v = ds.probes(p, samples=S, max_depth=DEPTH, seed=SEED, aux=True)
    _check(sh, want, "after the refusals")
    _check(v, aux, "after the refusals, visibility record")
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=2, seed=3)
    assert np.isfinite(r.render_shard(sc, spt.OutputConfig(W, H, None, CAMERAS[name]))).any()


# ---- 9. the CLI ---------------------------------------------------------------------------------------------------------------------

def test_the_cli_writes_the_words_of_probes(tmp_path):
    name = "t_textured"
    cli = os.path.join(spt.LIB_DIR, "spt")
    p = _points(name)[:50]
    src, out = tmp_path / "points.txt", tmp_path / "probes.txt"
    src.write_text("".join("%.9g %.9g %.9g\n" % tuple(float(v) for v in row) for row in p) + "\n")
    renderer = os.path.join(_util.SCENES, "pt.json")
    res = subprocess.run([cli, "-s", os.path.join(_util.SCENES, name + ".json"), "-r", renderer, "-o", str(out), "--bake-probes", str(src),
                          "--probe-samples", "4", "--seed", "5"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    depth = spt.load_renderer(renderer).max_depth
    sh, vis = _ds(name).probes(p, samples=4, max_depth=depth, seed=5, aux=True)
    got = np.array([[float(v) for v in line.split()] for line in out.read_text().splitlines()])
    assert got.shape == (50, 31)
    _check(got[:, :27].astype(f32).reshape(50, 9, 3), sh, "the CLI's coefficients")
    _check(got[:, 27:].astype(f32), vis, "the CLI's visibility records")
    assert np.abs(sh).max() > 0.01

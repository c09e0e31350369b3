"""spt_scene_deform (Scene.set_mesh_positions + DeviceScene.update, DeviceScene.update_arrays(meshes=...)): a scene after a
deformation behaves, word for word, like a scene freshly created from the edited descriptor.

The scene is the one of tests/_scene_deform_scenes.py.  48 x 32 pixels @ 4 spp, max_depth 4 unless a test says otherwise.  Every
comparison is _util.same_words against the exhaustive oracle on the host scene of that moment and / or against a fresh device scene."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _radiance_ref
import _scene_deform_scenes as S
import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32
W, H, SPP, DEPTH, SEED = 48, 32, 4, 4, 7
INVALID_ARG, UNSUPPORTED = 1, 4
FLAGS = _util.ORACLE_EXHAUSTIVE

_DIR = None


def _tracer(spp=SPP, seed=SEED):
    return spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=spp, seed=seed)


@pytest.fixture(scope="module", autouse=True)
def _files(tmp_path_factory):
    global _DIR
    d = str(tmp_path_factory.mktemp("scene_deform"))
    for agg in ("bvh", "group"):
        S.write_scene(d, "uniform_%s.json" % agg, aggregate=agg)
    S.write_scene(d, "power_is_bvh.json", light_sampler="power_is")
    S.write_scene(d, "big.json", big=True)
    _DIR = d
    yield d
    for cached in (_ref_scene, _rest, _rays, _plan_rays, _first):
        cached.cache_clear()
    _BIG.clear()


def _load(which="uniform", agg="bvh"):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_DIR, "%s_%s.json" % (which, agg) if which != "big" else "big.json"))


@functools.lru_cache(maxsize=None)
def _ref_scene(which="uniform", agg="bvh"):
    return _load(which, agg)      # never edited


@functools.lru_cache(maxsize=None)
def _rest(name):
    """The file's own vertex positions of a mesh; read-only."""
    p = _ref_scene().mesh_positions(name)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _rays():
    rays = _util.random_rays(_ref_scene(), 4096, seed=3, spread=3.0)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def _plan_rays():
    rays = _radiance_ref.plan_rays(spt, _ref_scene(), _tracer(), W, H, 0, SPP).reshape(-1)
    rays.setflags(write=False)
    return rays


def _oracle(sc):
    """film, closest hits, occlusion and the plan's samples of a host scene as it stands, by the exhaustive oracle."""
    film, _ = _util.oracle_render(sc, _tracer(), W, H, flags=FLAGS)
    return (film, _util.oracle_trace_closest(sc, _rays(), FLAGS), _util.oracle_trace_any(sc, _rays(), FLAGS),
            _util.oracle_render_samples(sc, _tracer(), W, H, 0, SPP, flags=FLAGS).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def _first(which, agg):
    """The oracle's answers on the file as loaded, once per file; read-only."""
    out = _oracle(_ref_scene(which, agg))
    for a in out:
        a.setflags(write=False)
    return out


def _render(scene, spp=SPP, w=W, h=H):
    return _tracer(spp).render_shard(scene, spt.OutputConfig(w, h)).copy()


def _same_hits(a, b):
    return all(_util.same_words(np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])) for f in a.dtype.names)


def _answers(scene):
    ds = scene.device_scene(0)
    return (_render(scene), ds.trace_closest(_rays()), ds.trace_any(_rays()), ds.radiance(_plan_rays(), max_depth=DEPTH, seed=SEED))


def _check_answers(got, want, what):
    assert _util.same_words(got[0], want[0]), what + ": film"
    assert _same_hits(got[1], want[1]), what + ": closest hits"
    assert np.array_equal(got[2], want[2]), what + ": occlusion"
    assert _util.same_words(got[3], want[3]), what + ": radiance"


def _deform(sc, edits):
    """{mesh name: new positions} on a host scene."""
    for name, pos in edits.items():
        sc.set_mesh_positions(name, pos)


def _fresh_answers(edits, which="uniform", agg="bvh"):
    """The answers of a device scene freshly created from a host scene with `edits` applied."""
    fresh = _load(which, agg)
    _deform(fresh, edits)
    out = _answers(fresh)
    fresh.close()
    return out


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------

MODES = {
    "default": ({}, "bvh"),
    "no_eye_blob": ({"SPT_NO_EYE_BLOB": "1"}, "bvh"),
    "no_lds_geo": ({"SPT_NO_LDS_GEO": "1"}, "bvh"),
    "no_lds_geo_no_stream": ({"SPT_NO_LDS_GEO": "1", "SPT_NO_STREAM": "1"}, "bvh"),
    "group": ({}, "group"),
    "group_no_lds_geo": ({"SPT_NO_LDS_GEO": "1"}, "group"),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_deform_equals_a_fresh_scene_and_the_oracle(mode, monkeypatch):
    env, agg = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = _load("uniform", agg)
    ds = sc.device_scene(0)
    first = _answers(sc)
    _check_answers(first, _first("uniform", agg), "as loaded")
    assert float(first[0].max()) > 0.05 and (first[1]["instance"] >= 0).sum() > 500
    edits = {name: fn(_rest(name)) for name, fn in S.DEFORMED.items()}
    _deform(sc, edits)
    ds.update()
    assert ds.render_info(4) == 1
    after = _answers(sc)
    _check_answers(after, _fresh_answers(edits, "uniform", agg), "deformed against a fresh scene")
    _check_answers(after, _oracle(sc), "deformed")
    assert not _util.same_words(after[0], first[0])
    _deform(sc, {name: _rest(name) for name in edits})
    ds.update()
    assert ds.render_info(4) == 2
    _check_answers(_answers(sc), first, "back to the file's positions")
    sc.close()


def test_power_is_scene_follows_the_quad(monkeypatch):
    """The emissive quad under the power_is sampler: its power, and with it the alias table, changes with its area."""
    sc = _load("power_is")
    ds = sc.device_scene(0)
    _check_answers(_answers(sc), _first("power_is", "bvh"), "as loaded")
    power = sc.array("lights")["power"].copy()
    edits = {"quad": S.bend(_rest("quad") * f32(1.5)), "cloth": S.wave(_rest("cloth"))}
    _deform(sc, edits)
    assert not np.array_equal(sc.array("lights")["power"], power)
    ds.update()
    after = _answers(sc)
    _check_answers(after, _fresh_answers(edits, "power_is"), "deformed against a fresh scene")
    _check_answers(after, _oracle(sc), "deformed")
    sc.close()


# ---- 2. exponent and degenerate paths ------------------------------------------------------------------------------------------

def _shapes():
    cloth, fan = _rest("cloth"), _rest("tri5")
    corner = cloth.min(axis=0)
    return {
        "scaled_far": {"cloth": ((cloth - corner) * f32(100.0) + corner + np.array([4000.0, -150.0, -9000.0], dtype=f32)).astype(f32)},
        "flat": {"cloth": (cloth * np.array([1.0, 0.0, 1.0], dtype=f32) + np.array([0.0, 0.125, 0.0], dtype=f32)).astype(f32)},
        "point": {"tri5": np.tile(np.array([[0.25, 0.5, -0.125]], dtype=f32), (len(fan), 1))},
    }


@pytest.mark.parametrize("lds", ["default", "no_lds_geo"])
@pytest.mark.parametrize("shape", ["scaled_far", "flat", "point"])
def test_exponent_and_degenerate_shapes(shape, lds, monkeypatch):
    if lds == "no_lds_geo":
        monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    edits = _shapes()[shape]
    sc = _load()
    ds = sc.device_scene(0)
    _render(sc)
    _deform(sc, edits)
    ds.update()
    after = _answers(sc)
    _check_answers(after, _fresh_answers(edits), shape + " against a fresh scene")
    _check_answers(after, _oracle(sc), shape)
    sc.close()


# ---- 3. only the named meshes move ---------------------------------------------------------------------------------------------

def _misses_box(rays, lo, hi):
    """True per ray whose line misses the box [lo, hi] widened by 1 % (slabs in f64)."""
    o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    pad = 0.01 * (hi - lo) + 1e-3
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - pad - o) / d, (hi + pad - o) / d
    near, far = np.fmin(t0, t1).max(axis=1), np.fmax(t0, t1).min(axis=1)
    return ~(near <= far)


def test_only_the_named_mesh_moves(monkeypatch):
    monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc = _load()
    ds = sc.device_scene(0)
    inst = sc.array("instances")
    cloth = sc.instance_index("cloth")
    # rays aimed at the middle of every other instance's box from above and in front, next to the random ones
    aimed = np.zeros(0, dtype=spt.RAY_DTYPE)
    for i in range(len(inst)):
        if i == cloth:
            continue
        c = (inst["bmin"][i] + inst["bmax"][i]) / 2
        rays = np.zeros(16, dtype=spt.RAY_DTYPE)
        o = c + np.array([0.0, 1.5, 4.0]) + np.random.default_rng(i).uniform(-0.2, 0.2, size=(16, 3))
        d = c - o
        rays["o"], rays["d"] = o.astype(f32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
        rays["t_min"], rays["t_max"] = 1e-4, f32(3.4028234663852886e38)
        aimed = np.concatenate([aimed, rays])
    rays = np.concatenate([_rays(), aimed])
    before = ds.trace_closest(rays)
    lo0, hi0 = inst["bmin"][cloth].astype(np.float64), inst["bmax"][cloth].astype(np.float64)
    sc.set_mesh_positions("cloth", S.wave(_rest("cloth"), phase=1.0, amp=0.4))
    ds.update()
    inst = sc.array("instances")
    cloth = sc.instance_index("cloth")
    lo, hi = np.minimum(lo0, inst["bmin"][cloth]), np.maximum(hi0, inst["bmax"][cloth])
    away = _misses_box(rays, lo, hi)
    after = ds.trace_closest(rays)
    assert _same_hits(after[away], before[away])
    hit = set(int(i) for i in after[away]["instance"] if i >= 0)
    assert hit == set(range(len(inst))) - {cloth}, "every other instance is hit by a ray that passes the cloth by"
    assert not _same_hits(after, before)
    assert _same_hits(after, _util.oracle_trace_closest(sc, rays, FLAGS))
    sc.close()


def test_a_deformation_copies_the_named_triangles_only(monkeypatch):
    """Next to a 60 552-triangle mesh that is not named (11.6 MB of records), on the large-scene path: counter 5 is at most the
    update's bound (1024 B per instance + 128 B per light + 16 KB, tests/test_gpu_scene_update.py) + 192 B per named triangle + 64."""
    monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc = _load("big")
    d = sc.desc
    assert d.n_tris >= 60000 + 288
    ds = sc.device_scene(0)
    r = _tracer()
    cfg = spt.OutputConfig(W, H)
    r.render_shard(sc, cfg)
    update_bound = 1024 * d.n_instances + 128 * d.n_lights + 16384
    named = 0
    for name in ("cloth", "quad"):
        sc.set_mesh_positions(name, S.DEFORMED[name](_rest(name)))
        named += int(sc.array("meshes")[sc.mesh_index(name)]["tri_count"])
        ds.update()
        copied = ds.render_info(5)
        print("bytes copied by the deformation of %s:" % name, copied)
        n = int(sc.array("meshes")[sc.mesh_index(name)]["tri_count"])
        assert 0 < copied <= update_bound + 192 * n + 64
    assert ds.render_info(4) == 2
    assert _util.same_words(r.render_shard(sc, cfg), _util.oracle_render(sc, r, W, H, flags=FLAGS)[0])
    sc.close()


_BIG = {}


def _big_reference():
    """The 60 552-triangle terrain deformed twice: per state the positions and the exhaustive oracle's film, closest hits and
    occlusion on the edited host scene (made once, shared by the modes; read-only)."""
    if not _BIG:
        host = _load("big")
        rest = host.mesh_positions("terrain")
        rays = _util.random_rays(host, 4096, seed=11, spread=2.0)
        states = {"rest": rest, "ridge": S.shear(S.wave(rest, phase=0.5, amp=0.3), k=0.5), "swell": S.wave(rest, phase=2.0, amp=0.12)}
        _BIG["rays"] = rays
        for key, pos in states.items():
            host.set_mesh_positions("terrain", pos)
            want = (_util.oracle_render(host, _tracer(), W, H, flags=FLAGS)[0], _util.oracle_trace_closest(host, rays, FLAGS), _util.oracle_trace_any(host, rays, FLAGS))
            _BIG[key] = (pos, want)
        host.close()
    return _BIG


@pytest.mark.parametrize("walker", ["stream", "no_stream"])
def test_a_mesh_of_many_workgroups_is_refitted(walker, monkeypatch):
    """The terrain: 237 workgroups of triangles, and a 4-wide tree of some twenty thousand nodes - dozens of workgroups per level
    launch, about ten levels.  Deformed twice (the second call finds the heights made), then back: every state equals the
    exhaustive oracle on the edited host scene and a scene freshly created from it."""
    monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    if walker == "no_stream":
        monkeypatch.setenv("SPT_NO_STREAM", "1")
    ref = _big_reference()
    rays = ref["rays"]

    def answers(scene):
        ds = scene.device_scene(0)
        return _render(scene), ds.trace_closest(rays), ds.trace_any(rays)

    def check(got, want, what):
        assert _util.same_words(got[0], want[0]), what + ": film"
        assert _same_hits(got[1], want[1]), what + ": closest hits"
        assert np.array_equal(got[2], want[2]), what + ": occlusion"

    sc = _load("big")
    ds = sc.device_scene(0)
    terrain = sc.instance_index("terrain")
    first = answers(sc)
    check(first, ref["rest"][1], "as loaded")
    assert (first[1]["instance"] == terrain).sum() > 500
    for key in ("ridge", "swell", "rest"):
        pos, want = ref[key]
        sc.set_mesh_positions("terrain", pos)
        ds.update()
        got = answers(sc)
        check(got, want, key)
        if key == "ridge":
            fresh = _load("big")
            fresh.set_mesh_positions("terrain", pos)
            check(got, answers(fresh), key + " against a fresh scene")
            fresh.close()
            moved = got[1]["t"][first[1]["instance"] == terrain] != first[1]["t"][first[1]["instance"] == terrain]
            assert moved.sum() > 300
    check(got, first, "back to the file's positions")
    assert ds.render_info(4) == 3
    sc.close()


# ---- 4. ordering ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lds", ["default", "no_lds_geo"])
def test_async_frames_around_a_deformation(lds, monkeypatch):
    if lds == "no_lds_geo":
        monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc, host = _load(), _load()          # `host`: the same edits without a device scene, for the oracle
    ds = sc.device_scene(0)
    r = _tracer()
    cfg = spt.OutputConfig(W, H)
    film_first = _first("uniform", "bvh")[0]
    pinned = ds.film_buffer(2 * H, W)
    pinned[:] = np.nan
    buf1, buf2 = pinned[:H], pinned[H:]
    r.render_shard(sc, cfg, film=buf1, wait=False)
    edits = {name: fn(_rest(name)) for name, fn in S.DEFORMED.items()}
    _deform(sc, edits)
    ds.update()                                   # no wait in between
    r.render_shard(sc, cfg, film=buf2, wait=False)
    r.wait(sc)
    assert _util.same_words(buf1, film_first)
    assert _util.same_words(buf2, _util.oracle_render(sc, r, W, H, flags=FLAGS)[0])
    # a burst: deformation + frame, six times over, one wait at the end
    bufs = ds.film_buffer(6 * H, W)
    want = []
    for k in range(6):
        edit = {"cloth": S.wave(_rest("cloth"), phase=0.7 * k), "cube": S.shear(_rest("cube"), k=0.1 * k)}
        _deform(sc, edit)
        ds.update()
        r.render_shard(sc, cfg, film=bufs[k * H:(k + 1) * H], wait=False)
        _deform(host, dict(edits, **edit))
        want.append(_render(host))                # a scene freshly created from the state of frame k
        host.close_device_scene(0)
    r.wait(sc)
    for k in range(6):
        assert _util.same_words(bufs[k * H:(k + 1) * H], want[k]), k
    assert not _util.same_words(want[0], want[1])
    sc.close()
    host.close()


# ---- 5. refusals and atomicity -------------------------------------------------------------------------------------------------

def _records(sc, name, positions=None):
    """(mesh index, TriPos records, TriAttr records) of a mesh as a host scene with `positions` set has them."""
    if positions is not None:
        sc.set_mesh_positions(name, positions)
    m = sc.mesh_index(name)
    mesh = sc.array("meshes")[m]
    a, b = int(mesh["tri_first"]), int(mesh["tri_first"]) + int(mesh["tri_count"])
    return m, sc.array("tri_pos")[a:b].copy(), sc.array("tri_attr")[a:b].copy()


@pytest.mark.parametrize("lds", ["default", "no_lds_geo"])
def test_refusals_leave_the_scene_as_it_was(lds, monkeypatch):
    if lds == "no_lds_geo":
        monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc, edited = _load(), _load()
    ds = sc.device_scene(0)
    first = _answers(sc)
    _check_answers(first, _first("uniform", "bvh"), "as loaded")
    m, tri_pos, tri_attr = _records(edited, "cloth", S.wave(_rest("cloth")))
    inst, lights = edited.array("instances"), edited.array("lights")

    def refused(status, meshes, instances=inst):
        with pytest.raises(spt.SptError) as e:
            ds.update_arrays(instances, lights, tlas_nodes=edited.array("tlas_nodes"), meshes=meshes)
        assert e.value.status == status, str(e.value)
        _check_answers(_answers(sc), first, "a refused deformation changed the scene")

    refused(INVALID_ARG, {sc.desc.n_meshes: (tri_pos, None)})                      # mesh index out of range
    refused(INVALID_ARG, {m: (tri_pos[:-1], None)})                                # wrong tri_count
    refused(INVALID_ARG, {m: (np.concatenate([tri_pos, tri_pos[:1]]), None)})
    for field, value in (("p0", np.nan), ("p1", np.inf), ("p2", -np.inf)):         # a position that is not finite
        bad = tri_pos.copy()
        bad[field][len(bad) // 2, 1] = value
        refused(INVALID_ARG, {m: (bad, tri_attr)})
    refused(INVALID_ARG, {m: (tri_pos, tri_attr)}, instances=inst[:-1])            # `u` gets the update's checks
    # a mesh named twice, null arrays: through the raw entry point
    d = edited.desc
    u = spt.SceneUpdateDesc(size=C.sizeof(spt.SceneUpdateDesc), flags=0, n_tlas_nodes=d.n_tlas_nodes, tlas_nodes=d.tlas_nodes, n_instances=d.n_instances,
                            instances=d.instances, n_lights=d.n_lights, lights=d.lights, light_alias=d.light_alias)
    edits = (spt.MeshDeform * 2)()
    for e in edits:
        e.mesh, e.tri_count = m, len(tri_pos)
        e.tri_pos = C.cast(tri_pos.ctypes.data, C.POINTER(spt.TriPos))
    lib = spt.hip_lib()
    assert lib.spt_scene_deform(ds._h, C.byref(u), 2, edits) == INVALID_ARG
    assert lib.spt_scene_deform(ds._h, C.byref(u), 1, None) == INVALID_ARG
    assert lib.spt_scene_deform(ds._h, None, 1, edits) == INVALID_ARG
    assert lib.spt_scene_deform(None, C.byref(u), 1, edits) == INVALID_ARG
    edits[0].tri_pos = None
    assert lib.spt_scene_deform(ds._h, C.byref(u), 1, edits) == INVALID_ARG
    edits[0].tri_pos = C.cast(tri_pos.ctypes.data, C.POINTER(spt.TriPos))
    u.flags = 1
    assert lib.spt_scene_deform(ds._h, C.byref(u), 1, edits) == INVALID_ARG
    u.flags = 0
    _check_answers(_answers(sc), first, "a refused deformation changed the scene")
    with _tracer().progressive(sc, spt.OutputConfig(W, H)) as pf:                  # a live film
        pf.render(1)
        assert lib.spt_scene_deform(ds._h, C.byref(u), 1, edits) == INVALID_ARG
        assert _util.same_words(pf.render(SPP - 1).mean(), first[0])
    assert ds.render_info(4) == 0
    assert lib.spt_scene_deform(ds._h, C.byref(u), 1, edits) == 0                  # the film is gone: the same call goes through
    _check_answers(_answers(sc), _answers(edited), "the deformation that went through")
    # no meshes: an update
    assert lib.spt_scene_deform(ds._h, C.byref(u), 0, None) == 0
    assert ds.render_info(4) == 2
    _check_answers(_answers(sc), _answers(edited), "a deformation without meshes")
    sc.close()
    edited.close()


def test_a_scene_on_the_callers_trees_refuses(monkeypatch):
    monkeypatch.setenv("SPT_REFERENCE_BVH", "1")
    sc = _load()
    ds = sc.device_scene(0)
    first = _answers(sc)
    sc.set_mesh_positions("cloth", S.wave(_rest("cloth")))
    with pytest.raises(spt.SptError) as e:
        ds.update()
    assert e.value.status == UNSUPPORTED, str(e.value)
    _check_answers(_answers(sc), first, "the refused deformation changed the scene")
    assert ds.render_info(4) == 0
    sc.close()


def test_lds_scene_that_outgrows_lds_refuses():
    """The LDS-resident form has room for 32 KB, of which this scene's 308 triangles take 14.8 KB and its instances 2 KB.  Every
    cloth triangle shrunk about its centroid leaves 288 islands, which the SAH builder separates down to one triangle per leaf:
    287 wide nodes of 64 B, 18.4 KB, where the cloth as loaded (leaves of up to four) takes about a third of that."""
    sc = _load()
    ds = sc.device_scene(0)
    first = _answers(sc)
    m, tri_pos, _ = _records(sc, "cloth")
    corners = np.stack([tri_pos["p0"], tri_pos["p1"], tri_pos["p2"]], axis=1)
    centre = corners.mean(axis=1, keepdims=True)
    shrunk = tri_pos.copy()
    for k, field in enumerate(("p0", "p1", "p2")):
        shrunk[field] = (centre + (corners - centre) * f32(0.05))[:, k].astype(f32)
    with pytest.raises(spt.SptError) as e:
        ds.update_arrays(sc.array("instances"), sc.array("lights"), meshes={m: (shrunk, None)})
    assert e.value.status == UNSUPPORTED and "recreate the scene" in str(e.value), str(e.value)
    _check_answers(_answers(sc), first, "the refused deformation changed the scene")
    assert ds.render_info(4) == 0
    sc.close()


def test_bezier_scene_forwards_the_deformation(tmp_path):
    """t_bezier-like content with one trimesh: the scene lives in the library with the Bezier primitive, the call is passed on.
    NOT covered: the refusal "the Bezier library does not export the symbol" (SPT_ERR_UNSUPPORTED).  The plain library opens the
    libspt_hip_bez.so that sits next to it and there is no way to hand it another one, so a library without spt_scene_deform cannot
    be put in its place from a test; the branch is the three lines in front of the forwarding call in spt_scene_deform, the same
    as spt_scene_update's (which its test does not reach either)."""
    import json
    _util.ensure_cpu_build()
    with open(os.path.join(_util.SCENES, "t_bezier.json")) as f:
        doc = json.load(f)
    import shutil
    for entry in doc["primitives"] + doc["textures"]:       # the files the scene names, next to the copy
        for key, rel in entry.items():
            if key.endswith("_file"):
                os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
                shutil.copy(os.path.join(_util.SCENES, rel), str(tmp_path / rel))
    S.write_models(tmp_path)
    doc["primitives"].append({"type": "trimesh", "name": "cloth", "obj_file": "models/cloth.obj"})
    doc["instances"].append({"name": "cloth", "primitive": "cloth", "material": doc["materials"][0]["name"], "scale": [0.8, 1.0, 0.8], "translate": [0.0, 0.6, 0.0]})
    path = str(tmp_path / "bezier_cloth.json")
    with open(path, "w") as f:
        json.dump(doc, f)
    sc, edited = spt.load_scene(path), spt.load_scene(path)
    assert sc.desc.n_bezier_patches > 0
    r = _tracer(spp=2)
    cfg = spt.OutputConfig(32, 24, None, "main")
    before = r.render_shard(sc, cfg).copy()
    pos = S.wave(sc.mesh_positions("cloth"), amp=0.5)
    for s in (sc, edited):
        s.set_mesh_positions("cloth", pos)
    sc.device_scene(0).update()
    assert sc.device_scene(0).render_info(4) == 1
    got = r.render_shard(sc, cfg).copy()
    assert _util.same_words(got, r.render_shard(edited, cfg))
    assert not _util.same_words(got, before)
    sc.close()
    edited.close()


# ---- 6. a long-lived scene -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_random_sessions_on_one_device_scene(seed, monkeypatch):
    if seed % 2:
        monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    rng = np.random.default_rng(2000 + seed)
    sizes = [(24, 16), (32, 20)]
    w, h = sizes[0]
    spp = 2
    sc = _load("power_is" if seed >= 2 else "uniform")
    ds = sc.device_scene(0)
    r = _tracer(spp, seed=seed + 1)
    calls = 0
    for step in range(8):
        op = rng.choice(["deform", "move", "light", "resize"], p=[0.55, 0.2, 0.15, 0.1]) if step else "deform"
        if op == "deform":
            name = str(rng.choice(S.MESHES))
            sc.set_mesh_positions(name, S.smooth(_rest(name), rng))
            ds.update()
            calls += 1
        elif op == "move":
            fwd = sc.array("instances")[sc.instance_index("cube_b")]["fwd"].copy()
            fwd[9:12] += rng.uniform(-0.4, 0.4, size=3).astype(f32)
            sc.set_transforms({"cube_b": fwd})
            ds.update()
            calls += 1
        elif op == "light":
            lights = sc.array("lights")
            light = spt.Light.from_buffer_copy(lights[int(np.flatnonzero(lights["type"] == 1)[0])].tobytes())
            light.pos[:] = [float(v) for v in rng.uniform(-3, 3, size=3) + np.array([0, 3.0, 0])]
            sc.set_light("bulb", light)
            ds.update()
            calls += 1
        else:
            w, h = sizes[1] if (w, h) == sizes[0] else sizes[0]
        cfg = spt.OutputConfig(w, h)
        check = step % 4
        if check == 0:
            assert _util.same_words(r.render_shard(sc, cfg), _util.oracle_render(sc, r, w, h, flags=FLAGS)[0]), (seed, step, op)
        elif check == 1:
            with r.progressive(sc, cfg) as pf:
                assert _util.same_words(pf.render(spp).mean(), _util.oracle_render(sc, r, w, h, flags=FLAGS)[0]), (seed, step, op)
        elif check == 2:
            rays = _util.random_rays(sc, 512, seed=int(rng.integers(1 << 30)), spread=3.0)
            assert _same_hits(ds.trace_closest(rays), _util.oracle_trace_closest(sc, rays, FLAGS)), (seed, step, op)
            assert np.array_equal(ds.trace_any(rays), _util.oracle_trace_any(sc, rays, FLAGS)), (seed, step, op)
        else:
            rays = _radiance_ref.plan_rays(spt, sc, r, w, h, 0, spp).reshape(-1)
            want = _util.oracle_render_samples(sc, r, w, h, 0, spp, flags=FLAGS).reshape(-1, 3)
            assert _util.same_words(ds.radiance(rays, max_depth=DEPTH, seed=seed + 1), want), (seed, step, op)
        assert ds.render_info(4) == calls
    sc.close()

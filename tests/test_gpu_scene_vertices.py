"""spt_scene_mesh_topology / spt_scene_deform_vertices / spt_scene_read_triangles (Scene.set_mesh_vertices + DeviceScene.update,
DeviceScene.set_topology / update_arrays(vertices=...) / read_triangles): a scene deformed from vertex arrays holds, word for word,
the records the host loader makes of the same vertices, and behaves like a scene freshly created from them.

The scene is the one of tests/_scene_deform_scenes.py.  48 x 32 pixels @ 4 spp, max_depth 4 unless a test says otherwise.  Every
comparison is _util.same_words: against a fresh device scene of a host scene edited with set_mesh_positions, against the exhaustive
oracle on the host scene, and of read_triangles against the host scene's tri_pos / tri_attr ranges."""
import ctypes as C
import functools
import json
import os
import shutil

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


def _normal_map_scene(d):
    """The scene with a normal map on the cloth: the image is a small PNG written here."""
    doc = S.scene_dict()
    rng = np.random.default_rng(5)
    img = np.zeros((16, 16, 3), dtype=np.uint8)
    img[..., 0:2] = rng.integers(40, 216, size=(16, 16, 2))      # tilted up to about 45 degrees, differently per texel
    img[..., 2] = 255
    os.makedirs(os.path.join(d, "textures"), exist_ok=True)
    spt.write_png(os.path.join(d, "textures", "tilt.png"), img)
    doc["textures"].append({"type": "image", "name": "tilt", "image_file": "textures/tilt.png", "tiling": [3.0, 3.0]})
    for s in doc["surfaces"]:
        if s["name"] == "s_cloth":
            s["normal_map"] = "tilt"
    path = os.path.join(d, "normal_map.json")
    with open(path, "w") as f:
        json.dump(doc, f)
    return path


@pytest.fixture(scope="module", autouse=True)
def _files(tmp_path_factory):
    global _DIR
    _util.ensure_cpu_build()
    d = str(tmp_path_factory.mktemp("scene_vertices"))
    for agg in ("bvh", "group"):
        S.write_scene(d, "uniform_%s.json" % agg, aggregate=agg)
    S.write_scene(d, "big.json", big=True)
    _normal_map_scene(d)
    _DIR = d
    yield d
    for cached in (_ref_scene, _rest, _rays, _plan_rays, _first):
        cached.cache_clear()


def _load(which="uniform", agg="bvh"):
    return spt.load_scene(os.path.join(_DIR, "%s_%s.json" % (which, agg) if which == "uniform" else which + ".json"))


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


def _same_records(a, b):
    return _util.same_words(np.frombuffer(a.tobytes(), dtype=f32), np.frombuffer(b.tobytes(), dtype=f32))


def _check_records(ds, host, what, names=S.MESHES):
    """read_triangles of the named meshes against the host scene's ranges (reading them makes the host's pending meshes)."""
    meshes, tri_pos, tri_attr = host.array("meshes"), host.array("tri_pos"), host.array("tri_attr")
    for name in names:
        m = host.mesh_index(name)
        a, b = int(meshes[m]["tri_first"]), int(meshes[m]["tri_first"]) + int(meshes[m]["tri_count"])
        got_pos, got_attr = ds.read_triangles(m)
        assert _same_records(got_pos, tri_pos[a:b]), "%s: tri_pos of %s" % (what, name)
        assert _same_records(got_attr, tri_attr[a:b]), "%s: tri_attr of %s" % (what, name)


def _by_vertices(sc, edits, normals=None):
    for name, pos in edits.items():
        sc.set_mesh_vertices(name, pos, (normals or {}).get(name))


def _by_positions(sc, edits, normals=None):
    for name, pos in edits.items():
        sc.set_mesh_positions(name, pos, (normals or {}).get(name))


def _fresh(edits, which="uniform", agg="bvh", normals=None):
    """A host scene with `edits` applied by set_mesh_positions, and the answers of a device scene freshly created from it."""
    fresh = _load(which, agg)
    _by_positions(fresh, edits, normals)
    return fresh, _answers(fresh)


# ---- 4. parity -----------------------------------------------------------------------------------------------------------------

MODES = {
    "default": ({}, "bvh"),                                   # LDS-resident: the records are made on the host
    "no_lds_geo": ({"SPT_NO_LDS_GEO": "1"}, "bvh"),
    "no_lds_geo_no_stream": ({"SPT_NO_LDS_GEO": "1", "SPT_NO_STREAM": "1"}, "bvh"),
    "group_no_lds_geo": ({"SPT_NO_LDS_GEO": "1"}, "group"),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_vertices_equal_a_fresh_scene_the_oracle_and_the_host_records(mode, monkeypatch):
    env, agg = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = _load("uniform", agg)
    ds = sc.device_scene(0)
    first = _answers(sc)
    _check_answers(first, _first("uniform", agg), "as loaded")
    _check_records(ds, sc, "as loaded")
    edits = {name: fn(_rest(name)) for name, fn in S.DEFORMED.items()}
    _by_vertices(sc, edits)
    ds.update()
    assert ds.render_info(4) == 1
    after = _answers(sc)
    fresh, want = _fresh(edits, "uniform", agg)
    _check_answers(after, want, "deformed against a fresh scene")
    _check_records(ds, fresh, "deformed against the host scene edited by positions")
    fresh.close()
    _check_answers(after, _oracle(sc), "deformed")
    _check_records(ds, sc, "deformed")
    assert not _util.same_words(after[0], first[0])
    _by_vertices(sc, {name: _rest(name) for name in edits})
    ds.update()
    assert ds.render_info(4) == 2
    _check_answers(_answers(sc), first, "back to the file's positions")
    _check_records(ds, _ref_scene("uniform", agg), "back to the file's positions")
    sc.close()


# ---- 5. normals and frames reach the film ----------------------------------------------------------------------------------------

def test_normals_and_frames_reach_the_film(monkeypatch):
    monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc = _load("normal_map")
    ds = sc.device_scene(0)
    assert _util.same_words(_render(sc), _util.oracle_render(sc, _tracer(), W, H, flags=FLAGS)[0]), "as loaded"
    pos = S.wave(sc.mesh_positions("cloth"))
    nrm = np.tile(np.array([[0.0, 0.8, 0.6]], dtype=f32), (len(pos), 1))
    nrm[::3] = np.array([0.36, 0.8, -0.48], dtype=f32)
    sc.set_mesh_vertices("cloth", pos)
    ds.update()
    old_normals = _render(sc)
    sc.set_mesh_vertices("cloth", pos, nrm)
    ds.update()
    got = _render(sc)
    fresh = _load("normal_map")
    fresh.set_mesh_positions("cloth", pos, nrm)
    assert _util.same_words(got, _render(fresh)), "against a fresh scene"
    _check_records(ds, fresh, "new normals", names=("cloth",))
    fresh.close()
    assert _util.same_words(got, _util.oracle_render(sc, _tracer(), W, H, flags=FLAGS)[0]), "against the oracle"
    assert not _util.same_words(got, old_normals)
    # the normals stay when none are given
    sc.set_mesh_vertices("cloth", S.wave(pos, phase=1.0))
    ds.update()
    _check_records(ds, sc, "normals kept", names=("cloth",))
    assert _util.same_words(_render(sc), _util.oracle_render(sc, _tracer(), W, H, flags=FLAGS)[0]), "normals kept"
    sc.close()


# ---- 6. many workgroups --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("walker", ["stream", "no_stream"])
def test_a_mesh_of_many_workgroups_is_assembled(walker, monkeypatch):
    """The terrain: 30 625 vertices and 60 552 triangles - 120 and 237 workgroups.  Deformed twice and back: per state the device's
    records are the host's, film and hits a fresh scene's."""
    monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    if walker == "no_stream":
        monkeypatch.setenv("SPT_NO_STREAM", "1")
    sc, host = _load("big"), _load("big")
    rays = _util.random_rays(sc, 4096, seed=11, spread=2.0)

    def answers(scene):
        ds = scene.device_scene(0)
        return _render(scene), ds.trace_closest(rays), ds.trace_any(rays)

    def check(got, want, what):
        assert _util.same_words(got[0], want[0]), what + ": film"
        assert _same_hits(got[1], want[1]), what + ": closest hits"
        assert np.array_equal(got[2], want[2]), what + ": occlusion"

    ds = sc.device_scene(0)
    rest = sc.mesh_positions("terrain")
    assert rest.shape[0] == 175 * 175
    first = answers(sc)
    terrain = sc.instance_index("terrain")
    assert (first[1]["instance"] == terrain).sum() > 500
    states = {"ridge": S.shear(S.wave(rest, phase=0.5, amp=0.3), k=0.5), "swell": S.wave(rest, phase=2.0, amp=0.12), "rest": rest}
    for key, pos in states.items():
        sc.set_mesh_vertices("terrain", pos)
        ds.update()
        host.set_mesh_positions("terrain", pos)
        _check_records(ds, host, key, names=("terrain", "cloth"))
        got = answers(sc)
        check(got, answers(host), key + " against a fresh scene")
        host.close_device_scene(0)
        if key == "ridge":
            assert not _same_hits(got[1], first[1])
    check(got, first, "back to the file's positions")
    assert ds.render_info(4) == 3
    sc.close()
    host.close()


# ---- 7. bytes ------------------------------------------------------------------------------------------------------------------

def test_a_vertex_deformation_copies_vertices_only(monkeypatch):
    """Next to the 60 552-triangle terrain that is not named, on the large-scene path: counter 5 is at most the update's bound
    (1024 B per instance + 128 B per light + 16 KB, tests/test_gpu_scene_update.py) + 12 B (24 B with normals) per vertex of the
    named mesh + 64 B per named mesh, and below what spt_scene_deform reports for the same mesh."""
    monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc, other = _load("big"), _load("big")
    ds, ds_records = sc.device_scene(0), other.device_scene(0)
    r = _tracer()
    cfg = spt.OutputConfig(W, H)
    r.render_shard(sc, cfg)
    n_inst, n_lights = sc.desc.n_instances, sc.desc.n_lights
    update_bound = 1024 * n_inst + 128 * n_lights + 16384
    for name, with_normals in (("cloth", False), ("cube", True)):
        pos = S.DEFORMED[name](_rest(name))
        nrm = sc.mesh_topology(name)["normals"][::-1].copy() if with_normals else None
        sc.set_mesh_vertices(name, pos, nrm)
        ds.update()
        copied = ds.render_info(5)
        other.set_mesh_positions(name, pos, nrm)
        ds_records.update()
        by_records = ds_records.render_info(5)
        print("bytes copied by the deformation of %s: %d by vertices, %d by records" % (name, copied, by_records))
        assert 0 < copied <= update_bound + (24 if with_normals else 12) * len(pos) + 64
        assert copied < by_records
    assert ds.render_info(4) == 2
    _check_records(ds, other, "after both")
    assert _util.same_words(r.render_shard(sc, cfg), r.render_shard(other, cfg))
    sc.close()
    other.close()


# ---- 8. degenerate shapes ------------------------------------------------------------------------------------------------------

def _shapes():
    cloth, fan = _rest("cloth"), _rest("tri5")
    corner = cloth.min(axis=0)
    return {
        "scaled_far": {"cloth": ((cloth - corner) * f32(100.0) + corner + np.array([4000.0, -150.0, -9000.0], dtype=f32)).astype(f32)},
        "flat": {"cloth": (cloth * np.array([1.0, 0.0, 1.0], dtype=f32) + np.array([0.0, 0.125, 0.0], dtype=f32)).astype(f32)},
        "point": {"tri5": np.tile(np.array([[0.25, 0.5, -0.125]], dtype=f32), (len(fan), 1))},      # NaN frames
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
    _by_vertices(sc, edits)
    ds.update()
    after = _answers(sc)
    fresh, want = _fresh(edits)
    _check_answers(after, want, shape + " against a fresh scene")
    _check_records(ds, fresh, shape)
    if shape == "point":
        m = fresh.mesh_index("tri5")
        assert np.isnan(ds.read_triangles(m)[1]["t"]).all(), "a collapsed fan with distinct uvs: every frame is NaN"
    fresh.close()
    _check_answers(after, _oracle(sc), shape)
    sc.close()


# ---- 9. refusals and atomicity -------------------------------------------------------------------------------------------------

def _register(ds, sc, name):
    t = sc.mesh_topology(name)
    ds.set_topology(t["mesh"], t["indices"], t["face_of_tri"], t["uv"], t["normals"])
    return t


@pytest.mark.parametrize("lds", ["default", "no_lds_geo"])
def test_refusals_leave_the_scene_as_it_was(lds, monkeypatch):
    if lds == "no_lds_geo":
        monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc, edited = _load(), _load()
    ds = sc.device_scene(0)
    first = _answers(sc)
    _check_answers(first, _first("uniform", "bvh"), "as loaded")
    new = S.wave(_rest("cloth"))
    edited.set_mesh_positions("cloth", new)
    inst, lights, tlas = edited.array("instances"), edited.array("lights"), edited.array("tlas_nodes")
    m, cube = sc.mesh_index("cloth"), sc.mesh_index("cube")
    lib = spt.hip_lib()

    def unchanged(what):
        _check_answers(_answers(sc), first, what + " changed the scene")
        _check_records(ds, _ref_scene(), what)

    def refused(status, vertices, instances=inst):
        with pytest.raises(spt.SptError) as e:
            ds.update_arrays(instances, lights, tlas_nodes=tlas, vertices=vertices)
        assert e.value.status == status, str(e.value)
        unchanged("a refused deformation")

    refused(INVALID_ARG, {m: (new, None)})                                         # no registration yet
    # registrations that are refused: an index out of range, a face_of_tri that is no permutation, values that are not finite
    t = sc.mesh_topology("cloth")
    for key, bad in (("indices", np.where(t["indices"] == 5, len(new), t["indices"])), ("face_of_tri", np.where(t["face_of_tri"] == 3, 4, t["face_of_tri"])),
                     ("face_of_tri", t["face_of_tri"] + 1), ("uv", np.where(t["uv"] == t["uv"][7], np.nan, t["uv"])),
                     ("normals", np.where(np.arange(len(new))[:, None] == 9, np.inf, t["normals"])), ("tri_count", None)):
        args = dict(t, **{key: bad})
        if key == "tri_count":
            args.update(indices=t["indices"][:-1], face_of_tri=None)               # a triangle fewer than the mesh has
        with pytest.raises(spt.SptError) as e:
            ds.set_topology(m, args["indices"], args["face_of_tri"], args["uv"], args["normals"])
        assert e.value.status == INVALID_ARG, (key, str(e.value))
        refused(INVALID_ARG, {m: (new, None)})                                     # ... and registers nothing
    with pytest.raises(spt.SptError) as e:
        ds.set_topology(sc.desc.n_meshes, t["indices"], t["face_of_tri"], t["uv"], t["normals"])
    assert e.value.status == INVALID_ARG
    _register(ds, sc, "cloth")
    refused(INVALID_ARG, {cube: (S.shear(_rest("cube")), None)})                   # another mesh: still unregistered
    refused(INVALID_ARG, {sc.desc.n_meshes: (new, None)})                          # mesh index out of range
    refused(INVALID_ARG, {m: (new[:-1], None)})                                    # a wrong vertex count
    refused(INVALID_ARG, {m: (np.concatenate([new, new[:1]]), None)})
    for value in (np.nan, np.inf, -np.inf):                                        # a value that is not finite
        bad = new.copy()
        bad[len(bad) // 2, 1] = value
        refused(INVALID_ARG, {m: (bad, None)})
        refused(INVALID_ARG, {m: (new, bad)})
    refused(INVALID_ARG, {m: (new, None)}, instances=inst[:-1])                    # `u` gets the update's checks
    # a mesh named twice, null arrays: through the raw entry point
    d = edited.desc
    u = spt.SceneUpdateDesc(size=C.sizeof(spt.SceneUpdateDesc), flags=0, n_tlas_nodes=d.n_tlas_nodes, tlas_nodes=d.tlas_nodes, n_instances=d.n_instances,
                            instances=d.instances, n_lights=d.n_lights, lights=d.lights, light_alias=d.light_alias)
    verts = (spt.MeshVertices * 2)()
    for v in verts:
        v.mesh, v.n_vertices = m, len(new)
        v.positions = C.cast(new.ctypes.data, C.POINTER(C.c_float))
    assert lib.spt_scene_deform_vertices(ds._h, C.byref(u), 2, verts) == INVALID_ARG
    assert lib.spt_scene_deform_vertices(ds._h, C.byref(u), 1, None) == INVALID_ARG
    assert lib.spt_scene_deform_vertices(ds._h, None, 1, verts) == INVALID_ARG
    assert lib.spt_scene_deform_vertices(None, C.byref(u), 1, verts) == INVALID_ARG
    verts[0].positions = None
    assert lib.spt_scene_deform_vertices(ds._h, C.byref(u), 1, verts) == INVALID_ARG
    verts[0].positions = C.cast(new.ctypes.data, C.POINTER(C.c_float))
    u.flags = 1
    assert lib.spt_scene_deform_vertices(ds._h, C.byref(u), 1, verts) == INVALID_ARG
    u.flags = 0
    n_tris = sc.desc.n_tris
    assert lib.spt_scene_read_triangles(ds._h, n_tris, 1, None, None) == INVALID_ARG      # range errors
    assert lib.spt_scene_read_triangles(ds._h, 1, n_tris, None, None) == INVALID_ARG
    assert lib.spt_scene_read_triangles(None, 0, 1, None, None) == INVALID_ARG
    assert lib.spt_scene_read_triangles(ds._h, 0, n_tris, None, None) == 0
    with pytest.raises(ValueError):
        ds.update_arrays(inst, lights, tlas_nodes=tlas, meshes={}, vertices={m: (new, None)})
    unchanged("a refused deformation")
    with _tracer().progressive(sc, spt.OutputConfig(W, H)) as pf:                  # a live film refuses the deformation, not a registration
        pf.render(1)
        assert lib.spt_scene_deform_vertices(ds._h, C.byref(u), 1, verts) == INVALID_ARG
        _register(ds, sc, "cloth")
        assert _util.same_words(pf.render(SPP - 1).mean(), first[0])
    assert ds.render_info(4) == 0
    assert lib.spt_scene_deform_vertices(ds._h, C.byref(u), 1, verts) == 0         # the film is gone: the same call goes through
    _check_answers(_answers(sc), _answers(edited), "the deformation that went through")
    _check_records(ds, edited, "the deformation that went through")
    assert lib.spt_scene_deform_vertices(ds._h, C.byref(u), 0, None) == 0          # no meshes: an update
    assert ds.render_info(4) == 2
    _check_answers(_answers(sc), _answers(edited), "a deformation without meshes")
    sc.close()
    edited.close()


def test_a_scene_on_the_callers_trees_refuses(monkeypatch):
    monkeypatch.setenv("SPT_REFERENCE_BVH", "1")
    sc = _load()
    ds = sc.device_scene(0)
    first = _answers(sc)
    t = sc.mesh_topology("cloth")
    with pytest.raises(spt.SptError) as e:
        ds.set_topology(t["mesh"], t["indices"], t["face_of_tri"], t["uv"], t["normals"])
    assert e.value.status == UNSUPPORTED, str(e.value)
    sc.set_mesh_vertices("cloth", S.wave(_rest("cloth")))
    with pytest.raises(spt.SptError) as e:
        ds.update()
    assert e.value.status == UNSUPPORTED, str(e.value)
    _check_answers(_answers(sc), first, "the refused deformation changed the scene")
    _check_records(ds, _ref_scene(), "the refused deformation")
    assert ds.render_info(4) == 0
    sc.close()


def _soup(sc, name):
    """The mesh as a triangle soup: every triangle of the descriptor's range with three vertices of its own (face k = triangle k)."""
    m = sc.mesh_index(name)
    mesh = sc.array("meshes")[m]
    a, b = int(mesh["tri_first"]), int(mesh["tri_first"]) + int(mesh["tri_count"])
    tp, ta = sc.array("tri_pos")[a:b], sc.array("tri_attr")[a:b]
    pos = np.stack([tp["p0"], tp["p1"], tp["p2"]], axis=1).reshape(-1, 3).astype(f32)
    return m, np.arange(3 * (b - a), dtype=np.uint32).reshape(-1, 3), pos, ta["uv"].reshape(-1, 2).copy(), ta["n"].reshape(-1, 3).copy()


@pytest.mark.parametrize("lds", ["default", "no_lds_geo"])
def test_a_registration_replaced_by_another_is_honoured(lds, monkeypatch):
    """The cube registered as the loader has it, then again as a soup of 12 unshared triangles (36 vertices, face_of_tri NULL): the
    soup's vertices move the triangles apart, which the shared vertices could not; the records keep the loader's normals and uvs,
    and the tangents of a soup are each face's own."""
    if lds == "no_lds_geo":
        monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc = _load()
    ds = sc.device_scene(0)
    _answers(sc)
    _register(ds, sc, "cube")
    m, idx, pos, uv, nrm = _soup(sc, "cube")
    ds.set_topology(m, idx, None, uv, nrm)
    inst, lights = sc.array("instances"), sc.array("lights")
    with pytest.raises(spt.SptError) as e:
        ds.update_arrays(inst, lights, vertices={m: (_rest("cube"), None)})        # the first registration's count
    assert e.value.status == INVALID_ARG
    tri = pos.reshape(-1, 3, 3)
    centre = tri.mean(axis=1, keepdims=True)
    apart = (centre + (tri - centre) * f32(0.6)).astype(f32)
    ds.update_arrays(inst, lights, vertices={m: (apart.reshape(-1, 3), None)})
    got_pos, got_attr = ds.read_triangles(m)
    assert np.array_equal(np.stack([got_pos["p0"], got_pos["p1"], got_pos["p2"]], axis=1), apart)
    want_attr = sc.array("tri_attr")[ds._mesh_ranges[m][0]:ds._mesh_ranges[m][0] + len(apart)]
    assert np.array_equal(got_attr["n"], want_attr["n"]) and np.array_equal(got_attr["uv"], want_attr["uv"])
    assert np.array_equal(got_attr["t"][:, 0], got_attr["t"][:, 1]) and np.array_equal(got_attr["t"][:, 0], got_attr["t"][:, 2])
    assert np.isfinite(got_attr["t"]).all()
    # the scene behaves like one created from these records
    other = _load()
    other.device_scene(0).update_arrays(inst, lights, meshes={m: (got_pos, got_attr)})
    _check_answers(_answers(sc), _answers(other), "the soup against the same records by spt_scene_deform")
    sc.close()
    other.close()


def test_lds_scene_that_outgrows_lds_refuses():
    """The 308-triangle case of tests/test_gpu_scene_deform.py through vertices: the cloth as a soup, every triangle shrunk about its
    centroid to 288 islands, which the SAH builder separates down to one triangle per leaf."""
    sc = _load()
    ds = sc.device_scene(0)
    first = _answers(sc)
    m, idx, pos, uv, nrm = _soup(sc, "cloth")
    ds.set_topology(m, idx, None, uv, nrm)
    tri = pos.reshape(-1, 3, 3)
    centre = tri.mean(axis=1, keepdims=True)
    shrunk = (centre + (tri - centre) * f32(0.05)).astype(f32).reshape(-1, 3)
    with pytest.raises(spt.SptError) as e:
        ds.update_arrays(sc.array("instances"), sc.array("lights"), vertices={m: (shrunk, None)})
    assert e.value.status == UNSUPPORTED and "recreate the scene" in str(e.value), str(e.value)
    _check_answers(_answers(sc), first, "the refused deformation changed the scene")
    _check_records(ds, _ref_scene(), "the refused deformation")
    assert ds.render_info(4) == 0
    sc.close()


# ---- 10. ordering --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lds", ["default", "no_lds_geo"])
def test_async_frames_around_a_vertex_deformation(lds, monkeypatch):
    if lds == "no_lds_geo":
        monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc, host = _load(), _load()          # `host`: the same edits by positions, for the fresh scenes
    ds = sc.device_scene(0)
    r = _tracer()
    cfg = spt.OutputConfig(W, H)
    film_first = _first("uniform", "bvh")[0]
    pinned = ds.film_buffer(2 * H, W)
    pinned[:] = np.nan
    buf1, buf2 = pinned[:H], pinned[H:]
    r.render_shard(sc, cfg, film=buf1, wait=False)
    edits = {name: fn(_rest(name)) for name, fn in S.DEFORMED.items()}
    _by_vertices(sc, edits)
    ds.update()                                   # no wait in between
    r.render_shard(sc, cfg, film=buf2, wait=False)
    r.wait(sc)
    assert _util.same_words(buf1, film_first)
    assert _util.same_words(buf2, _util.oracle_render(sc, r, W, H, flags=FLAGS)[0])
    # a burst: deformation + frame, four times over, one wait at the end
    bufs = ds.film_buffer(4 * H, W)
    want = []
    _by_positions(host, edits)
    for k in range(4):
        edit = {"cloth": S.wave(_rest("cloth"), phase=0.7 * k), "cube": S.shear(_rest("cube"), k=0.1 * k)}
        _by_vertices(sc, edit)
        ds.update()
        r.render_shard(sc, cfg, film=bufs[k * H:(k + 1) * H], wait=False)
        _by_positions(host, edit)
        want.append(_render(host))                # a scene freshly created from the state of frame k
        host.close_device_scene(0)
    r.wait(sc)
    for k in range(4):
        assert _util.same_words(bufs[k * H:(k + 1) * H], want[k]), k
    assert not _util.same_words(want[0], want[1])
    _check_records(ds, host, "after the burst")
    sc.close()
    host.close()


# ---- 11. Bezier forwarding -----------------------------------------------------------------------------------------------------

def test_bezier_scene_forwards_the_three_calls(tmp_path):
    """t_bezier-like content with one trimesh: the scene lives in the library with the Bezier primitive, and the registration, the
    deformation and the read-back are passed on.  (NOT covered, as in tests/test_gpu_scene_deform.py: the refusal "the Bezier
    library does not export the symbol".)"""
    with open(os.path.join(_util.SCENES, "t_bezier.json")) as f:
        doc = json.load(f)
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
    ds = sc.device_scene(0)
    _check_records(ds, sc, "as loaded", names=("cloth",))
    pos = S.wave(sc.mesh_positions("cloth"), amp=0.5)
    sc.set_mesh_vertices("cloth", pos)
    edited.set_mesh_positions("cloth", pos)
    ds.update()
    assert ds.render_info(4) == 1
    _check_records(ds, edited, "deformed", names=("cloth",))
    got = r.render_shard(sc, cfg).copy()
    assert _util.same_words(got, r.render_shard(edited, cfg))
    assert not _util.same_words(got, before)
    sc.close()
    edited.close()


# ---- 12. mixed edits -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lds", ["default", "no_lds_geo"])
def test_edits_of_both_kinds_before_one_update(lds, monkeypatch):
    if lds == "no_lds_geo":
        monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc = _load()
    ds = sc.device_scene(0)
    _answers(sc)
    edits = {"cloth": S.wave(_rest("cloth")), "cube": S.shear(_rest("cube"))}
    sc.set_mesh_vertices("cloth", edits["cloth"])
    ds.update()                                             # by vertices: the cloth is registered
    sc.set_mesh_vertices("cloth", S.wave(_rest("cloth"), phase=1.0))
    sc.set_mesh_positions("cube", edits["cube"])            # one by records,
    sc.set_mesh_vertices("cloth", edits["cloth"])           # one by vertices: the update goes by records
    ds.update()
    assert ds.render_info(4) == 2
    got = _answers(sc)
    fresh, want = _fresh(edits)
    _check_answers(got, want, "the mix against a fresh scene")
    _check_records(ds, fresh, "the mix")
    fresh.close()
    sc.close_device_scene(0)                                # a second device scene of the same Scene, created after the edits
    _check_answers(_answers(sc), want, "a device scene created after the edits")
    # ... and by vertices again, with normals that a records edit brought after the registration
    ds = sc.device_scene(0)
    sc.set_mesh_vertices("cloth", S.wave(_rest("cloth"), phase=2.0))
    ds.update()
    nrm = np.tile(np.array([[0.6, 0.8, 0.0]], dtype=f32), (len(_rest("cloth")), 1))
    sc.set_mesh_positions("cloth", edits["cloth"], nrm)
    ds.update()
    sc.set_mesh_vertices("cloth", _rest("cloth"))
    ds.update()
    _check_records(ds, sc, "vertices after normals by records")
    assert np.array_equal(ds.read_triangles(sc.mesh_index("cloth"))[1]["n"][0, 0], nrm[0])
    sc.close()

"""Shadow and extension rays against per-origin-triangle candidate sets (k_shade<0, ., kFused, ..., OriginCand>, origin.h): the film
with the path on, the film with SPT_NO_ORIGIN_CANDIDATES=1 (the two tree walks) and the exhaustive oracle are the same words.

64 x 48 and 50 x 37 pixels @ 16 spp in two passes of 8, max_depth 4 (bounce 0, bounce 1 and the tail loop all run).  The scenes are
written into a directory of the test's: OBJ meshes, one per instance (the path wants every mesh used once); the scene writer is the
one of test_gpu_block_candidates.py."""
import functools
import json
import os

import numpy as np
import pytest

import _scene_update_scenes as S
import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32
SIZES = [(64, 48), (50, 37)]
SPP, PASS, DEPTH, SEED = 16, 8, 4, 5
SWITCH = "SPT_NO_ORIGIN_CANDIDATES"

TRIANGLE_OBJ = "v -1 -1 0\nv 1 -1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\n"


def _icosahedron_obj():
    """20 triangles with smooth normals: a vertex's normal is its direction from the centre."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]])
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    lines = ["v %.9g %.9g %.9g" % tuple(x) for x in v] + ["vt 0 0"] + ["vn %.9g %.9g %.9g" % tuple(x) for x in v]
    lines += ["f %d/1/%d %d/1/%d %d/1/%d" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1) for a, b, c in f]
    return "\n".join(lines) + "\n"


def _scene_dict(camera, instances, bulb=(0.5, 3.0, 6.0), aggregate="group"):
    """instances: (primitive kind, transform dict) - every instance gets a primitive (and an OBJ file) of its own."""
    d = {"cameras": [dict(camera, type="perspective", name="main")],
         "textures": [{"type": "scalar", "name": "white", "value": [0.8, 0.8, 0.8]}],
         "materials": [{"type": "lambert", "name": "m", "albedo": "white"}],
         "mediums": [], "surfaces": [], "primitives": [], "instances": [],
         "lights": [{"type": "directional", "name": "sun", "direction": [-1.0, -1.0, -1.0], "strength": [5.0, 5.0, 5.0]},
                    {"type": "point", "name": "bulb", "position": list(bulb), "strength": [30.0, 30.0, 30.0]}],
         "aggregate": aggregate}
    for k, (kind, xf) in enumerate(instances):
        d["primitives"].append({"type": "trimesh", "name": "p%d" % k, "obj_file": "models/%s_%d.obj" % (kind, k)})
        d["instances"].append(dict(xf, name="i%d" % k, primitive="p%d" % k, material="m"))
    return d


CAM = {"eye": [0.0, 0.0, 7.0], "forward": [0.0, 0.0, -1.0], "up": [0.0, 1.0, 0.0], "fov": 45.0}
ROT = {"rotate": [0.0, 60.0, 0.0]}


def _grid(n_cubes, extra):
    """n_cubes small cubes in a row of rows plus `extra` (kind, transform) instances."""
    inst = []
    for k in range(n_cubes):
        inst.append(("cube", {"scale": [0.45, 0.45, 0.45], "rotate": [10.0 * k, 25.0 + 15.0 * k, 0.0],
                              "translate": [-2.0 + 1.0 * (k % 5), -0.8 + 1.6 * (k // 5), -0.5 * (k % 2)]}))
    return inst + extra


PLANES = [("plane", {"scale": [3.0, 1.0, 3.0], "translate": [0.0, -1.4, 0.0]}),
          ("plane", {"scale": [2.0, 1.0, 2.0], "rotate": [90.0, 0.0, 0.0], "translate": [0.0, 0.0, -2.5]})]
SCENES = {
    "cube": (CAM, [("cube", ROT)]),
    "eye_inside": ({"eye": [0.2, 0.1, 0.3], "forward": [0.3, -0.1, -1.0], "up": [0.0, 1.0, 0.0], "fov": 70.0}, [("cube", ROT)], (0.3, 0.4, -0.2)),   # the bulb inside too
    # two cubes that share the plane x = 0 in world space: their touching faces coincide
    "coincident": (CAM, [("cube", {"translate": [-1.0, 0.0, 0.0]}), ("cube", {"translate": [1.0, 0.0, 0.0]})]),
    "scaled_rotated": (CAM, [("cube", {"scale": [1.6, 0.5, 0.9], "rotate": [20.0, 40.0, 65.0], "translate": [0.3, -0.2, 0.5]})]),
    # planes under and behind cubes: inter-reflection, and the bulb's light is occluded
    "tris64": (CAM, _grid(5, PLANES)),
    "tris65": (CAM, _grid(5, PLANES + [("triangle", {"scale": [0.6, 0.6, 0.6], "translate": [0.0, 1.6, 1.0]})])),
    "smooth": (CAM, [("icosahedron", {"scale": [1.5, 1.5, 1.5], "rotate": [10.0, 20.0, 0.0]}), ("plane", {"scale": [3.0, 1.0, 3.0], "translate": [0.0, -1.6, 0.0]})]),
}
AGGREGATES = ["group", "bvh"]
PATH_OFF = {"tris65"}     # 65 triangles: the gate is off

_DIR = None


@pytest.fixture(scope="module", autouse=True)
def _files(tmp_path_factory):
    global _DIR
    d = str(tmp_path_factory.mktemp("origin_candidates"))
    os.makedirs(os.path.join(d, "models"))
    objs = {"cube": S.CUBE_OBJ, "plane": S.PLANE_OBJ, "triangle": TRIANGLE_OBJ, "icosahedron": _icosahedron_obj()}
    for name, (cam, inst, *rest) in SCENES.items():
        for k, (kind, _) in enumerate(inst):
            with open(os.path.join(d, "models", "%s_%d.obj" % (kind, k)), "w") as f:
                f.write(objs[kind])
        for agg in AGGREGATES:
            with open(os.path.join(d, "%s_%s.json" % (name, agg)), "w") as f:
                json.dump(_scene_dict(cam, inst, *rest, aggregate=agg), f)
    _DIR = d
    _util.ensure_cpu_build()
    yield d
    _oracle.cache_clear()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in (SWITCH, "SPT_NO_FUSED", "SPT_NO_EYE_BLOB", "SPT_NO_TAIL_LOOP"):
        monkeypatch.delenv(name, raising=False)


def _load(name, agg="group"):
    return spt.load_scene(os.path.join(_DIR, "%s_%s.json" % (name, agg)))


def _tracer():
    return spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=SPP, seed=SEED)


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h):
    """The exhaustive oracle's film: it tests every triangle, so one film serves both aggregates."""
    sc = _load(name)
    film, _ = _util.oracle_render(sc, _tracer(), w, h, flags=_util.ORACLE_EXHAUSTIVE)
    sc.close()
    film.setflags(write=False)
    return film


def _render(sc, w, h, monkeypatch, on, **kw):
    if on:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, "1")
    r = _tracer()
    film = r.render_shard(sc, spt.OutputConfig(w, h), samples_per_pass=PASS, **kw).copy()
    return film, r.last_stats


def _table(sc, monkeypatch, on=True):
    if on:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, "1")
    return sc.device_scene(0).origin_candidates()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("agg", AGGREGATES)
@pytest.mark.parametrize("name", list(SCENES))
def test_path_walk_and_oracle_agree(name, agg, size, monkeypatch):
    w, h = size
    sc = _load(name, agg)
    n_tris = len(sc.array("tri_pos"))
    assert n_tris == {"tris64": 64, "tris65": 65}.get(name, n_tris)
    want = _oracle(name, w, h)
    on, st_on = _render(sc, w, h, monkeypatch, True)
    off, st_off = _render(sc, w, h, monkeypatch, False)
    assert float(want.max()) > 0.01, "the camera sees nothing"
    assert _util.same_words(on, off), "candidate sets against the two walks"
    assert _util.same_words(on, want), "candidate sets against the exhaustive oracle"
    for field in ("samples", "segments_closest", "segments_shadow", "primary_hits", "path_vertices", "shadow_first", "vertices_second"):
        assert getattr(st_on, field) == getattr(st_off, field), field
    assert st_on.segments_shadow > 0 and st_on.vertices_second >= 0
    # the query says which kernels ran
    table = _table(sc, monkeypatch)
    assert _table(sc, monkeypatch, on=False) is None
    if name in PATH_OFF:
        assert table is None
    else:
        words, info = table
        assert words.shape == (n_tris, 4) and info["reach"] > 7.5, "the path serves this camera"
        assert ((words >> np.uint64(n_tris)) == 0).all() if n_tris < 64 else True
        if name == "smooth":   # the icosahedron's rows keep everything; the plane under it is flat: nothing of the body is below it
            full = np.uint64((1 << n_tris) - 1)
            assert (words[:20] == full).all() and (words[20:, 1] != full).all()
        if name in ("cube", "eye_inside"):
            assert info["tight"] and (words[:, 2] == 0).all()
    sc.close()


def test_some_union_occludes(monkeypatch):
    """tris64 has real occlusion and inter-reflection: paths go on after bounce 0, and light samples are shadowed."""
    sc = _load("tris64")
    film, st = _render(sc, 64, 48, monkeypatch, True)
    words, _ = _table(sc, monkeypatch)
    assert st.vertices_second > 0, "no extension ray hit anything"
    assert (words != 0).any()
    sc.close()


def test_update_then_deform(monkeypatch):
    """Render, move an instance (spt_scene_update), render, deform a mesh (spt_scene_deform), render: each film equals the switch-off
    film and the oracle's of the same state, and the table follows the scene."""
    w, h = 64, 48
    sc = _load("coincident")
    ds = sc.device_scene(0)
    first, _ = _render(sc, w, h, monkeypatch, True)
    assert _util.same_words(first, _oracle("coincident", w, h))
    words0, _ = _table(sc, monkeypatch)
    # 1. rotate and translate the second cube: its face no longer coincides with the first cube's
    fwd = S.fwd_by_name(sc, ["i1"])["i1"]
    c, s = np.cos(0.4), np.sin(0.4)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    fwd[0:9] = (rot @ fwd[0:9].reshape(3, 3).T.astype(np.float64)).T.reshape(9).astype(f32)
    fwd[9:12] += np.array([0.6, 0.3, -0.4], dtype=f32)
    sc.set_transforms({"i1": fwd})
    ds.update()
    films = [first]
    tables = [words0]
    for step in ("update", "deform"):
        if step == "deform":   # 2. the first cube squeezed along x about its centre: axis-aligned faces, the file's normals still fit
            pos = sc.mesh_positions("p0").copy()
            pos[:, 0] *= f32(0.5)
            sc.set_mesh_positions("p0", pos)
            ds.update()
        want, _ = _util.oracle_render(sc, _tracer(), w, h, flags=_util.ORACLE_EXHAUSTIVE)
        on, _ = _render(sc, w, h, monkeypatch, True)
        off, _ = _render(sc, w, h, monkeypatch, False)
        assert not _util.same_words(on, films[-1]), step + ": the scene did not change"
        assert _util.same_words(on, off), step + ": a stale table?"
        assert _util.same_words(on, want), step
        words, _ = _table(sc, monkeypatch)
        assert words.shape == words0.shape and not np.array_equal(words, tables[-1]), step + ": the table did not follow"
        films.append(on)
        tables.append(words)
    # before the update the touching faces hid each other from tight rays; afterwards the second cube reaches over the first's face
    assert (int(tables[1][0:12, 2].max()) != 0) or (int(tables[1][12:24, 2].max()) != 0)
    sc.close()

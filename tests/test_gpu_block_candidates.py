"""Camera rays against per-block candidate masks (k_block_candidates + k_primary<..., BlockCand>): the film with the path on, the
film with SPT_NO_BLOCK_CANDIDATES=1 (the tree walk) and the exhaustive oracle are the same words.

64 x 48 and 50 x 37 pixels @ 16 spp in two passes of 8, max_depth 3.  The scenes are written into a directory of the test's: OBJ
cubes, one mesh per instance (the eye-relative copy wants every mesh used once)."""
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
SPP, PASS, DEPTH, SEED = 16, 8, 3, 5
SWITCH = "SPT_NO_BLOCK_CANDIDATES"
OTHER = spt.KERNEL_NAMES.index("other")

TRIANGLE_OBJ = "v -1 -1 0\nv 1 -1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\n"


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


SCENES = {
    "cube": (CAM, [("cube", ROT)]),
    "eye_inside": ({"eye": [0.2, 0.1, 0.3], "forward": [0.3, -0.1, -1.0], "up": [0.0, 1.0, 0.0], "fov": 70.0}, [("cube", ROT)], (0.3, 0.4, -0.2)),   # the bulb inside too
    # the eye on the plane of the face y = +1, outside the face: the face projects to a line
    "edge_on": ({"eye": [0.0, 1.0, 6.0], "forward": [0.0, 0.0, -1.0], "up": [0.0, 1.0, 0.0], "fov": 45.0}, [("cube", {"rotate": [0.0, 30.0, 0.0]})]),
    "far": ({"eye": [0.0, 0.0, 150.0], "forward": [0.001, 0.002, -1.0], "up": [0.0, 1.0, 0.0], "fov": 45.0}, [("cube", ROT)]),
    # two cubes that share the plane x = 0 in world space: their touching faces coincide
    "coincident": (CAM, [("cube", {"translate": [-1.0, 0.0, 0.0]}), ("cube", {"translate": [1.0, 0.0, 0.0]})]),
    "scaled_rotated": (CAM, [("cube", {"scale": [1.6, 0.5, 0.9], "rotate": [20.0, 40.0, 65.0], "translate": [0.3, -0.2, 0.5]})]),
    "tris64": (CAM, _grid(5, [("plane", {"scale": [3.0, 1.0, 3.0], "translate": [0.0, -1.4, 0.0]}),
                              ("plane", {"scale": [2.0, 1.0, 2.0], "rotate": [90.0, 0.0, 0.0], "translate": [0.0, 0.0, -2.5]})])),
    "tris65": (CAM, _grid(5, [("plane", {"scale": [3.0, 1.0, 3.0], "translate": [0.0, -1.4, 0.0]}),
                              ("plane", {"scale": [2.0, 1.0, 2.0], "rotate": [90.0, 0.0, 0.0], "translate": [0.0, 0.0, -2.5]}),
                              ("triangle", {"scale": [0.6, 0.6, 0.6], "translate": [0.0, 1.6, 1.0]})])),
}

_DIR = None


@pytest.fixture(scope="module", autouse=True)
def _files(tmp_path_factory):
    global _DIR
    d = str(tmp_path_factory.mktemp("block_candidates"))
    os.makedirs(os.path.join(d, "models"))
    objs = {"cube": S.CUBE_OBJ, "plane": S.PLANE_OBJ, "triangle": TRIANGLE_OBJ}
    for name, (cam, inst, *rest) in SCENES.items():
        for k, (kind, _) in enumerate(inst):
            with open(os.path.join(d, "models", "%s_%d.obj" % (kind, k)), "w") as f:
                f.write(objs[kind])
        with open(os.path.join(d, name + ".json"), "w") as f:
            json.dump(_scene_dict(cam, inst, *rest), f)
    _DIR = d
    _util.ensure_cpu_build()
    yield d
    _oracle.cache_clear()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv("SPT_NO_EYE_BLOB", raising=False)


def _load(name):
    return spt.load_scene(os.path.join(_DIR, name + ".json"))


def _tracer():
    return spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=SPP, seed=SEED)


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, shard=0, shards=1, strip=16):
    sc = _load(name)
    film, _ = _util.oracle_render(sc, _tracer(), w, h, flags=_util.ORACLE_EXHAUSTIVE, shard_index=shard, shard_count=shards, strip_rows=strip)
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


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(SCENES))
def test_path_walk_and_oracle_agree(name, size, monkeypatch):
    w, h = size
    sc = _load(name)
    n_tris = len(sc.array("tri_pos"))
    assert n_tris == {"tris64": 64, "tris65": 65}.get(name, n_tris)
    want = _oracle(name, w, h)
    on, _ = _render(sc, w, h, monkeypatch, True)
    off, _ = _render(sc, w, h, monkeypatch, False)
    assert float(want.max()) > 0.01, "the camera sees nothing"
    assert _util.same_words(on, off), "candidate masks against the tree walk"
    assert _util.same_words(on, want), "candidate masks against the exhaustive oracle"
    # which primary instance ran: the path launches k_block_candidates once per render, counted under "other" in a profiled run
    _, st_on = _render(sc, w, h, monkeypatch, True, profile=True)
    _, st_off = _render(sc, w, h, monkeypatch, False, profile=True)
    takes_path = n_tris <= 64
    assert st_on.kernel_launches[OTHER] == st_off.kernel_launches[OTHER] + (1 if takes_path else 0)
    sc.close()


@pytest.mark.parametrize("strip_rows", [2, 4])
@pytest.mark.parametrize("name", ["cube", "scaled_rotated"])
def test_shards_of_three(name, strip_rows, monkeypatch):
    w, h = 50, 37
    sc = _load(name)
    for shard in range(3):
        kw = dict(shard_index=shard, shard_count=3, strip_rows=strip_rows)
        on, _ = _render(sc, w, h, monkeypatch, True, **kw)
        off, _ = _render(sc, w, h, monkeypatch, False, **kw)
        assert _util.same_words(on, off), shard
        assert _util.same_words(on, _oracle(name, w, h, shard, 3, strip_rows)), shard
    sc.close()


def test_chunked_instance(monkeypatch):
    """Two sample chunks per tile (SPT_PRIMARY_CHUNKS=2, passes of 16): the chunked candidate instance, which large images take."""
    monkeypatch.setenv("SPT_PRIMARY_CHUNKS", "2")
    w, h = 50, 37
    sc = _load("scaled_rotated")
    r = _tracer()
    films = []
    for on in (True, False):
        if on:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, "1")
        films.append(r.render_shard(sc, spt.OutputConfig(w, h), samples_per_pass=16).copy())
    assert _util.same_words(films[0], films[1])
    assert _util.same_words(films[0], _oracle("scaled_rotated", w, h))
    sc.close()


def test_adaptive_film_increment(monkeypatch):
    """One increment after spt_film_adapt has retired some pixels: the masked candidate instance against the masked walk."""
    w, h = 64, 48
    sc = _load("cube")
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RANDOM, spp=32, seed=SEED)
    out = {}
    for on in (True, False):
        if on:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, "1")
        with r.progressive(sc, spt.OutputConfig(w, h), moments=True, samples_per_pass=PASS) as film:
            film.render(16)
            active = film.adapt(0.15, 0.0, 8)
            film.render(16)
            out[on] = (active, film.sample_counts(), film.sum(), film.sum_sq())
    active, counts = out[True][0], out[True][1]
    assert 0 < active < w * h and (counts == 16).any() and (counts == 32).any(), "the adapt retired nothing or everything"
    assert out[True][0] == out[False][0] and np.array_equal(counts, out[False][1])
    assert _util.same_words(out[True][2], out[False][2]) and _util.same_words(out[True][3], out[False][3])
    sc.close()


def test_scene_update_between_two_renders(monkeypatch):
    """The masks are made by every render: an instance moved by spt_scene_update under an unmoved camera."""
    w, h = 64, 48
    sc, moved = _load("cube"), _load("cube")
    before, _ = _render(sc, w, h, monkeypatch, True)
    assert _util.same_words(before, _oracle("cube", w, h))
    fwd = S.fwd_by_name(sc, ["i0"])["i0"]
    fwd[0:9] = (fwd[0:9].reshape(3, 3) * np.array([[0.7], [1.2], [0.6]], dtype=f32)).reshape(9)      # the columns scaled apart
    fwd[9:12] += np.array([1.1, 0.4, -0.5], dtype=f32)
    for s in (sc, moved):
        s.set_transforms({"i0": fwd})
    sc.device_scene(0).update()
    want, _ = _util.oracle_render(sc, _tracer(), w, h, flags=_util.ORACLE_EXHAUSTIVE)
    after, _ = _render(sc, w, h, monkeypatch, True)
    assert not _util.same_words(after, before)
    assert _util.same_words(after, want), "a stale mask?"
    assert _util.same_words(after, _render(sc, w, h, monkeypatch, False)[0])
    assert _util.same_words(after, _render(moved, w, h, monkeypatch, True)[0])
    sc.close()
    moved.close()

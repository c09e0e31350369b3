"""spt_scene_update (DeviceScene.update / update_arrays): a scene after an update behaves, word for word, like a scene freshly
created from the edited descriptor.

The scene is the one of tests/test_scene_update_host.py (tests/_scene_update_scenes.py): two files A and B that differ in instance
transforms only.  48 x 32 pixels @ 4 spp, max_depth 4 unless a test says otherwise.  Every comparison is _util.same_words against
the oracle on the descriptor of that moment (under device_oracle_flags()) and / or against a fresh device scene."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import _radiance_ref
import _scene_update_scenes as S
import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32
W, H, SPP, DEPTH, SEED = 48, 32, 4, 4, 7
NAMES = sorted(S.TRANSFORMS_A)
CLI = os.path.join(spt.LIB_DIR, "spt")
INVALID_ARG, UNSUPPORTED = 1, 4


def _tracer(spp=SPP, seed=SEED):
    return spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=spp, seed=seed)


_DIR = None


@pytest.fixture(scope="module", autouse=True)
def _files(tmp_path_factory):
    """A and B under both aggregates and the renderer file, written once."""
    global _DIR
    d = str(tmp_path_factory.mktemp("scene_update"))
    for agg in ("bvh", "group"):
        S.write_scene(d, "a_%s.json" % agg, S.TRANSFORMS_A, aggregate=agg)
        S.write_scene(d, "b_%s.json" % agg, S.TRANSFORMS_B, aggregate=agg)
    S.write_renderer(d, SPP, DEPTH)
    _DIR = d
    yield d
    for cached in (_ref_scene, _fwd, _rays, _plan_rays, _oracle):
        cached.cache_clear()


def _path(which, agg="bvh"):
    return os.path.join(_DIR, "%s_%s.json" % (which, agg))


def _load(which, agg="bvh"):
    """A host scene of the test's own: tests move its instances."""
    _util.ensure_cpu_build()
    return spt.load_scene(_path(which, agg))


@functools.lru_cache(maxsize=None)
def _ref_scene(which, agg):
    return _load(which, agg)      # never edited


@functools.lru_cache(maxsize=None)
def _fwd(which, agg="bvh"):
    return S.fwd_by_name(_ref_scene(which, agg), NAMES)


@functools.lru_cache(maxsize=None)
def _rays():
    rays = _util.random_rays(_ref_scene("a", "bvh"), 4096, seed=3, spread=3.0)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def _plan_rays():
    rays = _radiance_ref.plan_rays(spt, _ref_scene("a", "bvh"), _tracer(), W, H, 0, SPP).reshape(-1)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def _oracle(which, agg, reference_bvh):
    """film, closest hits, occlusion and the plan's samples of the file `which`, once per oracle configuration; read-only."""
    flags = _util.ORACLE_DEVICE if reference_bvh else _util.ORACLE_EXHAUSTIVE
    sc = _ref_scene(which, agg)
    film, _ = _util.oracle_render(sc, _tracer(), W, H, flags=flags)
    closest = _util.oracle_trace_closest(sc, _rays(), flags)
    occluded = _util.oracle_trace_any(sc, _rays(), flags)
    samples = _util.oracle_render_samples(sc, _tracer(), W, H, 0, SPP, flags=flags).reshape(-1, 3)
    for a in (film, closest, occluded, samples):
        a.setflags(write=False)
    return film, closest, occluded, samples


def _render(scene, spp=SPP, w=W, h=H):
    return _tracer(spp).render_shard(scene, spt.OutputConfig(w, h)).copy()


def _same_hits(a, b):
    return all(_util.same_words(np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])) for f in a.dtype.names)


def _answers(scene):
    """Everything the parity test compares of a device scene: the film, closest hits, occlusion and the radiance of the plan's rays."""
    ds = scene.device_scene(0)
    return (_render(scene), ds.trace_closest(_rays()), ds.trace_any(_rays()), ds.radiance(_plan_rays(), max_depth=DEPTH, seed=SEED))


def _check_answers(got, want, what):
    assert _util.same_words(got[0], want[0]), what + ": film"
    assert _same_hits(got[1], want[1]), what + ": closest hits"
    assert np.array_equal(got[2], want[2]), what + ": occlusion"
    assert _util.same_words(got[3], want[3]), what + ": radiance"


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------

MODES = {
    "default": ({}, "bvh"),
    "no_lds_geo": ({"SPT_NO_LDS_GEO": "1"}, "bvh"),
    "no_lds_geo_no_stream": ({"SPT_NO_LDS_GEO": "1", "SPT_NO_STREAM": "1"}, "bvh"),
    "no_eye_blob": ({"SPT_NO_EYE_BLOB": "1"}, "bvh"),
    "group": ({}, "group"),
    "group_no_lds_geo": ({"SPT_NO_LDS_GEO": "1"}, "group"),
    "reference_bvh": ({"SPT_REFERENCE_BVH": "1"}, "bvh"),
    "reference_bvh_no_lds_geo": ({"SPT_REFERENCE_BVH": "1", "SPT_NO_LDS_GEO": "1"}, "bvh"),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_update_equals_a_fresh_scene_and_the_oracle(mode, monkeypatch):
    env, agg = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)      # (read when a device scene is made, and by an update)
    reference = "SPT_REFERENCE_BVH" in env
    sc = _load("a", agg)
    ds = sc.device_scene(0)
    first = _answers(sc)
    if not reference:       # (the caller's trees: compared with the freshly created scene only)
        _check_answers(first, _oracle("a", agg, False), "A")
        assert float(first[0].max()) > 0.05 and (first[1]["instance"] >= 0).sum() > 500
    sc.set_transforms(_fwd("b", agg))
    ds.update()
    assert ds.render_info(4) == 1
    after = _answers(sc)
    fresh_b = _load("b", agg)
    _check_answers(after, _answers(fresh_b), "B against a fresh scene")
    fresh_b.close()
    if not reference:
        _check_answers(after, _oracle("b", agg, False), "B")
    assert not _util.same_words(after[0], first[0])
    sc.set_transforms(_fwd("a", agg))
    ds.update()
    assert ds.render_info(4) == 2
    _check_answers(_answers(sc), first, "back to A")
    sc.close()


def test_eye_relative_copy_is_remade():
    """cfg2_cube.json takes k_primary through the eye-relative copy of its geometry, whose key is the eye position alone."""
    _util.ensure_cpu_build()
    path = os.path.join(_util.SCENES, "cfg2_cube.json")
    sc, moved = spt.load_scene(path), spt.load_scene(path)
    with open(path) as f:
        doc = json.load(f)
    name, cam = doc["instances"][0]["name"], None
    r = _tracer()
    cfg = spt.OutputConfig(W, H, None, cam)
    assert _util.same_words(r.render_shard(sc, cfg), _util.oracle_render(sc, r, W, H, camera=cam, flags=_util.device_oracle_flags())[0])
    fwd = S.fwd_by_name(sc, [name])[name]
    fwd[0:9] = (fwd[0:9].reshape(3, 3) * f32(0.5)).reshape(9)[[3, 4, 5, 0, 1, 2, 6, 7, 8]]      # half the size, two columns swapped
    fwd[9] += f32(0.8)
    for s in (sc, moved):
        s.set_transforms({name: fwd})
    sc.device_scene(0).update()
    want, _ = _util.oracle_render(sc, r, W, H, camera=cam, flags=_util.device_oracle_flags())
    got = r.render_shard(sc, cfg)
    assert float(want.max()) > 0.05
    assert _util.same_words(got, want)
    assert _util.same_words(got, r.render_shard(moved, cfg))
    sc.close()
    moved.close()


# ---- 2. stale caches -----------------------------------------------------------------------------------------------------------

def test_a_moved_object_under_an_unmoved_camera():
    film_a, film_b = _oracle("a", "bvh", False)[0], _oracle("b", "bvh", False)[0]
    # cube_l (red) stands in the left half in A and in the right half in B: the reddest pixels say where
    red_a, red_b = (film_a[..., 0] - film_a[..., 2]), (film_b[..., 0] - film_b[..., 2])
    assert np.unravel_index(red_a.argmax(), red_a.shape)[1] < W // 2 <= np.unravel_index(red_b.argmax(), red_b.shape)[1]
    sc = _load("a")
    ds = sc.device_scene(0)
    assert _util.same_words(_render(sc), film_a)
    assert ds.render_info(4) == 0 and ds.render_info(5) == 0
    sc.set_transforms(_fwd("b"))
    ds.update()
    assert _util.same_words(_render(sc), film_b)      # the same camera and image size: the row spans' key has not changed
    assert ds.render_info(4) == 1 and ds.render_info(5) > 0
    sc.close()


# ---- 3. ordering ---------------------------------------------------------------------------------------------------------------

def test_async_frames_around_an_update():
    film_a, film_b = _oracle("a", "bvh", False)[0], _oracle("b", "bvh", False)[0]
    sc = _load("a")
    ds = sc.device_scene(0)
    r = _tracer()
    cfg = spt.OutputConfig(W, H)
    pinned = ds.film_buffer(2 * H, W)
    pinned[:] = np.nan
    buf1, buf2 = pinned[:H], pinned[H:]
    r.render_shard(sc, cfg, film=buf1, wait=False)
    sc.set_transforms(_fwd("b"))
    ds.update()                                   # no wait in between
    r.render_shard(sc, cfg, film=buf2, wait=False)
    r.wait(sc)
    assert _util.same_words(buf1, film_a)
    assert _util.same_words(buf2, film_b)
    # and a burst: update + frame, eight times over, one wait at the end
    bufs = ds.film_buffer(8 * H, W)
    for k in range(8):
        sc.set_transforms(_fwd("a" if k % 2 else "b"))
        ds.update()
        r.render_shard(sc, cfg, film=bufs[k * H:(k + 1) * H], wait=False)
    r.wait(sc)
    for k in range(8):
        assert _util.same_words(bufs[k * H:(k + 1) * H], film_a if k % 2 else film_b), k
    sc.close()


# ---- 4. refusals and atomicity -------------------------------------------------------------------------------------------------

def _raw_update(ds, u):
    return spt.hip_lib().spt_scene_update(ds._h, C.byref(u) if u is not None else None)


def test_refusals_leave_the_scene_as_it_was():
    film_a, film_b = _oracle("a", "bvh", False)[0], _oracle("b", "bvh", False)[0]
    sc = _load("a")
    ds = sc.device_scene(0)
    assert _util.same_words(_render(sc), film_a)
    sc.set_transforms(_fwd("b"))                  # the host scene is B now; the device scene still A
    inst, lights, nodes = sc.array("instances"), sc.array("lights"), sc.array("tlas_nodes")
    shape = int(np.flatnonzero(lights["type"] == 3)[0])

    def refused(status, instances=inst, lights_=lights, **kw):
        with pytest.raises(spt.SptError) as e:
            ds.update_arrays(instances, lights_, **kw)
        assert e.value.status == status, str(e.value)
        assert _util.same_words(_render(sc), film_a), "a refused update changed the scene"

    refused(INVALID_ARG, instances=inst[:-1])                                     # wrong n_instances
    refused(INVALID_ARG, lights_=lights[:-1])                                     # wrong n_lights
    refused(INVALID_ARG, lights_=np.concatenate([lights, lights[:1]]))
    bad = inst.copy()
    bad["prim_id"][int(np.flatnonzero(inst["prim_type"] == 1)[0])] = 7            # mesh index out of range
    refused(INVALID_ARG, instances=bad)
    bad = inst.copy()
    bad["prim_id"][int(np.flatnonzero(inst["prim_type"] == 0)[0])] = 1            # sphere index out of range
    refused(INVALID_ARG, instances=bad)
    bad = lights.copy()
    bad["instance"][shape] = len(inst)                                            # light.instance out of range
    refused(INVALID_ARG, lights_=bad)
    bad = lights.copy()
    bad["instance"][shape] = (int(lights["instance"][shape]) + 1) % len(inst)     # a shape light that is not its instance's light
    refused(INVALID_ARG, lights_=bad)
    bad = inst.copy()
    bad["prim_type"][0], bad["prim_id"][0] = 2, 0                                 # a Bezier instance offered to the plain library
    refused(UNSUPPORTED, instances=bad)
    bad = nodes.copy()
    bad["a"][0], bad["b"][0] = 0, 0                                               # an inner node that is its own child
    refused(INVALID_ARG, tlas_nodes=bad)
    d = sc.desc
    u = spt.SceneUpdateDesc(size=C.sizeof(spt.SceneUpdateDesc), flags=0, n_tlas_nodes=d.n_tlas_nodes, tlas_nodes=d.tlas_nodes, n_instances=d.n_instances,
                            instances=d.instances, n_lights=d.n_lights, lights=d.lights, light_alias=d.light_alias)
    u.size -= 8                                                                   # a short size
    assert _raw_update(ds, u) == INVALID_ARG
    u.size += 8
    assert _raw_update(ds, None) == INVALID_ARG                                   # null pointers
    assert spt.hip_lib().spt_scene_update(None, C.byref(u)) == INVALID_ARG
    u.instances = None
    assert _raw_update(ds, u) == INVALID_ARG
    u.instances = d.instances
    u.flags = 1
    assert _raw_update(ds, u) == INVALID_ARG
    u.flags = 0
    assert _util.same_words(_render(sc), film_a)
    with _tracer().progressive(sc, spt.OutputConfig(W, H)) as pf:                 # a live film
        pf.render(1)
        with pytest.raises(spt.SptError) as e:
            ds.update()
        assert e.value.status == INVALID_ARG and "films first" in str(e.value)
        assert _util.same_words(pf.render(SPP - 1).mean(), film_a)
    assert ds.render_info(4) == 0
    assert _raw_update(ds, u) == 0                                                # the film is gone: the same update goes through
    assert _util.same_words(_render(sc), film_b)
    sc.close()


def test_env_light_keeps_its_type():
    _util.ensure_cpu_build()
    sc = spt.load_scene(os.path.join(_util.SCENES, "t_power_is.json"))
    ds = sc.device_scene(0)
    r = _tracer()
    cfg = spt.OutputConfig(W, H, None, "main")
    before = r.render_shard(sc, cfg).copy()
    lights = sc.array("lights")
    env = sc.desc.env_light_index
    assert env >= 0 and lights["type"][env] == 4
    bad = lights.copy()
    bad["type"][env] = 1
    with pytest.raises(spt.SptError) as e:
        ds.update_arrays(sc.array("instances"), bad)
    assert e.value.status == INVALID_ARG
    assert _util.same_words(r.render_shard(sc, cfg), before)
    ds.update()                                   # the unchanged arrays: the same film
    assert _util.same_words(r.render_shard(sc, cfg), before)
    sc.close()


# ---- 5. patches: the call is forwarded to the library with the Bezier primitive ------------------------------------------------

def test_bezier_scene_forwards_the_update():
    _util.ensure_cpu_build()
    path = os.path.join(_util.SCENES, "t_bezier.json")
    sc, edited = spt.load_scene(path), spt.load_scene(path)
    r = _tracer(spp=2)
    cfg = spt.OutputConfig(32, 24, None, "main")
    before = r.render_shard(sc, cfg).copy()
    fwd = S.fwd_by_name(sc, ["hill"])["hill"]
    fwd[9:12] += np.array([0.7, 0.3, -0.5], dtype=f32)
    for s in (sc, edited):
        s.set_transforms({"hill": fwd})
    sc.device_scene(0).update()
    assert sc.device_scene(0).render_info(4) == 1
    got = r.render_shard(sc, cfg).copy()
    assert _util.same_words(got, r.render_shard(edited, cfg))       # a scene freshly created from the edited descriptor
    assert not _util.same_words(got, before)
    sc.close()
    edited.close()


# ---- 6. bytes ------------------------------------------------------------------------------------------------------------------

def test_an_update_copies_no_geometry(tmp_path, monkeypatch):
    """One grid mesh of 4232 triangles (203 KB of tri_pos), 4 instances, 2 lights, the large-scene path: an update copies at most
    1024 B per instance + 128 B per light + 16 KB (the records as they stand: per instance 192 B record + 192 B blob copy + 96 B
    streaming entry + 4 B order + <= 2 x 64 B 2-wide TLAS nodes + <= 64 B 4-wide node + a class byte; per light 64 B + 12 B alias)."""
    n = 46
    lines = []
    for j in range(n + 1):
        for i in range(n + 1):
            x, z = i / n * 2 - 1, j / n * 2 - 1
            lines.append("v %r %r %r" % (x, float(0.15 * np.sin(3 * x) * np.cos(2 * z)), z))
    lines += ["vt 0 0", "vn 0 1 0"]
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i + 1, j * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 1
            lines += ["f %d/1/1 %d/1/1 %d/1/1" % (a, d, c), "f %d/1/1 %d/1/1 %d/1/1" % (a, c, b)]
    os.makedirs(tmp_path / "models")
    (tmp_path / "models" / "grid.obj").write_text("\n".join(lines) + "\n")

    def scene(offset):
        return {
            "cameras": [{"type": "perspective", "name": "main", "eye": [0.0, 2.5, 6.0], "forward": [0.0, -0.4, -1.0], "up": [0.0, 1.0, 0.0], "fov": 45.0}],
            "textures": [{"type": "scalar", "name": "white", "value": [0.8, 0.8, 0.8]}],
            "materials": [{"type": "lambert", "name": "m_white", "albedo": "white"}],
            "mediums": [], "surfaces": [],
            "primitives": [{"type": "trimesh", "name": "grid", "obj_file": "models/grid.obj"}],
            "instances": [{"name": "g%d" % k, "primitive": "grid", "material": "m_white", "rotate": [0.0, 20.0 * k + offset, 5.0 * k],
                           "translate": [2.2 * (k % 2) - 1.1 + 0.01 * offset, 0.4 * k - 0.5, 2.2 * (k // 2) - 1.1]} for k in range(4)],
            "lights": [{"type": "point", "name": "p0", "position": [2.0, 3.0, 2.0], "strength": [9.0, 9.0, 9.0]},
                       {"type": "point", "name": "p1", "position": [-2.0, 2.0, 3.0], "strength": [3.0, 4.0, 6.0]}],
            "light_sampler": "power_is",
        }

    paths = []
    for k, offset in enumerate((0.0, 35.0)):
        paths.append(str(tmp_path / ("grid%d.json" % k)))
        with open(paths[-1], "w") as f:
            json.dump(scene(offset), f)
    monkeypatch.setenv("SPT_NO_LDS_GEO", "1")
    sc, moved = spt.load_scene(paths[0]), spt.load_scene(paths[1])
    d = sc.desc
    assert d.n_tris >= 4096 and d.n_tris * 48 >= 196 * 1024 and d.n_instances == 4 and d.n_lights == 2
    ds = sc.device_scene(0)
    r = _tracer()
    cfg = spt.OutputConfig(W, H)
    r.render_shard(sc, cfg)
    sc.set_transforms(S.fwd_by_name(moved, ["g0", "g1", "g2", "g3"]))
    ds.update()
    copied = ds.render_info(5)
    print("bytes copied by the update:", copied)
    assert 0 < copied <= 1024 * d.n_instances + 128 * d.n_lights + 16384
    assert _util.same_words(r.render_shard(sc, cfg), _util.oracle_render(moved, r, W, H, flags=_util.device_oracle_flags())[0])
    sc.close()
    moved.close()


# ---- 7. a long-lived scene -----------------------------------------------------------------------------------------------------

def _random_fwd(rng):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(0, 2 * np.pi)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    rot = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    m = rot * rng.uniform(0.3, 0.9)
    t = rng.uniform(-1.5, 1.5, size=3) * np.array([1.0, 0.5, 1.0])
    return np.concatenate([m.T.reshape(9), t]).astype(f32)        # columns, then the translation


@pytest.mark.parametrize("seed", range(6))
def test_random_sessions_on_one_device_scene(seed):
    rng = np.random.default_rng(1000 + seed)
    w, h, spp = 24, 16, 2
    sc = _load("a", "bvh" if seed % 2 == 0 else "group")
    ds = sc.device_scene(0)
    r = _tracer(spp, seed=seed + 1)
    cfg = spt.OutputConfig(w, h)
    flags = _util.device_oracle_flags()
    movable = [n for n in NAMES if n != "floor"]
    updates = 0
    for step in range(12):
        op = rng.choice(["update", "light", "render", "trace", "film"], p=[0.3, 0.15, 0.25, 0.15, 0.15]) if step else "update"
        if op == "update":
            names = [n for n in movable if rng.uniform() < 0.5] or [movable[0]]
            sc.set_transforms({n: _random_fwd(rng) for n in names})
            ds.update()
            updates += 1
        elif op == "light":
            lights = sc.array("lights")
            light = spt.Light.from_buffer_copy(lights[int(np.flatnonzero(lights["type"] == 1)[0])].tobytes())
            light.pos[:] = [float(v) for v in rng.uniform(-3, 3, size=3) + np.array([0, 3.0, 0])]
            sc.set_light("bulb", light)
            ds.update()
            updates += 1
        elif op == "render":
            assert _util.same_words(r.render_shard(sc, cfg), _util.oracle_render(sc, r, w, h, flags=flags)[0]), (seed, step)
        elif op == "trace":
            rays = _util.random_rays(sc, 512, seed=int(rng.integers(1 << 30)), spread=3.0)
            assert _same_hits(ds.trace_closest(rays), _util.oracle_trace_closest(sc, rays, flags)), (seed, step)
            assert np.array_equal(ds.trace_any(rays), _util.oracle_trace_any(sc, rays, flags)), (seed, step)
        else:
            with r.progressive(sc, cfg) as pf:
                assert _util.same_words(pf.render(spp).mean(), _util.oracle_render(sc, r, w, h, flags=flags)[0]), (seed, step)
        assert ds.render_info(4) == updates
    assert _util.same_words(r.render_shard(sc, cfg), _util.oracle_render(sc, r, w, h, flags=flags)[0]), seed
    sc.close()


# ---- 8. CLI --------------------------------------------------------------------------------------------------------------------

def test_cli_animate_writes_the_frames_of_plain_runs(tmp_path):
    frames = [{"cube_l": S.TRANSFORMS_B["cube_l"]},
              {"cube_r": {"scale": [0.4, 0.4, 0.4], "rotate": [0.0, 70.0, 0.0], "translate": [0.9, -0.6, 1.4]}, "lamp": S.TRANSFORMS_B["lamp"]},
              {"cube_l": S.TRANSFORMS_A["cube_l"]}]
    scene = S.write_scene(tmp_path, "a.json", S.TRANSFORMS_A)
    pt = S.write_renderer(tmp_path, 2, DEPTH)
    (tmp_path / "frames.json").write_text(json.dumps({"frames": frames}))
    common = ["-r", pt, "-w", "32", "-h", "24", "--seed", "5"]
    res = subprocess.run([CLI, "-s", scene, "-o", str(tmp_path / "anim.png"), "--animate", str(tmp_path / "frames.json")] + common, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    state = {k: dict(v) for k, v in S.TRANSFORMS_A.items()}
    for k, frame in enumerate(frames):
        state.update(frame)         # instances a frame does not name keep their last transform
        one = S.write_scene(tmp_path, "frame%d.json" % k, state)
        res = subprocess.run([CLI, "-s", one, "-o", str(tmp_path / ("plain%d.png" % k))] + common, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        with open(tmp_path / ("anim_%04d.png" % k), "rb") as f, open(tmp_path / ("plain%d.png" % k), "rb") as g:
            assert f.read() == g.read(), k
    assert not (tmp_path / "anim.png").exists() and not (tmp_path / "anim_0003.png").exists()
    imgs = [spt.read_png(str(tmp_path / ("anim_%04d.png" % k))) for k in range(3)]
    assert not np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[1], imgs[2])

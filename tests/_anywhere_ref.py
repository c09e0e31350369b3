"""Rays no pinhole camera makes, and the oracle's answer for them: the batches of tests/test_gpu_radiance_anywhere.py.

Every batch is a flat PATH_RAY_DTYPE array (with RAY_AUX_DTYPE records or None) of at most about 2500 rays; its expected colours are
oracle_radiance's and its expected hits oracle_trace_closest's, under the oracle configuration the device is held to.  Nothing here
touches a device: the points the rays start from are found with the oracle too, so the batches and what they must give can be looked
at on a machine without a GPU.

  surface    bake_rays (one gather ray per point) at the mesh hits of a 48 x 36 camera grid plus, on up to 16 triangles of every mesh
             instance, the three corners, the three edge midpoints and the centroid; "t0": the same rays with t_min = 0 (self-hits
             and ties at t = 0); "x3" / "x025": the same rays with d scaled (d is taken as it is)
  world      bake_rays at WORLD points where the grid hits something that is not a mesh (patches, spheres)
  free       probe_rays, 32 per point, from 24 points: the scene's points of interest (inside a closed body, inside a glass or
             medium-bounded one), one about 10^3 scene radii away in the void, the rest random around the scene
  thin_lens, orthographic, panorama
             tests/_camera_ref.py's rays of one sample per pixel of a 48 x 36 plan (random sampler: rng_skip = 2) with their
             auxiliary records, whose origins differ from the ray's; "noaux": the same rays alone
  axes       directions with zero and -0.0 components through every mesh vertex, rays along mesh edges, rays aimed at mesh vertices
  big        probe_rays, 129 per point, from 129 points: 16 641 rays (two intake workgroups share a queue shard)
"""
import functools
import os

import numpy as np

import _bake_ref
import _camera_ref
import _radiance_ref
import _util

spt = _util.load_pkg()
f32 = np.float32

W, H, DEPTH, SEED = 48, 36, 5, 11
F32_MAX = np.finfo(f32).max
CAMERAS = {"cfg2_cube": None, "t_materials": "main", "t_medium": None, "t_textured": None, "t_pndf": "main", "t_bezier": "main"}
# points of interest for the free batch
INSIDE = {"cfg2_cube": [(0.0, 0.0, 0.0)],                                      # the closed cube: back faces only
          "t_materials": [(2.2, -0.39, -0.6), (0.0, 0.0, -0.4)],                 # the glass cube, the rough glass sphere
          "t_medium": [(1.2, 1.2, -1.2), (2.4, -0.8, 0.8)]}                      # the fog box (beside the blob), the absorbing ball
CORNERS = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (0.25, 0.5)]


@functools.lru_cache(maxsize=None)
def scene(name):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_util.SCENES, name + ".json"))


def oracle(name):
    return _util.OracleScene(scene(name))


def bounds(name):
    """Centre and radius of the instances' boxes (the floor planes included), float64."""
    inst = scene(name).array("instances")
    lo, hi = inst["bmin"].min(axis=0).astype(np.float64), inst["bmax"].max(axis=0).astype(np.float64)
    return (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2


@functools.lru_cache(maxsize=None)
def grid_hits(name):
    """The first segments of a 48 x 36 pinhole grid and the oracle's closest hits."""
    sc = scene(name)
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RECURRENCE, spp=1, seed=SEED)
    seg = _util.first_segments(_radiance_ref.plan_rays(spt, sc, r, W, H, 0, 1, camera=CAMERAS[name]))
    return seg, oracle(name).trace_closest(seg)


@functools.lru_cache(maxsize=None)
def surface_points(name):
    """SURFACE points: the grid's mesh hits, then corners, edge midpoints and an inner point of up to 16 triangles per mesh instance."""
    sc = scene(name)
    _, hits = grid_hits(name)
    inst, meshes = sc.array("instances"), sc.array("meshes")
    on_mesh = (hits["instance"] >= 0) & (inst["prim_type"][np.maximum(hits["instance"], 0)] == 1)
    grid = np.zeros(int(on_mesh.sum()), dtype=spt.BAKE_POINT_DTYPE)
    for f in ("instance", "prim", "v", "w"):
        grid[f] = hits[f][on_mesh]
    out = [grid]
    for i, rec in enumerate(inst):
        if rec["prim_type"] != 1:
            continue
        m = meshes[rec["prim_id"]]
        tris = np.unique(np.linspace(0, int(m["tri_count"]) - 1, 16).astype(np.int64))
        pts = np.zeros((len(tris), len(CORNERS)), dtype=spt.BAKE_POINT_DTYPE)
        pts["instance"] = i
        pts["prim"] = (int(m["tri_first"]) + tris)[:, None]
        pts["v"], pts["w"] = [c[0] for c in CORNERS], [c[1] for c in CORNERS]
        out.append(pts.reshape(-1))
    return np.concatenate(out)


def _flat(rays):
    rays = np.ascontiguousarray(rays).reshape(-1).copy()
    return rays


def surface_rays(name, variant=""):
    rays = _flat(spt.bake_rays(scene(name), surface_points(name), samples=1, seed=SEED)["rays"])
    if variant == "t0":
        rays["t_min"] = f32(0)
    elif variant == "x3":
        rays["d"] = rays["d"] * f32(3)
    elif variant == "x025":
        rays["d"] = rays["d"] * f32(0.25)
    else:
        assert variant == ""
    return rays, None


def world_rays(name):
    seg, hits = grid_hits(name)
    inst = scene(name).array("instances")
    other = (hits["instance"] >= 0) & (inst["prim_type"][np.maximum(hits["instance"], 0)] != 1)
    pts = np.zeros(int(other.sum()), dtype=spt.BAKE_WORLD_DTYPE)
    pts["p"] = seg["o"][other] + seg["d"][other] * hits["t"][other][:, None]
    pts["n"] = -seg["d"][other]
    return _flat(spt.bake_rays(scene(name), pts, samples=1, seed=SEED, world=True)["rays"]), None


def void_point(name):
    centre, radius = bounds(name)
    return centre + np.array([0.6, 0.64, -0.48]) * (1000.0 * radius)


def free_points(name):
    """24 points: the scene's points of interest, the void point, the rest uniform in the scene's box grown by 30 %."""
    centre, radius = bounds(name)
    inst = scene(name).array("instances")
    lo, hi = inst["bmin"].min(axis=0).astype(np.float64), inst["bmax"].max(axis=0).astype(np.float64)
    half = np.maximum((hi - lo) / 2, 0.5) * 1.3
    special = [np.array(p) for p in INSIDE.get(name, [])] + [void_point(name)]
    rest = centre + np.random.default_rng(21).uniform(-1, 1, size=(24 - len(special), 3)) * half
    return np.concatenate([np.array(special), rest]).astype(f32)


def free_rays(name):
    return _flat(spt.probe_rays(scene(name), free_points(name), samples=32, seed=SEED)["rays"]), None


def big_rays(name):
    centre, radius = bounds(name)
    p = centre + np.random.default_rng(22).uniform(-1, 1, size=(129, 3)) * min(radius, 4.0)
    return _flat(spt.probe_rays(scene(name), p.astype(f32), samples=129, seed=SEED)["rays"]), None


def camera_models(name):
    """The models of tests/test_gpu_camera_models.py: a thin lens of radius 0.15 focused at the world origin's depth, an orthographic
    view of about the pinhole's framing there, a panorama from the camera's eye."""
    cam = scene(name).get_camera(CAMERAS[name])
    eye, fwd = np.array(cam.eye[:], dtype=np.float64), np.array(cam.forward[:], dtype=np.float64)
    focus = max(float(np.dot(-eye, fwd)), 1.0)
    return {"thin_lens": spt.CameraModel.thin_lens(cam, 0.15, focus),
            "orthographic": spt.CameraModel.orthographic(cam, focus / float(cam.half_cot_half_fov)),
            "panorama": spt.CameraModel.panorama(cam.eye[:])}


def camera_tracer():
    return spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RANDOM, spp=4, seed=SEED)


def model_rays(name, kind, aux=True):
    rays, ax = _camera_ref.plan_rays(spt, camera_models(name)[kind], camera_tracer(), W, H, 0, 1, aux=True)
    return _flat(rays), (_flat(ax) if aux else None)


def axis_rays(name):
    sc = scene(name)
    tab = _bake_ref.tables(sc)
    inst, meshes = tab["instances"], tab["meshes"]
    tri_pts = []
    for i, rec in enumerate(inst):
        if rec["prim_type"] != 1:
            continue
        m = meshes[rec["prim_id"]]
        tris = np.unique(np.linspace(0, int(m["tri_count"]) - 1, 12).astype(np.int64))
        pts = np.zeros((len(tris), 3), dtype=spt.BAKE_POINT_DTYPE)
        pts["instance"], pts["prim"] = i, (int(m["tri_first"]) + tris)[:, None]
        pts["v"], pts["w"] = [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
        tri_pts.append(pts)
    tri_pts = np.concatenate(tri_pts)
    P = _bake_ref.resolve(tab, tri_pts.reshape(-1))[0].reshape(-1, 3, 3)       # world corners of every chosen triangle
    verts = np.unique(P.reshape(-1, 3), axis=0)
    centre, radius = bounds(name)
    o_list, d_list = [], []
    # 1. axis-parallel through every vertex, every sign pattern of the two zero components
    for a in range(3):
        for s in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    d = np.zeros(3, dtype=f32)
                    d[(a + 1) % 3], d[(a + 2) % 3] = z1, z2
                    d[a] = s
                    o = verts.copy()
                    o[:, a] = f32(centre[a] - s * 1.5 * radius)
                    o_list.append(o)
                    d_list.append(np.broadcast_to(d, o.shape))
    # 2. along every edge of the chosen triangles, from two edge lengths before its first end
    for k in range(3):
        a, b = P[:, k], P[:, (k + 1) % 3]
        e = b - a
        o_list.append((a - e * f32(2)).astype(f32))
        d_list.append(_bake_ref.normalize(e))
    # 3. aimed at every vertex from the camera's eye and from two points beside and above the scene
    cam = sc.get_camera(CAMERAS[name])
    for eye in (np.array(cam.eye[:], dtype=f32), (centre + np.array([1.2, 0.3, 0.1]) * radius).astype(f32), (centre + np.array([-0.2, 1.1, -0.4]) * radius).astype(f32)):
        o_list.append(np.broadcast_to(eye, verts.shape))
        d_list.append(_bake_ref.normalize(verts - eye))
    o, d = np.concatenate(o_list).astype(f32), np.concatenate(d_list).astype(f32)
    rays = np.zeros(o.shape[0], dtype=spt.PATH_RAY_DTYPE)
    rays["o"], rays["d"], rays["t_min"] = o, d, f32(0.0001)
    rays["stream_a"], rays["stream_b"] = np.arange(o.shape[0], dtype=np.uint32), 3
    assert np.signbit(rays["d"][rays["d"] == 0]).any() and (~np.signbit(rays["d"][rays["d"] == 0])).any()
    return rays, None


def make(name, kind):
    """(rays, aux or None, rng_skip) of a batch; kind as in the module's docstring, variants after a colon."""
    base, _, variant = kind.partition(":")
    if base == "surface":
        return surface_rays(name, variant) + (0,)
    if base == "world":
        return world_rays(name) + (0,)
    if base == "free":
        return free_rays(name) + (0,)
    if base == "big":
        return big_rays(name) + (0,)
    if base == "axes":
        return axis_rays(name) + (0,)
    assert base in ("thin_lens", "orthographic", "panorama") and variant in ("", "noaux")
    return model_rays(name, base, aux=variant == "") + (_radiance_ref.rng_skip(spt, camera_tracer()),)


@functools.lru_cache(maxsize=None)
def batch(name, kind, repeats=1):
    """(rays, aux, rng_skip, the oracle's colours (n, 3), the oracle's hits); read-only, computed once."""
    rays, aux, skip = make(name, kind)
    orc = oracle(name)
    rgb, hits = orc.radiance(rays, aux, repeats=repeats, max_depth=DEPTH, seed=SEED, rng_skip=skip, hits=True)
    for a in (rays, aux, rgb, hits):
        if a is not None:
            a.setflags(write=False)
    return rays, aux, skip, rgb, hits


def live(rgb):
    """Rays whose colour is finite and not black."""
    return np.isfinite(rgb).all(axis=-1) & (rgb != 0).any(axis=-1)


def census(rgb):
    """(fraction of rays with a finite non-zero colour, number of distinct such colours)."""
    ok = live(rgb)
    return float(ok.mean()), len(np.unique(np.ascontiguousarray(rgb[ok]).view(np.uint32), axis=0))

"""Pins for the CPU oracle.  The reference ships no tests / golden outputs for this path and cannot
be built here ("parity unpinned" vs the Rust binary), so the oracle is pinned by
  1. closed-form images of the two shipped scenes (convex Lambert object, one delta light),
  2. hand-derived known answers for the geometric and BxDF formulas it restates,
  3. internal consistency: BVH vs brute force, divide vs reciprocal slab test, libm vs detmath.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _util

spt = _util.load_pkg()
F32_MAX = np.float32(3.4028234663852886e38)


def _scene(name):
    return spt.load_scene(os.path.join(_util.SCENES, name))


def _write_scene(tmp_path, prims, instances, objs=None, extra=None):
    for fname, text in (objs or {}).items():
        (tmp_path / fname).write_text(text)
    sc = {"cameras": {"type": "perspective", "name": "c", "eye": [0.0, 0.0, 5.0], "forward": [0.0, 0.0, -1.0], "up": [0.0, 1.0, 0.0], "fov": 45.0},
          "textures": [{"type": "scalar", "name": "w", "value": [1.0, 1.0, 1.0]}],
          "materials": [{"type": "lambert", "name": "m", "albedo": "w"}], "mediums": [], "surfaces": [],
          "primitives": prims, "instances": instances,
          "lights": [{"type": "directional", "name": "l", "direction": [0.0, -1.0, 0.0], "strength": [1.0, 1.0, 1.0]}]}
    sc.update(extra or {})
    p = tmp_path / "scene.json"
    p.write_text(json.dumps(sc))
    return spt.load_scene(str(p))


def _rays(o, d, t_min=1e-4, t_max=F32_MAX):
    o, d = np.atleast_2d(np.asarray(o, np.float32)), np.atleast_2d(np.asarray(d, np.float32))
    r = np.zeros(len(o), dtype=spt.RAY_DTYPE)
    r["o"], r["d"], r["t_min"], r["t_max"] = o, d, t_min, t_max
    return r


# ---------------------------------------------------------------- 1. closed-form images
def test_scene01_cube_closed_form():
    """L = strength * rho/pi * max(n.l, 0): faces +z' and -x' of the cube rotated 60 deg about Y."""
    sc = _scene("cfg2_cube.json")
    r = spt.PathTracer(max_depth=8, spp=16, seed=1)
    film, st = _util.oracle_render(sc, r, 256, 256)
    l = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    c, s = np.cos(np.radians(60.0)), np.sin(np.radians(60.0))
    n_front, n_left = np.array([s, 0.0, c]), np.array([-c, 0.0, s])   # glam from_rotation_y columns
    lum = [5.0 / np.pi * max(n @ l, 0.0) for n in (n_front, n_left)]
    assert abs(lum[0] - 1.2552) < 1e-3 and abs(lum[1] - 0.3363) < 1e-3
    g = film[..., 0]
    assert np.array_equal(film[..., 0], film[..., 1]) and np.array_equal(film[..., 1], film[..., 2])
    near = lambda v: np.abs(g - v) < 2e-5
    interior = near(0.0) | near(lum[0]) | near(lum[1])
    assert interior.mean() > 0.97                       # only silhouette / edge pixels are mixtures
    assert abs(near(lum[0]).mean() + near(lum[1]).mean() - 0.1846) < 0.012   # hit fraction
    assert abs(g.mean() - 0.11295) < 2e-3
    assert near(lum[1]).sum() > near(lum[0]).sum() > 1000
    # u8 image values of the reference's color_to_rgb: 85 and 255
    u8 = spt.film_to_rgb8(film)
    vals = set(np.unique(u8[interior]))
    assert vals == {0, 85, 255}
    assert abs(st.segments_closest / st.samples - 1.175) < 0.02   # 1 primary + 0.185 * 0.95 bounce rays


def test_scene00_sphere_closed_form():
    sc = _scene("cfg1_sphere.json")
    r = spt.PathTracer(max_depth=8, spp=16, seed=1)
    film, _ = _util.oracle_render(sc, r, 256, 256)
    mean = film.reshape(-1, 3).mean(0)
    assert np.allclose(mean, [0.0671, 0.0940, 0.1342], atol=1.5e-3)
    assert abs(film.max() - 5.0 / np.pi) < 2e-3          # blue channel where n = l
    assert np.allclose(film[..., 0] * 2.0, film[..., 2], atol=1e-6)   # albedo (0.5, 0.7, 1.0)
    # per-pixel closed form at pixel centres, away from silhouette and terminator
    h = w = 256
    j, i = np.mgrid[0:h, 0:w]
    x = ((i + 0.5) / w - 0.5) * 1.0
    y = ((h - j - 1) + 0.5) / h - 0.5
    half_cot = 0.5 / np.tan(np.radians(45.0) / 2)
    d = np.stack([x, y, -half_cot * np.ones_like(x)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.array([0.0, 0.0, 5.0]) - np.array([0.5, 0.0, 0.0])
    b = d @ o
    disc = b * b - (o @ o - 1.0)
    hit = disc > 0.02
    t = -b - np.sqrt(np.where(hit, disc, 0))
    n = o + d * t[..., None]
    cosl = np.clip(n @ (np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)), 0, None)
    ok = hit & (cosl > 0.05)
    assert ok.sum() > 4000
    assert np.abs(film[..., 2][ok] - 5.0 / np.pi * cosl[ok]).max() < 0.02


# ---------------------------------------------------------------- 2. geometric known answers
TRI_OBJ = "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1\n"


def test_triangle_moller_trumbore_known_answers(tmp_path):
    sc = _write_scene(tmp_path, [{"type": "trimesh", "name": "t", "obj_file": "t.obj"}],
                      [{"name": "i", "primitive": "t", "material": "m"}], {"t.obj": TRI_OBJ})
    o = [[0.25, 0.25, 2.0], [0.0, 0.0, 2.0], [0.5, 0.5, 2.0], [0.5, 0.0, 2.0], [0.6, 0.6, 2.0], [-0.001, 0.2, 2.0],
         [0.25, 0.25, -3.0], [0.25, 0.25, 2.0]]
    d = [[0, 0, -1]] * 6 + [[0, 0, 1], [0, 0, 1]]
    h = _util.oracle_trace_closest(sc, _rays(o, d), _util.ORACLE_BRUTE_FORCE)
    assert h["instance"].tolist() == [0, 0, 0, 0, -1, -1, 0, -1]      # vertex, hypotenuse and edge hits count (>= 0)
    # through the BLAS the vertex / edge rays lie IN a bounding plane with a zero direction component:
    # (p_min - o)/d = 0/0 = NaN, f32::min(NaN, +inf) = +inf, so Bbox::intersect_ray culls them
    # (bbox.rs:68-84) -- reference behaviour, kept
    hb = _util.oracle_trace_closest(sc, _rays(o, d))
    assert hb["instance"].tolist() == [0, -1, 0, -1, -1, -1, 0, -1]
    assert np.allclose(h["t"][:4], 2.0) and h["t"][6] == 3.0           # two-sided: back face hit too
    assert np.allclose([h["v"][0], h["w"][0]], [0.25, 0.25])          # v, w = barycentrics of p1, p2
    assert h["t"][4] == F32_MAX and h["prim"][4] == -1
    # t_min / t_max are strict bounds
    r = _rays([[0.25, 0.25, 2.0]] * 3, [[0, 0, -1]] * 3)
    r["t_min"] = [2.0, 1.9999, 1e-4]
    r["t_max"] = [F32_MAX, F32_MAX, 2.0]
    assert _util.oracle_trace_closest(sc, r)["instance"].tolist() == [-1, 0, -1]
    assert _util.oracle_trace_any(sc, r).tolist() == [0, 1, 0]
    # ray parallel to the plane: det == 0 -> no hit, no NaN leakage
    assert _util.oracle_trace_closest(sc, _rays([[-1, 0.2, 0.0]], [[1, 0, 0]]))["instance"][0] == -1


def test_sphere_roots_inside_outside_and_scaled_instance(tmp_path):
    sc = _write_scene(tmp_path, [{"type": "sphere", "name": "s", "center": [0.0, 0.0, 0.0], "radius": 1.0}],
                      [{"name": "i", "primitive": "s", "material": "m", "scale": [2.0, 2.0, 2.0], "translate": [1.0, 0.0, 0.0]}])
    # world sphere: centre (1,0,0), radius 2.  outside: near root; inside: far root; tangent miss
    h = _util.oracle_trace_closest(sc, _rays([[1, 0, 10], [1, 0, 0], [1, 2.01, 10], [1, 0, -10]],
                                              [[0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, -1]]))
    assert h["instance"].tolist() == [0, 0, -1, -1]
    assert np.allclose(h["t"][:2], [8.0, 2.0], atol=1e-5)    # t is shared between world and object space
    # intersect_test uses `min < t_max && max > t_min` (sphere.rs:51-56): a sphere entirely behind t_max passes
    r = _rays([[1, 0, 10]], [[0, 0, -1]], t_max=9.0)
    assert _util.oracle_trace_any(sc, r)[0] == 1
    r["t_max"] = 7.9
    assert _util.oracle_trace_any(sc, r)[0] == 0


def test_slab_zero_direction_components_and_nan_lanes(tmp_path):
    sc = _write_scene(tmp_path, [{"type": "trimesh", "name": "c", "obj_file": "c.obj"}],
                      [{"name": "i", "primitive": "c", "material": "m"}],
                      {"c.obj": open(os.path.join(_util.SCENES, "models", "cube.obj")).read()}, {"aggregate": "bvh"})
    o = [[0.3, 0.2, 5.0], [1.0, 0.2, 5.0], [1.5, 0.2, 5.0], [0.0, 0.0, 0.0]]
    d = [[0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, 1]]
    for flags in (0, _util.ORACLE_SLAB_RECIPROCAL, _util.ORACLE_BRUTE_FORCE):
        h = _util.oracle_trace_closest(sc, _rays(o, d), flags)
        assert h["instance"][0] == 0 and h["t"][0] == 4.0
        assert h["instance"][2] == -1                      # outside the slab on an axis with d = 0
        assert h["instance"][3] == 0 and h["t"][3] == 1.0  # origin inside the box
    # origin exactly on the x = 1 face plane with d.x = 0: (p_max.x - o.x)/d.x = 0/0 = NaN and
    # (p_min.x - o.x)/d.x = -inf; f32::min/max ignore the NaN, x-slab = [-inf, -inf] -> culled by the
    # box although the triangles of that face would report a hit (reference behaviour, both slab forms)
    assert _util.oracle_trace_closest(sc, _rays(o, d), 0)["instance"][1] == -1
    assert _util.oracle_trace_closest(sc, _rays(o, d), _util.ORACLE_SLAB_RECIPROCAL)["instance"][1] == -1
    assert _util.oracle_trace_closest(sc, _rays(o, d), _util.ORACLE_BRUTE_FORCE)["instance"][1] == 0


# ---------------------------------------------------------------- 3. consistency on real scenes
@pytest.mark.parametrize("name", ["cfg1_sphere.json", "cfg2_cube.json", "t_materials.json", "t_power_is.json", "t_medium.json"])
def test_bvh_equals_brute_force_and_reciprocal_slab(name):
    sc = _scene(name)
    rays = _util.random_rays(sc, 60_000, seed=3)
    ref = _util.oracle_trace_closest(sc, rays, _util.ORACLE_BRUTE_FORCE)
    assert (ref["instance"] >= 0).mean() > 0.2
    for flags in (0, _util.ORACLE_SLAB_RECIPROCAL, _util.ORACLE_DEVICE):
        got = _util.oracle_trace_closest(sc, rays, flags)
        # culling cannot change the closest distance, except between coincident surfaces (objects
        # resting on the floor plane): there the slab distance of the flat floor box and the triangle
        # distance differ in the last bit, so culling against an equal-depth earlier hit can win
        # (inherent to bbox.rs:86-92 + triangle.rs:187 in the reference too)
        same_t = got["t"].view(np.uint32) == ref["t"].view(np.uint32)
        assert same_t.mean() > 0.999
        hit = ref["instance"] >= 0
        assert np.array_equal(hit, got["instance"] >= 0)
        assert (np.abs(got["t"][hit] - ref["t"][hit]) <= 4e-7 * ref["t"][hit]).all()
        tie =(got["prim"] != ref["prim"]) | (got["instance"] != ref["instance"])
        assert tie.mean() < 5e-3                 # equal-depth candidates may resolve differently by visit order
    rays["t_max"] = np.where(ref["instance"] >= 0, ref["t"] * np.float32(0.99), np.float32(4.0))
    a = _util.oracle_trace_any(sc, rays, _util.ORACLE_BRUTE_FORCE)
    assert np.array_equal(a, _util.oracle_trace_any(sc, rays, 0))
    assert np.array_equal(a, _util.oracle_trace_any(sc, rays, _util.ORACLE_SLAB_RECIPROCAL))


@pytest.mark.parametrize("name,cam", [("t_materials.json", "main"), ("t_medium.json", None)])
def test_render_modes_agree(name, cam):
    """reference-faithful mode (divide slab, libm) vs the modes the GPU parity tests use."""
    sc = _scene(name)
    r = spt.PathTracer(max_depth=8, sampler=spt.SAMPLER_RANDOM, spp=8, seed=4)
    base, _ = _util.oracle_render(sc, r, 96, 72, camera=cam)
    recip, _ = _util.oracle_render(sc, r, 96, 72, camera=cam, flags=_util.ORACLE_SLAB_RECIPROCAL)
    device, _ = _util.oracle_render(sc, r, 96, 72, camera=cam, flags=_util.ORACLE_DEVICE)
    brute, _ = _util.oracle_render(sc, r, 96, 72, camera=cam, flags=_util.ORACLE_BRUTE_FORCE)
    libm, _ = _util.oracle_render(sc, r, 96, 72, camera=cam, flags=_util.ORACLE_LIBM)
    scale = max(float(base.mean()), 1e-3)
    assert np.abs(base - recip).mean() / scale < 1e-4
    assert np.abs(base - device).mean() / scale < 1e-4      # what the GPU parity tests compare against
    assert np.abs(base - brute).mean() / scale < 2e-3
    # libm vs deterministic kernels: 1-ulp direction changes can flip a rare hit, never the statistics
    assert np.abs(base - libm).mean() / scale < 5e-2
    assert abs(float(libm.mean()) - float(base.mean())) / scale < 5e-3


def test_thread_count_and_sharding_do_not_change_the_image():
    sc = _scene("t_materials.json")
    r = spt.PathTracer(max_depth=6, sampler=spt.SAMPLER_RANDOM, spp=4, seed=9)
    a, _ = _util.oracle_render(sc, r, 64, 48, camera="main", threads=1)
    b, _ = _util.oracle_render(sc, r, 64, 48, camera="main", threads=7)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    out = np.zeros_like(a)
    for k in range(3):
        rows = spt.shard_rows(48, k, 3, 4)
        out[rows], _ = _util.oracle_render(sc, r, 64, 48, camera="main", shard_index=k, shard_count=3, strip_rows=4)
    assert np.array_equal(a.view(np.uint32), out.view(np.uint32))


def test_tie_rule_is_order_independent(tmp_path):
    """Two instances of the same quad at the same place: every hit is an exact tie.  The reference rule
    keeps the first instance in visit order; ORACLE_TIE_MIN_ID keeps the smallest (instance, prim),
    whatever the order (BVH, brute force)."""
    quad = "v -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nvn 0 0 1\nf 1//1 2//1 3//1\nf 1//1 3//1 4//1\n"
    sc = _write_scene(tmp_path, [{"type": "trimesh", "name": "q", "obj_file": "q.obj"}],
                      [{"name": "a", "primitive": "q", "material": "m"}, {"name": "b", "primitive": "q", "material": "m"}],
                      {"q.obj": quad}, {"aggregate": "bvh"})
    rng = np.random.default_rng(0)
    o = np.c_[rng.uniform(-0.9, 0.9, (500, 2)), np.full(500, 3.0)]
    rays = _rays(o, np.tile([0.0, 0.0, -1.0], (500, 1)))
    ref = _util.oracle_trace_closest(sc, rays, 0)
    tie = _util.oracle_trace_closest(sc, rays, _util.ORACLE_TIE_MIN_ID)
    brute = _util.oracle_trace_closest(sc, rays, _util.ORACLE_TIE_MIN_ID | _util.ORACLE_BRUTE_FORCE)
    assert (ref["t"] == 3.0).all() and (tie["t"] == 3.0).all()
    assert (tie["instance"] == 0).all() and np.array_equal(tie["prim"], brute["prim"]) and (brute["instance"] == 0).all()
    # on the shared diagonal both triangles of the quad tie as well: the lower prim index wins
    diag = _rays([[0.3, 0.3, 3.0]], [[0.0, 0.0, -1.0]])
    assert _util.oracle_trace_closest(sc, diag, _util.ORACLE_TIE_MIN_ID)["prim"][0] == 0


# ---------------------------------------------------------------- the headline workload's mesh
REF_CUBE = os.path.join(_util.GOLDEN, "reference_scenes", "models", "cube.obj")   # the reference's scenes/models/cube.obj (data fixture)


def _obj_triangles(path):
    """{triangle} of an OBJ file, each a frozenset of its three (position, normal) corners: what the integrator can see of a
    mesh whose material ignores texcoords (vertex order, face order and index sharing do not matter)."""
    v, vn, tris = [], [], set()
    for line in open(path):
        t = line.split()
        if not t:
            continue
        if t[0] == "v":
            v.append(tuple(float(x) for x in t[1:4]))
        elif t[0] == "vn":
            vn.append(tuple(float(x) for x in t[1:4]))
        elif t[0] == "f":
            c = []
            for w in t[1:]:
                idx = w.split("/")
                c.append((v[int(idx[0]) - 1], vn[int(idx[2]) - 1]))
            for k in range(1, len(c) - 1):
                tris.add(frozenset((c[0], c[k], c[k + 1])))
    return tris


def test_generated_cube_is_the_reference_cube(tmp_path):
    """scenes_amd/models/cube.obj is generated (24 vertices, another face / uv order); the headline workload claims to be the
    reference's scenes/test_scene_01.json.  With the reference's own cube.obj kept as a data fixture under tests/golden:
    the two files describe the same 12 triangles with the same normals, and the scene rendered from the reference's own
    file has the same closed-form film (interior pixels to 1e-5; the two visible face radiances 0.3363 / 1.2552)."""
    ours = _obj_triangles(os.path.join(_util.SCENES, "models", "cube.obj"))
    theirs = _obj_triangles(REF_CUBE)
    assert len(ours) == len(theirs) == 12 and ours == theirs
    scene = json.load(open(os.path.join(_util.SCENES, "cfg2_cube.json")))
    n_prims = 0
    for prim in (scene["primitives"] if isinstance(scene["primitives"], list) else [scene["primitives"]]):
        if prim.get("obj_file"):
            prim["obj_file"] = os.path.relpath(REF_CUBE, str(tmp_path))     # (the loader resolves model files against the scene file)
            n_prims += 1
    assert n_prims == 1
    p = tmp_path / "scene_01_with_reference_cube.json"
    p.write_text(json.dumps(scene))
    r = spt.PathTracer(max_depth=8, spp=4, seed=1)
    a, _ = _util.oracle_render(_scene("cfg2_cube.json"), r, 192, 192)
    b, _ = _util.oracle_render(spt.load_scene(str(p)), r, 192, 192)
    lum = (5.0 / np.pi * np.array([np.sin(np.radians(60.0)) + np.cos(np.radians(60.0)), np.sin(np.radians(60.0)) - np.cos(np.radians(60.0))]) / np.sqrt(3.0))
    for film in (a, b):
        g = film[..., 0]
        interior = (np.abs(g) < 2e-5) | (np.abs(g - lum[0]) < 2e-5) | (np.abs(g - lum[1]) < 2e-5)
        assert interior.mean() > 0.96 and abs((g > 0.01).mean() - 0.1846) < 0.012
    same = np.abs(a - b) < 1e-5
    assert same.mean() > 0.995      # silhouette / edge samples can fall either side in the last bit: another vertex order rounds differently
    assert np.abs(a - b).mean() < 1e-4


# ---------------------------------------------------------------- MIS direct lighting against the form-factor integral
def test_area_light_mis_equals_the_form_factor_integral(tmp_path):
    """A pin for the arithmetic no closed-form IMAGE of the shipped scenes reaches (round 3): a black, one-sided emissive quad
    above a Lambert floor.  With max_depth >= 2 a pixel's expectation is emission-free direct lighting,
        L(p) = rho / pi * Le * integral over the quad of cos(theta_p) cos(theta_l) / r^2 dA,
    assembled by the integrator from TWO estimators - the light sample (Triangle::sample, ShapeLight's area-to-solid-angle pdf,
    pdf_shape_light) and the BSDF sample that happens to hit the quad (emission weighted against pdf_shape_light) - under the
    power heuristic (pt.rs:129-181, 298-302).  The integral is evaluated in float64 by quadrature; nothing of oracle.cpp is used.
    Either estimator alone (max_depth 1 = light samples only) must give the same mean: the MIS weights sum to one."""
    (tmp_path / "plane.obj").write_text(open(os.path.join(_util.SCENES, "models", "plane.obj")).read())
    # the quad in world coordinates, identity transform (Triangle::pdf is an OBJECT-space density, triangle.rs:224-289), facing down
    (tmp_path / "quad.obj").write_text("v -0.5 1.5 -0.4\nv 0.5 1.5 -0.4\nv 0.5 1.5 0.4\nv -0.5 1.5 0.4\nvn 0 -1 0\nvt 0 0\nf 1/1/1 2/1/1 3/1/1\nf 1/1/1 3/1/1 4/1/1\n")
    rho, le = 0.8, 10.0
    sc = {"cameras": {"type": "perspective", "name": "c", "eye": [0.0, 1.0, 3.0], "forward": [0.0, -0.6, -1.0], "up": [0.0, 1.0, 0.0], "fov": 30.0},
          "textures": [{"type": "scalar", "name": "w", "value": [rho, rho, rho]}, {"type": "scalar", "name": "k", "value": [0.0, 0.0, 0.0]}],
          "materials": [{"type": "lambert", "name": "white", "albedo": "w"}, {"type": "lambert", "name": "black", "albedo": "k"}], "mediums": [],
          "surfaces": [{"name": "glow", "material": "black", "emissive": [le, le, le]}],
          "primitives": [{"type": "trimesh", "name": "plane", "obj_file": "plane.obj"}, {"type": "trimesh", "name": "quad", "obj_file": "quad.obj"}],
          "instances": [{"name": "floor", "primitive": "plane", "material": "white", "scale": [4.0, 1.0, 4.0]},
                        {"name": "lamp", "primitive": "quad", "surface": "glow"}],
          "lights": []}
    p = tmp_path / "mis.json"
    p.write_text(json.dumps(sc))
    scene = spt.load_scene(str(p))
    w = h = 24
    # expected radiance at the pixel centres, float64
    cam = scene.get_camera(None)
    eye, fwd, up, right = (np.array(list(v), float) for v in (cam.eye, cam.forward, cam.up, cam.right))
    j, i = np.mgrid[0:h, 0:w]
    x = ((i + 0.5) / w - 0.5) * (w / h)
    y = ((h - j - 1) + 0.5) / h - 0.5
    d = fwd * cam.half_cot_half_fov + right * x[..., None] + up * y[..., None]
    t = -eye[1] / d[..., 1]
    pt = eye + d * t[..., None]                                   # on the floor y = 0
    assert (t > 0).all() and (np.abs(pt[..., [0, 2]]) < 3.9).all()  # every pixel sees the floor, none sees the lamp
    qx, qz = np.meshgrid((np.arange(160) + 0.5) / 160 - 0.5, ((np.arange(128) + 0.5) / 128 - 0.5) * 0.8)
    q = np.stack([qx, np.full_like(qx, 1.5), qz], -1).reshape(-1, 3)
    da = 1.0 * 0.8 / len(q)
    v = q[None, None] - pt[:, :, None]                            # (h, w, nq, 3)
    r2 = (v * v).sum(-1)
    cos_p = v[..., 1] / np.sqrt(r2)                               # floor normal +y
    cos_l = v[..., 1] / np.sqrt(r2)                               # lamp normal -y, direction from the lamp = -v
    want = rho / np.pi * le * (cos_p * cos_l / r2).sum(-1) * da
    assert 0.05 < want.min() and want.max() < 3.0
    for depth, spp in ((2, 1024), (8, 512), (1, 1024)):
        r = spt.PathTracer(max_depth=depth, sampler=spt.SAMPLER_RANDOM, spp=spp, seed=7)
        film, _ = _util.oracle_render(scene, r, w, h)
        assert np.allclose(film[..., 0], film[..., 1]) and np.isfinite(film).all()
        rel = film[..., 0].mean() / want.mean() - 1.0
        assert abs(rel) < 0.01, (depth, rel)                      # the image mean: ~0.3 % noise at these sample counts
        blocks = film[..., 0].reshape(4, h // 4, 4, w // 4).mean(axis=(1, 3)) / want.reshape(4, h // 4, 4, w // 4).mean(axis=(1, 3))
        assert np.abs(blocks - 1.0).max() < 0.04, (depth, blocks)  # and block by block across the penumbra-free gradient


def test_point_and_spot_light_closed_forms(tmp_path):
    """Delta lights over a Lambert floor, max_depth 1: every sample of a pixel returns rho / pi * cos(theta) * strength(w) / r^2 at
    its own floor point - no noise beyond the sub-pixel position.  Written from src/light/point.rs:23-32 and spot.rs:50-66 (linear
    falloff of dot(direction, -wi) between cos(outer) and cos(inner), the spot's `direction` used as given, not normalised)."""
    (tmp_path / "plane.obj").write_text(open(os.path.join(_util.SCENES, "models", "plane.obj")).read())
    rho = 0.6
    pos = np.array([0.3, 2.0, -0.2])
    direction = np.array([0.1, -1.0, 0.05])
    direction /= np.linalg.norm(direction)
    inner, outer = 15.0, 40.0
    for kind in ("point", "spot"):
        light = {"type": kind, "name": "l", "position": pos.tolist(), "strength": [4.0, 2.0, 1.0]}
        if kind == "spot":
            light.update({"direction": direction.tolist(), "inner_angle": inner, "outer_angle": outer})
        sc = {"cameras": {"type": "perspective", "name": "c", "eye": [0.0, 2.5, 4.0], "forward": [0.0, -0.7, -1.0], "up": [0.0, 1.0, 0.0], "fov": 35.0},
              "textures": [{"type": "scalar", "name": "w", "value": [rho, rho, rho]}], "materials": [{"type": "lambert", "name": "white", "albedo": "w"}],
              "mediums": [], "surfaces": [], "primitives": [{"type": "trimesh", "name": "plane", "obj_file": "plane.obj"}],
              "instances": [{"name": "floor", "primitive": "plane", "material": "white", "scale": [6.0, 1.0, 6.0]}], "lights": [light]}
        p = tmp_path / ("%s.json" % kind)
        p.write_text(json.dumps(sc))
        scene = spt.load_scene(str(p))
        w = h = 32
        cam = scene.get_camera(None)
        eye, fwd, up, right = (np.array(list(v), float) for v in (cam.eye, cam.forward, cam.up, cam.right))
        j, i = np.mgrid[0:h, 0:w]
        d = fwd * cam.half_cot_half_fov + right * (((i + 0.5) / w - 0.5) * (w / h))[..., None] + up * (((h - j - 1) + 0.5) / h - 0.5)[..., None]
        pt = eye + d * (-eye[1] / d[..., 1])[..., None]
        v = pos - pt
        r2 = (v * v).sum(-1)
        wi = v / np.sqrt(r2)[..., None]
        strength = np.array([4.0, 2.0, 1.0])[None, None] * np.ones_like(r2)[..., None]
        if kind == "spot":
            co, ci = np.cos(np.radians(outer)), np.cos(np.radians(inner))
            atten = np.clip(((-wi) @ direction - co) / max(ci - co, 1e-4), 0.0, 1.0)
            strength = strength * atten[..., None]
        want = rho / np.pi * wi[..., 1:2] * strength / r2[..., None]
        film, _ = _util.oracle_render(scene, spt.PathTracer(max_depth=1, sampler=spt.SAMPLER_RANDOM, spp=64, seed=2), w, h)
        lit = want[..., 0] > 1e-3
        if kind == "spot":
            lit &= atten > 0.3          # the rim of the cone (and the pixels straddling it) are compared through the image mean only
        assert lit.mean() > (0.9 if kind == "point" else 0.15)
        # pixel mean over 64 jittered positions vs the centre value: a smooth function, second-order difference only
        assert np.abs(film[lit] / want[lit] - 1.0).max() < (0.05 if kind == "point" else 0.15), kind
        assert abs(film[lit].mean() / want[lit].mean() - 1.0) < 0.004, kind
        assert abs(film.mean() / want.mean() - 1.0) < 0.01, kind
        if kind == "spot":
            assert (film[want[..., 0] == 0.0] == 0.0).mean() > 0.9      # outside the cone: black (pixels straddling the edge aside)

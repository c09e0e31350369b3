"""spt_bake without a device: spt_host_bake_rays (include/spt_bake.h, the header the device kernels include) against
tests/_bake_ref.py, word for word; float64 checks of what the rays mean; the lightmap rasteriser; the validity predicate; the
structs' layout in C and in the binding; the stand-alone sanitizer program."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _bake_ref
import _util

spt = _util.load_pkg()
SCENE_NAMES = ["cfg2_cube", "t_materials", "t_textured"]
SAMPLES, SEED = 3, 77


@pytest.fixture(scope="module")
def scenes():
    _util.ensure_cpu_build()
    loaded = {n: spt.load_scene(os.path.join(_util.SCENES, n + ".json")) for n in SCENE_NAMES}
    yield loaded
    for sc in loaded.values():
        sc.close()


def words(a):
    return np.ascontiguousarray(a).view(np.uint8)


def surface_points(scene, per_instance, seed):
    """Random points on every mesh instance, then the three corners of a triangle of each."""
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
        a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
        pts["v"][:per_instance], pts["w"][:per_instance] = a, b
        pts["v"][per_instance:], pts["w"][per_instance:] = [0, 1, 0], [0, 0, 1]
        out.append(pts)
    return np.concatenate(out)


def world_points(n, seed):
    rng = np.random.default_rng(seed)
    pts = np.zeros(n + 2, dtype=spt.BAKE_WORLD_DTYPE)
    pts["p"] = rng.uniform(-2, 2, size=(n + 2, 3))
    d = rng.normal(size=(n + 2, 3))
    pts["n"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    pts["n"][n], pts["n"][n + 1] = [0, 1, 0], [0, -1, 0]   # the two poles of the frame
    return pts


def assert_same(got, want):
    for key in ("pos", "nrm", "delta_li"):
        assert np.array_equal(words(got[key]), words(want[key])), key
    for f in ("o", "t_min", "d", "stream_a", "stream_b", "pad"):
        assert np.array_equal(words(got["rays"][f]), words(want["rays"][f])), f
    for f in ("o", "t_min", "d", "t_max"):
        assert np.array_equal(words(got["delta_rays"][f]), words(want["delta_rays"][f])), f


@pytest.mark.parametrize("flip", [False, True], ids=["", "flip"])
@pytest.mark.parametrize("offsets", [(0, 0), (0xFFFFFFF0, 5)], ids=["first0", "offsets"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_host_rays_equal_the_restated_specification(scenes, name, offsets, flip):
    scene = scenes[name]
    pts = surface_points(scene, 24, 5)
    fp, fs = offsets
    got = spt.bake_rays(scene, pts, samples=SAMPLES, seed=SEED, first_point=fp, first_sample=fs, flip=flip)
    want = _bake_ref.bake_inputs(spt, _bake_ref.tables(scene), pts, SAMPLES, SEED, fp, fs, flip=flip)
    assert got["rays"].shape == (len(pts), SAMPLES)
    assert_same(got, want)
    if name == "t_materials":   # all three delta light types reach some point, the spot with a partial attenuation too
        types = scene.array("lights")["type"]
        for kind in (0, 1, 2):
            assert np.any(got["delta_li"][:, types == kind] != 0), kind


@pytest.mark.parametrize("flip", [False, True], ids=["", "flip"])
@pytest.mark.parametrize("name", ["t_materials"])
def test_world_points_equal_the_restated_specification(scenes, name, flip):
    scene = scenes[name]
    pts = world_points(40, 9)
    got = spt.bake_rays(scene, pts, samples=SAMPLES, seed=SEED, first_point=3, first_sample=1, world=True, flip=flip)
    want = _bake_ref.bake_inputs(spt, _bake_ref.tables(scene), pts, SAMPLES, SEED, 3, 1, world=True, flip=flip)
    assert_same(got, want)
    sign = -1.0 if flip else 1.0
    assert np.array_equal(got["pos"], pts["p"]) and np.array_equal(got["nrm"], sign * pts["n"])


def test_spot_attenuation_is_partial_somewhere(scenes):
    """The cone of t_materials' spot light has a soft edge: the attenuation takes values strictly inside (0, 1) on the floor."""
    scene = scenes["t_materials"]
    lights = scene.array("lights")
    spot = int(np.flatnonzero(lights["type"] == 2)[0])
    lt = lights[spot]
    g = np.linspace(-6, 6, 61, dtype=np.float32)
    pts = np.zeros(61 * 61, dtype=spt.BAKE_WORLD_DTYPE)
    pts["p"][:, 0], pts["p"][:, 2] = np.repeat(g, 61), np.tile(g, 61)
    pts["p"][:, 1] = 0.0
    pts["n"] = [0, 1, 0]
    got = spt.bake_rays(scene, pts, samples=1, world=True)
    sv = lt["pos"].astype(np.float64) - pts["p"].astype(np.float64)
    dist = np.linalg.norm(sv, axis=1)
    x = ((-sv / dist[:, None]) @ lt["dir"].astype(np.float64) - lt["cos_outer"]) / max(float(lt["cos_inner"]) - float(lt["cos_outer"]), 1e-4)
    partial = (x > 0.05) & (x < 0.95) & (sv[:, 1] > 0)
    assert partial.any()
    want = lt["strength"][None, :].astype(np.float64) * np.clip(x, 0, 1)[:, None] / (dist ** 2)[:, None] / np.pi * (sv[:, 1] / dist)[:, None]
    assert np.allclose(got["delta_li"][partial, spot], want[partial], rtol=1e-4, atol=0)
    assert np.array_equal(words(got["delta_li"]), words(_bake_ref.bake_inputs(spt, _bake_ref.tables(scene), pts, 1, 1, world=True)["delta_li"]))


def test_positions_lie_on_their_triangles_and_rays_leave_the_surface(scenes):
    scene = scenes["t_textured"]
    pts = surface_points(scene, 40, 3)
    got = spt.bake_rays(scene, pts, samples=8, seed=4)
    inst, tp = scene.array("instances")[pts["instance"]], scene.array("tri_pos")[pts["prim"]]
    fwd = inst["fwd"].astype(np.float64)
    corners = []
    for key in ("p0", "p1", "p2"):
        q = tp[key].astype(np.float64)
        corners.append(fwd[:, 0:3] * q[:, 0:1] + fwd[:, 3:6] * q[:, 1:2] + fwd[:, 6:9] * q[:, 2:3] + fwd[:, 9:12])
    v, w = pts["v"].astype(np.float64)[:, None], pts["w"].astype(np.float64)[:, None]
    want = corners[0] * (1 - v - w) + corners[1] * v + corners[2] * w
    scale = np.max(np.abs(np.stack(corners)), axis=(0, 2)) + 1
    assert np.all(np.abs(got["pos"] - want) <= 8 * np.finfo(np.float32).eps * scale[:, None])
    d, n = got["rays"]["d"].astype(np.float64), got["nrm"].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(d, axis=-1) - 1) <= 4 * np.finfo(np.float32).eps)   # |d| = 1 within 4 ulp
    assert np.all(np.abs(np.linalg.norm(n, axis=-1) - 1) <= 4 * np.finfo(np.float32).eps)
    assert np.all(np.einsum("nkc,nc->nk", d, n) > 0)
    assert np.array_equal(got["rays"]["o"], np.broadcast_to(got["pos"][:, None, :], d.shape))
    cos = np.einsum("nkc,nc->nk", d, n)
    assert np.allclose(got["rays"]["t_min"], 1e-4 / np.maximum(cos, 1e-5), rtol=1e-3)


def test_directions_are_cosine_distributed(scenes):
    """Over N = 65536 draws at one point: E[cos] = 2/3 with sigma = sqrt(1/18), so the mean lies within 6 sigma / sqrt(N) = 0.0055;
    a tangential component has mean 0 and standard deviation 0.5, so its mean lies within 6 * 0.5 / sqrt(N) = 0.012."""
    N = 65536
    pt = np.zeros(1, dtype=spt.BAKE_WORLD_DTYPE)
    nrm = np.array([0.36, 0.48, 0.8])
    pt["n"] = nrm
    got = spt.bake_rays(scenes["cfg2_cube"], pt, samples=N, seed=123, world=True)
    d, n = got["rays"]["d"][0].astype(np.float64), got["nrm"][0].astype(np.float64)
    cos = d @ n
    assert np.all(cos > 0)
    assert abs(cos.mean() - 2 / 3) <= 6 * np.sqrt(1 / 18) / np.sqrt(N)
    t1 = np.cross(n, [0.0, 1.0, 0.0])
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(n, t1)
    assert abs((d @ t1).mean()) <= 6 * 0.5 / np.sqrt(N) and abs((d @ t2).mean()) <= 6 * 0.5 / np.sqrt(N)


# ---- the rasteriser

def uv_of(scene, pts):
    uv = scene.array("tri_attr")["uv"][pts["prim"]].astype(np.float64)
    v, w = pts["v"].astype(np.float64)[:, None], pts["w"].astype(np.float64)[:, None]
    return uv[:, 0] * (1 - v - w) + uv[:, 1] * v + uv[:, 2] * w


@pytest.mark.parametrize("size", [(16, 16), (13, 7), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_a_plane_that_tiles_the_unit_square_covers_every_texel_once(scenes, size):
    scene = scenes["t_textured"]
    W, H = size
    pts, texels = scene.lightmap_points("floor", W, H)
    assert np.array_equal(texels, np.arange(W * H, dtype=np.uint32))     # every texel, once, in texel order
    assert np.all(pts["instance"] == scene.instance_index("floor"))
    m = scene.array("meshes")[scene.array("instances")[scene.instance_index("floor")]["prim_id"]]
    assert np.all((pts["prim"] >= m["tri_first"]) & (pts["prim"] < m["tri_first"] + m["tri_count"]))
    centre = np.stack([(texels % W + 0.5) / W, (texels // W + 0.5) / H], axis=-1)
    assert np.all(np.abs(uv_of(scene, pts) - centre) <= 1e-6)
    # a centre on the shared diagonal belongs to the lower triangle index
    uv = scene.array("tri_attr")["uv"][m["tri_first"]:m["tri_first"] + m["tri_count"]].astype(np.float64)
    for k in np.flatnonzero(np.isclose(centre[:, 0], centre[:, 1], atol=0, rtol=0)):
        assert pts["prim"][k] == m["tri_first"]
    assert uv.shape == (2, 3, 2)
    # the points are valid bake points
    spt.bake_rays(scene, pts, samples=1)


def half_square_scene(tmp_path):
    (tmp_path / "models").mkdir()
    (tmp_path / "models" / "half.obj").write_text(
        "v -1 0 -1\nv -1 0 1\nv 1 0 1\nv 1 0 -1\nvt 0 0\nvt 0 1\nvt 0.5 1\nvt 0.5 0\nvt 0.25 0.25\nvn 0 1 0\n"
        "f 1/5/1 2/5/1 3/5/1\nf 1/1/1 2/2/1 3/3/1\nf 1/1/1 3/3/1 4/4/1\n")
    src = json.load(open(os.path.join(_util.SCENES, "cfg2_cube.json")))
    src["primitives"] = [{"type": "trimesh", "name": "half", "obj_file": "models/half.obj"}]
    src["instances"] = [{"name": "quad", "primitive": "half", "material": "mat_cube"}]
    path = tmp_path / "half.json"
    path.write_text(json.dumps(src))
    return str(path)


def test_a_mesh_over_half_the_square_gives_the_analytic_count(tmp_path):
    _util.ensure_cpu_build()
    scene = spt.load_scene(half_square_scene(tmp_path))
    try:
        W, H = 16, 8
        pts, texels = scene.lightmap_points("quad", W, H)
        # centres with u = (x + 0.5) / 16 <= 0.5: x = 0 .. 7, every row; the zero-area uv triangle covers nothing
        assert len(pts) == 8 * H and np.array_equal(texels, np.array([y * W + x for y in range(H) for x in range(8)], dtype=np.uint32))
        centre = np.stack([(texels % W + 0.5) / W, (texels // W + 0.5) / H], axis=-1)
        assert np.all(np.abs(uv_of(scene, pts) - centre) <= 1e-6)
        # capacity 0 only counts
        lib, n = spt.host_lib(), C.c_uint64(0)
        assert lib.spt_host_lightmap_points(scene._h, b"quad", W, H, None, None, 0, C.byref(n)) == 0 and n.value == 8 * H
        # a short capacity writes that many records and still reports the count
        few, idx = np.zeros(5, dtype=spt.BAKE_POINT_DTYPE), np.zeros(5, dtype=np.uint32)
        assert lib.spt_host_lightmap_points(scene._h, b"quad", W, H, few.ctypes.data, idx.ctypes.data, 5, C.byref(n)) == 0 and n.value == 8 * H
        assert np.array_equal(words(few), words(pts[:5])) and np.array_equal(idx, texels[:5])
        assert lib.spt_host_lightmap_points(scene._h, b"nobody", W, H, None, None, 0, C.byref(n)) != 0
        assert lib.spt_host_lightmap_points(scene._h, b"quad", 0, H, None, None, 0, C.byref(n)) != 0
    finally:
        scene.close()


def test_a_sphere_instance_has_no_lightmap(scenes):
    with pytest.raises(spt.SptError):
        scenes["t_materials"].lightmap_points("gold", 4, 4)


# ---- the predicate

def test_the_predicate_refuses_bad_points(scenes):
    scene = scenes["t_materials"]
    inst, meshes = scene.array("instances"), scene.array("meshes")
    good = surface_points(scene, 2, 1)
    spt.bake_rays(scene, good, samples=1)
    sphere = int(np.flatnonzero(inst["prim_type"] == 0)[0])
    cube_inst = int(np.flatnonzero((inst["prim_type"] == 1) & (inst["prim_id"] == 0))[0])
    other = meshes[1]

    def refused(at, **fields):
        pts = good.copy()
        for k, v in fields.items():
            pts[k][at] = v
        with pytest.raises(spt.SptError) as e:
            spt.bake_rays(scene, pts, samples=1)
        assert e.value.status == 1 and ("point %d " % at) in str(e.value)

    refused(1, instance=sphere)
    refused(0, instance=cube_inst, prim=other["tri_first"])                        # a triangle of another mesh
    refused(3, instance=cube_inst, prim=meshes[0]["tri_first"] + meshes[0]["tri_count"])
    refused(2, instance=len(inst))
    refused(2, instance=0xFFFFFFFF)
    refused(1, v=np.nan)
    refused(1, w=np.inf)
    wp = world_points(3, 1)
    for field, value in (("n", [0, 0, 0]), ("n", [np.nan, 0, 1]), ("p", [0, np.inf, 0])):
        bad = wp.copy()
        bad[field][2] = value
        with pytest.raises(spt.SptError) as e:
            spt.bake_rays(scene, bad, samples=1, world=True)
        assert "point 2 " in str(e.value)


def test_vertex_points_name_every_corner(scenes):
    scene = scenes["cfg2_cube"]
    pts = spt.vertex_points(scene, "cube")
    assert pts.shape == (12, 3)
    got = spt.bake_rays(scene, pts.reshape(-1), samples=1)
    tp, fwd = scene.array("tri_pos"), scene.array("instances")[0]["fwd"].astype(np.float64)
    for c, key in enumerate(("p0", "p1", "p2")):
        q = tp[key].astype(np.float64)
        want = fwd[0:3] * q[:, 0:1] + fwd[3:6] * q[:, 1:2] + fwd[6:9] * q[:, 2:3] + fwd[9:12]
        assert np.allclose(got["pos"].reshape(12, 3, 3)[:, c], want, atol=1e-5)


# ---- layout

@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path_factory.mktemp("bake_layout") / "bake_layout_check")
    src = os.path.join(_util.ROOT, "tests", "bake_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}


def test_the_binding_declares_the_headers_layout(c_layout):
    assert c_layout["SPT_ABI_VERSION"] == 14
    assert c_layout["sizeof.spt_bake_point"] == spt.BAKE_POINT_DTYPE.itemsize == 16
    assert c_layout["sizeof.spt_bake_world_point"] == spt.BAKE_WORLD_DTYPE.itemsize == 32
    assert c_layout["sizeof.spt_bake_job"] == C.sizeof(spt.BakeJob)
    for f in ("instance", "prim", "v", "w"):
        assert c_layout["spt_bake_point." + f] == spt.BAKE_POINT_DTYPE.fields[f][1]
    for f in ("p", "pad0", "n", "pad1"):
        assert c_layout["spt_bake_world_point." + f] == spt.BAKE_WORLD_DTYPE.fields[f][1]
    for f, _ in spt.BakeJob._fields_:
        assert c_layout["spt_bake_job." + f] == getattr(spt.BakeJob, f).offset, f
    assert (c_layout["SPT_BAKE_DEVICE_POINTERS"], c_layout["SPT_BAKE_FLIP"], c_layout["SPT_BAKE_POINTS_WORLD"]) == \
        (spt.BAKE_DEVICE_POINTERS, spt.BAKE_FLIP, spt.BAKE_POINTS_WORLD)


def test_the_salt_is_a_stream_of_its_own():
    text = open(os.path.join(_util.ROOT, "include", "spt_abi.h")).read()
    assert "#define SPT_BAKE_SEED_SALT 0x%Xull" % _bake_ref.SALT in text
    assert _bake_ref.SALT != 0x4C454E5343414D31   # SPT_CAMERA_SEED_SALT


# ---- the CLI's refusals (before any device is touched)

@pytest.mark.parametrize("extra", [
    ["--preview-every", "2"], ["--denoise"], ["--robust", "3"], ["--variance-out", "v.exr"], ["--panorama"], ["--orthographic", "3"],
    ["--animate", "frames.json"], ["--gpus", "2"], ["--devices", "0"], ["--film-devices", "0,0", "--time-limit", "1"],
], ids=lambda e: e[0])
def test_the_cli_refuses_a_lightmap_beside_another_mode(tmp_path, extra):
    cli = os.path.join(spt.LIB_DIR, "spt")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-s", "-C", _util.ROOT, "cli"])
    base = [cli, "-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(tmp_path / "map.exr")]
    res = subprocess.run(base + ["--bake-lightmap", "cube", "--bake-size", "16x16"] + extra, capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "--bake-lightmap" in res.stderr, res.stdout + res.stderr
    assert not (tmp_path / "map.exr").exists()


def test_the_cli_needs_a_size_for_a_lightmap(tmp_path):
    cli = os.path.join(spt.LIB_DIR, "spt")
    base = [cli, "-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(tmp_path / "map.exr")]
    for extra in (["--bake-lightmap", "cube"], ["--bake-size", "16x16"], ["--bake-lightmap", "cube", "--bake-size", "16"],
                  ["--bake-lightmap", "cube", "--bake-size", "16x0"], ["--bake-lightmap", "cube", "--bake-size", "16x16", "--bake-samples", "0"]):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert res.returncode == 2, res.stdout + res.stderr


# ---- the stand-alone program under AddressSanitizer + UBSan

def test_the_sanitizer_program_runs_clean():
    res = subprocess.run(["make", "-s", "-C", _util.ROOT, "bake-check"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run([os.path.join(_util.ROOT, "build", "selftest", "bake_check"), os.path.join(_util.SCENES, "t_materials.json"), "floor", "red_cube",
                          "panel", os.path.join(_util.SCENES, "t_textured.json"), "floor", "c", os.path.join(_util.SCENES, "t_medium.json"), "blob"],
                         capture_output=True, text=True, timeout=120)
    report = res.stdout + res.stderr
    assert res.returncode == 0, report
    assert "bake_check ok" in res.stdout, report
    for word in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer", "CHECK failed"):
        assert word not in report, report

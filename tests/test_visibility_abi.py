"""spt_occluded and spt_ao without a device: the layout of their structs (include/spt_abi.h as a C compiler sees it, against the
binding's ctypes and numpy declarations), the exports of both libraries, the refusals of the command-line program that come before
any device is touched, the packing helpers, and tests/_visibility_ref.py over the CPU oracle: the expected records of the GPU tests
are shown here to be neither all open nor all closed."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _util
import _visibility_ref as ref

spt = _util.load_pkg()
f32 = np.float32

W, H, S, SEED = 48, 36, 4, 11
CAMERAS = {"cfg2_cube": None, "t_materials": "main", "t_textured": None}


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path_factory.mktemp("visibility_layout") / "visibility_layout_check")
    src = os.path.join(_util.ROOT, "tests", "visibility_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}


def test_the_ao_record_is_two_16_byte_words(c_layout):
    assert c_layout["sizeof.spt_ao_rec"] == spt.AO_DTYPE.itemsize == 32
    want = {"sum": 0, "open": 12, "bent": 16, "count": 28}
    assert list(spt.AO_DTYPE.names) == list(want)
    for f, off in want.items():
        assert c_layout["spt_ao_rec." + f] == spt.AO_DTYPE.fields[f][1] == off, f
    for f, kind in (("sum", "<f4"), ("open", "<f4"), ("bent", "<f4"), ("count", "<u4")):
        assert spt.AO_DTYPE.fields[f][0].base == np.dtype(kind), f
    assert c_layout["sizeof.spt_ray"] == spt.RAY_DTYPE.itemsize == 32
    for f in ("o", "t_min", "d", "t_max"):
        assert c_layout["spt_ray." + f] == spt.RAY_DTYPE.fields[f][1], f
    assert (c_layout["sizeof.spt_bake_point"], c_layout["sizeof.spt_bake_world_point"]) == (spt.BAKE_POINT_DTYPE.itemsize, spt.BAKE_WORLD_DTYPE.itemsize)


def test_the_binding_declares_the_headers_jobs(c_layout):
    assert c_layout["SPT_ABI_VERSION"] == spt.SPT_ABI_VERSION == 14
    assert c_layout["sizeof.spt_occluded_job"] == C.sizeof(spt.OccludedJob) == 40
    want = {"size": 0, "flags": 4, "n_rays": 8, "rays": 16, "out": 24, "rays_per_pass": 32, "pad": 36}
    assert [f for f, _ in spt.OccludedJob._fields_] == list(want)
    for f, off in want.items():
        assert c_layout["spt_occluded_job." + f] == getattr(spt.OccludedJob, f).offset == off, f
    assert c_layout["sizeof.spt_ao_job"] == C.sizeof(spt.AoJob) == 72
    want = {"size": 0, "flags": 4, "kind": 8, "pad": 12, "n_points": 16, "points": 24, "out": 32, "samples": 40, "max_distance": 44, "seed": 48,
            "first_point": 56, "first_sample": 60, "points_per_pass": 64, "pad1": 68}
    assert [f for f, _ in spt.AoJob._fields_] == list(want)
    for f, off in want.items():
        assert c_layout["spt_ao_job." + f] == getattr(spt.AoJob, f).offset == off, f
    assert (c_layout["SPT_OCCLUDED_DEVICE_POINTERS"], c_layout["SPT_OCCLUDED_PACKED"]) == (spt.OCCLUDED_DEVICE_POINTERS, spt.OCCLUDED_PACKED) == (1, 2)
    assert (c_layout["SPT_AO_DEVICE_POINTERS"], c_layout["SPT_AO_FLIP"]) == (spt.AO_DEVICE_POINTERS, spt.AO_FLIP) == (1, 2)
    assert c_layout["SPT_AO_FLIP"] == c_layout["SPT_BAKE_FLIP"] == spt.BAKE_FLIP


def test_both_libraries_export_both_calls():
    lib = spt.hip_lib()
    bez = C.CDLL(os.path.join(spt.LIB_DIR, "libspt_hip_bez.so"))
    for name in ("spt_occluded", "spt_ao"):
        assert hasattr(lib, name) and hasattr(bez, name), name
    # the refusals that need no scene
    job = spt.OccludedJob(size=C.sizeof(spt.OccludedJob))
    assert lib.spt_occluded(None, C.byref(job)) == 1      # SPT_ERR_INVALID_ARG
    assert b"occluded" in lib.spt_last_error()
    ao = spt.AoJob(size=C.sizeof(spt.AoJob), samples=1, max_distance=1.0)
    assert lib.spt_ao(None, C.byref(ao)) == 1
    assert b"ao" in lib.spt_last_error()


def test_packing_round_trip():
    rng = np.random.default_rng(5)
    for n in (0, 1, 63, 64, 65, 257, 1000):
        occ = (rng.random(n) < 0.4).astype(np.uint8)
        words = spt.pack_occluded(occ)
        assert words.dtype == np.dtype("<u8") and words.shape == ((n + 63) // 64,)
        for i in range(n):      # the specification, bit by bit
            assert (int(words[i >> 6]) >> (i & 63)) & 1 == occ[i]
        if n % 64:
            assert int(words[-1]) >> (n % 64) == 0
        assert np.array_equal(spt.unpack_occluded(words, n), occ)
        assert np.array_equal(spt.unpack_occluded(words.view(np.int64), n), occ)      # (the torch result's dtype)


# ---- the reference over the CPU oracle: not trivial

@functools.lru_cache(maxsize=None)
def _scene(name):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_util.SCENES, name + ".json"))


@functools.lru_cache(maxsize=None)
def _grid_points(name):
    """The mesh hits of the 48 x 36 camera grid, found by the oracle, as SURFACE points."""
    scene = _scene(name)
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=1, seed=SEED)
    pr = spt.camera_rays(spt.CameraModel.perspective(scene.get_camera(CAMERAS[name])), r, W, H).reshape(-1)
    hits = _util.OracleScene(scene).trace_closest(_util.first_segments(pr))
    inst = scene.array("instances")
    on_mesh = (hits["instance"] >= 0) & (inst["prim_type"][np.maximum(hits["instance"], 0)] == 1)
    pts = np.zeros(int(on_mesh.sum()), dtype=spt.BAKE_POINT_DTYPE)
    for f in ("instance", "prim", "v", "w"):
        pts[f] = hits[f][on_mesh]
    return pts


@pytest.mark.parametrize("name,n_points", [("t_materials", 502), ("t_textured", 529)])
def test_the_expected_records_are_not_trivial(name, n_points):
    scene = _scene(name)
    pts = _grid_points(name)
    assert len(pts) == n_points
    made = spt.bake_rays(scene, pts, samples=S, seed=SEED)
    oracle = _util.OracleScene(scene)
    for dist in (np.inf, ref.scene_extent(scene) / f32(16)):
        rec = ref.ao_records(spt, made, oracle.trace_any, dist)
        share = 1.0 - rec["count"].sum() / (S * len(pts))
        by_count = np.bincount(rec["count"], minlength=S + 1)
        print("%s, max_distance %g: occluded share %.3f, points by count %s" % (name, dist, share, by_count.tolist()))
        assert 0.2 <= share <= 0.6
        if not np.isfinite(dist):
            assert len(by_count) == S + 1 and (by_count > 0).all()
        # the record's own consistency
        assert np.array_equal(rec["open"], rec["count"].astype(f32) * f32(0.25))
        some = rec["count"] > 0
        assert np.allclose(np.linalg.norm(rec["bent"][some], axis=-1), 1.0, atol=1e-6) and not rec["bent"][~some].any() and not rec["sum"][~some].any()
        # a bent normal lies on the normal's side: every unoccluded direction does
        assert (np.einsum("ij,ij->i", rec["bent"][some], made["nrm"][some]) > 0).all()


def test_a_convex_body_in_the_void_is_all_open_and_all_closed_inside():
    name = "cfg2_cube"
    scene = _scene(name)
    pts = _grid_points(name)
    assert len(pts) == 241
    oracle = _util.OracleScene(scene)
    made = spt.bake_rays(scene, pts, samples=S, seed=SEED)
    for dist in (np.inf, ref.scene_extent(scene) / f32(16)):
        rec = ref.ao_records(spt, made, oracle.trace_any, dist)
        assert (rec["count"] == S).all() and (rec["open"] == 1).all()
    inward = spt.bake_rays(scene, pts, samples=S, seed=SEED, flip=True)
    rec = ref.ao_records(spt, inward, oracle.trace_any)
    assert (rec["count"] == 0).all() and not ref.words(rec)[:, :7].any()


# ---- the command-line program's refusals (before any device is touched)

def _cli():
    cli = os.path.join(spt.LIB_DIR, "spt")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-s", "-C", _util.ROOT, "cli"])
    return [cli, "-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json")]


@pytest.mark.parametrize("extra", [
    ["--preview-every", "2"], ["--time-limit", "1"], ["--variance-out", "v.exr"], ["--adaptive", "0.1"], ["--samples-out", "c.exr"], ["--denoise"],
    ["--robust", "3"], ["--film-devices", "0"], ["--lens-radius", "0.1", "--focus-distance", "2"], ["--orthographic", "2"], ["--panorama"],
    ["--animate", "frames.json"], ["--debug-normal"], ["--gpus", "1"], ["--devices", "0"], ["--bake-lightmap", "cube"], ["--bake-probes", "points.txt"],
    ["--gbuffer-out", "g"],
], ids=lambda e: e[0])
def test_the_cli_refuses_an_ao_bake_beside_another_mode(tmp_path, extra):
    res = subprocess.run(_cli() + ["-o", str(tmp_path / "ao.exr"), "--bake-ao", "cube", "--bake-size", "16x16"] + extra, capture_output=True, text=True,
                         timeout=60, cwd=str(tmp_path))
    assert res.returncode == 2 and "--bake-ao" in res.stderr, res.stdout + res.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("args,word", [
    (["--bake-ao", "cube"], "--bake-size"), (["--bake-ao", "cube", "--bake-size", "16"], "--bake-size"),
    (["--bake-ao", "cube", "--bake-size", "16x16", "--ao-samples", "0"], "--ao-samples"),
    (["--bake-ao", "cube", "--bake-size", "16x16", "--ao-samples", "16777217"], "--ao-samples"),
    (["--bake-ao", "cube", "--bake-size", "16x16", "--ao-distance", "0"], "--ao-distance"),
    (["--bake-ao", "cube", "--bake-size", "16x16", "--ao-distance", "nan"], "--ao-distance"),
    (["--ao-samples", "4"], "--bake-ao"), (["--ao-distance", "1"], "--bake-ao"), (["--bent-out", "b.exr"], "--bake-ao"),
], ids=lambda a: " ".join(a) if isinstance(a, list) else None)
def test_the_cli_checks_the_ao_options(tmp_path, args, word):
    res = subprocess.run(_cli() + ["-o", str(tmp_path / "ao.exr")] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 2 and word in res.stderr, res.stdout + res.stderr
    assert os.listdir(tmp_path) == []

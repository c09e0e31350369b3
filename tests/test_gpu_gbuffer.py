"""spt_gbuffer (DeviceScene.gbuffer, camera_gbuffer, `spt --gbuffer-out`): first-hit surface records along caller rays, word for word.

Expected records come from tests/_gbuffer_ref.py, never from the code under test: hits from oracle_trace_closest under
device_oracle_flags(), p and flags restated in float32 numpy, albedo from oracle_radiance over the emissive stand-in of
tests/_albedo_ref.py, mesh normals from _bake_ref.resolve, sphere normals restated from the records (tests/test_gbuffer_abi.py holds
both to the oracle's debug-normal film on the CPU).  A patch hit has no reference normal for rays of any origin: its n words and its
BACKFACING bit alone are left out of the record comparison, and the normals of every primitive kind are compared on pinhole rays with
the oracle's SPT_RENDER_DEBUG_NORMAL film.  Comparisons are of words (uint32): no tolerance.  The batches are those of
tests/_anywhere_ref.py, at most about 2 500 rays (the `big` one 16 641)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _anywhere_ref as ref
import _gbuffer_ref as G
import _scene_deform_scenes as SD
import _scene_update_scenes as SU
import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32
INVALID_ARG, UNSUPPORTED = 1, 4
PATTERN = 0xA5C3F00D
CLI = os.path.join(spt.LIB_DIR, "spt")


def _ds(name):
    return ref.scene(name).device_scene(0)


@functools.lru_cache(maxsize=None)
def _batch(name, kind, flags):
    """(rays, aux, expected records, n_known) of an _anywhere_ref batch; read-only.  `flags`: the oracle configuration (cache key)."""
    assert flags == _util.device_oracle_flags()
    rays, aux, _ = ref.make(name, kind)
    want, known = G.expected(ref.scene(name), rays, aux)
    for a in (rays, aux, want, known):
        if a is not None:
            a.setflags(write=False)
    return rays, aux, want, known


def _compare(name, kind, ds=None, **kw):
    rays, aux, want, known = _batch(name, kind, _util.device_oracle_flags())
    got = (_ds(name) if ds is None else ds).gbuffer(rays, aux, **kw)
    assert got.dtype == spt.GBUFFER_DTYPE and got.shape == want.shape
    why = G.difference(got, want, known)
    assert why is None, "%s, %s: %s" % (name, kind, why)
    return got


def _same_records(a, b):
    return a.shape == b.shape and np.array_equal(G.words(a), G.words(b))


# ---- 1. whole records ---------------------------------------------------------------------------------------------------------------

CASES = [("cfg2_cube", "free"), ("cfg2_cube", "axes"), ("cfg2_cube", "surface:t0"),
         ("t_materials", "free"), ("t_materials", "world"), ("t_materials", "thin_lens"), ("t_materials", "axes"),
         ("t_textured", "thin_lens"), ("t_textured", "thin_lens:noaux"), ("t_textured", "orthographic"), ("t_textured", "free"),
         ("t_pndf", "thin_lens"), ("t_plastic", "free"), ("t_subsurface", "free"), ("t_medium", "free"),
         ("t_bezier", "thin_lens"), ("t_bezier", "world")]


@pytest.mark.parametrize("name,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_records_are_the_references(name, kind):
    rays, aux, want, known = _batch(name, kind, _util.device_oracle_flags())
    share, distinct = G.census(want)
    hit = want["instance"] >= 0
    print("%s, %s: %d rays, hit share %.2f, %d distinct albedos, %d backfacing, %d on lights, n known for %.0f %%"
          % (name, kind, rays.shape[0], share, distinct, int((want["flags"] & spt.GBUF_BACKFACING != 0).sum()),
             int((want["flags"] & spt.GBUF_LIGHT != 0).sum()), 100 * known.mean()))
    assert hit.any() and (~hit).any()
    # the expected values alone: no trivial batch
    if (name, kind) in (("t_materials", "free"), ("t_materials", "thin_lens"), ("t_materials", "axes"), ("t_textured", "free"), ("t_textured", "thin_lens"),
                        ("t_bezier", "thin_lens")):
        assert share >= 0.15
    if name == "t_textured" and kind in ("free", "thin_lens"):
        assert distinct >= 50
    if name != "t_bezier":
        assert known.all()
    if kind == "thin_lens:noaux":      # the footprint matters to the reference
        assert aux is None and not _same_records(want, _batch(name, "thin_lens", _util.device_oracle_flags())[2])
    _compare(name, kind)


# ---- 2. normals of every primitive kind, on pinhole rays ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["t_materials", "t_textured", "t_bezier"])
def test_pinhole_normals_are_the_oracles_debug_normals(name):
    scene = ref.scene(name)
    rays, film = G.debug_normal_words(scene, 48, 36, camera=ref.CAMERAS[name])
    hits = _util.oracle_trace_closest(scene, _util.first_segments(rays), _util.device_oracle_flags())
    hit = hits["instance"] >= 0
    kinds = scene.array("instances")["prim_type"][np.maximum(hits["instance"], 0)][hit]
    assert hit.sum() >= 800 and len(np.unique(kinds)) >= 2, (int(hit.sum()), np.unique(kinds))
    got = _ds(name).gbuffer(rays)
    assert np.array_equal(got["instance"], np.where(hit, hits["instance"], -1))
    w = got["n"] * f32(0.5) + f32(0.5)
    bad = (w.view(np.uint32) != film.view(np.uint32)).any(axis=-1) & hit
    assert not bad.any(), "%d of %d hit pixels differ, first %d: %r against %r" % (int(bad.sum()), int(hit.sum()), int(np.flatnonzero(bad)[0]),
                                                                                 w[bad][0], film[bad][0])
    assert np.array_equal(got["flags"][hit] >> 8, kinds)


# ---- 3. scene forms -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("switches", [{"SPT_NO_LDS_GEO": "1"}, {"SPT_NO_LDS_GEO": "1", "SPT_NO_STREAM": "1"}, {"SPT_REFERENCE_BVH": "1"}],
                         ids=["stream", "memory", "reference_bvh"])
@pytest.mark.parametrize("name", ["t_materials", "t_textured"])
def test_scene_forms(monkeypatch, switches, name):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)      # (read when the device scene is made; SPT_REFERENCE_BVH also picks the oracle's configuration)
    sc = spt.load_scene(os.path.join(_util.SCENES, name + ".json"))
    try:
        for kind in ("thin_lens", "free"):
            _compare(name, kind, ds=sc.device_scene(0))
    finally:
        sc.close()


# ---- 4. cutting ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cut_batch():
    """2 500 rays of t_textured with their auxiliary rays (the thin lens' and 772 of the orthographic view's) and the uncut call's records."""
    a, b = ref.make("t_textured", "thin_lens"), ref.make("t_textured", "orthographic")
    rays, aux = np.concatenate([a[0], b[0][:772]]), np.concatenate([a[1], b[1][:772]])
    assert rays.shape[0] == 2500
    uncut = _ds("t_textured").gbuffer(rays, aux)
    want, known = G.expected(ref.scene("t_textured"), rays, aux)
    assert G.difference(uncut, want, known) is None
    for x in (rays, aux, uncut):
        x.setflags(write=False)
    return rays, aux, uncut


@pytest.mark.parametrize("per_pass", [1000, 256, 1])
def test_passes_do_not_matter(per_pass):
    rays, aux, uncut = _cut_batch()
    assert _same_records(_ds("t_textured").gbuffer(rays, aux, rays_per_pass=per_pass), uncut)


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_short_calls(n):
    rays, aux, uncut = _cut_batch()
    assert _same_records(_ds("t_textured").gbuffer(rays[:n], aux[:n]), uncut[:n])
    assert _same_records(_ds("t_textured").gbuffer(rays[2500 - n:], aux[2500 - n:]), uncut[2500 - n:])


def test_a_shuffled_batch_gives_the_shuffled_records():
    rays, aux, uncut = _cut_batch()
    order = np.random.default_rng(4).permutation(rays.shape[0])
    assert _same_records(_ds("t_textured").gbuffer(rays[order], aux[order], rays_per_pass=700), uncut[order])


def test_16641_rays():
    rays, aux, want, known = _batch("t_materials", "big", _util.device_oracle_flags())
    assert rays.shape[0] == 16641 and G.census(want)[0] >= 0.15
    uncut = _compare("t_materials", "big")
    assert _same_records(_ds("t_materials").gbuffer(rays, rays_per_pass=5000), uncut)


def test_no_rays():
    got = _ds("cfg2_cube").gbuffer(np.zeros(0, dtype=spt.PATH_RAY_DTYPE))
    assert got.shape == (0,) and got.dtype == spt.GBUFFER_DTYPE


# ---- 5. device pointers -------------------------------------------------------------------------------------------------------------

_CHILD = r"""
import ctypes, os, sys
import torch                                  # before the package: the tensor path must work in a process torch initialised
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import _util
import _anywhere_ref as ref
spt = _util.load_pkg()
rays, aux, _ = ref.make("t_textured", "thin_lens")
n = rays.shape[0]
ds = ref.scene("t_textured").device_scene(0)
want = ds.gbuffer(rays, aux)
words = want.view(np.uint32).reshape(n, 16)
assert (want["instance"] >= 0).mean() > 0.15
dev = torch.device("cuda", 0)
t_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 12).copy()).to(dev)
t_aux = torch.from_numpy(aux.view(np.float32).reshape(n, 16).copy()).to(dev)
got = ds.gbuffer(t_rays, t_aux)
assert got.device == dev and got.shape == (n, 16) and got.dtype == torch.float32
assert np.array_equal(got.view(torch.int32).cpu().numpy().view(np.uint32), words), "tensor records differ from the host path"
assert np.array_equal(got.view(torch.int32)[:, 7].cpu().numpy(), want["instance"])
no_aux = ds.gbuffer(t_rays)
assert np.array_equal(no_aux.view(torch.int32).cpu().numpy().view(np.uint32), ds.gbuffer(rays).view(np.uint32).reshape(n, 16))
# a view one row into a larger allocation: the base address is not the allocation's
big_rays, big_aux = torch.zeros((n + 1, 12), dtype=torch.float32, device=dev), torch.zeros((n + 1, 16), dtype=torch.float32, device=dev)
big_rays[1:], big_aux[1:] = t_rays, t_aux
v_rays, v_aux = big_rays[1:], big_aux[1:]
assert v_rays.is_contiguous() and v_rays.data_ptr() == big_rays.data_ptr() + 48
got = ds.gbuffer(v_rays, v_aux, rays_per_pass=500)
assert np.array_equal(got.view(torch.int32).cpu().numpy().view(np.uint32), words), "records of a row-offset view differ"
# refusals: a misaligned tensor, a host pointer under the flag; `out` keeps its fill
lib = spt.hip_lib()
fill = torch.full((n, 16), 7.0, dtype=torch.float32, device=dev)
flat = torch.zeros(n * 12 + 1, dtype=torch.float32, device=dev)
odd = flat[1:].view(n, 12)
odd.copy_(t_rays)
host_out = np.full((n, 16), np.float32(7.0))
def refused(rays_ptr, aux_ptr, out_ptr, word):
    job = spt.GBufferJob(size=ctypes.sizeof(spt.GBufferJob), flags=spt.GBUFFER_DEVICE_POINTERS, n_rays=n)
    job.rays, job.aux, job.out = rays_ptr, aux_ptr, out_ptr
    assert lib.spt_gbuffer(ds._h, ctypes.byref(job)) == 1
    assert word in lib.spt_last_error().decode(), lib.spt_last_error()
    torch.cuda.synchronize()
    assert bool((fill == 7.0).all()) and (host_out == 7.0).all()
refused(odd.data_ptr(), None, fill.data_ptr(), "16-byte aligned")
refused(t_rays.data_ptr(), t_aux.data_ptr() + 4, fill.data_ptr(), "16-byte aligned")
refused(t_rays.data_ptr(), None, fill.data_ptr() + 8, "16-byte aligned")
refused(rays.ctypes.data, None, fill.data_ptr(), "not device memory")
refused(t_rays.data_ptr(), aux.ctypes.data, fill.data_ptr(), "not device memory")
refused(t_rays.data_ptr(), None, host_out.ctypes.data, "not device memory")
try:
    ds.gbuffer(odd)
    raise AssertionError("a misaligned tensor was taken")
except spt.SptError as e:
    assert e.status == 1
again = ds.gbuffer(t_rays, t_aux)
assert np.array_equal(again.view(torch.int32).cpu().numpy().view(np.uint32), words)
print("gbuffer tensors ok")
"""


def test_device_pointers_in_a_process_that_imported_torch_first():
    res = subprocess.run([sys.executable, "-c", _CHILD, _util.ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "gbuffer tensors ok" in res.stdout, res.stdout + res.stderr


# ---- 6. scene edits -----------------------------------------------------------------------------------------------------------------

def _path_rays(scene, n, seed):
    seg = _util.random_rays(scene, n, seed=seed, spread=3.0)
    rays = np.zeros(n, dtype=spt.PATH_RAY_DTYPE)
    rays["o"], rays["d"], rays["t_min"] = seg["o"], seg["d"], seg["t_min"]
    return rays


def _against_reference(scene, got, rays, what):
    want, known = G.expected(scene, rays)
    assert (want["instance"] >= 0).mean() > 0.15, what
    why = G.difference(got, want, known)
    assert why is None, "%s: %s" % (what, why)


def test_records_follow_moved_instances(tmp_path):
    _util.ensure_cpu_build()
    SU.write_scene(str(tmp_path), "a.json", SU.TRANSFORMS_A)
    SU.write_scene(str(tmp_path), "b.json", SU.TRANSFORMS_B)
    sc, fresh = spt.load_scene(str(tmp_path / "a.json")), spt.load_scene(str(tmp_path / "b.json"))
    try:
        rays = _path_rays(sc, 2048, 3)
        ds = sc.device_scene(0)
        first = ds.gbuffer(rays)
        _against_reference(sc, first, rays, "as loaded")
        sc.set_transforms(SU.fwd_by_name(fresh, sorted(SU.TRANSFORMS_A)))
        ds.update()
        after = ds.gbuffer(rays)
        assert _same_records(after, fresh.device_scene(0).gbuffer(rays)), "against a fresh scene"
        _against_reference(sc, after, rays, "after the update")
        assert not _same_records(after, first)
    finally:
        sc.close()
        fresh.close()


def test_records_follow_deformed_vertices(tmp_path):
    _util.ensure_cpu_build()
    SD.write_scene(str(tmp_path), "s.json")
    sc, fresh = spt.load_scene(str(tmp_path / "s.json")), spt.load_scene(str(tmp_path / "s.json"))
    try:
        rays = _path_rays(sc, 2048, 3)
        ds = sc.device_scene(0)
        first = ds.gbuffer(rays)
        _against_reference(sc, first, rays, "as loaded")
        for name, fn in SD.DEFORMED.items():
            pos = fn(sc.mesh_positions(name))
            sc.set_mesh_vertices(name, pos)
            fresh.set_mesh_positions(name, pos)
        ds.update()
        after = ds.gbuffer(rays)
        assert _same_records(after, fresh.device_scene(0).gbuffer(rays)), "against a fresh scene"
        _against_reference(fresh, after, rays, "after the deformation")
        assert not _same_records(after, first)
    finally:
        sc.close()
        fresh.close()


def test_an_open_film_is_left_alone():
    name = "t_materials"
    sc = ref.scene(name)
    r = spt.PathTracer(max_depth=ref.DEPTH, sampler=spt.SAMPLER_RANDOM, spp=4, seed=ref.SEED)
    cfg = spt.OutputConfig(ref.W, ref.H, None, ref.CAMERAS[name])
    rays, aux, want, known = _batch(name, "thin_lens", _util.device_oracle_flags())
    with r.progressive(sc, cfg, moments=True) as undisturbed:
        undisturbed.render(4)
        s, q = undisturbed.sum().copy(), undisturbed.sum_sq().copy()
    with r.progressive(sc, cfg, moments=True) as film:
        film.render(2)
        assert G.difference(_ds(name).gbuffer(rays, aux), want, known) is None
        film.render(2)
        assert _util.same_words(film.sum(), s) and _util.same_words(film.sum_sq(), q)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_leave_the_scene_usable():
    name = "cfg2_cube"
    rays, _, want, known = _batch(name, "free", _util.device_oracle_flags())
    rays = rays.copy()
    ds = _ds(name)
    lib = spt.hip_lib()
    n = rays.shape[0]
    out = np.empty(n, dtype=spt.GBUFFER_DTYPE)

    def job(rays_arr=rays, **kw):
        j = spt.GBufferJob(size=C.sizeof(spt.GBufferJob), n_rays=rays_arr.shape[0])
        j.rays, j.out = rays_arr.ctypes.data, out.ctypes.data
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(j, scene=ds._h, word=None, status=INVALID_ARG):
        out.view(np.uint32)[:] = PATTERN
        assert lib.spt_gbuffer(scene, C.byref(j) if j is not None else None) == status
        assert (out.view(np.uint32) == PATTERN).all()
        if word is not None:
            assert word in lib.spt_last_error().decode(), lib.spt_last_error()

    refused(job(), scene=None, word="null")
    refused(None, word="null")
    refused(job(rays=None), word="null rays or out")
    refused(job(out=None), word="null rays or out")
    refused(job(size=C.sizeof(spt.GBufferJob) - 8), word="size")
    refused(job(flags=2), word="unknown flags")
    refused(job(flags=0x80000000), word="unknown flags")
    refused(job(n_rays=(1 << 40) + 1), word="2^40", status=UNSUPPORTED)
    for field, value, word in (("o", np.nan, "non-finite"), ("d", np.inf, "non-finite"), ("t_min", -np.inf, "non-finite")):
        bad = rays.copy()
        bad[field][n // 2] = value
        refused(job(bad), word=word)
        assert ("ray %d " % (n // 2)) in lib.spt_last_error().decode()
    bad = rays.copy()
    bad["d"][n - 1] = 0.0
    refused(job(bad), word="all-zero direction")
    refused(job(bad, rays_per_pass=100), word="all-zero direction")      # the earlier passes ran: still nothing written
    refused(job(flags=spt.GBUFFER_DEVICE_POINTERS), word="not device memory")
    # n_rays == 0 is SPT_OK and does nothing, whatever the pointers
    out.view(np.uint32)[:] = PATTERN
    assert lib.spt_gbuffer(ds._h, C.byref(job(n_rays=0, rays=None, out=None))) == 0 and (out.view(np.uint32) == PATTERN).all()
    # a good call afterwards
    assert lib.spt_gbuffer(ds._h, C.byref(job())) == 0
    assert G.difference(out, want, known) is None


# ---- 8. camera_gbuffer and the command-line program ---------------------------------------------------------------------------------

W2, H2, N = 48, 32, 3


def _images(ds, model, renderer):
    """camera_gbuffer's images restated from gbuffer over camera_rays, in the stated order."""
    albedo, normal = np.zeros((H2, W2, 3), dtype=f32), np.zeros((H2, W2, 3), dtype=f32)
    t_sum, hits = np.zeros((H2, W2), dtype=f32), np.zeros((H2, W2), dtype=f32)
    for k in range(N):
        rays, aux = spt.camera_rays(model, renderer, W2, H2, k, 1, aux=True)
        rec = ds.gbuffer(rays.reshape(-1), aux.reshape(-1)).reshape(H2, W2)
        hit = rec["instance"] >= 0
        assert (rec["albedo"][~hit] == 0).all() and (rec["n"][~hit] == 0).all()
        albedo, normal = albedo + rec["albedo"], normal + rec["n"]
        t_sum = t_sum + np.where(hit, rec["t"], f32(0))
        hits = hits + hit.astype(f32)
    inv = f32(1) / f32(N)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(hits > 0, t_sum / hits, f32(0))
    return {"albedo": albedo * inv, "normal": normal * inv, "depth": depth.astype(f32), "coverage": hits / f32(N)}


@pytest.mark.parametrize("option", [["--lens-radius", "0.1", "--focus-distance", "4"], ["--panorama"]], ids=["thin_lens", "panorama"])
def test_camera_gbuffer_and_the_cli(option, tmp_path):
    name, seed = "cfg2_cube", 3
    scene_file, renderer_file = os.path.join(_util.SCENES, name + ".json"), os.path.join(_util.SCENES, "pt.json")
    sc = ref.scene(name)
    cam = sc.get_camera(None)
    model = spt.CameraModel.thin_lens(cam, 0.1, 4.0) if option[0] == "--lens-radius" else spt.CameraModel.panorama(cam.eye[:])
    ren = spt.load_renderer(renderer_file, seed=seed)
    ren.spp = 4
    want = _images(_ds(name), model, ren)
    # hits and misses (the cube fills about 1 % of its panorama: enough pixels, not a share); behind the lens, pixels some of whose samples hit
    assert (want["coverage"] > 0).sum() >= 3 and (want["coverage"] == 0).any() and (want["depth"] > 0).sum() >= 3
    if option[0] == "--lens-radius":
        assert want["coverage"].mean() > 0.1 and len(np.unique(want["coverage"])) >= 3
    got = spt.camera_gbuffer(sc, model, ren, W2, H2, samples=N)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key].dtype == f32 and _util.same_words(got[key], want[key]), key
    assert _util.same_words(spt.camera_gbuffer(_ds(name), model, ren, W2, H2, samples=N)["albedo"], want["albedo"])
    # the program: the three files alone without -o, and beside an unchanged image with it
    base = [CLI, "-s", scene_file, "-r", renderer_file, "-w", str(W2), "-h", str(H2), "--spp", "4", "--seed", str(seed)] + option
    stem = str(tmp_path / "g")
    res = subprocess.run(base + ["--gbuffer-out", stem, "--gbuffer-samples", str(N)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert sorted(os.listdir(tmp_path)) == ["g_albedo.exr", "g_depth.exr", "g_normal.exr"]
    assert _util.same_words(spt.read_exr(stem + "_albedo.exr"), want["albedo"])
    assert _util.same_words(spt.read_exr(stem + "_normal.exr"), want["normal"])
    depth = spt.read_exr(stem + "_depth.exr")
    assert _util.same_words(depth[..., 0], want["depth"]) and _util.same_words(depth[..., 1], want["coverage"]) and (depth[..., 2].view(np.uint32) == 0).all()
    plain, both = tmp_path / "plain.png", tmp_path / "both.png"
    for out, extra in ((plain, []), (both, ["--gbuffer-out", str(tmp_path / "h"), "--gbuffer-samples", str(N)])):
        res = subprocess.run(base + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
    assert plain.read_bytes() == both.read_bytes()
    assert (tmp_path / "h_albedo.exr").read_bytes() == (tmp_path / "g_albedo.exr").read_bytes()


def test_the_cli_takes_the_scenes_own_camera(tmp_path):
    """Without a camera-model option the rays are the pinhole's (SPT_CAMERA_PERSPECTIVE through spt_host_camera_rays)."""
    name, seed = "cfg2_cube", 3
    scene_file, renderer_file = os.path.join(_util.SCENES, name + ".json"), os.path.join(_util.SCENES, "pt.json")
    ren = spt.load_renderer(renderer_file, seed=seed)
    ren.spp = 4
    model = spt.CameraModel.perspective(ref.scene(name).get_camera(None))
    want = _images(_ds(name), model, ren)
    stem = str(tmp_path / "g")
    res = subprocess.run([CLI, "-s", scene_file, "-r", renderer_file, "-w", str(W2), "-h", str(H2), "--spp", "4", "--seed", str(seed), "--gbuffer-out", stem,
                          "--gbuffer-samples", str(N), "--device", "0"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert _util.same_words(spt.read_exr(stem + "_albedo.exr"), want["albedo"]) and _util.same_words(spt.read_exr(stem + "_normal.exr"), want["normal"])


@pytest.mark.parametrize("extra,word", [
    (["--gpus", "2"], "one device"), (["--devices", "0,0"], "one device"), (["--film-devices", "0,0", "--preview-every", "2"], "one device"),
    (["--animate", "frames.json"], "--animate"), (["--bake-lightmap", "cube", "--bake-size", "16x16"], "--bake-lightmap"),
    (["--bake-probes", "points.txt"], "--bake-probes"), (["--gbuffer-samples", "0"], "N >= 1"),
], ids=lambda e: e[0] if isinstance(e, list) else None)
def test_the_cli_refuses_a_gbuffer_beside_another_mode(tmp_path, extra, word):
    base = [CLI, "-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(tmp_path / "o.png")]
    res = subprocess.run(base + ["--gbuffer-out", str(tmp_path / "g")] + extra, capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "--gbuffer-" in res.stderr and word in res.stderr, res.stdout + res.stderr
    assert os.listdir(tmp_path) == []

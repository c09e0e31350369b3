"""Camera models without a device: spt_host_camera_rays (the header the device kernel includes) against tests/_camera_ref.py, word
for word; float64 pins of what each model means; the struct's layout in C and in the binding; the CLI's refusals."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _camera_ref
import _radiance_ref
import _util
import _wide_film_ref

spt = _util.load_pkg()
CLI = os.path.join(spt.LIB_DIR, "spt")
SIZES = [(7, 5), (33, 18)]
SAMPLERS = [spt.SAMPLER_RANDOM, spt.SAMPLER_RECURRENCE]
SPP, FIRST, COUNT = 6, 2, 3


@pytest.fixture(scope="module")
def scene():
    _util.ensure_cpu_build()
    sc = spt.load_scene(os.path.join(_util.SCENES, "cfg2_cube.json"))
    yield sc
    sc.close()


def models(scene):
    cam = scene.get_camera(None)
    return {
        "perspective": spt.CameraModel.perspective(cam),
        "thin_lens": spt.CameraModel.thin_lens(cam, 0.15, 4.5),
        "orthographic": spt.CameraModel.orthographic(cam, 3.0),
        "panorama": spt.CameraModel.panorama([0.25, 0.5, -1.0]),
    }


def renderer(sampler):
    return spt.PathTracer(max_depth=4, sampler=sampler, spp=SPP, seed=11)


def words(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("sampler", SAMPLERS, ids=["random", "recurrence"])
@pytest.mark.parametrize("kind", ["perspective", "thin_lens", "orthographic", "panorama"])
def test_host_rays_equal_the_restated_specification(scene, kind, sampler, size):
    w, h = size
    m, r = models(scene)[kind], renderer(sampler)
    want, want_aux = _camera_ref.plan_rays(spt, m, r, w, h, FIRST, COUNT, aux=True)
    got, got_aux = spt.camera_rays(m, r, w, h, first=FIRST, count=COUNT, aux=True)
    assert got.shape == (COUNT, h, w)
    for f in ("o", "t_min", "d", "stream_a", "stream_b", "pad"):
        assert np.array_equal(words(got[f]), words(want[f])), f
    for f in ("rx_o", "rx_d", "ry_o", "ry_d"):
        assert np.array_equal(words(got_aux[f]), words(want_aux[f])), f
    # aux off: the same rays; first = 0 and the default count: the whole plan, whose tail is the block above
    assert np.array_equal(words(spt.camera_rays(m, r, w, h, first=FIRST, count=COUNT)), words(got))
    whole = spt.camera_rays(m, r, w, h)
    assert whole.shape == (SPP, h, w) and np.array_equal(words(whole[FIRST:FIRST + COUNT]), words(got))


@pytest.mark.parametrize("sampler", SAMPLERS, ids=["random", "recurrence"])
def test_perspective_equals_the_oracle_camera(scene, sampler):
    w, h = 33, 18
    r = renderer(sampler)
    want, want_aux = _radiance_ref.plan_rays(spt, scene, r, w, h, FIRST, COUNT, aux=True)
    got, got_aux = spt.camera_rays(spt.CameraModel.perspective(scene.get_camera(None)), r, w, h, first=FIRST, count=COUNT, aux=True)
    assert np.array_equal(words(got), words(want))
    assert np.array_equal(words(got_aux), words(want_aux))


def screen64(r, w, h, first, count):
    off = _wide_film_ref.offsets(spt, r.seed, w, h, r.spp, r.sampler, first, count)
    x, y = _radiance_ref.screen_points(w, h, off)
    return x.astype(np.float64), y.astype(np.float64)


def cam64(cam):
    return [np.array(v[:], dtype=np.float64) for v in (cam.eye, cam.forward, cam.up, cam.right)] + [float(cam.half_cot_half_fov)]


def test_thin_lens_rays_meet_the_plane_of_focus_at_the_pinhole_point(scene):
    """Every ray meets the plane at focus_distance along forward where the pinhole ray through the same screen point does.
    Tolerance 1e-5 of focus_distance.  Derivation: in exact arithmetic o + (du*ft - lo) = eye + du*ft, the pinhole's point.  In f32,
    du takes 5 rounded operations per component, ft one, du*ft - lo two, lo three, o one, the normalisation five: about 17 roundings
    of relative size 2^-24 = 6e-8, each moving the point by at most that fraction of the ray's length to the plane (<= 1.5
    focus_distance at this field of view), together 1.5e-6 of focus_distance; the scene camera's f32 basis is orthonormal to
    about 1e-7.  1e-5 is that with room, and 1e4 times below what a wrong lens offset (radius 0.15) would give."""
    w, h, fd, radius = 33, 18, 4.5, 0.15
    r = renderer(spt.SAMPLER_RANDOM)
    cam = scene.get_camera(None)
    rays = spt.camera_rays(spt.CameraModel.thin_lens(cam, radius, fd), r, w, h, first=FIRST, count=COUNT)
    eye, fwd, up, right, hc = cam64(cam)
    x, y = screen64(r, w, h, FIRST, COUNT)
    du = fwd * hc + right * x[..., None] + up * y[..., None]
    focus = eye + du * (fd / hc)
    o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    t = (fd - ((o - eye) * fwd).sum(-1)) / (d * fwd).sum(-1)
    hit = o + d * t[..., None]
    err = np.abs(hit - focus).max()
    print("thin lens: worst distance from the pinhole point %.3g (focus_distance %.3g)" % (err, fd))
    assert err <= 1e-5 * fd
    lens = np.linalg.norm(o - eye, axis=-1)
    assert lens.max() <= radius * (1 + 1e-6) and lens.max() > 0.5 * radius and np.unique(words(rays["o"]).reshape(-1, 12), axis=0).shape[0] > 1


def test_orthographic_rays_are_parallel_and_span_the_view(scene):
    w, h, vh = 33, 18, 3.0
    r = renderer(spt.SAMPLER_RECURRENCE)
    cam = scene.get_camera(None)
    rays = spt.camera_rays(spt.CameraModel.orthographic(cam, vh), r, w, h)
    eye, fwd, up, right, _ = cam64(cam)
    assert np.array_equal(words(rays["d"]), words(np.broadcast_to(np.array(cam.forward[:], dtype=np.float32), rays["d"].shape)))
    rel = rays["o"].astype(np.float64) - eye
    u, v = (rel * right).sum(-1), (rel * up).sum(-1)
    aspect = w / h
    assert np.abs(u).max() <= vh * aspect / 2 * (1 + 1e-6) and np.abs(v).max() <= vh / 2 * (1 + 1e-6)
    # the samples reach within one pixel of every edge
    assert vh * aspect - (u.max() - u.min()) <= 2 * vh * aspect / w and vh - (v.max() - v.min()) <= 2 * vh / h
    assert np.abs((rel * fwd).sum(-1)).max() <= 1e-5


def test_panorama_angles(scene):
    """acos(d.y) and atan2(d.x, d.z) reproduce th and ph.  A unit vector's f32 components carry a few 2^-24 of absolute error
    (eps = 1e-6 covers the deterministic sin / cos and the normalisation); an angle read back from them is off by at most
    eps / sin(th), both angles being ill-conditioned at the poles alike."""
    w, h = 33, 18
    r = renderer(spt.SAMPLER_RANDOM)
    rays = spt.camera_rays(spt.CameraModel.panorama([0.25, 0.5, -1.0]), r, w, h)
    x, y = screen64(r, w, h, 0, SPP)
    th = (0.5 - y) * np.pi
    ph = x / (np.float64(np.float32(w) / np.float32(h))) * 2 * np.pi
    d = rays["d"].astype(np.float64)
    tol = 1e-6 / np.maximum(np.sin(th), 1e-9) + 1e-6
    dth = np.abs(np.arccos(np.clip(d[..., 1], -1, 1)) - th)
    dph = np.abs((np.arctan2(d[..., 0], d[..., 2]) - ph + np.pi) % (2 * np.pi) - np.pi)
    print("panorama: worst th error %.3g, worst ph error %.3g" % (dth.max(), dph.max()))
    assert (dth <= tol).all() and (dph <= tol).all()
    assert np.array_equal(words(rays["o"]), words(np.broadcast_to(np.array([0.25, 0.5, -1.0], dtype=np.float32), rays["o"].shape)))
    # row 0 starts at the +y pole, the image centre looks along +z
    assert d[:, 0, :, 1].min() > np.cos(np.pi / h) - 1e-6 and d[:, h // 2, w // 2, 2].min() > 0.9


def test_host_rays_refusals(scene):
    lib = spt.host_lib()
    cam = scene.get_camera(None)
    r = renderer(spt.SAMPLER_RANDOM)
    p = r.params(7, 5)
    rays = np.zeros((1, 5, 7), dtype=spt.PATH_RAY_DTYPE)
    bad = [spt.CameraModel.thin_lens(cam, -0.1, 1.0), spt.CameraModel.thin_lens(cam, 0.1, 0.0), spt.CameraModel.thin_lens(cam, float("nan"), 1.0),
           spt.CameraModel.orthographic(cam, 0.0), spt.CameraModel.orthographic(cam, float("inf")), spt.CameraModel._make(4, cam)]
    small = spt.CameraModel.panorama([0, 0, 0])
    small.size -= 4
    for m in bad + [small]:
        assert lib.spt_host_camera_rays(C.byref(m), C.byref(p), 0, 1, rays.ctypes.data, None) == 1
    assert lib.spt_host_camera_rays(None, C.byref(p), 0, 1, rays.ctypes.data, None) == 1
    assert lib.spt_host_camera_rays(C.byref(spt.CameraModel.panorama([0, 0, 0])), C.byref(p), SPP, 1, rays.ctypes.data, None) == 1   # past the plan


def test_struct_layout_in_c_and_ctypes(tmp_path):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path / "camera_model_layout_check")
    src = os.path.join(_util.ROOT, "tests", "camera_model_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    c = {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}
    M = spt.CameraModel
    assert c["sizeof.spt_camera_model"] == C.sizeof(M) == 76 and c["sizeof.spt_camera"] == C.sizeof(spt.Camera) == 52
    for f in ("size", "type", "base", "lens_radius", "focus_distance", "view_height", "pad"):
        assert c["spt_camera_model." + f] == getattr(M, f).offset, f
    assert c["SPT_ABI_VERSION"] == spt.SPT_ABI_VERSION == 14
    assert [c["SPT_CAMERA_" + n] for n in ("PERSPECTIVE", "THIN_LENS", "ORTHOGRAPHIC", "PANORAMA")] == \
        [spt.CAMERA_PERSPECTIVE, spt.CAMERA_THIN_LENS, spt.CAMERA_ORTHOGRAPHIC, spt.CAMERA_PANORAMA] == [0, 1, 2, 3]
    assert (c["SPT_CAMERA_SEED_SALT_HI"] << 32) | c["SPT_CAMERA_SEED_SALT_LO"] == spt.CAMERA_SEED_SALT == _camera_ref.SALT


def test_entry_points_and_null_arguments_need_no_device():
    _util.ensure_cpu_build()
    lib = spt.hip_lib()
    assert hasattr(lib, "spt_render_camera") and hasattr(lib, "spt_film_create_camera")
    p = spt.PathTracer(spp=4).params(8, 8)
    out = np.zeros((8, 8, 3), dtype=np.float32)
    film = C.c_void_p()
    assert lib.spt_render_camera(None, None, C.byref(p), out.ctypes.data, None) == 1
    assert lib.spt_film_create_camera(None, None, C.byref(p), 0, 0, C.byref(film)) == 1


def test_multi_device_classes_refuse_a_camera_model(scene):
    from test_multi_device import StubDevices
    m = spt.CameraModel.panorama([0, 0, 0])
    r = spt.PathTracer(spp=4)
    stub = StubDevices(scene)
    multi = spt.MultiDevice(scene, [0, 1], api=stub.api)
    try:
        with pytest.raises(spt.SptError):
            multi.render(r, spt.OutputConfig(16, 8), camera_model=m)
        with pytest.raises(spt.SptError):
            multi.progressive(r, spt.OutputConfig(16, 8), camera_model=m)
    finally:
        multi.close()


ARGS = ["-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-w", "32", "-h", "16", "--spp", "4"]
LENS = ["--lens-radius", "0.1", "--focus-distance", "4"]


ONE_MODEL, BOTH_LENS, ONE_DEVICE = "exclude each other (one camera model)", "a thin lens needs both", "a camera model (--lens-radius, --orthographic, --panorama) renders on one device"


@pytest.mark.parametrize("extra,message", [
    (LENS + ["--orthographic", "3"], ONE_MODEL), (LENS + ["--panorama"], ONE_MODEL), (["--orthographic", "3", "--panorama"], ONE_MODEL),
    (["--lens-radius", "0.1"], BOTH_LENS), (["--focus-distance", "4"], BOTH_LENS),
    (LENS + ["--gpus", "2"], ONE_DEVICE), (["--panorama", "--devices", "0,0"], ONE_DEVICE),
    (["--orthographic", "3", "--film-devices", "0,0", "--preview-every", "2"], ONE_DEVICE),
    (["--panorama", "--animate", "frames.json"], ONE_DEVICE), (LENS + ["--denoise", "--guide", "albedo"], ONE_DEVICE),
    (LENS + ["--denoise", "--guide", "both"], ONE_DEVICE),
    # what --film-devices is refused for without a camera model, it is refused for with one: the model does not hide it
    (["--panorama", "--film-devices", "0"], "--film-devices needs a progressive option"),
    (["--panorama", "--film-devices", "0", "--gpus", "1", "--preview-every", "2"], "--film-devices and --gpus / --devices exclude each other"),
    (["--panorama", "--film-devices", "x", "--preview-every", "2"], "--film-devices takes a list of device indices"),
], ids=lambda e: " ".join(e) if isinstance(e, list) else None)
def test_cli_refuses_the_excluded_combinations(tmp_path, extra, message):
    """Exit code 2 with the refusal's own message on stderr (an option the program does not know also exits with 2, through the usage text)."""
    res = subprocess.run([CLI] + ARGS + ["-o", str(tmp_path / "o.png")] + extra, capture_output=True, text=True, timeout=60)
    assert res.returncode == 2, res.stderr
    assert "Error: " in res.stderr and message in res.stderr, res.stderr
    assert not (tmp_path / "o.png").exists()


def test_a_bucket_count_in_the_models_position_is_refused(scene):
    """`buckets` stays the last keyword of PathTracer.progressive; a count passed by position where camera_model now sits is an error, not a model."""
    r = spt.PathTracer(spp=4)
    with pytest.raises(TypeError, match="buckets= by keyword"):
        r.progressive(scene, spt.OutputConfig(8, 8), 0, 0, False, 0, 1, 16, 0, 0, False, 5)

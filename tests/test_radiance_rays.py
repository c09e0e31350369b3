"""The ray generators of the binding (perspective_rays, orthographic_rays, panorama_rays, thin_lens_rays) on the CPU.

perspective_rays promises the camera rays of a plan bit for bit: it is held to oracle_camera_ray at the screen points of
pt.rs:269-271 (tests/_radiance_ref.py restates those from the oracle's own pixel offsets), and its auxiliary rays to the same
function at x + aux_dx / y + aux_dy.  The other generators promise unit directions and their documented conventions.  A direction
normalised in float64 and rounded once has |d|^2 within 2 u = 2^-23 of 1 (u = 2^-24 per component, 2 u sum c_i^2 in the square):
one ulp of 1.0f, measured here in float64 on the float32 components."""
import numpy as np
import pytest

import _radiance_ref
import _util
import _wide_film_ref

spt = _util.load_pkg()
f32 = np.float32
W, H = 24, 18


@pytest.fixture(scope="module")
def scene():
    _util.ensure_cpu_build()
    sc = spt.load_scene(_util.SCENES + "/t_textured.json")
    yield sc
    sc.close()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("sampler", [spt.SAMPLER_RECURRENCE, spt.SAMPLER_RANDOM], ids=["recurrence", "random"])
def test_perspective_rays_are_the_oracles_camera_rays(scene, sampler):
    renderer = spt.PathTracer(max_depth=5, sampler=sampler, spp=4, seed=7)
    cam = scene.get_camera("main")
    off = _wide_film_ref.offsets(spt, renderer.seed, W, H, renderer.spp, sampler, 1, 3)
    rays, aux = spt.perspective_rays(cam, W, H, off, aux_spp=renderer.spp, first_sample=1)
    ref, ref_aux = _radiance_ref.plan_rays(spt, scene, renderer, W, H, 1, 3, camera="main", aux=True)
    assert rays.shape == (3, H, W) and aux.shape == (3, H, W)
    for field in ("o", "t_min", "d", "stream_a", "stream_b", "pad"):
        assert np.array_equal(words(rays[field]), words(ref[field])), field
    for field in ("rx_o", "rx_d", "ry_o", "ry_d"):
        assert np.array_equal(words(aux[field]), words(ref_aux[field])), field
    # the auxiliary directions are not the ray's own (the offsets are not zero)
    assert not np.array_equal(aux["rx_d"], rays["d"]) and not np.array_equal(aux["ry_d"], rays["d"])
    # without aux_spp only the rays come back, the same ones
    assert np.array_equal(words(spt.perspective_rays(cam, W, H, off, first_sample=1)["d"]), words(rays["d"]))


def norm2_error(d):
    d = np.asarray(d, dtype=np.float64)
    return np.abs(np.sum(d * d, axis=-1) - 1.0).max()


def some_offsets(seed, count=2):
    return np.random.default_rng(seed).random((count, H, W, 2), dtype=np.float32)


def test_other_generators_return_unit_directions(scene):
    cam = scene.get_camera("main")
    off = some_offsets(1)
    ortho = spt.orthographic_rays(cam, W, H, off, view_height=3.0)
    pano = spt.panorama_rays((0.5, 1.0, -2.0), W, H, off)
    lens = spt.thin_lens_rays(cam, W, H, off, some_offsets(2), lens_radius=0.05, focus_distance=4.0)
    for rays in (ortho, pano, lens):
        assert rays.dtype == spt.PATH_RAY_DTYPE and rays.shape == (2, H, W)
        assert norm2_error(rays["d"]) <= 2.0 ** -23
        assert np.all(rays["t_min"] == f32(spt.CAMERA_T_MIN))
        assert np.array_equal(rays["stream_a"][1], np.arange(W * H, dtype=np.uint32).reshape(H, W))
        assert np.all(rays["stream_b"][1] == 1)


def test_orthographic_convention(scene):
    cam = scene.get_camera("main")
    centre = np.full((H, W, 2), 0.5, dtype=f32)
    rays = spt.orthographic_rays(cam, W, H, centre, view_height=2.0)[0]
    fwd, up, right, eye = (np.array(list(v), dtype=np.float64) for v in (cam.forward, cam.up, cam.right, cam.eye))
    assert np.allclose(rays["d"], fwd / np.linalg.norm(fwd), atol=1e-6)
    rel = rays["o"].astype(np.float64) - eye
    assert np.abs(rel @ fwd).max() < 1e-5                                   # origins lie in the plane through the eye
    assert np.allclose(rel[0, 0] @ up, (0.5 - 0.5 / H) * 2.0, atol=1e-5)    # row 0 on top
    assert np.allclose(rel[H - 1, 0] @ up, -(0.5 - 0.5 / H) * 2.0, atol=1e-5)
    assert np.allclose(rel[0, W - 1] @ right, (0.5 - 0.5 / W) * (W / H) * 2.0, atol=1e-5)   # x grows to the right


def test_panorama_poles_and_seam():
    zero = np.zeros((H, W, 2), dtype=f32)
    rays = spt.panorama_rays((1.0, 2.0, 3.0), W, H, zero)[0]
    assert np.all(rays["o"] == np.array([1.0, 2.0, 3.0], dtype=f32))
    d = rays["d"]
    assert np.allclose(d[0], [0.0, 1.0, 0.0], atol=1e-6)                    # row 0 starts at theta 0: +y for every column
    mid = d[H // 2]                                                          # theta = pi / 2: the horizon
    assert np.abs(mid[:, 1]).max() < 1e-6
    assert np.allclose(mid[0], [0.0, 0.0, -1.0], atol=1e-6)                 # phi 0 (the seam, left edge of column 0): -z
    assert np.allclose(mid[W // 2], [0.0, 0.0, 1.0], atol=1e-6)             # phi pi (the image centre): +z
    assert np.allclose(mid[W // 4], [-1.0, 0.0, 0.0], atol=1e-6)            # phi pi / 2: -x
    # the environment map's parametrisation gives the pixel back: theta = acos(d.y), phi = atan2(d.x, d.z) + pi
    theta = np.arccos(np.clip(d[..., 1].astype(np.float64), -1, 1))
    assert np.allclose(theta, (np.arange(H) / H * np.pi)[:, None], atol=1e-5)
    phi = np.arctan2(d[1:, :, 0].astype(np.float64), d[1:, :, 2].astype(np.float64)) + np.pi
    want = np.broadcast_to(np.arange(W) / W * 2 * np.pi, phi.shape)
    assert np.allclose(np.minimum(np.abs(phi - want), 2 * np.pi - np.abs(phi - want)), 0.0, atol=1e-4)
    last = spt.panorama_rays((0, 0, 0), W, H, np.full((H, W, 2), 0.999999, dtype=f32))[0]["d"][H - 1]
    assert np.allclose(last, [0.0, -1.0, 0.0], atol=1e-5)                   # the last row ends at theta pi: -y


def test_thin_lens_focus_and_pinhole_limit(scene):
    cam = scene.get_camera("main")
    off, uv = some_offsets(3, 1), some_offsets(4, 1)
    pin = spt.perspective_rays(cam, W, H, off)
    lens0 = spt.thin_lens_rays(cam, W, H, off, uv, lens_radius=0.0, focus_distance=5.0)
    assert np.allclose(lens0["d"], pin["d"], atol=1e-6) and np.allclose(lens0["o"], pin["o"], atol=1e-6)
    lens = spt.thin_lens_rays(cam, W, H, off, uv, lens_radius=0.1, focus_distance=5.0)
    fwd, eye = np.array(list(cam.forward), dtype=np.float64), np.array(list(cam.eye), dtype=np.float64)
    # both rays of a pixel pass through the same point of the plane of focus, 5 along forward from the eye
    def at_focus(r):
        o, d = r["o"].astype(np.float64), r["d"].astype(np.float64)
        t = (5.0 - (o - eye) @ fwd) / (d @ fwd)
        return o + d * t[..., None]
    assert np.allclose(at_focus(lens), at_focus(pin), atol=1e-4)
    rel = lens["o"].astype(np.float64) - eye
    assert np.abs(rel @ fwd).max() < 1e-6 and np.linalg.norm(rel, axis=-1).max() <= 0.1 + 1e-6

"""What spt_radiance must return for the rays of a camera plan, from the oracle's own functions.

Sample s of pixel (i, j) of a plan is a ray - oracle_camera_ray at the screen point of pt.rs:269-271, restated here in float32 numpy
from the pixel offsets the oracle's sampler gives (_wide_film_ref.offsets) - traced under the stream (pixel, s) of
oracle_rng_state.  Its colour is oracle_render_samples' value for that sample and pixel, so "the radiance of ray r under stream
(a, b)" has an exact expected value whenever r is some camera's ray.  Nothing here reads the package's ray generators.
"""
import ctypes as C

import numpy as np

import _util
import _wide_film_ref

f32 = np.float32


def screen_points(width, height, off):
    """x, y of pt.rs:269-271 for offsets (count, H, W, 2): f32 arrays (count, H, W), one rounded operation at a time."""
    off = np.asarray(off, dtype=f32)
    aspect = f32(width) / f32(height)
    width_inv, height_inv = f32(1) / f32(width), f32(1) / f32(height)
    i = np.arange(width).astype(f32)[None, None, :]
    rows = np.array([height - j - 1 for j in range(height)], dtype=f32)[None, :, None]
    x = ((i + off[..., 0]) * width_inv - f32(0.5)) * aspect
    y = (rows + off[..., 1]) * height_inv - f32(0.5)
    return x, y


def aux_offsets(width, height, spp):
    """aux_dx, aux_dy as plan_ctx computes them (pt.rs:253-254, 272-275)."""
    aspect = f32(width) / f32(height)
    width_inv, height_inv = f32(1) / f32(width), f32(1) / f32(height)
    spp_sqrt_inv = f32(1) / f32(np.sqrt(f32(spp)))
    return f32(f32(aspect * width_inv) * spp_sqrt_inv), f32(height_inv * spp_sqrt_inv)


def oracle_rays(cam, x, y):
    """oracle_camera_ray at every (x, y): origins and directions, shape x.shape + (3,)."""
    lib = _util.oracle_lib()
    o, d = np.zeros(x.shape + (3,), dtype=f32), np.zeros(x.shape + (3,), dtype=f32)
    bo, bd = (C.c_float * 3)(), (C.c_float * 3)()
    of, df = o.reshape(-1, 3), d.reshape(-1, 3)
    for k, (xv, yv) in enumerate(zip(x.reshape(-1), y.reshape(-1))):
        lib.oracle_camera_ray(C.byref(cam), float(xv), float(yv), bo, bd)
        of[k] = bo[:]
        df[k] = bd[:]
    return o, d


def plan_rays(spt, scene, renderer, width, height, first, count, camera=None, aux=False, t_min=None):
    """The rays of the plan's samples first .. first + count - 1 as (count, H, W) PATH_RAY_DTYPE records with streams (pixel,
    sample); aux: their auxiliary rays too, (rays, aux)."""
    cam = scene.get_camera(camera)
    off = _wide_film_ref.offsets(spt, renderer.seed, width, height, renderer.spp, renderer.sampler, first, count)
    x, y = screen_points(width, height, off)
    rays = np.zeros((count, height, width), dtype=spt.PATH_RAY_DTYPE)
    rays["o"], rays["d"] = oracle_rays(cam, x, y)
    rays["t_min"] = f32(spt.CAMERA_T_MIN if t_min is None else t_min)
    rays["stream_a"] = (np.arange(height, dtype=np.uint32)[:, None] * np.uint32(width) + np.arange(width, dtype=np.uint32)[None, :])[None]
    rays["stream_b"] = (np.uint32(first) + np.arange(count, dtype=np.uint32))[:, None, None]
    if not aux:
        return rays
    dx, dy = aux_offsets(width, height, renderer.spp)
    ax = np.zeros(rays.shape, dtype=spt.RAY_AUX_DTYPE)
    ax["rx_o"], ax["rx_d"] = oracle_rays(cam, x + dx, y)
    ax["ry_o"], ax["ry_d"] = oracle_rays(cam, x, y + dy)
    return rays, ax


def expected(scene, renderer, width, height, first, count, camera=None):
    """(count, H, W, 3) f32: the oracle's colour of every one of those samples, under the configuration the device is held to."""
    return _util.oracle_render_samples(scene, renderer, width, height, first, count, camera=camera, flags=_util.device_oracle_flags())


def rng_skip(spt, renderer):
    """Draws a camera sample's stream has made before trace_ray starts: the two pixel offsets of the random sampler."""
    return 0 if renderer.sampler == spt.SAMPLER_RECURRENCE else 2

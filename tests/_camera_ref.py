"""The camera models of spt_render_camera / spt_film_create_camera, restated in float32 numpy from their specification.

All arithmetic is IEEE f32, one rounded operation at a time, in the written order (numpy does not contract).  x, y are the screen
point of pt.rs:269-271 (_radiance_ref.screen_points), hc = base.half_cot_half_fov, t_min = 0.0001f for every model.

  PERSPECTIVE   o = eye, d = normalize((forward*hc + right*x) + up*y)
  THIN_LENS     u1, u2: the first two draws of the stream (seed ^ SALT, pixel, plan index), made whatever the radius
                a = 2*u1 - 1, b = 2*u2 - 1; a == 0 && b == 0: lx = ly = 0; |a| > |b|: r = a, phi = (PI/4) * (b/a);
                otherwise r = b, phi = PI/2 - (PI/4) * (a/b); lx = r*cos(phi), ly = r*sin(phi)
                ft = focus_distance / hc; du = (forward*hc + right*x) + up*y
                lo_k = (right_k*lx + up_k*ly) * lens_radius; o = eye + lo; d = normalize(du*ft - lo)
  ORTHOGRAPHIC  sx = x*view_height, sy = y*view_height; o_k = eye_k + (right_k*sx + up_k*sy); d = forward
  PANORAMA      ph = (x * aspect_inv) * (2*PI), aspect_inv = 1/aspect; th = (0.5 - y) * PI; st = sin(th)
                o = eye; d = normalize((st*sin(ph), cos(th), st*cos(ph)))
  Auxiliary rays: the same model at (x + aux_dx, y) and (x, y + aux_dy) with the same lens point.

sin / cos are the oracle's deterministic ones (oracle_detmath), the lens draws come from oracle_rng_stream, the pixel offsets from
_wide_film_ref.offsets.  Nothing here includes the library's header or calls the package's generators.
"""
import numpy as np

import _radiance_ref
import _util
import _wide_film_ref

f32 = np.float32
PI = f32(3.14159265358979323846)
SALT = 0x4C454E5343414D31
T_MIN = f32(0.0001)
PERSPECTIVE, THIN_LENS, ORTHOGRAPHIC, PANORAMA = 0, 1, 2, 3


def _det(fn, a):
    a = np.ascontiguousarray(a, dtype=f32)
    out = np.zeros(a.shape, dtype=f32)
    _util.oracle_lib().oracle_detmath(fn, a.size, a.ctypes.data, a.ctypes.data, out.ctypes.data)
    return out


def det_sin(a):
    return _det(0, a)


def det_cos(a):
    return _det(1, a)


def normalize(v):
    v = np.asarray(v, dtype=f32)
    n = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    return v / n[..., None]


def lens_points(seed, width, height, first, count):
    """(count, H, W) f32 lx, ly: the disk map of the first two draws of stream (seed ^ SALT, pixel, plan index)."""
    lib = _util.oracle_lib()
    u = np.zeros((count, height, width, 2), dtype=f32)
    buf = np.zeros(2, dtype=f32)
    for s in range(count):
        for j in range(height):
            for i in range(width):
                lib.oracle_rng_stream((seed ^ SALT) & 0xFFFFFFFFFFFFFFFF, j * width + i, first + s, 2, buf.ctypes.data)
                u[s, j, i] = buf
    a = f32(2) * u[..., 0] - f32(1)
    b = f32(2) * u[..., 1] - f32(1)
    zero = (a == 0) & (b == 0)
    wide = np.abs(a) > np.abs(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(wide, a, b)
        phi = np.where(wide, (PI / f32(4)) * (b / a), PI / f32(2) - (PI / f32(4)) * (a / b)).astype(f32)
    phi = np.where(zero, f32(0), phi).astype(f32)
    lx = np.where(zero, f32(0), r * det_cos(phi)).astype(f32)
    ly = np.where(zero, f32(0), r * det_sin(phi)).astype(f32)
    return lx, ly


def _cam_vectors(cam):
    return (np.array(cam.eye[:], dtype=f32), np.array(cam.forward[:], dtype=f32), np.array(cam.up[:], dtype=f32),
            np.array(cam.right[:], dtype=f32), f32(cam.half_cot_half_fov))


def model_rays(model, width, height, x, y, lx, ly):
    """o, d (x.shape + (3,)) of the model at screen points x, y with lens points lx, ly."""
    eye, fwd, up, right, hc = _cam_vectors(model.base)
    x = np.asarray(x, dtype=f32)[..., None]
    y = np.asarray(y, dtype=f32)[..., None]
    kind = int(model.type)
    if kind == ORTHOGRAPHIC:
        vh = f32(model.view_height)
        sx, sy = x * vh, y * vh
        o = eye + (right * sx + up * sy)
        d = np.broadcast_to(fwd, o.shape).astype(f32)
        return o.astype(f32), d
    if kind == PANORAMA:
        aspect_inv = f32(1) / (f32(width) / f32(height))
        ph = ((x[..., 0] * aspect_inv) * (f32(2) * PI)).astype(f32)
        th = ((f32(0.5) - y[..., 0]) * PI).astype(f32)
        st = det_sin(th)
        v = np.stack([st * det_sin(ph), det_cos(th), st * det_cos(ph)], axis=-1).astype(f32)
        return np.broadcast_to(eye, v.shape).astype(f32), normalize(v)
    du = (fwd * hc + right * x) + up * y
    if kind == THIN_LENS:
        ft = f32(model.focus_distance) / hc
        lo = (right * np.asarray(lx, dtype=f32)[..., None] + up * np.asarray(ly, dtype=f32)[..., None]) * f32(model.lens_radius)
        return (eye + lo).astype(f32), normalize(du * ft - lo)
    assert kind == PERSPECTIVE
    return np.broadcast_to(eye, du.shape).astype(f32), normalize(du)


def plan_rays(spt, model, renderer, width, height, first, count, aux=False):
    """The model's rays of the plan's samples first .. first + count - 1: (count, H, W) PATH_RAY_DTYPE records with streams (pixel,
    plan index); aux: their auxiliary rays too, (rays, aux)."""
    off = _wide_film_ref.offsets(spt, renderer.seed, width, height, renderer.spp, renderer.sampler, first, count)
    x, y = _radiance_ref.screen_points(width, height, off)
    if int(model.type) == THIN_LENS:
        lx, ly = lens_points(renderer.seed, width, height, first, count)
    else:
        lx = ly = np.zeros(x.shape, dtype=f32)
    rays = np.zeros((count, height, width), dtype=spt.PATH_RAY_DTYPE)
    rays["o"], rays["d"] = model_rays(model, width, height, x, y, lx, ly)
    rays["t_min"] = T_MIN
    rays["stream_a"] = (np.arange(height, dtype=np.uint32)[:, None] * np.uint32(width) + np.arange(width, dtype=np.uint32)[None, :])[None]
    rays["stream_b"] = (np.uint32(first) + np.arange(count, dtype=np.uint32))[:, None, None]
    if not aux:
        return rays
    dx, dy = _radiance_ref.aux_offsets(width, height, renderer.spp)
    ax = np.zeros(rays.shape, dtype=spt.RAY_AUX_DTYPE)
    ax["rx_o"], ax["rx_d"] = model_rays(model, width, height, x + dx, y, lx, ly)
    ax["ry_o"], ax["ry_d"] = model_rays(model, width, height, x, y + dy, lx, ly)
    return rays, ax

"""spt_bake's specification (include/spt_abi.h, "irradiance at surface points") restated in float32 numpy from descriptor arrays.

All arithmetic is IEEE f32, one rounded operation at a time, in the written order (numpy does not contract).

  SURFACE  u = (1 - v) - w; object position (p0*u + p1*v) + p2*w, to the world ((c0*x + c1*y) + c2*z) + t with fwd's columns
           normal: n = normalize((n0*u + n1*v) + n2*w), world normalize((nrm0*n.x + nrm1*n.y) + nrm2*n.z)
  WORLD    p, n as given;  FLIP: n = -n after it is resolved
  frame    s = sqrt(1 - n.y*n.y); s != 0: bitangent = n * (-n.y / s) with y := s, tangent = cross(bitangent, n);
           else n.y > 0: bitangent (1,0,0), tangent (0,0,1); else bitangent (-1,0,0), tangent (0,0,-1)
  sample   rx, ry: the first two draws of stream (seed ^ SALT, a = first_point + i, b = first_sample + k)
           phi = rx * 2 * PI; st = sqrt(ry), ct = sqrt(1 - ry); local (st*cos, st*sin, ct)
           d = normalize((tangent*lx + bitangent*ly) + n*lz); t_min = 0.0001 / max(ct, 0.00001); o = p; path stream (a, b)
  delta    directional: dir = -dir_l, strength, dist = f32::MAX;  point: sv = pos - p, dist = sqrt(dot(sv, sv)), dir = sv / dist,
           strength * (1 / dot(sv, sv));  spot: the same with strength * atten first,
           atten = clamp((dot(dir_l, -dir) - cos_outer) / max(cos_inner - cos_outer, 0.0001), 0, 1)
           c = dot(n, dir) > 0; li = (strength * FRAC_1_PI) * c, not all zero; shadow ray (p, dir, 0.0001 / max(c, 0.00001), dist - 0.001)
  result   D + (((0 + x0) + x1) + ...) * (1 / S), D the in-order sum of the unoccluded li

sin / cos are the oracle's deterministic ones (oracle_detmath), the draws come from oracle_rng_stream.  Nothing here includes the
library's header or calls the package's generators.
"""
import numpy as np

import _util

f32 = np.float32
PI = f32(3.14159265358979323846)
FRAC_1_PI = f32(0.318309886183790671538)
F32_MAX = f32(3.40282346638528859812e+38)
SALT = 0x42414B45504F4E54
EPS = f32(0.0001)
DIRECTIONAL, POINT, SPOT = 0, 1, 2


def _det(fn, a):
    a = np.ascontiguousarray(a, dtype=f32)
    out = np.zeros(a.shape, dtype=f32)
    _util.oracle_lib().oracle_detmath(fn, a.size, a.ctypes.data, a.ctypes.data, out.ctypes.data)
    return out


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(v):
    v = np.asarray(v, dtype=f32)
    return v / np.sqrt(dot(v, v))[..., None]


def tables(scene):
    """The arrays the reference reads, from a Scene's descriptor."""
    return {k: scene.array(k) for k in ("instances", "meshes", "tri_pos", "tri_attr", "lights")}


def resolve(tab, points, world=False, flip=False):
    """World position and normal, (n, 3) f32 each."""
    if world:
        p, n = np.array(points["p"], dtype=f32), np.array(points["n"], dtype=f32)
    else:
        inst = tab["instances"][points["instance"]]
        tp, ta = tab["tri_pos"][points["prim"]], tab["tri_attr"][points["prim"]]
        v, w = points["v"].astype(f32)[:, None], points["w"].astype(f32)[:, None]
        u = (f32(1) - v) - w
        op = (tp["p0"] * u + tp["p1"] * v) + tp["p2"] * w
        fwd, nrm = inst["fwd"], inst["nrm"]
        p = ((fwd[:, 0:3] * op[:, 0:1] + fwd[:, 3:6] * op[:, 1:2]) + fwd[:, 6:9] * op[:, 2:3]) + fwd[:, 9:12]
        nn = ta["n"]
        on = normalize((nn[:, 0] * u + nn[:, 1] * v) + nn[:, 2] * w)
        n = normalize((nrm[:, 0:3] * on[:, 0:1] + nrm[:, 3:6] * on[:, 1:2]) + nrm[:, 6:9] * on[:, 2:3])
    if flip:
        n = -n
    assert p.dtype == f32 and n.dtype == f32
    return p, n


def frame(n):
    """sphere_frame: tangent, bitangent."""
    ny = n[:, 1]
    s = np.sqrt(f32(1) - ny * ny)
    with np.errstate(divide="ignore", invalid="ignore"):
        bt = n * (-ny / s)[:, None]
        bt[:, 1] = s
        tg = np.stack([bt[:, 1] * n[:, 2] - bt[:, 2] * n[:, 1], bt[:, 2] * n[:, 0] - bt[:, 0] * n[:, 2], bt[:, 0] * n[:, 1] - bt[:, 1] * n[:, 0]], axis=-1)
    pole, up = s == 0, (ny > 0)[:, None]
    bt = np.where(pole[:, None], np.where(up, np.array([1, 0, 0], dtype=f32), np.array([-1, 0, 0], dtype=f32)), bt).astype(f32)
    tg = np.where(pole[:, None], np.where(up, np.array([0, 0, 1], dtype=f32), np.array([0, 0, -1], dtype=f32)), tg).astype(f32)
    return tg, bt


def gather_rays(spt, p, n, samples, seed, first_point=0, first_sample=0):
    """(n, samples) PATH_RAY_DTYPE."""
    lib = _util.oracle_lib()
    count = p.shape[0]
    u = np.zeros((count, samples, 2), dtype=f32)
    buf = np.zeros(2, dtype=f32)
    for i in range(count):
        for k in range(samples):
            lib.oracle_rng_stream((seed ^ SALT) & 0xFFFFFFFFFFFFFFFF, (first_point + i) & 0xFFFFFFFF, first_sample + k, 2, buf.ctypes.data)
            u[i, k] = buf
    rx, ry = u[..., 0], u[..., 1]
    phi = rx * f32(2) * PI
    sp, cp = _det(0, phi), _det(1, phi)
    st, ct = np.sqrt(ry), np.sqrt(f32(1) - ry)
    lx, ly, lz = (st * cp)[..., None], (st * sp)[..., None], ct[..., None]
    tg, bt = frame(n)
    d = normalize((tg[:, None, :] * lx + bt[:, None, :] * ly) + n[:, None, :] * lz)
    rays = np.zeros((count, samples), dtype=spt.PATH_RAY_DTYPE)
    rays["o"] = p[:, None, :]
    rays["d"] = d
    rays["t_min"] = EPS / np.maximum(ct, f32(0.00001))
    rays["stream_a"] = ((first_point + np.arange(count, dtype=np.uint64)) & 0xFFFFFFFF).astype(np.uint32)[:, None]
    rays["stream_b"] = (np.uint32(first_sample) + np.arange(samples, dtype=np.uint32))[None, :]
    assert d.dtype == f32
    return rays


def delta_lights(spt, tab, p, n):
    """(n, n_lights) RAY_DTYPE shadow rays and (n, n_lights, 3) li; zeros where a light is skipped."""
    lights = tab["lights"]
    count = p.shape[0]
    rays = np.zeros((count, len(lights)), dtype=spt.RAY_DTYPE)
    li_out = np.zeros((count, len(lights), 3), dtype=f32)
    for l, lt in enumerate(lights):
        kind = int(lt["type"])
        strength = np.broadcast_to(np.array(lt["strength"], dtype=f32), (count, 3)).astype(f32)
        if kind == DIRECTIONAL:
            dr = np.broadcast_to(-np.array(lt["dir"], dtype=f32), (count, 3)).astype(f32)
            dist = np.full(count, F32_MAX, dtype=f32)
        elif kind in (POINT, SPOT):
            sv = np.array(lt["pos"], dtype=f32) - p
            dist_sqr = dot(sv, sv)
            dist = np.sqrt(dist_sqr)
            dr = sv / dist[:, None]
            if kind == SPOT:
                ld = np.array(lt["dir"], dtype=f32)
                cs = dot(np.broadcast_to(ld, (count, 3)), -dr)
                x = (cs - f32(lt["cos_outer"])) / np.maximum(f32(lt["cos_inner"]) - f32(lt["cos_outer"]), f32(0.0001))
                atten = np.where(x < 0, f32(0), np.where(x > 1, f32(1), x)).astype(f32)
                strength = strength * atten[:, None]
            strength = strength * (f32(1) / dist_sqr)[:, None]
        else:
            continue
        c = dot(n, dr)
        li = (strength * FRAC_1_PI) * c[:, None]
        want = (c > 0) & ~np.all(li == 0, axis=-1)
        assert li.dtype == f32 and dr.dtype == f32
        rays["o"][:, l] = np.where(want[:, None], p, f32(0))
        rays["d"][:, l] = np.where(want[:, None], dr, f32(0))
        with np.errstate(divide="ignore", invalid="ignore"):
            rays["t_min"][:, l] = np.where(want, EPS / np.maximum(c, f32(0.00001)), f32(0))
        rays["t_max"][:, l] = np.where(want, dist - f32(0.001), f32(0))
        li_out[:, l] = np.where(want[:, None], li, f32(0))
    return rays, li_out


def bake_inputs(spt, tab, points, samples, seed, first_point=0, first_sample=0, world=False, flip=False):
    """What bake_rays returns, from the specification."""
    p, n = resolve(tab, points, world, flip)
    delta_rays, delta_li = delta_lights(spt, tab, p, n)
    return {"rays": gather_rays(spt, p, n, samples, seed, first_point, first_sample), "pos": p, "nrm": n, "delta_rays": delta_rays, "delta_li": delta_li}


def delta_sum(ds, ref):
    """D: the in-order sum of li over the lights whose shadow ray DeviceScene.trace_any finds unoccluded."""
    li, rays = ref["delta_li"], ref["delta_rays"]
    D = np.zeros((li.shape[0], 3), dtype=f32)
    for l in range(li.shape[1]):
        want = np.any(li[:, l] != 0, axis=-1)
        if not want.any():
            continue
        occ = np.ones(li.shape[0], dtype=bool)
        occ[want] = ds.trace_any(np.ascontiguousarray(rays[want, l])) != 0
        D = np.where((want & ~occ)[:, None], D + li[:, l], D).astype(f32)
    return D


def bake_from_existing_calls(ds, ref, max_depth, seed):
    """want_i = D_ref + in-order mean over k of ds.radiance(rays_ref[i, k], repeats=1, rng_skip=0); also returns D and the gather sum."""
    D = delta_sum(ds, ref)
    rays = ref["rays"]
    S = rays.shape[1]
    acc = np.zeros((rays.shape[0], 3), dtype=f32)
    if max_depth > 0:
        for k in range(S):
            acc = acc + ds.radiance(np.ascontiguousarray(rays[:, k]), repeats=1, max_depth=max_depth, seed=seed, rng_skip=0)
    out = D + acc * (f32(1) / f32(S))
    assert out.dtype == f32
    return out, D, acc

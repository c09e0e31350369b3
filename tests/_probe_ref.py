"""spt_probe's specification (include/spt_abi.h, "spherical-harmonic light probes") restated in float32 numpy.

All arithmetic is IEEE f32, one rounded operation at a time, in the written order (numpy does not contract).

  probe    valid iff p is finite
  sample   rx, ry: the first two draws of stream (seed ^ SALT, a = first_point + i, b = first_sample + k)
           z = 1 - 2*rx; r = sqrt(max(0, 1 - z*z)); phi = ry * 2 * PI; d = normalize(r*cos, r*sin, z); o = p; t_min = 0.0001;
           path stream (a, b)
  basis    Y0 = 0.282094792; Y1 = 0.488602512*y; Y2 = 0.488602512*z; Y3 = 0.488602512*x; Y4 = 1.092548431*(x*y);
           Y5 = 1.092548431*(y*z); Y6 = 0.315391565*(3*(z*z) - 1); Y7 = 1.092548431*(x*z); Y8 = 0.546274215*(x*x - y*y)
  delta    directional: dir = -dir_l, strength, dist = f32::MAX;  point: sv = pos - p, dist = sqrt(dot(sv, sv)), dir = sv / dist,
           strength * (1 / dot(sv, sv));  spot: the same with strength * atten first,
           atten = clamp((dot(dir_l, -dir) - cos_outer) / max(cos_inner - cos_outer, 0.0001), 0, 1)
           li = strength, not all zero; shadow ray (p, dir, 0.0001, dist - 0.001); D[j][c] += li[c] * Y_j(dir) where unoccluded
  result   sh[j][c] = D[j][c] + (((0 + x_c(0)*Y_j(d_0)) + x_c(1)*Y_j(d_1)) + ...) * w, w = (4*PI) * (1 / S)
  aux      hits / S, backfacing / S (mesh hits with dot(n, d) > 0, n as a bake point's normal), sum of t in k order / hits or 0,
           smallest t or f32::MAX

sin / cos are the oracle's deterministic ones (oracle_detmath), the draws come from oracle_rng_stream.  Nothing here includes the
library's headers or calls the package's generators.
"""
import numpy as np

import _bake_ref
import _util

f32 = np.float32
PI = f32(3.14159265358979323846)
F32_MAX = f32(3.40282346638528859812e+38)
SALT = 0x50524F4245534831
EPS = f32(0.0001)
DIRECTIONAL, POINT, SPOT = 0, 1, 2
K0, K1, K2, K3, K4 = f32(0.282094792), f32(0.488602512), f32(1.092548431), f32(0.315391565), f32(0.546274215)

dot = _bake_ref.dot
normalize = _bake_ref.normalize


def weight(samples):
    return (f32(4) * PI) * (f32(1) / f32(samples))


def sphere_map(rx, ry):
    """The uniform sphere map of draws, (..., 3) f32."""
    rx, ry = np.asarray(rx, dtype=f32), np.asarray(ry, dtype=f32)
    z = f32(1) - f32(2) * rx
    r = np.sqrt(np.maximum(f32(0), f32(1) - z * z))
    phi = ry * f32(2) * PI
    sp, cp = _bake_ref._det(0, phi), _bake_ref._det(1, phi)
    d = normalize(np.stack([r * cp, r * sp, z], axis=-1))
    assert d.dtype == f32
    return d


def draws(count, samples, seed, first_point=0, first_sample=0):
    """(count, samples, 2) f32: rx, ry of every (probe, sample)."""
    lib = _util.oracle_lib()
    u = np.zeros((count, samples, 2), dtype=f32)
    buf = np.zeros(2, dtype=f32)
    for i in range(count):
        for k in range(samples):
            lib.oracle_rng_stream((seed ^ SALT) & 0xFFFFFFFFFFFFFFFF, (first_point + i) & 0xFFFFFFFF, first_sample + k, 2, buf.ctypes.data)
            u[i, k] = buf
    return u


def basis(d):
    """(..., 9) f32."""
    d = np.asarray(d, dtype=f32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    Y = np.stack([np.full(x.shape, K0, dtype=f32), K1 * y, K1 * z, K1 * x, K2 * (x * y), K2 * (y * z), K3 * (f32(3) * (z * z) - f32(1)), K2 * (x * z),
                  K4 * (x * x - y * y)], axis=-1)
    assert Y.dtype == f32
    return Y


def gather_rays(spt, p, samples, seed, first_point=0, first_sample=0):
    """(n, samples) PATH_RAY_DTYPE and the (n, samples, 9) weights."""
    count = p.shape[0]
    u = draws(count, samples, seed, first_point, first_sample)
    d = sphere_map(u[..., 0], u[..., 1])
    rays = np.zeros((count, samples), dtype=spt.PATH_RAY_DTYPE)
    rays["o"] = p[:, None, :]
    rays["d"] = d
    rays["t_min"] = EPS
    rays["stream_a"] = ((first_point + np.arange(count, dtype=np.uint64)) & 0xFFFFFFFF).astype(np.uint32)[:, None]
    rays["stream_b"] = (np.uint32(first_sample) + np.arange(samples, dtype=np.uint32))[None, :]
    return rays, basis(d)


def delta_lights(spt, lights, p):
    """(n, n_lights) RAY_DTYPE shadow rays, (n, n_lights, 3) li and (n, n_lights, 9) basis; zeros where a light is skipped."""
    count = p.shape[0]
    rays = np.zeros((count, len(lights)), dtype=spt.RAY_DTYPE)
    li_out = np.zeros((count, len(lights), 3), dtype=f32)
    y_out = np.zeros((count, len(lights), 9), dtype=f32)
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
            with np.errstate(divide="ignore", invalid="ignore"):
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
        li = strength
        want = ~np.all(li == 0, axis=-1)
        assert li.dtype == f32 and dr.dtype == f32
        rays["o"][:, l] = np.where(want[:, None], p, f32(0))
        rays["d"][:, l] = np.where(want[:, None], dr, f32(0))
        rays["t_min"][:, l] = np.where(want, EPS, f32(0))
        rays["t_max"][:, l] = np.where(want, dist - f32(0.001), f32(0))
        li_out[:, l] = np.where(want[:, None], li, f32(0))
        y_out[:, l] = np.where(want[:, None], basis(dr), f32(0))
    return rays, li_out, y_out


def probe_inputs(spt, lights, p, samples, seed, first_point=0, first_sample=0):
    """What probe_rays returns, from the specification.  p: (n, 3) f32."""
    p = np.ascontiguousarray(p, dtype=f32)
    assert np.isfinite(p).all()
    rays, weights = gather_rays(spt, p, samples, seed, first_point, first_sample)
    delta_rays, delta_li, delta_basis = delta_lights(spt, lights, p)
    return {"rays": rays, "weights": weights, "delta_rays": delta_rays, "delta_li": delta_li, "delta_basis": delta_basis}


def delta_sum(ds, ref):
    """D (n, 9, 3): the in-order sum of li * Y(dir) over the lights whose shadow ray DeviceScene.trace_any finds unoccluded."""
    li, rays, Y = ref["delta_li"], ref["delta_rays"], ref["delta_basis"]
    D = np.zeros((li.shape[0], 9, 3), dtype=f32)
    for l in range(li.shape[1]):
        want = np.any(li[:, l] != 0, axis=-1)
        if not want.any():
            continue
        occ = np.ones(li.shape[0], dtype=bool)
        occ[want] = ds.trace_any(np.ascontiguousarray(rays[want, l])) != 0
        term = li[:, l][:, None, :] * Y[:, l][:, :, None]
        D = np.where((want & ~occ)[:, None, None], D + term, D).astype(f32)
    return D


def visibility(tab, rays, hits):
    """aux (n, 4) from the first-segment hits (n, S) HIT_DTYPE of the gather rays (n, S)."""
    S = rays.shape[1]
    inv = f32(1) / f32(S)
    hit = hits["instance"] >= 0
    inst = tab["instances"]
    mesh = hit & (inst["prim_type"][np.maximum(hits["instance"], 0)] == 1)
    back = np.zeros(hit.shape, dtype=bool)
    if mesh.any():
        pts = np.zeros(int(mesh.sum()), dtype=_bake_ref_point_dtype())
        for f in ("instance", "prim", "v", "w"):
            pts[f] = hits[f][mesh]
        _, n = _bake_ref.resolve(tab, pts)
        back[mesh] = dot(n, rays["d"][mesh]) > 0
    n_hit = hit.sum(axis=1)
    aux = np.zeros((rays.shape[0], 4), dtype=f32)
    aux[:, 0] = n_hit.astype(f32) * inv
    aux[:, 1] = back.sum(axis=1).astype(f32) * inv
    t_sum = np.zeros(rays.shape[0], dtype=f32)
    t_min = np.full(rays.shape[0], F32_MAX, dtype=f32)
    for k in range(S):
        t_sum = np.where(hit[:, k], t_sum + hits["t"][:, k], t_sum).astype(f32)
        t_min = np.where(hit[:, k] & (hits["t"][:, k] < t_min), hits["t"][:, k], t_min).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        aux[:, 2] = np.where(n_hit > 0, t_sum / n_hit.astype(f32), f32(0))
    aux[:, 3] = t_min
    return aux


def _bake_ref_point_dtype():
    return np.dtype([("instance", "<u4"), ("prim", "<u4"), ("v", "<f4"), ("w", "<f4")])


def probes_from_existing_calls(ds, ref, max_depth, seed, tab=None, total=None):
    """want (n, 9, 3) = D_ref + (in-order sum over k of ds.radiance(rays_ref[:, k]) * Y_ref[:, k]) * w; also D, the sum, and aux
    (n, 4) when `tab` (the scene's tables) is given.  `total`: the S of w when the rays are a slice of a longer run."""
    D = delta_sum(ds, ref)
    rays, Y = ref["rays"], ref["weights"]
    S = rays.shape[1]
    acc = np.zeros((rays.shape[0], 9, 3), dtype=f32)
    hits = np.zeros(rays.shape, dtype=[("t", "<f4"), ("instance", "<i4"), ("prim", "<i4"), ("v", "<f4"), ("w", "<f4")])
    for k in range(S):
        if max_depth > 0 or tab is not None:
            x, h = ds.radiance(np.ascontiguousarray(rays[:, k]), repeats=1, max_depth=max_depth, seed=seed, rng_skip=0, hits=True)
            hits[:, k] = h
            acc = acc + x[:, None, :] * Y[:, k][:, :, None]
    out = D + acc * weight(total if total is not None else S)
    assert out.dtype == f32 and acc.dtype == f32
    aux = visibility(tab, rays, hits) if tab is not None else None
    return out, D, acc, aux

"""What spt_gbuffer (include/spt_abi.h, "first-hit surface records") must return, from sources that are not the code under test.

  hits      _util.oracle_trace_closest over _util.first_segments(rays) under _util.device_oracle_flags(): t, instance, prim, v, w
  p         o + d * t per component, float32 numpy (one rounded operation at a time; numpy does not contract)
  albedo    _util.oracle_radiance over the emissive stand-in of tests/_albedo_ref.py (every surface emits its albedo, nothing else
            adds light, max_depth 1) with the rays' aux records: le for a hit, +0 for a miss.  Nothing in it is random.
  n         mesh hits: _bake_ref.resolve(tables, hits), the normal spt_bake_resolve gives;
            sphere hits: the reconstruction restated here in float32 numpy from the instance and sphere records - object ray
            ((c0*o.x + c1*o.y) + c2*o.z) + t and (c0*d.x + c1*d.y) + c2*d.z of `inv`, n = (o' + d'*t - centre) / radius, world
            normalize((nrm0*n.x + nrm1*n.y) + nrm2*n.z) - which tests/test_gbuffer_abi.py holds to the oracle's debug-normal film;
            patch hits have no such source for rays of any origin: `n_known` is False there, the record's n is left +0 and its
            BACKFACING bit clear, and `same_records` leaves those words of those rays out (their normals are compared on pinhole
            rays, where the oracle's debug-normal film answers for every primitive kind: `debug_normal_words`)
  surface   the instance's `surface`
  flags     BACKFACING iff (n0*d0 + n1*d1) + n2*d2 > 0 with the n above, LIGHT iff the instance's light >= 0, prim_type << 8
  miss      t = f32::MAX, instance = prim = -1, every other word +0
"""
import numpy as np

import _albedo_ref
import _bake_ref
import _util

spt = _util.load_pkg()
f32 = np.float32
F32_MAX = np.finfo(f32).max
PRIM_SPHERE, PRIM_MESH, PRIM_BEZIER = 0, 1, 2


def sphere_normals(scene, rays, hits, inst):
    """World normals of sphere hits (every row is taken to be one), (n, 3) f32."""
    sph = scene.array("spheres")[inst["prim_id"]]
    inv, nrm = inst["inv"], inst["nrm"]
    o, d, t = rays["o"], rays["d"], hits["t"][:, None]
    oo = ((inv[:, 0:3] * o[:, 0:1] + inv[:, 3:6] * o[:, 1:2]) + inv[:, 6:9] * o[:, 2:3]) + inv[:, 9:12]
    od = (inv[:, 0:3] * d[:, 0:1] + inv[:, 3:6] * d[:, 1:2]) + inv[:, 6:9] * d[:, 2:3]
    on = ((oo + od * t) - sph["center"]) / sph["radius"][:, None]
    n = _bake_ref.normalize((nrm[:, 0:3] * on[:, 0:1] + nrm[:, 3:6] * on[:, 1:2]) + nrm[:, 6:9] * on[:, 2:3])
    assert n.dtype == f32
    return n


def normals(scene, rays, hits):
    """(n (count, 3) f32, known (count,) bool): the reference normal of every hit that has one (module docstring); +0 elsewhere."""
    rays = np.asarray(rays).reshape(-1)
    hit = hits["instance"] >= 0
    instances = scene.array("instances")
    inst = instances[np.maximum(hits["instance"], 0)]
    n = np.zeros((rays.shape[0], 3), dtype=f32)
    mesh = hit & (inst["prim_type"] == PRIM_MESH)
    if mesh.any():
        pts = np.zeros(int(mesh.sum()), dtype=spt.BAKE_POINT_DTYPE)
        for f in ("instance", "prim", "v", "w"):
            pts[f] = hits[f][mesh]
        n[mesh] = _bake_ref.resolve(_bake_ref.tables(scene), pts)[1]
    sphere = hit & (inst["prim_type"] == PRIM_SPHERE)
    if sphere.any():
        n[sphere] = sphere_normals(scene, rays[sphere], hits[sphere], inst[sphere])
    return n, mesh | sphere


def expected(scene, rays, aux=None):
    """(records GBUFFER_DTYPE, n_known bool) for flat PATH_RAY_DTYPE rays and their RAY_AUX_DTYPE records or None."""
    rays = np.ascontiguousarray(rays, dtype=spt.PATH_RAY_DTYPE).reshape(-1)
    flags = _util.device_oracle_flags()
    hits = _util.oracle_trace_closest(scene, _util.first_segments(rays), flags)
    hit = hits["instance"] >= 0
    albedo = _util.oracle_radiance(_albedo_ref.StandIn(scene), rays, aux, repeats=1, max_depth=1, seed=1, rng_skip=0, flags=flags)
    assert (albedo[~hit].view(np.uint32) == 0).all() and np.isfinite(albedo).all(), "the stand-in must give +0 on a miss and finite colours"
    assert (albedo[hit] != 0).any(axis=-1).all(), "the stand-in must give a colour on every hit"
    inst = scene.array("instances")[np.maximum(hits["instance"], 0)]
    n, n_known = normals(scene, rays, hits)
    rec = np.zeros(rays.shape[0], dtype=spt.GBUFFER_DTYPE)
    rec["t"], rec["instance"], rec["prim"] = np.where(hit, hits["t"], F32_MAX), np.where(hit, hits["instance"], -1), np.where(hit, hits["prim"], -1)
    rec["v"], rec["w"] = np.where(hit, hits["v"], f32(0)), np.where(hit, hits["w"], f32(0))
    with np.errstate(over="ignore", invalid="ignore"):
        p = rays["o"] + rays["d"] * hits["t"][:, None]
    assert p.dtype == f32
    rec["p"] = np.where(hit[:, None], p, f32(0))
    rec["n"] = n
    rec["albedo"] = albedo
    rec["surface"] = np.where(hit, inst["surface"], 0)
    back = n_known & (_bake_ref.dot(n, rays["d"]) > 0)
    word = (inst["prim_type"].astype(np.uint32) << np.uint32(8)) | np.where(inst["light"] >= 0, np.uint32(spt.GBUF_LIGHT), np.uint32(0)) \
        | np.where(back, np.uint32(spt.GBUF_BACKFACING), np.uint32(0))
    rec["flags"] = np.where(hit, word, 0)
    return rec, n_known | ~hit


def words(rec):
    """(n, 16) uint32 view of GBUFFER_DTYPE records (or of an (n, 16) float32 array)."""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 16)


def compared_words(n_known):
    """(n, 16) bool: the words `same_records` compares - all of them, but n and the BACKFACING bit where no source gives n."""
    keep = np.ones((n_known.shape[0], 16), dtype=bool)
    keep[~n_known, 4:7] = False
    return keep


def difference(got, want, n_known):
    """None, or a message naming the first ray whose record differs from the expected one in a compared word."""
    g, w = words(got).copy(), words(want).copy()
    assert g.shape == w.shape, (g.shape, w.shape)
    g[~n_known, 15] &= ~np.uint32(spt.GBUF_BACKFACING)
    bad = (g != w) & compared_words(n_known)
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad.any(axis=1))[0])
    names = ["p0", "p1", "p2", "t", "n0", "n1", "n2", "instance", "albedo0", "albedo1", "albedo2", "prim", "v", "w", "surface", "flags"]
    return "%d of %d records differ; the first is ray %d in %s: got %r, expected %r" % (
        int(bad.any(axis=1).sum()), g.shape[0], i, [names[k] for k in np.flatnonzero(bad[i])], g[i].view(spt.GBUFFER_DTYPE)[0], w[i].view(spt.GBUFFER_DTYPE)[0])


def census(rec):
    """(hit share, distinct albedos among the hits)."""
    hit = rec["instance"] >= 0
    return float(hit.mean()), len(np.unique(np.ascontiguousarray(rec["albedo"][hit]).view(np.uint32), axis=0))


def debug_normal_words(scene, width, height, camera=None, seed=11):
    """(rays (H*W,) of a one-sample recurrence plan, film (H*W, 3) f32): the pinhole rays of tests/_radiance_ref.plan_rays and the
    oracle's SPT_RENDER_DEBUG_NORMAL film of the same plan, n * 0.5 + 0.5 at every hit pixel (the environment at a miss)."""
    import _radiance_ref
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=1, seed=seed, debug_normal=True)
    rays = _radiance_ref.plan_rays(spt, scene, r, width, height, 0, 1, camera=camera).reshape(-1)
    film, _ = _util.oracle_render(scene, r, width, height, camera=camera, flags=_util.device_oracle_flags())
    return rays, film.reshape(-1, 3)

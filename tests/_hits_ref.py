"""spt_hits restated in float32 numpy (include/spt_abi.h, "all hits along caller rays"): exhaustive over instances x primitives, no
tree.  Every operation is one rounded f32 operation in the order of the device code: xf_point / xf_vector (device_math.h) into the
instance's object space, tri_test_edges on p0, p1 - p0, p2 - p0 and sphere_roots (trace.h).  The crossings of a ray are sorted by the
key (t, instance, prim, backfacing)."""
import numpy as np

f32 = np.float32
F32_MAX = np.finfo(f32).max
PRIM_SPHERE, PRIM_MESH = 0, 1
BACKFACING = 1


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _xf_vector(m, v):
    """(m[0:3] * v.x + m[3:6] * v.y) + m[6:9] * v.z per component; v is (n, 3)."""
    return np.stack([(m[k] * v[:, 0] + m[3 + k] * v[:, 1]) + m[6 + k] * v[:, 2] for k in range(3)], axis=1)


def to_object(inv, o, d):
    m = np.asarray(inv, dtype=f32)
    oo = _xf_vector(m, o) + m[9:12][None, :]
    return oo.astype(f32), _xf_vector(m, d).astype(f32)


def crossings(scene, rays, chunk=128):
    """Every crossing of every ray: a dict of flat arrays (ray, t, instance, prim, back, ptype, v, w), sorted by (ray, t, instance,
    prim, back)."""
    rays = np.asarray(rays).reshape(-1)
    inst = scene.array("instances")
    meshes = scene.array("meshes")
    tri = scene.array("tri_pos")
    sph = scene.array("spheres")
    out = {k: [] for k in ("ray", "t", "instance", "prim", "back", "ptype", "v", "w")}

    def emit(ray, t, ii, prim, back, ptype, v, w):
        out["ray"].append(ray.astype(np.int64)); out["t"].append(t.astype(f32))
        out["instance"].append(np.full(ray.shape, ii, dtype=np.int32)); out["prim"].append(prim.astype(np.int32))
        out["back"].append(back.astype(np.uint32)); out["ptype"].append(np.full(ray.shape, ptype, dtype=np.uint32))
        out["v"].append(v.astype(f32)); out["w"].append(w.astype(f32))

    with np.errstate(all="ignore"):
        for ii in range(len(inst)):
            ptype, pid = int(inst["prim_type"][ii]), int(inst["prim_id"][ii])
            assert ptype in (PRIM_SPHERE, PRIM_MESH), "spt_hits refuses patches"
            for r0 in range(0, len(rays), chunk):
                rs = rays[r0:r0 + chunk]
                o, d = to_object(inst["inv"][ii], rs["o"].astype(f32), rs["d"].astype(f32))
                t_min, t_max = rs["t_min"].astype(f32), rs["t_max"].astype(f32)
                if ptype == PRIM_SPHERE:
                    c, rad = sph["center"][pid].astype(f32), f32(sph["radius"][pid])
                    oc = [o[:, k] - c[k] for k in range(3)]
                    dd = [d[:, k] for k in range(3)]
                    a = _dot(dd, dd)
                    b = _dot(dd, oc)
                    cc = _dot(oc, oc) - rad * rad
                    delta = b * b - a * cc
                    sq = np.sqrt(delta)
                    mn, mx = (-b - sq) / a, (-b + sq) / a
                    ok = delta >= 0
                    for root, back in ((mn, 0), (mx, BACKFACING)):
                        at = np.nonzero(ok & (t_min < root) & (root < t_max))[0]
                        z = np.zeros(len(at), dtype=f32)
                        emit(at + r0, root[at], ii, np.full(len(at), pid), np.full(len(at), back), ptype, z, z)
                    continue
                first, count = int(meshes["tri_first"][pid]), int(meshes["tri_count"][pid])
                T = tri[first:first + count]
                p0 = [T["p0"][None, :, k].astype(f32) for k in range(3)]
                e1 = [(T["p1"][:, k].astype(f32) - T["p0"][:, k].astype(f32))[None, :] for k in range(3)]
                e2 = [(T["p2"][:, k].astype(f32) - T["p0"][:, k].astype(f32))[None, :] for k in range(3)]
                oo = [o[:, k][:, None] for k in range(3)]
                dd = [d[:, k][:, None] for k in range(3)]
                q = _cross(dd, e2)
                det = _dot(e1, q)
                inv = f32(1) / det
                s = [oo[k] - p0[k] for k in range(3)]
                v = _dot(s, q) * inv
                rr = _cross(s, e1)
                w = _dot(dd, rr) * inv
                u = f32(1) - v - w
                t = _dot(e2, rr) * inv
                ok = (det != 0) & (v >= 0) & (w >= 0) & (u >= 0) & (t > t_min[:, None]) & (t < t_max[:, None])
                ri, ti = np.nonzero(ok)
                emit(ri + r0, t[ri, ti], ii, ti + first, (det[ri, ti] < 0).astype(np.uint32), ptype, v[ri, ti], w[ri, ti])
    cr = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in out.items()}
    for k, ty in (("ray", np.int64), ("t", f32), ("instance", np.int32), ("prim", np.int32), ("back", np.uint32), ("ptype", np.uint32), ("v", f32), ("w", f32)):
        cr[k] = cr[k].astype(ty)
    order = np.lexsort((cr["back"], cr["prim"], cr["instance"], cr["t"], cr["ray"]))
    cr = {k: v[order] for k, v in cr.items()}
    cr["n_rays"] = len(rays)
    return cr


def rank(cr):
    """The place of each crossing in its ray's list."""
    n = cr["n_rays"]
    per_ray = np.bincount(cr["ray"], minlength=n)
    start = np.concatenate([[0], np.cumsum(per_ray)[:-1]])
    return np.arange(len(cr["ray"])) - start[cr["ray"]], per_ray


def records(spt, cr, max_hits, count_all=False):
    """(records (n, K) HIT_REC_DTYPE, counts (n,) HIT_COUNT_DTYPE) of a call with max_hits = K."""
    n, K = cr["n_rays"], max_hits
    j, per_ray = rank(cr)
    rec = np.zeros((n, K), dtype=spt.HIT_REC_DTYPE)
    rec["t"], rec["instance"], rec["prim"] = F32_MAX, -1, -1
    keep = j < K
    r, jj = cr["ray"][keep], j[keep]
    rec["t"][r, jj] = cr["t"][keep]
    rec["instance"][r, jj] = cr["instance"][keep]
    rec["prim"][r, jj] = cr["prim"][keep]
    rec["flags"][r, jj] = cr["back"][keep] | (cr["ptype"][keep] << 8)
    rec["v"][r, jj] = cr["v"][keep]
    rec["w"][r, jj] = cr["w"][keep]
    counts = np.zeros(n, dtype=spt.HIT_COUNT_DTYPE)
    which = np.ones(len(j), dtype=bool) if count_all else keep
    counts["total"] = np.bincount(cr["ray"][which], minlength=n)
    counts["back"] = np.bincount(cr["ray"][which], weights=cr["back"][which], minlength=n).astype(np.uint32)
    return rec, counts


def words(rec):
    """HIT_REC_DTYPE records as (..., 8) uint32."""
    rec = np.ascontiguousarray(rec)
    return rec.view(np.uint32).reshape(rec.shape + (8,))


def census(cr):
    """Shares of rays with 0, 1, 2, 3-4 and more than 4 crossings, with a sphere's exit root, and with a tie in t."""
    n = cr["n_rays"]
    _, per_ray = rank(cr)
    exit_root = np.zeros(n, dtype=bool)
    exit_root[cr["ray"][(cr["ptype"] == PRIM_SPHERE) & (cr["back"] == BACKFACING)]] = True
    same = (cr["ray"][1:] == cr["ray"][:-1]) & (cr["t"][1:] == cr["t"][:-1])
    tied = np.zeros(n, dtype=bool)
    tied[cr["ray"][1:][same]] = True
    return {"0": float((per_ray == 0).mean()), "1": float((per_ray == 1).mean()), "2": float((per_ray == 2).mean()),
            "3-4": float(((per_ray >= 3) & (per_ray <= 4)).mean()), ">4": float((per_ray > 4).mean()),
            "exit": float(exit_root.mean()), "tied": float(tied.mean())}


# ---- the batches of the tests

def scene_box(scene):
    inst = scene.array("instances")
    return inst["bmin"].min(axis=0).astype(np.float64), inst["bmax"].max(axis=0).astype(np.float64)


def scene_extent(scene):
    lo, hi = scene_box(scene)
    return f32(np.linalg.norm(hi - lo))


def through_rays(spt, scene, n, seed):
    """Segments through the whole bounds from outside: from a point on a sphere around the scene's box through a point inside the
    box of one of its instances, each instance as often as any other (a floor is large and thin: aiming at the scene's box as a
    whole mostly finds the floor alone)."""
    lo, hi = scene_box(scene)
    inst = scene.array("instances")
    rng = np.random.default_rng(seed)
    c, r = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    o = rng.normal(size=(n, 3))
    o = c + o / np.linalg.norm(o, axis=1, keepdims=True) * r * 1.5
    which = rng.integers(0, len(inst), n)
    ilo, ihi = inst["bmin"][which].astype(np.float64), inst["bmax"][which].astype(np.float64)
    tgt = (ilo + ihi) / 2 + rng.uniform(-0.4, 0.4, size=(n, 3)) * (ihi - ilo)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(n, dtype=spt.RAY_DTYPE)
    rays["o"], rays["d"] = o.astype(f32), d.astype(f32)
    rays["t_min"], rays["t_max"] = 1e-4, F32_MAX
    return rays


def edge_rays(spt, scene, n, seed, max_tris=64):
    """Rays through points on the edges that two triangles of a small mesh share (the quarter points and the middle), from random
    directions: a good share of them passes both triangle tests with the same t, the tie that the key's prim decides."""
    inst, meshes, tri = scene.array("instances"), scene.array("meshes"), scene.array("tri_pos")
    rng = np.random.default_rng(seed)
    targets = []
    for ii in range(len(inst)):
        if inst["prim_type"][ii] != PRIM_MESH:
            continue
        m = meshes[inst["prim_id"][ii]]
        if m["tri_count"] > max_tris:
            continue
        fwd = inst["fwd"][ii].astype(np.float64)
        M, tr = fwd[:9].reshape(3, 3).T, fwd[9:12]
        edges = {}
        for k, t in enumerate(tri[m["tri_first"]:m["tri_first"] + m["tri_count"]]):
            P = [tuple(t["p0"]), tuple(t["p1"]), tuple(t["p2"])]
            for a, b in ((0, 1), (1, 2), (2, 0)):
                edges.setdefault(tuple(sorted((P[a], P[b]))), []).append(k)
        for (a, b), ks in edges.items():
            if len(ks) == 2:
                a, b = M @ np.array(a, dtype=np.float64) + tr, M @ np.array(b, dtype=np.float64) + tr
                targets += [a + (b - a) * f for f in (0.25, 0.5, 0.75)]
    pick = np.array(targets)[rng.integers(0, len(targets), n)]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(n, dtype=spt.RAY_DTYPE)
    rays["o"], rays["d"] = (pick - d * 4).astype(f32), d.astype(f32)
    rays["t_min"], rays["t_max"] = 1e-4, F32_MAX
    return rays


def window(rays, cr, extent):
    """The same lines with the origin moved to extent / 32 before the first crossing, t_min = 0 and t_max = extent / 16: the end of
    the segment falls between the crossings of a ray (unchanged rays, shortened, where there is no crossing)."""
    out = rays.copy()
    j, _ = rank(cr)
    first = j == 0
    r, t = cr["ray"][first], cr["t"][first]
    out["o"][r] = (rays["o"][r].astype(np.float64) + rays["d"][r].astype(np.float64) * (t - f32(extent) / f32(32))[:, None]).astype(f32)
    out["t_min"] = 0
    out["t_max"] = f32(extent) / f32(16)
    return out


def batches(spt, scene, camera, variants=True):
    """name -> rays: the camera grid, _util.random_rays, segments through the bounds and rays through shared edges; with `variants`
    also each of them cut at t_max = extent / 16 (":short"), moved to a window of that length around the first crossing (":window")
    and with t_min moved past the first crossing (":past")."""
    import _util
    base = {"grid": grid_rays(spt, scene, camera), "random": _util.random_rays(scene, 1200, 3, spread=2.0), "through": through_rays(spt, scene, 1200, 5),
            "edges": edge_rays(spt, scene, 1024, 7)}
    if not variants:
        return base
    extent = scene_extent(scene)
    out = {}
    for name, rays in base.items():
        cr = crossings(scene, rays)
        out[name] = rays
        out[name + ":short"] = shortened(rays, extent)
        out[name + ":window"] = window(rays, cr, extent)
        out[name + ":past"] = past_first(rays, cr)
    return out


def grid_rays(spt, scene, camera, width=48, height=36, seed=11):
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=1, seed=seed)
    pr = spt.camera_rays(spt.CameraModel.perspective(scene.get_camera(camera)), r, width, height).reshape(-1)
    seg = np.zeros(pr.shape[0], dtype=spt.RAY_DTYPE)
    seg["o"], seg["t_min"], seg["d"], seg["t_max"] = pr["o"], pr["t_min"], pr["d"], F32_MAX
    return seg


def shortened(rays, extent):
    out = rays.copy()
    out["t_max"] = f32(extent) / f32(16)
    return out


def past_first(rays, cr):
    """The same rays with t_min moved just past their first crossing, to the next float behind its t (unchanged where there is
    none)."""
    out = rays.copy()
    j, _ = rank(cr)
    first = j == 0
    out["t_min"][cr["ray"][first]] = np.nextafter(cr["t"][first], f32(np.inf))
    return out


def sphere_root_at_t_min(scene, rays):
    """How many rays have a sphere root exactly equal to their t_min: the one case in which record 0 and trace_closest differ."""
    rays = np.asarray(rays).reshape(-1)
    open_rays = rays.copy()
    open_rays["t_min"], open_rays["t_max"] = -F32_MAX, F32_MAX
    cr = crossings(scene, open_rays)
    on_sphere = cr["ptype"] == PRIM_SPHERE
    return int((cr["t"][on_sphere] == rays["t_min"][cr["ray"][on_sphere]]).sum())

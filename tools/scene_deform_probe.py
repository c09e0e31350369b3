#!/usr/bin/env python3
"""Where a refitted scene and a freshly created one differ, on one GPU -> profiles/scene_deform_mismatch.json.

The grid of tools/scene_deform_cost.py (>= 1 M triangles, large-scene form) under that tool's medium deformation, a smooth
displacement of 25 % of the extent: one device scene created on the file's positions and deformed (spt_scene_deform: refitted tree),
one created from the deformed host scene (rebuilt tree).  Both hold the same triangles, so they may differ only in the triangle
test's own false positives: a ray grazing a triangle's plane can be accepted at a point outside the triangle's padded box, and
whether a walk reaches that triangle depends on the boxes above it (scene_build.cpp, "device-side BLAS").

  1. films: 1024 x 1024 @ 16 spp of both, the pixels whose words differ; for the first four of them the exhaustive oracle's
     pixel (its image row rendered with every triangle tested) says which scene has the words of the triangle set itself.
  2. closest hits of --rays rays (camera-like rays from the eye, and rays between random points around the mesh, which graze it the
     way secondary rays do): every ray whose hit words differ is classified.  The EXTRA hit is the nearer one (the other scene
     culled it, or found the same t on another triangle).  In f64, in the mesh's object space: is the hit point outside the padded
     box of the triangle it names (the documented exception), and does the exhaustive oracle - every triangle tested, no tree -
     return the extra hit as well (then the triangle test accepts it, and the scene without it lost it to a box, not to a bug)?

  python tools/scene_deform_probe.py [--grid 710] [--rays 16000000]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
f32 = np.float32


def make_rays(spt, rng, n, kind):
    rays = np.zeros(n, dtype=spt.RAY_DTYPE)
    if kind == "camera":
        o = np.tile(np.array([[0.0, 2.2, 4.5]]), (n, 1))
        tgt = rng.uniform(-1, 1, size=(n, 3)) * np.array([2.6, 0.9, 2.6])
    else:
        o = rng.uniform(-1, 1, size=(n, 3)) * np.array([2.6, 1.2, 2.6])
        tgt = rng.uniform(-1, 1, size=(n, 3)) * np.array([2.6, 1.2, 2.6])
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["o"], rays["d"] = o.astype(f32), d.astype(f32)
    rays["t_min"], rays["t_max"] = 1e-4, f32(3.4028234663852886e38)
    return rays


def pad(lo, hi):
    """box_pad of the builder, per axis, in f32."""
    lo, hi = lo.astype(f32), hi.astype(f32)
    return (hi - lo) * f32(1.52587890625e-5) + np.maximum(np.abs(lo), np.abs(hi)) * f32(9.5367431640625e-7) + f32(1e-30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=710)
    ap.add_argument("--rays", type=int, default=16000000)
    ap.add_argument("--chunk", type=int, default=4000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_deform_mismatch.json"))
    args = ap.parse_args()
    import bench
    import scene_deform_cost as cost
    import _util
    spt = bench.load_pkg()
    if spt.device_count() < 1:
        sys.exit("scene_deform_probe: no GPU")
    os.environ.pop("SPT_NO_LDS_GEO", None)
    path = cost.write_grid_scene(os.path.join(ROOT, "scenes_amd", "generated"), args.grid)
    refit, fresh = spt.load_scene(path), spt.load_scene(path)
    rest = refit.mesh_positions("grid")
    extent = float((rest.max(axis=0) - rest.min(axis=0)).max())
    moved = (rest + 0.25 * extent * np.sin(3.0 * rest[:, [2, 0, 1]] + 1.0)).astype(f32)      # the cost tool's medium case
    ds_refit = refit.device_scene(0)           # the tree of the file's positions
    refit.set_mesh_positions("grid", moved)
    ds_refit.update()                          # refitted
    fresh.set_mesh_positions("grid", moved)
    ds_fresh = fresh.device_scene(0)           # rebuilt
    assert refit.array("tri_pos").tobytes() == fresh.array("tri_pos").tobytes()
    r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
    r.spp = 16
    cfg = spt.OutputConfig(1024, 1024)
    film_a, film_b = r.render_shard(refit, cfg).copy(), r.render_shard(fresh, cfg).copy()
    pixels = int((film_a.view(np.uint32) != film_b.view(np.uint32)).any(axis=2).sum())
    out = {"what": "tools/scene_deform_probe.py on one MI355X: a %d-triangle grid deformed by 25 %% of its extent, the refitted scene against a freshly created one"
                   % refit.desc.n_tris,
           "film": {"width": 1024, "height": 1024, "spp": 16, "pixels_that_differ": pixels},
           "rays": {}}
    # every pixel that differs (the first four): its image row rendered by the exhaustive oracle - every triangle tested, no tree -
    # says which of the two scenes has the words of the triangle set itself
    flags = _util.ORACLE_EXHAUSTIVE
    rows = []
    for y, x in np.argwhere((film_a.view(np.uint32) != film_b.view(np.uint32)).any(axis=2))[:4]:
        want = _util.oracle_render(fresh, r, 1024, 1024, flags=flags, shard_index=int(y), shard_count=1024, strip_rows=1)[0][0, int(x)]
        rows.append({"pixel": [int(x), int(y)], "refitted": [float(v) for v in film_a[y, x]], "fresh": [float(v) for v in film_b[y, x]],
                     "exhaustive_oracle": [float(v) for v in want],
                     "refitted_is_the_oracles": bool(np.array_equal(want.view(np.uint32), film_a[y, x].view(np.uint32))),
                     "fresh_is_the_oracles": bool(np.array_equal(want.view(np.uint32), film_b[y, x].view(np.uint32)))})
        print(rows[-1], file=sys.stderr, flush=True)
    out["film"]["pixels"] = rows
    tri = fresh.array("tri_pos")
    inst = fresh.array("instances")[0]
    inv = inst["inv"].astype(np.float64)
    flags = _util.ORACLE_EXHAUSTIVE
    rng = np.random.default_rng(9)
    for kind in ("camera", "between_random_points"):
        total = differ = outside = in_oracle = same_t = 0
        examples = []
        for first in range(0, args.rays // 2, args.chunk):
            n = min(args.chunk, args.rays // 2 - first)
            rays = make_rays(spt, rng, n, kind)
            ha, hb = ds_refit.trace_closest(rays), ds_fresh.trace_closest(rays)
            total += n
            bad = np.flatnonzero((ha.view(np.uint32).reshape(n, -1) != hb.view(np.uint32).reshape(n, -1)).any(axis=1))
            differ += len(bad)
            if not len(bad):
                continue
            want = _util.oracle_trace_closest(fresh, rays[bad], flags)
            for k, i in enumerate(bad):
                a, b = ha[i], hb[i]
                ta = float(a["t"]) if a["instance"] >= 0 else np.inf
                tb = float(b["t"]) if b["instance"] >= 0 else np.inf
                same_t += int(ta == tb)
                extra = a if ta <= tb else b
                o, d = rays["o"][i].astype(np.float64), rays["d"][i].astype(np.float64)
                pw = o + float(extra["t"]) * d
                po = inv[0:3] * pw[0] + inv[3:6] * pw[1] + inv[6:9] * pw[2] + inv[9:12]
                t = tri[int(extra["prim"])]
                corners = np.stack([t["p0"], t["p1"], t["p2"]]).astype(np.float64)
                lo, hi = corners.min(axis=0), corners.max(axis=0)
                p = pad(lo, hi).astype(np.float64)
                is_outside = bool(((po < lo - p) | (po > hi + p)).any())
                outside += int(is_outside)
                found = bool(want[k].tobytes() == extra.tobytes())
                in_oracle += int(found)
                if len(examples) < 4:
                    examples.append({"t_refitted": None if np.isinf(ta) else ta, "t_fresh": None if np.isinf(tb) else tb,
                                     "extra_hit_in": "refitted" if ta <= tb else "fresh", "triangle": int(extra["prim"]),
                                     "beyond_the_padded_box_by": float(np.maximum(lo - p - po, po - hi - p).max()), "exhaustive_oracle_has_it": found})
        out["rays"][kind] = {"rays": total, "hits_that_differ": differ, "extra_hit_outside_its_triangles_padded_box": outside,
                             "extra_hit_is_the_exhaustive_oracles": in_oracle, "same_t_on_both": same_t, "examples": examples}
        print(kind, out["rays"][kind], file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))
    refit.close()
    fresh.close()


if __name__ == "__main__":
    main()
